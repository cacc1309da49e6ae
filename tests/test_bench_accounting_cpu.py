"""bench.py's algorithmic-byte accounting, host logic only.

The roofline `achieved` figure is bytes per launch / measured launch time, so the byte
model has to follow the tile layout the library actually picks (hedge_env.hip
kGreeksInStepMinEnvs, Params::tile_greeks) and whether the market rides in the step
grid (step_market_kernel; not with a book).
"""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default_and_steps_are_taken_as_given(bench):
    a = bench.parse(["--gpus", "1", "--steps", "10", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (10, 3, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (bench.MIN_TIMED_STEPS, 256, True, "out")
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_threshold_matches_library(bench):
    src = open(os.path.join(REPO, "cantorrl_amd", "csrc", "hedge_env.hip")).read()
    assert f"constexpr int64_t kGreeksInStepMinEnvs = {bench.GREEKS_IN_STEP_MIN_ENVS};" in src


def test_tile_layout(bench, monkeypatch):
    monkeypatch.delenv("HE_GREEKS_IN_STEP_MIN_ENVS", raising=False)
    assert bench.tile_layout("gbm", 65536) == "gbm"
    assert bench.tile_layout("gbm", 262144) == "gbm_step"
    assert bench.tile_layout("heston", 1 << 20) == "heston"
    monkeypatch.setenv("HE_GREEKS_IN_STEP_MIN_ENVS", "0")
    assert bench.tile_layout("gbm", 1) == "gbm_step"


def test_per_step_bytes_add_up(bench):
    # rollout step: action 8 + post tile + obs 52 + reward 4 + terminated 1
    for lay, tile in (("gbm", 24), ("gbm_step", 12), ("heston", 32)):
        assert bench.ROLLOUT_BYTES_PER_ENV[lay] == 8 + tile + 52 + 4 + 1
        assert bench.MARKET_BYTES_PER_ENV[lay] == tile
    # he_step: state 16 + action 8 + tile slots read; state 16 + obs 52 + reward 4 + flags 2 written
    assert bench.STEP_BYTES_PER_ENV["gbm"] == 16 + 8 + 36 + 74
    assert bench.STEP_BYTES_PER_ENV["gbm_step"] == 16 + 8 + 24 + 74
    assert bench.STEP_BYTES_PER_ENV["heston"] == 16 + 8 + 48 + 74


def test_achieved_is_priced_on_survey_bytes(bench, monkeypatch):
    """roofline.achieved uses SURVEY 8(d)'s algorithmic bytes (rollout 66 B per env-step
    + 120 B per env per launch; he_step 186 B), whatever the kernel moves besides."""
    n, rk = 65536, 256
    r = bench.roofline("rollout", n, 0.25, rk, False, "gbm", lds=True)
    assert r["bytes_per_launch"] == n * (rk * 66 + 120)
    assert r["kernel"].startswith("lds_rollout_kernel")
    assert r["kernel_bytes_per_launch"] == n * (rk * 65 + 80) and r["overhead_bytes_per_launch"] == 0
    assert abs(r["achieved"] - n * (rk * 66 + 120) / 0.25e-3 / 1e9) < 0.1
    assert abs(r["frac"] - r["achieved"] / bench.HBM_PEAK_GBS) < 1e-4
    s = bench.roofline("graph", n, 0.005, 1, False, "gbm")
    assert s["bytes_per_launch"] == n * 186


def test_tile_path_reports_the_market_tile_as_overhead(bench, monkeypatch):
    n, rk = 65536, 64
    monkeypatch.setenv("HE_FUSED_MARKET", "1")
    r = bench.roofline("rollout", n, 0.1, rk, False, "gbm")
    step = n * (rk * 89 + 44)
    market = n * (rk * 24 + bench.MARKET_STATE_BYTES)
    # round 1's figure (profiles/r01s21_bench.jsonl) = the 8(d) I/O + the tile round trip
    assert r["kernel_bytes_per_launch"] + r["overhead_bytes_per_launch"] == step + market == 481558528
    assert r["bytes_per_launch"] == n * (rk * 66 + 120)
    assert r["kernel"].startswith("step_market_kernel")
    # a book keeps the market on the side stream: the step kernel's tile reads only
    rb = bench.roofline("rollout", n, 0.1, rk, True, "gbm")
    assert rb["kernel_bytes_per_launch"] + rb["overhead_bytes_per_launch"] == n * (rk * (89 + 8) + 44)
    assert rb["kernel"].startswith("step_kernel")
    monkeypatch.setenv("HE_FUSED_MARKET", "0")
    r0 = bench.roofline("rollout", n, 0.1, rk, False, "gbm")
    assert r0["kernel_bytes_per_launch"] + r0["overhead_bytes_per_launch"] == step == 376176640
    assert abs(r0["frac"] - r0["achieved"] / bench.HBM_PEAK_GBS) < 1e-4


def test_lds_path_selection(bench, monkeypatch):
    monkeypatch.delenv("HE_LDS_ROLLOUT", raising=False)
    assert bench.lds_rollout(bench.CONFIGS[2]) and bench.lds_rollout(bench.CONFIGS[3])
    assert bench.lds_rollout(bench.CONFIGS[4]) and bench.lds_rollout(bench.CONFIGS[5])  # GBM + book; Heston + book
    # the LDS kernel's own bytes: + 16 per env for the book's running max, + 16 for Heston's v
    n, rk = 131072, 256
    r5 = bench.roofline("rollout", n, 1.0, rk, True, "heston", lds=True)
    assert r5["kernel_bytes_per_launch"] == n * (rk * 65 + 80 + 16 + 16)
    assert r5["overhead_bytes_per_launch"] == 0 and r5["kernel"].startswith("lds_rollout_kernel")
    monkeypatch.setenv("HE_LDS_ROLLOUT", "0")
    assert not bench.lds_rollout(bench.CONFIGS[2])


def _roof(bench):
    return bench.roofline("rollout", 65536, 0.3, 256, False, "gbm", lds=True)


@pytest.mark.parametrize("config", [2, 3, 4, 5, 6])
def test_bound_is_fixed_per_config(bench, config):
    """configs 4 / 5 (a book, Heston) are VALU-bound and say so whether or
    not the PMC passes ran; the others are HBM-bound.  Without counters a VALU line keeps the
    figure null with a note, never an HBM fraction in the headline fields."""
    cfg = bench.CONFIGS[config]
    want = "valu" if config in (4, 5) else "hbm"
    assert bench.config_bound(cfg) == want
    r = bench.finish_roofline(_roof(bench), cfg, (None, "skipped"), (None, "skipped"), 0.3)
    assert r["bound"] == want
    if want == "valu":
        assert r["frac"] is None and r["achieved"] is None and "valu_note" in r
        assert r["hbm"]["frac"] == _roof(bench)["frac"]
    else:
        assert r["frac"] == _roof(bench)["frac"] and r["unit"] == "GB/s"
    # with the VALU pass: the issue rate is the headline figure
    valu = {"lds_rollout_kernel": dict(valu_insts=1e9, f64_share=0.5, issue_per_simd_cycle=0.2,
                                       issue_bound_per_simd_cycle=0.333, valu_issue_frac=0.6, f64_flop=1e12,
                                       cycles_profiled=1e6)}
    r = bench.finish_roofline(_roof(bench), cfg, (valu, None), (1.1e9, {"FETCH_SIZE": 1.0, "WRITE_SIZE": 1.0}), 0.3)
    assert r["bound"] == want and r["traffic"] == int(1.1e9)
    if want == "valu":
        assert r["frac"] == 0.6 and r["unit"].startswith("VALU")
    else:
        assert r["valu"]["valu_issue_frac"] == 0.6 and r["unit"] == "GB/s"


def test_host_cores_follow_the_grant(bench, monkeypatch):
    """every core of the affinity mask, capped by the per-GPU grant the
    pool states (OMP_NUM_THREADS), and the line says which."""
    avail = len(os.sched_getaffinity(0))
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert bench.host_cores()[:2] == (avail, avail)
    if avail > 1:
        monkeypatch.setenv("OMP_NUM_THREADS", "1")
        c, a, why = bench.host_cores()
        assert (c, a) == (1, avail) and "OMP_NUM_THREADS=1" in why
    monkeypatch.setenv("OMP_NUM_THREADS", str(avail + 5))
    assert bench.host_cores()[0] == avail


def test_step_api_frac_is_on_the_kernel_bytes(bench, monkeypatch):
    """the step_api line's `frac` is priced on the bytes step1_kernel itself
    moves (134 B per env at 65,536 envs, where it reads the greeks from the market tile; 122 B
    from 262,144 envs, where it evaluates them), with SURVEY 8(d)'s 186 B beside it as
    `frac_survey_8d`; `traffic` is the kernel's own PMC bytes per launch."""
    monkeypatch.delenv("HE_GREEKS_IN_STEP_MIN_ENVS", raising=False)
    for n, per_env in ((65536, 134), (1 << 20, 122)):
        lay = bench.tile_layout("gbm", n)
        us = 5.0 if n == 65536 else 25.0
        rf = bench.roofline("graph", n, us * 1e-3, 1, False, lay)
        line = bench.step_api_line(n, 2560, 0.0125, rf, (n * per_env * 1.02, {"FETCH_SIZE": 1.0, "WRITE_SIZE": 2.0}),
                                   lay)
        assert line["kernel_bytes_per_launch"] == n * per_env and line["kernel_bytes_per_env"] == per_env
        assert line["bytes_per_launch"] == n * 186
        assert abs(line["achieved_gbs"] - n * per_env / (us * 1e-6) / 1e9) < 0.1
        assert abs(line["frac"] - line["achieved_gbs"] / bench.HBM_PEAK_GBS) < 1e-4
        assert abs(line["frac_survey_8d"] - n * 186 / (us * 1e-6) / 1e9 / bench.HBM_PEAK_GBS) < 1e-4
        assert line["frac"] < line["frac_survey_8d"]
        assert line["traffic"] == int(n * per_env * 1.02) and line["traffic_over_kernel_bytes"] == 1.02
    skipped = bench.step_api_line(64, 64, 1e-3, bench.roofline("graph", 64, 1e-3, 1, False, "gbm"),
                                  (None, "skipped"), "gbm")
    assert skipped["traffic"] is None and skipped["traffic_note"] == "skipped"


def test_rbergomi_roofline_from_the_valu_pass(bench):
    """VERDICT r4 missing 3: the rBergomi line carries a VALU roofline computed from the
    counters of mc_kernel (issue per SIMD-cycle against the bound of its f64 mix, f64 TFLOP/s)."""
    res = {"mc_kernel": {"SQ_INSTS_VALU": 2.0e10, "SQ_INSTS_VALU_FMA_F64": 6.0e9, "SQ_INSTS_VALU_ADD_F64": 1.0e9,
                         "SQ_INSTS_VALU_MUL_F64": 1.0e9, "SQ_INSTS_VALU_TRANS_F64": 1.0e8, "GRBM_GUI_ACTIVE": 8 * 8.0e7}}
    v = bench.valu_summary(res)["mc_kernel"]
    share = 8.1e9 / 2.0e10
    assert abs(v["f64_share"] - share) < 1e-4
    assert abs(v["issue_per_simd_cycle"] - 2.0e10 / (8.0e7 * 1024)) < 1e-4
    bound = 1 / (2 * (1 - share) + 4 * share)
    r = bench.rb_roofline((v, None), (3.0e6, {"FETCH_SIZE": 1000.0, "WRITE_SIZE": 1000.0}), 1000.0, 2048 * 252 * 2)
    assert r["bound"] == "valu" and abs(r["peak"] - bound) < 1e-4
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3
    assert abs(r["f64_tflops"] - 64 * (2 * 6.0e9 + 2.0e9) / 1.0 / 1e12) < 1e-3
    assert r["traffic"] == 3000000
    r0 = bench.rb_roofline((None, "rocprofv3 not found"), (None, "rocprofv3 not found"), 1000.0, 10)
    assert r0["frac"] is None and r0["valu_note"] == "rocprofv3 not found" and r0["traffic"] is None


def test_traffic_bytes_from_sized_read_requests(bench):
    """bench.traffic_bytes: reads by request size (32 / 64 / 128 B; unsized remainder at 64 B) +
    WRITE_SIZE KiB -- the calibrated reading (profiles/r05s10_traffic_calib.log: a 1 GiB read is
    8,388,608 requests of 128 B)."""
    c = dict(TCC_EA0_RDREQ_sum=8388608.0, TCC_EA0_RDREQ_32B_sum=0.0, TCC_EA0_RDREQ_64B_sum=0.0,
             TCC_EA0_RDREQ_128B_sum=8388608.0, WRITE_SIZE=0.0)
    assert bench.traffic_bytes(c) == 2.0 ** 30
    c = dict(TCC_EA0_RDREQ_sum=10.0, TCC_EA0_RDREQ_32B_sum=1.0, TCC_EA0_RDREQ_64B_sum=2.0,
             TCC_EA0_RDREQ_128B_sum=3.0, WRITE_SIZE=2.0)
    assert bench.traffic_bytes(c) == 32 + 64 * (2 + 4) + 128 * 3 + 2048
