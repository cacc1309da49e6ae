"""librbergomi's Philox mode -- the one that ships -- against the host replay of its draws
(tests/_rbergomi_replay.py, written from include/rbergomi.h) pushed through the oracle.

Stage by stage, as test_generator_reference_draws_match_golden: each stage's oracle is fed
the device's output of the stage before, so tolerances do not compound and K = rint(S)
cannot flip on a tie.  tests/test_rbergomi_replay_cpu.py proves for every mark case here
that a wrong draw layout moves a compared mark by more than 100 times its tolerance."""
import numpy as np
import pytest

from oracle import rbergomi_oracle as orc

import _rbergomi_replay as rep
import _rbergomi_replay_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_RTOL = 1e-12            # tests/test_rbergomi_gpu.py: same draws, different libm, 252 chained steps

OFFSETS = (0, 2 ** 32 - 2)
SEEDS = (42, 2 ** 32 + 7, 2 ** 64 - 1)
BASES = ((496.48, 0.029, 0.1, 1.0, -0.7),
         (100.0, 0.04, 0.49, 1.9, -0.99),      # H and rho on their upper / lower clip limits
         (100.0, 0.04, 0.01, 0.6, -0.01))      # and on the other two


def _rb():
    from cantorrl_amd import rbergomi
    return rbergomi


def _ref_params(base, seed, off, n):
    return np.stack(orc.perturb_params(base, [s * u for s, u in zip(orc.PERTURB_STD, rep.unit_normals(seed, off, n))]))


# Parameters: out = base (1 + std z) (clipped).  he::box_muller is within 8 ulp of the radius of
# the libm formula (test_box_muller_within_ulps_of_libm): |dz| <= 8 * 2^-52 * 8.6 = 1.5e-14, times
# perturb_std <= 0.2 is 3e-15 absolute on a factor 1 + std z that is >= 0.22 for |z| <= 3.9 (the
# largest |z| of the draws below is 3.86), so 1.4e-14 relative: rtol 1e-13 is a ceiling.
PARAMS_RTOL = 1e-13


@pytest.mark.parametrize("n", [1, 257])
def test_params_philox_against_replay(n):
    rb = _rb()
    for off in OFFSETS:
        for seed in SEEDS:
            for base in BASES:
                cfg = rb.make_config(n, seed=seed, path_offset=off)
                got = rb.sample_params(cfg, base, DEV).cpu().numpy()
                ref = _ref_params(base, seed, off, n)
                np.testing.assert_allclose(got, ref, rtol=PARAMS_RTOL, atol=0, err_msg=str((n, off, seed, base)))
                if n > 1:      # both clip branches taken, and exactly
                    for row, lim in ((2, orc.CLIP_H), (4, orc.CLIP_RHO)):
                        on = np.isin(ref[row], lim)
                        assert 0 < on.sum() < n or base is BASES[0]
                        np.testing.assert_array_equal(got[row][on], ref[row][on])


@pytest.mark.parametrize("n_steps", [1, 5, 63, 64, 252])
def test_main_paths_philox_against_replay(n_steps):
    """M = 2, 8, 64 (T = M - 1), 128, 256: block j for every j < M, the padded points of the
    circular convolution included."""
    rb = _rb()
    M = orc.next_pow2(n_steps + 1)
    for off in OFFSETS:
        for seed in SEEDS:
            cfg = rb.make_config(3, n_steps=n_steps, seed=seed, path_offset=off)
            params = rb.sample_params(cfg, BASES[(OFFSETS.index(off) + SEEDS.index(seed)) % 3], DEV)
            paths, vol = rb.simulate_paths(cfg, params, DEV)
            ref_paths, ref_vol = orc.simulate_paths(*params.cpu().numpy(), rep.w_to_z(rep.main_W(seed, off, 3, M)),
                                                    cases.R, cases.DT, n_steps)
            msg = str((n_steps, off, seed))
            np.testing.assert_allclose(vol.cpu().numpy(), ref_vol, rtol=PATH_RTOL, atol=0, err_msg=msg)
            np.testing.assert_allclose(paths.cpu().numpy(), ref_paths, rtol=PATH_RTOL, atol=0, err_msg=msg)


def _price(case, kind, normals):
    return _rb().price_rbergomi_option(case.S0, case.K, case.T, cases.R, case.xi, case.H, case.eta, case.rho, kind,
                                       case.n_mc, cases.DT, device=DEV, seed=cases.SEED, index_offset=cases.OFF,
                                       normals=normals).cpu().numpy()


def _check_list_case(case, normals):
    for kind in cases.KINDS:
        got = _price(case, kind, normals)
        ref = case.oracle(kind, case.W(kind, normals))
        rel = np.abs(got - ref)[:case.rows] / case.S0[:case.rows]
        print(f"{case.name} {normals} {kind}: max |device - replay| / S0 = {rel.max():.3e}")
        case.check(kind, normals, got, ref)


@pytest.mark.parametrize("normals", ["f64", "f32"])
@pytest.mark.parametrize("n", cases.MC_STEPS)
def test_list_marks_philox_against_replay(n, normals):
    """Every mc_kernel grid: M_opt 2, 4, 8, 16, 32 (both guard variants), 64; n = M - 1,
    n < kXc, n = kXc, odd n; one thread, a partial wave, two paths on thread 0, an uneven tail."""
    for n_mc in cases.MC_PATHS:
        _check_list_case(cases.list_case(n, n_mc), normals)


@pytest.mark.parametrize("normals", ["f64", "f32"])
def test_list_marks_edge_inputs_philox_against_replay(normals):
    _check_list_case(cases.list_case(3, 3, edge=True), normals)


@pytest.mark.parametrize("which,normals", [("small", "f64"), ("small", "f32"), ("default", "f64")])
def test_atm_marks_philox_against_replay(which, normals):
    """rb_generate: day d, type t of path p draws under gid = path_offset + p, sub = 2 d + t;
    the inputs of every option are the device's own params, paths and volatilities."""
    rb = _rb()
    kw = cases.ATM_SMALL if which == "small" else cases.ATM_DEFAULT
    res = rb.generate_paths_and_options(cases.history(), cases.ATM_PATHS, seed=cases.SEED, path_offset=cases.OFF,
                                        normals=normals, device=DEV, **kw)
    T = kw["n_steps"]
    params, paths, vol = (res[k].cpu().numpy() for k in ("params", "paths", "volatilities"))
    # the first two stages of the one-call entry, as in the staged tests above
    np.testing.assert_allclose(params, _ref_params(res["base_params"], cases.SEED, cases.OFF, cases.ATM_PATHS),
                               rtol=PARAMS_RTOL, atol=0)
    Zm = rep.w_to_z(rep.main_W(cases.SEED, cases.OFF, cases.ATM_PATHS, orc.next_pow2(T + 1)))
    ref_paths, ref_vol = orc.simulate_paths(*params, Zm, cases.R, cases.DT, T)
    np.testing.assert_allclose(vol, ref_vol, rtol=PATH_RTOL, atol=0)
    np.testing.assert_allclose(paths, ref_paths, rtol=PATH_RTOL, atol=0)
    case = cases.atm_case(which, params, paths, vol, **kw)
    for kind, key in (("call", "call_prices_atm"), ("put", "put_prices_atm")):
        got = res[key].cpu().numpy().reshape(-1)               # [p, d] row-major = option p T + d
        ref = case.oracle(kind, case.W(kind, normals))
        print(f"atm {which} {normals} {kind}: max |device - replay| / S0 = {(np.abs(got - ref) / case.S0).max():.3e}")
        case.check(kind, normals, got, ref)
