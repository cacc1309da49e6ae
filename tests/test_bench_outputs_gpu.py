"""bench.py's plain run on the GPU at a small size: --steps is the number of timed steps
exactly (a count that is no multiple of the launch included), --dump-outputs writes what the
last timed step returned as f32 .npy files, the same in every run, and a plain run and a
--full run of the same arguments compute the same arrays.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1280   # 5 workgroups of 256 envs


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_outputs_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.MIN_WARMUP_SECONDS = 0.02   # the clocks do not matter here
    return mod


def run(bench, capsys, out, *extra):
    capsys.readouterr()
    bench.main(["--gpus", "1", "--envs", str(N), "--dump-outputs", str(out), *extra])
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    return line, {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


@pytest.mark.parametrize("mode,steps,warmup,names", [
    ("rollout", 300, 10, {"obs": (N, 13), "reward": (N,), "terminated": (N,), "launch_obs": (44, 256, 13),
                          "launch_reward": (44, 256), "launch_terminated": (44, 256)}),
    ("rollout", 512, 0, {"obs": (N, 13), "reward": (N,), "terminated": (N,), "launch_obs": (256, 256, 13),
                         "launch_reward": (256, 256), "launch_terminated": (256, 256)}),
    ("graph", 70, 64, {"obs": (N, 13), "reward": (N,), "terminated": (N,), "truncated": (N,)}),
])
def test_plain_run_times_the_steps_asked_for_and_repeats_its_outputs(bench, capsys, tmp_path, mode, steps, warmup,
                                                                     names):
    args = ("--mode", mode, "--steps", str(steps), "--warmup", str(warmup))
    line, a = run(bench, capsys, tmp_path / "a", *args)
    assert line["steps"] == steps and line["requested_steps"] == steps
    assert line["ms_per_step"] > 0 and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    # ms_per_step is printed to 1e-6 ms, a step here takes over 2e-4 ms: 0.5e-6 / 2e-4 = 2.5e-3
    assert line["ms_per_step"] > 2e-4
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3), rel=2.5e-3)
    # nothing but the headline's own measurement
    for leg in ("step_api", "sb3_api", "policy_api", "shard_check", "cpu_baseline"):
        assert line[leg] is None
    assert {k: v.shape for k, v in a.items()} == names
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.isfinite(a["obs"]).all() and np.abs(a["obs"]).max() > 0
    _, b = run(bench, capsys, tmp_path / "b", *args)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    if mode == "rollout":
        # the last step's arrays are the last row of the launch's: the sampled envs agree
        rows = np.sort(np.random.default_rng(42).choice(N, 256, replace=False))
        assert np.array_equal(a["launch_obs"][-1], a["obs"][rows])
        assert np.array_equal(a["launch_reward"][-1], a["reward"][rows])


def test_full_run_computes_what_the_plain_run_does(bench, capsys, tmp_path):
    """--full adds legs around the timed steps (here: the kernel probe, the policy leg and the
    shard check; no rocprofv3 children, no CPU baseline) and leaves what they compute alone."""
    args = ("--steps", "300", "--warmup", "256")
    _, a = run(bench, capsys, tmp_path / "plain", *args)
    line, b = run(bench, capsys, tmp_path / "full", *args, "--full", "--no-pmc", "--no-cpu-baseline", "--no-step-api",
                  "--no-sb3-api")
    assert line["shard_check"]["result"] == "bit-identical"
    assert line["policy_api"]["kernel_us"] > 0 and line["roofline"]["kernel_us_probe"] > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
