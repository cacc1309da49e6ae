"""ha_host_ppo_loss, the host build of the PPO loss kernels (include/hedge_actor.h, contract L1-L6; no GPU
needed), against tests/_ppo_loss_contract.py, the contract written again in NumPy f64:

* bit for bit where exp cannot differ (log_prob == old_log_prob, so r = exp_k(0) = 1 exactly);
* on general inputs within one f32 ulp per statistic and gradient element: the f64 value before the one
  rounding carries a relative error of a few 2^-52 (he::exp_k is within one f64 ulp of exp), so the f32
  output is the reference's rounding or its neighbour; approx_kl gets 2^-48 absolute on top for the
  cancellation in (r - 1) - d;
* the same bound against torch autograd in f64 (tests/_ppo_reference.loss, and the clipped-value loss);
* seven deliberate mistakes in the restatement, each of which must break the agreement;
* the refusals, the Python surface (train.ppo_loss_kernel, ppo_loss's and ppo_update's new keywords), the
  structs' layout against the header, and no scratch in the new kernels."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _ppo_loss_contract as lc
from cantorrl_amd import agent

CLIP, ENT, VF, CLIP_VF = 0.3, 1e-5, 0.5, 0.2
HYPER = dict(clip_range=CLIP, ent_coef=ENT, vf_coef=VF)
BITWISE_N = (2, 3, 255, 256, 257, lc.BLOCK - 1, lc.BLOCK, lc.BLOCK + 1, 2 * lc.BLOCK + 3)
F32, F64 = np.float32, np.float64
_CASES = {}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def cases():
    if not _CASES:
        _CASES.update(lc.general_cases())
    return _CASES


def check_inputs(x, normalize, clip_vf):
    """The conditions under which the library's f64 takes the restatement's branches, on the restatement
    alone (as _ppo_reference.check_replay_inputs): chosen seeds meet them."""
    stats, _, aux = lc.contract(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)
    r, A = aux["ratio"], aux["adv"]
    assert np.abs(np.abs(r - 1.0) - CLIP).min() >= 1e-5, "a ratio within 1e-5 of a clip edge: choose another seed"
    assert np.abs(A).min() >= 1e-5, "|A'| < 1e-5: choose another seed"
    assert 0.05 <= stats["clip_fraction"] <= 0.95, stats["clip_fraction"]
    if clip_vf is not None:
        assert np.abs(np.abs(aux["dv"]) - clip_vf).min() >= 1e-5, "|v - old_v| within 1e-5 of clip_range_vf"
        assert 0.05 <= 1.0 - aux["passes"].mean() <= 0.95, aux["passes"].mean()


# --------------------------------------------------------------------------- 1: bit for bit
@pytest.mark.parametrize("clip_vf", (None, 0.25))
@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("N", BITWISE_N)
def test_host_build_equals_the_restatement_bitwise_where_exp_cannot_differ(N, normalize, clip_vf):
    x = lc.quantised_inputs(N, seed=100 + N)
    st, stats, grads = lc.host_loss(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)
    assert st == 0
    want_stats, want_grads = lc.rounded(*lc.contract(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)[:2])
    for j, k in enumerate(lc.STATS):
        assert bits(stats[j]) == bits(want_stats[j]), (k, stats[j], want_stats[j])
    for k in lc.GRADS:
        np.testing.assert_allclose(grads[k], want_grads[k], rtol=0, atol=0, err_msg=k)
        assert np.array_equal(bits(grads[k]), bits(want_grads[k])), k
    assert stats[4] == 0.0 and stats[5] == 0.0                       # r = 1: no KL, nothing clipped
    assert (stats[6], stats[7]) == (0.0, 1.0) or normalize
    if clip_vf is not None and N >= 255:                             # both sides of the value clip are there
        assert 0 < np.count_nonzero(grads["values"]) < N


# --------------------------------------------------------------------------- 2, 3: general inputs
@pytest.mark.parametrize("clip_vf", (None, CLIP_VF))
@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("name", sorted(lc.general_cases()))
def test_general_inputs_within_one_f32_ulp_of_the_restatement(name, normalize, clip_vf):
    x = cases()[name]
    check_inputs(x, normalize, clip_vf)
    st, stats, grads = lc.host_loss(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)
    assert st == 0
    want_stats, want_grads, aux = lc.contract(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)
    for j, k in enumerate(lc.STATS):
        print(f"{name} {k}: {stats[j]!r} reference {want_stats[k]!r}")
        assert lc.within_one_ulp(stats[j], want_stats[k], 2.0 ** -48 if k == "approx_kl" else 0.0), (k, stats[j], want_stats[k])
    for k in lc.GRADS:
        assert lc.within_one_ulp(grads[k], want_grads[k]), k
    assert lc.agrees(stats, grads, want_stats, want_grads)
    if name == "six_regions":
        r, A = aux["ratio"], aux["adv"]
        where = np.where(r < 1 - CLIP, 0, np.where(r > 1 + CLIP, 2, 1))
        assert len({(bool(a >= 0), int(w)) for a, w in zip(A, where)}) == 6
        assert 0 < np.count_nonzero(grads["log_prob"]) < x["values"].size
    # without a value clip the restatement is _ppo_reference.loss_numpy's loss: the two agree to f64 accuracy
    if clip_vf is None:
        import _ppo_reference as ref
        s, g = ref.loss_numpy(*(x[k] for k in lc.INPUTS), CLIP, ENT, VF, normalize)
        for k in lc.STATS[:6]:
            assert abs(s[k] - want_stats[k]) <= 1e-12 * max(1.0, abs(s[k])), k
        for k in lc.GRADS:
            assert np.abs(g[k] - want_grads[k]).max() <= 1e-12 * max(1.0, np.abs(g[k]).max()), k


# --------------------------------------------------------------------------- 4: against autograd
@pytest.mark.parametrize("clip_vf", (None, CLIP_VF))
@pytest.mark.parametrize("normalize", (True, False))
@pytest.mark.parametrize("name", ("pair0", "six_regions", "two_blocks"))
def test_gradients_within_one_f32_ulp_of_torch_autograd_in_f64(name, normalize, clip_vf):
    torch = pytest.importorskip("torch")
    import _ppo_reference as ref
    x = cases()[name]
    st, stats, grads = lc.host_loss(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)
    assert st == 0
    t = {k: torch.from_numpy(v.astype(F64)) for k, v in x.items()}
    leaves = [t[k].requires_grad_() for k in lc.GRADS]
    loss, ts = lc.torch_loss_clipped(ref, t, CLIP, ENT, VF, normalize, clip_vf)
    auto = torch.autograd.grad(loss, leaves)
    for k, g in zip(lc.GRADS, auto):
        assert lc.within_one_ulp(grads[k], g.numpy()), k
    for j, k in enumerate(lc.STATS[:6]):
        assert lc.within_one_ulp(stats[j], float(ts[k]), 2.0 ** -48 if k == "approx_kl" else 0.0), k


# --------------------------------------------------------------------------- 5: ties
def test_a_ratio_on_the_clip_edge_is_not_clipped_and_a_value_on_the_edge_passes_gradient():
    """log_prob - old_log_prob = 0 gives r = 1, so clip_range = 0 puts every row exactly on the edge:
    |r - 1| > 0 is false.  |v - old_v| = 0.25 = clip_range_vf exactly: torch.clamp passes gradient there."""
    x = lc.quantised_inputs(4, seed=1)
    x["old_values"] = (x["values"] + np.array([0.25, -0.25, 0.5, 0.0], F32)).astype(F32)
    st, stats, grads = lc.host_loss(x, 0.0, ENT, VF, False, 0.25)
    assert st == 0 and stats[5] == 0.0
    assert np.all(grads["log_prob"] == 0.0) and np.all(grads["values"][[0, 1, 3]] != 0.0) and grads["values"][2] == 0.0
    # a ratio off the edge by one f32 step of log_prob is counted
    x["log_prob"][0] = np.nextafter(x["log_prob"][0], F32(np.inf))
    st, stats, _ = lc.host_loss(x, 0.0, ENT, VF, False, 0.25)
    assert st == 0 and stats[5] == 0.25


# --------------------------------------------------------------------------- 6: mistakes are caught
@pytest.mark.parametrize("mistake", lc.MISTAKES)
def test_each_mistake_in_the_restatement_breaks_the_agreement(mistake):
    x = cases()["six_regions"]
    st, stats, grads = lc.host_loss(x, normalize_advantage=True, clip_range_vf=CLIP_VF, **HYPER)
    assert st == 0
    right = lc.contract(x, normalize_advantage=True, clip_range_vf=CLIP_VF, **HYPER)
    wrong = lc.contract(x, normalize_advantage=True, clip_range_vf=CLIP_VF, mistake=mistake, **HYPER)
    assert lc.agrees(stats, grads, right[0], right[1])
    assert not lc.agrees(stats, grads, wrong[0], wrong[1]), mistake


# --------------------------------------------------------------------------- 7: refusals
def test_entry_points_refuse_bad_arguments_and_leave_the_outputs_untouched():
    lib = agent.load()
    err = lambda: lib.ha_policy_last_error(None)
    x = lc.quantised_inputs(3, seed=2)

    def refused(status, word, **kw):
        call = dict(dict(HYPER, normalize_advantage=True, clip_range_vf=None), **kw)
        xx = call.pop("x", x)
        st, stats, grads = lc.host_loss(xx, fill=7.0, **call)
        assert st == status and word in err(), (st, err(), kw)
        assert np.all(stats == 7.0) and all(np.all(g == 7.0) for g in grads.values())

    assert lc.host_loss(x, **HYPER)[0] == 0
    refused(2, b"n_rows", n_rows=0)                                                      # HE_ESHAPE
    refused(2, b"n_rows", n_rows=lc.BLOCK * lc.MAX_BLOCKS + 1)
    refused(2, b"two rows", n_rows=1)
    assert lc.host_loss(x, normalize_advantage=False, n_rows=1, **HYPER)[0] == 0
    refused(1, b"NULL", x=dict(x, returns=None))                                         # HE_EINVAL
    refused(1, b"old_values", x=dict(x, old_values=None), clip_range_vf=0.2)
    assert lc.host_loss(dict(x, old_values=None), **HYPER)[0] == 0                       # not needed without a clip
    refused(1, b"clip_range", clip_range=-0.1)
    refused(1, b"clip_range", clip_range=math.nan)
    refused(1, b"clip_range", clip_range=math.inf)
    # a misaligned pointer, NULL structs, and the device call's checks (made before any launch: no GPU here)
    raw = np.zeros(3 * 4 + 1, np.uint8)
    io = lc.Io(*([x["values"].ctypes.data] * 11))
    io.log_prob = raw.ctypes.data + 1
    hy = lc.Hyper(CLIP, 0.0, ENT, VF, 1)
    assert lib.ha_host_ppo_loss(3, ctypes.byref(io), ctypes.byref(hy)) == 1 and b"aligned" in err()
    assert lib.ha_host_ppo_loss(3, None, ctypes.byref(hy)) == 1 and lib.ha_host_ppo_loss(3, ctypes.byref(io), None) == 1
    io.log_prob = x["log_prob"].ctypes.data
    assert lib.ha_ppo_loss(0, ctypes.byref(io), ctypes.byref(hy), None, None) == 2
    assert lib.ha_ppo_loss(3, ctypes.byref(io), ctypes.byref(hy), None, None) == 1 and b"workspace" in err()
    assert lib.ha_ppo_loss(3, ctypes.byref(io), ctypes.byref(hy), ctypes.c_void_p(12), None) == 1 and b"workspace" in err()
    # the workspace: seven f64 per block
    size = lib.ha_ppo_loss_workspace_bytes
    assert [size(n) for n in (0, 1, lc.BLOCK, lc.BLOCK + 1)] == [0, 56, 56, 112]
    assert size(256 * 16384) == 56 * lc.MAX_BLOCKS and size(256 * 16384 + 1) == 0


# --------------------------------------------------------------------------- 8: the Python surface
def test_ppo_loss_kernel_returns_the_inputs_shape_and_the_host_builds_bits():
    torch = pytest.importorskip("torch")
    import cantorrl_amd
    from cantorrl_amd import train
    assert cantorrl_amd.ppo_loss_kernel is train.ppo_loss_kernel
    L, B = 7, 5
    x = lc.random_inputs(L * B, 3)
    t = {k: torch.from_numpy(v.copy()).reshape(L, B) for k, v in x.items()}
    t["values"].requires_grad_()                                     # detached inside
    for clip_vf in (None, CLIP_VF):
        stats, grads = train.ppo_loss_kernel(*(t[k] for k in lc.INPUTS), CLIP, ENT, VF, True, clip_vf,
                                             None if clip_vf is None else t["old_values"])
        st, want_stats, want_grads = lc.host_loss(x, normalize_advantage=True, clip_range_vf=clip_vf, **HYPER)
        assert st == 0 and tuple(stats) == lc.STATS == train.LOSS_STATS
        for j, k in enumerate(lc.STATS):
            assert stats[k].dim() == 0 and bits(stats[k].numpy()) == bits(want_stats[j]), k
        for k, g in zip(lc.GRADS, grads):
            assert tuple(g.shape) == (L, B) and not g.requires_grad
            assert np.array_equal(bits(g.numpy().reshape(-1)), bits(want_grads[k])), k
    with pytest.raises(ValueError, match="two rows"):
        train.ppo_loss_kernel(*(t[k][:1, :1] for k in lc.INPUTS), CLIP, ENT, VF)
    with pytest.raises(ValueError, match="old_values"):
        train.ppo_loss_kernel(*(t[k] for k in lc.INPUTS), CLIP, ENT, VF, clip_range_vf=0.2)
    with pytest.raises(ValueError, match="float32"):
        train.ppo_loss_kernel(t["values"].double(), *(t[k] for k in lc.INPUTS[1:]), CLIP, ENT, VF)


def test_ppo_loss_without_a_value_clip_returns_the_bits_it_returned_and_clips_as_sb3_with_one():
    torch = pytest.importorskip("torch")
    import _ppo_reference as ref
    from cantorrl_amd import train
    x = lc.random_inputs(300, 4)
    t = {k: torch.from_numpy(v.copy()) for k, v in x.items()}
    args = [t[k] for k in lc.INPUTS] + [CLIP, ENT, VF]
    a, sa = train.ppo_loss(*args)
    b, sb = train.ppo_loss(*args, clip_range_vf=None, old_values=t["old_values"])
    assert bits(a.numpy()) == bits(b.numpy()) and set(sa) == set(sb) == set(lc.STATS[:6])
    assert all(bits(sa[k].numpy()) == bits(sb[k].numpy()) for k in sa)
    # with a clip: the f64 run is the restated clipped loss to f64 accuracy
    t64 = {k: v.double() for k, v in t.items()}
    got, _ = train.ppo_loss(*(t64[k] for k in lc.INPUTS), CLIP, ENT, VF, clip_range_vf=CLIP_VF, old_values=t64["old_values"])
    want, _ = lc.torch_loss_clipped(ref, t64, CLIP, ENT, VF, True, CLIP_VF)
    assert abs(float(got) - float(want)) <= 1e-12 and abs(float(got) - float(a)) > 1e-4
    with pytest.raises(ValueError, match="old_values"):
        train.ppo_loss(*args, clip_range_vf=0.2)


def test_ppo_update_with_the_kernel_loss_runs_an_epoch_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    from cantorrl_amd import train
    from test_ppo_replay_cpu import buffer, policy
    K, n, per, W = 8, 5, 2, 4
    pol, buf = policy("random"), buffer("random", K, n)
    start = train.RecurrentPPOModule.from_policy(pol, device="cpu")
    out = {}
    for loss, clip_vf in (("kernel", None), ("torch", None), ("kernel", CLIP_VF)):
        m = train.RecurrentPPOModule.from_policy(pol, device="cpu")
        opt = train.DeviceAdam(m.parameters(), lr=1e-4, eps=1e-5)
        stats = train.ppo_update(m, opt, buf, n_epochs=1, envs_per_batch=per, window=W, loss=loss, clip_range_vf=clip_vf,
                                 generator=torch.Generator().manual_seed(3))
        assert set(stats) >= set(lc.STATS[:6]) | {"grad_norm", "mean_loss"}
        assert all(v.dim() == 0 and bool(torch.isfinite(v)) for v in stats.values()), stats
        assert int(opt.state[m.log_std]["step"]) == 3 * 2
        assert all(not torch.equal(p, q) for p, q in zip(m.parameters(), start.parameters()))
        out[loss, clip_vf] = (m, stats)
    # the two paths take the same steps to f32 accuracy (no bound claimed on parameters: a sanity check)
    a, b = out["kernel", None][0], out["torch", None][0]
    assert max(float((p - q).detach().abs().max()) for p, q in zip(a.parameters(), b.parameters())) < 1e-5
    assert abs(float(out["kernel", None][1]["loss"]) - float(out["torch", None][1]["loss"])) < 1e-4
    assert float(out["kernel", CLIP_VF][1]["adv_std"]) > 0.0
    with pytest.raises(ValueError, match="loss must be"):
        train.ppo_update(a, torch.optim.SGD(a.parameters(), lr=1e-3), buf, n_epochs=1, loss="x")


# --------------------------------------------------------------------------- the structs and the kernels
def test_python_mirrors_of_the_loss_structs_match_the_header(tmp_path):
    pytest.importorskip("torch")
    from cantorrl_amd import train
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler (cc, gcc, clang) on the path")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    mirrors = (("ha_ppo_loss_hyper", train.HaPpoLossHyper, lc.Hyper), ("ha_ppo_loss_io", train.HaPpoLossIo, lc.Io))
    lines = ['printf("%d %d\\n", HA_LOSS_BLOCK, HA_LOSS_MAX_BLOCKS);']
    for cname, mirror, _ in mirrors:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hedge_actor.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", include, "-o", str(tmp_path / "abi"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.split()
    want = [lc.BLOCK, lc.MAX_BLOCKS]
    for _, mirror, twin in mirrors:
        layout = [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
        assert layout == [ctypes.sizeof(twin)] + [getattr(twin, f[0]).offset for f in twin._fields_]
        want += layout
    assert [int(v) for v in out] == want
    assert (train.LOSS_BLOCK, train.LOSS_MAX_BLOCKS) == (lc.BLOCK, lc.MAX_BLOCKS)


def test_loss_kernels_use_no_scratch():
    import importlib.util
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for tool in ("llvm-readelf", "clang-offload-bundler"):
        if not os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", tool)):
            pytest.skip(f"{tool} absent")
    if shutil.which("objcopy") is None:
        pytest.skip("objcopy absent")
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(root, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    meta = {}
    with tempfile.TemporaryDirectory() as td:
        for co in km.code_objects(agent.LIB_PATH, td):
            meta.update(km.metadata(co))
    for name in ("loss_mean_kernel", "loss_spread_kernel", "loss_rows_kernel", "loss_stats_kernel"):
        rows = [v for k, v in meta.items() if name in k]
        assert len(rows) == 1, (name, sorted(meta))
        assert rows[0]["scratch_B"] == 0 and rows[0]["vgpr_spill"] == 0 and rows[0]["sgpr_spill"] == 0, (name, rows[0])
