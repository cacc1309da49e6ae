"""ha_host_adam_step on the CPU (no GPU needed): the gradient-norm clip and Adam's step of
include/hedge_actor.h, contract O1-O5, against a NumPy restatement bit for bit (NumPy's f32 * + / and
sqrt are correctly rounded, one rounding per operation; the f64 tree of O1 is restated with slices),
against an f64 restatement of clip_grad_norm_ + Adam within 4 x the error of torch's own f32
clip_grad_norm_ + torch.optim.Adam (the bound of DESIGN 18-20), DeviceAdam's state dict in
torch.optim.Adam's layout, and what the entry points refuse."""
import ctypes
import math

import numpy as np
import pytest

from cantorrl_amd import agent
from cantorrl_amd.agent import POLICY_KEYS

SIZES = (1, 2, 255, 256, 257, 1027)          # below, at and above one block of 256; four blocks and a tail
MODULE_SHAPES = tuple(shape for _, _, shape in POLICY_KEYS)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
F32 = np.float32


class Tensor(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("numel", ctypes.c_int64)]


class Hyper(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("lr", "beta1", "beta2", "eps", "max_grad_norm")] + \
               [("t", ctypes.c_int64), ("grad_norm_out", ctypes.c_void_p)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_state(shapes, seed, grad_scale=None):
    """Parameters +-0.5, zero moments, and gradients of per-tensor scales 1e-4 .. 1 (log-spaced)."""
    rng = np.random.default_rng(seed)
    scales = np.logspace(-4, 0, len(shapes)) if grad_scale is None else np.full(len(shapes), grad_scale)
    st = []
    for shape, s in zip(shapes, scales):
        st.append(dict(param=rng.uniform(-0.5, 0.5, shape).astype(F32), exp_avg=np.zeros(shape, F32),
                       exp_avg_sq=np.zeros(shape, F32), grad=(rng.standard_normal(shape) * s).astype(F32)))
    return st


def new_grads(state, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    scales = np.logspace(-4, 0, len(state)) * scale
    for T, s in zip(state, scales):
        T["grad"] = (rng.standard_normal(T["grad"].shape) * s).astype(F32)


def copy_state(state):
    return [{k: v.copy() for k, v in T.items()} for T in state]


def host_step(state, t, max_grad_norm, **hyper):
    """ha_host_adam_step over the arrays of `state`, in place -> (status, grad_norm)."""
    lib = agent.load()
    arr = (Tensor * max(len(state), 1))()
    for a, T in zip(arr, state):
        for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
            assert T[k].dtype == F32 and T[k].flags.c_contiguous
            setattr(a, k, T[k].ctypes.data)
        a.numel = T["param"].size
    norm = np.full(1, np.nan, F32)
    h = dict(HYPER, **hyper)
    hy = Hyper(h["lr"], h["beta1"], h["beta2"], h["eps"], max_grad_norm, t, norm.ctypes.data)
    return lib.ha_host_adam_step(len(state), arr, ctypes.byref(hy)), norm[0]


def numpy_step(state, t, max_grad_norm, lr, beta1, beta2, eps):
    """Contract O1-O5 restated: `state` updated in place -> grad_norm (f32)."""
    total = np.float64(0.0)
    for T in state:                                             # O1, O2
        g = T["grad"].reshape(-1)
        nb = -(-g.size // 256)
        q = np.zeros(nb * 256, np.float64)
        q[:g.size] = g.astype(np.float64)
        q = (q * q).reshape(nb, 256)
        off = 128
        while off >= 1:
            q = q[:, :off] + q[:, off:2 * off]
            off //= 2
        for s in q[:, 0]:
            total = total + s
    norm = F32(np.sqrt(total))                                  # O3
    c = F32(1.0)                                                # O4
    if max_grad_norm > 0.0 and math.isfinite(max_grad_norm):
        q = F32(max_grad_norm) / (norm + F32(1e-6))
        c = q if q < F32(1.0) else F32(1.0)
    b1, b2, a1, a2 = F32(beta1), F32(beta2), F32(1.0 - beta1), F32(1.0 - beta2)
    ss, bc2s, e = F32(lr / (1.0 - beta1 ** t)), F32(math.sqrt(1.0 - beta2 ** t)), F32(eps)
    for T in state:                                             # O5
        gc = T["grad"] * c
        m = b1 * T["exp_avg"] + a1 * gc
        v = b2 * T["exp_avg_sq"] + a2 * (gc * gc)
        den = np.sqrt(v) / bc2s + e
        p = T["param"] - ss * (m / den)
        for k, x in (("exp_avg", m), ("exp_avg_sq", v), ("param", p)):
            assert x.dtype == F32
            T[k] = x
    return norm


def assert_same_bits(a, b, what):
    for j, (x, y) in enumerate(zip(a, b)):
        for k in ("param", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(bits(x[k]), bits(y[k])), (what, j, k)


def shapes_of(kind):
    return [(n,) for n in SIZES] if kind == "sizes" else list(MODULE_SHAPES)


# max_grad_norm against gradients of norm ~ sqrt(numel) x scale: far above (c = 1 exactly), far below, none
CLIPS = {"below_max": 1e6, "above_max": 0.5, "no_clip": 0.0, "inf": math.inf}


@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("kind", ["sizes", "module"])
def test_host_build_equals_the_numpy_restatement_bitwise_over_five_steps(kind, clip):
    mgn = CLIPS[clip]
    a = make_state(shapes_of(kind), seed=11)
    b = copy_state(a)
    for t in range(1, 6):
        new_grads(a, 100 + t)
        for x, y in zip(a, b):
            y["grad"] = x["grad"].copy()
        keep = [x["grad"].copy() for x in a]
        st, norm = host_step(a, t, mgn)
        want = numpy_step(b, t, mgn, **HYPER)
        assert st == 0
        assert bits(norm) == bits(want), (t, norm, want)
        assert_same_bits(a, b, t)
        for x, g in zip(a, keep):
            assert np.array_equal(bits(x["grad"]), bits(g))     # grad is read, never written
        if clip == "above_max":
            assert norm > 2 * mgn
        if clip == "below_max":
            assert norm < mgn / 2
    assert all(np.isfinite(x["param"]).all() and np.abs(x["exp_avg"]).max() > 0 for x in a)


def test_clip_coefficient_is_one_where_nothing_clips_and_zero_gradients_move_nothing_at_step_one():
    a = make_state(shapes_of("sizes"), seed=3)
    b, c = copy_state(a), copy_state(a)
    st, n1 = host_step(a, 1, 1e6)
    st2, n2 = host_step(b, 1, 0.0)
    assert st == 0 and st2 == 0 and bits(n1) == bits(n2)
    assert_same_bits(a, b, "c == 1")                            # g * 1 is g: the same bits as no clip
    for T in c:
        T["grad"][...] = 0.0
    before = copy_state(c)
    st, n0 = host_step(c, 1, 0.5)
    want = numpy_step(before, 1, 0.5, **HYPER)
    assert st == 0 and n0 == 0.0 and want == 0.0
    assert_same_bits(c, before, "zero gradient")
    for T, B in zip(c, make_state(shapes_of("sizes"), seed=3)):
        assert np.array_equal(T["param"], B["param"]) and not T["exp_avg"].any() and not T["exp_avg_sq"].any()


def test_nothing_depends_on_how_tensors_are_grouped():
    """(a) Without a clip the update of an element depends on its own tensor alone: the list split over
    two calls gives the bits of one call.  (b) With a clip the norm spans the call, and a tensor cut at
    a multiple of 256 elements into two tensors has the same blocks in the same order: the same bits."""
    one = make_state(shapes_of("sizes"), seed=5)
    two = copy_state(one)
    assert host_step(one, 3, 0.0)[0] == 0
    assert host_step(two[:2], 3, 0.0)[0] == 0 and host_step(two[2:], 3, 0.0)[0] == 0
    assert_same_bits(one, two, "split list")
    whole = make_state([(1027,), (300,)], seed=6, grad_scale=1.0)
    cut = []
    for T in whole:
        n = T["param"].size
        for sl in ((slice(0, 512), slice(512, n)) if n > 512 else (slice(0, 256), slice(256, n))):
            cut.append({k: v[sl].copy() for k, v in T.items()})
    st, n_whole = host_step(whole, 2, 0.5)
    st2, n_cut = host_step(cut, 2, 0.5)
    assert st == 0 and st2 == 0 and n_whole > 1.0 and bits(n_whole) == bits(n_cut)
    glued = [{k: np.concatenate([cut[2 * j][k], cut[2 * j + 1][k]]) for k in cut[0]} for j in range(2)]
    assert_same_bits(whole, glued, "cut at a block boundary")


# --------------------------------------------------------------------------- against f64, torch's error as the yardstick
def f64_step(state, t, max_grad_norm, lr, beta1, beta2, eps):
    """clip_grad_norm_ + Adam restated in f64 over f64 copies (the gradients are the f32 ones)."""
    g64 = [T["grad"].astype(np.float64) for T in state]
    norm = math.sqrt(sum(float((g * g).sum()) for g in g64))
    c = min(1.0, max_grad_norm / (norm + 1e-6))
    for T, g in zip(state, g64):
        g = g * c
        T["exp_avg"] = beta1 * T["exp_avg"] + (1.0 - beta1) * g
        T["exp_avg_sq"] = beta2 * T["exp_avg_sq"] + (1.0 - beta2) * g * g
        den = np.sqrt(T["exp_avg_sq"]) / math.sqrt(1.0 - beta2 ** t) + eps
        T["param"] = T["param"] - lr / (1.0 - beta1 ** t) * (T["exp_avg"] / den)


def five_steps_against_f64(run_build, run_torch, shapes, mgn=0.5):
    """The build's and torch's f32 parameters after 5 steps against the f64 restatement, per tensor ->
    [(error of the build, d_ref, one ulp of the tensor's largest parameter)]."""
    start = make_state(shapes, seed=21)
    grads = []
    for t in range(1, 6):
        new_grads(start, 300 + t)
        grads.append([T["grad"].copy() for T in start])
    ref = [{k: v.astype(np.float64) for k, v in T.items()} for T in start]
    for t, gs in enumerate(grads, 1):
        for T, g in zip(ref, gs):
            T["grad"] = g
        f64_step(ref, t, mgn, **HYPER)
    build = run_build(copy_state(start), grads, mgn)
    torch_p = run_torch(copy_state(start), grads, mgn)
    out = []
    for j, T in enumerate(ref):
        err = float(np.abs(build[j].astype(np.float64) - T["param"]).max())
        d_ref = float(np.abs(torch_p[j].astype(np.float64) - T["param"]).max())
        ulp = float(np.spacing(F32(np.abs(start[j]["param"]).max())))
        out.append((err, d_ref, ulp))
    return out


def torch_adam_steps(state, grads, mgn, device="cpu", **kw):
    import torch
    ps = [torch.nn.Parameter(torch.from_numpy(T["param"].copy()).to(device)) for T in state]
    opt = torch.optim.Adam(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], **kw)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy()).to(device)
        torch.nn.utils.clip_grad_norm_(ps, mgn)
        opt.step()
    return [p.detach().cpu().numpy() for p in ps]


def host_adam_steps(state, grads, mgn):
    for t, gs in enumerate(grads, 1):
        for T, g in zip(state, gs):
            T["grad"] = g.copy()
        assert host_step(state, t, mgn)[0] == 0
    return [T["param"] for T in state]


@pytest.mark.parametrize("kind", ["sizes", "module"])
def test_five_steps_stay_within_4_d_ref_of_the_f64_restatement(kind):
    pytest.importorskip("torch")
    res = five_steps_against_f64(host_adam_steps, torch_adam_steps, shapes_of(kind))
    for j, (err, d_ref, ulp) in enumerate(res):
        print(f"tensor {j}: build {err:.3e} torch {d_ref:.3e} ulp {ulp:.3e}")
        assert err <= 4 * d_ref + ulp, (j, err, d_ref, ulp)
    assert max(d for _, d, _ in res) > 0.0


# --------------------------------------------------------------------------- DeviceAdam on CPU parameters
def test_device_adam_on_cpu_parameters_runs_the_host_build_and_trades_state_with_torch_adam():
    torch = pytest.importorskip("torch")
    import cantorrl_amd
    from cantorrl_amd import train
    assert cantorrl_amd.DeviceAdam is train.DeviceAdam and issubclass(train.DeviceAdam, torch.optim.Optimizer)
    state = make_state(shapes_of("sizes"), seed=8)
    ps = [torch.nn.Parameter(torch.from_numpy(T["param"].copy())) for T in state]
    opt = train.DeviceAdam(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"])
    with pytest.raises(ValueError, match="no gradient"):
        opt.clip_and_step(0.5)
    for t in (1, 2):
        new_grads(state, 50 + t)
        for p, T in zip(ps, state):
            p.grad = torch.from_numpy(T["grad"].copy())
        norm = opt.clip_and_step(0.5) if t == 1 else (opt.step(), None)[1]
        want = numpy_step(state, t, 0.5 if t == 1 else 0.0, **HYPER)
        if t == 1:
            assert norm.dim() == 0 and bits(norm.numpy()) == bits(want)
        for p, T in zip(ps, state):
            assert np.array_equal(bits(p.detach().numpy()), bits(T["param"]))
            assert np.array_equal(bits(opt.state[p]["exp_avg_sq"].numpy()), bits(T["exp_avg_sq"]))
    # the scheduler's lr is the one the next step uses
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: 0.5)
    assert opt.param_groups[0]["lr"] == 0.5 * HYPER["lr"]
    del sched
    # torch.optim.Adam's layout: into an Adam, one step there, and back
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 2.0
    adam = torch.optim.Adam(ps, lr=1.0)
    adam.load_state_dict(sd)
    assert adam.param_groups[0]["lr"] == 0.5 * HYPER["lr"]
    assert torch.equal(adam.state[ps[3]]["exp_avg"], opt.state[ps[3]]["exp_avg"])
    adam.step()
    back = train.DeviceAdam(ps)
    back.load_state_dict(adam.state_dict())
    assert float(back.state[ps[0]]["step"]) == 3.0 and back.param_groups[0]["eps"] == HYPER["eps"]
    before = [p.detach().clone() for p in ps]
    back.step()
    assert float(back.state[ps[0]]["step"]) == 4.0
    assert all(not torch.equal(p.detach(), b) for p, b in zip(ps, before))


# --------------------------------------------------------------------------- what the entry points refuse
def test_adam_entry_points_refuse_bad_arguments():
    lib = agent.load()
    err = lambda: lib.ha_policy_last_error(None)
    one = make_state([(5,)], seed=1)
    assert host_step(one, 1, 0.5)[0] == 0
    assert host_step([], 1, 0.5)[0] == 2 and b"n_tensors" in err()                       # HE_ESHAPE
    assert host_step(make_state([(1,)] * 65, seed=1), 1, 0.5)[0] == 2
    assert host_step(make_state([(1,)] * 64, seed=1), 1, 0.5)[0] == 0
    assert host_step(make_state([(4096 * 256 + 1,)], seed=1), 1, 0.5)[0] == 2 and b"blocks" in err()
    assert host_step(one, 0, 0.5)[0] == 1 and b"step count" in err()                     # HE_EINVAL
    assert host_step(one, 1, 0.5, beta1=1.0)[0] == 1
    assert host_step(one, 1, 0.5, eps=-1.0)[0] == 1
    assert host_step(one, 1, 0.5, lr=math.nan)[0] == 1
    arr = (Tensor * 1)()
    hy = Hyper(1e-3, 0.9, 0.999, 1e-8, 0.5, 1, None)
    p = one[0]["param"]
    arr[0].param, arr[0].grad, arr[0].exp_avg, arr[0].exp_avg_sq = p.ctypes.data, None, p.ctypes.data, p.ctypes.data
    arr[0].numel = 0
    assert lib.ha_host_adam_step(1, arr, ctypes.byref(hy)) == 2 and b"numel" in err()
    assert lib.ha_adam_workspace_bytes(1, arr) == 0
    arr[0].numel = 5
    assert lib.ha_host_adam_step(1, arr, ctypes.byref(hy)) == 1 and b"NULL" in err()
    assert lib.ha_host_adam_step(1, None, ctypes.byref(hy)) == 1
    assert lib.ha_host_adam_step(1, arr, None) == 1
    # the workspace: one f64 per block of 256
    assert lib.ha_adam_workspace_bytes(1, arr) == 8
    arr[0].numel = 257
    assert lib.ha_adam_workspace_bytes(1, arr) == 16
    blocks = sum(-(-int(np.prod(s)) // 256) for s in MODULE_SHAPES)
    assert blocks == 677                                                                 # the module's 21 tensors
    # the device call checks before it launches (no device is touched: this runs without a GPU)
    assert lib.ha_adam_step(0, arr, ctypes.byref(hy), None, None) == 2
    arr[0].grad = p.ctypes.data
    assert lib.ha_adam_step(1, arr, ctypes.byref(hy), None, None) == 1 and b"workspace" in err()


def test_new_kernels_use_no_scratch():
    import importlib.util
    import os
    import shutil
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
    for name in ("opt_norm_kernel", "opt_adam_kernel", "policy_pack_kernel"):
        rows = [v for k, v in meta.items() if name in k]
        assert len(rows) == 1, (name, sorted(meta))
        assert rows[0]["scratch_B"] == 0 and rows[0]["vgpr_spill"] == 0 and rows[0]["sgpr_spill"] == 0, (name, rows[0])
