"""The LSTM's weight gradients on the CPU (no GPU needed): ha_host_lstm_seq_weight_grads -- contract
W1-W4 of include/hedge_actor.h, the device kernels' arithmetic compiled for the host -- against the
definition of z on exactly representable data, against a NumPy restatement of W1-W4 bit for bit,
against torch autograd of the f64 restatement within the project's 4 x d_ref, the masking at episode
starts, pair against single, the raw ABI's argument checks and the built code object."""
import importlib.util
import os
import shutil
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cantorrl_amd import _lib, agent, train  # noqa: E402
from test_lstm_seq_cpu import (GRAD_NAMES, PATTERNS, WEIGHTS, autograd_reference, bits, d_h_for, host_backward,  # noqa: E402
                               net_inputs, seq_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, CHUNK = train.WGRAD_BLOCK, train.WGRAD_CHUNK
T = torch.from_numpy


def test_constants_mirror_the_header():
    src = open(os.path.join(ROOT, "include", "hedge_actor.h")).read()
    assert f"#define HA_WGRAD_BLOCK {BLOCK} " in src and f"#define HA_WGRAD_CHUNK {CHUNK} " in src


# --------------------------------------------------------------------------- helpers
def z_rows(x, es, h, h0):
    """z [R, 142] of the contract: x, h_prev (h shifted by a step, h0 in front, 0 at a start), 1."""
    L, B = es.shape
    h_prev = np.concatenate([h0[None], h[:-1]]) * (es == 0)[:, :, None].astype(np.float32)
    return np.concatenate([x, h_prev, np.ones((L, B, 1), np.float32)], -1).reshape(L * B, 142)


def split(total):
    """W4: [512, 142] f64 -> d_w_ih, d_w_hh, d_b, each rounded once."""
    t = total.astype(np.float32)
    return t[:, :13], t[:, 13:141], t[:, 141]


def host_wgrad(x, es, nets):
    """The host build: nets = dicts of NumPy d_gates, h, h0 -> [(d_w_ih, d_w_hh, d_b)] as NumPy."""
    out = train.lstm_seq_weight_grads(T(x), T(es), [{k: T(v) for k, v in n.items()} for n in nets], host=True)
    return [tuple(t.numpy() for t in g) for g in out]


def random_starts(rng, L, B):
    """Random starts that include t = 0 and an env that starts at every step."""
    es = (rng.random((L, B)) < 0.3).astype(np.uint8)
    es[0, ::2] = 1
    es[:, B // 2] = 1
    return es


def random_case(L, B, seed, quantised):
    rng = np.random.default_rng(seed)

    def draw(shape):
        if quantised:   # multiples of 2^-6 in [-1, 1]
            return (rng.integers(-64, 65, shape) / 64.0).astype(np.float32)
        return rng.standard_normal(shape).astype(np.float32)

    nets = [dict(d_gates=draw((L, B, 4, 128)), h=draw((L, B, 128)), h0=draw((B, 128))) for _ in range(2)]
    return draw((L, B, 13)), random_starts(rng, L, B), nets


EDGE_SHAPES = ((1, 1), (2, 2), (9, 33), (1, BLOCK), (1, BLOCK + 1), (2, BLOCK * CHUNK // 2 + 1))


# --------------------------------------------------------------------------- 1. layout and masking
@pytest.mark.parametrize("L,B", EDGE_SHAPES)
def test_layout_and_masking_exact_on_quantised_data(L, B):
    """Multiples of 2^-6 in [-1, 1]: a product has 14 bits, a 128-row sum fits 24, every chain is exact
    in any order, so the outputs are the f64 einsum of the definition, rounded once."""
    x, es, nets = random_case(L, B, 100 * L + B, quantised=True)
    assert es[0].any() and es.all(0).any()
    assert (L, B) != EDGE_SHAPES[-1] or L * B == BLOCK * CHUNK + 2
    got = host_wgrad(x, es, nets[:1])[0]
    n = nets[0]
    total = np.einsum("ru,rk->uk", n["d_gates"].reshape(L * B, 512).astype(np.float64),
                      z_rows(x, es, n["h"], n["h0"]).astype(np.float64))
    for name, a, b in zip(("d_w_ih", "d_w_hh", "d_b"), got, split(total)):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (name, L, B)
    assert np.abs(got[0]).max() > 0 and np.abs(got[2]).max() > 0
    assert L == 1 and es.all() or np.abs(got[1]).max() > 0


# --------------------------------------------------------------------------- 2. order
def restate(dg, z):
    """W1-W4 one row at a time, fmaf emulated as f32(f64(a) f64(b) + f64(s)) (the product is exact in
    f64) -> total [512, 142] f64 and the mask of elements whose chain met a value where the
    emulation can differ from fmaf: an f64 sum that was ROUNDED onto an f32 midpoint, or a subnormal
    result.  (A sum that is exact in f64 and lies on a midpoint -- every other term of the bias column,
    whose products are d_gates itself -- rounds to even in one step as fmaf does: it is compared, not
    left out.  Whether the f64 sum was exact is the error term of Knuth's TwoSum.)"""
    R = dg.shape[0]
    dg64, z64 = dg.astype(np.float64), z.astype(np.float64)
    total = np.zeros((512, 142))
    doubt = np.zeros((512, 142), bool)
    tiny = float(np.finfo(np.float32).tiny)
    for c0 in range(0, R, BLOCK * CHUNK):
        part = np.zeros((512, 142))
        for b0 in range(c0, min(c0 + BLOCK * CHUNK, R), BLOCK):
            s = np.zeros((512, 142), np.float32)
            for r in range(b0, min(b0 + BLOCK, R)):
                prod, s_in = dg64[r][:, None] * z64[r][None, :], s.astype(np.float64)
                s64 = prod + s_in
                mid = (s64.view(np.int64) & 0x1FFFFFFF) == 0x10000000
                if mid.any():
                    bb = s64 - prod
                    doubt |= mid & (((prod - (s64 - bb)) + (s_in - bb)) != 0.0)
                doubt |= (np.abs(s64) < tiny) & (s64 != 0.0)
                s = s64.astype(np.float32)
            if b0 + BLOCK > R:
                s = s + np.float32(0.0)   # the padding terms fmaf(+0, +0, s)
            part += s.astype(np.float64)
        total += part
    return total, doubt


def test_order_equals_the_numpy_restatement_bitwise():
    kind, L, B = "golden", 40, 65
    case = seq_case(kind, "mid", L, B)
    d_gates = host_backward(kind, case, d_h_for(case))
    nets = [dict(d_gates=dg.numpy(), h=o[0].numpy(), h0=case["states"][2 * k])
            for k, (dg, o) in enumerate(zip(d_gates, case["out"]))]
    got = host_wgrad(case["x"], case["es"], nets)
    for k, n in enumerate(nets[:1]):   # (the actor: the restatement is a Python loop over the rows)
        total, doubt = restate(n["d_gates"].reshape(L * B, 512), z_rows(case["x"], case["es"], n["h"], n["h0"]))
        frac = doubt.mean()
        print(f"net {k}: {int(doubt.sum())} of {doubt.size} elements left out ({100 * frac:.3f} %)")
        assert frac <= 0.005
        keep = ~doubt
        for name, a, b, m in zip(("d_w_ih", "d_w_hh", "d_b"), got[k], split(total), split(keep)):
            m = m.astype(bool)
            assert np.array_equal(bits(a)[m], bits(b)[m]), (name, k)
        assert np.abs(got[k][1]).max() > 1e-3


# --------------------------------------------------------------------------- 3. accuracy
_REF = {}


def references(kind, pattern, L, B, k):
    """(r64, r32) of autograd_reference for network k of a case, computed once."""
    key = (kind, pattern, L, B, k)
    if key not in _REF:
        case = seq_case(kind, pattern, L, B)
        net = net_inputs(kind, case["states"])[k]
        x, es = T(case["x"]), T(case["es"])
        d_h = d_h_for(case)[k]
        _REF[key] = (autograd_reference(net, x, es, d_h, torch.float64), autograd_reference(net, x, es, d_h, torch.float32))
    return _REF[key]


def kernel_mode_grads(kind, case, device="cpu"):
    """The weight gradients of sum(h d_h) of both networks through lstm_sequence(weight_grads="kernel")."""
    x, es = T(case["x"]).to(device), T(case["es"]).to(device)
    out = []
    for net, d_h in zip(net_inputs(kind, case["states"]), d_h_for(case)):
        net = {k: v.to(device) for k, v in net.items()}
        w = [net[k].clone().requires_grad_() for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
        h = train.lstm_sequence(x, es, net["h0"], net["c0"], *w, weight_grads="kernel")
        (h * d_h.to(device)).sum().backward()
        out.append([p.grad.cpu() for p in w])
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", WEIGHTS)
def test_kernel_mode_within_4_d_ref_of_f64_autograd(kind, pattern):
    worst = 0.0
    for L, B in ((2, 33), (9, 33), (40, 65)):
        case = seq_case(kind, pattern, L, B)
        for k, grads in enumerate(kernel_mode_grads(kind, case)):
            r64, r32 = references(kind, pattern, L, B, k)
            for name, g, b, r in zip(GRAD_NAMES[1:], grads, r32[1:], r64[1:]):
                assert g.dtype == torch.float32
                err, d_ref = float((g.double() - r).abs().max()), float((b - r).abs().max())
                ratio = err / d_ref if d_ref > 0.0 else 0.0
                worst = max(worst, ratio)
                print(f"{kind} {pattern} L {L} B {B} net {k} {name}: kernel mode {err:.3e} reference {d_ref:.3e} "
                      f"ratio {ratio:.2f}")
                assert d_ref > 0.0 or err == 0.0
                assert err <= 4 * d_ref, (name, err, d_ref)
    print(f"{kind} {pattern}: largest ratio {worst:.2f}")


# --------------------------------------------------------------------------- 4. masking
def test_no_leak_across_a_start():
    L, B = 5, 3
    x, _, nets = random_case(L, B, 3, quantised=False)
    es = np.zeros((L, B), np.uint8)
    es[2, 1] = 1   # env 1 starts at step 2: h[1][1] is not its h_prev; env 0 runs on
    base = host_wgrad(x, es, nets[:1])[0]
    for env, same in ((1, True), (0, False)):
        bumped = dict(nets[0], h=nets[0]["h"].copy())
        bumped["h"][1, env] += 1.0
        moved = host_wgrad(x, es, [bumped])[0]
        assert np.array_equal(bits(moved[0]), bits(base[0])) and np.array_equal(bits(moved[2]), bits(base[2]))
        assert np.array_equal(bits(moved[1]), bits(base[1])) == same, env
    # h0 of an env that starts at t = 0 is not read either
    es[0, 2] = 1
    base = host_wgrad(x, es, nets[:1])[0]
    bumped = dict(nets[0], h0=nets[0]["h0"].copy())
    bumped["h0"][2] += 1.0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(host_wgrad(x, es, [bumped])[0], base))
    bumped["h0"][0] += 1.0
    assert not np.array_equal(host_wgrad(x, es, [bumped])[0][1], base[1])


# --------------------------------------------------------------------------- 5. pair and single
def test_pair_equals_the_two_single_calls_bitwise():
    for L, B in ((3, 43), (1, BLOCK + 1)):
        x, es, nets = random_case(L, B, 11, quantised=False)
        pair = host_wgrad(x, es, nets)
        for k in range(2):
            single = host_wgrad(x, es, [nets[k]])[0]
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(pair[k], single)), (L, B, k)
        assert not np.array_equal(pair[0][1], pair[1][1])


# --------------------------------------------------------------------------- 6. the raw ABI
def test_abi_argument_checks_return_the_status_codes():
    lib = agent.load()
    L = B = 2
    x, es, nets = random_case(L, B, 1, quantised=False)
    x, es = T(x), T(es)
    arr = (train.HaLstmSeqWgrad * 2)()
    keep = []
    for k, n in enumerate(nets):
        for name, v in n.items():
            keep.append(T(v))
            setattr(arr[k], name, keep[-1].data_ptr())
        for name, shape in (("d_w_ih", (512, 13)), ("d_w_hh", (512, 128)), ("d_b", (512,))):
            keep.append(torch.zeros(shape))
            setattr(arr[k], name, keep[-1].data_ptr())
    host = lib.ha_host_lstm_seq_weight_grads
    err = lib.ha_policy_last_error
    assert host(2, L, B, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_OK
    assert float(keep[-1].abs().max()) > 0.0
    assert host(3, L, B, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE and b"n_nets" in err(None)
    assert host(0, L, B, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert host(2, 0, B, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE and b"steps" in err(None)
    assert host(2, L, 0, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert host(2, L, 2 ** 31, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert host(2, L, B, None, es.data_ptr(), arr) == _lib.HE_EINVAL
    assert host(2, L, B, x.data_ptr(), None, arr) == _lib.HE_EINVAL
    assert host(2, L, B, x.data_ptr(), es.data_ptr(), None) == _lib.HE_EINVAL and b"nets" in err(None)
    bad = (train.HaLstmSeqWgrad * 2).from_buffer_copy(arr)
    bad[1].d_b = None
    assert host(2, L, B, x.data_ptr(), es.data_ptr(), bad) == _lib.HE_EINVAL and b"ha_lstm_seq_wgrad" in err(None)
    assert host(1, L, B, x.data_ptr(), es.data_ptr(), bad) == _lib.HE_OK   # the second struct is not read
    # the device entry point checks before it launches: nothing below reaches a kernel
    dev = lib.ha_lstm_seq_weight_grads
    ws = torch.zeros(16)
    assert dev(2, L, B, x.data_ptr(), es.data_ptr(), arr, None, None) == _lib.HE_EINVAL and b"workspace" in err(None)
    assert dev(2, L, B, x.data_ptr(), es.data_ptr(), arr, ws.data_ptr() + 4, None) == _lib.HE_EINVAL
    bad = (train.HaLstmSeqWgrad * 2).from_buffer_copy(arr)
    bad[0].h0 = arr[0].h0 + 4
    assert dev(2, L, B, x.data_ptr(), es.data_ptr(), bad, ws.data_ptr(), None) == _lib.HE_EINVAL
    assert b"aligned" in err(None)
    assert dev(2, L, B, None, es.data_ptr(), arr, ws.data_ptr(), None) == _lib.HE_EINVAL
    assert dev(4, L, B, x.data_ptr(), es.data_ptr(), arr, ws.data_ptr(), None) == _lib.HE_ESHAPE
    assert dev(2, L, -1, x.data_ptr(), es.data_ptr(), arr, ws.data_ptr(), None) == _lib.HE_ESHAPE
    assert dev(2, 2 ** 30, 2 ** 30, x.data_ptr(), es.data_ptr(), arr, ws.data_ptr(), None) == _lib.HE_ESHAPE
    assert b"chunks" in err(None)
    size = lib.ha_lstm_seq_weight_grads_workspace_bytes
    one = size(1, L, B)
    assert one == 512 * 142 * 8 and size(2, L, B) == 2 * one and size(1, 1, BLOCK * CHUNK) == one
    assert size(1, 1, BLOCK * CHUNK + 1) == 2 * one
    assert size(3, L, B) == 0 and size(0, L, B) == 0 and size(1, 0, B) == 0 and size(1, L, 2 ** 31) == 0
    # the Python layer
    nets_t = [{k: T(v) for k, v in n.items()} for n in nets]
    with pytest.raises(ValueError, match="x must be"):
        train.lstm_seq_weight_grads(x[:, :, :12], es, nets_t)
    with pytest.raises(ValueError, match="d_gates"):
        train.lstm_seq_weight_grads(x, es, [dict(nets_t[0], d_gates=nets_t[0]["d_gates"][:, :, :2])])
    with pytest.raises(ValueError, match="n_nets"):
        train.lstm_seq_weight_grads(x, es, nets_t + nets_t[:1])


def test_a_bad_weight_grads_keyword_is_a_value_error():
    case = seq_case("random", "none", 2, 2)
    n = net_inputs("random", case["states"])
    x, es = T(case["x"]), T(case["es"])
    tup = [tuple(m[k] for k in train.NET_INPUTS) for m in n]
    with pytest.raises(ValueError, match="weight_grads"):
        train.lstm_sequence(x, es, *tup[0], weight_grads="rocblas")
    with pytest.raises(ValueError, match="weight_grads"):
        train.lstm_sequence_pair(x, es, tup[0], tup[1], weight_grads=None)
    with pytest.raises(ValueError, match="weight_grads"):
        train.RecurrentPPOModule(weight_grads="Kernel")
    assert train.RecurrentPPOModule().weight_grads == "torch"
    assert train.RecurrentPPOModule(weight_grads="kernel").weight_grads == "kernel"


def test_module_passes_the_keyword_on():
    """evaluate_actions of a weight_grads="kernel" module on the host build: db_ih equals db_hh, and the
    LSTM parameters' gradients are close to the default module's without being the same bits."""
    kind, L, B = "golden", 9, 33
    case = seq_case(kind, "mid", L, B)
    from test_lstm_seq_cpu import policy
    x, es = T(case["x"]), T(case["es"])
    states0 = tuple(T(s) for s in case["states"])
    acts = torch.zeros((L, B, 2))
    grads = {}
    for mode in train.WEIGHT_GRADS:
        m = train.RecurrentPPOModule.from_policy(policy(kind), device="cpu", weight_grads=mode)
        v, lp, _ = m.evaluate_actions(x, acts, es, states0)
        (v.sum() + lp.sum()).backward()
        grads[mode] = [p.grad.clone() for p in (*m.lstm_actor.tensors(), *m.lstm_critic.tensors())]
    k = grads["kernel"]
    assert torch.equal(k[2], k[3]) and torch.equal(k[6], k[7])
    # (a CPU BLAS may sum a 128-row block in the chain's own order: then only the bias sums differ)
    assert any(not torch.equal(a, b) for a, b in zip(k, grads["torch"]))
    for a, b in zip(k, grads["torch"]):
        assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())


# --------------------------------------------------------------------------- 7. the code object
def test_wgrad_kernels_use_no_scratch():
    for tool in ("llvm-readelf", "clang-offload-bundler"):
        if not os.path.exists(os.path.join("/opt/rocm/lib/llvm/bin", tool)):
            pytest.skip(f"{tool} absent")
    if shutil.which("objcopy") is None:
        pytest.skip("objcopy absent")
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    meta = {}
    with tempfile.TemporaryDirectory() as td:
        for co in km.code_objects(agent.LIB_PATH, td):
            meta.update(km.metadata(co))
    kernels = {k: v for k, v in meta.items() if "lstm_wgrad_" in k}
    assert len(kernels) == 2, sorted(meta)
    for k, v in kernels.items():
        assert v["scratch_B"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
    main = [v for k, v in kernels.items() if "lstm_wgrad_kernel" in k][0]
    red = [v for k, v in kernels.items() if "lstm_wgrad_reduce_kernel" in k][0]
    # z of two 32-row sub-blocks, 160 columns
    assert main["lds_B"] == 2 * 32 * 160 * 4 and red["lds_B"] == 0, (main, red)
    # one workgroup of 4 waves per CU, one wave per SIMD: 512 registers a lane (gfx950's vgpr_count is the
    # unified total, accumulation registers included)
    assert max(main["vgpr"], main["agpr"]) <= 512 and main["agpr"] <= 256, main
    assert red["vgpr"] + red["agpr"] <= 64, red
