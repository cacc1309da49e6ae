"""The LSTM over a stored sequence on the CPU (no GPU needed): ha_host_lstm_seq_forward /
ha_host_lstm_seq_backward -- the device kernels' arithmetic compiled for the host -- against L
successive ha_host_policy_step calls bit for bit (contract F1), the stored gates recombined through
cell_update (F2), torch autograd of an f64 restatement of the same sequence (B1-B4), the gradient
masking at episode starts, the raw ABI's argument checks and the built code object.

Tolerance of the gradient comparison, as test_actor_cpu.py: d_ref = max |torch f32 restatement - torch
f64 restatement| per quantity, and the build has to stay within 4 x d_ref of the f64 restatement."""
import ctypes
import importlib.util
import os
import shutil
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from cantorrl_amd import _lib, agent, train  # noqa: E402
from cantorrl_amd.agent import POLICY_KEYS, RecurrentPolicy  # noqa: E402
from test_actor_cpu import golden, normalize  # noqa: E402
from test_policy_collect_cpu import bits, policy_state_dict, random_policy_weights  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS, LS = (1, 2, 33, 65), (1, 2, 9, 40)
PATTERNS = ("none", "ends", "mid")
WEIGHTS = ("golden", "random")
ACTOR = ("w_ih", "w_hh", "b_ih", "b_hh")
CRITIC = ("c_w_ih", "c_w_hh", "c_b_ih", "c_b_hh")


def start_pattern(pattern, L, B):
    """none; a start at t = 0 (even envs) and at t = L - 1 (every third env: env 0 has both); two
    consecutive starts mid-sequence at a step that differs per env, every fourth env left running."""
    es = np.zeros((L, B), np.uint8)
    if pattern == "ends":
        es[0, ::2] = 1
        es[L - 1, ::3] = 1
    elif pattern == "mid":
        for e in range(B):
            if e % 4 == 3:
                continue
            t0 = 1 + e % (L - 2) if L >= 3 else 0
            es[t0:t0 + 2, e] = 1
    return es


_POL, _CASE = {}, {}


def policy(kind):
    """A RecurrentPolicy without statistics: x is fed as it is."""
    if kind not in _POL:
        _POL[kind] = RecurrentPolicy.from_state_dict(policy_state_dict()) if kind == "golden" \
            else RecurrentPolicy(random_policy_weights(7))
    return _POL[kind]


def net_inputs(kind, states):
    """The NET_INPUTS dicts of actor and critic as CPU tensors."""
    a = policy(kind)._arrays
    T = torch.from_numpy
    return [dict(h0=T(states[0]), c0=T(states[1]), **{n: T(a[f]) for n, f in zip(ACTOR, ACTOR)}),
            dict(h0=T(states[2]), c0=T(states[3]), **{n: T(a[f]) for n, f in zip(ACTOR, CRITIC)})]


def seq_case(kind, pattern, L, B):
    """Inputs and the host build's forward of one case, computed once: x, es, states (h_pi, c_pi, h_vf,
    c_vf before step 0, non-zero), out = [(h, c, gates)] * 2."""
    key = (kind, pattern, L, B)
    if key not in _CASE:
        rng = np.random.default_rng(1000 * L + B)
        if kind == "golden":   # the checkpoint's own normalised obs, a different stretch per env
            g = golden()
            xn = normalize(g["obs"], g, 10.0)
            x = np.stack([np.stack([xn[(t + 7 * e) % xn.shape[0], e % xn.shape[1]] for e in range(B)]) for t in range(L)])
        else:
            x = rng.uniform(-2, 2, (L, B, 13)).astype(np.float32)
        states = tuple(rng.uniform(-0.5, 0.5, (B, 128)).astype(np.float32) for _ in range(4))
        es = start_pattern(pattern, L, B)
        out = train.lstm_seq_forward(torch.from_numpy(x), torch.from_numpy(es), net_inputs(kind, states), host=True)
        _CASE[key] = dict(x=x, es=es, states=states, out=out)
    return _CASE[key]


def host_backward(kind, case, d_h):
    """d_gates of both networks from the host build, for d_h = [d_h_pi, d_h_vf] CPU tensors."""
    nets = [dict(w_hh=n["w_hh"], c0=n["c0"], c=o[1], gates=o[2], d_h=d)
            for n, o, d in zip(net_inputs(kind, case["states"]), case["out"], d_h)]
    return train.lstm_seq_backward(torch.from_numpy(case["es"]), nets, host=True)


def d_h_for(case, seed=5):
    g = torch.Generator().manual_seed(seed)
    L, B = case["es"].shape
    return [torch.randn((L, B, 128), generator=g), torch.randn((L, B, 128), generator=g)]


# --------------------------------------------------------------------------- forward
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", WEIGHTS)
def test_host_forward_equals_successive_policy_steps(kind, pattern, B):
    pol = policy(kind)
    for L in LS:
        case = seq_case(kind, pattern, L, B)
        st = tuple(s.copy() for s in case["states"])
        for t in range(L):
            pol.host_step(case["x"][t], case["es"][t], st, seed=1, step_index=t, deterministic=True)
            for k, (net, which) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                got = case["out"][net][which][t].numpy()
                assert np.array_equal(bits(got), bits(st[k])), (L, t, agent.STATE_NAMES[k])
        assert np.isfinite(st[0]).all() and 0.0 < np.abs(st[0]).mean() < 1.0
        assert not np.array_equal(st[0], st[2])
    if pattern != "none":
        assert case["es"].any()
        if B >= 4:
            assert 0 < case["es"].any(0).sum() < B   # fresh and running envs in one tile


def tanhf_r(x):
    """ha_math.h tanhf_r over an f32 array: tanh_f64 on the library's exp_k, rounded once."""
    lib = _lib.load()
    x = np.ascontiguousarray(x, np.float64).reshape(-1)
    ax = np.abs(x)
    arg = np.ascontiguousarray(-2.0 * ax)
    e = np.empty_like(arg)
    assert lib.he_host_math(0, arg.ctypes.data, arg.size, e.ctypes.data) == 0
    t = (1.0 - e) / (1.0 + e)
    t = np.where(x < 0.0, -t, t)
    t = np.where(ax < 2.0 ** -13, x * (1.0 - (x * x) * (1.0 / 3.0)), t)
    t = np.where(ax < 20.0, t, np.sign(x))
    return t.astype(np.float32)


@pytest.mark.parametrize("kind", WEIGHTS)
def test_gates_recombine_to_c_and_h_bitwise(kind):
    for pattern, L, B in (("mid", 9, 33), ("ends", 40, 2), ("none", 2, 65), ("ends", 1, 1)):
        case = seq_case(kind, pattern, L, B)
        keep = (case["es"] == 0)[:, :, None]
        for net in range(2):
            h, c, gates = (t.numpy() for t in case["out"][net])
            i, f, g, o = (gates[:, :, k] for k in range(4))
            c_prev = np.where(keep, np.concatenate([case["states"][2 * net + 1][None], c[:-1]]), np.float32(0.0))
            fc = (f * c_prev).astype(np.float32)
            ig = (i * g).astype(np.float32)
            cn = (fc + ig).astype(np.float32)
            assert np.array_equal(bits(cn), bits(c)), (pattern, L, B, net)
            hn = (o * tanhf_r(cn).reshape(cn.shape)).astype(np.float32)
            assert np.array_equal(bits(hn), bits(h)), (pattern, L, B, net)
            assert (i > 0).all() and (i < 1).all() and (np.abs(g) <= 1).all() and np.abs(g).max() > 0.1


# --------------------------------------------------------------------------- backward against autograd
def torch_lstm_loop(x, es, h0, c0, w_ih, w_hh, b_ih, b_hh, pre_out=None):
    """sb3_contrib's _process_sequence as explicit cell equations: one step at a time, the state zeroed
    where es is set.  x [L,B,13], es [L,B] -> h [L,B,128]; pre_out collects the pre-activations."""
    h, c = h0, c0
    hs = []
    for t in range(x.shape[0]):
        keep = (es[t] == 0).to(x.dtype).unsqueeze(-1)
        h, c = h * keep, c * keep
        pre = x[t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        if pre_out is not None:
            pre.retain_grad()
            pre_out.append(pre)
        i, f, g, o = pre.chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs)


GRAD_NAMES = ("d_gates", "dW_ih", "dW_hh", "db_ih", "db_hh")


def autograd_reference(net, x, es, d_h, dtype):
    """d_gates and the four weight gradients of sum(h d_h) from torch autograd in `dtype`, as f64."""
    w = {k: net[k].to(dtype).clone().requires_grad_() for k in ("w_ih", "w_hh", "b_ih", "b_hh")}
    pres = []
    h = torch_lstm_loop(x.to(dtype), es, net["h0"].to(dtype), net["c0"].to(dtype), w["w_ih"], w["w_hh"], w["b_ih"],
                        w["b_hh"], pre_out=pres)
    (h * d_h.to(dtype)).sum().backward()
    L, B = es.shape
    dg = torch.stack([p.grad for p in pres]).reshape(L, B, 4, 128)
    return [t.to(torch.float64) for t in (dg, w["w_ih"].grad, w["w_hh"].grad, w["b_ih"].grad, w["b_hh"].grad)]


def build_grads(d_gates, net, x, es, h):
    """The build's d_gates [L,B,4,128] f32 and the weight gradients from it by f64 matmul."""
    L, B = es.shape
    f64 = torch.float64
    dg = d_gates.to(f64).reshape(L * B, 512)
    h_prev = torch.cat([net["h0"].unsqueeze(0), h[:-1]], 0).to(f64) * (es == 0).to(f64).unsqueeze(-1)
    db = dg.sum(0)
    return [d_gates.to(f64), dg.t() @ x.to(f64).reshape(L * B, 13), dg.t() @ h_prev.reshape(L * B, 128), db, db]


def grad_errors(net, x, es, d_h, d_gates, h):
    """[(name, build error, d_ref)]: the build and torch's f32 run against the f64 restatement."""
    r64 = autograd_reference(net, x, es, d_h, torch.float64)
    r32 = autograd_reference(net, x, es, d_h, torch.float32)
    got = build_grads(d_gates, net, x, es, h)
    return [(n, float((a - r).abs().max()), float((b - r).abs().max())) for n, a, b, r in zip(GRAD_NAMES, got, r32, r64)]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", WEIGHTS)
def test_host_backward_within_4_d_ref_of_f64_autograd(kind, pattern):
    # (d_ref is a maximum over the case's elements: over a handful of envs it is one draw, not a bound)
    for L, B in ((2, 33), (9, 33), (40, 65)):
        case = seq_case(kind, pattern, L, B)
        d_h = d_h_for(case)
        d_gates = host_backward(kind, case, d_h)
        x, es = torch.from_numpy(case["x"]), torch.from_numpy(case["es"])
        for k, net in enumerate(net_inputs(kind, case["states"])):
            for name, err, d_ref in grad_errors(net, x, es, d_h[k], d_gates[k], case["out"][k][0]):
                print(f"{kind} {pattern} L {L} B {B} net {k} {name}: build {err:.3e} reference {d_ref:.3e}")
                assert d_ref > 0.0 or err == 0.0   # (every step a start: dW_hh is exactly zero on both sides)
                assert err <= 4 * d_ref, (name, err, d_ref)
            assert float(d_gates[k].abs().max()) > 1e-3


# --------------------------------------------------------------------------- gradient masking
def test_no_gradient_crosses_an_episode_start():
    kind, L, B, s = "golden", 9, 2, 4
    case = dict(seq_case(kind, "none", L, B))
    es = np.zeros((L, B), np.uint8)
    es[s, 0] = 1   # env 0 starts an episode at step s, env 1 runs through
    case["es"] = es
    case["out"] = train.lstm_seq_forward(torch.from_numpy(case["x"]), torch.from_numpy(es),
                                         net_inputs(kind, case["states"]), host=True)
    d_h = d_h_for(case)
    base = host_backward(kind, case, d_h)
    bumped = [d.clone() for d in d_h]
    for d in bumped:
        d[s:] += 1.0
    moved = host_backward(kind, case, bumped)
    for a, b in zip(base, moved):
        a, b = a.numpy(), b.numpy()
        assert np.array_equal(bits(a[:s, 0]), bits(b[:s, 0]))        # cut at the start
        assert not np.array_equal(a[s:, 0], b[s:, 0])
        assert (np.abs(a[:s, 1] - b[:s, 1]) > 0).mean() > 0.5        # the running env carries it back
        assert (a[s, 0, 1] == 0.0).all()                             # c_prev = 0 at the start: no forget-gate gradient
        assert np.abs(a[s, 0, 0]).max() > 0.0


def test_single_step_with_a_start_has_a_zero_forget_gradient():
    for kind in WEIGHTS:
        case = seq_case(kind, "ends", 1, 2)   # L = 1: env 0 starts, env 1 runs on from (h0, c0)
        assert case["es"].tolist() == [[1, 0]]
        for dg in host_backward(kind, case, d_h_for(case)):
            dg = dg.numpy()
            assert (dg[0, 0, 1] == 0.0).all() and np.abs(dg[0, 1, 1]).max() > 0.0
            assert np.abs(dg[0, 0, [0, 2, 3]]).max() > 0.0


def test_autograd_function_on_the_host_build():
    kind, L, B = "random", 9, 2
    case = seq_case(kind, "mid", L, B)
    net = net_inputs(kind, case["states"])[0]
    x, es = torch.from_numpy(case["x"]), torch.from_numpy(case["es"])
    w = [net[k].clone().requires_grad_() for k in ACTOR]
    h = train.lstm_sequence(x, es, net["h0"], net["c0"], *w)
    assert np.array_equal(bits(h.detach().numpy()), bits(case["out"][0][0].numpy()))
    d_h = d_h_for(case)[0]
    (h * d_h).sum().backward()
    r64 = autograd_reference(net, x, es, d_h, torch.float64)
    r32 = autograd_reference(net, x, es, d_h, torch.float32)
    for name, p, b, r in zip(GRAD_NAMES[1:], w, r32[1:], r64[1:]):
        err, d_ref = float((p.grad.double() - r).abs().max()), float((b - r).abs().max())
        print(f"{name}: lstm_sequence {err:.3e} reference {d_ref:.3e}")
        assert err <= 4 * d_ref, (name, err, d_ref)
    # weight_grads' blocked sums: a block and a pass smaller than the case, against the plain f64 sums
    dg = host_backward(kind, case, [d_h, d_h])[0]
    want = build_grads(dg, net, x, es, case["out"][0][0])[1:]
    for kw in (dict(), dict(rows=4, block=4), dict(rows=6, block=5)):
        for a, b in zip(train.weight_grads(dg, x, case["out"][0][0], net["h0"], es, **kw), want):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    # the pair is the two single calls
    n2 = net_inputs(kind, case["states"])
    pair = train.lstm_sequence_pair(x, es, tuple(n2[0][k] for k in train.NET_INPUTS), tuple(n2[1][k] for k in train.NET_INPUTS))
    assert np.array_equal(bits(pair[0].numpy()), bits(case["out"][0][0].numpy()))
    assert np.array_equal(bits(pair[1].numpy()), bits(case["out"][1][0].numpy()))


# --------------------------------------------------------------------------- the module
def test_module_state_dict_feeds_the_policy():
    pol = policy("golden")
    m = train.RecurrentPPOModule.from_policy(pol, device="cpu")
    sd = m.state_dict()
    assert sorted(sd) == sorted(k for k, _, _ in POLICY_KEYS) and len(sd) == 21
    for k, f, shape in POLICY_KEYS:
        assert tuple(sd[k].shape) == shape and np.array_equal(sd[k].numpy(), pol._arrays[f]), k
    fresh = RecurrentPolicy.from_state_dict(policy_state_dict())
    fresh.load_state_dict({k: v + 0.25 for k, v in sd.items()})
    assert np.array_equal(fresh._arrays["c_w_hh"], pol._arrays["c_w_hh"] + np.float32(0.25))
    with pytest.raises(ValueError, match="activation"):
        train.RecurrentPPOModule(activation="gelu")
    relu = train.RecurrentPPOModule(activation="relu")
    assert isinstance(relu.mlp_extractor.policy_net[1], torch.nn.ReLU)


def test_evaluate_actions_on_the_host_build_matches_the_policy_steps():
    """values and log_prob of the stored actions against ha_host_policy_step's, within 4 x the error of
    the all-torch f32 composition against the same."""
    kind, L, B = "golden", 9, 33
    pol = policy(kind)
    case = seq_case(kind, "mid", L, B)
    st = tuple(s.copy() for s in case["states"])
    acts, vals, lps = [], [], []
    for t in range(L):
        r = pol.host_step(case["x"][t], case["es"][t], st, seed=3, step_index=t)
        acts.append(r["actions"]), vals.append(r["values"]), lps.append(r["log_probs"])
    acts, vals, lps = (torch.from_numpy(np.stack(a)) for a in (acts, vals, lps))
    m = train.RecurrentPPOModule.from_policy(pol, device="cpu")
    x, es = torch.from_numpy(case["x"]), torch.from_numpy(case["es"])
    states0 = tuple(torch.from_numpy(s) for s in case["states"])
    with torch.no_grad():
        v, lp, ent = m.evaluate_actions(x, acts, es, states0)
        nets = net_inputs(kind, case["states"])
        h_pi, h_vf = (torch_lstm_loop(x, es, *(n[k] for k in train.NET_INPUTS)) for n in nets)
        tv, tlp, _ = m.heads(h_pi, h_vf, acts)
    ev, elp = float((v - vals).abs().max()), float((lp - lps).abs().max())
    dv, dlp = float((tv - vals).abs().max()), float((tlp - lps).abs().max())
    print(f"values: module {ev:.3e} all-torch {dv:.3e}; log_prob: module {elp:.3e} all-torch {dlp:.3e}")
    assert ev <= 4 * dv and elp <= 4 * dlp
    assert v.shape == lp.shape == ent.shape == (L, B) and torch.isfinite(ent).all()
    want = float((0.5 + 0.5 * np.log(2 * np.pi) + pol._arrays["log_std"].astype(np.float64)).sum())
    assert abs(float(ent[0, 0]) - want) < 1e-5


# --------------------------------------------------------------------------- the raw ABI
def raw_nets(case, kind):
    nets = net_inputs(kind, case["states"])
    L, B = case["es"].shape
    arr = (train.HaLstmSeqNet * 2)()
    keep = []
    for k, n in enumerate(nets):
        for name in train.NET_INPUTS:
            setattr(arr[k], name, n[name].data_ptr())
        for name, shape in (("h", (L, B, 128)), ("c", (L, B, 128)), ("gates", (L, B, 4, 128))):
            t = torch.zeros(shape)
            keep.append(t)
            setattr(arr[k], name, t.data_ptr())
    return arr, keep + nets


def test_abi_argument_checks_return_the_status_codes():
    lib = agent.load()
    kind = "random"
    case = seq_case(kind, "none", 2, 2)
    x, es = torch.from_numpy(case["x"]), torch.from_numpy(case["es"])
    arr, keep = raw_nets(case, kind)
    fwd = lib.ha_host_lstm_seq_forward
    assert fwd(2, 2, 2, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_OK
    assert fwd(3, 2, 2, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert b"n_nets" in lib.ha_policy_last_error(None)
    assert fwd(0, 2, 2, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert fwd(2, 0, 2, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert fwd(2, 2, 0, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert fwd(2, 2, 2 ** 31, x.data_ptr(), es.data_ptr(), arr) == _lib.HE_ESHAPE
    assert fwd(2, 2, 2, None, es.data_ptr(), arr) == _lib.HE_EINVAL
    assert fwd(2, 2, 2, x.data_ptr(), es.data_ptr(), None) == _lib.HE_EINVAL
    bad = (train.HaLstmSeqNet * 2).from_buffer_copy(arr)
    bad[1].gates = None
    assert fwd(2, 2, 2, x.data_ptr(), es.data_ptr(), bad) == _lib.HE_EINVAL
    assert b"ha_lstm_seq_net" in lib.ha_policy_last_error(None)
    assert fwd(1, 2, 2, x.data_ptr(), es.data_ptr(), bad) == _lib.HE_OK   # the second struct is not read
    # the device entry points check before they launch: a misaligned or missing pointer never reaches a kernel
    ws = torch.zeros(16)
    dev = lib.ha_lstm_seq_forward
    assert dev(2, 2, 2, x.data_ptr(), es.data_ptr(), arr, None, None) == _lib.HE_EINVAL
    assert b"workspace" in lib.ha_policy_last_error(None)
    bad = (train.HaLstmSeqNet * 2).from_buffer_copy(arr)
    bad[0].h0 = arr[0].h0 + 4
    assert dev(2, 2, 2, x.data_ptr(), es.data_ptr(), bad, ws.data_ptr(), None) == _lib.HE_EINVAL
    assert b"aligned" in lib.ha_policy_last_error(None)
    assert dev(4, 2, 2, x.data_ptr(), es.data_ptr(), arr, ws.data_ptr(), None) == _lib.HE_ESHAPE
    barr = (train.HaLstmSeqBwd * 2)()
    assert lib.ha_host_lstm_seq_backward(2, 2, 2, es.data_ptr(), barr) == _lib.HE_EINVAL
    assert lib.ha_host_lstm_seq_backward(5, 2, 2, es.data_ptr(), barr) == _lib.HE_ESHAPE
    assert lib.ha_lstm_seq_backward(2, 2, 2, es.data_ptr(), barr, ws.data_ptr(), None) == _lib.HE_EINVAL
    assert lib.ha_lstm_seq_backward(2, 2, -1, es.data_ptr(), barr, ws.data_ptr(), None) == _lib.HE_ESHAPE
    one, two = lib.ha_lstm_seq_workspace_bytes(1), lib.ha_lstm_seq_workspace_bytes(2)
    assert one > 0 and two == 2 * one and one % 16 == 0 and lib.ha_lstm_seq_workspace_bytes(3) == 0
    # the Python layer refuses wrong shapes before the library sees them
    with pytest.raises(ValueError, match="x must be"):
        train.lstm_seq_forward(x[:, :, :12], es, net_inputs(kind, case["states"]))
    with pytest.raises(ValueError, match="w_hh"):
        n = net_inputs(kind, case["states"])
        n[0]["w_hh"] = n[0]["w_hh"][:, :64]
        train.lstm_seq_forward(x, es, n)
    with pytest.raises(ValueError, match="n_nets"):
        n = net_inputs(kind, case["states"])
        train.lstm_seq_forward(x, es, n + n[:1])


# --------------------------------------------------------------------------- the code object
def test_lstm_seq_kernels_use_no_scratch():
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
    kernels = {k: v for k, v in meta.items() if "lstm_seq_" in k}
    assert len(kernels) == 4, sorted(meta)   # forward, backward and their two packing kernels
    for k, v in kernels.items():
        assert v["scratch_B"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
    fwd = [v for k, v in kernels.items() if "lstm_seq_fwd_kernel" in k][0]
    bwd = [v for k, v in kernels.items() if "lstm_seq_bwd_kernel" in k][0]
    assert 0 < fwd["lds_B"] <= 64 * 1024, fwd
    # d_gates of 32 envs at a 33-float stride: two workgroups fit a CU's 160 KiB
    assert bwd["lds_B"] == 512 * 33 * 4 and 2 * bwd["lds_B"] <= 160 * 1024, bwd
    # two workgroups of 4 waves per CU: at most 256 registers a lane
    assert fwd["vgpr"] + fwd["agpr"] <= 256 and bwd["vgpr"] + bwd["agpr"] <= 256
    # the step kernels are what they were before the sequence kernels joined the library
    step = {n: [v for k, v in meta.items() if n in k][0] for n in ("12actor_kernel", "policy_step_kernel")}
    assert step["12actor_kernel"]["vgpr"] == 134 and step["policy_step_kernel"]["vgpr"] == 135, step
    assert all(v["scratch_B"] == 0 and v["lds_B"] == 52536 for v in step.values())
