"""ha_host_ppo_heads_forward / _backward, the host build of the PPO heads kernels (include/hedge_actor.h,
contract H1-H6; no GPU needed):

* the forward on the LSTMs' outputs of a stored sequence equals L successive ha_host_policy_step calls bit for
  bit (values, log_probs, mean_out), and the entropy equals H3 restated in NumPy f64 bit for bit;
* every row is independent of the others except in d_log_std;
* the backward, with train.heads_weight_grads' 13 weight gradients, against torch.autograd.grad of
  tests/_ppo_reference.heads in f64 within 4 x d_ref per quantity, d_ref the f32 torch run of the same
  restatement against the f64 one (no d_ref pooled); relu's masked entries are exactly +0;
* H6's sum bit for bit against L1's order restated in NumPy;
* seven deliberate mistakes in the restatement, each of which must break the agreement;
* RecurrentPPOModule(heads="kernel") against heads="torch", and ppo_update over 12 optimizer steps against the
  f64 replay of tests/_ppo_reference.py under test_ppo_replay_cpu's bound;
* the refusals, the structs' layout against the header, the four kernels' resources."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _ppo_heads_contract as hc
from cantorrl_amd import agent
from test_policy_collect_cpu import make_policy

F32, F64 = np.float32, np.float64
ACTS = ("tanh", "relu")
BACKWARD_R = (1, 2, 31, 32, 33, 65, 1025, 2051)
_POL, _REF = {}, {}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def policy(kind, act):
    if (kind, act) not in _POL:
        _POL[kind, act] = make_policy(kind, activation=act)
    return _POL[kind, act]


def tensors(kind, act="tanh"):
    return hc.policy_tensors(policy(kind, act))


def reference(kind, act, R):
    """(rows, the host build's outputs with the weight gradients, the f64 reference, d_ref), computed once."""
    key = (kind, act, R)
    if key not in _REF:
        import torch
        import _ppo_reference as ref
        from cantorrl_amd import train
        w, x = tensors(kind), hc.rows(R, seed=1000 + R)
        got = hc.host_both(w, act, x)
        t = {k: torch.from_numpy(v) for k, v in dict(x, **got).items()}
        grads = train.heads_weight_grads(t, t)
        got.update({"g_" + k: g.numpy() for k, g in zip(hc.TENSORS, grads)})
        _REF[key] = (x, got) + hc.d_refs(ref, w, act, x)
    return _REF[key]


# --------------------------------------------------------------------------- 1: the step kernel's bits
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", ("golden", "random"))
@pytest.mark.parametrize("L", (1, 9))
@pytest.mark.parametrize("B", (1, 33))
def test_forward_equals_successive_policy_steps_bitwise(B, L, kind, act):
    torch = pytest.importorskip("torch")
    from cantorrl_amd import train
    pol = policy(kind, act)
    rng = np.random.default_rng(10 * B + L)
    st = tuple(rng.uniform(-0.5, 0.5, (B, 128)).astype(F32) for _ in range(4))
    s0 = [s.copy() for s in st]
    obs = rng.uniform(-1, 1, (L, B, 13)).astype(F32)
    starts = (rng.uniform(size=(L, B)) < 0.2).astype(np.uint8)
    steps = [pol.host_step(obs[t], starts[t], st, seed=9, step_index=t) for t in range(L)]
    x = torch.from_numpy(np.stack([s["obs_norm"] for s in steps]))
    _, a = pol._host_weights()
    nets = [dict(h0=torch.from_numpy(s0[2 * k]), c0=torch.from_numpy(s0[2 * k + 1]),
                 **{n: torch.from_numpy(a[p + n]) for n in ("w_ih", "w_hh", "b_ih", "b_hh")}) for k, p in enumerate(("", "c_"))]
    (h_pi, _, _), (h_vf, _, _) = train.lstm_seq_forward(x, torch.from_numpy(starts), nets)
    assert np.array_equal(bits(h_pi[-1].numpy()), bits(st[0])) and np.array_equal(bits(h_vf[-1].numpy()), bits(st[2]))
    rows = dict(h_pi=h_pi.numpy().reshape(L * B, 128), h_vf=h_vf.numpy().reshape(L * B, 128),
                actions=np.stack([s["actions"] for s in steps]).reshape(L * B, 2))
    w = hc.policy_tensors(pol)
    status, out = hc.host_forward(w, act, rows)
    assert status == 0
    for name, step_name in (("values", "values"), ("log_prob", "log_probs"), ("mean", "mean")):
        want = np.stack([s[step_name] for s in steps]).reshape(out[name].shape)
        np.testing.assert_allclose(out[name], want, rtol=0, atol=0, err_msg=name)
        assert np.array_equal(bits(out[name]), bits(want)), name
    assert np.all(bits(out["entropy"]) == bits(hc.entropy_h3(w["log_std"])))
    assert np.isfinite(out["a1_pi"]).all() and np.isfinite(out["a2_vf"]).all()
    # the Python wrapper returns the same bits
    res = train.ppo_heads_forward(*(torch.from_numpy(rows[k]) for k in hc.FWD_IN),
                                  [torch.from_numpy(w[k]) for k in hc.TENSORS], act)
    assert tuple(res) == hc.FWD_OUT and all(np.array_equal(bits(res[k].numpy()), bits(out[k])) for k in hc.FWD_OUT)


# --------------------------------------------------------------------------- 2: rows are independent
@pytest.mark.parametrize("act", ACTS)
def test_a_row_of_a_65_row_call_is_the_one_row_call_and_a_perturbed_row_stays_alone(act):
    R = 65
    w, x = tensors("random"), hc.rows(R, seed=5)
    whole = hc.host_both(w, act, x)
    per_row = [k for k in hc.FWD_OUT + hc.BWD_OUT if k != "d_log_std"]
    for r in range(R):
        one = hc.host_both(w, act, {k: v[r:r + 1] for k, v in x.items()})
        for k in per_row:
            assert np.array_equal(bits(one[k][0]), bits(whole[k][r])), (k, r)
    r = 40
    y = dict(x, d_log_prob=x["d_log_prob"].copy())
    y["d_log_prob"][r] *= F32(1.5)
    moved = hc.host_both(w, act, y)
    for k in per_row:
        same = np.array([np.array_equal(bits(moved[k][i]), bits(whole[k][i])) for i in range(R)])
        changes = k in ("d_mean", "d_h_pi", "d_z1_pi", "d_z2_pi")
        assert same[np.arange(R) != r].all() and same[r] != changes, k
    assert not np.array_equal(bits(moved["d_log_std"]), bits(whole["d_log_std"]))


# --------------------------------------------------------------------------- 3: against autograd in f64
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("R", BACKWARD_R)
def test_backward_and_weight_gradients_within_4_d_ref_of_f64_autograd(R, act):
    pytest.importorskip("torch")
    kind = "golden" if R in (33, 1025) else "random"
    x, got, r64, d_ref = reference(kind, act, R)
    err = hc.errors(got, r64, hc.BACKWARD + hc.FORWARD)
    for k in hc.BACKWARD + hc.FORWARD:
        print(f"R {R} {act} {k}: err {err[k]:.3e} d_ref {d_ref[k]:.3e} ratio {err[k] / d_ref[k] if d_ref[k] else float('nan'):.2f}")
    for k in hc.BACKWARD:   # the forward's bits are the step kernel's (test 1): no bound of this kind is claimed there
        assert err[k] <= 4 * d_ref[k], (k, err[k], d_ref[k])
    assert all(np.abs(r64[k]).max() > 0 for k in hc.BACKWARD)
    if act == "relu":
        for net in ("pi", "vf"):
            for layer in ("1", "2"):
                a, d = got[f"a{layer}_{net}"], got[f"d_z{layer}_{net}"]
                assert np.all(bits(d)[a == 0] == 0), (net, layer)       # exactly +0, not -0
                assert 0 < np.count_nonzero(a == 0) < a.size
    # the f64 NumPy restatement is the torch reference to f64 accuracy
    want = hc.restate(tensors(kind), act, x)
    for k in hc.BACKWARD + hc.FORWARD:
        assert np.abs(want[k] - r64[k]).max() <= 1e-11 * max(1.0, np.abs(r64[k]).max()), k


# --------------------------------------------------------------------------- 4: H6's sum
@pytest.mark.parametrize("R", (255, 256, 257, 1024, 1025, 2051))
def test_d_log_std_is_l1s_sum_bitwise_on_quantised_actions(R):
    rng = np.random.default_rng(R)
    w = dict(tensors("random"), log_std=np.zeros(2, F32))                 # std = exp_k(0) = 1 exactly
    x = hc.rows(R, seed=R)
    x["mean"] = (np.round(rng.normal(0, 1, (R, 2)) * 8.0) / 8.0).astype(F32)
    x["actions"] = (x["mean"] + np.round(rng.normal(0, 1, (R, 2)) * 8.0) / 8.0).astype(F32)   # z a multiple of 1/8
    # gradients over 40 binades: the order of the additions shows
    x["d_log_prob"] = (np.round(rng.normal(0, 1, R) * 1024.0) / 1024.0 * 2.0 ** rng.integers(-20, 21, R)).astype(F32)
    x["d_entropy"] = (np.round(rng.normal(0, 1, R) * 1024.0) / 1024.0 * 2.0 ** rng.integers(-20, 21, R)).astype(F32)
    for k in ("a1_pi", "a2_pi", "a1_vf", "a2_vf"):
        x[k] = rng.uniform(-1, 1, (R, 64)).astype(F32)
    st, out = hc.host_backward(w, "tanh", x)
    assert st == 0
    want = hc.lsd_h6(x["d_log_prob"], x["d_entropy"], x["actions"], x["mean"], np.ones(2, F32))
    assert np.array_equal(bits(out["d_log_std"]), bits(want)), (out["d_log_std"], want)
    z = x["actions"].astype(F64) - x["mean"].astype(F64)
    plain = (x["d_log_prob"].astype(F64)[:, None] * (z * z - 1.0) + x["d_entropy"].astype(F64)[:, None])
    assert np.isfinite(want).all() and np.abs(plain).max() / np.abs(plain).min(initial=np.inf, where=plain != 0) > 2.0 ** 40


# --------------------------------------------------------------------------- 5: mistakes are caught
@pytest.mark.parametrize("mistake", hc.MISTAKES)
def test_each_mistake_in_the_restatement_breaks_the_agreement(mistake):
    pytest.importorskip("torch")
    act = "relu" if mistake == "relu_ge" else "tanh"
    x, got, r64, d_ref = reference("random", act, 65)
    w = tensors("random")
    assert hc.agrees(got, hc.restate(w, act, x), d_ref)
    assert not hc.agrees(got, hc.restate(w, act, x, mistake=mistake), d_ref), mistake


# --------------------------------------------------------------------------- 6: the module and the update
def test_evaluate_actions_with_kernel_heads_gives_the_torch_heads_gradients():
    torch = pytest.importorskip("torch")
    import _ppo_reference as ref
    from cantorrl_amd import train
    from test_ppo_replay_cpu import HYPER, buffer, policy as replay_policy
    pol, buf = replay_policy("random"), buffer("random", 8, 5)
    idx = torch.arange(5)
    mb = train.minibatch(buf, idx, 0, 8)
    hyper = (HYPER["clip_range"], HYPER["ent_coef"], HYPER["vf_coef"])
    grads = {}
    for heads in train.HEADS:
        m = train.RecurrentPPOModule.from_policy(pol, device="cpu", heads=heads)
        assert m.heads_mode == heads
        out = m.evaluate_actions(mb["observations"], mb["actions"], mb["episode_starts"], mb["states0"])
        assert all(o.shape == (8, 5) for o in out)
        loss, _ = train.ppo_loss(*out, mb["log_probs"], mb["advantages"], mb["returns"], *hyper)
        loss.backward()
        grads[heads] = {k: p.grad.detach().double() for k, p in m.named_parameters()}
    p64 = {k: v.requires_grad_() for k, v in ref.parameters(m, torch.float64).items()}
    out = ref.evaluate(p64, ref.constants(pol), mb["observations"], mb["actions"], mb["episode_starts"], mb["states0"])
    loss, _ = ref.loss(*out, mb["log_probs"].double(), mb["advantages"].double(), mb["returns"].double(), *hyper)
    g64 = dict(zip(p64, torch.autograd.grad(loss, list(p64.values()))))
    assert len(g64) == 21
    for k in g64:
        err = float((grads["kernel"][k] - grads["torch"][k]).abs().max())
        d_ref = float((grads["torch"][k] - g64[k]).abs().max())
        ulp = float(np.spacing(F32(float(g64[k].abs().max()))))
        print(f"{k}: kernel - torch {err:.3e} d_ref {d_ref:.3e} ulp {ulp:.3e}")
        assert err <= 4 * d_ref + ulp, (k, err, d_ref, ulp)
    for bad in ("x", None):
        with pytest.raises(ValueError, match="heads must be"):
            train.RecurrentPPOModule(heads=bad)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    assert train.RecurrentPPOModule.from_state_dict(sd, heads="kernel").heads_mode == "kernel"
    assert train.RecurrentPPOModule.from_state_dict(sd).heads_mode == "torch"


@pytest.mark.parametrize("optimizer", ("adam", "sgd"))
@pytest.mark.parametrize("kind", ("golden", "random"))
def test_ppo_update_with_kernel_heads_lands_where_the_f64_replay_lands(kind, optimizer):
    torch = pytest.importorskip("torch")
    import _ppo_reference as ref
    from cantorrl_amd import train
    from test_ppo_replay_cpu import EPOCHS, HYPER, OPTIMIZERS, PERM_SEED, STEPS, buffer, policy as replay_policy, replays
    shape = (8, 5, 2, 4)
    K, n, per, W = shape
    p0, p32, p64, trace = replays(kind, shape, optimizer)
    assert len(trace) == STEPS
    ref.check_replay_inputs(trace, HYPER["clip_range"], need_clipping=(kind, optimizer) != ("random", "sgd"))
    m = train.RecurrentPPOModule.from_policy(replay_policy(kind), device="cpu", heads="kernel")
    lr = OPTIMIZERS[optimizer]
    opt = torch.optim.SGD(m.parameters(), lr=lr) if optimizer == "sgd" else train.DeviceAdam(m.parameters(), lr=lr, eps=1e-5)
    train.ppo_update(m, opt, buffer(kind, K, n), n_epochs=EPOCHS, envs_per_batch=per, window=W,
                     generator=torch.Generator().manual_seed(PERM_SEED), **HYPER)
    got = dict(m.named_parameters())
    for k, err, d_ref, ulp in ref.replay_bound(p0, p32, p64, got):
        print(f"{k}: err {err:.3e} d_ref {d_ref:.3e} ulp {ulp:.3e} ratio {err / (4 * d_ref + ulp):.2f}")
        assert float((got[k].detach().double() - p0[k]).abs().max()) > 0.0, k
        assert err <= 4 * d_ref + ulp, (k, err, d_ref, ulp)


def test_ppo_heads_is_differentiable_in_h_and_the_13_tensors_and_exported():
    torch = pytest.importorskip("torch")
    import cantorrl_amd
    from cantorrl_amd import train
    for name in ("ppo_heads", "ppo_heads_forward", "ppo_heads_backward", "heads_weight_grads"):
        assert getattr(cantorrl_amd, name) is getattr(train, name)
    x, got, r64, d_ref = reference("random", "tanh", 65)
    w = [torch.from_numpy(v.copy()).requires_grad_() for v in tensors("random").values()]
    h_pi, h_vf = (torch.from_numpy(x[k]).reshape(5, 13, 128).requires_grad_() for k in ("h_pi", "h_vf"))
    actions = torch.from_numpy(x["actions"]).reshape(5, 13, 2).requires_grad_()
    out = train.ppo_heads(h_pi, h_vf, actions, *w, activation="tanh")
    assert all(o.shape == (5, 13) and o.requires_grad for o in out)
    torch.autograd.backward(list(out), [torch.from_numpy(x[k]).reshape(5, 13) for k in ("d_values", "d_log_prob", "d_entropy")])
    assert actions.grad is None
    assert np.array_equal(bits(h_pi.grad.numpy().reshape(65, 128)), bits(got["d_h_pi"]))
    assert np.array_equal(bits(h_vf.grad.numpy().reshape(65, 128)), bits(got["d_h_vf"]))
    for k, t in zip(hc.TENSORS, w):
        assert np.array_equal(bits(t.grad.numpy()), bits(got["g_" + k])), k


# --------------------------------------------------------------------------- 7: refusals
def test_entry_points_refuse_bad_arguments_and_leave_the_outputs_untouched():
    torch = pytest.importorskip("torch")
    from cantorrl_amd import train
    lib = agent.load()
    err = lambda: lib.ha_policy_last_error(None)
    w, x = tensors("random"), hc.rows(3, seed=2)
    st, f = hc.host_forward(w, "tanh", x)
    assert st == 0
    xb = dict(x, **f)

    def refused(status, word, backward=False, **kw):
        ww, act = kw.pop("w", w), kw.pop("activation", "tanh")
        xx = kw.pop("x", xb if backward else x)
        st, out = (hc.host_backward if backward else hc.host_forward)(ww, act, xx, fill=7.0, **kw)
        assert st == status and word in err(), (st, err(), kw)
        assert all(np.all(a == 7.0) for a in out.values())

    for backward in (False, True):
        refused(2, b"n_rows", backward, n_rows=0)                                     # HE_ESHAPE
        refused(2, b"n_rows", backward, n_rows=hc.MAX_ROWS + 1)
        refused(1, b"activation", backward, activation=2)                             # HE_EINVAL
        refused(1, b"NULL", backward, w=dict(w, v2=None))
        refused(1, b"NULL", backward, w=dict(w, log_std=None))
        refused(1, b"NULL", backward, x=dict(xb if backward else x, actions=None))
        refused(1, b"aligned", backward, extra={"d_mean" if backward else "mean": x["actions"].ctypes.data + 2})
    refused(1, b"NULL", True, x=dict(xb, a2_vf=None))
    refused(1, b"NULL", False, extra={"values": None})
    assert lib.ha_host_ppo_heads_forward(3, None, None) == 1 and lib.ha_host_ppo_heads_backward(3, None, None) == 1
    # the device calls check before any launch (no GPU here): shape, 16-byte alignment, the workspace
    ws, io = hc.Weights(*([x["h_pi"].ctypes.data] * 13), 0), hc.Fwd(*([x["h_pi"].ctypes.data] * 11))
    bio = hc.Bwd(*([x["h_pi"].ctypes.data] * 17))
    assert x["h_pi"].ctypes.data % 16 == 0
    for fn, s in ((lib.ha_ppo_heads_forward, io), (lib.ha_ppo_heads_backward, bio)):
        assert fn(0, ctypes.byref(ws), ctypes.byref(s), None, None) == 2
        assert fn(3, ctypes.byref(ws), ctypes.byref(s), None, None) == 1 and b"workspace" in err()
        assert fn(3, ctypes.byref(ws), ctypes.byref(s), ctypes.c_void_p(8), None) == 1 and b"workspace" in err()
        s.a1_pi = x["h_pi"].ctypes.data + 4
        assert fn(3, ctypes.byref(ws), ctypes.byref(s), ctypes.c_void_p(16), None) == 1 and b"16-byte" in err()
    size = lib.ha_ppo_heads_workspace_bytes
    base = size(1) - 16
    assert [size(n) for n in (0, 1, 1024, 1025, hc.MAX_ROWS, hc.MAX_ROWS + 1)] == \
        [0, base + 16, base + 16, base + 32, base + 16 * 4096, 0]
    assert base == 4 * (2 * (2 * 64 * 128 + 2 * 64 * 64) + 4)
    # the wrappers raise ValueError with the library's message
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    tw = [torch.from_numpy(v) for v in w.values()]
    with pytest.raises(ValueError, match="n_rows"):
        train.ppo_heads_forward(t["h_pi"][:0], t["h_vf"][:0], t["actions"][:0], tw)
    with pytest.raises(ValueError, match="activation"):
        train.ppo_heads_forward(t["h_pi"], t["h_vf"], t["actions"], tw, "gelu")
    with pytest.raises(ValueError, match="float32"):
        train.ppo_heads_forward(t["h_pi"].double(), t["h_vf"], t["actions"], tw)
    with pytest.raises(ValueError, match="13"):
        train.ppo_heads_forward(t["h_pi"], t["h_vf"], t["actions"], tw[:12])


# --------------------------------------------------------------------------- the structs and the kernels
def test_python_mirrors_of_the_heads_structs_match_the_header(tmp_path):
    pytest.importorskip("torch")
    from cantorrl_amd import train
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler (cc, gcc, clang) on the path")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    mirrors = (("ha_ppo_heads_weights", train.HaPpoHeadsWeights, hc.Weights), ("ha_ppo_heads_fwd", train.HaPpoHeadsFwd, hc.Fwd),
               ("ha_ppo_heads_bwd", train.HaPpoHeadsBwd, hc.Bwd))
    lines = []
    for cname, mirror, _ in mirrors:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        lines += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hedge_actor.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", include, "-o", str(tmp_path / "abi"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.split()
    want = []
    for _, mirror, twin in mirrors:
        layout = [ctypes.sizeof(mirror)] + [getattr(mirror, f[0]).offset for f in mirror._fields_]
        assert [f[0] for f in mirror._fields_] == [f[0] for f in twin._fields_]
        assert layout == [ctypes.sizeof(twin)] + [getattr(twin, f[0]).offset for f in twin._fields_]
        want += layout
    assert [int(v) for v in out] == want
    assert train.HEADS_TENSORS == hc.TENSORS


def test_heads_kernels_appear_once_each_and_use_no_scratch():
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
    for name in ("heads_pack_kernel", "heads_fwd_kernel", "heads_bwd_kernel", "heads_lsd_kernel"):
        found = [v for k, v in meta.items() if name in k]
        assert len(found) == 1, (name, sorted(meta))
        assert found[0]["scratch_B"] == 0 and found[0]["vgpr_spill"] == 0 and found[0]["sgpr_spill"] == 0, (name, found[0])
    # two workgroups a CU: the two tile kernels stay within half the LDS and half the registers
    for name in ("heads_fwd_kernel", "heads_bwd_kernel"):
        row = [v for k, v in meta.items() if name in k][0]
        assert row["lds_B"] <= 80 * 1024 and row["vgpr"] + row["agpr"] <= 256, (name, row)
