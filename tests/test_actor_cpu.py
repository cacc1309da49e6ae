"""RecurrentActor on the CPU (no GPU needed): ha_host_step -- the device kernel's arithmetic
compiled for the host -- against the golden recorded from the reference's own actor
(tests/golden/ag_lossabs_final.npz, tools/golden/make_golden_actor.py), the bitwise parts of the
arithmetic contract (include/hedge_actor.h), the loaders, and the built library.

Tolerance of the golden comparison: measured, not chosen.  d_ref = max |reference f32 - f64
restatement| over the golden, separately for actions and h; the build has to stay within
4 x d_ref of the same f64 restatement (two valid f32 summation orders differ by a small factor
over a 300-step recurrence)."""
import importlib.util
import io
import os
import re
import shutil
import tempfile
import zipfile

import numpy as np
import pytest

from cantorrl_amd import agent
from cantorrl_amd.agent import ACTOR_KEYS, RecurrentActor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ag_lossabs_final.npz")
# flavour -> (activation, squash, clip_obs, golden prefix)
FLAVOURS = {"sb3": ("tanh", "clip", 10.0), "ref": ("relu", "tanh", None)}


def golden():
    return np.load(GOLDEN)


def state_dict(g):
    return {k: g[k.replace(".", "__")] for k, _, _ in ACTOR_KEYS}


def make_actor(g, flavour, sd=None, norm=True):
    act, sq, clip = FLAVOURS[flavour]
    stats = {"obs_mean": g["obs_mean"], "obs_var": g["obs_var"]} if norm else None
    return RecurrentActor.from_state_dict(sd or state_dict(g), normalization=stats, clip_obs=clip, activation=act,
                                          squash=sq)


def normalize(obs, g, clip):
    z = (obs.astype(np.float64) - g["obs_mean"]) / np.sqrt(g["obs_var"] + 1e-8)
    if clip is not None:
        z = np.clip(z, -clip, clip)
    return z.astype(np.float32)


def f64_sequence(g, flavour):
    """The contract in f64 NumPy over the golden's sequence: actions [T,N,2], h [T,N,128]."""
    act, sq, clip = FLAVOURS[flavour]
    sd = {k: v.astype(np.float64) for k, v in state_dict(g).items()}
    x_all = normalize(g["obs"], g, clip).astype(np.float64)
    T, N = g["episode_start"].shape
    h = np.zeros((N, 128))
    c = np.zeros((N, 128))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    f = np.tanh if act == "tanh" else (lambda v: np.maximum(v, 0.0))
    A, H = [], []
    for t in range(T):
        keep = 1.0 - g["episode_start"][t].astype(np.float64)[:, None]
        h, c = h * keep, c * keep
        pre = (sd["lstm_actor.bias_ih_l0"] + sd["lstm_actor.bias_hh_l0"] + x_all[t] @ sd["lstm_actor.weight_ih_l0"].T
               + h @ sd["lstm_actor.weight_hh_l0"].T)
        i, fg, gg, o = (pre[:, k * 128:(k + 1) * 128] for k in range(4))
        c = sig(fg) * c + sig(i) * np.tanh(gg)
        h = sig(o) * np.tanh(c)
        a = f(h @ sd["mlp_extractor.policy_net.0.weight"].T + sd["mlp_extractor.policy_net.0.bias"])
        a = f(a @ sd["mlp_extractor.policy_net.2.weight"].T + sd["mlp_extractor.policy_net.2.bias"])
        m = a @ sd["action_net.weight"].T + sd["action_net.bias"]
        A.append(np.clip(np.tanh(m) if sq == "tanh" else m, -1.0, 1.0))
        H.append(h)
    return np.stack(A), np.stack(H)


def host_sequence(g, flavour):
    actor = make_actor(g, flavour)
    T, N = g["episode_start"].shape
    h = np.zeros((N, 128), np.float32)
    c = np.zeros((N, 128), np.float32)
    A, H = [], []
    for t in range(T):
        A.append(actor.host_step(g["obs"][t], g["episode_start"][t], h, c))
        H.append(h.copy())
    return np.stack(A), np.stack(H)


_F64 = {}


def f64_cached(g, flavour):
    if flavour not in _F64:
        _F64[flavour] = f64_sequence(g, flavour)
    return _F64[flavour]


def d_ref(g, flavour):
    """(d_ref actions, d_ref h): the reference's own f32 error against the f64 restatement."""
    A64, H64 = f64_cached(g, flavour)
    hs = g["h_steps"]
    return (float(np.abs(g[flavour + "_actions"] - A64).max()), float(np.abs(g[flavour + "_h"] - H64[hs]).max()))


@pytest.mark.parametrize("flavour", ["sb3", "ref"])
def test_host_step_matches_golden_within_4_d_ref(flavour):
    g = golden()
    A64, H64 = f64_cached(g, flavour)
    da, dh = d_ref(g, flavour)
    A, H = host_sequence(g, flavour)
    ea, eh = float(np.abs(A - A64).max()), float(np.abs(H - H64).max())
    print(f"{flavour}: actions build {ea:.3e} reference {da:.3e}; h build {eh:.3e} reference {dh:.3e}")
    assert 0.0 < da < 1e-5 and 0.0 < dh < 1e-5   # the golden is the f32 reference, not the restatement
    assert ea <= 4 * da, (ea, da)
    assert eh <= 4 * dh, (eh, dh)
    assert g["episode_start"][252].all() and g["episode_start"].sum() == 2 * 16   # the boundary is inside


@pytest.mark.parametrize("clip", [10.0, None])
def test_obs_normalisation_is_the_numpy_expression_bitwise(clip):
    g = golden()
    obs = g["obs"][:40].reshape(-1, 13).copy()
    # rows pushed beyond +-10 sigma, both signs
    sd = np.sqrt(g["obs_var"] + 1e-8)
    obs[3] = (g["obs_mean"] + 25.0 * sd).astype(np.float32)
    obs[4] = (g["obs_mean"] - 1e3 * sd).astype(np.float32)
    obs[5, ::2] = (g["obs_mean"] + 10.0 * sd).astype(np.float32)[::2]
    n = obs.shape[0]
    actor = RecurrentActor.from_state_dict(state_dict(g), normalization={"obs_mean": g["obs_mean"], "obs_var": g["obs_var"]},
                                           clip_obs=clip)
    out = np.empty((n, 13), np.float32)
    actor.host_step(obs, np.ones(n, np.uint8), np.zeros((n, 128), np.float32), np.zeros((n, 128), np.float32),
                    obs_norm_out=out)
    want = normalize(obs, g, clip)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    if clip is not None:
        assert np.abs(want[3]).max() == 10.0 and np.abs(want[4]).max() == 10.0
    else:
        assert np.abs(want[4]).max() > 100.0


def test_episode_start_restarts_the_state_bitwise():
    g = golden()
    actor = make_actor(g, "sb3")
    rng = np.random.default_rng(5)
    n = 6
    obs = g["obs"][7, :n]
    h0 = rng.uniform(-1, 1, (n, 128)).astype(np.float32)
    c0 = rng.uniform(-2, 2, (n, 128)).astype(np.float32)
    start = np.array([1, 0, 1, 0, 0, 1], np.uint8)
    h, c = h0.copy(), c0.copy()
    h[start == 1] = np.nan   # garbage where the state restarts
    c[start == 1] = 1e30
    a = actor.host_step(obs, start, h, c)
    # from zeros
    hz, cz = np.zeros_like(h0), np.zeros_like(c0)
    az = actor.host_step(obs, np.zeros(n, np.uint8), hz, cz)
    # every row alone, with its own state
    for e in range(n):
        he, ce = h0[e:e + 1].copy(), c0[e:e + 1].copy()
        ae = actor.host_step(obs[e:e + 1], start[e:e + 1], he, ce)
        assert np.array_equal(ae[0], a[e]) and np.array_equal(he[0], h[e]) and np.array_equal(ce[0], c[e])
    s = start == 1
    assert np.array_equal(a[s], az[s]) and np.array_equal(h[s], hz[s]) and np.array_equal(c[s], cz[s])
    assert not np.array_equal(a[~s], az[~s])


def test_loaders_round_trip_and_refuse_other_architectures(tmp_path):
    import torch
    g = golden()
    sd = {k: torch.from_numpy(v.copy()) for k, v in state_dict(g).items()}
    full = dict(sd)
    for k in list(sd):   # the critic's keys, as the checkpoint has them
        if k.startswith("lstm_actor."):
            full[k.replace("lstm_actor", "lstm_critic")] = torch.zeros_like(sd[k])
    full["mlp_extractor.value_net.0.weight"] = torch.zeros(64, 128)
    full["value_net.weight"] = torch.zeros(1, 64)
    path = tmp_path / "model.zip"
    buf = io.BytesIO()
    torch.save(full, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("data", "{}")
    import pickle
    pk = tmp_path / "normalization_stats.pkl"
    with open(pk, "wb") as f:
        pickle.dump({"obs_mean": g["obs_mean"], "obs_var": g["obs_var"]}, f)
    a = RecurrentActor.from_sb3_zip(path, normalization=str(pk))
    b = make_actor(g, "sb3")
    obs, start = g["obs"][0], g["episode_start"][0]
    outs = []
    for actor in (a, b):
        h, c = np.zeros((16, 128), np.float32), np.zeros((16, 128), np.float32)
        outs.append((actor.host_step(obs, start, h, c), h))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert a.clip_obs == 10.0 and a.activation == "tanh" and a.squash == "clip"

    two = dict(sd)
    two["lstm_actor.weight_ih_l1"] = torch.zeros(512, 128)
    with pytest.raises(ValueError, match="n_lstm_layers"):
        RecurrentActor.from_state_dict(two)
    small = dict(sd)
    small["lstm_actor.weight_ih_l0"] = torch.zeros(256, 13)
    small["lstm_actor.weight_hh_l0"] = torch.zeros(256, 64)
    small["lstm_actor.bias_ih_l0"] = torch.zeros(256)
    small["lstm_actor.bias_hh_l0"] = torch.zeros(256)
    small["mlp_extractor.policy_net.0.weight"] = torch.zeros(64, 64)
    with pytest.raises(ValueError, match="128"):
        RecurrentActor.from_state_dict(small)
    obs12 = dict(sd)
    obs12["lstm_actor.weight_ih_l0"] = torch.zeros(512, 12)
    with pytest.raises(ValueError, match="13"):
        RecurrentActor.from_state_dict(obs12)
    with pytest.raises(ValueError):
        RecurrentActor.from_state_dict(sd, activation="gelu")


def test_abi_refuses_other_shapes():
    """The C entry points check the shapes themselves (HE_ESHAPE), whatever the binding did."""
    import ctypes
    g = golden()
    actor = make_actor(g, "sb3")
    w = agent.HaWeights.from_buffer_copy(actor._w)
    w.n_lstm_layers = 2
    n = 1
    z = np.zeros((n, 128), np.float32)
    o = np.zeros((n, 13), np.float32)
    a = np.zeros((n, 2), np.float32)
    es = np.ones(n, np.uint8)
    st = actor.lib.ha_host_step(ctypes.byref(w), n, o.ctypes.data, es.ctypes.data, z.ctypes.data, z.ctypes.data,
                                a.ctypes.data, None, None)
    assert st == 2 and b"n_lstm_layers" in actor.lib.ha_last_error(None)
    w = agent.HaWeights.from_buffer_copy(actor._w)
    w.hidden = 64
    assert actor.lib.ha_host_step(ctypes.byref(w), n, o.ctypes.data, es.ctypes.data, z.ctypes.data, z.ctypes.data,
                                  a.ctypes.data, None, None) == 2


def header_symbols():
    src = open(os.path.join(ROOT, "include", "hedge_actor.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ha_[a-z_]+)\s*\(", src)))


def test_library_exports_every_header_symbol_and_is_gfx950():
    lib = agent.load()
    syms = header_symbols()
    assert len(syms) >= 7, syms
    for s in syms:
        assert hasattr(lib, s), f"libhedgeactor does not export {s}"
    assert set(syms) == set(agent.EXPORTS)
    assert b"gfx950" in lib.ha_version()
    assert b"gfx950" in open(agent.LIB_PATH, "rb").read()
    # hedge_env.h's symbol set is untouched: nothing of the actor is an he_* entry point
    env_h = open(os.path.join(ROOT, "include", "hedge_env.h")).read()
    assert "ha_" not in env_h


def test_actor_kernels_use_no_scratch():
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
    kernels = {k: v for k, v in meta.items() if "actor_kernel" in k or "accumulate_kernel" in k}
    assert len(kernels) == 2, sorted(meta)
    for k, v in kernels.items():
        assert v["scratch_B"] == 0 and v["vgpr_spill"] == 0, (k, v)
    ak = [v for k, v in kernels.items() if "actor_kernel" in k][0]
    assert ak["lds_B"] <= 64 * 1024, ak
