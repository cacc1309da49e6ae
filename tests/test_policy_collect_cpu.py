"""RecurrentPolicy on the CPU (no GPU needed): ha_host_policy_step / ha_host_gae -- the device
kernels' arithmetic compiled for the host -- against the critic golden
(tests/golden/cr_lossabs_final.npz, tools/golden/make_golden_critic.py), the actor's host build,
the Philox oracle, torch's Normal and the literal NumPy GAE loop of the contract
(include/hedge_actor.h, P1-P7); the loaders, the raw ABI and the built code object.

Tolerance of the golden comparison, as test_actor_cpu.py: d_ref = max |torch f32 golden - f64
restatement|, and the build has to stay within 4 x d_ref of the same restatement."""
import ctypes
import importlib.util
import os
import shutil
import tempfile

import numpy as np
import pytest

from cantorrl_amd import agent
from cantorrl_amd.agent import CRITIC_KEYS, POLICY_KEYS, RecurrentActor, RecurrentPolicy
from test_actor_cpu import golden, normalize, state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRITIC_GOLDEN = os.path.join(ROOT, "tests", "golden", "cr_lossabs_final.npz")
HALF_LOG_2PI = 0.9189385332046727


def critic_golden():
    return np.load(CRITIC_GOLDEN)


def policy_state_dict(g=None, c=None):
    g = golden() if g is None else g
    c = critic_golden() if c is None else c
    sd = state_dict(g)
    sd.update({k: c[k.replace(".", "__")] for k, _, _ in CRITIC_KEYS})
    return sd


def random_policy_weights(seed):
    """Uniform +-0.5 tensors, log_std in +-0.5."""
    rng = np.random.default_rng(seed)
    return {f: rng.uniform(-0.5, 0.5, shape).astype(np.float32) for _, f, shape in POLICY_KEYS}


def make_policy(kind="golden", norm=True, **kw):
    if kind == "golden":
        g = golden()
        stats = {"obs_mean": g["obs_mean"], "obs_var": g["obs_var"]} if norm else None
        return RecurrentPolicy.from_state_dict(policy_state_dict(g), normalization=stats, **kw)
    rng = np.random.default_rng(99)
    return RecurrentPolicy(random_policy_weights(7), obs_mean=rng.uniform(-1, 1, 13), obs_var=rng.uniform(4, 36, 13),
                           **kw)


def zero_states(n):
    return tuple(np.zeros((n, 128), np.float32) for _ in range(4))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


# --------------------------------------------------------------------------- values against the golden
def critic_f64_sequence(g, c):
    """Contract P2 in f64 NumPy over the golden's sequence: values [T,N], h [T,N,128]."""
    sd = {k: c[k.replace(".", "__")].astype(np.float64) for k, _, _ in CRITIC_KEYS}
    x_all = normalize(g["obs"], g, 10.0).astype(np.float64)
    T, N = g["episode_start"].shape
    h = np.zeros((N, 128))
    cc = np.zeros((N, 128))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    V, H = [], []
    for t in range(T):
        keep = 1.0 - g["episode_start"][t].astype(np.float64)[:, None]
        h, cc = h * keep, cc * keep
        pre = (sd["lstm_critic.bias_ih_l0"] + sd["lstm_critic.bias_hh_l0"] + x_all[t] @ sd["lstm_critic.weight_ih_l0"].T
               + h @ sd["lstm_critic.weight_hh_l0"].T)
        i, fg, gg, o = (pre[:, k * 128:(k + 1) * 128] for k in range(4))
        cc = sig(fg) * cc + sig(i) * np.tanh(gg)
        h = sig(o) * np.tanh(cc)
        a = np.tanh(h @ sd["mlp_extractor.value_net.0.weight"].T + sd["mlp_extractor.value_net.0.bias"])
        a = np.tanh(a @ sd["mlp_extractor.value_net.2.weight"].T + sd["mlp_extractor.value_net.2.bias"])
        V.append((a @ sd["value_net.weight"].T + sd["value_net.bias"])[:, 0])
        H.append(h)
    return np.stack(V), np.stack(H)


_F64 = {}


def critic_f64_cached():
    if not _F64:
        _F64["v"], _F64["h"] = critic_f64_sequence(golden(), critic_golden())
    return _F64["v"], _F64["h"]


def critic_d_ref():
    """(d_ref values, d_ref h): torch's own f32 error against the f64 restatement."""
    c = critic_golden()
    V64, H64 = critic_f64_cached()
    return float(np.abs(c["values"] - V64).max()), float(np.abs(c["critic_h"] - H64[c["h_steps"]]).max())


def test_host_values_match_golden_within_4_d_ref():
    g, c = golden(), critic_golden()
    V64, H64 = critic_f64_cached()
    dv, dh = critic_d_ref()
    pol = make_policy()
    T, N = g["episode_start"].shape
    st = zero_states(N)
    V, H = [], []
    for t in range(T):
        V.append(pol.host_step(g["obs"][t], g["episode_start"][t], st, seed=1, step_index=t, deterministic=True)["values"])
        H.append(st[2].copy())
    ev, eh = float(np.abs(np.stack(V) - V64).max()), float(np.abs(np.stack(H) - H64).max())
    print(f"values build {ev:.3e} reference {dv:.3e}; critic h build {eh:.3e} reference {dh:.3e}")
    assert 0.0 < dv < 1e-5 and 0.0 < dh < 1e-5   # the golden is torch's f32 run, not the restatement
    assert ev <= 4 * dv, (ev, dv)
    assert eh <= 4 * dh, (eh, dh)
    assert c["values"].shape == (300, 16) and c["critic_h"].shape == (len(c["h_steps"]), 16, 128)
    assert "RESTATED" in str(c["doc"])


# --------------------------------------------------------------------------- the actor half
def test_deterministic_step_is_the_actor_bitwise():
    g = golden()
    pol = make_policy()
    actor = RecurrentActor.from_state_dict(state_dict(g), normalization={"obs_mean": g["obs_mean"], "obs_var": g["obs_var"]})
    n = 16
    st = zero_states(n)
    h, c = np.zeros((n, 128), np.float32), np.zeros((n, 128), np.float32)
    for t in (0, 1, 2, 251, 252, 253):
        obs, start = g["obs"][t], g["episode_start"][t]
        mean = np.empty((n, 2), np.float32)
        xn = np.empty((n, 13), np.float32)
        act = actor.host_step(obs, start, h, c, mean_out=mean, obs_norm_out=xn)
        r = pol.host_step(obs, start, st, seed=3, step_index=t, deterministic=True)
        assert np.array_equal(bits(r["actions"]), bits(mean)) and np.array_equal(bits(r["mean"]), bits(mean))
        assert np.array_equal(bits(r["env_actions"]), bits(act))
        assert np.array_equal(bits(r["obs_norm"]), bits(xn))
        assert np.array_equal(bits(st[0]), bits(h)) and np.array_equal(bits(st[1]), bits(c))
        # deterministic: z = 0, so the log-probability is -sum(log_std) - log(2 pi)
        want = np.float32(-np.float64(g["log_std"]).sum() - 2 * HALF_LOG_2PI)
        assert np.all(np.abs(r["log_probs"] - want) <= ulp32(want))
    assert np.abs(st[0]).mean() > 0.0 and np.abs(st[2]).mean() > 0.0 and not np.array_equal(st[0], st[2])


# --------------------------------------------------------------------------- sampling and the log-probability
SAMPLING_CASES = [(0, 0), (5, 7), (1000003, 2 ** 32 + 5), (2 ** 33 + 1, 2 ** 40)]   # (env_id_offset, step_index)


def sampled(kind, n, off, step, seed=0x9E3779B97F4A7C15):
    g = golden()
    pol = make_policy(kind)
    rng = np.random.default_rng(n + off % 1000)
    obs = g["obs"][3, :1].repeat(n, 0) + rng.normal(0, 0.01, (n, 13)).astype(np.float32) if kind == "golden" \
        else rng.uniform(-10, 10, (n, 13)).astype(np.float32)
    st = zero_states(n)
    r = pol.host_step(obs, np.ones(n, np.uint8), st, seed=seed, step_index=step, env_id_offset=off)
    return pol, obs, r, seed


@pytest.mark.parametrize("kind", ["golden", "random"])
@pytest.mark.parametrize("off,step", SAMPLING_CASES)
def test_sampling_matches_the_philox_oracle(kind, off, step):
    from oracle.hedging_oracle import philox_normals
    n = 33
    pol, obs, r, seed = sampled(kind, n, off, step)
    z0, z1 = philox_normals(seed, off + np.arange(n), step)
    z = np.stack([z0, z1], 1)
    log_std = pol._arrays["log_std"]
    std = np.exp(log_std.astype(np.float64)).astype(np.float32).astype(np.float64)
    mean = r["mean"].astype(np.float64)
    want = mean + std * z
    err = np.abs(r["actions"].astype(np.float64) - want)
    scale = np.maximum(np.maximum(np.abs(r["actions"]), np.abs(r["mean"])), np.abs(std * z).astype(np.float32))
    print(f"{kind} off {off} step {step}: max err / ulp {float((err / ulp32(scale)).max()):.3f}")
    assert np.all(err <= 2 * ulp32(scale))
    assert np.array_equal(bits(r["env_actions"]), bits(np.clip(r["actions"], -1.0, 1.0)))
    assert np.abs(z).max() > 1.0 and np.abs(r["actions"] - r["mean"]).max() > 0.0   # noise was drawn
    if kind == "random":
        assert (np.abs(r["actions"]) > 1.0).any()   # the clip is exercised

    # the log-probability: torch's Normal in f64, rounded once; within 1 f32 ulp
    import torch
    a64 = torch.from_numpy(r["actions"].astype(np.float64))
    ref = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(std)).log_prob(a64).sum(-1)
    ref32 = ref.numpy().astype(np.float32)
    d = np.abs(r["log_probs"].astype(np.float64) - ref32.astype(np.float64))
    print(f"log_prob: max |d| / ulp {float((d / ulp32(ref32)).max()):.3f}; range {ref32.min():.3f} .. {ref32.max():.3f}")
    assert np.isfinite(r["log_probs"]).all()
    assert np.all(d <= ulp32(ref32))


def test_split_calls_give_the_bits_of_one_call():
    n, off, step = 33, 11, 2 ** 32 + 9
    pol, obs, whole, seed = sampled("golden", n, off, step)
    parts = []
    for lo, hi in ((0, 16), (16, 33)):
        st = zero_states(hi - lo)
        parts.append(pol.host_step(obs[lo:hi], np.ones(hi - lo, np.uint8), st, seed=seed, step_index=step,
                                   env_id_offset=off + lo))
    for k in whole:
        assert np.array_equal(bits(np.concatenate([p[k] for p in parts])), bits(whole[k])), k
    # and a different seed, step or offset is a different draw
    for kw in (dict(seed=seed + 1, step_index=step, env_id_offset=off), dict(seed=seed, step_index=step + 1, env_id_offset=off),
               dict(seed=seed, step_index=step, env_id_offset=off + 1)):
        other = pol.host_step(obs, np.ones(n, np.uint8), zero_states(n), **kw)
        assert not np.array_equal(other["actions"], whole["actions"])
        assert np.array_equal(bits(other["values"]), bits(whole["values"]))


def test_log_prob_is_finite_for_the_checkpoint_log_std():
    g = golden()
    assert np.allclose(g["log_std"], [-3.73, -3.48], atol=0.01)
    pol, obs, r, _ = sampled("golden", 257, 0, 1)
    assert np.isfinite(r["log_probs"]).all() and r["log_probs"].max() < 5.4   # -sum(log_std) - log(2 pi) = 5.37


@pytest.mark.parametrize("deterministic", [False, True])
def test_write_state_false_changes_no_state(deterministic):
    g = golden()
    pol = make_policy()
    n = 16
    st = zero_states(n)
    pol.host_step(g["obs"][0], g["episode_start"][0], st, seed=5, step_index=0)
    pol.host_step(g["obs"][1], g["episode_start"][1], st, seed=5, step_index=1)
    assert all(np.abs(s).mean() > 0.0 for s in st)
    start = np.array([0, 1] * 8, np.uint8)
    keep = tuple(s.copy() for s in st)
    dry = pol.host_step(g["obs"][2], start, st, seed=5, step_index=2, deterministic=deterministic, write_state=False)
    for s, k in zip(st, keep):
        assert np.array_equal(bits(s), bits(k))
    copies = tuple(s.copy() for s in st)
    wet = pol.host_step(g["obs"][2], start, copies, seed=5, step_index=2, deterministic=deterministic, write_state=True)
    for k in dry:
        assert np.array_equal(bits(dry[k]), bits(wet[k])), k
    assert not any(np.array_equal(s, k) for s, k in zip(copies, keep))


# --------------------------------------------------------------------------- GAE
def gae_numpy(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """Contract P7 literally, every operation an f32 NumPy scalar operation."""
    f = np.float32
    K, n = rewards.shape
    g32, gl32 = f(gamma), f(np.float64(gamma) * np.float64(gae_lambda))
    adv = np.empty((K, n), f)
    ret = np.empty((K, n), f)
    for e in range(n):
        last = f(0.0)
        for k in range(K - 1, -1, -1):
            if k == K - 1:
                nnt = f(1.0) - f(last_dones[e])
                nv = f(last_values[e])
            else:
                nnt = f(1.0) - f(episode_starts[k + 1, e])
                nv = f(values[k + 1, e])
            delta = f(f(f(rewards[k, e]) + f(f(g32 * nv) * nnt)) - f(values[k, e]))
            last = f(delta + f(f(gl32 * nnt) * last))
            adv[k, e] = last
            ret[k, e] = f(last + f(values[k, e]))
    return adv, ret


def gae_case(K, n, seed):
    rng = np.random.default_rng(seed)
    rewards = rng.normal(0, 1, (K, n)).astype(np.float32)
    values = rng.normal(0, 1, (K, n)).astype(np.float32)
    last_values = rng.normal(0, 1, n).astype(np.float32)
    es = (rng.uniform(size=(K, n)) < 0.3).astype(np.uint8)
    es[0, ::2] = 1                    # a start at k = 0
    es[K - 1, ::3] = 1                # at k = K - 1
    if K >= 3:
        es[K - 3:K - 1, -1] = 1       # on consecutive steps
    last_dones = (np.arange(n) % 2).astype(np.uint8) if n > 1 else np.array([seed % 2], np.uint8)
    return rewards, values, es, last_values, last_dones


@pytest.mark.parametrize("K", [1, 2, 7])
@pytest.mark.parametrize("n", [1, 33])
def test_host_gae_is_the_numpy_loop_bitwise(K, n):
    c = critic_golden()
    gamma, lam = float(c["gamma"]), float(c["gae_lambda"])
    assert abs(gamma - 0.98242) < 1e-5 and abs(lam - 0.91788) < 1e-5
    pol = make_policy()
    for seed in (0, 1):   # n = 1: last_dones clear, then set
        case = gae_case(K, n, seed)
        adv, ret = pol.host_gae(*case, gamma, lam)
        wa, wr = gae_numpy(*case, gamma, lam)
        assert np.array_equal(bits(adv), bits(wa)) and np.array_equal(bits(ret), bits(wr))
        assert np.isfinite(adv).all() and np.abs(adv).min() > 0.0 and np.abs(adv).max() < 1e3
    if n > 1:
        assert case[4].any() and not case[4].all()


# --------------------------------------------------------------------------- loaders and the ABI
def test_loaders_refuse_a_state_dict_without_a_critic_lstm(tmp_path):
    import io
    import zipfile
    import torch
    sd = policy_state_dict()
    no_critic = {k: v for k, v in sd.items() if not k.startswith("lstm_critic.")}
    with pytest.raises(ValueError, match="enable_critic_lstm.*shared_lstm"):
        RecurrentPolicy.from_state_dict(no_critic)
    RecurrentActor.from_state_dict(no_critic)   # the actor's loader keeps ignoring critic keys
    two = dict(sd)
    two["lstm_critic.weight_ih_l1"] = np.zeros((512, 128), np.float32)
    with pytest.raises(ValueError, match="n_lstm_layers"):
        RecurrentPolicy.from_state_dict(two)
    wide = dict(sd)
    wide["value_net.weight"] = np.zeros((2, 64), np.float32)
    with pytest.raises(ValueError, match="value_net.weight"):
        RecurrentPolicy.from_state_dict(wide)
    # from_sb3_zip reads the same tensors
    path = tmp_path / "model.zip"
    buf = io.BytesIO()
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, buf)
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("policy.pth", buf.getvalue())
        z.writestr("data", "{}")
    g = golden()
    a = RecurrentPolicy.from_sb3_zip(path)
    b = RecurrentPolicy.from_state_dict(sd)
    ra = a.host_step(g["obs"][0], g["episode_start"][0], zero_states(16), seed=1, step_index=0)
    rb = b.host_step(g["obs"][0], g["episode_start"][0], zero_states(16), seed=1, step_index=0)
    assert all(np.array_equal(bits(ra[k]), bits(rb[k])) for k in ra)


def raw_host_step(pol, w, n=1):
    z = [np.zeros((n, 128), np.float32) for _ in range(4)]
    o = np.zeros((n, 13), np.float32)
    es = np.ones(n, np.uint8)
    a, ea, v, lp = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    return pol.lib.ha_host_policy_step(ctypes.byref(w), n, 0, 1, 0, 0, 1, o.ctypes.data, es.ctypes.data,
                                       *(t.ctypes.data for t in z), a.ctypes.data, ea.ctypes.data, v.ctypes.data,
                                       lp.ctypes.data, None, None)


def test_abi_refuses_other_shapes():
    pol = make_policy()
    assert raw_host_step(pol, pol._w) == 0
    w = agent.HaPolicyWeights.from_buffer_copy(pol._w)
    w.hidden = 64
    assert raw_host_step(pol, w) == 2   # HE_ESHAPE
    assert b"128" in pol.lib.ha_policy_last_error(None)
    w = agent.HaPolicyWeights.from_buffer_copy(pol._w)
    w.n_lstm_layers = 2
    assert raw_host_step(pol, w) == 2 and b"n_lstm_layers" in pol.lib.ha_policy_last_error(None)
    w = agent.HaPolicyWeights.from_buffer_copy(pol._w)
    w.c_w_hh = None
    assert raw_host_step(pol, w) == 1 and b"critic" in pol.lib.ha_policy_last_error(None)   # HE_EINVAL
    w = agent.HaPolicyWeights.from_buffer_copy(pol._w)
    w.log_std = None
    assert raw_host_step(pol, w) == 1
    w = agent.HaPolicyWeights.from_buffer_copy(pol._w)
    w.abi_version = 2
    assert raw_host_step(pol, w) == 1


def test_load_state_dict_equals_a_fresh_object():
    g = golden()
    pol = make_policy("random")
    sd = policy_state_dict(g)
    fresh = RecurrentPolicy(sd, obs_mean=pol._arrays["obs_mean"], obs_var=pol._arrays["obs_var"])
    obs, start = g["obs"][0], g["episode_start"][0]
    before = pol.host_step(obs, start, zero_states(16), seed=2, step_index=4)
    pol.load_state_dict(sd)
    st_a, st_b = zero_states(16), zero_states(16)
    ra = pol.host_step(obs, start, st_a, seed=2, step_index=4)
    rb = fresh.host_step(obs, start, st_b, seed=2, step_index=4)
    for k in ra:
        assert np.array_equal(bits(ra[k]), bits(rb[k])), k
    for a, b in zip(st_a, st_b):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(before["values"], ra["values"]) and not np.array_equal(before["actions"], ra["actions"])


# --------------------------------------------------------------------------- the code object
def test_policy_kernels_use_no_scratch():
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
    kernels = {k: v for k, v in meta.items() if "policy_step_kernel" in k or "gae_kernel" in k}
    assert len(kernels) == 2, sorted(meta)
    for k, v in kernels.items():
        assert v["scratch_B"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, (k, v)
        assert v["lds_B"] <= 64 * 1024, (k, v)
    ps = [v for k, v in kernels.items() if "policy_step_kernel" in k][0]
    assert ps["lds_B"] > 0
