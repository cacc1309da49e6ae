"""RecurrentPolicy and RolloutCollector on the GPU: policy_step_kernel and gae_kernel against the
host build of the same arithmetic bit for bit, and the collector's closed loop: recorded obs
replayed through the host policy, recorded actions replayed through the oracle env, advantages
against ha_host_gae, and the same loop over a DeviceVecNormalize."""
import numpy as np
import pytest

from test_actor_gpu import GBM_CFG, GBM_GEN, gbm_env
from test_policy_collect_cpu import bits, critic_golden, gae_case, make_policy, policy_state_dict, zero_states

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd.agent import STATE_NAMES, STEP_OUTPUTS, RecurrentPolicy  # noqa: E402
from cantorrl_amd.collect import RolloutCollector  # noqa: E402

DEV = "cuda:0"
SEED = 0x51ED270B9F3C11A7


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_outputs(n, fill=7.0):
    return {name: torch.full((n,) + tail, fill, device=DEV) for name, tail in STEP_OUTPUTS}


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("weights_kind", ["golden", "random"])
@pytest.mark.parametrize("n", [1, 16, 33, 257])
def test_device_step_equals_host_build_bitwise(n, weights_kind, deterministic):
    pol = make_policy(weights_kind, device=DEV)
    rng = np.random.default_rng(2000 + n)
    starts = [np.ones(n, np.uint8), (rng.uniform(size=n) < 0.5).astype(np.uint8), np.zeros(n, np.uint8)]
    host = zero_states(n)
    pol.reset_states(n)
    # garbage in the device state: the all-ones first step has to discard it
    for t, v in zip(pol.states, (float("nan"), 3.0, float("nan"), -2.0)):
        t.fill_(v)
    off = 1000 * n
    for s, start in enumerate(starts):
        obs = rng.uniform(-10, 10, (n, 13)).astype(np.float32)
        d_obs, d_start = to_dev(obs), to_dev(start)
        step = 2 ** 32 - 1 + s
        # write_state = 0 first: every output, no state touched
        before = [t.clone() for t in pol.states]
        keep = tuple(a.copy() for a in host)
        h_dry = pol.host_step(obs, start, host, SEED, step, deterministic=deterministic, write_state=False,
                              env_id_offset=off)
        d_dry = pol.step(d_obs, d_start, SEED, step, deterministic=deterministic, write_state=False, env_id_offset=off,
                         out=device_outputs(n))
        for a, k in zip(host, keep):
            assert np.array_equal(bits(a), bits(k))
        if s > 0:   # (the NaN garbage before the first step is not comparable with ==)
            for t, b in zip(pol.states, before):
                assert torch.equal(t, b)
        h_out = pol.host_step(obs, start, host, SEED, step, deterministic=deterministic, env_id_offset=off)
        d_out = pol.step(d_obs, d_start, SEED, step, deterministic=deterministic, env_id_offset=off,
                         out=device_outputs(n))
        torch.cuda.synchronize()
        for name, _ in STEP_OUTPUTS:
            assert np.array_equal(bits(d_out[name].cpu().numpy()), bits(h_out[name])), (name, s)
            assert np.array_equal(bits(d_dry[name].cpu().numpy()), bits(h_dry[name])), (name, s, "write_state=0")
            assert np.array_equal(bits(h_dry[name]), bits(h_out[name]))
        for name, t, a in zip(STATE_NAMES, pol.states, host):
            assert np.array_equal(bits(t.cpu().numpy()), bits(a)), (name, s)
        assert all(np.isfinite(h_out[k]).all() for k in h_out)
        if not deterministic:
            assert np.abs(h_out["actions"] - h_out["mean"]).max() > 0.0
    # the test is not vacuous: no state is zero or saturated everywhere
    for a in (host[0], host[2]):
        assert 0.0 < np.abs(a).mean() < 1.0
    assert not np.array_equal(host[0], host[2])
    pol.close()


def test_load_state_dict_on_the_device_equals_a_fresh_handle():
    n = 33
    pol = make_policy("random", device=DEV)
    rng = np.random.default_rng(5)
    obs = to_dev(rng.uniform(-10, 10, (n, 13)).astype(np.float32))
    start = torch.ones(n, dtype=torch.uint8, device=DEV)
    before = pol.step(obs, start, SEED, 0)
    sd = policy_state_dict()
    pol.load_state_dict(sd)
    fresh = RecurrentPolicy(sd, obs_mean=pol._arrays["obs_mean"], obs_var=pol._arrays["obs_var"], device=DEV)
    out = []
    for p in (pol, fresh):
        p.reset_states(n)
        r = p.step(obs, start, SEED, 1, out=device_outputs(n))
        r = p.step(obs, torch.zeros_like(start), SEED, 2, out=device_outputs(n))
        out.append((r, p.states))
    torch.cuda.synchronize()
    for name, _ in STEP_OUTPUTS:
        assert torch.equal(out[0][0][name], out[1][0][name]), name
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a, b)
    assert not torch.equal(before["values"], out[0][0]["values"])
    # and the host build of the new tensors agrees
    host = zero_states(n)
    pol.host_step(obs.cpu().numpy(), np.ones(n, np.uint8), host, SEED, 1)
    h = pol.host_step(obs.cpu().numpy(), np.zeros(n, np.uint8), host, SEED, 2)
    assert np.array_equal(bits(out[0][0]["values"].cpu().numpy()), bits(h["values"]))
    assert np.array_equal(bits(out[0][0]["actions"].cpu().numpy()), bits(h["actions"]))
    pol.close()
    fresh.close()


@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("n", [1, 257])
def test_device_gae_equals_host_gae_bitwise(K, n):
    c = critic_golden()
    gamma, lam = float(c["gamma"]), float(c["gae_lambda"])
    pol = make_policy(device=DEV)
    for seed in (0, 1):
        case = gae_case(K, n, seed)
        ha, hr = pol.host_gae(*case, gamma, lam)
        da, dr = pol.gae(*(to_dev(a) for a in case), gamma, lam)
        torch.cuda.synchronize()
        assert np.array_equal(bits(da.cpu().numpy()), bits(ha)) and np.array_equal(bits(dr.cpu().numpy()), bits(hr))
    pol.close()


def host_replay(pol, buf_obs, buf_start, seed, step0, states):
    K = buf_start.shape[0]
    out = {k: [] for k in ("actions", "env_actions", "values", "log_probs")}
    for k in range(K):
        r = pol.host_step(buf_obs[k], buf_start[k], states, seed, step0 + k)
        for name in out:
            out[name].append(r[name])
    return {k: np.stack(v) for k, v in out.items()}


def test_collector_closed_loop_on_a_gbm_env():
    from oracle.hedging_oracle import OracleVecEnv
    from test_gpu_parity import compare_obs, greeks_log_allowance
    from _compare import assert_same
    n, seed = 33, 42
    c = critic_golden()
    gamma, lam = float(c["gamma"]), float(c["gae_lambda"])
    pol = make_policy("golden", device=DEV)   # the checkpoint's own statistics on the raw obs
    venv = gbm_env(n, seed, ("per_share_step_pnl",))
    col = RolloutCollector(venv, pol, gamma, lam, seed=SEED)
    b1 = col.collect(12)
    snap1 = {k: getattr(b1, k).cpu().numpy() for k in ("observations", "actions", "rewards", "values", "log_probs",
                                                       "advantages", "returns", "episode_starts", "last_values",
                                                       "last_dones") + STATE_NAMES}
    after1 = [t.cpu().numpy() for t in pol.states]
    final_obs1 = col._obs.cpu().numpy()
    b2 = col.collect(8)
    torch.cuda.synchronize()
    snap2 = {k: getattr(b2, k).cpu().numpy() for k in snap1}
    after2 = [t.cpu().numpy() for t in pol.states]
    assert col.step_index == 20
    # every env begins an episode at step 0 and crosses a boundary (episode_length 8) inside the first call
    assert snap1["episode_starts"][0].all() and snap1["episode_starts"][8].all() and snap1["episode_starts"].sum() == 2 * n
    for s in STATE_NAMES:
        assert not snap1[s].any()   # the states before step 0 of the first call
    # (a) the recorded obs and flags replayed through the host policy
    host = zero_states(n)
    for snap, step0, after in ((snap1, 0, after1), (snap2, 12, after2)):
        for s, a in zip(STATE_NAMES, host):
            assert np.array_equal(bits(snap[s]), bits(a)), s
        rep = host_replay(pol, snap["observations"], snap["episode_starts"], SEED, step0, host)
        for k in ("actions", "values", "log_probs"):
            assert np.array_equal(bits(rep[k]), bits(snap[k])), k
        # last_values came from a call that changed no state: the states equal the replay's
        for a, d in zip(host, after):
            assert np.array_equal(bits(a), bits(d))
    assert np.array_equal(bits(snap2["observations"][0]), bits(final_obs1))
    lv = pol.host_step(final_obs1, snap1["last_dones"], tuple(a.copy() for a in after1), SEED, 12, deterministic=True,
                       write_state=False)["values"]
    assert np.array_equal(bits(lv), bits(snap1["last_values"]))
    assert np.array_equal(snap2["episode_starts"][0], snap1["last_dones"])

    # (b) the oracle env stepped with clip(actions, +-1) reproduces rewards and obs
    orc = OracleVecEnv(n, mode="gbm", gen=dict(GBM_GEN, seed=seed, env_offset=0), **GBM_CFG)
    orc.seed_envs_at(np.arange(n), [seed] * n)
    compare_obs(snap1["observations"][0], orc.reset(), "reset_obs")
    acts = np.concatenate([snap1["actions"], snap2["actions"]])
    rew = np.concatenate([snap1["rewards"], snap2["rewards"]])
    nxt_obs = np.concatenate([snap1["observations"][1:], snap2["observations"], col._obs.cpu().numpy()[None]])
    nxt_start = np.concatenate([snap1["episode_starts"][1:], snap2["episode_starts"], snap2["last_dones"][None]])
    assert np.abs(acts).max() > 0.0 and np.abs(acts).std() > 0.0
    for s in range(20):
        clipped = np.clip(acts[s], -1.0, 1.0)
        oo, orew, oterm, _, _ = orc.step(clipped)
        assert_same(nxt_start[s].astype(bool), oterm, f"terminated[{s}]")
        assert_same(rew[s], orew.astype(np.float32), f"reward[{s}]")
        compare_obs(nxt_obs[s], oo, f"obs[{s}]", gk_atol=greeks_log_allowance(orc.S, orc.v))

    # (c) advantages and returns are ha_host_gae of the recorded columns
    for snap in (snap1, snap2):
        adv, ret = pol.host_gae(snap["rewards"], snap["values"], snap["episode_starts"], snap["last_values"],
                                snap["last_dones"], gamma, lam)
        assert np.array_equal(bits(adv), bits(snap["advantages"])) and np.array_equal(bits(ret), bits(snap["returns"]))
        assert np.isfinite(adv).all() and np.abs(adv).max() > 0.0
    venv.close()
    pol.close()


def test_collector_over_device_vecnormalize_in_training_mode():
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    n, K, seed = 16, 10, 7
    c = critic_golden()
    gamma, lam = float(c["gamma"]), float(c["gae_lambda"])
    pol = make_policy("golden", norm=False, device=DEV)   # the wrapper normalises
    env = DeviceVecNormalize(gbm_env(n, seed, ("per_share_step_pnl",)), training=True, gamma=gamma)
    col = RolloutCollector(env, pol, gamma, lam, seed=SEED)
    b = col.collect(K, states=True)
    torch.cuda.synchronize()
    for k in ("observations", "actions", "rewards", "values", "log_probs", "advantages", "returns", "states"):
        assert torch.isfinite(getattr(b, k)).all(), k
    assert b.states.shape == (K, n, 4, 128) and not b.states[0].any() and b.states[K - 1].abs().mean() > 0
    # a manual loop with the same seeds: the recorded obs are the wrapper's normalised ones
    pol2 = make_policy("golden", norm=False, device=DEV)
    env2 = DeviceVecNormalize(gbm_env(n, seed, ("per_share_step_pnl",)), training=True, gamma=gamma)
    o = env2.reset_tensors()
    start = torch.ones(n, dtype=torch.uint8, device=DEV)
    raw = gbm_env(n, seed, ("per_share_step_pnl",))
    raw_obs0 = raw.reset_tensors().clone()
    for k in range(K):
        assert torch.equal(b.observations[k], o), k
        assert torch.equal(b.episode_starts[k], start), k
        r = pol2.step(o.clone(), start, SEED, k)
        assert torch.equal(r["actions"], b.actions[k])
        o, rew, term, _ = env2.step_tensors(r["env_actions"], info=False)
        assert torch.equal(rew, b.rewards[k])
        start = term.clone()
    assert not torch.equal(b.observations[0], raw_obs0)   # normalised, not the env's raw obs
    assert b.episode_starts.sum() == 2 * n
    for x in (env, env2, raw, pol, pol2):
        x.close()
