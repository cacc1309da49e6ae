"""RecurrentActor on the GPU: the gfx950 kernel against the host build of the same arithmetic
(ha_host_step) bit for bit, against the reference's golden within the measured bound of
test_actor_cpu.py (4 x d_ref), and the closed loop around he_step (rollout_actor /
evaluate_actor): recorded obs replayed through the host actor, recorded actions replayed through
the oracle env, episode records against the step-ordered f64 sums of the info columns."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_actor_cpu import FLAVOURS, d_ref, f64_cached, golden, make_actor, state_dict

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import _lib  # noqa: E402
from cantorrl_amd.agent import ACTOR_KEYS, RECORD_INFO_KEYS, RecurrentActor  # noqa: E402

DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_weights(seed):
    rng = np.random.default_rng(seed)
    return {f: rng.uniform(-0.5, 0.5, shape).astype(np.float32) for _, f, shape in ACTOR_KEYS}


def actor_for(weights_kind, flavour):
    act, sq, clip = FLAVOURS[flavour]
    if weights_kind == "golden":
        g = golden()
        return make_actor(g, flavour)
    rng = np.random.default_rng(99)
    return RecurrentActor(random_weights(7), obs_mean=rng.uniform(-1, 1, 13), obs_var=rng.uniform(4, 36, 13),
                          clip_obs=clip, activation=act, squash=sq, device=DEV)


@pytest.mark.parametrize("flavour", ["sb3", "ref"])
@pytest.mark.parametrize("weights_kind", ["golden", "random"])
@pytest.mark.parametrize("n", [1, 16, 33, 257])
def test_device_step_equals_host_build_bitwise(n, weights_kind, flavour):
    actor = actor_for(weights_kind, flavour)
    rng = np.random.default_rng(1000 + n)
    starts = [np.ones(n, np.uint8), (rng.uniform(size=n) < 0.5).astype(np.uint8), np.zeros(n, np.uint8)]
    hh = np.zeros((n, 128), np.float32)
    hc = np.zeros((n, 128), np.float32)
    actor.reset_states(n)
    # garbage in the device state: the all-ones first step has to discard it
    actor.h.fill_(float("nan"))
    actor.c.fill_(3.0)
    worst = {}
    for s, start in enumerate(starts):
        obs = rng.uniform(-10, 10, (n, 13)).astype(np.float32)
        hm = np.empty((n, 2), np.float32)
        hx = np.empty((n, 13), np.float32)
        ha = actor.host_step(obs, start, hh, hc, mean_out=hm, obs_norm_out=hx)
        dm = torch.full((n, 2), 7.0, device=DEV)
        dx = torch.full((n, 13), 7.0, device=DEV)
        da = actor.step(torch.from_numpy(obs).to(DEV), torch.from_numpy(start).to(DEV), mean_out=dm, obs_norm_out=dx)
        torch.cuda.synchronize()
        got = dict(actions=da, mean=dm, obs_norm=dx, h=actor.h, c=actor.c)
        exp = dict(actions=ha, mean=hm, obs_norm=hx, h=hh, c=hc)
        for k in got:
            gk = got[k].cpu().numpy()
            worst[k] = max(worst.get(k, 0.0), float(np.nanmax(np.abs(gk.astype(np.float64) - exp[k]))))
            assert np.array_equal(bits(gk), bits(exp[k])), (k, s, worst)
        assert np.isfinite(hh).all() and np.isfinite(hm).all()
    # the test is not vacuous: the state is neither zero nor saturated everywhere
    assert 0.0 < np.abs(hh).mean() < 1.0
    actor.close()


@pytest.mark.parametrize("flavour", ["sb3", "ref"])
def test_golden_sequence_on_device_within_4_d_ref(flavour):
    g = golden()
    A64, H64 = f64_cached(g, flavour)
    da, dh = d_ref(g, flavour)
    actor = make_actor(g, flavour)
    T, N = g["episode_start"].shape
    obs = torch.from_numpy(g["obs"]).to(DEV)
    start = torch.from_numpy(g["episode_start"]).to(DEV)
    acts = torch.empty((T, N, 2), device=DEV)
    hs = torch.empty((T, N, 128), device=DEV)
    actor.reset_states(N)
    for t in range(T):
        actor.step(obs[t], start[t], out=acts[t])
        hs[t].copy_(actor.h)
    torch.cuda.synchronize()
    ea = float(np.abs(acts.cpu().numpy() - A64).max())
    eh = float(np.abs(hs.cpu().numpy() - H64).max())
    print(f"{flavour}: actions device {ea:.3e} reference {da:.3e}; h device {eh:.3e} reference {dh:.3e}")
    assert ea <= 4 * da, (ea, da)
    assert eh <= 4 * dh, (eh, dh)
    actor.close()


def host_replay(actor, obs_fed, start_fed, zero_by_hand=False):
    """ha_host_step over recorded [K,N,13] obs and [K,N] episode_start -> actions, h, c."""
    K, n = start_fed.shape
    h = np.zeros((n, 128), np.float32)
    c = np.zeros((n, 128), np.float32)
    out = []
    for k in range(K):
        st = start_fed[k]
        if zero_by_hand:
            h[st != 0] = 0.0
            c[st != 0] = 0.0
            st = np.zeros_like(st)
        out.append(actor.host_step(obs_fed[k], st, h, c))
    return np.stack(out), h, c


def sorted_records(recs):
    return recs[np.lexsort((recs["reward_sum"], recs["env_id"]))]


def expected_records(info, term, n_off=0):
    """The sequential f64 sums of the per-step info columns [K,N], cut at terminated."""
    K, n = term.shape
    rows = []
    for e in range(n):
        s = np.zeros(7)
        length = 0
        for k in range(K):
            for j, key in enumerate(RECORD_INFO_KEYS):
                s[j] = s[j] + info[key][k, e]
            length += 1
            if term[k, e]:
                rows.append((n_off + e, length, 0, *s, 0.0))
                s = np.zeros(7)
                length = 0
    return np.array(rows, dtype=_lib.EPISODE_RECORD)


GBM_CFG = dict(loss_type="abs", pnl_penalty_weight=0.001, lambda_cost=0.0001, theta_weight=0.0002, slippage_bps=1.0)
GBM_GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=8)


def gbm_env(n, seed, info_keys):
    from cantorrl_amd.vec_env import HedgingVecEnv
    return HedgingVecEnv(n, mode="gbm", generate=GBM_GEN, seed=seed, info_keys=info_keys, return_numpy=False,
                         device=DEV, **GBM_CFG)


def test_closed_loop_generate_mode():
    from oracle.hedging_oracle import OracleVecEnv
    from test_gpu_parity import compare_obs, greeks_log_allowance
    from _compare import assert_same
    n, K, seed = 33, 20, 42
    g = golden()
    actor = make_actor(g, "sb3")
    venv = gbm_env(n, seed, RECORD_INFO_KEYS)
    obs0 = venv.reset_tensors().clone()
    acts = torch.empty((K, n, 2), device=DEV)
    obs = torch.empty((K, n, 13), device=DEV)
    rew = torch.empty((K, n), device=DEV)
    term = torch.empty((K, n), dtype=torch.uint8, device=DEV)
    recs = torch.zeros((4 * n, 80), dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    venv.rollout_actor(actor, 12, actions_out=acts[:12], obs=obs[:12], reward=rew[:12], terminated=term[:12],
                       records=recs, record_count=cnt)
    venv.rollout_actor(actor, 8, actions_out=acts[12:], obs=obs[12:], reward=rew[12:], terminated=term[12:],
                       records=recs, record_count=cnt)   # a second call continues the loop
    torch.cuda.synchronize()
    acts_h, obs_h, rew_h, term_h = (t.cpu().numpy() for t in (acts, obs, rew, term))
    count = int(cnt.item())
    got = sorted_records(recs[:count].cpu().numpy().view(_lib.EPISODE_RECORD).reshape(count))
    assert term_h.sum() == 2 * n and count == 2 * n
    assert (got["length"] == 8).all()

    # (a) the host actor fed the recorded obs and flags gives the recorded actions bit for bit
    fed = np.concatenate([obs0.cpu().numpy()[None], obs_h[:-1]])
    start = np.concatenate([np.ones((1, n), np.uint8), term_h[:-1]])
    host_a, host_h, host_c = host_replay(actor, fed, start)
    assert np.array_equal(bits(host_a), bits(acts_h))
    assert np.array_equal(bits(host_h), bits(actor.h.cpu().numpy()))
    assert np.array_equal(bits(host_c), bits(actor.c.cpu().numpy()))
    assert np.abs(acts_h).max() <= 1.0 and np.abs(acts_h).std() > 0.0

    # (b) the oracle env stepped with the recorded actions reproduces obs / reward / terminated
    orc = OracleVecEnv(n, mode="gbm", gen=dict(GBM_GEN, seed=seed, env_offset=0), **GBM_CFG)
    orc.seed_envs_at(np.arange(n), [seed] * n)
    compare_obs(obs0.cpu().numpy(), orc.reset(), "reset_obs")
    for s in range(K):
        oo, orew, oterm, _, _ = orc.step(acts_h[s])
        assert_same(term_h[s].astype(bool), oterm, f"terminated[{s}]")
        assert_same(rew_h[s], orew.astype(np.float32), f"reward[{s}]")
        compare_obs(obs_h[s], oo, f"obs[{s}]", gk_atol=greeks_log_allowance(orc.S, orc.v))

    # (c) a manual loop of actor.step / step_tensors / accumulate with the same seeds: the same
    # records bit for bit, and each equals the step-ordered f64 sums of the info columns
    actor2 = make_actor(g, "sb3")
    venv2 = gbm_env(n, seed, RECORD_INFO_KEYS)
    o = venv2.reset_tensors()
    actor2.reset_states(n)
    st = torch.ones(n, dtype=torch.uint8, device=DEV)
    recs2 = torch.zeros_like(recs)
    cnt2 = torch.zeros_like(cnt)
    info = {k: np.empty((K, n)) for k in RECORD_INFO_KEYS}
    for k in range(K):
        a = actor2.step(o, st)
        o, _, t, _ = venv2.step_tensors(a)
        actor2.accumulate({key: venv2.info_tensor(key) for key in RECORD_INFO_KEYS}, t, recs2, cnt2)
        st = t.clone()
        for key in RECORD_INFO_KEYS:
            info[key][k] = venv2.info_tensor(key).cpu().numpy()
        assert np.array_equal(t.cpu().numpy(), term_h[k])
    count2 = int(cnt2.item())
    got2 = sorted_records(recs2[:count2].cpu().numpy().view(_lib.EPISODE_RECORD).reshape(count2))
    assert got.tobytes() == got2.tobytes()
    exp = sorted_records(expected_records(info, term_h))
    assert got.tobytes() == exp.tobytes()
    assert np.abs(got["reward_sum"]).min() > 0.0
    for x in (venv, venv2, actor, actor2):
        x.close()


def test_closed_loop_replay_mode_crosses_the_episode_boundary():
    from oracle.hedging_oracle import load_golden
    cfg, d = load_golden(os.path.join(GOLDEN, "g1_v2_train.npz"))
    from cantorrl_amd.vec_env import HedgingVecEnv
    n, K = 16, 260
    venv = HedgingVecEnv(n, tables=(d["paths"], d["volatilities"], d["call_prices_atm"], d["put_prices_atm"]),
                         variant=int(d["variant"]), info_keys=RECORD_INFO_KEYS, return_numpy=False, device=DEV, **cfg)
    venv.seed_envs([int(d["seed_base"]) + i for i in range(n)])
    g = golden()
    actor = make_actor(g, "sb3")
    obs0 = venv.reset_tensors(episode_idx=d["ep_idx0"]).clone()
    acts = torch.empty((K, n, 2), device=DEV)
    obs = torch.empty((K, n, 13), device=DEV)
    term = torch.empty((K, n), dtype=torch.uint8, device=DEV)
    recs = torch.zeros((2 * n, 80), dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    venv.rollout_actor(actor, K, actions_out=acts, obs=obs, terminated=term, records=recs, record_count=cnt)
    torch.cuda.synchronize()
    term_h, obs_h, acts_h = term.cpu().numpy(), obs.cpu().numpy(), acts.cpu().numpy()
    assert term_h[251].all() and term_h.sum() == n and int(cnt.item()) == n   # t = 252 is crossed
    fed = np.concatenate([obs0.cpu().numpy()[None], obs_h[:-1]])
    start = np.concatenate([np.ones((1, n), np.uint8), term_h[:-1]])
    host_a, host_h, host_c = host_replay(actor, fed, start)
    assert np.array_equal(bits(host_a), bits(acts_h))
    # h, c restart from zero at the boundary: zeroing them by hand there (and passing no flag)
    # is the same computation
    hand_a, hand_h, hand_c = host_replay(actor, fed, start, zero_by_hand=True)
    assert np.array_equal(bits(hand_a), bits(acts_h))
    assert np.array_equal(bits(hand_h), bits(actor.h.cpu().numpy()))
    assert np.array_equal(bits(hand_c), bits(actor.c.cpu().numpy()))
    r = recs[:n].cpu().numpy().view(_lib.EPISODE_RECORD).reshape(n)
    assert (r["length"] == 252).all() and sorted(r["env_id"]) == list(range(n))
    venv.close()
    actor.close()


def test_evaluate_actor_row_count_and_missing_info_keys():
    g = golden()
    actor = make_actor(g, "sb3")
    n = 33
    venv = gbm_env(n, 3, RECORD_INFO_KEYS)
    recs = venv.evaluate_actor(actor, 50, chunk=8)
    assert recs.dtype == _lib.EPISODE_RECORD and recs.shape == (50,)
    assert (recs["length"] == 8).all() and np.isfinite(recs["reward_sum"]).all()
    assert set(recs["env_id"]) <= set(range(n))
    venv.close()
    bare = gbm_env(n, 3, ("per_share_step_pnl", "raw_pnl_deviation_abs", "transaction_costs_total"))
    with pytest.raises(ValueError, match="reward_step"):
        bare.evaluate_actor(actor, 5)
    with pytest.raises(ValueError, match="step_pnl_total"):
        bare.rollout_actor(actor, 1)
    bare.close()
    actor.close()
