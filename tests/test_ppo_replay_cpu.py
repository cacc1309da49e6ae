"""train.ppo_update on the host build (no GPU needed) against tests/_ppo_reference.replay, the same
loop over epochs, env groups and time windows written again in torch f64: a CPU RolloutBuffer filled
as RolloutCollector.collect fills one (RecurrentPolicy.host_step, host_gae), then 12 optimizer steps
with torch.optim.SGD or train.DeviceAdam, either weight_grads mode, and the parameters they leave.

Bound, as DESIGN 18-20: per tensor err = max |p_build - p_f64| <= 4 d_ref + ulp, d_ref = max |p_f32 -
p_f64| between the replay run in f32 and in f64 (all torch, never the code under test), ulp = 2^-23 max
|p_initial| (the parameters are stored in f32)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _ppo_reference as ref  # noqa: E402
from cantorrl_amd import train  # noqa: E402
from cantorrl_amd.agent import STATE_NAMES  # noqa: E402
from cantorrl_amd.collect import RolloutBuffer  # noqa: E402
from test_policy_collect_cpu import critic_golden, make_policy  # noqa: E402

HYPER = dict(clip_range=0.3, ent_coef=1e-5, vf_coef=0.5, max_grad_norm=0.5)
SHAPES = ((8, 5, 2, 4), (16, 33, 16, 8))          # K, n, envs_per_batch, window: 12 steps each
OPTIMIZERS = {"sgd": 1e-2, "adam": 1e-4}          # name -> lr
EPOCHS, STEPS = 2, 12
# (policy, K): the seed of the buffer's data; PERM_SEED: of ppo_update's permutations.  Chosen so that the
# f64 replay meets check_replay_inputs (no ratio within 1e-5 of a clip edge, no |A| < 1e-5).
DATA_SEED = {("golden", 8): 1, ("golden", 16): 2, ("random", 8): 3, ("random", 16): 4}
PERM_SEED = 3
_POL, _BUF, _REPLAY = {}, {}, {}


def policy(kind):
    if kind not in _POL:
        _POL[kind] = make_policy(kind)
    return _POL[kind]


def fill_buffer(pol, K, n, seed):
    """A CPU RolloutBuffer(K, n, states=True) filled as RolloutCollector.collect does: per step the
    obs, the starts, states[k], then host_step; host_gae at the end.  Non-zero initial states, obs
    uniform +-1, rewards N(0, 0.1), starts at rate 0.15 plus one on step 0 and one on the window edge K/2."""
    c = critic_golden()
    rng = np.random.default_rng(seed)
    buf = RolloutBuffer(K, n, "cpu", states=True)
    st = tuple(rng.uniform(-0.5, 0.5, (n, 128)).astype(np.float32) for _ in range(4))
    for name, s in zip(STATE_NAMES, st):
        getattr(buf, name).copy_(torch.from_numpy(s))
    starts = (rng.uniform(size=(K, n)) < 0.15).astype(np.uint8)
    starts[0, n - 1] = 1
    starts[K // 2, 0] = 1
    for k in range(K):
        obs = rng.uniform(-1, 1, (n, 13)).astype(np.float32)
        buf.observations[k].copy_(torch.from_numpy(obs))
        buf.episode_starts[k].copy_(torch.from_numpy(starts[k]))
        for i, s in enumerate(st):
            buf.states[k, :, i].copy_(torch.from_numpy(s))
        r = pol.host_step(obs, starts[k], st, seed=9, step_index=k)
        for name in ("actions", "values", "log_probs"):
            getattr(buf, name)[k].copy_(torch.from_numpy(r[name]))
    buf.rewards.copy_(torch.from_numpy(rng.normal(0, 0.1, (K, n)).astype(np.float32)))
    last_dones = (rng.uniform(size=n) < 0.15).astype(np.uint8)
    last = pol.host_step(rng.uniform(-1, 1, (n, 13)).astype(np.float32), last_dones, st, seed=9, step_index=K,
                         deterministic=True, write_state=False)
    buf.last_values.copy_(torch.from_numpy(last["values"]))
    buf.last_dones.copy_(torch.from_numpy(last_dones))
    adv, ret = pol.host_gae(buf.rewards.numpy(), buf.values.numpy(), starts, last["values"], last_dones,
                            float(c["gamma"]), float(c["gae_lambda"]))
    buf.advantages.copy_(torch.from_numpy(adv))
    buf.returns.copy_(torch.from_numpy(ret))
    return buf


def buffer(kind, K, n):
    if (kind, K, n) not in _BUF:
        _BUF[kind, K, n] = fill_buffer(policy(kind), K, n, DATA_SEED[kind, K])
    return _BUF[kind, K, n]


def replays(kind, shape, optimizer):
    """(initial parameters, the f32 replay, the f64 replay, the f64 replay's trace), computed once."""
    key = (kind, shape, optimizer)
    if key not in _REPLAY:
        K, n, per, W = shape
        pol, buf = policy(kind), buffer(kind, K, n)
        p0 = ref.parameters(train.RecurrentPPOModule.from_policy(pol, device="cpu"), torch.float64)
        trace = []
        run = lambda dt, tr: ref.replay(p0, buf, dt, optimizer, OPTIMIZERS[optimizer], EPOCHS, per, W, PERM_SEED, HYPER,
                                        ref.constants(pol), trace=tr)
        _REPLAY[key] = (p0, run(torch.float32, None), run(torch.float64, trace), trace)
    return _REPLAY[key]


# --------------------------------------------------------------------------- the windows
@pytest.mark.parametrize("kind", ("golden", "random"))
def test_a_window_from_the_stored_states_reproduces_the_sequence_bitwise(kind):
    K, n = 8, 5
    pol, buf = policy(kind), buffer(kind, K, n)
    assert buf.episode_starts[0, n - 1] == 1 and buf.episode_starts[K // 2, 0] == 1
    assert 0 < int(buf.episode_starts.sum()) < K * n and float(buf.h_vf.abs().mean()) > 0
    m = train.RecurrentPPOModule.from_policy(pol, device="cpu")
    s0 = tuple(getattr(buf, s) for s in STATE_NAMES)
    mb = train.minibatch(buf, torch.arange(n), 4, 8)
    with torch.no_grad():
        whole = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, s0)
        part = m.evaluate_actions(mb["observations"], mb["actions"], mb["episode_starts"], mb["states0"])
        tv, tlp, _ = ref.evaluate(ref.parameters(m, torch.float32), ref.constants(pol), buf.observations, buf.actions,
                                  buf.episode_starts, s0)
    for name, a, b in zip(("values", "log_prob", "entropy"), whole, part):
        assert torch.equal(a[4:8].contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    # and the whole sequence is what host_step stored, as far as the all-torch f32 composition is
    ev, elp = float((whole[0] - buf.values).abs().max()), float((whole[1] - buf.log_probs).abs().max())
    dv, dlp = float((tv - buf.values).abs().max()), float((tlp - buf.log_probs).abs().max())
    print(f"{kind} values: module {ev:.3e} all-torch {dv:.3e}; log_prob: module {elp:.3e} all-torch {dlp:.3e}")
    assert dv > 0.0 and dlp > 0.0
    assert ev <= 4 * dv, (ev, dv)
    assert elp <= 4 * dlp, (elp, dlp)


# --------------------------------------------------------------------------- the replay
@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
@pytest.mark.parametrize("mode", train.WEIGHT_GRADS)
@pytest.mark.parametrize("kind", ("golden", "random"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ppo_update_lands_where_the_f64_replay_lands(shape, kind, mode, optimizer):
    K, n, per, W = shape
    groups = [min(per, n - lo) for lo in range(0, n, per)]
    assert EPOCHS * len(groups) * (K // W) == STEPS and groups[-1] < per and 1 in groups
    p0, p32, p64, trace = replays(kind, shape, optimizer)
    assert len(trace) == STEPS
    edge, small, fractions = ref.check_replay_inputs(trace, HYPER["clip_range"],
                                                     need_clipping=(kind, optimizer) != ("random", "sgd"))
    print(f"closest ratio to a clip edge {edge:.2e}; smallest |A| {small:.2e}; clip fractions "
          + " ".join(f"{f:.2f}" for f in fractions))
    m = train.RecurrentPPOModule.from_policy(policy(kind), device="cpu", weight_grads=mode)
    lr, count = OPTIMIZERS[optimizer], [0]
    if optimizer == "sgd":
        opt = torch.optim.SGD(m.parameters(), lr=lr)
        opt.register_step_post_hook(lambda *a: count.__setitem__(0, count[0] + 1))
    else:
        opt = train.DeviceAdam(m.parameters(), lr=lr, eps=1e-5)
    stats = train.ppo_update(m, opt, buffer(kind, K, n), n_epochs=EPOCHS, envs_per_batch=per, window=W,
                             generator=torch.Generator().manual_seed(PERM_SEED), **HYPER)
    if optimizer == "adam":
        count[0] = {int(opt.state[p]["step"]) for p in m.parameters()}
        assert len(count[0]) == 1
        count[0] = count[0].pop()
    assert count[0] == STEPS
    # no ratio stands within 1e-5 of an edge: the last minibatch clips the rows the f64 replay clips
    assert abs(float(stats["clip_fraction"]) - fractions[-1]) <= 1e-6
    got = dict(m.named_parameters())
    assert len(got) == 21
    worst = 0.0
    for k, err, d_ref, ulp in ref.replay_bound(p0, p32, p64, got):
        moved = float((got[k].detach().double() - p0[k]).abs().max())
        ratio = err / (4 * d_ref + ulp)
        worst = max(worst, ratio)
        print(f"{k}: err {err:.3e} d_ref {d_ref:.3e} ulp {ulp:.3e} err/d_ref {err / d_ref if d_ref else float('nan'):.2f} "
              f"ratio {ratio:.2f} moved {moved:.3e}")
        assert moved > 0.0, k
        assert err <= 4 * d_ref + ulp, (k, err, d_ref, ulp)
    print(f"worst err / (4 d_ref + ulp): {worst:.2f}")
