"""train.ppo_update on the host build (no GPU needed) against tests/_ppo_reference.replay, the same
loop over epochs, env groups and time windows written again in torch f64: a CPU RolloutBuffer filled
as RolloutCollector.collect fills one (RecurrentPolicy.host_step, host_gae), then 12 optimizer steps
with torch.optim.SGD or train.DeviceAdam, either weight_grads mode, and the parameters they leave.  Then
every route (heads x loss x weight_grads, each "torch" or "kernel") with SB3's value clip, the all-torch and
the all-kernel route on raw advantages with and without it, and seven mistakes put into the replay, each of
which must put the all-kernel route's parameters outside the bound.

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
# The golden policy (log_std about -3.6, ratios up to 44) at K = 16: the two all-torch replays' ratios differ by
# d_ratio = 4e-4 (adam 1e-4) and 4e-3 (sgd 1e-2), and among 3,168 rows no data seed leaves 4 d_ratio free on
# both sides of 1 +- clip_range.  A tenth of the step brings d_ratio to 1e-4, which a seed can meet.
LR = {("golden", 16, "adam"): 1e-5, ("golden", 16, "sgd"): 1e-3}   # (policy, K, optimizer) -> lr, else OPTIMIZERS'
EPOCHS, STEPS = 2, 12
# (policy, K): the seed of the buffer's data; PERM_SEED: of ppo_update's permutations.  Chosen so that the two
# all-torch replays meet check_replay_inputs in every setting: no f64 ratio within max(1e-5, 4 d_ratio) of a clip
# edge, no |dv| within max(1e-5, 4 d_dv) of clip_range_vf, no |A| < 1e-5.  golden 16 was 2: the closest ratio
# stood 6.6e-4 from an edge with 4 d_ratio = 1.8e-3; 22 is the first of seeds 1-24 that leaves the room in all of
# its eight settings (MARGINS).  The other three stand as they stood.
DATA_SEED = {("golden", 8): 1, ("golden", 16): 22, ("random", 8): 3, ("random", 16): 4}
PERM_SEED = 3
ROUTES = tuple((h, l, w) for h in train.HEADS for l in train.LOSSES for w in train.WEIGHT_GRADS)   # heads, loss, weight_grads
# On the host build weight_grads "torch" and "kernel" leave the same bits at (8, 5, 2, 4) (one block of rows each)
# and different ones at (16, 33, 16, 8); both run at both shapes, as on the device they always differ.
# (policy, K, optimizer, normalize_advantage) -> clip_range_vf, found on the f64 replay's trace alone: a value in
# the |dv| rows' upper half that leaves the margin free and clips between 5% and 95% of at least two minibatches.
# With sgd at golden 16 the values move by 3e-3 at most and 3,168 rows lie 1e-6 apart: only the tail has a gap.
CLIP_RANGE_VF = {
    ("golden", 8, "adam", True): 0.078, ("golden", 8, "adam", False): 0.13,
    ("golden", 8, "sgd", True): 0.021, ("golden", 8, "sgd", False): 0.01,
    ("golden", 16, "adam", True): 0.022, ("golden", 16, "adam", False): 0.022,
    ("golden", 16, "sgd", True): 0.0028, ("golden", 16, "sgd", False): 0.00264,
    ("random", 8, "adam", True): 0.27, ("random", 8, "adam", False): 0.27,
    ("random", 8, "sgd", True): 0.061, ("random", 8, "sgd", False): 0.1,
    ("random", 16, "adam", True): 0.45, ("random", 16, "adam", False): 0.45,
    ("random", 16, "sgd", True): 0.36, ("random", 16, "sgd", False): 0.18,
}
# MARGINS, measured on the two all-torch replays (policy, K, optimizer, setting; plain = no value clip, normalised;
# vf = value clip; raw = normalize_advantage=False).  d_ratio, d_dv: the largest |f32 - f64| of a row's ratio and
# dv; edge: the f64 rows' smallest distance from 1 +- clip_range, and of |dv| from clip_range_vf; clipped: the
# smallest and largest share over minibatches 1-11 (value-clipped: 0-11), in brackets how many lie in [0.05, 0.95].
#   golden  8 adam plain  d_ratio 8.2e-05 edge 1.6e-02 |A| 1.8e-02 clipped 0.12-1.00 (9)
#   golden  8 adam vf     d_ratio 5.4e-05 edge 1.6e-02 |A| 1.8e-02 clipped 0.12-1.00 (9); 0.078: d_dv 5.5e-07 edge 2.3e-03 value-clipped 0.00-0.88 (9)
#   golden  8 adam raw    d_ratio 9.3e-05 edge 6.9e-03 |A| 1.2e-02 clipped 0.12-1.00 (10)
#   golden  8 adam vf_raw d_ratio 1.2e-04 edge 5.1e-03 |A| 1.2e-02 clipped 0.12-1.00 (10); 0.13: d_dv 7.0e-07 edge 9.1e-04 value-clipped 0.00-0.75 (7)
#   golden  8 sgd  plain  d_ratio 2.1e-04 edge 1.0e-03 |A| 1.8e-02 clipped 0.00-1.00 (8)
#   golden  8 sgd  vf     d_ratio 1.6e-04 edge 1.0e-03 |A| 1.8e-02 clipped 0.00-1.00 (8); 0.021: d_dv 5.7e-07 edge 1.7e-04 value-clipped 0.00-0.25 (5)
#   golden  8 sgd  raw    d_ratio 5.0e-04 edge 3.6e-03 |A| 1.2e-02 clipped 0.12-1.00 (10)
#   golden  8 sgd  vf_raw d_ratio 1.8e-04 edge 3.6e-03 |A| 1.2e-02 clipped 0.12-1.00 (10); 0.01: d_dv 4.2e-07 edge 3.1e-04 value-clipped 0.00-0.38 (5)
#   golden 16 adam plain  d_ratio 9.6e-05 edge 1.4e-03 |A| 2.0e-03 clipped 0.00-0.16 (7)
#   golden 16 adam vf     d_ratio 7.1e-05 edge 1.5e-03 |A| 2.0e-03 clipped 0.00-0.16 (7); 0.022: d_dv 6.7e-07 edge 3.8e-05 value-clipped 0.00-0.75 (7)
#   golden 16 adam raw    d_ratio 1.0e-04 edge 2.0e-03 |A| 1.0e-03 clipped 0.00-0.25 (6)
#   golden 16 adam vf_raw d_ratio 9.1e-05 edge 2.1e-03 |A| 1.0e-03 clipped 0.00-0.25 (6); 0.022: d_dv 7.1e-07 edge 5.4e-05 value-clipped 0.00-0.75 (7)
#   golden 16 sgd  plain  d_ratio 8.0e-05 edge 2.5e-03 |A| 2.0e-03 clipped 0.00-0.12 (2)
#   golden 16 sgd  vf     d_ratio 8.0e-05 edge 2.5e-03 |A| 2.0e-03 clipped 0.00-0.12 (2); 0.0028: d_dv 7.2e-07 edge 4.1e-05 value-clipped 0.00-0.50 (3)
#   golden 16 sgd  raw    d_ratio 1.1e-04 edge 1.5e-03 |A| 1.0e-03 clipped 0.00-0.08 (1)
#   golden 16 sgd  vf_raw d_ratio 1.1e-04 edge 1.5e-03 |A| 1.0e-03 clipped 0.00-0.08 (1); 0.00264: d_dv 6.7e-07 edge 3.4e-05 value-clipped 0.00-0.25 (3)
#   random  8 adam plain  d_ratio 3.2e-06 edge 2.9e-02 |A| 8.1e-03 clipped 0.00-0.38 (4)
#   random  8 adam vf     d_ratio 2.3e-06 edge 2.2e-02 |A| 8.1e-03 clipped 0.00-0.38 (4); 0.27: d_dv 1.5e-06 edge 2.0e-03 value-clipped 0.00-0.75 (6)
#   random  8 adam raw    d_ratio 3.0e-06 edge 9.4e-03 |A| 4.3e-02 clipped 0.00-0.38 (4)
#   random  8 adam vf_raw d_ratio 2.7e-06 edge 1.1e-02 |A| 4.3e-02 clipped 0.00-0.38 (4); 0.27: d_dv 1.5e-06 edge 3.3e-03 value-clipped 0.00-0.75 (6)
#   random  8 sgd  plain  d_ratio 3.4e-06 edge 1.2e-01 |A| 8.1e-03 clipped 0.00-0.00 (0)
#   random  8 sgd  vf     d_ratio 3.0e-06 edge 1.1e-01 |A| 8.1e-03 clipped 0.00-0.00 (0); 0.061: d_dv 2.4e-06 edge 1.5e-03 value-clipped 0.00-1.00 (6)
#   random  8 sgd  raw    d_ratio 3.1e-06 edge 8.7e-02 |A| 4.3e-02 clipped 0.00-0.00 (0)
#   random  8 sgd  vf_raw d_ratio 2.0e-06 edge 8.6e-02 |A| 4.3e-02 clipped 0.00-0.00 (0); 0.1: d_dv 1.7e-06 edge 2.5e-03 value-clipped 0.00-0.62 (5)
#   random 16 adam plain  d_ratio 8.6e-06 edge 4.9e-04 |A| 9.6e-04 clipped 0.00-0.25 (7)
#   random 16 adam vf     d_ratio 7.6e-06 edge 2.1e-03 |A| 9.6e-04 clipped 0.00-0.25 (7); 0.45: d_dv 2.0e-06 edge 1.3e-03 value-clipped 0.00-0.57 (6)
#   random 16 adam raw    d_ratio 9.4e-06 edge 5.8e-04 |A| 6.9e-03 clipped 0.00-0.25 (7)
#   random 16 adam vf_raw d_ratio 6.2e-06 edge 5.1e-04 |A| 6.9e-03 clipped 0.00-0.12 (7); 0.45: d_dv 2.2e-06 edge 1.4e-04 value-clipped 0.00-0.57 (6)
#   random 16 sgd  plain  d_ratio 1.0e-05 edge 1.2e-01 |A| 9.6e-04 clipped 0.00-0.00 (0)
#   random 16 sgd  vf     d_ratio 5.5e-06 edge 1.2e-01 |A| 9.6e-04 clipped 0.00-0.00 (0); 0.36: d_dv 2.5e-06 edge 5.0e-04 value-clipped 0.00-0.48 (4)
#   random 16 sgd  raw    d_ratio 5.9e-06 edge 6.9e-02 |A| 6.9e-03 clipped 0.00-0.00 (0)
#   random 16 sgd  vf_raw d_ratio 5.4e-06 edge 2.4e-02 |A| 6.9e-03 clipped 0.00-0.00 (0); 0.18: d_dv 3.4e-06 edge 2.5e-04 value-clipped 0.00-0.71 (7)
# the random policy under sgd 1e-2 moves no ratio past 1 +- 0.3 in 12 steps, with or without a value clip
NO_RATIO_CLIPPING = {("random", "sgd")}
# mistake -> the (policy, shape, optimizer) whose all-kernel run must leave the wrong replay's bound; the worst
# err / (4 d_ref + ulp) measured against the wrong replay stands beside it (against the right one: 0.2 to 0.8)
SENSITIVITY = {
    "no_vf_clip": ("random", SHAPES[0], "sgd"),                # 24124
    "vf_max_of_both": ("random", SHAPES[0], "sgd"),            # 2364
    "old_values_first_window": ("golden", SHAPES[0], "adam"),  # 4895
    "old_values_unpermuted": ("random", SHAPES[1], "sgd"),     # 11093
    "biased_std": ("golden", SHAPES[0], "sgd"),                # 552
    "normalize_dropped": ("golden", SHAPES[0], "adam"),        # 7736
    "clip_before_sum": ("random", SHAPES[0], "adam"),          # 2049
}
_POL, _BUF, _REPLAY, _KERNEL_RUN = {}, {}, {}, {}


def lr_of(kind, K, optimizer):
    return LR.get((kind, K, optimizer), OPTIMIZERS[optimizer])


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


def replays_full(kind, shape, optimizer, clip_range_vf=None, normalize_advantage=True):
    """(initial parameters, the f32 replay, the f64 replay, the f64 replay's trace, the f32 replay's
    trace), computed once per setting."""
    key = (kind, shape, optimizer, clip_range_vf, normalize_advantage)
    if key not in _REPLAY:
        K, n, per, W = shape
        pol, buf = policy(kind), buffer(kind, K, n)
        p0 = ref.parameters(train.RecurrentPPOModule.from_policy(pol, device="cpu"), torch.float64)
        trace, trace32 = [], []
        run = lambda dt, tr: ref.replay(p0, buf, dt, optimizer, lr_of(kind, K, optimizer), EPOCHS, per, W, PERM_SEED, HYPER,
                                        ref.constants(pol), trace=tr, clip_range_vf=clip_range_vf,
                                        normalize_advantage=normalize_advantage)
        _REPLAY[key] = (p0, run(torch.float32, trace32), run(torch.float64, trace), trace, trace32)
    return _REPLAY[key]


def replays(kind, shape, optimizer):
    """(initial parameters, the f32 replay, the f64 replay, the f64 replay's trace): no value clip,
    normalised advantages."""
    return replays_full(kind, shape, optimizer)[:4]


def run_update(kind, shape, optimizer, heads="torch", loss="torch", weight_grads="torch", clip_range_vf=None,
               normalize_advantage=True):
    """One ppo_update of STEPS steps on the host build over the route (heads, loss, weight_grads) ->
    (the module, the last minibatch's statistics); the optimizer's step count is checked."""
    K, n, per, W = shape
    m = train.RecurrentPPOModule.from_policy(policy(kind), device="cpu", weight_grads=weight_grads, heads=heads)
    lr, count = lr_of(kind, K, optimizer), [0]
    if optimizer == "sgd":
        opt = torch.optim.SGD(m.parameters(), lr=lr)
        opt.register_step_post_hook(lambda *a: count.__setitem__(0, count[0] + 1))
    else:
        opt = train.DeviceAdam(m.parameters(), lr=lr, eps=1e-5)
    stats = train.ppo_update(m, opt, buffer(kind, K, n), n_epochs=EPOCHS, envs_per_batch=per, window=W, loss=loss,
                             generator=torch.Generator().manual_seed(PERM_SEED), clip_range_vf=clip_range_vf,
                             normalize_advantage=normalize_advantage, **HYPER)
    if optimizer == "adam":
        count[0] = {int(opt.state[p]["step"]) for p in m.parameters()}
        assert len(count[0]) == 1
        count[0] = count[0].pop()
    assert count[0] == STEPS
    return m, stats


def hold_to_the_bound(p0, p32, p64, m):
    """Every tensor of module m moved and stands within 4 d_ref + ulp of the f64 replay -> the worst
    err / (4 d_ref + ulp), printed per tensor."""
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
    return worst


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
    p0, p32, p64, trace, trace32 = replays_full(kind, shape, optimizer)
    assert len(trace) == STEPS
    edge, small, fractions = ref.check_replay_inputs(trace, HYPER["clip_range"], trace32=trace32,
                                                     need_clipping=(kind, optimizer) not in NO_RATIO_CLIPPING)
    print(ref.describe_margins(ref.replay_margins(trace, trace32, HYPER["clip_range"])))
    m, stats = run_update(kind, shape, optimizer, weight_grads=mode)
    # no ratio stands within the margin of an edge: the last minibatch clips the rows the f64 replay clips
    assert abs(float(stats["clip_fraction"]) - fractions[-1]) <= 1e-6
    hold_to_the_bound(p0, p32, p64, m)


# --------------------------------------------------------------------------- every route, value clip, raw advantages
def setting_of(name, kind, K, optimizer):
    """A setting's (clip_range_vf, normalize_advantage)."""
    normalize = name == "vf"
    return (None if name == "raw" else CLIP_RANGE_VF[kind, K, optimizer, normalize]), normalize


def check_case(kind, shape, optimizer, route, setting):
    heads, loss, mode = route
    K = shape[0]
    clip_vf, normalize = setting_of(setting, kind, K, optimizer)
    p0, p32, p64, trace, trace32 = replays_full(kind, shape, optimizer, clip_vf, normalize)
    assert len(trace) == len(trace32) == STEPS
    need = (kind, optimizer) not in NO_RATIO_CLIPPING
    _, _, fractions = ref.check_replay_inputs(trace, HYPER["clip_range"], need_clipping=need, trace32=trace32,
                                              clip_range_vf=clip_vf)
    print(ref.describe_margins(ref.replay_margins(trace, trace32, HYPER["clip_range"], clip_vf)))
    m, stats = run_update(kind, shape, optimizer, heads, loss, mode, clip_vf, normalize)
    assert abs(float(stats["clip_fraction"]) - fractions[-1]) <= 1e-6
    return hold_to_the_bound(p0, p32, p64, m)


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
@pytest.mark.parametrize("route", ROUTES, ids="-".join)
@pytest.mark.parametrize("kind", ("golden", "random"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_route_with_a_value_clip_lands_where_the_f64_replay_lands(shape, kind, route, optimizer):
    check_case(kind, shape, optimizer, route, "vf")


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
@pytest.mark.parametrize("setting", ("raw", "vf_raw"))
@pytest.mark.parametrize("route", (ROUTES[0], ROUTES[-1]), ids="-".join)
@pytest.mark.parametrize("kind", ("golden", "random"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_advantages_land_where_the_f64_replay_lands(shape, kind, route, setting, optimizer):
    check_case(kind, shape, optimizer, route, setting)


# --------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("mistake", ref.MISTAKES)
def test_each_mistake_in_the_replay_puts_the_all_kernel_route_outside_the_bound(mistake):
    """The all-kernel route's parameters against the replay with one thing wrong: at least one tensor
    must stand outside 4 d_ref + ulp, d_ref from the two right replays."""
    kind, shape, optimizer = SENSITIVITY[mistake]
    K, n, per, W = shape
    clip_vf, normalize = setting_of("vf", kind, K, optimizer)
    p0, p32, p64, trace, trace32 = replays_full(kind, shape, optimizer, clip_vf, normalize)
    ref.check_replay_inputs(trace, HYPER["clip_range"], trace32=trace32, clip_range_vf=clip_vf,
                            need_clipping=(kind, optimizer) not in NO_RATIO_CLIPPING)
    key = (kind, shape, optimizer)
    if key not in _KERNEL_RUN:
        _KERNEL_RUN[key] = run_update(kind, shape, optimizer, *ROUTES[-1], clip_vf, normalize)[0]
    got = dict(_KERNEL_RUN[key].named_parameters())
    wrong = ref.replay(p0, buffer(kind, K, n), torch.float64, optimizer, lr_of(kind, K, optimizer), EPOCHS, per, W, PERM_SEED,
                       HYPER, ref.constants(policy(kind)), clip_range_vf=clip_vf, normalize_advantage=normalize,
                       mistake=mistake)
    worst = 0.0
    for k, err, d_ref, ulp in ref.replay_bound(p0, p32, p64, got):
        assert err <= 4 * d_ref + ulp, k           # against the right replay the route holds
        worst = max(worst, float((got[k].detach().double() - wrong[k]).abs().max()) / (4 * d_ref + ulp))
    print(f"{mistake}: worst err / (4 d_ref + ulp) against the wrong replay {worst:.2f}")
    assert worst > 1.0, mistake
