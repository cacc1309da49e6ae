"""train.ppo_update on the GPU against tests/_ppo_reference.replay run on the device in torch f64, as
test_ppo_replay_cpu.py does on the host build: the collector's buffer of test_ppo_update_gpu.rollout()
(33 envs = one 32-env tile plus one, 16 steps, stored states), 2 epochs of groups of 16 envs x windows of
8 steps = 12 optimizer steps, torch.optim.SGD and train.DeviceAdam; every route (heads x loss x
weight_grads, each "torch" or "kernel") with SB3's value clip, the all-torch and the all-kernel route
also on raw advantages; and the LSTM kernels over a window from minibatch's states against the same rows
of the whole sequence.

Bound: per tensor max |p_device - p_f64| <= 4 d_ref + ulp, d_ref = max |p_f32 - p_f64| between the two
all-torch replays, ulp = 2^-23 max |p_initial|."""
import pytest

import _ppo_reference as ref
from test_ppo_update_gpu import HYPER, rollout, states0

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402

DEV = "cuda:0"
# name -> lr.  They were 1e-2 and 1e-4: on this buffer (the golden policy, log_std about -3.6) the two all-torch
# replays' ratios then differ by d_ratio = 1e-4 to 4e-3, and with PERM_SEED 3 to 18 the closest of the 3,168 f64
# ratios stood nearer than 4 d_ratio to 1 +- clip_range (sgd: 2.0e-5 from it, 4 d_ratio = 1.5e-3; adam: 2.4e-4
# from it, 4 d_ratio = 4.2e-4).  A tenth of the step brings d_ratio to 3e-5 and the margin holds (MARGINS below).
OPTIMIZERS = {"sgd": 1e-3, "adam": 1e-5}
EPOCHS, PER, W, STEPS = 2, 16, 8, 12
PERM_SEED = 3
POOLED = ()                                # groups of tensors that share a d_ref (none needed)
ROUTES = tuple((h, l, w) for h in train.HEADS for l in train.LOSSES for w in train.WEIGHT_GRADS)   # heads, loss, weight_grads
# (optimizer, normalize_advantage) -> clip_range_vf, found on the f64 replay's trace alone: of 60 values between
# the median and the 97th percentile of the rows' |dv|, the one that leaves most room before the margins.
CLIP_RANGE_VF = {("adam", True): 0.016, ("adam", False): 0.0135, ("sgd", True): 0.001855}
# MARGINS, measured on the two all-torch replays on the device.  d_ratio, d_dv: the largest |f32 - f64| of a row's
# ratio and dv; edge: the f64 rows' smallest distance from 1 +- clip_range, and of |dv| from clip_range_vf.
#   adam plain  d_ratio 2.7e-05 edge 1.7e-03 |A| 3.5e-02 clipped 0 0 .02 .02 0 0 .02 .06 .03 .04 .12 0
#   adam vf     d_ratio 2.7e-05 edge 1.7e-03 |A| 3.5e-02 clipped as plain; 0.016: d_dv 5.8e-07 edge 7.1e-05
#               value-clipped 0 0 0 0 0 0 .20 .38 .50 .74 .75 .88
#   adam raw    d_ratio 2.3e-05 edge 6.4e-03 |A| 2.4e-03 clipped 0 0 .02 .02 0 0 .03 .02 0 .01 .12 0
#   adam vf_raw d_ratio 2.1e-05 edge 6.3e-03 |A| 2.4e-03 clipped as raw; 0.0135: d_dv 4.3e-07 edge 5.7e-05
#               value-clipped 0 0 0 0 0 0 .38 .50 .73 .75 .88 .88
#   sgd  plain  d_ratio 2.7e-05 edge 8.5e-04 |A| 3.5e-02 clipped 0 .08 .14 0 0 0 .05 0 .06 .01 .12 .12
#   sgd  vf     d_ratio 2.7e-05 edge 8.5e-04 |A| 3.5e-02 clipped as plain; 0.001855: d_dv 4.4e-07 edge 1.1e-04
#               value-clipped 0 0 0 0 0 0 0 0 .88 .88 .88 .88 (under sgd the values move together, the rows' |dv|
#               lie 1e-6 apart, and every value with room takes 7 rows of 8 of a second-epoch minibatch or none)
_REPLAY = {}


@pytest.fixture(scope="module")
def collected():
    pol, venv, col, buf = rollout()
    yield pol, buf
    venv.close()
    pol.close()


def replays_full(pol, buf, optimizer, clip_range_vf=None, normalize_advantage=True):
    """(initial parameters, the f32 replay, the f64 replay, the f64 replay's trace, the f32 replay's
    trace), computed once per (optimizer, clip_range_vf, normalize_advantage)."""
    key = (optimizer, clip_range_vf, normalize_advantage)
    if key not in _REPLAY:
        p0 = ref.parameters(train.RecurrentPPOModule.from_policy(pol), torch.float64)
        trace, trace32 = [], []
        run = lambda dt, tr: ref.replay(p0, buf, dt, optimizer, OPTIMIZERS[optimizer], EPOCHS, PER, W, PERM_SEED, HYPER,
                                        ref.constants(pol), trace=tr, clip_range_vf=clip_range_vf,
                                        normalize_advantage=normalize_advantage)
        _REPLAY[key] = (p0, run(torch.float32, trace32), run(torch.float64, trace), trace, trace32)
    return _REPLAY[key]


def replays(pol, buf, optimizer):
    """(initial parameters, the f32 replay, the f64 replay, the f64 replay's trace): no value clip,
    normalised advantages."""
    return replays_full(pol, buf, optimizer)[:4]


def run_update(pol, buf, optimizer, heads="torch", loss="torch", weight_grads="torch", clip_range_vf=None,
               normalize_advantage=True):
    """One ppo_update of STEPS steps on the device over the route (heads, loss, weight_grads) ->
    (the module, the last minibatch's statistics); the optimizer's step count is checked."""
    m = train.RecurrentPPOModule.from_policy(pol, weight_grads=weight_grads, heads=heads)
    lr, count = OPTIMIZERS[optimizer], [0]
    if optimizer == "sgd":
        opt = torch.optim.SGD(m.parameters(), lr=lr)
        opt.register_step_post_hook(lambda *a: count.__setitem__(0, count[0] + 1))
    else:
        opt = train.DeviceAdam(m.parameters(), lr=lr, eps=1e-5)
    stats = train.ppo_update(m, opt, buf, n_epochs=EPOCHS, envs_per_batch=PER, window=W, loss=loss,
                             generator=torch.Generator(device=DEV).manual_seed(PERM_SEED), clip_range_vf=clip_range_vf,
                             normalize_advantage=normalize_advantage, **HYPER)
    torch.cuda.synchronize()
    if optimizer == "adam":
        steps = {int(opt.state[p]["step"]) for p in m.parameters()}
        assert len(steps) == 1
        count[0] = steps.pop()
    assert count[0] == STEPS
    return m, stats


def hold_to_the_bound(p0, p32, p64, m):
    """Every tensor of module m moved and stands within 4 d_ref + ulp of the f64 replay -> the worst
    err / (4 d_ref + ulp), printed per tensor."""
    got = dict(m.named_parameters())
    assert len(got) == 21
    worst = 0.0
    for k, err, d_ref, ulp in ref.replay_bound(p0, p32, p64, got, POOLED):
        moved = float((got[k].detach().double() - p0[k]).abs().max())
        ratio = err / (4 * d_ref + ulp)
        worst = max(worst, ratio)
        print(f"{k}: err {err:.3e} d_ref {d_ref:.3e} ulp {ulp:.3e} err/d_ref {err / d_ref if d_ref else float('nan'):.2f} "
              f"ratio {ratio:.2f} moved {moved:.3e}")
        assert moved > 0.0, k
        assert err <= 4 * d_ref + ulp, (k, err, d_ref, ulp)
    print(f"worst err / (4 d_ref + ulp): {worst:.2f}")
    return worst


def test_the_lstm_kernels_over_a_window_give_the_bits_of_the_whole_sequence(collected):
    pol, buf = collected
    K, n = buf.k_steps, buf.n_envs
    assert (K, n) == (16, 33) and buf.states is not None and int(buf.episode_starts[8:].sum()) > 0
    m = train.RecurrentPPOModule.from_policy(pol)
    const = ref.constants(pol)
    mb = train.minibatch(buf, torch.arange(n, device=DEV), 8, 16)
    s0 = states0(buf)
    with torch.no_grad():
        nets = lambda s: ((s[0], s[1], *m.lstm_actor.tensors()), (s[2], s[3], *m.lstm_critic.tensors()))
        whole = train.lstm_sequence_pair(ref.normalize(buf.observations, const), buf.episode_starts, *nets(s0))
        part = train.lstm_sequence_pair(ref.normalize(mb["observations"], const), mb["episode_starts"], *nets(mb["states0"]))
        v, lp, _ = m.evaluate_actions(mb["observations"], mb["actions"], mb["episode_starts"], mb["states0"])
        tv, tlp, _ = ref.evaluate(ref.parameters(m, torch.float32), const, buf.observations, buf.actions,
                                  buf.episode_starts, s0)
    torch.cuda.synchronize()
    for name, a, b in zip(("h_pi", "h_vf"), whole, part):
        assert float(b.abs().mean()) > 0.0
        assert torch.equal(a[8:16].contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    # the heads are torch's GEMMs over another row count: held to the buffer as the whole sequence is
    ev, elp = float((v - buf.values[8:16]).abs().max()), float((lp - buf.log_probs[8:16]).abs().max())
    dv, dlp = float((tv[8:16] - buf.values[8:16]).abs().max()), float((tlp[8:16] - buf.log_probs[8:16]).abs().max())
    print(f"window values: module {ev:.3e} all-torch {dv:.3e}; log_prob: module {elp:.3e} all-torch {dlp:.3e}")
    assert dv > 0.0 and dlp > 0.0
    assert ev <= 4 * dv, (ev, dv)
    assert elp <= 4 * dlp, (elp, dlp)


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
@pytest.mark.parametrize("mode", train.WEIGHT_GRADS)
def test_ppo_update_lands_where_the_f64_replay_lands(collected, mode, optimizer):
    pol, buf = collected
    p0, p32, p64, trace, trace32 = replays_full(pol, buf, optimizer)
    assert len(trace) == STEPS
    ref.check_replay_inputs(trace, HYPER["clip_range"], trace32=trace32)
    print(ref.describe_margins(ref.replay_margins(trace, trace32, HYPER["clip_range"])))
    m, _ = run_update(pol, buf, optimizer, weight_grads=mode)
    hold_to_the_bound(p0, p32, p64, m)


# --------------------------------------------------------------------------- every route, value clip, raw advantages
def check_case(pol, buf, optimizer, route, setting, monkeypatch):
    normalize = setting == "vf"
    clip_vf = None if setting == "raw" else CLIP_RANGE_VF[optimizer, normalize]
    p0, p32, p64, trace, trace32 = replays_full(pol, buf, optimizer, clip_vf, normalize)
    assert len(trace) == len(trace32) == STEPS
    ref.check_replay_inputs(trace, HYPER["clip_range"], trace32=trace32, clip_range_vf=clip_vf)
    print(ref.describe_margins(ref.replay_margins(trace, trace32, HYPER["clip_range"], clip_vf)))
    calls = []   # what the loss kernel was handed: (values, old_values) per minibatch
    if route[1] == "kernel":
        kernel = train.ppo_loss_kernel
        monkeypatch.setattr(train, "ppo_loss_kernel", lambda *a, **kw: (calls.append((a[0].detach(), a[11])), kernel(*a, **kw))[1])
    m, stats = run_update(pol, buf, optimizer, *route, clip_vf, normalize)
    if route == ROUTES[-1]:
        # no ratio or |dv| stands within the margin of an edge: the last minibatch clips the rows the f64 replay clips
        assert len(calls) == STEPS
        assert abs(float(stats["clip_fraction"]) - trace[-1]["clip_fraction"]) <= 1e-6
        if clip_vf is not None:
            values, old_values = calls[-1]
            got = float(((values - old_values).abs() > clip_vf).double().mean())
            print(f"last minibatch: clip fraction {float(stats['clip_fraction']):.4f} value-clipped {got:.4f}")
            assert abs(got - trace[-1]["vf_clip_fraction"]) <= 1e-6
    return hold_to_the_bound(p0, p32, p64, m)


@pytest.mark.parametrize("optimizer", sorted(OPTIMIZERS))
@pytest.mark.parametrize("route", ROUTES, ids="-".join)
def test_every_route_with_a_value_clip_lands_where_the_f64_replay_lands(collected, route, optimizer, monkeypatch):
    check_case(*collected, optimizer, route, "vf", monkeypatch)


@pytest.mark.parametrize("setting", ("raw", "vf_raw"))
@pytest.mark.parametrize("route", (ROUTES[0], ROUTES[-1]), ids="-".join)
def test_raw_advantages_land_where_the_f64_replay_lands(collected, route, setting, monkeypatch):
    check_case(*collected, "adam", route, setting, monkeypatch)
