"""train.ppo_update on the GPU against tests/_ppo_reference.replay run on the device in torch f64, as
test_ppo_replay_cpu.py does on the host build: the collector's buffer of test_ppo_update_gpu.rollout()
(33 envs = one 32-env tile plus one, 16 steps, stored states), 2 epochs of groups of 16 envs x windows of
8 steps = 12 optimizer steps, torch.optim.SGD and train.DeviceAdam, either weight_grads mode; and the
LSTM kernels over a window from minibatch's states against the same rows of the whole sequence.

Bound: per tensor max |p_device - p_f64| <= 4 d_ref + ulp, d_ref = max |p_f32 - p_f64| between the two
all-torch replays, ulp = 2^-23 max |p_initial|."""
import pytest

import _ppo_reference as ref
from test_ppo_update_gpu import HYPER, rollout, states0

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402

DEV = "cuda:0"
OPTIMIZERS = {"sgd": 1e-2, "adam": 1e-4}   # name -> lr
EPOCHS, PER, W, STEPS = 2, 16, 8, 12
PERM_SEED = 3
POOLED = ()                                # groups of tensors that share a d_ref (none needed)
_REPLAY = {}


@pytest.fixture(scope="module")
def collected():
    pol, venv, col, buf = rollout()
    yield pol, buf
    venv.close()
    pol.close()


def replays(pol, buf, optimizer):
    """(initial parameters, the f32 replay, the f64 replay, the f64 replay's trace), computed once."""
    if optimizer not in _REPLAY:
        p0 = ref.parameters(train.RecurrentPPOModule.from_policy(pol), torch.float64)
        trace = []
        run = lambda dt, tr: ref.replay(p0, buf, dt, optimizer, OPTIMIZERS[optimizer], EPOCHS, PER, W, PERM_SEED, HYPER,
                                        ref.constants(pol), trace=tr)
        _REPLAY[optimizer] = (p0, run(torch.float32, None), run(torch.float64, trace), trace)
    return _REPLAY[optimizer]


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
    p0, p32, p64, trace = replays(pol, buf, optimizer)
    assert len(trace) == STEPS
    edge, small, fractions = ref.check_replay_inputs(trace, HYPER["clip_range"])
    print(f"closest ratio to a clip edge {edge:.2e}; smallest |A| {small:.2e}; clip fractions "
          + " ".join(f"{f:.2f}" for f in fractions))
    m = train.RecurrentPPOModule.from_policy(pol, weight_grads=mode)
    lr, count = OPTIMIZERS[optimizer], [0]
    if optimizer == "sgd":
        opt = torch.optim.SGD(m.parameters(), lr=lr)
        opt.register_step_post_hook(lambda *a: count.__setitem__(0, count[0] + 1))
    else:
        opt = train.DeviceAdam(m.parameters(), lr=lr, eps=1e-5)
    train.ppo_update(m, opt, buf, n_epochs=EPOCHS, envs_per_batch=PER, window=W,
                     generator=torch.Generator(device=DEV).manual_seed(PERM_SEED), **HYPER)
    torch.cuda.synchronize()
    if optimizer == "adam":
        steps = {int(opt.state[p]["step"]) for p in m.parameters()}
        assert len(steps) == 1
        count[0] = steps.pop()
    assert count[0] == STEPS
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
