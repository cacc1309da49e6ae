"""RecurrentPPOModule.evaluate_actions and ppo_update on the GPU, against what the RolloutCollector
stored and against the all-torch f32 composition of the module's tensors (tests/_ppo_reference.py: the
LSTM as sb3_contrib's Python loop of one cell per time step, the heads and the loss from their
formulas).  Bounds are measured: the all-torch f32 composition's own error against the same
reference, times 4 (as DESIGN 18 and 19)."""
import copy

import pytest

import _ppo_reference as ref
from test_actor_gpu import gbm_env
from test_policy_collect_cpu import critic_golden, make_policy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402
from cantorrl_amd.agent import STATE_NAMES  # noqa: E402
from cantorrl_amd.collect import RolloutCollector  # noqa: E402

DEV = "cuda:0"
HYPER = dict(clip_range=0.3, ent_coef=1e-5, vf_coef=0.5, max_grad_norm=0.5)


def loop_evaluate(m, obs, actions, es, states0):
    """evaluate_actions over module m's tensors (f32 or f64) from torch ops alone: the restatement, which
    calls nothing of the module's."""
    return ref.evaluate(dict(m.named_parameters()), ref.constants(m), obs, actions, es, states0)


def rollout(n=33, K=16, states=True, seed=42):
    c = critic_golden()
    pol = make_policy("golden", device=DEV)   # the checkpoint's statistics on the raw obs
    venv = gbm_env(n, seed, ("per_share_step_pnl",))
    col = RolloutCollector(venv, pol, float(c["gamma"]), float(c["gae_lambda"]), seed=9)
    col.collect(3)                            # begin mid-episode (episode_length 8), from non-zero states
    buf = col.collect(K, states=states)
    torch.cuda.synchronize()
    return pol, venv, col, buf


def states0(buf):
    return tuple(getattr(buf, s) for s in STATE_NAMES)


def test_evaluate_actions_reproduces_the_buffer():
    pol, venv, col, buf = rollout()
    assert buf.episode_starts.sum() >= 33 and buf.h_vf.abs().mean() > 0
    m = train.RecurrentPPOModule.from_policy(pol)
    with torch.no_grad():
        v, lp, ent = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))
        tv, tlp, _ = loop_evaluate(m, buf.observations, buf.actions, buf.episode_starts, states0(buf))
    ev, elp = float((v - buf.values).abs().max()), float((lp - buf.log_probs).abs().max())
    dv, dlp = float((tv - buf.values).abs().max()), float((tlp - buf.log_probs).abs().max())
    print(f"values: module {ev:.3e} all-torch {dv:.3e}; log_prob: module {elp:.3e} all-torch {dlp:.3e}")
    assert dv > 0.0 and dlp > 0.0
    assert ev <= 4 * dv, (ev, dv)
    assert elp <= 4 * dlp, (elp, dlp)
    assert v.shape == lp.shape == ent.shape == (16, 33) and torch.isfinite(ent).all()
    venv.close()
    pol.close()


def clipped_grads(m, buf):
    """The gradient RecurrentPPO.train takes for the whole buffer as one minibatch, from torch ops
    alone in m's dtype, after the gradient-norm clip."""
    dt = m.log_std.dtype
    v, lp, ent = loop_evaluate(m, buf.observations, buf.actions, buf.episode_starts, states0(buf))
    loss, _ = ref.loss(v, lp, ent, buf.log_probs.to(dt), buf.advantages.to(dt), buf.returns.to(dt),
                       HYPER["clip_range"], HYPER["ent_coef"], HYPER["vf_coef"])
    m.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(list(m.parameters()), HYPER["max_grad_norm"])
    return {k: p.grad.detach().to(torch.float64) for k, p in m.named_parameters()}


def test_one_sgd_minibatch_moves_the_parameters_by_the_all_torch_gradient():
    pol, venv, col, buf = rollout()
    lr = 1e-2
    m = train.RecurrentPPOModule.from_policy(pol)
    g32 = clipped_grads(copy.deepcopy(m), buf)
    g64 = clipped_grads(copy.deepcopy(m).double(), buf)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    stats = train.ppo_update(m, torch.optim.SGD(m.parameters(), lr=lr), buf, n_epochs=1, **HYPER)
    torch.cuda.synchronize()
    assert len(before) == 21
    for k, p in m.named_parameters():
        d_ref = float((g32[k] - g64[k]).abs().max())
        moved = p.detach().double() - before[k].double()
        err = float((moved + lr * g32[k]).abs().max())
        # the step itself rounds once to f32: at most one ulp of the tensor's largest parameter
        ulp = float(torch.finfo(torch.float32).eps * before[k].abs().max())
        print(f"{k}: |step + lr g32| {err:.3e}; lr 4 d_ref {4 * lr * d_ref:.3e}; |lr g32| {lr * float(g32[k].abs().max()):.3e}")
        assert float(g32[k].abs().max()) > 0.0, k
        assert err <= 4 * d_ref * lr + ulp, (k, err, d_ref)
    assert set(stats) >= {"loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction",
                          "grad_norm", "mean_loss"}
    for k, v in stats.items():
        assert v.device.type == "cuda" and v.dim() == 0 and bool(torch.isfinite(v)), k
    venv.close()
    pol.close()


def test_window_needs_stored_states_and_a_divisor():
    pol, venv, col, buf = rollout(n=2, K=8, states=False)
    m = train.RecurrentPPOModule.from_policy(pol)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="states=True"):
        train.ppo_update(m, opt, buf, n_epochs=1, window=4)
    with pytest.raises(ValueError, match="divide"):
        train.ppo_update(m, opt, buf, n_epochs=1, window=3)
    stats = train.ppo_update(m, opt, buf, n_epochs=1, window=8, envs_per_batch=1)   # the whole K needs none
    assert bool(torch.isfinite(stats["mean_loss"]))
    venv.close()
    pol.close()


def test_collect_update_load_collect_cycle():
    pol, venv, col, buf = rollout()
    m = train.RecurrentPPOModule.from_policy(pol)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-5)
    with torch.no_grad():
        v0 = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))[0].clone()
    gen = torch.Generator(device=DEV).manual_seed(3)
    stats = train.ppo_update(m, opt, buf, n_epochs=2, envs_per_batch=16, window=8, generator=gen, **HYPER)
    with torch.no_grad():
        v1 = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))[0]
    assert all(bool(torch.isfinite(v)) for v in stats.values())
    assert float((v1 - v0).abs().max()) > 1e-4          # the update changed the critic
    pol.load_state_dict(m.state_dict())
    buf2 = col.collect(16, states=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        v2, lp2, _ = m.evaluate_actions(buf2.observations, buf2.actions, buf2.episode_starts, states0(buf2))
    # the collector now runs the updated tensors: the module reproduces what it stored
    assert torch.isfinite(buf2.values).all()
    assert float((v2 - buf2.values).abs().max()) <= 1e-4 * max(1.0, float(buf2.values.abs().max()))
    ckpt = make_policy("golden", device=DEV)
    m0 = train.RecurrentPPOModule.from_policy(ckpt)
    with torch.no_grad():
        old = m0.evaluate_actions(buf2.observations, buf2.actions, buf2.episode_starts, states0(buf2))[0]
    assert float((old - buf2.values).abs().max()) > 1e-4   # and the checkpoint's own tensors do not
    venv.close()
    pol.close()
