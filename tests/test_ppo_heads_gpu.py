"""ha_ppo_heads_forward / _backward on the GPU (heads_pack_kernel, heads_fwd_kernel, heads_bwd_kernel,
heads_lsd_kernel) against the host build of the same contract (H1-H6 of include/hedge_actor.h) bit for bit; on
a freshly collected buffer, where evaluate_actions(heads="kernel") returns the buffer's own values and
log_probs; and inside ppo_update: a collect -> update -> refresh -> collect cycle whose first minibatch agrees
with heads="torch" within 4 x d_ref plus one f32 ulp, worded as test_ppo_loss_kernel_gpu.py words it: d_ref the
torch path's (torch heads, torch loss: the code before this path existed) own distance from the f64
restatement of the loss on that path's f32 inputs.

Not the reference here: the f64 restatement of evaluate_actions itself (tests/_ppo_reference.evaluate).  Its
log_prob is 1.6e-5 away from the buffer's, which is the step kernel's f32 rounding of a cancelling a - mean, so
its first-epoch ratio is not 1 and its policy term not -mean(A').  With the kernel heads the ratio is exactly 1,
as the definition says; measured on one MI355X, loss: kernel heads 0.23105229, torch heads 0.23105204, that f64
run 0.23105206.  The test prints both."""
import numpy as np
import pytest

import _ppo_heads_contract as hc
import _ppo_loss_contract as lc
import _ppo_reference as ref
from test_ppo_heads_cpu import bits, tensors
from test_ppo_loss_kernel_cpu import CLIP, CLIP_VF, ENT, VF
from test_ppo_loss_kernel_gpu import first_minibatch
from test_ppo_update_gpu import HYPER as UPDATE_HYPER, rollout, states0

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402

DEV = "cuda:0"
DEVICE_R = (1, 31, 32, 33, 65, 1025, 2051)


def device_both(w, act, x):
    """train.ppo_heads_forward, then train.ppo_heads_backward on its saved tensors, on the device -> one dict
    of f32 arrays."""
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    tw = [torch.from_numpy(w[k]).to(DEV) for k in hc.TENSORS]
    f = train.ppo_heads_forward(t["h_pi"], t["h_vf"], t["actions"], tw, act)
    b = train.ppo_heads_backward(t["d_values"], t["d_log_prob"], t["d_entropy"], t["actions"],
                                 {k: f[k] for k in hc.BWD_IN[4:]}, tw, act)
    return {k: v.cpu().numpy() for k, v in dict(f, **b).items()}


@pytest.mark.parametrize("act", ("tanh", "relu"))
@pytest.mark.parametrize("kind", ("golden", "random"))
def test_device_equals_the_host_build_bitwise(kind, act):
    w = tensors(kind)
    for R in DEVICE_R:
        x = hc.rows(R, seed=2000 + R)
        want = hc.host_both(w, act, x)
        got = device_both(w, act, x)
        assert set(got) == set(hc.FWD_OUT + hc.BWD_OUT)
        for k in hc.FWD_OUT + hc.BWD_OUT:
            assert got[k].shape == want[k].shape and np.isfinite(want[k]).all(), (R, k)
            assert np.array_equal(bits(got[k]), bits(want[k])), (R, k, np.abs(got[k] - want[k]).max())


@pytest.fixture(scope="module")
def collected():
    pol, venv, col, buf = rollout()
    yield pol, col, buf
    venv.close()
    pol.close()


def test_evaluate_actions_returns_the_collected_buffers_own_values_and_log_probs(collected):
    pol, col, buf = collected
    assert (buf.k_steps, buf.n_envs) == (16, 33) and buf.episode_starts.sum() >= 33
    m = train.RecurrentPPOModule.from_policy(pol, heads="kernel")
    with torch.no_grad():
        v, lp, ent = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))
    torch.testing.assert_close(v, buf.values, rtol=0, atol=0)
    torch.testing.assert_close(lp, buf.log_probs, rtol=0, atol=0)
    assert torch.equal(v.view(torch.int32), buf.values.view(torch.int32))
    assert torch.equal(lp.view(torch.int32), buf.log_probs.view(torch.int32))
    stats, _ = train.ppo_loss_kernel(v, lp, ent, buf.log_probs, buf.advantages, buf.returns, CLIP, ENT, VF)
    assert float(stats["approx_kl"]) == 0.0 and float(stats["clip_fraction"]) == 0.0
    # the torch heads do not: the reason for this path
    with torch.no_grad():
        tv, tlp, _ = train.RecurrentPPOModule.from_policy(pol).evaluate_actions(buf.observations, buf.actions,
                                                                                buf.episode_starts, states0(buf))
    print(f"torch heads: values off by {float((tv - buf.values).abs().max()):.3e}, "
          f"log_prob by {float((tlp - buf.log_probs).abs().max()):.3e}")


def first_minibatch_f64(pol, buf, seed):
    """The first minibatch of ppo_update(n_epochs=1) with one group and one window, evaluated by the f64
    restatement (tests/_ppo_reference.evaluate) -> f64 tensors of lc.INPUTS and old_values."""
    m = train.RecurrentPPOModule.from_policy(pol)
    perm = torch.randperm(buf.n_envs, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    mb = train.minibatch(buf, perm, 0, buf.k_steps)
    with torch.no_grad():
        v, lp, ent = ref.evaluate(ref.parameters(m, torch.float64), ref.constants(m), mb["observations"], mb["actions"],
                                  mb["episode_starts"], mb["states0"])
    t = dict(values=v, log_prob=lp, entropy=ent, old_log_prob=mb["log_probs"], advantages=mb["advantages"],
             returns=mb["returns"], old_values=buf.values.index_select(1, perm))
    return {k: x.reshape(-1).double() for k, x in t.items()}


def test_collect_update_refresh_collect_cycle_with_the_kernel_heads(collected):
    pol, col, buf = collected
    hyper = dict(UPDATE_HYPER, clip_range_vf=CLIP_VF)
    first = {}
    for heads, loss, wg in (("torch", "torch", "torch"), ("kernel", "kernel", "kernel")):
        m = train.RecurrentPPOModule.from_policy(pol, heads=heads, weight_grads=wg)
        opt = train.DeviceAdam(m.parameters(), lr=1e-3, eps=1e-5)
        first[heads] = train.ppo_update(m, opt, buf, n_epochs=1, loss=loss,
                                        generator=torch.Generator(device=DEV).manual_seed(3), **hyper)
    x = {k: v.reshape(-1).cpu().numpy() for k, v in first_minibatch(pol, buf, 3).items()}   # the torch heads' outputs
    want = lc.contract(x, CLIP, ENT, VF, True, CLIP_VF)[0]
    whole = lc.torch_loss_clipped(ref, first_minibatch_f64(pol, buf, 3), CLIP, ENT, VF, True, CLIP_VF)[1]
    for k in ("loss", "value_loss", "approx_kl"):
        got, base = float(first["kernel"][k]), float(first["torch"][k])
        d_ref = abs(base - float(want[k]))
        ulp = float(np.spacing(np.float32(abs(want[k]))))
        print(f"{k}: kernel heads {got!r} torch heads {base!r} f64 loss {float(want[k])!r} d_ref {d_ref:.3e} ulp {ulp:.3e}; "
              f"f64 through evaluate_actions {float(whole[k])!r}")
        assert abs(got - base) <= 4 * d_ref + ulp, (k, got, base, d_ref, ulp)
    assert float(first["kernel"]["approx_kl"]) == 0.0              # the first epoch's ratio is exactly 1
    # the cycle: 2 epochs x 3 groups x 2 windows, every part of the update a kernel, then the refreshed policy
    m = train.RecurrentPPOModule.from_policy(pol, heads="kernel", weight_grads="kernel")
    opt = train.DeviceAdam(m.parameters(), lr=1e-3, eps=1e-5)
    with torch.no_grad():
        v0 = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))[0].clone()
    stats = train.ppo_update(m, opt, buf, n_epochs=2, envs_per_batch=16, window=8, loss="kernel",
                             generator=torch.Generator(device=DEV).manual_seed(3), **hyper)
    assert set(stats) >= set(lc.STATS) | {"grad_norm", "mean_loss"}
    assert all(v.device.type == "cuda" and v.dim() == 0 and bool(torch.isfinite(v)) for v in stats.values()), stats
    assert int(opt.state[m.log_std]["step"]) == 12
    with torch.no_grad():
        v1 = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))[0]
    assert float((v1 - v0).abs().max()) > 1e-4                      # the update changed the critic
    pol.load_device_state_dict(m.state_dict())
    buf2 = col.collect(16, states=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        v2, lp2, _ = m.evaluate_actions(buf2.observations, buf2.actions, buf2.episode_starts, states0(buf2))
    assert torch.isfinite(buf2.values).all() and torch.isfinite(buf2.log_probs).all()
    assert torch.equal(v2.view(torch.int32), buf2.values.view(torch.int32))       # the refreshed policy's bits again
    assert torch.equal(lp2.view(torch.int32), buf2.log_probs.view(torch.int32))
