"""ha_ppo_loss on the GPU (loss_mean_kernel, loss_spread_kernel, loss_rows_kernel, loss_stats_kernel)
against the host build of the same contract (L1-L6 of include/hedge_actor.h) bit for bit, against
tests/_ppo_reference.loss_numpy on a real minibatch of the collector's buffer within the bound of
test_ppo_loss_kernel_cpu.py, and inside ppo_update: a collect -> update -> refresh -> collect cycle with
loss="kernel" and a value clip, whose first minibatch agrees with loss="torch" within 4 x d_ref plus one
f32 ulp, d_ref the torch path's own distance from the f64 restatement on those inputs."""
import numpy as np
import pytest

import _ppo_loss_contract as lc
import _ppo_reference as ref
from test_ppo_loss_kernel_cpu import BITWISE_N, CLIP, CLIP_VF, ENT, HYPER, VF, bits, cases
from test_ppo_update_gpu import HYPER as UPDATE_HYPER, rollout, states0

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402

DEV = "cuda:0"
F64 = np.float64


def device_loss(x, normalize, clip_vf, shape=None):
    """train.ppo_loss_kernel over the arrays of x on the device -> (stats [8] f32, {name: f32 gradient})."""
    t = {k: torch.from_numpy(v).to(DEV) for k, v in x.items()}
    if shape is not None:
        t = {k: v.reshape(shape) for k, v in t.items()}
    stats, grads = train.ppo_loss_kernel(*(t[k] for k in lc.INPUTS), CLIP, ENT, VF, normalize, clip_vf,
                                         None if clip_vf is None else t["old_values"])
    return (torch.stack([stats[k] for k in lc.STATS]).cpu().numpy(),
            {k: g.reshape(-1).cpu().numpy() for k, g in zip(lc.GRADS, grads)})


@pytest.mark.parametrize("clip_vf", (None, CLIP_VF))
@pytest.mark.parametrize("normalize", (True, False))
def test_device_equals_the_host_build_bitwise(normalize, clip_vf):
    inputs = {f"quantised{N}": lc.quantised_inputs(N, seed=100 + N) for N in BITWISE_N}
    inputs.update(cases())
    assert inputs["two_blocks"]["values"].size == 2 * lc.BLOCK + 3
    for name, x in inputs.items():
        st, want_stats, want_grads = lc.host_loss(x, normalize_advantage=normalize, clip_range_vf=clip_vf, **HYPER)
        assert st == 0
        stats, grads = device_loss(x, normalize, clip_vf)
        for j, k in enumerate(lc.STATS):
            assert bits(stats[j]) == bits(want_stats[j]), (name, k, stats[j], want_stats[j])
        for k in lc.GRADS:
            assert np.array_equal(bits(grads[k]), bits(want_grads[k])), (name, k)


@pytest.mark.parametrize("normalize", (True, False))
def test_device_equals_the_host_build_bitwise_beyond_one_staging_pass_of_block_sums(normalize):
    """The kernels add the blocks' sums from LDS 512 blocks at a time: 514 blocks take two passes."""
    x = lc.random_inputs(513 * lc.BLOCK + 5, 31)
    st, want_stats, want_grads = lc.host_loss(x, normalize_advantage=normalize, clip_range_vf=CLIP_VF, **HYPER)
    assert st == 0 and np.isfinite(want_stats).all() and 0.05 < want_stats[5] < 0.95
    stats, grads = device_loss(x, normalize, CLIP_VF)
    assert np.array_equal(bits(stats), bits(want_stats)), (stats, want_stats)
    for k in lc.GRADS:
        assert np.array_equal(bits(grads[k]), bits(want_grads[k])), k


@pytest.fixture(scope="module")
def collected():
    pol, venv, col, buf = rollout()
    yield pol, col, buf
    venv.close()
    pol.close()


def first_minibatch(pol, buf, seed):
    """What ppo_update(n_epochs=1) with one group and one window evaluates first: the module's outputs on
    the envs in the order of the generator's permutation, as f32 arrays, and the rows' old values."""
    m = train.RecurrentPPOModule.from_policy(pol)
    perm = torch.randperm(buf.n_envs, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    mb = train.minibatch(buf, perm, 0, buf.k_steps)
    with torch.no_grad():
        v, lp, ent = m.evaluate_actions(mb["observations"], mb["actions"], mb["episode_starts"], mb["states0"])
    t = dict(values=v, log_prob=lp, entropy=ent, old_log_prob=mb["log_probs"], advantages=mb["advantages"],
             returns=mb["returns"], old_values=buf.values.index_select(1, perm))
    return {k: x.contiguous() for k, x in t.items()}


def test_a_real_minibatch_against_loss_numpy(collected):
    pol, col, buf = collected
    assert (buf.k_steps, buf.n_envs) == (16, 33)
    t = first_minibatch(pol, buf, 3)
    stats, grads = train.ppo_loss_kernel(*(t[k] for k in lc.INPUTS), **HYPER)
    assert all(tuple(g.shape) == (16, 33) for g in grads)
    x = {k: v.reshape(-1).cpu().numpy() for k, v in t.items()}
    want_stats, want_grads = ref.loss_numpy(*(x[k] for k in lc.INPUTS), CLIP, ENT, VF)
    for k in lc.STATS[:6]:
        got = stats[k].cpu().numpy()
        print(f"{k}: kernel {got!r} loss_numpy {want_stats[k]!r}")
        assert lc.within_one_ulp(got, want_stats[k], 2.0 ** -48 if k == "approx_kl" else 0.0), (k, got, want_stats[k])
    for k, g in zip(lc.GRADS, grads):
        assert lc.within_one_ulp(g.reshape(-1).cpu().numpy(), want_grads[k]), k
    assert float(stats["adv_std"]) > 0.0 and np.count_nonzero(x["values"]) == x["values"].size


def test_collect_update_refresh_collect_cycle_with_the_kernel_loss(collected):
    pol, col, buf = collected
    hyper = dict(UPDATE_HYPER, clip_range_vf=CLIP_VF)
    # the first minibatch from the same start, either loss path: one group of all envs, the whole K
    first = {}
    for loss in train.LOSSES:
        m = train.RecurrentPPOModule.from_policy(pol)
        opt = train.DeviceAdam(m.parameters(), lr=1e-3, eps=1e-5)
        first[loss] = train.ppo_update(m, opt, buf, n_epochs=1, loss=loss,
                                       generator=torch.Generator(device=DEV).manual_seed(3), **hyper)
    x = {k: v.reshape(-1).cpu().numpy() for k, v in first_minibatch(pol, buf, 3).items()}
    want = lc.contract(x, CLIP, ENT, VF, True, CLIP_VF)[0]
    for k in ("loss", "value_loss", "approx_kl"):
        got, base = float(first["kernel"][k]), float(first["torch"][k])
        d_ref = abs(base - float(want[k]))
        ulp = float(np.spacing(np.float32(abs(want[k]))))
        print(f"{k}: kernel {got!r} torch {base!r} f64 {float(want[k])!r} d_ref {d_ref:.3e} ulp {ulp:.3e}")
        assert abs(got - base) <= 4 * d_ref + ulp, (k, got, base, d_ref, ulp)
    # the cycle: 2 epochs x 3 groups x 2 windows with the kernel loss and DeviceAdam, then the refreshed policy
    m = train.RecurrentPPOModule.from_policy(pol)
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
        v2 = m.evaluate_actions(buf2.observations, buf2.actions, buf2.episode_starts, states0(buf2))[0]
    assert torch.isfinite(buf2.values).all()
    assert float((v2 - buf2.values).abs().max()) <= 1e-4 * max(1.0, float(buf2.values.abs().max()))
