"""StackedRecurrentActor on the GPU: stack_step_kernel against the host build of the same arithmetic
(ha_host_stack_step) bit for bit in every output and every state layer -- what catches a wrong fragment
order, a missed barrier between layers or a stale recurrent half -- and the closed loop of
evaluate_actor at 128 x 1 against RecurrentActor's."""
import numpy as np
import pytest

from test_stacked_actor_cpu import CLIP, STEPS, host_sequence, make_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd.agent import RECORD_INFO_KEYS, RecurrentActor, StackedRecurrentActor  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("n", [1, 33, 70])   # one env, a ragged second tile, a third tile
@pytest.mark.parametrize("hid,nl", [(128, 1), (128, 2), (256, 1), (512, 4)])
def test_device_step_equals_host_build_bitwise(hid, nl, n):
    sd, stats, obs, start, _ = make_case(hid, nl, n)
    actor = StackedRecurrentActor.from_state_dict(sd, normalization=stats, clip_obs=CLIP, device=DEV)
    exp = host_sequence(actor, obs, start, n)
    actor.reset_states(n)
    for t in range(STEPS):
        dm = torch.full((n, 2), 7.0, device=DEV)
        dx = torch.full((n, 13), 7.0, device=DEV)
        da = actor.step(torch.from_numpy(obs[t]).to(DEV), torch.from_numpy(start[t]).to(DEV), mean_out=dm, obs_norm_out=dx)
        torch.cuda.synchronize()
        for k, v in dict(actions=da, mean=dm, obs_norm=dx, h=actor.h, c=actor.c).items():
            assert np.array_equal(v.cpu().numpy().view(np.uint32), exp[k][t].view(np.uint32)), (k, t)
    assert actor.h.shape == (nl, n, hid) and 0.0 < np.abs(exp["h"][-1]).mean() < 1.0
    actor.close()


def test_evaluate_actor_at_128_x_1_gives_recurrent_actor_records():
    from cantorrl_amd.vec_env import HedgingVecEnv
    sd, stats, _, _, _ = make_case(128, 1, 1)
    recs = []
    for cls in (RecurrentActor, StackedRecurrentActor):
        actor = cls.from_state_dict(sd, device=DEV)
        venv = HedgingVecEnv(64, mode="gbm", seed=11, info_keys=RECORD_INFO_KEYS, return_numpy=False, device=DEV,
                             generate=dict(s0=496.48, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=8))
        r = venv.evaluate_actor(actor, 128, chunk=8)
        recs.append(r[np.argsort(r["env_id"], kind="stable")])
        venv.close()
        actor.close()
    assert recs[0].shape == (128,) and np.abs(recs[0]["reward_sum"]).min() > 0.0
    assert recs[0].tobytes() == recs[1].tobytes()
