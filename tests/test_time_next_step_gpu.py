"""he_time_next_step on every route that honours it: the armed handle's next step-kernel
dispatch goes out bracketed by the caller's two HIP events, and by nothing else does it
differ from the plain launch.  Per route two handles with the same seed, one armed, one not:
their outputs and state blobs are bit-equal, the events give a positive elapsed time, and a
later un-armed call leaves that time as it was (the arm is one-shot).

n = 65 envs: two LDS workgroups (the second with one live lane), one step workgroup; K = 9
steps: one full 8-slot LDS block and a one-step tail; episodes of 8 steps end inside the call
and make the replay table LDS-eligible."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
N, K, T = 65, 9, 8
KW = dict(loss_type="abs", pnl_penalty_weight=0.001, lambda_cost=0.0001, theta_weight=0.0002, slippage_bps=1.0)
GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=T)

# route: (he_step or he_rollout, replay table, info keys, VecNormalize training flag, environment)
ROUTES = {
    "step": ("step", False, (), None, {}),
    "step_info": ("step", False, ("reward_step",), None, {}),
    "step_vecnorm_train": ("step", False, (), True, {}),
    "step_vecnorm_eval": ("step", False, (), False, {}),
    "rollout_lds": ("rollout", False, (), None, {}),
    "rollout_fused_market": ("rollout", False, (), None, {"HE_LDS_ROLLOUT": "0"}),
    "rollout_side_stream": ("rollout", False, (), None, {"HE_LDS_ROLLOUT": "0", "HE_FUSED_MARKET": "0"}),
    "rollout_replay_lds": ("rollout", True, (), None, {}),
}


class _Handle:
    """One env (under DeviceVecNormalize where the route asks for it) and its driver."""

    def __init__(self, replay, info_keys, vn_training):
        from cantorrl_amd.vec_env import HedgingVecEnv
        if replay:
            import bench
            self.env = HedgingVecEnv(N, tables=bench.replay_tables(paths=64, cols=T + 1), seed=11, device=DEV,
                                     return_numpy=False, info_keys=info_keys, **KW)
        else:
            self.env = HedgingVecEnv(N, mode="gbm", generate=GEN, seed=11, device=DEV, return_numpy=False,
                                     info_keys=info_keys, **KW)
        self.top = self.env
        if vn_training is not None:
            from cantorrl_amd.vec_normalize import DeviceVecNormalize
            self.top = DeviceVecNormalize(self.env, training=vn_training)
        self.top.reset_tensors()

    def steps(self, acts):
        """he_step per row of acts: every step's raw (and VecNormalize) outputs, on the host."""
        out = []
        for a in acts:
            if self.top is self.env:
                res = self.env.step_tensors(a)[:3]
            else:
                res = self.top.step_tensors(a, info=False)[:3] + (self.env._obs, self.env._rew)
            out.append([t.cpu().numpy().copy() for t in res])
        return out

    def rollout(self, acts):
        return [[t.cpu().numpy().copy() for t in self.env.rollout(acts)]]

    def close(self):
        self.env.close()


def _same(x, y):
    return len(x) == len(y) and all(p.tobytes() == q.tobytes() for s, t in zip(x, y) for p, q in zip(s, t))


@pytest.mark.parametrize("route", list(ROUTES))
def test_armed_dispatch_is_timed_once_and_computes_the_same(route, monkeypatch):
    import bench
    api, replay, info_keys, vn_training, environ = ROUTES[route]
    for k, v in environ.items():
        monkeypatch.setenv(k, v)
    hev = bench.HipEvents()
    e0, e1 = hev.create(), hev.create()
    armed, plain = _Handle(replay, info_keys, vn_training), _Handle(replay, info_keys, vn_training)
    acts = torch.rand((2 * K, N, 2), device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 2 - 1
    if api == "step":   # the first he_step armed, the other K - 1 not
        first, second = acts[:1], acts[1:K]
        run = lambda h, a: h.steps(a)
    else:               # the first he_rollout of K steps armed, the second not
        first, second = acts[:K], acts[K:]
        run = lambda h, a: h.rollout(a)
    assert armed.env.lib.he_time_next_step(armed.env._h, e0, e1) == 0
    got, want = run(armed, first), run(plain, first)
    torch.cuda.synchronize()
    ms = hev.elapsed_ms(e0, e1)   # (b) both events were recorded: raises otherwise
    assert ms > 0.0
    got += run(armed, second)
    want += run(plain, second)
    torch.cuda.synchronize()
    assert hev.elapsed_ms(e0, e1) == ms   # (c) one-shot: the later dispatches left the events alone
    assert _same(got, want)   # (a)
    assert any(s[2].any() for s in got)   # episodes ended inside the calls
    assert np.array_equal(armed.env.get_state(), plain.env.get_state())
    hev.destroy(e0, e1)
    armed.close()
    plain.close()
