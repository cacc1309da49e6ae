"""The host (NumPy) paths the reference's agents drive, after round 5's single-copy rework:
`HedgingVecEnv.step_wait` (SB3 collect_rollouts, train_ppo_v2.py:127-141,230) pulls obs,
reward and done flags in ONE pinned copy, episode ends in one more, and builds the info
dicts lazily; `HedgingEnv.step` (baselines.py:45-51) copies the env's whole io buffer once.
These tests hold the contract those shortcuts must keep: returned arrays are never
overwritten by later steps, an info list read late still shows its own step (terminal obs,
Monitor episode), and the NumPy path returns exactly what the device path produced."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
KW = dict(loss_type="abs", pnl_penalty_weight=0.001, lambda_cost=0.0001, theta_weight=0.0002, slippage_bps=1.0)
GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=5)
MON = ("per_share_step_pnl", "raw_pnl_deviation_abs", "transaction_costs_total")


def _pair(n, host_io="auto"):
    from cantorrl_amd.vec_env import HedgingVecEnv
    a = HedgingVecEnv(n, mode="gbm", generate=GEN, seed=21, device=DEV, monitor_keywords=MON, host_io=host_io, **KW)
    b = HedgingVecEnv(n, mode="gbm", generate=GEN, seed=21, device=DEV, return_numpy=False,
                      info_keys=MON + ("reward_step",), **KW)
    return a, b


@pytest.mark.parametrize("n,host_io", [(2, "auto"), (300, "auto"), (300, False), (5000, "auto"), (9000, "auto")])
def test_numpy_path_equals_device_path_and_late_infos_keep_their_step(n, host_io):
    """step_wait through the host-mapped block (host_io: n <= HOST_IO_MAX_ENVS by default) and through
    the device io buffer + one pinned DMA (n = 9000, or host_io=False) against step_tensors."""
    a, b = _pair(n, host_io)
    from cantorrl_amd.vec_env import HOST_IO_MAX_ENVS
    assert (a._hio is not None) == (host_io == "auto" and n <= HOST_IO_MAX_ENVS)
    oa = a.reset()
    ob = b.reset_tensors().cpu().numpy()
    assert np.array_equal(oa, ob)
    rng = np.random.default_rng(1)
    kept, rets = [], np.zeros(n)
    for s in range(12):
        act = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        a.step_async(act)
        obs, rew, done, infos = a.step_wait()
        o2, r2, t2, _ = b.step_tensors(torch.from_numpy(act).to(DEV))
        tobs_b = b._tobs.cpu().numpy().copy()
        info_b = {k: b.info_tensor(k).cpu().numpy().copy() for k in MON}
        rew64 = b.info_tensor("reward_step").cpu().numpy().copy()
        assert obs.dtype == np.float32 and obs.shape == (n, 13) and done.dtype == np.bool_
        assert np.array_equal(obs, o2.cpu().numpy()) and np.array_equal(rew, r2.cpu().numpy())
        assert np.array_equal(done, t2.cpu().numpy().astype(bool))
        # Monitor sums the env's f64 reward (train_ppo_v2.py:119, hedging_env_v2.py:262,294),
        # which the f32 VecEnv reward is the cast of
        assert np.array_equal(rew, rew64.astype(np.float32))
        rets += rew64
        # keep every array and the info list unread, across the later steps
        kept.append((obs, obs.copy(), rew, rew.copy(), done, done.copy(), infos, tobs_b, info_b, rets.copy()))
        rets[done] = 0.0
    for s, (obs, obs_c, rew, rew_c, done, done_c, infos, tobs_b, info_b, ret_s) in enumerate(kept):
        assert np.array_equal(obs, obs_c) and np.array_equal(rew, rew_c) and np.array_equal(done, done_c), s
        assert len(infos) == n
        for i in range(n):
            d = infos[i]
            assert d["TimeLimit.truncated"] is False
            assert "reward_step" not in d   # Monitor's hidden f64 column is not an info key here
            for k in MON:
                assert d[k] == info_b[k][i], (s, i, k)
            if done[i]:
                assert np.array_equal(d["terminal_observation"], tobs_b[i]), (s, i)
                ep = d["episode"]
                assert ep["l"] == 5 and ep["r"] == round(float(ret_s[i]), 6), (s, i, ep)
                assert ep["per_share_step_pnl"] == info_b["per_share_step_pnl"][i]
            else:
                assert "terminal_observation" not in d and "episode" not in d
    assert sum(int(k[4].sum()) for k in kept) == 2 * n   # steps 5 and 10 end every episode
    a.close()
    b.close()


@pytest.mark.parametrize("n", [2, 5])
def test_step_pointers_are_base_plus_layout_offset_and_both_paths_write_the_same_bytes(n):
    """The pointers he_step gets -- the device io buffer's (step_tensors) and the host-mapped block's
    (step_host) -- are base + the IoLayout offset of (n, info keys + Monitor's hidden reward_step), and
    a step() on one env and a step_host() on its twin leave identical bytes in the two buffers."""
    from cantorrl_amd import _lib
    from cantorrl_amd._layout import IoLayout
    from cantorrl_amd.vec_env import HedgingVecEnv
    a, b = (HedgingVecEnv(n, mode="gbm", generate=GEN, seed=21, device=DEV, monitor_keywords=MON, host_io=h, **KW)
            for h in (False, True))
    L = IoLayout(n, MON + ("reward_step",))
    # the device io buffer
    base = a._obs.data_ptr()
    assert a._hio is None
    assert a._info_flat.data_ptr() == base + L.info0 and a._info_flat.numel() == L.total - L.info0
    assert a._step_args[:4] == (base, base + L.reward, base + L.terminated, base + L.truncated)
    assert a._step_args[4] == a._tobs.data_ptr()
    assert [a._rew.data_ptr(), a._term.data_ptr(), a._trunc.data_ptr()] == list(a._step_args[1:4])
    assert list(a._info_t) == list(L.fields) and a._rew64 is a._info_t["reward_step"]
    # the host-mapped block: its device address is the obs pointer, its host address the io view's
    z = b._hio
    d = z.step_args[1]
    host = z.io.ctypes.data
    assert z.step_args[:6] == (d + L.actions, d, d + L.reward, d + L.terminated, d + L.truncated, d + L.terminal_obs)
    assert z.io.size == L.total and z.act.shape == (n, 2) and z.tobs.shape == (n, 13)
    assert z.act.ctypes.data == host + L.actions and z.tobs.ctypes.data == host + L.terminal_obs
    assert (z.d_flag, z.h_flag) == (d + L.flag, host + L.flag)
    assert a._step_args[5]._obj is a._info and z.step_args[6]._obj is z.info   # byref of the struct checked below
    for info, start in ((a._info, base), (z.info, d)):
        for k, _ in _lib.INFO_FIELDS:
            assert getattr(info, k) == (start + L.fields[k][1] if k in L.fields else None), k
    spans = [(0, L.truncated + n)] + [(o, o + nb) for _, o, nb in L.fields.values()]   # every byte a step writes
    # twin envs, the same actions: identical bytes through either path, episode ends included
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa, ob)
    rng = np.random.default_rng(5)
    for s in range(6):
        act = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        obs, rew, done, _ = a.step(act)
        io = b.step_host(act).io
        dev = a._io.cpu().numpy()
        for lo, hi in spans:
            assert dev[lo:hi].tobytes() == io[lo:hi].tobytes(), (s, lo)
        o2, r2, d2 = L.unpack(io)
        assert obs.tobytes() == o2.tobytes() and rew.tobytes() == r2.tobytes() and np.array_equal(done, d2)
        assert done.all() == (s == 4)
        if done.any():
            assert a._tobs.cpu().numpy().tobytes() == b._hio.tobs.tobytes()
    a.close()
    b.close()


def test_single_env_step_matches_vector_env_and_holds_no_aliases():
    """HedgingEnv.step's one copy per step returns the same obs / reward / info as the
    vector env's device path, and its returned obs is a private array."""
    from cantorrl_amd.env import HedgingEnv
    from cantorrl_amd.vec_env import HedgingVecEnv
    env = HedgingEnv(mode="gbm", generate=GEN, **KW)
    ref = HedgingVecEnv(1, mode="gbm", generate=GEN, seed=7, device=DEV, autoreset=False, return_numpy=False,
                        info_keys=("reward_step", "cash", "call_contracts", "portfolio_value"), **KW)
    o, _ = env.reset(seed=7)
    r0 = ref.reset_tensors().cpu().numpy()[0]
    assert np.array_equal(o, r0)
    prev = o
    prev_c = o.copy()
    for s in range(5):
        act = np.array([0.4, -0.7], np.float32) * (s + 1) / 5
        o, r, term, trunc, info = env.step(act)
        ob, rb, tb, _ = ref.step_tensors(torch.from_numpy(act).reshape(1, 2).to(DEV))
        assert np.array_equal(o, ob.cpu().numpy()[0])
        assert r == ref.info_tensor("reward_step").cpu().numpy()[0]
        assert info["cash"] == ref.info_tensor("cash").cpu().numpy()[0]
        assert info["call_contracts"] == ref.info_tensor("call_contracts").cpu().numpy()[0]
        assert term == bool(tb.cpu().numpy()[0]) and trunc is False
        assert np.array_equal(prev, prev_c)   # the last step's obs was not overwritten
        prev, prev_c = o, o.copy()
    assert term
    env.close()
    ref.close()


@pytest.mark.parametrize("n", [2, 3000])
def test_step_signal_raises_each_armed_step_once(n):
    """he_step_signal / he_signal_wait (the host_io step's completion): the armed step's kernel
    stores its sequence number after its outputs -- with 12 workgroups (n = 3000) only the last one
    to finish, its counter re-armed for the next step; an unarmed step leaves the word alone; the
    signal refuses a step with VecNormalize attached."""
    import ctypes
    from cantorrl_amd import _lib
    a, b = _pair(n)
    z = a._hio
    lib, h = a.lib, a._h
    flag = np.frombuffer((ctypes.c_uint32 * 1).from_address(z.h_flag), np.uint32)
    st = torch.cuda.current_stream().cuda_stream
    a.reset()
    b.reset_tensors()
    assert lib.he_signal_wait(h, z.h_flag, st) == _lib.HE_ESTATE   # nothing signalled yet
    assert lib.he_step_signal(h, z.d_flag + 1) == _lib.HE_EINVAL   # misaligned
    rng = np.random.default_rng(3)
    for s in range(1, 41):
        act = rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)
        obs, rew, done, _ = a.step(act)
        o2, r2, t2, _ = b.step_tensors(torch.from_numpy(act).to(DEV))
        assert lib.he_signal_seq(h) == s and int(flag[0]) == s
        assert np.array_equal(obs, o2.cpu().numpy()) and np.array_equal(rew, r2.cpu().numpy())
        assert np.array_equal(done, t2.cpu().numpy().astype(bool))
    # one-shot: a step nobody armed does not touch the word
    np.copyto(z.act, 0.0)
    assert lib.he_step(h, *z.step_args, st) == _lib.HE_OK
    torch.cuda.synchronize()
    assert int(flag[0]) == 40 and lib.he_signal_seq(h) == 40
    # an armed step that fails its argument checks consumes the arm too
    args = list(z.step_args)
    assert lib.he_step_signal(h, z.d_flag) == _lib.HE_OK
    assert lib.he_step(h, None, *args[1:], st) == _lib.HE_EINVAL
    assert lib.he_step(h, *z.step_args, st) == _lib.HE_OK
    torch.cuda.synchronize()
    assert int(flag[0]) == 40 and lib.he_signal_seq(h) == 40
    # armed again: the counter of the 12-workgroup grid was left at 0 by the last signalled step
    assert lib.he_step_signal(h, z.d_flag) == _lib.HE_OK
    assert lib.he_step(h, *z.step_args, st) == _lib.HE_OK
    assert lib.he_signal_wait(h, z.h_flag, st) == _lib.HE_OK and int(flag[0]) == 41
    # with VecNormalize armed the signal is refused (the launch would not end with the step)
    p = _lib.HeVecnormParams(obs_dim=13, training=1, norm_obs=1, norm_reward=1, gamma=0.99,
                             clip_obs=10.0, clip_reward=10.0, epsilon=1e-8)
    ret = torch.zeros(n, dtype=torch.float64, device=DEV)
    stats = torch.zeros(int(lib.he_vecnorm_stats_len(13)), dtype=torch.float64, device=DEV)
    scr = torch.zeros(int(lib.he_vecnorm_scratch_bytes(n, 13)), dtype=torch.uint8, device=DEV)
    assert lib.he_vecnorm_attach(h, ctypes.byref(p), ret.data_ptr(), stats.data_ptr(), scr.data_ptr()) == _lib.HE_OK
    assert lib.he_step_signal(h, z.d_flag) == _lib.HE_OK
    assert lib.he_step(h, *z.step_args, st) == _lib.HE_EINVAL
    assert b"VecNormalize" in lib.he_last_error(h)
    torch.cuda.synchronize()
    assert int(flag[0]) == 41
    a.close()
    b.close()


def test_signal_wait_behind_long_work_falls_back_to_the_stream():
    """he_signal_wait on a step queued behind ~1 ms of other work on the same stream: the host's
    spin (200 us) runs out, the stream synchronize takes over, and the flag then holds the step."""
    import ctypes
    import time
    from cantorrl_amd import _lib
    from cantorrl_amd.vec_env import HedgingVecEnv
    a, b = _pair(2)
    b.close()
    z = a._hio
    lib, h = a.lib, a._h
    flag = np.frombuffer((ctypes.c_uint32 * 1).from_address(z.h_flag), np.uint32)
    st = torch.cuda.current_stream().cuda_stream
    a.reset()
    a.step(np.zeros((2, 2), np.float32))   # the first armed step allocates the counter (a device sync)
    big = HedgingVecEnv(65536, mode="gbm", generate=GEN, seed=3, device=DEV, return_numpy=False, info_keys=(), **KW)
    big.reset_tensors()
    acts = torch.rand((256, 65536, 2), device=DEV) * 2 - 1
    outs = big.rollout(acts)    # the output buffers allocated (a fresh hipMalloc synchronizes)
    torch.cuda.synchronize()
    for _ in range(4):          # ~1 ms of rollouts ahead of the step on the same stream
        big.rollout(acts, *outs)
    np.copyto(z.act, 0.25)
    seq = lib.he_signal_seq(h) + 1
    assert lib.he_step_signal(h, z.d_flag) == _lib.HE_OK
    assert lib.he_step(h, *z.step_args, st) == _lib.HE_OK
    t0 = time.perf_counter()
    assert lib.he_signal_wait(h, z.h_flag, st) == _lib.HE_OK
    waited = time.perf_counter() - t0
    assert int(flag[0]) == seq == lib.he_signal_seq(h)
    assert waited > 200e-6   # the rollouts were still running when the wait began
    big.close()
    a.close()
