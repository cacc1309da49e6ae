"""DeviceVecNormalize's one-launch host route (host_io: he_vecnorm_attach_step + he_step_signal,
step1_vnw_kernel) on the GPU: step_wait through host-mapped memory against the unchanged route
(host_io=False: he_step, the VecNormalize launches, a pinned DMA and an event wait) and against
VecNormalizeOracle, on BIT PATTERNS -- both routes perform the same IEEE operations in the same
order, so the tolerance is zero.  episode_length = 12 and 30 steps: every env ends twice."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.hedging_oracle import load_golden
from oracle.vecnorm_oracle import VecNormalizeOracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(loss_type="abs", pnl_penalty_weight=0.001, lambda_cost=0.0001, theta_weight=0.0002, slippage_bps=1.0)
GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=12)
MON = ("per_share_step_pnl",)
STEPS = 30
D = 13


def _env(n, mode="gbm", seed=7, **kw):
    from cantorrl_amd.vec_env import HedgingVecEnv
    kw = dict(dict(info_keys=MON, monitor_keywords=MON), **kw)
    return HedgingVecEnv(n, mode=mode, generate=GEN, seed=seed, device=DEV, **kw, **KW)


NO_INFO = dict(info_keys=(), monitor_keywords=None)   # no info column at all: he_step gets info = NULL


def _replay_env(**kw):
    from cantorrl_amd.vec_env import HedgingVecEnv
    cfg, d = load_golden(os.path.join(GOLDEN, "g1_v2_train.npz"))
    kw = dict(dict(info_keys=MON, monitor_keywords=MON), **kw)
    env = HedgingVecEnv(2, tables=(d["paths"], d["volatilities"], d["call_prices_atm"], d["put_prices_atm"]),
                        variant=int(d["variant"]), **kw, **cfg)
    env.seed_envs([int(d["seed_base"]) + i for i in range(2)])
    # the recording holds one episode end per env: two passes over its actions give two
    acts = [np.ascontiguousarray(d["actions"][s][:2]) for s in range(int(d["n_steps"]))] * 2
    return env, acts


def _actions(n, steps=STEPS, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, size=(n, 2)).astype(np.float32) for _ in range(steps)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.nonzero(_bits(got).ravel() != _bits(exp).ravel())[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got.ravel()[bad[:5]], exp.ravel()[bad[:5]])


def _state(vn):
    return {k: getattr(vn, k).cpu().numpy() for k in ("_stats", "_returns", "_ep_ret", "_ep_len")}


def _same_step(k, got, exp, mon=MON):
    """One step's (obs, reward, done, infos) of two wrappers; returns the episodes it finished."""
    for name, g, e in zip(("obs", "reward", "done"), got[:3], exp[:3]):
        _same(g, e, f"{name} step {k}")
    done = np.nonzero(exp[2])[0]
    for i in done:
        gi, ei = got[3][int(i)], exp[3][int(i)]
        _same(gi["terminal_observation"], ei["terminal_observation"], f"terminal obs step {k} row {i}")
        assert ("episode" in gi) == ("episode" in ei) == (mon is not None)
        keys = () if mon is None else ("r", "l") + tuple(mon)   # not "t": wall time
        for key in keys:
            g, e = gi["episode"][key], ei["episode"][key]
            assert type(g) is type(e), (k, i, key, type(g), type(e))
            _same(np.float64(g), np.float64(e), f"episode[{key!r}] step {k} row {i}")
    return len(done)


def _same_state(k, a, b):
    sa, sb = _state(a), _state(b)
    for key in sa:
        _same(sa[key], sb[key], f"{key} after step {k}")


@functools.lru_cache(maxsize=None)
def _trained_stats(mode, n, moments, info=True):
    """(obs_rms, ret_rms) of a 5-step training run, made once per case."""
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    kw = {} if info else NO_INFO
    if mode == "replay":
        env, acts = _replay_env(**kw)
    else:
        env, acts = _env(n, mode, seed=5, **kw), _actions(n, 5, seed=1)
    vn = DeviceVecNormalize(env, gamma=0.95, moments=moments, host_io=False)
    vn.reset()
    for a in acts[:5]:
        vn.step(a)
    out = vn.obs_rms, vn.ret_rms
    vn.close()
    return out


def _pair(mode, n, moments, training, info=True):
    """(host-route wrapper, host_io=False wrapper, actions) over identically built envs."""
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    kw = {} if info else NO_INFO
    pair = []
    for host_io in ("auto", False):
        if mode == "replay":
            env, acts = _replay_env(**kw)
        else:
            env, acts = _env(n, mode, **kw), _actions(n)
        assert (env._info_ref is not None) == info
        vn = DeviceVecNormalize(env, training=training, gamma=0.95, moments=moments, host_io=host_io)
        if not training:
            vn.obs_rms, vn.ret_rms = _trained_stats(mode, n, moments, info)
        pair.append(vn)
    assert pair[0]._hout is not None and pair[1]._hout is None
    return pair[0], pair[1], acts


CASES = [(mode, n) for mode in ("gbm", "heston") for n in (1, 2, 9, 255, 256)] + [("replay", 2)]


def _compare_routes(mode, n, moments, training, info):
    a, b, acts = _pair(mode, n, moments, training, info)
    _same(a.reset(), b.reset(), "reset obs")
    finished = 0
    for k, act in enumerate(acts):
        got, exp = a.step(act), b.step(act)
        finished += _same_step(k, got, exp, MON if info else None)
        _same(a.get_original_obs(), b.get_original_obs(), f"original obs step {k}")
        _same(a.get_original_reward(), b.get_original_reward(), f"original reward step {k}")
        _same_state(k, a, b)
    assert finished >= 2 * n   # the comparison covers episode ends, twice per env
    a.close()
    b.close()


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("moments", ["f64", "sb3"])
@pytest.mark.parametrize("mode,n", CASES)
def test_host_route_equals_the_unchanged_route_bit_for_bit(mode, n, moments, training):
    """Monitor on: every he_step requests info fields (the INFO kernels; f64 training sums in
    moments_body's order, as vn_moments_after_step_kernel makes them on the other route)."""
    _compare_routes(mode, n, moments, training, True)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("moments", ["f64", "sb3"])
@pytest.mark.parametrize("mode,n", CASES)
def test_host_route_without_info_fields_equals_the_unchanged_route_bit_for_bit(mode, n, moments, training):
    """No info column and no Monitor: he_step gets info = NULL, so the other route takes the FAST
    step kernels and, for f64 training, step1_vn_kernel's column-major sums -- which agree with
    moments_body's to rounding only.  The armed step must take the same ones."""
    _compare_routes(mode, n, moments, training, False)


@pytest.mark.parametrize("info", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("moments", ["f64", "sb3"])
def test_greeks_made_in_the_step_kernel(monkeypatch, moments, training, info):
    """The GBM instances that evaluate the obs greeks themselves (by default from 262,144 envs,
    which the host route never has): forced at he_create for both wrappers."""
    monkeypatch.setenv("HE_GREEKS_IN_STEP_MIN_ENVS", "0")
    _compare_routes("gbm", 9, moments, training, info)


@pytest.mark.parametrize("n", [2, 256])
def test_host_route_equals_numpy_bit_for_bit(n):
    """moments="sb3" against VecNormalizeOracle(moments="sb3") fed the raw values of the step."""
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    env = _env(n)
    vn = DeviceVecNormalize(env, gamma=0.95, moments="sb3")
    assert vn._hout is not None
    ref = VecNormalizeOracle(n, gamma=0.95, moments="sb3")
    obs = vn.reset()
    _same(obs, ref.reset(vn.get_original_obs()), "reset obs")
    finished = 0
    for k, act in enumerate(_actions(n)):
        o, r, done, infos = vn.step(act)
        raw_o, raw_r = vn.get_original_obs(), vn.get_original_reward()
        raw_r64 = infos._host["reward_step"]
        assert np.array_equal(raw_r, raw_r64.astype(np.float32), equal_nan=True)
        eo, er, et, eps = ref.step(raw_o, raw_r, done, env._hio.tobs.copy(), env_rewards=raw_r64)
        _same(o, eo, f"obs step {k}")
        _same(r, np.asarray(er).astype(np.float32), f"reward step {k}")
        _same(vn._returns.cpu().numpy(), ref.returns, f"returns step {k}")
        stats = np.concatenate([ref.obs_rms.mean, ref.obs_rms.var, [ref.obs_rms.count], [ref.ret_rms.mean],
                                [ref.ret_rms.var], [ref.ret_rms.count]]).astype(np.float64)
        _same(vn._stats.cpu().numpy(), stats, f"stats step {k}")
        for i, t in et.items():
            _same(infos[i]["terminal_observation"], t, f"terminal obs step {k} row {i}")
            _same(vn._hout.ep_ret_done[i], np.float64(eps[i][0]), f"episode return step {k} row {i}")
            ep = infos[i]["episode"]
            assert ep["r"] == round(float(eps[i][0]), 6) and ep["l"] == eps[i][1] == 12
            finished += 1
    assert finished >= 2 * n
    vn.close()


def test_route_and_refusals():
    from cantorrl_amd import _lib
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    big = _env(257)
    vn = DeviceVecNormalize(big)   # "auto": more than one step workgroup keeps the other route
    assert vn._hout is None
    with pytest.raises(ValueError, match="256"):
        DeviceVecNormalize(big, host_io=True)
    c = vn._call_args()
    assert vn.lib.he_vecnorm_attach_step(big._h, c[2], c[4], None) == _lib.HE_EINVAL
    assert b"256" in vn.lib.he_last_error(big._h)
    vn.reset()
    o, r, d, _ = vn.step(_actions(257, 1)[0])
    assert o.shape == (257, D) and np.isfinite(o).all()
    vn.close()

    env = _env(2)
    vn = DeviceVecNormalize(env)
    w, z, lib, h = vn._hout, env._hio, vn.lib, env._h
    assert w is not None
    vn.reset()
    acts = _actions(2, 6)
    # the flag word advances by exactly one per host-route step
    seq = lib.he_signal_seq(h)
    for k, a in enumerate(acts[:3]):
        vn.step(a)
        assert lib.he_signal_seq(h) == seq + k + 1
    # an armed step without the obs buffer: HE_EINVAL, and the arm is consumed
    views = (w.io, w.tobs.view(np.uint8), w.ep_ret_done.view(np.uint8), w.ep_len_done.view(np.uint8))
    for v in views:
        v[...] = 0xA5
    state = _state(vn)
    c = vn._call_args()
    assert lib.he_vecnorm_attach_step(h, c[2], w.out_ref, None) == _lib.HE_OK
    args = list(z.step_args)
    args[1] = None
    assert lib.he_step(h, *args, vn._stream()) == _lib.HE_EINVAL
    assert b"he_vecnorm_attach_step" in lib.he_last_error(h)
    # ... so the next step, which nobody armed, leaves the wrapper's block and state alone
    env.step(acts[3])
    torch.cuda.synchronize()
    for v in views:
        assert (v == 0xA5).all()
    for key, val in _state(vn).items():
        _same(val, state[key], key)
    o, r, d, _ = vn.step(acts[4])   # the wrapper still steps
    assert np.isfinite(o).all() and np.isfinite(r).all()
    vn.close()

    manual = _env(2, autoreset=False)   # the step keeps a done row's terminal obs where it resets the row
    vn = DeviceVecNormalize(manual)
    assert vn._hout is None
    with pytest.raises(ValueError, match="autoreset"):
        DeviceVecNormalize(manual, host_io=True)
    vn.close()

    tens = _env(2, return_numpy=False)
    with pytest.raises(ValueError, match="device tensors"):
        DeviceVecNormalize(tens, host_io=True)
    tens.close()


def test_returned_arrays_are_private():
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    vn = DeviceVecNormalize(_env(9), gamma=0.95, moments="sb3")
    assert vn._hout is not None
    vn.reset()
    acts = _actions(9, 14)
    for a in acts[:11]:
        vn.step(a)
    o, r, d, infos = vn.step(acts[11])   # step 12 of 12: every env ends its episode
    assert d.all()
    raw_o, raw_r = vn.get_original_obs(), vn.get_original_reward()
    rows = [dict(infos[i]) for i in range(9)]
    kept = [x.copy() for x in (o, r, d, raw_o, raw_r)]
    kept_rows = [dict(terminal_observation=x["terminal_observation"].copy(), episode=dict(x["episode"])) for x in rows]
    for a in acts[12:14]:
        vn.step(a)
    for x, y, name in zip((o, r, d, raw_o, raw_r), kept, ("obs", "reward", "done", "original obs", "original reward")):
        _same(x, y, name)
    for i in range(9):
        _same(rows[i]["terminal_observation"], kept_rows[i]["terminal_observation"], f"terminal obs row {i}")
        _same(infos[i]["terminal_observation"], kept_rows[i]["terminal_observation"], f"view terminal obs row {i}")
        assert rows[i]["episode"] == kept_rows[i]["episode"] == infos[i]["episode"]
    vn.close()


@pytest.mark.parametrize("moments", ["f64", "sb3"])
def test_step_wait_and_step_tensors_interleave(moments):
    a, b, acts = _pair("gbm", 9, moments, True)
    _same(a.reset(), b.reset(), "reset obs")
    for a_ in acts[:11]:   # up to the step before the episodes end
        a.step(a_)
        b.step(a_)
    for k, act in enumerate(acts[11:14]):
        exp = b.step(act)
        if k == 1:
            o, r, t, _ = a.step_tensors(act)
            _same(o.cpu().numpy(), exp[0], "obs of step_tensors")
            _same(r.cpu().numpy(), exp[1], "reward of step_tensors")
            _same(t.cpu().numpy().astype(bool), exp[2], "done of step_tensors")
        else:
            _same_step(k, a.step(act), exp)
        _same(a.get_original_obs(), b.get_original_obs(), f"original obs step {k}")
        _same(a.get_original_reward(), b.get_original_reward(), f"original reward step {k}")
        _same_state(k, a, b)
    a.close()
    b.close()


def test_device_actions_keep_the_device_route():
    """Actions that are already a device tensor are not copied back to the host: that step takes
    the device-buffer route, with the same results."""
    a, b, acts = _pair("gbm", 2, "f64", True)
    _same(a.reset(), b.reset(), "reset obs")
    seq = a.lib.he_signal_seq(a.venv._h)
    for k, act in enumerate(acts[:13]):
        dev = k % 2 == 1
        _same_step(k, a.step(torch.as_tensor(act, device=DEV) if dev else act), b.step(act))
        _same(a.get_original_obs(), b.get_original_obs(), f"original obs step {k}")
        _same_state(k, a, b)
    assert a.lib.he_signal_seq(a.venv._h) == seq + 7   # the 7 host-route steps
    a.close()
    b.close()


@pytest.mark.parametrize("host_io", ["auto", False])
def test_reward_step_column_without_monitor(host_io):
    """info_keys=("reward_step",) exposes the f64 reward column; without monitor_keywords there is
    no Monitor, so a done row has its terminal observation and no episode."""
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    env = _env(2, info_keys=("reward_step",), monitor_keywords=None)
    vn = DeviceVecNormalize(env, host_io=host_io)
    assert not vn._monitor and (vn._hout is not None) == (host_io == "auto")
    vn.reset()
    ended = 0
    for a in _actions(2, 13):
        o, r, d, infos = vn.step(a)
        for i in range(2):
            assert "episode" not in infos[i]
            assert ("terminal_observation" in infos[i]) == bool(d[i])
            # the exposed column is the f64 reward the env rounded into its f32 buffer
            assert np.float32(infos[i]["reward_step"]) == vn.get_original_reward()[i]
            ended += bool(d[i])
    assert ended == 2
    vn.close()
