"""The row-tail routes of he_vecnorm_step that no env-driven test reaches exactly, on random device
tensors through ctypes (no env), statistics frozen (training = 0), Monitor buffers given, about one
row in eight done:

  moments = f64, n = 65,793 = 256 * 257 + 1   more than 256 rows per workgroup on 256 workgroups
      (258: ceil(n / 256)), so vn_apply_kernel takes its chunked branch (a second chunk of two
      rows; the last workgroup's three rows are resident) -- against the same rows in two calls of
      n <= 65,536, which take the resident branch.  Both branches apply the same per-element
      arithmetic to the same statistics: the bits are equal.
  moments = sb3, n = 257   vn_sb3_kernel's strided pass and second row trip -- against the host
      mirror he_host_vecnorm_sb3 (the same functions run by one thread), on what the mirror produces."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 13


def _params(moments):
    from cantorrl_amd import _lib
    p = _lib.HeVecnormParams()
    p.obs_dim, p.training, p.norm_obs, p.norm_reward = D, 0, 1, 1
    p.gamma, p.clip_obs, p.clip_reward, p.epsilon = 0.95, 10.0, 10.0, 1e-8
    p.moments = _lib.VN_MOMENTS[moments]
    return p


def _inputs(n, seed):
    """Host arrays: obs and terminal obs with per-column scales 1e-2 .. 1e3 and offsets +-100 (a few
    elements past the clip), rewards, dones, Monitor's state, and statistics that fit them."""
    rng = np.random.default_rng(seed)
    scale, offset = np.logspace(-2, 3, D), rng.uniform(-100, 100, D)
    mk = lambda: (rng.normal(size=(n, D)) * 4.0 * scale + offset).astype(np.float32)  # noqa: E731
    x = dict(obs=mk(), reward=rng.normal(scale=3.0, size=n).astype(np.float32),
             done=(rng.random(n) < 0.125).astype(np.uint8), tobs=mk(), returns=rng.normal(size=n),
             ep_reward=rng.normal(size=n), ep_ret=rng.normal(scale=5.0, size=n),
             ep_len=rng.integers(0, 250, n).astype(np.int32))
    x["stats"] = np.concatenate([offset, scale * scale, [1000.0], [0.3], [2.5], [1000.0]])
    return x


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _device_step(lib, p, x, spans):
    """he_vecnorm_step over the row spans [lo, hi) of the inputs, one call each, on fresh copies of
    the in/out state; every output and the state after the calls."""
    n = x["obs"].shape[0]
    t = {k: torch.as_tensor(v, device=DEV) for k, v in x.items()}
    out = dict(obs_out=torch.zeros((n, D), dtype=torch.float32, device=DEV),
               reward_out=torch.zeros(n, dtype=torch.float32, device=DEV),
               tobs_out=torch.zeros((n, D), dtype=torch.float32, device=DEV),
               ep_ret_done=torch.zeros(n, dtype=torch.float64, device=DEV),
               ep_len_done=torch.zeros(n, dtype=torch.int32, device=DEV))
    scratch = torch.zeros(lib.he_vecnorm_scratch_bytes(n, D) // 8, dtype=torch.float64, device=DEV)
    for lo, hi in spans:
        s = lambda a: _ptr(a[lo:hi])  # noqa: E731
        st = lib.he_vecnorm_step(ctypes.byref(p), hi - lo, s(t["obs"]), s(t["reward"]), s(t["done"]), s(t["tobs"]),
                                 s(t["returns"]), _ptr(t["stats"]), _ptr(scratch), s(out["obs_out"]),
                                 s(out["reward_out"]), s(out["tobs_out"]), s(t["ep_ret"]), s(t["ep_len"]),
                                 s(out["ep_ret_done"]), s(out["ep_len_done"]), s(t["ep_reward"]), None)
        assert st == 0, st
    torch.cuda.synchronize()
    out.update(returns=t["returns"], ep_ret=t["ep_ret"], ep_len=t["ep_len"], stats=t["stats"])
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.nonzero(np.ascontiguousarray(got).view(bits).ravel() != np.ascontiguousarray(exp).view(bits).ravel())[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got.ravel()[bad[:5]], exp.ravel()[bad[:5]])


@pytest.fixture(scope="module")
def lib():
    from cantorrl_amd import _lib
    return _lib.load()


def test_chunked_apply_equals_resident_apply_bit_for_bit(lib):
    n = 256 * 257 + 1
    x = _inputs(n, 11)
    p = _params("f64")
    whole = _device_step(lib, p, x, [(0, n)])
    parts = _device_step(lib, p, x, [(0, 65536), (65536, n)])
    dn = x["done"] != 0
    assert 0.1 < dn.mean() < 0.15
    # the step did its work: normalized and clipped obs, done rows' returns zeroed, the others kept
    assert np.abs(whole["obs_out"]).max() == 10.0 and not np.array_equal(whole["obs_out"], x["obs"])
    assert np.all(whole["returns"][dn] == 0.0) and np.array_equal(whole["returns"][~dn], x["returns"][~dn])
    assert np.array_equal(whole["ep_len"], np.where(dn, 0, x["ep_len"] + 1))
    assert np.array_equal(whole["ep_len_done"][dn], x["ep_len"][dn] + 1)
    assert np.array_equal(whole["stats"], x["stats"])
    for k in ("obs_out", "reward_out", "returns", "ep_ret", "ep_len", "ep_ret_done", "ep_len_done"):
        _same(whole[k], parts[k], k)
    _same(whole["tobs_out"][dn], parts["tobs_out"][dn], "terminal_obs_out on done rows")
    assert np.abs(whole["tobs_out"][dn]).max() == 10.0


def test_sb3_device_equals_host_mirror_bit_for_bit(lib):
    n = 257
    x = _inputs(n, 12)
    x["done"][[0, 255, 256]] = 1   # a done row in the first row trip's ends and in the second trip
    p = _params("sb3")
    dev = _device_step(lib, p, x, [(0, n)])
    h = {k: v.copy() for k, v in x.items()}
    host = dict(obs_out=np.zeros((n, D), np.float32), reward_out=np.zeros(n, np.float32),
                tobs_out=np.zeros((n, D), np.float32))
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    st = lib.he_host_vecnorm_sb3(ctypes.byref(p), n, hp(h["obs"]), hp(h["reward"]), hp(h["done"]), hp(h["tobs"]),
                                 hp(h["returns"]), hp(h["stats"]), hp(host["obs_out"]), hp(host["reward_out"]),
                                 hp(host["tobs_out"]))
    assert st == 0, st
    dn = x["done"] != 0
    assert np.abs(dev["obs_out"]).max() == 10.0 and np.all(dev["returns"][dn] == 0.0)
    for k in ("obs_out", "reward_out"):
        _same(dev[k], host[k], k)
    _same(dev["tobs_out"][dn], host["tobs_out"][dn], "terminal_obs_out on done rows")
    _same(dev["returns"], h["returns"], "returns")
    _same(dev["stats"], h["stats"], "stats")
    # Monitor, which the mirror does not have: the sums of the env's f64 rewards
    assert np.array_equal(dev["ep_ret_done"][dn], (x["ep_ret"] + x["ep_reward"])[dn])
    assert np.array_equal(dev["ep_ret"], np.where(dn, 0.0, x["ep_ret"] + x["ep_reward"]))
    assert np.array_equal(dev["ep_len"], np.where(dn, 0, x["ep_len"] + 1))
