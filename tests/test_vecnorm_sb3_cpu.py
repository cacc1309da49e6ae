"""moments="sb3" on the host: he_host_vecnorm_sb3 (a single-threaded run of the functions of
cantorrl_amd/csrc/vn_sb3.h that vn_sb3_kernel runs) against VecNormalizeOracle(moments="sb3"),
i.e. against NumPy's own np.mean / np.var, on BIT PATTERNS: both sides perform the same IEEE
operations in the same order, so the tolerance is zero.

n covers the pairwise sum's boundaries (8 accumulators from n = 8, a split above 128, leaves
with a tail) and counts that are no power of two (where the f32 batch_var * n matters)."""
import ctypes

import numpy as np
import pytest

from oracle.vecnorm_oracle import VecNormalizeOracle

D = 13
NS = [1, 2, 7, 8, 9, 129, 137, 257, 1000, 4096]
STEPS = 6


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.nonzero(_bits(got).ravel() != _bits(exp).ravel())[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got.ravel()[bad[:5]], exp.ravel()[bad[:5]])


def _stats(o):
    return np.concatenate([o.obs_rms.mean, o.obs_rms.var, [o.obs_rms.count], [o.ret_rms.mean], [o.ret_rms.var],
                           [o.ret_rms.count]]).astype(np.float64)


@pytest.fixture(scope="module")
def lib():
    from cantorrl_amd import _lib
    return _lib.load()


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class HostSb3:
    """The host mirror with VecNormalizeOracle's reset / step surface."""

    def __init__(self, lib, n, training, norm_reward, gamma):
        from cantorrl_amd import _lib
        self.lib, self.n = lib, n
        p = _lib.HeVecnormParams()
        p.obs_dim, p.training, p.norm_obs, p.norm_reward = D, int(training), 1, int(norm_reward)
        p.gamma, p.clip_obs, p.clip_reward, p.epsilon = gamma, 10.0, 10.0, 1e-8
        p.moments = _lib.HE_VN_MOMENTS_SB3
        self.p = p
        self.stats = np.concatenate([np.zeros(D), np.ones(D), [1e-4, 0.0, 1.0, 1e-4]])
        self.returns = np.zeros(n)
        self.obs_out = np.empty((n, D), np.float32)
        self.rew_out = np.empty(n, np.float32)
        self.tobs_out = np.zeros((n, D), np.float32)

    def _call(self, obs, rew, done, tobs):
        st = self.lib.he_host_vecnorm_sb3(ctypes.byref(self.p), self.n, _ptr(obs), _ptr(rew), _ptr(done), _ptr(tobs),
                                          _ptr(self.returns), _ptr(self.stats), _ptr(self.obs_out),
                                          _ptr(self.rew_out), _ptr(self.tobs_out))
        assert st == 0, st

    def reset(self, obs):
        self._call(obs, None, None, None)
        return self.obs_out.copy()

    def step(self, obs, rew, done, tobs):
        d8 = np.ascontiguousarray(done, np.uint8)
        self._call(obs, rew, d8, tobs)
        return self.obs_out.copy(), self.rew_out.copy(), self.tobs_out.copy()


def _batches(n, seed):
    """Random f32 obs with per-column scales 1e-2 .. 1e3 and offsets +-100, rewards, dones."""
    rng = np.random.default_rng(seed)
    scale = np.logspace(-2, 3, D)
    offset = rng.uniform(-100, 100, D)
    mk = lambda: (rng.normal(size=(n, D)) * scale + offset).astype(np.float32)  # noqa: E731
    first = mk()
    steps = [(mk(), rng.normal(scale=3.0, size=n).astype(np.float32), rng.random(n) < 0.3, mk())
             for _ in range(STEPS)]
    return first, steps


@pytest.mark.parametrize("norm_reward", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("n", NS)
def test_host_mirror_equals_numpy_bit_for_bit(lib, n, training, norm_reward):
    first, steps = _batches(n, 100 + n)
    ref = VecNormalizeOracle(n, training=training, norm_reward=norm_reward, gamma=0.95, moments="sb3")
    got = HostSb3(lib, n, training, norm_reward, 0.95)
    if not training:   # evaluate with statistics worth normalizing by
        warm = VecNormalizeOracle(n, gamma=0.95, moments="sb3")
        warm.reset(first)
        for o, r, dn, t in steps[:2]:
            warm.step(o, r, dn, t)
        ref.obs_rms, ref.ret_rms = warm.obs_rms, warm.ret_rms
        got.stats[:] = _stats(warm)
    _same(got.reset(first), ref.reset(first), "reset obs")
    _same(got.returns, ref.returns, "reset returns")
    _same(got.stats, _stats(ref), "reset stats")
    for k, (o, r, dn, t) in enumerate(steps):
        eo, er, et, _ = ref.step(o, r, dn, t)
        go, gr, gt = got.step(o, r, dn, t)
        _same(go, eo, f"obs step {k}")
        _same(gr, np.asarray(er).astype(np.float32), f"reward step {k}")
        for i, row in et.items():
            _same(gt[i], row, f"terminal obs step {k} row {i}")
        _same(got.returns, ref.returns, f"returns step {k}")
        _same(got.stats, _stats(ref), f"stats step {k}")


def test_host_mirror_refuses_more_than_4096_rows(lib):
    got = HostSb3(lib, 4097, True, True, 0.95)
    obs = np.zeros((4097, D), np.float32)
    st = lib.he_host_vecnorm_sb3(ctypes.byref(got.p), 4097, _ptr(obs), None, None, None, _ptr(got.returns),
                                 _ptr(got.stats), _ptr(got.obs_out), None, None)
    assert st == 1   # HE_EINVAL
