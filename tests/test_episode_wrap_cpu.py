"""he_math.h episode_wrap / episode_wrap_le (the LDS kernels' episode-step wrap: a conditional
subtraction in place of the integer modulo) against `%`, exhaustively over the episode lengths
and block offsets the kernels can meet, through the host build (he_host_episode_wrap)."""
import numpy as np

from cantorrl_amd import _lib


def test_episode_wrap_equals_modulo_exhaustively():
    lib = _lib.load()
    ts, ks, Ts = [], [], []
    for T in range(1, 1025):
        t = np.arange(T, dtype=np.uint32)
        for k in range(0, 9):
            ts.append(t)
            ks.append(np.full(T, k, np.uint32))
            Ts.append(np.full(T, T, np.uint32))
    t, k, T = (np.ascontiguousarray(np.concatenate(a)) for a in (ts, ks, Ts))
    assert t.size == 9 * 1024 * 1025 // 2
    ref = (t.astype(np.uint64) + k) % T
    for le in (0, 1):
        out = np.full(t.size, 0xFFFFFFFF, np.uint32)
        assert lib.he_host_episode_wrap(t.ctypes.data, k.ctypes.data, T.ctypes.data, t.size, le,
                                        out.ctypes.data) == 0
        # episode_wrap_le holds only for k <= T; episode_wrap everywhere
        ok = (k <= T) if le else np.ones(t.size, bool)
        assert ok.sum() > 4_700_000
        assert np.array_equal(out[ok], ref[ok].astype(np.uint32)), le


def test_episode_wrap_large_offsets_and_lengths():
    """k > T (the general form) and episode lengths near 2^31 (no 32-bit overflow of t + k)."""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    T = np.concatenate([rng.integers(1, 40, 20000), rng.integers(2 ** 31 - 1000, 2 ** 31, 20000)]).astype(np.uint32)
    t = (rng.integers(0, 2 ** 62, T.size).astype(np.uint64) % T).astype(np.uint32)
    k = rng.integers(0, 300, T.size).astype(np.uint32)
    out = np.empty(T.size, np.uint32)
    assert lib.he_host_episode_wrap(t.ctypes.data, k.ctypes.data, T.ctypes.data, T.size, 0, out.ctypes.data) == 0
    assert np.array_equal(out, ((t.astype(np.uint64) + k) % T).astype(np.uint32))


def test_episode_wrap_rejects_null():
    lib = _lib.load()
    assert lib.he_host_episode_wrap(None, None, None, 4, 0, None) != 0
    assert lib.he_host_episode_wrap(None, None, None, 0, 0, None) == 0
