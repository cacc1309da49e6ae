"""Host replay of librbergomi's Philox draws, written from include/rbergomi.h.

TEST INFRASTRUCTURE ONLY.  Plain NumPy on the oracle's Philox4x32-10 and u01 (both
pinned to known answers and to rocRAND by tests/test_lib_cpu.py); nothing here
imports the product.  Each function returns what one kernel consumes when its
caller passes no normals, in the layout the header documents:

  counter = (block, domain << 24 | (sub & 0xFFFFFF), lo(gid), hi(gid))
  key     = (lo(seed), hi(seed))
  domain 1  parameter perturbations: blocks 0..2 of gid = path_offset + path, sub 0
  domain 2  main-path W_j: block j, sub 0
  domain 3  option MC, sub = day * 2 + type:
            f64  block m M + b:       b < M/2 Re W pairs, b = M/2 + j/2 Im W pairs
            f32  block m M/2 + b:     b < M/4 Re W quads, b = M/4 + j/4 Im W quads
                 (M = 2: block m alone, Re W0, Re W1, Im W0 = its first three normals)

Normals.  f64: sqrt(-2 log u1) (cos, sin)(2 pi u2) with libm on u1 = u01(x.x, x.y),
u2 = u01(x.z, x.w) -- the textbook formula, not a restatement of the kernels'
polynomial Box-Mullers (those are held to it by test_box_muller_within_ulps_of_libm
and test_mc_box_muller_extreme_uniforms).  f32: the four uniforms ((x >> 8) + 1/2) 2^-24
are formed in float32 as the kernel forms them (the + 1/2 rounds to even above 2^23,
so u = 1 and a zero radius occur); radius and angle are then evaluated in f64.

`perturb` arguments are hooks of the checker-sensitivity test
(tests/test_rbergomi_replay_cpu.py): deliberately wrong layouts.
"""
import numpy as np

from oracle.hedging_oracle import philox4x32_10, u01_from_words

DOM_PARAMS, DOM_MAIN, DOM_MC = 1, 2, 3
PERTURBATIONS = ("im_shift", "swap_pair", "drop_hi_gid", "sub_flip", "zero_pad")

_M32 = 0xFFFFFFFF


def _u64(x):
    """uint64 array of Python ints / arrays (values up to 2^64 - 1)."""
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind not in "ui":
        a = np.array([int(v) for v in np.ravel(x)], dtype=np.uint64).reshape(np.shape(x))
    return a.astype(np.uint64)


def words(seed, domain, sub, gid, block, *, drop_hi_gid=False):
    """The four Philox words of every (sub, gid, block), broadcast together."""
    seed = int(seed)
    sub, gid, block = np.broadcast_arrays(_u64(sub), _u64(gid), _u64(block))
    c0 = (block & np.uint64(_M32)).astype(np.uint32)
    c1 = ((np.uint64(domain) << np.uint64(24)) | (sub & np.uint64(0xFFFFFF))).astype(np.uint32)
    c2 = (gid & np.uint64(_M32)).astype(np.uint32)
    c3 = (gid >> np.uint64(32)).astype(np.uint32)
    if drop_hi_gid:
        c3 = np.zeros_like(c3)
    return philox4x32_10(c0, c1, c2, c3, np.uint32(seed & _M32), np.uint32(seed >> 32))


def normal_pairs(x, *, swap=False):
    """[..., 2] f64 normals of Philox words x (four arrays): libm Box-Muller."""
    u1 = u01_from_words(x[0], x[1])
    u2 = u01_from_words(x[2], x[3])
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)
    return z[..., ::-1] if swap else z


def uniforms_f32(x):
    """The kernel's f32 uniform of a word: ((x >> 8) + 1/2) 2^-24 in float32 arithmetic."""
    k = (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32)
    u = (k + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return u


def normal_quads(x, *, swap=False):
    """[..., 4] normals of Philox words x from the f32 uniforms, evaluated in f64:
    (ra cos u2, ra sin u2, rb cos u4, rb sin u4), ra = sqrt(-2 ln u1), rb = sqrt(-2 ln u3),
    angles in revolutions."""
    u1, u2, u3, u4 = (uniforms_f32(w).astype(np.float64) for w in x)
    ra = np.sqrt(-2.0 * np.log(u1) + 0.0)      # + 0.0: u = 1 gives -0.0
    rb = np.sqrt(-2.0 * np.log(u3) + 0.0)
    a2, a4 = 2.0 * np.pi * u2, 2.0 * np.pi * u4
    z = np.stack([ra * np.cos(a2), ra * np.sin(a2), rb * np.cos(a4), rb * np.sin(a4)], axis=-1)
    return z[..., [1, 0, 3, 2]] if swap else z


def host_style_normals(seed, domain, sub, gid, block0, n):
    """n f64 normals of blocks [block0, block0 + ceil(n / 2)): rb_host_normals' contract."""
    nb = (n + 1) // 2
    z = normal_pairs(words(seed, domain, sub, gid, (int(block0) + np.arange(nb)) & _M32))
    return z.reshape(-1)[:n]


def unit_normals(seed, off, n):
    """[5, n] unit normals of rb_sample_params: z0..z4 of blocks 0..2, gid = off + path."""
    gid = _u64([int(off) + i for i in range(n)])
    z = normal_pairs(words(seed, DOM_PARAMS, 0, gid[:, None], np.arange(3)[None, :]))   # [n, 3, 2]
    return z.reshape(n, 6)[:, :5].T.copy()


def main_W(seed, off, n, M):
    """[n, M, 2] (Re, Im) of rb_simulate_paths: block j for every j < M, padded points included."""
    gid = _u64([int(off) + i for i in range(n)])
    return normal_pairs(words(seed, DOM_MAIN, 0, gid[:, None], np.arange(M)[None, :]))


def mc_W(seed, gid, sub, n_mc, M_opt, normals="f64", *, n=None, perturb=None):
    """[B, n_mc, M_opt, 2] (Re, Im) of the MC pricer for options with global ids gid [B]
    and draw streams sub (scalar or [B]).  With n (Euler steps of the option) given, the
    Im W entries the kernel never draws (j >= n) are 0; the oracle never reads them."""
    assert perturb in (None,) + PERTURBATIONS, perturb
    M = int(M_opt)
    gid = np.atleast_1d(_u64(gid))
    sub = np.broadcast_to(_u64(sub), gid.shape)
    if perturb == "sub_flip":
        sub = sub ^ np.uint64(1)               # day * 2 + (1 - type)
    kw = dict(drop_hi_gid=perturb == "drop_hi_gid")
    swap = perturb == "swap_pair"
    im_shift = 1 if perturb == "im_shift" else 0
    g, s = gid[:, None, None], sub[:, None, None]
    m = np.arange(n_mc)[None, :, None]
    W = np.zeros((gid.size, n_mc, M, 2))
    j = np.arange(M)
    if normals == "f64":
        re = normal_pairs(words(seed, DOM_MC, s, g, m * M + np.arange(M // 2)[None, None, :], **kw), swap=swap)
        W[..., 0] = re.reshape(gid.size, n_mc, M)
        im = normal_pairs(words(seed, DOM_MC, s, g, m * M + (M // 2 + j // 2 + im_shift)[None, None, :], **kw),
                          swap=swap)
        W[..., 1] = np.take_along_axis(im, np.broadcast_to((j & 1)[None, None, :, None], im.shape[:3] + (1,)),
                                       axis=-1)[..., 0]
    elif normals == "f32" and M == 2:
        q = normal_quads(words(seed, DOM_MC, s, g, m, **kw), swap=swap)              # [B, n_mc, 1, 4]
        W[..., 0] = q[..., 0, :2]
        qi = q if not im_shift else normal_quads(words(seed, DOM_MC, s, g, m + 1, **kw), swap=swap)
        W[..., 0, 1] = qi[..., 0, 2]
    elif normals == "f32":
        h = M // 2
        re = normal_quads(words(seed, DOM_MC, s, g, m * h + np.arange(M // 4)[None, None, :], **kw), swap=swap)
        W[..., 0] = re.reshape(gid.size, n_mc, M)
        im = normal_quads(words(seed, DOM_MC, s, g, m * h + (M // 4 + j // 4 + im_shift)[None, None, :], **kw),
                          swap=swap)
        W[..., 1] = np.take_along_axis(im, np.broadcast_to((j & 3)[None, None, :, None], im.shape[:3] + (1,)),
                                       axis=-1)[..., 0]
    else:
        raise ValueError(normals)
    if n is not None:
        W[:, :, n:, 1] = 0.0
        if perturb == "zero_pad":
            W[:, :, n + 1:, 0] = 0.0
    return W


def w_to_z(W):
    """Z = fft(W_re + i W_im) / sqrt(M): the inverse of the oracle's z_to_w."""
    W = np.asarray(W, dtype=np.float64)
    M = W.shape[-2]
    return np.fft.fft(W[..., 0] + 1j * W[..., 1], axis=-1) / np.sqrt(float(M))
