"""Contract L1-L6 of include/hedge_actor.h (ha_ppo_loss) written again in NumPy f64, from the header's text
and not from ha_math.h: the block sums with the lanes' order and the tree written out, np.exp for the
ratio, the value clip, the eight statistics and the three gradients.  `mistake` names one deliberate
error, for the tests that show each of them is caught.  Also the clipped-value loss in torch f64 under
autograd (tests/_ppo_reference.loss has no value clip), the raw ctypes call of the host build, and the
one-ulp comparison the tests share."""
import ctypes

import numpy as np

BLOCK, LANES, MAX_BLOCKS = 1024, 256, 4096          # HA_LOSS_BLOCK, the lanes of L1, HA_LOSS_MAX_BLOCKS
STATS = ("loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
GRADS = ("values", "log_prob", "entropy")
INPUTS = ("values", "log_prob", "entropy", "old_log_prob", "advantages", "returns")
MISTAKES = ("biased_std", "max_for_min", "clamp_edge", "entropy_sign", "no_vf_coef", "vf_mask_inverted", "no_1_over_n")
F32, F64 = np.float32, np.float64


def block_sum(terms):
    """L1: blocks of BLOCK rows, the last padded with +0; lane i adds rows i, i + 256, ... from 0.0, the tree
    q_i += q_(i + 128) ... q_0 += q_1, then the blocks' sums from 0.0 in order."""
    t = np.asarray(terms, F64).reshape(-1)
    nb = -(-t.size // BLOCK)
    q = np.zeros(nb * BLOCK, F64)
    q[:t.size] = t
    q = q.reshape(nb, BLOCK // LANES, LANES)
    lane = np.zeros((nb, LANES), F64)
    for m in range(BLOCK // LANES):
        lane = lane + q[:, m]
    off = LANES // 2
    while off >= 1:
        lane = lane[:, :off] + lane[:, off:2 * off]
        off //= 2
    total = F64(0.0)
    for s in lane[:, 0]:
        total = total + s
    return total


def contract(x, clip_range, ent_coef, vf_coef, normalize_advantage=True, clip_range_vf=None, mistake=None):
    """x: dict of flat f32 arrays (INPUTS, and old_values with a value clip) -> (stats, grads, aux): the
    eight statistics and the three gradients in f64 BEFORE the one rounding to f32, and aux with the
    rows' r, A', pass."""
    assert mistake is None or mistake in MISTAKES
    for k in INPUTS:
        assert x[k].dtype == F32
    v, lp, ent, old, A, ret = (x[k].astype(F64).reshape(-1) for k in INPUTS)
    N, c = v.size, F64(clip_range)
    n = F64(N)
    mean, std = F64(0.0), F64(1.0)
    if normalize_advantage:                                    # L2, L3
        mean = block_sum(A) / n
        dev = A - mean
        std = np.sqrt(block_sum(dev * dev) / (n if mistake == "biased_std" else n - 1.0))
        A = dev / (std + 1e-8)
    d = lp - old                                               # L4
    r = np.exp(d)
    lo, hi = 1.0 - c, 1.0 + (2.0 * c if mistake == "clamp_edge" else c)
    rc = np.where(r < lo, lo, np.where(r > hi, hi, r))
    s1, s2 = A * r, A * rc
    pol = np.where(s2 > s1, s2, s1) if mistake == "max_for_min" else np.where(s2 < s1, s2, s1)
    active = np.where(A >= 0.0, r < hi, r > lo)
    if clip_range_vf is None:
        vp, passes = v, np.ones(N, bool)
    else:
        cv, ov = F64(clip_range_vf), x["old_values"].astype(F64).reshape(-1)
        dv = v - ov
        vp = ov + np.where(dv < -cv, -cv, np.where(dv > cv, cv, dv))
        passes = np.abs(dv) <= cv
        if mistake == "vf_mask_inverted":
            passes = ~passes
    e = ret - vp
    kl = (r - 1.0) - d
    clipped = (np.abs(r - 1.0) > c).astype(F64)
    policy = -block_sum(pol) / n                               # L5
    value = block_sum(e * e) / n
    entropy_loss = block_sum(ent) / n if mistake == "entropy_sign" else -block_sum(ent) / n
    vf = F64(1.0 if mistake == "no_vf_coef" else vf_coef)
    stats = dict(loss=(policy + F64(ent_coef) * entropy_loss) + vf * value, policy_gradient_loss=policy,
                 value_loss=value, entropy_loss=entropy_loss, approx_kl=block_sum(kl) / n,
                 clip_fraction=block_sum(clipped) / n, adv_mean=mean, adv_std=std)
    div = F64(1.0) if mistake == "no_1_over_n" else n          # L6
    grads = dict(log_prob=np.where(active, -s1 / div, 0.0), values=np.where(passes, -((2.0 * vf) * e) / n, 0.0),
                 entropy=np.full(N, -F64(ent_coef) / n))
    return stats, grads, dict(ratio=r, adv=A, passes=passes, dv=None if clip_range_vf is None else dv)


def rounded(stats, grads):
    """The contract's outputs as the library stores them: each rounded once to f32."""
    return np.array([stats[k] for k in STATS], F64).astype(F32), {k: grads[k].astype(F32) for k in GRADS}


def within_one_ulp(got, want64, extra=0.0):
    """got (f32) is want64's rounding to f32 or a neighbour of it; `extra`: an absolute allowance on top."""
    got, w32 = np.asarray(got, F32), np.asarray(want64, F64).astype(F32)
    return bool(np.all(np.abs(got.astype(F64) - w32.astype(F64)) <= np.spacing(np.abs(w32)).astype(F64) + extra))


def agrees(stats32, grads32, want_stats, want_grads):
    """The general-input bound: every statistic and gradient element within one f32 ulp of the f64
    restatement, approx_kl with 2^-48 absolute on top for the cancellation in (r - 1) - d."""
    ok = all(within_one_ulp(stats32[j], want_stats[k], 2.0 ** -48 if k == "approx_kl" else 0.0)
             for j, k in enumerate(STATS))
    return ok and all(within_one_ulp(grads32[k], want_grads[k]) for k in GRADS)


def torch_loss_clipped(ref, t, clip_range, ent_coef, vf_coef, normalize_advantage, clip_range_vf):
    """tests/_ppo_reference.loss with SB3 2.6.0's value clip in front: values_pred = old_values +
    clamp(values - old_values, -clip_range_vf, clip_range_vf), torch tensors of any dtype under autograd."""
    import torch
    values = t["values"]
    if clip_range_vf is not None:
        values = t["old_values"] + torch.clamp(values - t["old_values"], -clip_range_vf, clip_range_vf)
    return ref.loss(values, t["log_prob"], t["entropy"], t["old_log_prob"], t["advantages"], t["returns"],
                    clip_range, ent_coef, vf_coef, normalize_advantage)


# --------------------------------------------------------------------------- the library, raw
class Hyper(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("clip_range", "clip_range_vf", "ent_coef", "vf_coef")] + \
               [("normalize_advantage", ctypes.c_int32)]


class Io(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in INPUTS + ("old_values", "d_values", "d_log_prob", "d_entropy", "stats")]


def host_loss(x, clip_range, ent_coef, vf_coef, normalize_advantage=True, clip_range_vf=None, n_rows=None, fill=np.nan):
    """ha_host_ppo_loss over the f32 arrays of x -> (status, stats [8] f32, {values, log_prob, entropy: f32
    gradients}); the outputs start as `fill`, so a refusal shows them untouched.  A key of x set to None
    is passed as NULL."""
    from cantorrl_amd import agent
    lib = agent.load()
    N = x["values"].size
    io, keep = Io(), []
    for k in INPUTS + ("old_values",):
        a = x.get(k)
        if a is not None:
            a = np.ascontiguousarray(a, F32)
            keep.append(a)
            setattr(io, k, a.ctypes.data)
    stats = np.full(8, fill, F32)
    grads = {k: np.full(N, fill, F32) for k in GRADS}
    io.d_values, io.d_log_prob, io.d_entropy = (grads[k].ctypes.data for k in GRADS)
    io.stats = stats.ctypes.data
    hy = Hyper(clip_range, 0.0 if clip_range_vf is None else clip_range_vf, ent_coef, vf_coef, int(normalize_advantage))
    st = lib.ha_host_ppo_loss(N if n_rows is None else n_rows, ctypes.byref(io), ctypes.byref(hy))
    return st, stats, grads


# --------------------------------------------------------------------------- inputs
def quantised_inputs(N, seed):
    """r = 1 exactly (log_prob == old_log_prob) and every value a multiple of 2^-6: exp cannot differ."""
    rng = np.random.default_rng(seed)
    q = lambda a: (np.round(a * 64.0) / 64.0).astype(F32)
    old = q(rng.normal(3.0, 1.0, N))
    v = q(rng.normal(0, 1, N))
    return dict(values=v, log_prob=old.copy(), entropy=q(rng.normal(-5.8, 0.1, N)), old_log_prob=old,
                advantages=q(rng.normal(0.05, 1.0, N)), returns=q(rng.normal(0, 1, N)),
                old_values=q(v + rng.normal(0, 0.25, N)))


def general_inputs(N, ratios, adv, seed, dv=None):
    """tests/test_ppo_loss_cpu.loss_inputs in f32, with old_values = values - dv (default: N(0, 0.2))."""
    rng = np.random.default_rng(seed)
    old = rng.normal(3.0, 1.0, N).astype(F32)
    v = rng.normal(0, 1, N).astype(F32)
    x = dict(values=v, log_prob=(old.astype(F64) + np.log(ratios)).astype(F32), entropy=rng.normal(-5.8, 0.1, N).astype(F32),
             old_log_prob=old, advantages=np.asarray(adv, F64).astype(F32), returns=rng.normal(0, 1, N).astype(F32))
    x["old_values"] = (v.astype(F64) - (rng.normal(0, 0.2, N) if dv is None else np.asarray(dv, F64))).astype(F32)
    return x


def six_region_inputs(seed=5):
    """N = 64 as test_ppo_loss_cpu.test_ppo_loss_with_all_six_regions_in_one_minibatch builds it."""
    N = 64
    rng = np.random.default_rng(11)
    kind = np.arange(N) % 3
    ratios = np.where(kind == 0, rng.uniform(0.4, 0.65, N), np.where(kind == 1, rng.uniform(0.75, 1.25, N),
                                                                     rng.uniform(1.4, 1.8, N)))
    sign = np.where((np.arange(N) // 3) % 2 == 0, 1.0, -1.0)
    return general_inputs(N, ratios, sign * rng.uniform(0.2, 2.0, N) + 0.05, seed)


def random_inputs(N, seed):
    rng = np.random.default_rng(seed)
    return general_inputs(N, np.exp(rng.normal(0, 0.3, N)), rng.normal(0.05, 1.0, N), seed + 1)


# four pairs with A = (+, -): exactly one row of each is outside the clip range of 0.3 and exactly one
# moves its value by more than the value clip of 0.2
PAIRS = ((1.5, 0.9), (0.5, 1.2), (1.1, 0.45), (0.9, 1.6))


def pair_inputs(j):
    return general_inputs(2, np.array(PAIRS[j]), (0.8, -0.3), j, dv=(0.5, 0.05) if j % 2 == 0 else (-0.03, -0.4))


def general_cases():
    """name -> inputs: the cases of the CPU file's test 2, shared with the GPU file."""
    cases = {f"pair{j}": pair_inputs(j) for j in range(len(PAIRS))}
    cases["six_regions"] = six_region_inputs()
    cases["two_blocks"] = random_inputs(2 * BLOCK + 3, 21)
    return cases
