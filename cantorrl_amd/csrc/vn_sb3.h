// vn_sb3.h -- the arithmetic of moments = "sb3" (HE_VN_MOMENTS_SB3): SB3 2.6.0 VecNormalize
// over NumPy, operation for operation, so that the device reproduces the bits of the
// reference's own stack (train_ppo_v2.py:204,305,450-453; oracle/vecnorm_oracle.py with
// moments="sb3").  __host__ __device__: vn_sb3_kernel (vecnorm.hip), the eval arm fused into
// he_step (vn_apply.h apply_frozen_rows) and the host mirror he_host_vecnorm_sb3 run the same
// functions.  The build keeps -ffp-contract=off and correctly rounded f32 divide / sqrt.
//
//   obs batch moments   np.mean / np.var over axis 0 of the [n][13] f32 batch: per column one
//                       f32 chain in row order (col_sum, col_sq), divided by (float)n;
//   returns moments     np.mean / np.var of the [n] f64 returns: NumPy's pairwise sum over all n
//                       elements (pw_node, pw_leaf);
//   update              RunningMeanStd.update_from_moments (rms_update); the obs batch variance
//                       times the count is an f32 product (batch_m2_obs);
//   normalization       f64 subtract, sqrt and divide, clipped, then rounded to f32 (norm_obs,
//                       norm_rew) -- no reciprocal.
// rms_update and clipd are also the default mode's (vecnorm.hip vn_apply_kernel, vn_apply.h
// SplitNorm): one copy of each.  vn_apply.h wraps norm_obs / norm_rew as the normaliser Sb3Norm.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hedge_env.h"

namespace sb3 {

#define VN_SB3_HD __host__ __device__ __forceinline__

constexpr int kD = HE_OBS_DIM;
constexpr int kMaxN = 4096;      // envs this mode covers
constexpr int kLeafMax = 128;    // NumPy's PW_BLOCKSIZE: a block summed with eight accumulators
// a level of splits leaves at most n / 2 + 4 elements: n <= 4096 is <= 128 after 6 levels
constexpr int kMaxLevels = 6;
constexpr int kNodes = 2 << kMaxLevels;   // heap slots (node 0 unused)

// ------------------------------------------------------------------ obs: f32 chains in row order
// Rows [0, rows) of one column (p[i * kD]) added to s in row order; first: s starts as row 0
// (np.add.reduce over axis 0 copies the first row, then adds the others).
// SQ: the same chain over q_i = (a_i - m)^2 (np.var: x = arr - mean; x = x * x; sum over axis 0).
// The adds are one dependent chain; the loads are not, so the rows come in batches of kBatch
// with the next batch's loads issued before the current one is added (on the device the rows are
// in LDS: a batch's adds cover the next one's read latency).  The order of the adds is the rows'.
constexpr int kBatch = 16;
template <bool SQ>
VN_SB3_HD float col_term(float x, float m) {
    if (!SQ) return x;
    const float d = x - m;
    return d * d;
}
template <bool SQ>
VN_SB3_HD float col_chain(float acc, bool first, float m, const float* p, int rows) {
    int i = 0;
    if (first && rows > 0) {
        acc = col_term<SQ>(p[0], m);
        i = 1;
    }
    const int nb = (rows - i) / kBatch;
    if (nb > 0) {
        float x[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) x[j] = p[(i + j) * kD];
        for (int b = 0; b < nb; ++b) {
            float y[kBatch];
            const bool more = b + 1 < nb;
            if (more) {
#pragma unroll
                for (int j = 0; j < kBatch; ++j) y[j] = p[(i + kBatch + j) * kD];
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) acc += col_term<SQ>(x[j], m);
            if (more) {
#pragma unroll
                for (int j = 0; j < kBatch; ++j) x[j] = y[j];
            }
            i += kBatch;
        }
    }
    for (; i < rows; ++i) acc += col_term<SQ>(p[i * kD], m);
    return acc;
}
VN_SB3_HD float col_sum(float s, bool first, const float* p, int rows) {
    return col_chain<false>(s, first, 0.0f, p, rows);
}
VN_SB3_HD float col_sq(float v, bool first, float m, const float* p, int rows) {
    return col_chain<true>(v, first, m, p, rows);
}

// ------------------------------------------------------------------ returns: NumPy's pairwise sum
// A block of n > 128 elements splits at n2 = n / 2 - (n / 2) % 8 into sum(first n2) + sum(rest);
// a block of <= 128 is a leaf (pw_leaf).  The tree's nodes in heap order -- 1 the root, 2 id and
// 2 id + 1 the halves of node id -- depend on n alone, so every thread finds its own node
// without a stack: the leaves are summed side by side, then the splits level by level upwards.
struct Node {
    int32_t lo, n;   // elements [lo, lo + n); n = 0: the tree has no such node
};
VN_SB3_HD int pw_half(int n) {
    const int h = n / 2;
    return h - h % 8;
}
// levels of splits below the root: the second halves are the larger ones
VN_SB3_HD int pw_levels(int n) {
    int d = 0;
    for (; n > kLeafMax; ++d) n -= pw_half(n);
    return d;
}
VN_SB3_HD Node pw_node(int n, int id) {
    int depth = 0;
    for (int k = id; k > 1; k >>= 1) ++depth;
    int lo = 0, m = n;
    for (int b = depth - 1; b >= 0; --b) {
        if (m <= kLeafMax) return Node{0, 0};   // an ancestor is a leaf
        const int n2 = pw_half(m);
        if ((id >> b) & 1) {
            lo += n2;
            m -= n2;
        } else {
            m = n2;
        }
    }
    return Node{lo, m};
}
// One leaf: n < 8 a plain left-to-right sum; else eight accumulators over the full groups
// of 8, combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 tail in order.
VN_SB3_HD double pw_leaf(const double* a, int n) {
    if (n < 8) {
        double res = n > 0 ? a[0] : 0.0;
        for (int i = 1; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
// ------------------------------------------------------------------ the statistics
// VecNormalize._update_reward's returns = returns * gamma + reward: an f64 multiply, then an add
VN_SB3_HD double ret_update(double ret, double gamma, float reward) { return ret * gamma + (double)reward; }

// m_b = batch_var * batch_count of the obs statistics: an f32 array times a Python int is an
// f32 product, widened afterwards (an f64 product differs at every n that is no power of two)
VN_SB3_HD double batch_m2_obs(float bvar, int n) { return (double)(bvar * (float)n); }

// RunningMeanStd.update_from_moments (SB3 common/running_mean_std.py) in f64, the batch mean
// already widened, m_b = batch_var * batch_count as its dtype made it
VN_SB3_HD void rms_update(double* mean, double* var, double* count, double bmean, double m_b, double bcount) {
    const double delta = bmean - *mean;
    const double tot = *count + bcount;
    const double new_mean = *mean + delta * bcount / tot;
    const double m_a = *var * *count;
    const double m2 = m_a + m_b + delta * delta * *count * bcount / tot;
    *mean = new_mean;
    *var = m2 / tot;
    *count = tot;
}

// ------------------------------------------------------------------ normalization
// np.clip (NaN stays NaN)
VN_SB3_HD double clipd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
// sqrt(var + eps) of a column, made once
VN_SB3_HD double norm_sd(double var, double eps) { return sqrt(var + eps); }
// np.clip((obs - mean) / sqrt(var + eps), -clip, clip).astype(np.float32)
VN_SB3_HD float norm_obs(float x, double mean, double sd, double clip) {
    return (float)clipd(((double)x - mean) / sd, -clip, clip);
}
// np.clip(reward / sqrt(ret_var + eps), -clip, clip), rounded to f32
VN_SB3_HD float norm_rew(float r, double sd, double clip) { return (float)clipd((double)r / sd, -clip, clip); }

}  // namespace sb3
