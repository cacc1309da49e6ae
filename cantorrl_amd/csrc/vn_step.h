// vn_step.h -- a whole VecNormalize step made by ONE workgroup of kVnThreads threads: what
// vn_sb3_kernel (vecnorm.hip; rows from global memory, any n <= sb3::kMaxN) and the step fused
// into he_step (hedge_env.hip step1_vnw_kernel, he_vecnorm_attach_step; rows <= kVnChunk, from
// the step's LDS tile and registers) both run.
//   sb3_returns_moments, sb3_update_stats   the workgroup-wide parts of moments = sb3 (the
//                                           per-element arithmetic is vn_sb3.h's);
//   step_rows                               the step over <= kVnChunk rows already in LDS, in
//                                           any mode: moments = sb3 or f64, training or frozen.
// Results are those of the separate launches bit for bit: sb3 is vn_sb3_kernel's code;
// f64 training is the partial of the one workgroup, in the order he_vecnorm_attach's route
// gives the same step (SumOrder; vn_moments.h moments_rows_to / moments_rows_block_order),
// merged as vn_apply_kernel merges one partial; frozen statistics are apply_frozen_rows
// (vn_apply.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vn_apply.h"
#include "vn_moments.h"
#include "vn_sb3.h"

namespace vn {

// Lanes 0 .. 12 carry an obs column's statistics, lane 13 the returns'; loaded before anything
// that waits.
struct StatLane {
    double mean, var, count;
};
__device__ __forceinline__ StatLane load_stat_lane(const double* stats) {
    const int t = threadIdx.x;
    StatLane s{0.0, 1.0, 0.0};
    if (t < kD) {
        s.mean = stats[t];
        s.var = stats[kD + t];
        s.count = stats[2 * kD];
    } else if (t == kD) {
        s.mean = stats[2 * kD + 1];
        s.var = stats[2 * kD + 2];
        s.count = stats[2 * kD + 3];
    }
    return s;
}

// np.mean (bret[0]) and np.var (bret[1]) of the n updated returns in rbuf (LDS, written by
// their threads, no barrier yet; left holding the squares): NumPy's pairwise sum with one
// thread per tree node (sb3::pw_node) -- the leaves side by side, then the splits level by
// level, once for the mean and once over (x - mean)^2.  nval: sb3::kNodes node sums (LDS).
// Every thread of the workgroup calls it and gets both values.
__device__ __forceinline__ void sb3_returns_moments(int n, double* rbuf, double* nval, double* bret) {
    const int t = threadIdx.x;
    // thread t is node t of the pairwise tree: a leaf, a split or (most) nothing
    const int levels = sb3::pw_levels(n);
    const sb3::Node nd = t >= 1 && t < (2 << levels) ? sb3::pw_node(n, t) : sb3::Node{0, 0};
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        if (nd.n > 0 && nd.n <= sb3::kLeafMax) nval[t] = sb3::pw_leaf(rbuf + nd.lo, nd.n);
        __syncthreads();
        for (int d = levels - 1; d >= 0; --d) {   // the splits of level d, their halves done
            if (nd.n > sb3::kLeafMax && (t >> d) == 1) nval[t] = nval[2 * t] + nval[2 * t + 1];
            __syncthreads();
        }
        bret[pass] = nval[1] / (double)n;
        if (pass == 0) {
            for (int r = t; r < n; r += kVnThreads) {
                const double d = rbuf[r] - bret[0];
                rbuf[r] = d * d;
            }
            __syncthreads();   // also: every thread has read nval[1] before the second pass writes it
        }
    }
}

// The 14 statistics of moments = sb3: RunningMeanStd.update_from_moments on the lanes'
// columns (bmean / bvar: lanes 0 .. 12's np.mean / np.var of their obs column; bret: the
// returns'), stored, and the columns' constants for sb3::norm_obs / norm_rew into LDS
// (smean, ssd [kD], srsd; the caller barriers).
__device__ __forceinline__ void sb3_update_stats(StatLane st, bool upd_obs, bool upd_ret, float bmean, float bvar,
                                                 const double* bret, int n, double* stats, double eps, double* smean,
                                                 double* ssd, double* srsd) {
    const int t = threadIdx.x;
    if (t < kD) {
        if (upd_obs) {
            sb3::rms_update(&st.mean, &st.var, &st.count, (double)bmean, sb3::batch_m2_obs(bvar, n), (double)n);
            stats[t] = st.mean;
            stats[kD + t] = st.var;
            if (t == 0) stats[2 * kD] = st.count;
        }
        smean[t] = st.mean;
        ssd[t] = sb3::norm_sd(st.var, eps);
    } else if (t == kD) {
        if (upd_ret) {
            sb3::rms_update(&st.mean, &st.var, &st.count, bret[0], bret[1] * (double)n, (double)n);
            stats[2 * kD + 1] = st.mean;
            stats[2 * kD + 2] = st.var;
            stats[2 * kD + 3] = st.count;
        }
        *srsd = sb3::norm_sd(st.var, eps);
    }
}

// ------------------------------------------------------------------ the step over rows in LDS
// he_vecnorm_attach_step's arguments: the two halves' blocks (m: n, upd_obs, upd_ret, gamma,
// returns, stats; no partials) and the mode.
struct StepArgs {
    MomentsArgs m;
    ApplyArgs a;
    int32_t training;
};
struct StepShared {
    FrozenNorm z;                  // the columns' constants, whichever mode made them
    double rbuf[kVnChunk];         // the updated returns
    double nval[4];                // sb3: the pairwise tree of <= 256 elements (a root, two leaves)
    double ssum[kPart];            // f64: the shifted sums
};
static_assert(kVnChunk <= 2 * sb3::kLeafMax, "StepShared::nval: one level of splits");
// f64 training, the order of the shifted sums -- the bits of the route the same he_step would
// take with he_vecnorm_attach: kColumns, step1_vn_kernel's moments_from_rows (no info fields);
// kBlock, moments_body + block_sum of vn_moments_after_step_kernel (info fields requested).
// They agree to rounding only (vn_moments.h), so the kernel's INFO parameter picks.
enum SumOrder { kColumns, kBlock };
// What a thread loads before the rows exist (off the step's critical path): its lane's
// statistics, its row's running return and Monitor sums, its column's shift (f64 training).
struct StepPre {
    StatLane st;
    double ret_prev, shift, er;
    int32_t el;
};
template <SumOrder ORDER>
__device__ __forceinline__ StepPre load_step(const StepArgs& w, bool live) {
    const int t = threadIdx.x;
    StepPre p{load_stat_lane(w.m.stats), 0.0, 0.0, 0.0, 0};
    if (w.training && !w.a.sb3) p.shift = ORDER == kBlock ? load_block_shift(w.m) : load_col_shift(w.m);
    if (w.m.upd_ret && live) p.ret_prev = w.m.returns[t];
    if (w.a.ep_ret && live) {
        p.er = w.a.ep_ret[t];
        p.el = w.a.ep_len[t];
    }
    return p;
}
// Frozen statistics: the columns' constants before the rows exist (prep_frozen; the caller's
// barrier after its rows publishes them).
__device__ __forceinline__ void prep_step(const StepArgs& w, StepShared& sh, const StepPre& p) {
    if (!w.training) prep_frozen(sh.z, w.a, FrozenPre{p.st.mean, p.st.var, p.er, p.el});
}
// Rows [0, rows) of the workgroup, rows <= kVnChunk, obs row t at tile + t kD and a done
// row's terminal obs at ttile + t kD (both LDS), after a workgroup barrier; thread t < rows
// owns row t: its reward (f32 for VecNormalize, f64 for Monitor) and done flag.  Every thread
// of the workgroup calls it (barriers inside) and returns from it.
template <SumOrder ORDER>
__device__ __forceinline__ void step_rows(const StepArgs& w, StepShared& sh, const StepPre& p, int rows,
                                          const float* tile, const float* ttile, float rew, double rew64, bool done) {
    const int t = threadIdx.x;
    const ApplyArgs& a = w.a;
    if (!w.training) {   // uniform, as every mode branch below
        apply_frozen_rows(a, sh.z, 0, rows, tile, FrozenPre{p.st.mean, p.st.var, p.er, p.el}, rew, rew64, done, ttile);
        return;
    }
    const RowIn in{rew, done, p.er, rew64, p.el};
    const auto elem = [tile](int, int k) { return tile[k]; };
    float* const dst = a.obs_out;
    const SplitNorm split{sh.z.cn, &sh.z.rinv, (float)a.clip_obs, a.clip_rew};
    const Sb3Norm sb{sh.z.m, sh.z.sd, &sh.z.rsd, a.clip_obs, a.clip_rew};
    if (a.sb3) {   // vn_sb3_kernel with the whole batch in one LDS chunk
        double bret[2] = {0.0, 1.0};
        if (w.m.upd_ret) {
            if (t < rows) {
                const double ret = sb3::ret_update(p.ret_prev, w.m.gamma, rew);
                w.m.returns[t] = ret;
                sh.rbuf[t] = ret;
            }
            sb3_returns_moments(rows, sh.rbuf, sh.nval, bret);
        }
        float bmean = 0.0f, bvar = 0.0f;
        if (w.m.upd_obs) {
            float v = 0.0f;
            if (t < kD) {
                bmean = sb3::col_sum(0.0f, true, tile + t, rows) / (float)rows;
                v = sb3::col_sq(0.0f, true, bmean, tile + t, rows);
            }
            bvar = v / (float)rows;
        }
        sb3_update_stats(p.st, w.m.upd_obs != 0, w.m.upd_ret != 0, bmean, bvar, bret, rows, w.m.stats, a.eps, sh.z.m,
                         sh.z.sd, &sh.z.rsd);
        __syncthreads();
        // the f64 divisions take the rolled pass (registers, as apply_frozen_rows)
        if (a.norm_obs)
            obs_pass<kStrided>(dst, rows * kD, true, sb, elem);
        else
            obs_pass<kUnrolled>(dst, rows * kD, false, split, elem);
        if (t < rows) row_tail(a, sb, ttile, t, in);
        return;
    }
    // moments = f64: vn_moments_kernel's partial of this one workgroup, then vn_apply_kernel's
    // merge of one partial (the sums themselves; the old statistics and the shifts are the
    // lanes' registers instead of the snapshot), update and apply
    if (ORDER == kColumns) {   // moments_from_rows' sums, kept in LDS (w.m.rows_per_block = kVnChunk)
        double* const ssum = sh.ssum;
        moments_rows_to(w.m, 0, tile, rew, p.ret_prev, p.shift, [ssum](int v, double x) { ssum[v] = x; });
    } else {
        if (w.m.upd_ret && t < rows) {
            const double ret = p.ret_prev * w.m.gamma + (double)rew;   // VecNormalize._update_reward
            w.m.returns[t] = ret;
            sh.rbuf[t] = ret;
        }
        __syncthreads();
        moments_rows_block_order(w.m, tile, sh.rbuf, rows, p.shift, sh.ssum);
    }
    __syncthreads();
    if (t <= kD) {
        const int c = t;
        double mean = p.st.mean, var = p.st.var;
        if ((c < kD && w.m.upd_obs) || (c == kD && w.m.upd_ret)) {
            const double n_a = (double)rows;
            double count = p.st.count, mean_a, m_b;
            batch_from_sums(p.st.mean, n_a, sh.ssum[c], sh.ssum[kD + 1 + c], &mean_a, &m_b);
            sb3::rms_update(&mean, &var, &count, mean_a, m_b, n_a);
            const int im = (c < kD) ? c : 2 * kD + 1, iv = (c < kD) ? kD + c : 2 * kD + 2;
            if (c == 0) w.m.stats[2 * kD] = count;
            if (c == kD) w.m.stats[2 * kD + 3] = count;
            w.m.stats[im] = mean;
            w.m.stats[iv] = var;
        }
        if (c < kD)
            sh.z.cn[c] = col_norm(mean, var, a.eps);
        else
            sh.z.rinv = 1.0 / sqrt(var + a.eps);
    }
    __syncthreads();
    obs_pass<kUnrolled>(dst, rows * kD, a.norm_obs != 0, split, elem);
    if (t < rows) row_tail(a, split, ttile, t, in);
}

}  // namespace vn
