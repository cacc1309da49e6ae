// vn_moments.h -- the first half of a VecNormalize step (SB3 2.6.0 VecNormalize.step_wait:
// obs_rms.update(obs), returns = returns * gamma + reward, ret_rms.update(returns);
// train_ppo_v2.py:204,305), shared by vecnorm.hip's vn_moments_kernel and by hedge_env.hip's
// step1_vn_kernel, which runs it as the epilogue of he_step on the rows its workgroup has
// just written (he_vecnorm_attach).
//
// Per workgroup of kVnThreads threads and up to rows_per_block rows: one pass of f64 sums
// S1 = sum d and S2 = sum d^2 with d = x - shift over the 13 obs columns and the updated
// running returns, stored as partial [kPart][kVnMaxBlocks] (count, S1[D + 1], S2[D + 1]);
// workgroup 0 also stores a snapshot of the old statistics and the shifts (store_snapshot),
// which vn_apply_kernel (vecnorm.hip) reads after the kernel boundary.  The second half of the
// step -- normalisers, obs pass, a row's tail, the fused eval step -- is vn_apply.h; the whole
// step by one workgroup (vn_step.h) takes the same sums from rows in LDS
// (moments_rows_block_order) and the batch moments from them as the merge does (batch_from_sums).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hedge_env.h"
#include "vn_sb3.h"

namespace vn {

constexpr int kD = HE_OBS_DIM;
constexpr int kVnThreads = 256;
constexpr int kVnMaxBlocks = 256;   // workgroups of a launch = partials merged per workgroup (one per thread)
constexpr int kVnChunk = kVnThreads;   // rows staged in LDS at a time (one per thread)
// scratch layout: [kPart][kVnMaxBlocks] doubles, then the 2 kD + 4 old statistics and
// the kD + 1 shifts of the sums
constexpr int kPart = 2 * kD + 3;   // count, S1[D + 1] (obs, returns), S2[D + 1]

struct MomentsArgs {
    int64_t n;
    int32_t rows_per_block;
    int32_t upd_obs, upd_ret;
    int32_t shift_mean;      // obs shift: 1 the old running mean (the fused epilogue: row 0 is
                             // another workgroup's output), 0 the batch's row 0
    double gamma;
    const float* obs;
    const float* reward;
    double* returns;
    double* stats;           // read here; the merge (vn_apply_kernel, vn_sb3_kernel) stores the update
    double* part;
};
// The half's arguments from the caller's parameters and buffers (host).  The site adds what is
// its own: rows_per_block, shift_mean, the obs and reward of the launch.
inline MomentsArgs moments_args(const he_vecnorm_params* p, int64_t n, double* returns, double* stats, void* scratch) {
    MomentsArgs m = {};
    m.n = n;
    m.upd_obs = p->training && p->norm_obs;
    m.upd_ret = p->training != 0;
    m.gamma = p->gamma;
    m.returns = returns;
    m.stats = stats;
    m.part = (double*)scratch;   // [kPart][kVnMaxBlocks] partials, then the old statistics and the shifts
    return m;
}

// Sum of v[0..NV) over the block into out[0..NV) (LDS), NV <= 32: every thread stores
// its NV values (row stride NV + 1), then TPV = 16 (NV <= 16) or 8 threads per value sum
// 256 / TPV rows each and finish with a butterfly inside their TPV-lane group -- against
// 6 shuffle levels per value (~180 LDS permutes per wave) of a butterfly over the whole
// wave.  The summation order is fixed.
template <int NV>
__device__ __forceinline__ void block_sum(const double* v, double* buf, double* out) {
    constexpr int TPV = NV <= 16 ? 16 : 8;
    static_assert(NV <= 32 && NV * TPV <= kVnThreads, "threads per value");
    constexpr int S = NV + 1;
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < NV; ++c) buf[t * S + c] = v[c];
    __syncthreads();
    if (t < NV * TPV) {
        const int c = t / TPV, j = t % TPV;
        double x = 0.0;
#pragma unroll
        for (int k = 0; k < kVnThreads / TPV; ++k) x += buf[(j + TPV * k) * S + c];
#pragma unroll
        for (int m = TPV / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, TPV);
        if (j == 0) out[c] = x;
    }
    __syncthreads();
}

// moments_body's partial of ONE workgroup whose rows are already in LDS (obs row r at
// tile + r * kD, the updated running returns in rbuf), bit for bit, without block_sum's 59 KB
// buffer: value c of v[] (S1 then S2, column c % (kD + 1), the returns last) is summed by the
// same 8 threads over the same rows in the same order -- thread (c, j) the rows j, j + 8, ...,
// then the butterfly over its 8-lane group -- each row's term made from the tile where
// block_sum reads it back.  A row past `rows`, or a value that is not updated, adds the 0.0
// moments_body leaves there.  shift: this thread's column's (load_block_shift).  The sums land
// in ssum[0 .. kPart - 1) in v[]'s order (LDS; the caller barriers before reading them).
constexpr int kBlockTpv = 8;   // block_sum<kPart - 1>'s threads per value
__device__ __forceinline__ double load_block_shift(const MomentsArgs& a) {
    const int c = (int)(threadIdx.x / kBlockTpv) % (kD + 1);
    return a.stats[c < kD ? c : 2 * kD + 1];
}
__device__ __forceinline__ void moments_rows_block_order(const MomentsArgs& a, const float* tile, const double* rbuf,
                                                         int rows, double shift, double* ssum) {
    static_assert((kPart - 1) * kBlockTpv <= kVnThreads && kPart - 1 > 16, "block_sum<kPart - 1>: 8 threads per value");
    const int t = threadIdx.x;
    if (t >= (kPart - 1) * kBlockTpv) return;
    const int c = t / kBlockTpv, j = t % kBlockTpv;
    const int col = c % (kD + 1);
    const bool sq = c > kD;
    const bool on = col < kD ? a.upd_obs != 0 : a.upd_ret != 0;
    double x = 0.0;
#pragma unroll 4
    for (int k = 0; k < kVnThreads / kBlockTpv; ++k) {
        const int r = j + kBlockTpv * k;
        double term = 0.0;
        if (on && r < rows) {
            const double d = (col < kD ? (double)tile[r * kD + col] : rbuf[r]) - shift;
            term = sq ? d * d : d;
        }
        x += term;
    }
#pragma unroll
    for (int m = kBlockTpv / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kBlockTpv);
    if (j == 0) ssum[c] = x;
}

// np.mean and np.var(ddof=0) * n of a batch of n_a values from their shifted sums
// s1 = sum d, s2 = sum d^2, d = x - shift: what RunningMeanStd.update_from_moments takes
// (vn_apply_kernel's merge and the one-workgroup step of vn_step.h).
__device__ __forceinline__ void batch_from_sums(double shift, double n_a, double s1, double s2, double* mean_a,
                                                double* m_b) {
    *mean_a = shift + s1 / n_a;
    const double m2 = s2 - s1 * (s1 / n_a);
    const double var_a = (m2 > 0.0 ? m2 : 0.0) / n_a;
    *m_b = var_a * n_a;
}

// Rows [c0, c0 + rows) of obs -> LDS tile, as a flat coalesced copy (the [N][13] rows are
// 52 B apart: per-row loads would touch 26 cache lines per wave instruction); the rows
// are then read from LDS with a stride of 13 words (odd: no bank conflicts).
__device__ __forceinline__ void load_tile(float* tile, const float* obs, int64_t c0, int rows) {
    const float* src = obs + c0 * kD;
    const int nf = rows * kD;
    for (int k = threadIdx.x; k < nf; k += kVnThreads) tile[k] = src[k];
    __syncthreads();
}

// Workgroup 0's snapshot, after the partials: the old statistics and the shifts of the sums
// (shift_t: column t's, of thread t <= kD), which the merge reads after the kernel boundary.
__device__ __forceinline__ void store_snapshot(const MomentsArgs& a, int bid, double shift_t) {
    const int t = threadIdx.x;
    double* snap = a.part + kVnMaxBlocks * kPart;
    if (bid == 0 && t < 2 * kD + 4) snap[t] = a.stats[t];
    if (bid == 0 && t <= kD) snap[2 * kD + 4 + t] = shift_t;
}

// The block sum of a workgroup's moments v, stored as its partial (+ the snapshot).
__device__ __forceinline__ void store_partial(const MomentsArgs& a, int bid, const double* v, const double* sft,
                                             int64_t rows) {
    __shared__ double sh[kVnThreads * (kPart + 1)];
    __shared__ double ssum[kPart];
    const int t = threadIdx.x;
    block_sum<kPart - 1>(v, sh, ssum);
    double* part = a.part + bid;
    if (t < kPart - 1) part[(1 + t) * kVnMaxBlocks] = ssum[t];
    if (t == 0) part[0] = (double)rows;
    store_snapshot(a, bid, sft[t <= kD ? t : 0]);
}

// The moments of workgroup `bid`'s rows (blockDim.x == kVnThreads).
__device__ __forceinline__ void moments_body(const MomentsArgs& a, int bid) {
    __shared__ float tile[kVnChunk * kD];
    const int64_t r0 = (int64_t)bid * a.rows_per_block;
    const int64_t r1 = (r0 + a.rows_per_block < a.n) ? r0 + a.rows_per_block : a.n;
    const int t = threadIdx.x;
    double sft[kD + 1];
#pragma unroll
    for (int c = 0; c < kD; ++c) sft[c] = a.shift_mean ? a.stats[c] : (double)a.obs[c];
    sft[kD] = a.stats[2 * kD + 1];
    double v[kPart - 1];
#pragma unroll
    for (int c = 0; c < kPart - 1; ++c) v[c] = 0.0;
    for (int64_t c0 = r0; c0 < r1; c0 += kVnChunk) {
        const int rows = (int)((r1 - c0) < kVnChunk ? (r1 - c0) : kVnChunk);
        if (a.upd_obs) load_tile(tile, a.obs, c0, rows);
        if (t < rows) {
            if (a.upd_obs) {
#pragma unroll
                for (int c = 0; c < kD; ++c) {
                    const double d = (double)tile[t * kD + c] - sft[c];
                    v[c] += d;
                    v[kD + 1 + c] += d * d;
                }
            }
            if (a.upd_ret) {
                const int64_t r = c0 + t;
                const double ret = a.returns[r] * a.gamma + (double)a.reward[r];   // VecNormalize._update_reward
                a.returns[r] = ret;
                const double d = ret - sft[kD];
                v[kD] += d;
                v[2 * kD + 1] += d * d;
            }
        }
        __syncthreads();
    }
    store_partial(a, bid, v, sft, r1 > r0 ? r1 - r0 : 0);
}

// The same moments from rows already in LDS (step1_vn_kernel: the he_step workgroup's obs
// staging tile, row t at tile + t * kD, after a workgroup barrier), the thread's reward
// `rew` (its row r0 + t) and its running return before the update `ret_prev`, with no global
// round trip.  Obs shift: the old running mean (a.shift_mean).
// col_shift: this thread's column's shift (the old running mean of obs column t % (kD + 1),
// or of the returns), loaded by the caller before its step so it is not a round trip here.
__device__ __forceinline__ double load_col_shift(const MomentsArgs& a) {
    const int c = (int)(threadIdx.x % (kD + 1));
    return a.stats[c < kD ? c : 2 * kD + 1];
}
// Column-major over the LDS rows: thread t < kColThreads takes column c = t % (kD + 1)
// (13 obs columns, then the returns) and rows g, g + kColGroups, ... (g = t / (kD + 1)), summing
// d and d^2 of its rows in f64; the kColGroups group sums of each column are then added in group
// order by 2 (kD + 1) threads.  ~6 KB of LDS traffic per workgroup against the row-major
// block_sum's 57 KB (every thread's 28 values written, then read back): the fused epilogue's
// cost on the step kernel.  The summation order differs from moments_body's (row-major), so
// the statistics agree to rounding, not bit for bit (test_fused_moments_equal_separate_launch).
constexpr int kColGroups = kVnThreads / (kD + 1);            // 18
constexpr int kColThreads = kColGroups * (kD + 1);           // 252
// moments_rows_to: the sums themselves, handed to sink(v, x) -- value v of the partial
// (v = w (kD + 1) + c: S1 then S2 of column c) by thread v -- so that the one-workgroup step
// (vn_step.h) keeps them in LDS where moments_from_rows stores the partial.
template <class Sink>
__device__ __forceinline__ int moments_rows_to(const MomentsArgs& a, int bid, const float* tile, float rew,
                                               double ret_prev, double col_shift, Sink sink) {
    __shared__ double rbuf[kVnThreads];
    __shared__ double red[kColGroups][kD + 1][2];
    const int64_t r0 = (int64_t)bid * a.rows_per_block;
    const int64_t r1 = (r0 + a.rows_per_block < a.n) ? r0 + a.rows_per_block : a.n;
    const int rows = (int)(r1 > r0 ? r1 - r0 : 0);
    const int t = threadIdx.x;
    if (a.upd_ret && t < rows) {
        const double ret = ret_prev * a.gamma + (double)rew;   // VecNormalize._update_reward
        a.returns[r0 + t] = ret;
        rbuf[t] = ret;
    }
    __syncthreads();
    if (t < kColThreads) {
        const int c = t % (kD + 1), g = t / (kD + 1);
        double s1 = 0.0, s2 = 0.0;
        if (c < kD ? a.upd_obs : a.upd_ret) {
            const double sh = col_shift;
            for (int r = g; r < rows; r += kColGroups) {
                const double x = (c < kD) ? (double)tile[r * kD + c] : rbuf[r];
                const double d = x - sh;
                s1 += d;
                s2 += d * d;
            }
        }
        red[g][c][0] = s1;
        red[g][c][1] = s2;
    }
    __syncthreads();
    if (t < 2 * (kD + 1)) {
        const int w = t / (kD + 1), c = t % (kD + 1);
        double x = 0.0;
#pragma unroll
        for (int g = 0; g < kColGroups; ++g) x += red[g][c][w];
        sink(w * (kD + 1) + c, x);
    }
    return rows;
}
__device__ __forceinline__ void moments_from_rows(const MomentsArgs& a, int bid, const float* tile, float rew,
                                                  double ret_prev, double col_shift) {
    // partial layout: [count, S1[kD + 1], S2[kD + 1]] (S1[kD] / S2[kD]: the returns)
    const int rows = moments_rows_to(a, bid, tile, rew, ret_prev, col_shift,
                                     [&a, bid](int v, double x) { a.part[(1 + v) * kVnMaxBlocks + bid] = x; });
    if (threadIdx.x == 0) a.part[bid] = (double)rows;
    store_snapshot(a, bid, col_shift);   // thread t <= kD: column t
}

}  // namespace vn
