// vecnorm.hip -- VecNormalize and Monitor statistics on the device (part of libhedgeenv;
// C ABI in include/hedge_env.h).
//
// The reference trains behind SB3 2.6.0's VecNormalize(norm_obs=True, norm_reward=True,
// gamma) (train_ppo_v2.py:204,305) and evaluates with the stats frozen (:450-453); every
// env is wrapped in Monitor(info_keywords=...) (:119).  On the host that is a NumPy
// pass over [N, 13] per step plus per-env Python lists -- the bottleneck once N is in
// the tens of thousands.  Here one step is two launches of G <= 256 workgroups, each
// owning a slice of 256 rows staged through LDS as flat coalesced copies:
//   vn_moments_kernel  one pass of f64 sums of d and d^2, d = x - shift (the batch's row 0
//                      for obs, the old running mean for the returns), over the slice's obs
//                      columns and updated running returns, stored as a partial (+ a
//                      snapshot of the old statistics and the shifts);
//   vn_apply_kernel    every workgroup merges all G partials itself (one block reduction in
//                      a fixed order, so the same result everywhere), applies
//                      RunningMeanStd.update_from_moments (workgroup 0 stores it), and
//                      normalizes its rows by (x - mean) * (1 / sqrt(var + eps)): obs /
//                      reward / terminal obs, returns[done] = 0 and the Monitor episode sums.
// Deterministic for a given grid; no atomics and no waiting between workgroups (the
// kernel boundary publishes the partials).  Eval mode (no statistics update) is the
// second launch alone.  68 B of obs + reward read and written per env.
//
// moments = HE_VN_MOMENTS_SB3 (n <= 4096) is one launch of one workgroup instead,
// vn_sb3_kernel: SB3's own NumPy arithmetic bit for bit (vn_sb3.h) -- the f32 row-order sums
// of the obs columns are one dependent chain per column, which no second workgroup could help.
//
// This file holds the kernels, their argument block and the C entry points.  What the kernels
// share with the epilogues fused into he_step (hedge_env.hip) and with the host mirror is in the
// headers: the moments and the snapshot in vn_moments.h; the normalisers, the flat obs pass, a
// row's tail and ApplyArgs in vn_apply.h; SB3's arithmetic, clipd and rms_update in vn_sb3.h; the
// workgroup-wide parts of vn_sb3_kernel, and the whole step of <= 256 envs inside he_step's own
// launch (he_vecnorm_attach_step), in vn_step.h.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/hedge_env.h"
#include "vn_apply.h"
#include "vn_moments.h"
#include "vn_sb3.h"
#include "vn_step.h"

namespace {

using vn::kD;
using vn::kPart;
using vn::kVnChunk;
using vn::kVnMaxBlocks;
using vn::kVnThreads;
using vn::block_sum;
using vn::load_tile;
using vn::ColNorm;
using vn::col_norm;
using vn::RowIn;

// A launch's arguments: the two halves (vn_moments.h, vn_apply.h; base_args) and what only
// these kernels read.
struct VnArgs {
    vn::MomentsArgs m;         // m.upd_ret: training && !reset
    vn::ApplyArgs a;
    const uint8_t* done;
    const float* tobs;
    const double* ep_reward;   // the env's f64 step rewards Monitor sums (he_info::reward_step)
    int blocks;
    int reset;   // he_vecnorm_reset: returns = 0 instead of the discounted update
};

struct VnRows {
    int64_t r0, r1;
    double cnt;
};
__device__ __forceinline__ VnRows rows_of(const vn::MomentsArgs& a) {
    VnRows w;
    w.r0 = (int64_t)blockIdx.x * a.rows_per_block;
    w.r1 = (w.r0 + a.rows_per_block < a.n) ? w.r0 + a.rows_per_block : a.n;
    w.cnt = (double)(w.r1 > w.r0 ? w.r1 - w.r0 : 0);
    return w;
}

// Launch 1 (training): the moments partials of each workgroup's rows (vn_moments.h;
// the obs shift is the batch's row 0).  The kernel boundary publishes the partials to
// launch 2 -- no atomics, no waiting (a single launch with a grid-wide wait measured
// 25 us at 65,536 envs: four dependent device-coherent round trips between workgroups).
__global__ void __launch_bounds__(kVnThreads) vn_moments_kernel(vn::MomentsArgs m) {
    vn::moments_body(m, blockIdx.x);
}

// A row's inputs (vn::RowIn) from memory.
__device__ __forceinline__ RowIn row_in(const VnArgs& a, int64_t r) {
    RowIn in;
    in.rw = a.m.reward[r];
    in.dn = a.done ? a.done[r] != 0 : false;
    in.er = a.a.ep_ret ? a.a.ep_ret[r] : 0.0;
    in.rw64 = a.a.ep_ret ? a.ep_reward[r] : 0.0;
    in.el = a.a.ep_ret ? a.a.ep_len[r] : 0;
    return in;
}

constexpr int kMergeLanes = 8;   // lanes per merged value (vn_apply_kernel)
static_assert(kMergeLanes * kPart <= kVnThreads, "one merge lane group per value");

// Launch 2: every workgroup merges all the partials itself (one block reduction in a
// fixed order, so the same statistics everywhere; workgroup 0 stores them), then
// normalizes its rows: obs / reward / terminal obs, returns[done] = 0, Monitor sums.
// (2 or 4 rows per thread, so fewer workgroups read the partials, measured slower: rocprof
// 7.5 / 10.2 / 15.9 us at 65,536 envs, r03s32 -- the merge's reads are not what the launch
// waits on; each thread's rows are.)
__global__ void __launch_bounds__(kVnThreads) vn_apply_kernel(VnArgs a) {
    __shared__ double ssum[kPart];
    __shared__ ColNorm snorm[kD];     // per obs column (col_norm)
    __shared__ double srinv;
    __shared__ float tile[kVnChunk * kD];
    const VnRows w = rows_of(a.m);
    const vn::SplitNorm nz{snorm, &srinv, (float)a.a.clip_obs, a.a.clip_rew};
    const int t = threadIdx.x;
    const bool resident = w.r1 - w.r0 <= kVnChunk;
    const int nrows = (int)(w.r1 - w.r0);
    // the rows' loads first -- obs, and the row's reward, done flag and Monitor sums: they
    // are all in flight while the partials are merged (one memory round trip per launch)
    float xr[kD];
    const int nres = resident ? nrows * kD : 0;
    const float* src = a.m.obs + w.r0 * kD;
#pragma unroll
    for (int q = 0; q < kD; ++q) {
        const int k = t + q * kVnThreads;
        xr[q] = k < nres ? src[k] : 0.0f;
    }
    RowIn pin = {};
    if (resident && !a.reset && t < nrows) pin = row_in(a, w.r0 + t);
    if (a.m.upd_obs || a.m.upd_ret) {
        // the merge, transposed: thread t < 8 kPart sums value c = t / 8 of the partials
        // b = t % 8, t % 8 + 8, ... (in b order), then a butterfly over its 8-lane group --
        // no block-wide LDS reduction (the row-major block_sum stored and re-read 61 KB)
        if (t < kMergeLanes * kPart) {
            const int c = t / kMergeLanes, j = t % kMergeLanes;
            const double* P = a.m.part + (size_t)c * kVnMaxBlocks;
            // every load issued before the first add (unrolled over the kVnMaxBlocks bound):
            // a rolled loop waited one round trip per partial
            double v[kVnMaxBlocks / kMergeLanes];
#pragma unroll
            for (int q = 0; q < kVnMaxBlocks / kMergeLanes; ++q) {
                const int b = j + q * kMergeLanes;
                v[q] = b < a.blocks ? P[b] : 0.0;
            }
            double x = 0.0;
#pragma unroll
            for (int q = 0; q < kVnMaxBlocks / kMergeLanes; ++q) x += v[q];
#pragma unroll
            for (int m = kMergeLanes / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kMergeLanes);
            if (j == 0) ssum[c] = x;   // ssum[0] = n, [1 .. kD + 1] = S1, then S2
        }
        __syncthreads();
        const int c = t;
        if (c <= kD) {
            const double* old = a.m.part + kVnMaxBlocks * kPart;   // launch 1's snapshot
            const double n_a = ssum[0], s1 = ssum[1 + c], s2 = ssum[2 + kD + c];
            // np.mean / np.var(ddof=0) of the batch from the shifted sums, then
            // RunningMeanStd.update_from_moments
            double mean_a, m_b;
            vn::batch_from_sums(old[2 * kD + 4 + c], n_a, s1, s2, &mean_a, &m_b);
            const int im = (c < kD) ? c : 2 * kD + 1, iv = (c < kD) ? kD + c : 2 * kD + 2;
            double mean = old[im], var = old[iv];
            if ((c < kD && a.m.upd_obs) || (c == kD && a.m.upd_ret)) {
                double count = (c < kD) ? old[2 * kD] : old[2 * kD + 3];
                sb3::rms_update(&mean, &var, &count, mean_a, m_b, n_a);
                if (blockIdx.x == 0) {
                    if (c == 0) a.m.stats[2 * kD] = count;
                    if (c == kD) a.m.stats[2 * kD + 3] = count;
                    a.m.stats[im] = mean;
                    a.m.stats[iv] = var;
                }
            }
            if (c < kD) {
                snorm[c] = col_norm(mean, var, a.a.eps);
            } else {
                srinv = 1.0 / sqrt(var + a.a.eps);
            }
        }
        __syncthreads();
    } else {
        if (t < kD) snorm[t] = col_norm(a.m.stats[t], a.m.stats[kD + t], a.a.eps);
        if (t == 0) srinv = 1.0 / sqrt(a.m.stats[2 * kD + 2] + a.a.eps);
        __syncthreads();
    }
    // the rows' own work (reward, returns, terminal obs, Monitor): thread t, row r0 + t
    auto row_work = [&](int64_t r, const RowIn& in) {
        if (a.reset)
            a.m.returns[r] = 0.0;
        else
            vn::row_tail(a.a, nz, a.tobs, r, in);
    };
    if (resident) {
        // the obs element-wise straight from the registers the loads landed in
        vn::obs_pass<vn::kUnrolled>(a.a.obs_out + w.r0 * kD, nres, a.a.norm_obs != 0, nz,
                                    [&xr](int q, int) { return xr[q]; });
        if (t < nrows) row_work(w.r0 + t, pin);
        return;
    }
    for (int64_t c0 = w.r0; c0 < w.r1; c0 += kVnChunk) {
        const int rows = (int)((w.r1 - c0) < kVnChunk ? (w.r1 - c0) : kVnChunk);
        load_tile(tile, a.m.obs, c0, rows);
        if (t < rows) {
            // the row in place in LDS, then stored back as a flat coalesced copy
            if (a.a.norm_obs) {
#pragma unroll
                for (int c = 0; c < kD; ++c) tile[t * kD + c] = nz.obs(tile[t * kD + c], c);
            }
            row_work(c0 + t, a.reset ? RowIn{} : row_in(a, c0 + t));
        }
        __syncthreads();
        float* dst = a.a.obs_out + c0 * kD;
        const int nf = rows * kD;
        for (int k = t; k < nf; k += kVnThreads) dst[k] = tile[k];
        __syncthreads();
    }
}

// moments = HE_VN_MOMENTS_SB3: the whole step -- batch moments, statistics update, apply -- in
// one launch of ONE workgroup, n <= sb3::kMaxN rows, with the arithmetic of vn_sb3.h.
//   returns   every thread updates its rows' returns into LDS; NumPy's pairwise sum takes one
//             thread per tree node (sb3::pw_node): the leaves (<= 128 elements, eight
//             accumulators) side by side, then the splits level by level, once for the mean
//             and once over (x - mean)^2;
//   obs       lanes 0 .. 12 carry the 13 f32 column chains in row order over 256-row chunks
//             staged flat and coalesced into LDS (the next chunk's loads are in flight during
//             the chain), one pass for the sums and one for the squares (a batch of <= 256
//             rows stays in LDS for both);
//   apply     lanes 0 .. 13 update and store the 14 statistics, then all threads normalize:
//             the obs as a flat coalesced pass, then a row per thread as vn_apply_kernel.
// The 2 n dependent f32 adds per column are the critical path at large n.
__global__ void __launch_bounds__(kVnThreads) vn_sb3_kernel(VnArgs a) {
    __shared__ float tile[kVnChunk * kD];
    __shared__ double rbuf[sb3::kMaxN];
    __shared__ double nval[sb3::kNodes];   // the pairwise tree's node sums, heap order
    __shared__ double smean[kD], ssd[kD], srsd;
    const int t = threadIdx.x;
    const int n = (int)a.m.n;
    const bool upd_ret = a.m.upd_ret;
    double bret[2] = {0.0, 1.0};   // the returns' batch mean and variance (every thread)
    // every load that depends on nothing first, in flight together: the first obs chunk, the
    // thread's first row (reward, done flag, Monitor sums, running return) and the statistics
    float nx[kD];
    auto fetch = [&](int ch) {
        const float* src = a.m.obs + (size_t)ch * kVnChunk * kD;
        const int nf = (n - ch * kVnChunk < kVnChunk ? n - ch * kVnChunk : kVnChunk) * kD;
#pragma unroll
        for (int q = 0; q < kD; ++q) {
            const int k = t + q * kVnThreads;
            nx[q] = k < nf ? src[k] : 0.0f;
        }
    };
    const bool tile_all = n <= kVnChunk;   // the whole batch is the first chunk: nx serves the apply too
    if (a.m.upd_obs || tile_all) fetch(0);
    RowIn pin = {};
    if (!a.reset && t < n) pin = row_in(a, t);
    double ret0 = upd_ret && t < n ? a.m.returns[t] : 0.0;
    const vn::StatLane st = vn::load_stat_lane(a.m.stats);   // lanes 0 .. 12 an obs column, lane 13 the returns
    if (upd_ret) {
        for (int r = t; r < n; r += kVnThreads) {
            const double ret = r == t ? sb3::ret_update(ret0, a.m.gamma, pin.rw)
                                      : sb3::ret_update(a.m.returns[r], a.m.gamma, a.m.reward[r]);
            a.m.returns[r] = ret;
            rbuf[r] = ret;
        }
        vn::sb3_returns_moments(n, rbuf, nval, bret);
    }
    float bmean = 0.0f, bvar = 0.0f;   // lanes 0 .. 12: np.mean / np.var of their obs column
    if (a.m.upd_obs) {
        const int nchunks = (n + kVnChunk - 1) / kVnChunk;
        const int iters = nchunks == 1 ? 1 : 2 * nchunks;   // one chunk serves both passes from LDS
        float s = 0.0f, v = 0.0f;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int q = 0; q < kD; ++q) tile[t + q * kVnThreads] = nx[q];
            __syncthreads();
            const int ch = it < nchunks ? it : it - nchunks;
            if (it + 1 < iters) fetch(it + 1 < nchunks ? it + 1 : it + 1 - nchunks);
            const int rows = n - ch * kVnChunk < kVnChunk ? n - ch * kVnChunk : kVnChunk;
            if (t < kD) {
                if (it < nchunks) {
                    s = sb3::col_sum(s, ch == 0, tile + t, rows);
                    if (ch == nchunks - 1) bmean = s / (float)n;
                }
                if (it >= nchunks || nchunks == 1) v = sb3::col_sq(v, ch == 0, bmean, tile + t, rows);
            }
            __syncthreads();
        }
        bvar = v / (float)n;
    }
    // the 14 statistics: RunningMeanStd.update_from_moments, stored, and the columns' constants
    vn::sb3_update_stats(st, a.m.upd_obs != 0, upd_ret, bmean, bvar, bret, n, a.m.stats, a.a.eps, smean, ssd, &srsd);
    __syncthreads();
    const vn::Sb3Norm nz{smean, ssd, &srsd, a.a.clip_obs, a.a.clip_rew};
    if (tile_all) {   // the thread's elements are still in its registers
        vn::obs_pass<vn::kUnrolled>(a.a.obs_out, n * kD, a.a.norm_obs != 0, nz, [&nx](int q, int) { return nx[q]; });
    } else {
        const float* obs = a.m.obs;
        vn::obs_pass<vn::kStrided>(a.a.obs_out, n * kD, a.a.norm_obs != 0, nz, [obs](int, int k) { return obs[k]; });
    }
    for (int r = t; r < n; r += kVnThreads) {
        if (a.reset)
            a.m.returns[r] = 0.0;
        else
            vn::row_tail(a.a, nz, a.tobs, r, r == t ? pin : row_in(a, r));
    }
}

int blocks_for(int64_t n) {
    int64_t b = (n + kVnChunk - 1) / kVnChunk;   // one row per thread up to 65,536 envs
    if (b > kVnMaxBlocks) b = kVnMaxBlocks;
    return (int)(b < 1 ? 1 : b);
}

__global__ void init_kernel(double* stats) {
    const int i = threadIdx.x;
    if (i < kD) {
        stats[i] = 0.0;
        stats[kD + i] = 1.0;
    }
    if (i == 0) {
        stats[2 * kD] = 1e-4;
        stats[2 * kD + 1] = 0.0;
        stats[2 * kD + 2] = 1.0;
        stats[2 * kD + 3] = 1e-4;
    }
}

he_status launch(VnArgs& a, hipStream_t s, bool moments = true) {
    if (a.a.sb3) {   // the whole step in one workgroup (the caller checked n <= sb3::kMaxN)
        a.blocks = 1;
        a.m.rows_per_block = (int)a.m.n;
        hipLaunchKernelGGL(vn_sb3_kernel, dim3(1), dim3(kVnThreads), 0, s, a);
        return hipGetLastError() == hipSuccess ? HE_OK : HE_EHIP;
    }
    a.blocks = blocks_for(a.m.n);
    a.m.rows_per_block = (int)((a.m.n + a.blocks - 1) / a.blocks);
    if (moments && (a.m.upd_obs || a.m.upd_ret)) {
        hipLaunchKernelGGL(vn_moments_kernel, dim3(a.blocks), dim3(kVnThreads), 0, s, a.m);
        if (hipGetLastError() != hipSuccess) return HE_EHIP;
    }
    hipLaunchKernelGGL(vn_apply_kernel, dim3(a.blocks), dim3(kVnThreads), 0, s, a);
    return hipGetLastError() == hipSuccess ? HE_OK : HE_EHIP;
}

bool params_ok(const he_vecnorm_params* p) {
    return p && p->obs_dim == kD && isfinite(p->gamma) && p->clip_obs >= 0.0 && p->clip_reward >= 0.0 &&
           p->epsilon >= 0.0 && (p->moments == HE_VN_MOMENTS_F64 || p->moments == HE_VN_MOMENTS_SB3);
}
// moments = HE_VN_MOMENTS_SB3 covers one workgroup's rows
bool count_ok(const he_vecnorm_params* p, int64_t n) {
    return p->moments != HE_VN_MOMENTS_SB3 || n <= sb3::kMaxN;
}

// The two halves of a launch over n rows of obs (reward NULL: he_vecnorm_reset); out.stats = stats.
VnArgs base_args(const he_vecnorm_params* p, int64_t n, const float* obs, const float* reward, double* stats,
                 void* scratch, const he_vecnorm_out& out) {
    VnArgs a = {};
    a.reset = reward == nullptr;
    a.m = vn::moments_args(p, n, out.returns, stats, scratch);
    a.m.upd_ret = a.m.upd_ret && !a.reset;
    a.m.obs = obs;
    a.m.reward = reward;
    a.a = vn::apply_args(p, out);
    return a;
}

__global__ void __launch_bounds__(kVnThreads) nonfinite_kernel(const float* __restrict__ a, int64_t n,
                                                               unsigned long long* count) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kVnThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVnThreads)
        c += isfinite(a[i]) ? 0ull : 1ull;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

}  // namespace

extern "C" {

he_status he_count_nonfinite(const float* a, int64_t n, unsigned long long* count, void* stream) {
    if (n < 0 || !count || (n > 0 && !a)) return HE_EINVAL;
    if (n == 0) return HE_OK;
    int64_t blocks = (n + kVnThreads - 1) / kVnThreads;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(nonfinite_kernel, dim3((unsigned)blocks), dim3(kVnThreads), 0, (hipStream_t)stream, a, n, count);
    return hipGetLastError() == hipSuccess ? HE_OK : HE_EHIP;
}


int64_t he_vecnorm_stats_len(int32_t obs_dim) { return 2 * (int64_t)obs_dim + 4; }

int64_t he_vecnorm_scratch_bytes(int64_t n, int32_t obs_dim) {
    (void)n;
    (void)obs_dim;
    return ((int64_t)kVnMaxBlocks * kPart + 3 * kD + 5) * (int64_t)sizeof(double);  // partials + old statistics + shifts
}

he_status he_vecnorm_init(double* stats, int32_t obs_dim, void* stream) {
    if (!stats || obs_dim != kD) return HE_EINVAL;
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats);
    return hipGetLastError() == hipSuccess ? HE_OK : HE_EHIP;
}

static he_status vecnorm_step(const he_vecnorm_params* p, int64_t n, const float* obs, const float* reward,
                              const uint8_t* done, const float* terminal_obs, double* returns, double* stats,
                              void* scratch, float* obs_out, float* reward_out, float* terminal_obs_out,
                              double* ep_return, int32_t* ep_length, double* ep_return_done,
                              int32_t* ep_length_done, const double* ep_reward, void* stream, bool moments) {
    if (!params_ok(p) || n < 0 || !count_ok(p, n)) return HE_EINVAL;
    if (n == 0) return HE_OK;
    if (!obs || !reward || !returns || !stats || !scratch || !obs_out || !reward_out) return HE_EINVAL;
    if ((ep_return != nullptr) != (ep_length != nullptr) ||
        (ep_return && (!ep_return_done || !ep_length_done || !done || !ep_reward)))
        return HE_EINVAL;
    VnArgs a = base_args(p, n, obs, reward, stats, scratch,
                         he_vecnorm_out{stats, returns, obs_out, reward_out, terminal_obs_out, ep_return, ep_length,
                                        ep_return_done, ep_length_done});
    a.done = done;
    a.tobs = terminal_obs;
    a.ep_reward = ep_reward;
    return launch(a, (hipStream_t)stream, moments);
}

he_status he_vecnorm_step(const he_vecnorm_params* p, int64_t n, const float* obs, const float* reward,
                          const uint8_t* done, const float* terminal_obs, double* returns, double* stats,
                          void* scratch, float* obs_out, float* reward_out, float* terminal_obs_out,
                          double* ep_return, int32_t* ep_length, double* ep_return_done, int32_t* ep_length_done,
                          const double* ep_reward, void* stream) {
    return vecnorm_step(p, n, obs, reward, done, terminal_obs, returns, stats, scratch, obs_out, reward_out,
                        terminal_obs_out, ep_return, ep_length, ep_return_done, ep_length_done, ep_reward, stream, true);
}

he_status he_vecnorm_apply(const he_vecnorm_params* p, int64_t n, const float* obs, const float* reward,
                           const uint8_t* done, const float* terminal_obs, double* returns, double* stats,
                           void* scratch, float* obs_out, float* reward_out, float* terminal_obs_out,
                           double* ep_return, int32_t* ep_length, double* ep_return_done, int32_t* ep_length_done,
                           const double* ep_reward, void* stream) {
    // training merges the fused partials, which cover <= 65,536 rows; frozen statistics read none
    if (p && p->training && n > (int64_t)kVnMaxBlocks * kVnThreads) return HE_EINVAL;
    // he_vecnorm_attach makes no partials in this mode: nothing to merge
    if (p && p->training && p->moments == HE_VN_MOMENTS_SB3) return HE_EINVAL;
    return vecnorm_step(p, n, obs, reward, done, terminal_obs, returns, stats, scratch, obs_out, reward_out,
                        terminal_obs_out, ep_return, ep_length, ep_return_done, ep_length_done, ep_reward, stream, false);
}

he_status he_vecnorm_reset(const he_vecnorm_params* p, int64_t n, const float* obs, double* returns, double* stats,
                           void* scratch, float* obs_out, void* stream) {
    if (!params_ok(p) || n < 0 || !count_ok(p, n)) return HE_EINVAL;
    if (n == 0) return HE_OK;
    if (!obs || !returns || !stats || !scratch || !obs_out) return HE_EINVAL;
    he_vecnorm_out out = {};
    out.stats = stats;
    out.returns = returns;
    out.obs_out = obs_out;
    VnArgs a = base_args(p, n, obs, nullptr, stats, scratch, out);
    return launch(a, (hipStream_t)stream);
}

he_status he_host_vecnorm_sb3(const he_vecnorm_params* p, int64_t n64, const float* obs, const float* reward,
                              const uint8_t* done, const float* terminal_obs, double* returns, double* stats,
                              float* obs_out, float* reward_out, float* terminal_obs_out) {
    if (!params_ok(p) || n64 < 0 || n64 > sb3::kMaxN) return HE_EINVAL;
    if (n64 == 0) return HE_OK;
    const bool reset = reward == nullptr;
    if (!obs || !returns || !stats || !obs_out || (!reset && !reward_out)) return HE_EINVAL;
    const int n = (int)n64;
    const bool training = p->training != 0, norm_obs = p->norm_obs != 0;
    if (training && norm_obs) {   // obs_rms.update(obs): one f32 chain per column, row order
        const double count0 = stats[2 * kD];
        for (int c = 0; c < kD; ++c) {
            const float bmean = sb3::col_sum(0.0f, true, obs + c, n) / (float)n;
            const float bvar = sb3::col_sq(0.0f, true, bmean, obs + c, n) / (float)n;
            double count = count0;
            sb3::rms_update(&stats[c], &stats[kD + c], &count, (double)bmean, sb3::batch_m2_obs(bvar, n), (double)n);
            stats[2 * kD] = count;
        }
    }
    if (training && !reset) {     // returns = returns * gamma + reward; ret_rms.update(returns)
        std::vector<double> buf(n);
        double nval[sb3::kNodes], bret[2];
        for (int r = 0; r < n; ++r) buf[r] = returns[r] = sb3::ret_update(returns[r], p->gamma, reward[r]);
        const int levels = sb3::pw_levels(n);
        for (int pass = 0; pass < 2; ++pass) {
            for (int id = 1; id < (2 << levels); ++id) {
                const sb3::Node nd = sb3::pw_node(n, id);
                if (nd.n > 0 && nd.n <= sb3::kLeafMax) nval[id] = sb3::pw_leaf(buf.data() + nd.lo, nd.n);
            }
            for (int d = levels - 1; d >= 0; --d)
                for (int id = 1 << d; id < (2 << d); ++id)
                    if (sb3::pw_node(n, id).n > sb3::kLeafMax) nval[id] = nval[2 * id] + nval[2 * id + 1];
            bret[pass] = nval[1] / (double)n;
            if (pass == 0)
                for (int r = 0; r < n; ++r) {
                    const double d = buf[r] - bret[0];
                    buf[r] = d * d;
                }
        }
        sb3::rms_update(&stats[2 * kD + 1], &stats[2 * kD + 2], &stats[2 * kD + 3], bret[0], bret[1] * (double)n,
                        (double)n);
    }
    double sd[kD];
    for (int c = 0; c < kD; ++c) sd[c] = sb3::norm_sd(stats[kD + c], p->epsilon);
    const double rsd = sb3::norm_sd(stats[2 * kD + 2], p->epsilon);
    for (int k = 0; k < n * kD; ++k)
        obs_out[k] = norm_obs ? sb3::norm_obs(obs[k], stats[k % kD], sd[k % kD], p->clip_obs) : obs[k];
    const vn::Sb3Norm nz{stats, sd, &rsd, p->clip_obs, p->clip_reward};
    he_vecnorm_out out = {};   // no Monitor
    out.stats = stats;
    out.returns = returns;
    out.obs_out = obs_out;
    out.reward_out = reward_out;
    out.terminal_obs_out = terminal_obs_out;
    const vn::ApplyArgs a = vn::apply_args(p, out);
    for (int r = 0; r < n; ++r) {
        if (reset)
            returns[r] = 0.0;
        else
            vn::row_tail(a, nz, terminal_obs, r, RowIn{reward[r], done && done[r], 0.0, 0.0, 0});
    }
    return HE_OK;
}

}  // extern "C"
