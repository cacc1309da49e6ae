// vn_apply.h -- the second half of a VecNormalize step (SB3 2.6.0 VecNormalize.step_wait after
// the statistics: normalize_obs, normalize_reward, the terminal obs of done rows,
// returns[dones] = 0) and Monitor's episode sums, written once for every site that runs it:
//   vn_apply_kernel, vn_sb3_kernel (vecnorm.hip)   the separate launches;
//   apply_frozen_rows (below)                      the eval step fused into he_step
//                                                  (hedge_env.hip step1_vne_kernel);
//   step_rows (vn_step.h)                          the whole step of <= 256 envs fused into
//                                                  he_step (hedge_env.hip step1_vnw_kernel);
//   he_host_vecnorm_sb3 (vecnorm.hip)              the host mirror, no Monitor.
// The pieces: the two normalisers (SplitNorm: moments = f64, the f32 split of the f64
// statistics; Sb3Norm: moments = sb3, SB3's own f64 arithmetic of vn_sb3.h), the flat coalesced
// obs pass (obs_pass), a row's tail (row_tail) and the argument block of the half (ApplyArgs,
// filled by apply_args).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hedge_env.h"
#include "vn_moments.h"
#include "vn_sb3.h"

namespace vn {

struct ColNorm {
    float mh, mls, sh, sl;   // mean = mh + ml, s = 1 / sqrt(var + eps) = sh + sl, mls = RN(ml s)
};
__device__ __forceinline__ ColNorm col_norm(double mean, double var, double eps) {
    const double s = 1.0 / sqrt(var + eps);
    const float mh = (float)mean, sh = (float)s;
    // s past FLT_MAX (var + eps = 0, e.g. epsilon = 0 on a constant column): the split terms
    // would be inf - inf and 0 * inf = NaN for every element; with them 0 an element is
    // (x - mh) * inf = +-inf -> +-clip, as the f64 (x - mean) / sqrt(var + eps) clips (0 / 0
    // stays NaN, as in SB3)
    if (!(sh <= 3.402823466e38f)) return ColNorm{mh, 0.0f, sh, 0.0f};
    return ColNorm{mh, (float)((mean - (double)mh) * s), sh, (float)(s - (double)sh)};
}
// VecNormalize.normalize_obs of one element in f32 from the merged f64 statistics, converted
// once per column (col_norm): y = (x - mh) (sh + sl) - ml s.  x - mh is exact within a factor
// 2 of the mean (Sterbenz), else one rounding; the two FMAs round once more (the sl and ml s
// terms are corrections far below y's last bit).  About 1 f32 ulp of y against the f64
// (x - mean) / sqrt(var + eps) -- the tests allow 2e-6 absolute at |y| <= clip = 10, ~2 ulp.
// np.clip in f32 (NaN stays NaN).
__device__ __forceinline__ float norm_elem(float x, const ColNorm& n, float clip) {
    const float d = x - n.mh;
    const float r = fmaf(d, n.sh, fmaf(d, n.sl, -n.mls));
    return r < -clip ? -clip : (r > clip ? clip : r);
}

// ------------------------------------------------------------------ the two normalisers
// A normaliser is where the per-column constants are (LDS on the device: read at the use, so
// they cost no registers in between) and the clips; obs(x, c) normalizes an element of obs
// column c, rew(r) a reward.  kTailUnroll: how far row_tail unrolls a terminal obs row (the
// f64 divisions of Sb3Norm stay rolled: the row is rare and, in the step kernel, registers are tight).
struct SplitNorm {
    static constexpr int kTailUnroll = kD;
    const ColNorm* cn;     // [kD] (col_norm)
    const double* rinv;    // 1 / sqrt(ret_var + eps)
    float clip_obs;
    double clip_rew;
    __device__ __forceinline__ float obs(float x, int c) const { return norm_elem(x, cn[c], clip_obs); }
    __device__ __forceinline__ float rew(float r) const {
        return (float)sb3::clipd((double)r * *rinv, -clip_rew, clip_rew);
    }
};
struct Sb3Norm {
    static constexpr int kTailUnroll = 1;
    const double* mean;    // [kD]
    const double* sd;      // [kD] sb3::norm_sd
    const double* rsd;     // sb3::norm_sd of the returns' variance
    double clip_obs, clip_rew;
    VN_SB3_HD float obs(float x, int c) const { return sb3::norm_obs(x, mean[c], sd[c], clip_obs); }
    VN_SB3_HD float rew(float r) const { return sb3::norm_rew(r, *rsd, clip_rew); }
};

// ------------------------------------------------------------------ the flat obs pass
// The obs of a workgroup's nf / kD rows as a flat coalesced pass: thread t takes the elements
// k = t + 256 q, which are column k % 13 (the rows start at a row boundary), stepped by
// 256 % 13 = 9 per trip without a division.  x(q, k) is the element -- trip q's register, or
// element k of an LDS tile or of global memory.  The trip structure is the caller's: kUnrolled
// is kD guarded trips (nf <= 256 kD; the elements can be registers), kStrided a loop over any
// nf, kept rolled (few registers: the f64 divisions of Sb3Norm, inside the step kernel too).
enum ObsTrips { kUnrolled, kStrided };
template <ObsTrips TRIPS, class Norm, class Elem>
__device__ __forceinline__ void obs_pass(float* dst, int nf, bool norm, const Norm& nz, Elem x) {
    const int t = threadIdx.x;
    int c = t % kD;
    const auto trip = [&](int q, int k) {
        if (k < nf) dst[k] = norm ? nz.obs(x(q, k), c) : x(q, k);
        c += kVnThreads % kD;
        c = c >= kD ? c - kD : c;
    };
    if (TRIPS == kUnrolled) {
#pragma unroll
        for (int q = 0; q < kD; ++q) trip(q, t + q * kVnThreads);
    } else {
#pragma unroll 1
        for (int k = t; k < nf; k += kVnThreads) trip(0, k);
    }
}

// ------------------------------------------------------------------ a row's tail
struct ApplyArgs {
    int32_t norm_obs, norm_reward;
    int32_t sb3;          // moments = HE_VN_MOMENTS_SB3: the f64 normalization of vn_sb3.h
    double clip_obs, clip_rew, eps;
    const double* stats;
    double* returns;
    float* obs_out;
    float* rew_out;
    float* tobs_out;
    double* ep_ret;       // Monitor sums (NULL: none)
    int32_t* ep_len;
    double* ep_ret_done;
    int32_t* ep_len_done;
};
// The half's arguments from the caller's parameters and output buffers (host).
inline ApplyArgs apply_args(const he_vecnorm_params* p, const he_vecnorm_out& o) {
    ApplyArgs a = {};
    a.norm_obs = p->norm_obs != 0;
    a.norm_reward = p->norm_reward != 0;
    a.sb3 = p->moments == HE_VN_MOMENTS_SB3;
    a.clip_obs = p->clip_obs;
    a.clip_rew = p->clip_reward;
    a.eps = p->epsilon;
    a.stats = o.stats;
    a.returns = o.returns;
    a.obs_out = o.obs_out;
    a.rew_out = o.reward_out;
    a.tobs_out = o.terminal_obs_out;
    a.ep_ret = o.ep_return;
    a.ep_len = o.ep_length;
    a.ep_ret_done = o.ep_return_done;
    a.ep_len_done = o.ep_length_done;
    return a;
}
// A row's inputs besides its obs: reward, done flag, Monitor running sums and the f64
// reward Monitor adds (Monitor wraps each env inside the VecEnv, train_ppo_v2.py:119, so it
// sums the env's own f64 reward, hedging_env_v2.py:262,294 -- not the f32 VecEnv buffer).
// Each site loads them where the loads cost it least and hands them over by value.
struct RowIn {
    float rw;
    bool dn;
    double er;
    double rw64;
    int32_t el;
};
// Row r after the statistics: the normalized reward, the normalized terminal obs of a done row
// (tobs / a.tobs_out may be NULL), returns[done] = 0 and Monitor's sums (a.ep_ret NULL: none).
template <class Norm>
VN_SB3_HD void row_tail(const ApplyArgs& a, const Norm& nz, const float* tobs, int64_t r, RowIn in) {
    a.rew_out[r] = a.norm_reward ? nz.rew(in.rw) : in.rw;
    if (in.dn && tobs && a.tobs_out) {   // rare: per-row accesses
#pragma unroll Norm::kTailUnroll
        for (int c = 0; c < kD; ++c) {
            const float x = tobs[r * kD + c];
            a.tobs_out[r * kD + c] = a.norm_obs ? nz.obs(x, c) : x;
        }
    }
    if (in.dn) a.returns[r] = 0.0;   // self.returns[dones] = 0
    if (a.ep_ret) {                  // Monitor: sum(rewards) of the env's f64 rewards, len(rewards)
        const double er = in.er + in.rw64;
        const int32_t el = in.el + 1;
        if (in.dn) {
            a.ep_ret_done[r] = er;
            a.ep_len_done[r] = el;
        }
        a.ep_ret[r] = in.dn ? 0.0 : er;
        a.ep_len[r] = in.dn ? 0 : el;
    }
}

// ------------------------------------------------------------------ eval: the whole step fused
// VecNormalize.step_wait with the statistics frozen (training=False, train_ppo_v2.py:450-453):
// no moments, so nothing crosses workgroups and he_step's own launch can finish the step
// (step1_vne_kernel, he_vecnorm_attach_eval) -- the obs rows normalized from the step's LDS
// staging tile, the reward from the thread's register (f32 for VecNormalize, the f64 one for
// Monitor), then the row's tail.  The same normalisers as vecnorm.hip's kernels: the same bits
// as he_step + he_vecnorm_apply.
// What a thread of the fused kernel loads before its step (off the epilogue's path): thread
// t < kD the statistics of obs column t, thread kD the returns' variance; its row's Monitor sums.
struct FrozenPre {
    double m, v, er;
    int32_t el;
};
__device__ __forceinline__ FrozenPre load_frozen(const ApplyArgs& a, int64_t r, bool live) {
    const int t = threadIdx.x;
    FrozenPre f{0.0, 1.0, 0.0, 0};
    if (t < kD) {
        f.m = a.stats[t];
        f.v = a.stats[kD + t];
    } else if (t == kD) {
        f.v = a.stats[2 * kD + 2];
    }
    if (a.ep_ret && live) {
        f.er = a.ep_ret[r];
        f.el = a.ep_len[r];
    }
    return f;
}
// The per-column constants in LDS, made before the step (their f64 square roots and divisions
// overlap the step's loads; the step's own barrier publishes them).
struct FrozenNorm {
    ColNorm cn[kD];
    double rinv;
    double m[kD], sd[kD], rsd;   // a.sb3: the columns' mean and sqrt(var + eps), the returns' sqrt(var + eps)
};
__device__ __forceinline__ void prep_frozen(FrozenNorm& z, const ApplyArgs& a, const FrozenPre& f) {
    const int t = threadIdx.x;
    if (a.sb3) {   // uniform
        if (t < kD) {
            z.m[t] = f.m;
            z.sd[t] = sb3::norm_sd(f.v, a.eps);
        }
        if (t == kD) z.rsd = sb3::norm_sd(f.v, a.eps);
        return;
    }
    if (t < kD) z.cn[t] = col_norm(f.m, f.v, a.eps);
    if (t == kD) z.rinv = 1.0 / sqrt(f.v + a.eps);
}
// rows [r0, r0 + rows) of the workgroup, obs staged at tile (row t at tile + t kD), after a
// workgroup barrier that follows prep_frozen; thread t < rows owns row r0 + t: its reward, done
// flag and terminal obs row.  This sits inside the step kernel, where registers are tight: the
// f64 divisions of Sb3Norm take the rolled pass, everything else (a copy included) the unrolled one.
__device__ __forceinline__ void apply_frozen_rows(const ApplyArgs& a, const FrozenNorm& z, int64_t r0, int rows,
                                                  const float* tile, const FrozenPre& f, float rew, double rew64,
                                                  bool done, const float* tobs) {
    const SplitNorm split{z.cn, &z.rinv, (float)a.clip_obs, a.clip_rew};
    const Sb3Norm sb{z.m, z.sd, &z.rsd, a.clip_obs, a.clip_rew};
    const int t = threadIdx.x;
    float* dst = a.obs_out + r0 * kD;
    const auto elem = [tile](int, int k) { return tile[k]; };
    if (a.sb3 && a.norm_obs)   // uniform
        obs_pass<kStrided>(dst, rows * kD, true, sb, elem);
    else
        obs_pass<kUnrolled>(dst, rows * kD, a.norm_obs != 0, split, elem);
    if (t >= rows) return;
    const RowIn in{rew, done, f.er, rew64, f.el};
    if (a.sb3)
        row_tail(a, sb, tobs, r0 + t, in);
    else
        row_tail(a, split, tobs, r0 + t, in);
}

}  // namespace vn
