// hedge_actor.hip -- libhedgeactor (include/hedge_actor.h): the RecurrentPPO actor of an SB3
// checkpoint as one gfx950 kernel, the closed-loop evaluation's episode sums, and the host
// build of the same arithmetic (ha_math.h).
//
// Kernel layout (actor_kernel): a workgroup of 4 waves owns a tile of 32 envs.
//   stage   [x | h | 0] of the tile goes to LDS as xh[k][env] (x normalised on the way, h zeroed
//           where episode_start is set): the B operand of v_mfma_f32_32x32x2_f32, lane l reading
//           xh[2 s + (l >> 5)][l & 31] at k-step s.
//   gates   wave w owns hidden units 32 w .. 32 w + 31 and keeps FOUR accumulators, the gates i,
//           f, g, o of those units: D[unit][env], so a lane holds the four pre-activations of the
//           same (unit, env) pairs in the same registers and the cell update needs no exchange.
//           The A operand is packed at ha_create as float4 {i, f, g, o}[w][s][lane]: one 16-byte
//           load per lane per k-step feeds the four MFMAs (independent accumulators: the 64-cycle
//           dependent latency is covered).  The whole K = 142 runs through one accumulator per
//           gate, starting from b_ih + b_hh, so each pre-activation is the k-ordered fmaf chain of
//           the contract.
//   cell    in registers; c read and c', h' written as float4 (four consecutive units per lane
//           and register group), h' also to LDS as the next B operand.
//   MLP     waves 0, 1 each own 32 of the 64 outputs of a layer (one accumulator, K = 128 then
//           64), activations through LDS; the 2 x 64 action head is a VALU fmaf chain.
// 512 x 142 x 4 B of packed gate weights are read per tile from L2.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/hedge_actor.h"
#include "ha_math.h"

using namespace ha;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;                 // envs per workgroup
constexpr int kThreads = 256;             // 4 waves: one per 32 hidden units
constexpr int kStepsG = kKp / 2;          // 71 k-steps of the gate product
constexpr int kLd = kTile + 1;            // LDS row stride (floats): staging writes run down a column

struct Params {
    int64_t n;
    const float* obs;
    const uint8_t* start;
    float* h;
    float* c;
    float* actions;
    float* mean_out;
    float* obs_norm_out;
    const float4* wg;     // [4][71][64] {i, f, g, o}
    const float* bg;      // [512] b_ih + b_hh
    const float* w1p;     // [2][64][64]
    const float* b1;
    const float* w2p;     // [2][32][64]
    const float* b2;
    const float* w3;      // [2][64]
    const float* b3;
    const double* stats;  // [3][13] mean, sd, RN(1 / sd); NULL = no normalisation
    double clip;
    int32_t has_clip, relu, tanh_squash;
};

// C/D row of accumulator register r in lane-half hi (32x32 tile): (r & 3) + 8 (r >> 2) + 4 hi

// one 32-output slice of a Linear layer for the tile: acc = bias, K / 2 k-steps, the activation,
// the result to out[row][env]
template <int K>
__device__ __forceinline__ void mlp_slice(const float* __restrict__ wp, const float* __restrict__ bias,
                                          const float (*in)[kLd], float (*out)[kLd], int rt, int lane, bool relu) {
    const int col = lane & 31, hi = lane >> 5;
    f32x16 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 b = *(const float4*)(bias + rt * 32 + 8 * q + 4 * hi);
        a[4 * q + 0] = b.x; a[4 * q + 1] = b.y; a[4 * q + 2] = b.z; a[4 * q + 3] = b.w;
    }
    const float* w = wp + (size_t)rt * (K / 2) * 64 + lane;
#pragma unroll 8
    for (int s = 0; s < K / 2; ++s) a = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s * 64], in[2 * s + hi][col], a, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi][col] = mlp_act(a[r], relu);
}

__global__ __launch_bounds__(kThreads, 2) void actor_kernel(const Params p) {
    __shared__ float xh[kKp][kLd];
    __shared__ float hn[kHid][kLd];
    __shared__ float a1[kMlp][kLd];
    __shared__ float a2[kMlp][kLd];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kTile;

    // ---- stage [x | h | 0]; envs past n are zero columns
    for (int idx = tid; idx < kTile * kObs; idx += kThreads) {
        const int el = idx / kObs, k = idx - el * kObs;
        const int64_t e = e0 + el;
        float v = 0.0f;
        if (e < p.n) {
            v = p.obs[e * kObs + k];
            if (p.stats) v = norm_obs(v, p.stats[k], p.stats[kObs + k], p.stats[2 * kObs + k], p.has_clip != 0, p.clip);
            if (p.obs_norm_out) p.obs_norm_out[e * kObs + k] = v;
        }
        xh[k][el] = v;
    }
    for (int idx = tid; idx < kTile * kHid; idx += kThreads) {
        const int el = idx >> 7, u = idx & (kHid - 1);
        const int64_t e = e0 + el;
        float v = 0.0f;
        if (e < p.n && !p.start[e]) v = p.h[e * kHid + u];
        xh[kObs + u][el] = v;
    }
    if (tid < kTile) xh[kKx][tid] = 0.0f;
    __syncthreads();

    // ---- gates: wave = unit group, four accumulators
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    {
        f32x16 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *(const float4*)(p.bg + g * kHid + wave * 32 + 8 * q + 4 * hi);
                acc[g][4 * q + 0] = b.x; acc[g][4 * q + 1] = b.y; acc[g][4 * q + 2] = b.z; acc[g][4 * q + 3] = b.w;
            }
        const float4* wp = p.wg + (size_t)wave * kStepsG * 64 + lane;
#pragma unroll 4
        for (int s = 0; s < kStepsG; ++s) {
            const float4 w = wp[s * 64];
            const float b = xh[2 * s + hi][col];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, b, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, b, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, b, acc[3], 0, 0, 0);
        }
        // ---- cell update in registers
        const int64_t e = e0 + col;
        const bool valid = e < p.n;
        const bool fresh = valid && p.start[e] != 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = wave * 32 + 8 * q + 4 * hi;
            float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (valid && !fresh) cv = *(const float4*)(p.c + e * kHid + u);
            float cc[4] = {cv.x, cv.y, cv.z, cv.w};
            float hv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * q + j;
                hv[j] = cell_update(acc[0][r], acc[1][r], acc[2][r], acc[3][r], &cc[j]);
                hn[u + j][col] = hv[j];
            }
            if (valid) {
                *(float4*)(p.c + e * kHid + u) = make_float4(cc[0], cc[1], cc[2], cc[3]);
                *(float4*)(p.h + e * kHid + u) = make_float4(hv[0], hv[1], hv[2], hv[3]);
            }
        }
    }
    __syncthreads();

    // ---- MLP and the action head
    if (wave < 2) mlp_slice<kHid>(p.w1p, p.b1, hn, a1, wave, lane, p.relu != 0);
    __syncthreads();
    if (wave < 2) mlp_slice<kMlp>(p.w2p, p.b2, a1, a2, wave, lane, p.relu != 0);
    __syncthreads();
    if (tid < kTile * kAct) {
        const int el = tid >> 1, j = tid & 1;
        const int64_t e = e0 + el;
        float m = p.b3[j];
        for (int k = 0; k < kMlp; ++k) m = fmaf(p.w3[j * kMlp + k], a2[k][el], m);
        if (e < p.n) {
            if (p.mean_out) p.mean_out[e * kAct + j] = m;
            p.actions[e * kAct + j] = squash_action(m, p.tanh_squash != 0);
        }
    }
}

struct AccIn {
    const double* col[7];
};

__global__ __launch_bounds__(256) void accumulate_kernel(int64_t n, int64_t goff, AccIn in, const uint8_t* term,
                                                         ha_episode_sums* sums, he_episode_record* rec, int64_t cap,
                                                         unsigned long long* count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    ha_episode_sums s = sums[e];
    s.s[0] = s.s[0] + in.col[0][e];
    s.s[1] = s.s[1] + in.col[1][e];
    s.s[2] = s.s[2] + in.col[2][e];
    s.s[3] = s.s[3] + in.col[3][e];
    s.s[4] = s.s[4] + in.col[4][e];
    s.s[5] = s.s[5] + in.col[5][e];
    s.s[6] = s.s[6] + in.col[6][e];
    s.length += 1;
    if (term[e]) {
        const unsigned long long r = atomicAdd(count, 1ull);
        if ((int64_t)r < cap) {
            he_episode_record o;
            o.env_id = goff + e;
            o.length = (int32_t)s.length;
            o.reserved = 0;
            o.reward_sum = s.s[0];
            o.pnl_sum = s.s[1];
            o.abs_pnl_sum = s.s[2];
            o.cost_sum = s.s[3];
            o.pnl_penalty_sum = s.s[4];
            o.cost_penalty_sum = s.s[5];
            o.per_share_pnl_sum = s.s[6];
            o.reserved2 = 0.0;
            rec[r] = o;
        }
        s.s[0] = s.s[1] = s.s[2] = s.s[3] = s.s[4] = s.s[5] = s.s[6] = 0.0;
        s.length = 0;
    }
    sums[e] = s;
}

thread_local char g_err[256] = "";

}  // namespace

struct ha_actor {
    char err[256];
    void* blob;   // one device allocation holding every packed tensor
    Params p;     // the constant part of the kernel's arguments
};

namespace {

ha_status fail(ha_actor* a, ha_status st, const char* msg) {
    snprintf(a ? a->err : g_err, 256, "%s", msg);
    return st;
}

ha_status check_weights(const ha_weights* w, ha_actor* a) {
    if (!w) return fail(a, HE_EINVAL, "weights is NULL");
    if (w->abi_version != HA_ABI_VERSION) return fail(a, HE_EINVAL, "ha_weights.abi_version mismatch");
    char m[200];
    if (w->n_lstm_layers != 1) {
        snprintf(m, sizeof m, "n_lstm_layers = %d: this actor has one LSTM layer", w->n_lstm_layers);
        return fail(a, HE_ESHAPE, m);
    }
    if (w->obs_dim != kObs || w->hidden != kHid || w->mlp_width != kMlp || w->act_dim != kAct) {
        snprintf(m, sizeof m, "actor shape obs %d / lstm %d / mlp %d / action %d: only 13 / 128 / 64 / 2 is built",
                 w->obs_dim, w->hidden, w->mlp_width, w->act_dim);
        return fail(a, HE_ESHAPE, m);
    }
    if (w->activation != HA_ACT_TANH && w->activation != HA_ACT_RELU) return fail(a, HE_EINVAL, "unknown activation");
    if (w->squash != HA_SQUASH_CLIP && w->squash != HA_SQUASH_TANH) return fail(a, HE_EINVAL, "unknown squash");
    if (!w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->w1 || !w->b1 || !w->w2 || !w->b2 || !w->w3 || !w->b3)
        return fail(a, HE_EINVAL, "an actor tensor is NULL");
    if ((w->obs_mean == nullptr) != (w->obs_var == nullptr))
        return fail(a, HE_EINVAL, "obs_mean and obs_var come together");
    return HE_OK;
}

// W[j][k] of the gate product over [x | h | 0]
inline float gate_w(const ha_weights* w, int j, int k) {
    return k < kObs ? w->w_ih[j * kObs + k] : (k < kKx ? w->w_hh[j * kHid + (k - kObs)] : 0.0f);
}

}  // namespace

extern "C" {

const char* ha_version(void) { return "libhedgeactor 1 (gfx950, v_mfma_f32_32x32x2_f32)"; }

const char* ha_last_error(const ha_actor* actor) { return actor ? actor->err : g_err; }

ha_status ha_create(const ha_weights* w, ha_actor** out) {
    if (!out) return fail(nullptr, HE_EINVAL, "out is NULL");
    *out = nullptr;
    ha_status st = check_weights(w, nullptr);
    if (st != HE_OK) return st;
    // the blob: float4-aligned sections, in floats
    const size_t o_wg = 0, n_wg = (size_t)4 * kStepsG * 64 * 4;
    const size_t o_bg = o_wg + n_wg, o_w1 = o_bg + kGates, o_b1 = o_w1 + (size_t)kMlp * kHid;
    const size_t o_w2 = o_b1 + kMlp, o_b2 = o_w2 + (size_t)kMlp * kMlp, o_w3 = o_b2 + kMlp;
    const size_t o_b3 = o_w3 + kAct * kMlp, o_st = o_b3 + 4;   // stats: doubles, 8-byte aligned (o_st even)
    const size_t total = o_st + 2 * 3 * kObs;
    std::vector<float> hbuf(total, 0.0f);
    for (int ug = 0; ug < 4; ++ug)
        for (int s = 0; s < kStepsG; ++s)
            for (int l = 0; l < 64; ++l)
                for (int g = 0; g < 4; ++g)
                    hbuf[o_wg + (((size_t)ug * kStepsG + s) * 64 + l) * 4 + g] =
                        gate_w(w, g * kHid + ug * 32 + (l & 31), 2 * s + (l >> 5));
    for (int j = 0; j < kGates; ++j) hbuf[o_bg + j] = w->b_ih[j] + w->b_hh[j];
    for (int rt = 0; rt < 2; ++rt)
        for (int l = 0; l < 64; ++l) {
            for (int s = 0; s < kHid / 2; ++s)
                hbuf[o_w1 + ((size_t)rt * (kHid / 2) + s) * 64 + l] = w->w1[(rt * 32 + (l & 31)) * kHid + 2 * s + (l >> 5)];
            for (int s = 0; s < kMlp / 2; ++s)
                hbuf[o_w2 + ((size_t)rt * (kMlp / 2) + s) * 64 + l] = w->w2[(rt * 32 + (l & 31)) * kMlp + 2 * s + (l >> 5)];
        }
    memcpy(&hbuf[o_b1], w->b1, kMlp * sizeof(float));
    memcpy(&hbuf[o_b2], w->b2, kMlp * sizeof(float));
    memcpy(&hbuf[o_w3], w->w3, kAct * kMlp * sizeof(float));
    memcpy(&hbuf[o_b3], w->b3, kAct * sizeof(float));
    if (w->obs_mean) {
        double stt[3 * kObs];
        for (int k = 0; k < kObs; ++k) {
            stt[k] = w->obs_mean[k];
            stt[kObs + k] = sqrt(w->obs_var[k] + w->epsilon);
            stt[2 * kObs + k] = 1.0 / stt[kObs + k];
        }
        memcpy(&hbuf[o_st], stt, sizeof stt);
    }
    ha_actor* a = new (std::nothrow) ha_actor();
    if (!a) return fail(nullptr, HE_ENOMEM, "host allocation failed");
    a->err[0] = 0;
    a->blob = nullptr;
    if (hipMalloc(&a->blob, total * sizeof(float)) != hipSuccess) {
        delete a;
        (void)hipGetLastError();
        return fail(nullptr, HE_ENOMEM, "hipMalloc of the packed weights failed (no HIP device?)");
    }
    if (hipMemcpy(a->blob, hbuf.data(), total * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(a->blob);
        delete a;
        return fail(nullptr, HE_EHIP, "upload of the packed weights failed");
    }
    const float* d = (const float*)a->blob;
    Params& p = a->p;
    memset(&p, 0, sizeof p);
    p.wg = (const float4*)(d + o_wg);
    p.bg = d + o_bg;
    p.w1p = d + o_w1;
    p.b1 = d + o_b1;
    p.w2p = d + o_w2;
    p.b2 = d + o_b2;
    p.w3 = d + o_w3;
    p.b3 = d + o_b3;
    p.stats = w->obs_mean ? (const double*)(d + o_st) : nullptr;
    p.clip = w->clip_obs;
    p.has_clip = w->has_clip;
    p.relu = w->activation == HA_ACT_RELU;
    p.tanh_squash = w->squash == HA_SQUASH_TANH;
    *out = a;
    return HE_OK;
}

ha_status ha_destroy(ha_actor* actor) {
    if (!actor) return HE_EINVAL;
    if (actor->blob) (void)hipFree(actor->blob);
    delete actor;
    return HE_OK;
}

ha_status ha_step(ha_actor* actor, int64_t n, const float* obs, const uint8_t* episode_start, float* h, float* c,
                  float* actions, float* mean_out, float* obs_norm_out, void* stream) {
    if (!actor) return HE_EINVAL;
    if (n < 1 || n > ((int64_t)1 << 30)) return fail(actor, HE_EINVAL, "n must be in [1, 2^30]");
    if (!obs || !episode_start || !h || !c || !actions) return fail(actor, HE_EINVAL, "a required buffer is NULL");
    if ((((uintptr_t)h) | ((uintptr_t)c)) & 15u) return fail(actor, HE_EINVAL, "h and c must be 16-byte aligned");
    Params p = actor->p;
    p.n = n;
    p.obs = obs;
    p.start = episode_start;
    p.h = h;
    p.c = c;
    p.actions = actions;
    p.mean_out = mean_out;
    p.obs_norm_out = obs_norm_out;
    const unsigned grid = (unsigned)((n + kTile - 1) / kTile);
    hipLaunchKernelGGL(actor_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return fail(actor, HE_EHIP, "actor_kernel launch failed");
    return HE_OK;
}

ha_status ha_accumulate(ha_actor* actor, int64_t n, int64_t env_id_offset, const double* reward_step,
                        const double* step_pnl_total, const double* raw_pnl_deviation_abs,
                        const double* transaction_costs_total, const double* reward_pnl_component,
                        const double* transaction_cost_penalty, const double* per_share_step_pnl,
                        const uint8_t* terminated, ha_episode_sums* sums, he_episode_record* records,
                        int64_t capacity, unsigned long long* count, void* stream) {
    if (!actor) return HE_EINVAL;
    if (n < 1) return fail(actor, HE_EINVAL, "n must be >= 1");
    AccIn in = {{reward_step, step_pnl_total, raw_pnl_deviation_abs, transaction_costs_total, reward_pnl_component,
                 transaction_cost_penalty, per_share_step_pnl}};
    for (int k = 0; k < 7; ++k)
        if (!in.col[k]) return fail(actor, HE_EINVAL, "an info column is NULL");
    if (!terminated || !sums || !count) return fail(actor, HE_EINVAL, "terminated, sums and count are required");
    if (capacity < 0 || (capacity > 0 && !records)) return fail(actor, HE_EINVAL, "records is NULL with capacity > 0");
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(accumulate_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, env_id_offset, in, terminated,
                       sums, records, capacity, count);
    if (hipGetLastError() != hipSuccess) return fail(actor, HE_EHIP, "accumulate_kernel launch failed");
    return HE_OK;
}

ha_status ha_host_step(const ha_weights* w, int64_t n, const float* obs, const uint8_t* episode_start, float* h,
                       float* c, float* actions, float* mean_out, float* obs_norm_out) {
    ha_status st = check_weights(w, nullptr);
    if (st != HE_OK) return st;
    if (n < 1 || !obs || !episode_start || !h || !c || !actions) return fail(nullptr, HE_EINVAL, "bad argument");
    double sd[kObs], y[kObs];
    if (w->obs_mean)
        for (int k = 0; k < kObs; ++k) {
            sd[k] = sqrt(w->obs_var[k] + w->epsilon);
            y[k] = 1.0 / sd[k];
        }
    const bool relu = w->activation == HA_ACT_RELU, tsq = w->squash == HA_SQUASH_TANH;
    for (int64_t e = 0; e < n; ++e) {
        float xh[kKp], hn[kHid], a1[kMlp], a2[kMlp];
        for (int k = 0; k < kObs; ++k) {
            float v = obs[e * kObs + k];
            if (w->obs_mean) v = norm_obs(v, w->obs_mean[k], sd[k], y[k], w->has_clip != 0, w->clip_obs);
            if (obs_norm_out) obs_norm_out[e * kObs + k] = v;
            xh[k] = v;
        }
        const bool fresh = episode_start[e] != 0;
        for (int u = 0; u < kHid; ++u) xh[kObs + u] = fresh ? 0.0f : h[e * kHid + u];
        xh[kKx] = 0.0f;
        for (int u = 0; u < kHid; ++u) {
            float pre[4];
            for (int g = 0; g < 4; ++g) {
                const int j = g * kHid + u;
                float acc = w->b_ih[j] + w->b_hh[j];
                for (int k = 0; k < kKp; ++k) acc = fmaf(gate_w(w, j, k), xh[k], acc);
                pre[g] = acc;
            }
            float cv = fresh ? 0.0f : c[e * kHid + u];
            hn[u] = cell_update(pre[0], pre[1], pre[2], pre[3], &cv);
            c[e * kHid + u] = cv;
        }
        for (int u = 0; u < kHid; ++u) h[e * kHid + u] = hn[u];
        for (int j = 0; j < kMlp; ++j) {
            float acc = w->b1[j];
            for (int k = 0; k < kHid; ++k) acc = fmaf(w->w1[j * kHid + k], hn[k], acc);
            a1[j] = mlp_act(acc, relu);
        }
        for (int j = 0; j < kMlp; ++j) {
            float acc = w->b2[j];
            for (int k = 0; k < kMlp; ++k) acc = fmaf(w->w2[j * kMlp + k], a1[k], acc);
            a2[j] = mlp_act(acc, relu);
        }
        for (int j = 0; j < kAct; ++j) {
            float m = w->b3[j];
            for (int k = 0; k < kMlp; ++k) m = fmaf(w->w3[j * kMlp + k], a2[k], m);
            if (mean_out) mean_out[e * kAct + j] = m;
            actions[e * kAct + j] = squash_action(m, tsq);
        }
    }
    return HE_OK;
}

}  // extern "C"
