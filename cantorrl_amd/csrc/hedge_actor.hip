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
//
// policy_step_kernel (ha_policy_step) is the same tile body (net_tile) over a grid of (tiles, 2):
// blockIdx.y = 0 runs the actor's packed tensors on h_pi / c_pi and ends in the sampling and the
// log-probability, blockIdx.y = 1 runs the critic's on h_vf / c_vf and ends in the value.  Both
// stage the same obs; registers and LDS stay at actor_kernel's figures.  gae_kernel (ha_gae) is
// one thread per env over [K][n] arrays.  lstm_seq_fwd_kernel / lstm_seq_bwd_kernel (the PPO update's
// LSTM over a stored sequence, forward and backward) and lstm_wgrad_kernel / lstm_wgrad_reduce_kernel
// (its weight gradients), policy_pack_kernel (ha_policy_refresh), opt_norm_kernel / opt_adam_kernel
// (ha_adam_step), the four loss_*_kernel (ha_ppo_loss) and the four heads_*_kernel (ha_ppo_heads_forward /
// _backward) are described where they stand.
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

// one network (LSTM + two Linear + head) packed in the kernel's fragment order
struct Net {
    const float4* wg;     // [4][71][64] {i, f, g, o}
    const float* bg;      // [512] b_ih + b_hh
    const float* w1p;     // [2][64][64]
    const float* b1;
    const float* w2p;     // [2][32][64]
    const float* b2;
    const float* w3;      // [2][64] (the critic: [1][64])
    const float* b3;
};

struct Params {
    int64_t n;
    const float* obs;
    const uint8_t* start;
    float* h;
    float* c;
    float* actions;
    float* mean_out;
    float* obs_norm_out;
    Net net;
    const double* stats;  // [3][13] mean, sd, RN(1 / sd); NULL = no normalisation
    double clip;
    int32_t has_clip, relu, tanh_squash;
};

struct PolicyParams {
    int64_t n, goff;
    uint64_t seed, step_index;
    const float* obs;
    const uint8_t* start;
    float* h_pi;
    float* c_pi;
    float* h_vf;
    float* c_vf;
    float* actions;
    float* env_actions;
    float* values;
    float* log_probs;
    float* mean_out;
    float* obs_norm_out;
    Net pi, vf;
    const float* ls;      // [4] log_std[2], std[2]
    const double* stats;
    double clip;
    int32_t has_clip, relu, deterministic, write_state;
};

// the tile's LDS: 52,536 B
struct Tile {
    float xh[kKp][kLd];
    float hn[kHid][kLd];
    float a1[kMlp][kLd];
    float a2[kMlp][kLd];
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

// The tile body: stage, gates, cell update (h, c stored when write_state), the two MLP layers.
// On return (after a barrier) t.a2[k][env] holds the last hidden layer of the tile's envs.
__device__ __forceinline__ void net_tile(Tile& t, const Net& net, int64_t n, int64_t e0, const float* __restrict__ obs,
                                         const uint8_t* __restrict__ start, float* h, float* c, bool write_state,
                                         float* obs_norm_out, const double* __restrict__ stats, bool has_clip,
                                         double clip, bool relu) {
    const int tid = threadIdx.x;
    // ---- stage [x | h | 0]; envs past n are zero columns
    for (int idx = tid; idx < kTile * kObs; idx += kThreads) {
        const int el = idx / kObs, k = idx - el * kObs;
        const int64_t e = e0 + el;
        float v = 0.0f;
        if (e < n) {
            v = obs[e * kObs + k];
            if (stats) v = norm_obs(v, stats[k], stats[kObs + k], stats[2 * kObs + k], has_clip, clip);
            if (obs_norm_out) obs_norm_out[e * kObs + k] = v;
        }
        t.xh[k][el] = v;
    }
    for (int idx = tid; idx < kTile * kHid; idx += kThreads) {
        const int el = idx >> 7, u = idx & (kHid - 1);
        const int64_t e = e0 + el;
        float v = 0.0f;
        if (e < n && !start[e]) v = h[e * kHid + u];
        t.xh[kObs + u][el] = v;
    }
    if (tid < kTile) t.xh[kKx][tid] = 0.0f;
    __syncthreads();

    // ---- gates: wave = unit group, four accumulators (lstm_seq_fwd_kernel's copy of this product: see there)
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    {
        f32x16 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *(const float4*)(net.bg + g * kHid + wave * 32 + 8 * q + 4 * hi);
                acc[g][4 * q + 0] = b.x; acc[g][4 * q + 1] = b.y; acc[g][4 * q + 2] = b.z; acc[g][4 * q + 3] = b.w;
            }
        const float4* wp = net.wg + (size_t)wave * kStepsG * 64 + lane;
#pragma unroll 4
        for (int s = 0; s < kStepsG; ++s) {
            const float4 w = wp[s * 64];
            const float b = t.xh[2 * s + hi][col];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, b, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, b, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, b, acc[3], 0, 0, 0);
        }
        // ---- cell update in registers
        const int64_t e = e0 + col;
        const bool valid = e < n;
        const bool fresh = valid && start[e] != 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = wave * 32 + 8 * q + 4 * hi;
            float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (valid && !fresh) cv = *(const float4*)(c + e * kHid + u);
            float cc[4] = {cv.x, cv.y, cv.z, cv.w};
            float hv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * q + j;
                hv[j] = cell_update(acc[0][r], acc[1][r], acc[2][r], acc[3][r], &cc[j]);
                t.hn[u + j][col] = hv[j];
            }
            if (valid && write_state) {
                *(float4*)(c + e * kHid + u) = make_float4(cc[0], cc[1], cc[2], cc[3]);
                *(float4*)(h + e * kHid + u) = make_float4(hv[0], hv[1], hv[2], hv[3]);
            }
        }
    }
    __syncthreads();

    // ---- MLP
    if (wave < 2) mlp_slice<kHid>(net.w1p, net.b1, t.hn, t.a1, wave, lane, relu);
    __syncthreads();
    if (wave < 2) mlp_slice<kMlp>(net.w2p, net.b2, t.a1, t.a2, wave, lane, relu);
    __syncthreads();
}

// one output of the head for env column el: chain(b; w a2)
__device__ __forceinline__ float head_chain(const float* __restrict__ w, float b, const float (*a2)[kLd], int el) {
    float m = b;
    for (int k = 0; k < kMlp; ++k) m = fmaf(w[k], a2[k][el], m);
    return m;
}

__global__ __launch_bounds__(kThreads, 2) void actor_kernel(const Params p) {
    __shared__ Tile t;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kTile;
    net_tile(t, p.net, p.n, e0, p.obs, p.start, p.h, p.c, true, p.obs_norm_out, p.stats, p.has_clip != 0, p.clip,
             p.relu != 0);
    if (tid < kTile * kAct) {
        const int el = tid >> 1, j = tid & 1;
        const int64_t e = e0 + el;
        const float m = head_chain(p.net.w3 + j * kMlp, p.net.b3[j], t.a2, el);
        if (e < p.n) {
            if (p.mean_out) p.mean_out[e * kAct + j] = m;
            p.actions[e * kAct + j] = squash_action(m, p.tanh_squash != 0);
        }
    }
}

// grid (tiles, 2): y = 0 the actor and the sampling, y = 1 the critic and the value
__global__ __launch_bounds__(kThreads, 2) void policy_step_kernel(const PolicyParams p) {
    __shared__ Tile t;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kTile;
    const bool critic = blockIdx.y != 0;
    const Net net = critic ? p.vf : p.pi;
    net_tile(t, net, p.n, e0, p.obs, p.start, critic ? p.h_vf : p.h_pi, critic ? p.c_vf : p.c_pi, p.write_state != 0,
             critic ? nullptr : p.obs_norm_out, p.stats, p.has_clip != 0, p.clip, p.relu != 0);
    if (tid >= kTile * kAct) return;   // wave 0: lane pair (2 el, 2 el + 1) = the two head outputs of env el
    const int el = tid >> 1, j = tid & 1;
    const int64_t e = e0 + el;
    if (critic) {
        if (j == 0) {
            const float v = head_chain(net.w3, net.b3[0], t.a2, el);
            if (e < p.n) p.values[e] = v;
        }
        return;
    }
    const float m = head_chain(net.w3 + j * kMlp, net.b3[j], t.a2, el);
    const float mo = __shfl_xor(m, 1);
    const float mean[kAct] = {j ? mo : m, j ? m : mo};
    if (j != 0 || e >= p.n) return;
    float a[kAct], ea[kAct], lp;
    sample_action(mean, p.ls, p.ls + kAct, p.seed, p.step_index, (uint64_t)(p.goff + e), p.deterministic != 0, a, ea,
                  &lp);
    *(float2*)(p.actions + e * kAct) = make_float2(a[0], a[1]);
    *(float2*)(p.env_actions + e * kAct) = make_float2(ea[0], ea[1]);
    p.log_probs[e] = lp;
    if (p.mean_out) *(float2*)(p.mean_out + e * kAct) = make_float2(mean[0], mean[1]);
}

__global__ __launch_bounds__(256) void gae_kernel(int64_t n, int64_t K, float g32, float gl32,
                                                  const float* __restrict__ rewards, const float* __restrict__ values,
                                                  const uint8_t* __restrict__ episode_starts,
                                                  const float* __restrict__ last_values,
                                                  const uint8_t* __restrict__ last_dones, float* __restrict__ advantages,
                                                  float* __restrict__ returns) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) gae_env(e, n, K, g32, gl32, rewards, values, episode_starts, last_values, last_dones, advantages, returns);
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

struct ha_policy {
    char err[256];
    void* blob;       // both packed networks, log_std / std, the statistics, then the tensors of the last refresh
    PolicyParams p;
    bool refreshed;   // ha_policy_refresh has run since the last create / update: the blob's tail is current
};

namespace {

ha_status fail_to(char* err, ha_status st, const char* msg) {
    snprintf(err ? err : g_err, 256, "%s", msg);
    return st;
}
template <class H>   // ha_actor or ha_policy; NULL: the thread's message
ha_status fail(H* a, ha_status st, const char* msg) { return fail_to(a ? a->err : nullptr, st, msg); }

// one kernel launch on `stream`: HE_OK, or HE_EHIP with "<name> launch failed" in err (NULL: the thread's)
template <class K, class... A>
ha_status launch(char* err, K kernel, dim3 grid, dim3 block, void* stream, const char* name, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, args...);
    if (hipGetLastError() == hipSuccess) return HE_OK;
    char m[96];
    snprintf(m, sizeof m, "%s launch failed", name);
    return fail_to(err, HE_EHIP, m);
}

// The packed tensors to the device: into *blob, allocated first where it is NULL (and freed again
// when the copy fails: the caller drops its handle).  Messages go to err (NULL: the thread's).
ha_status upload_blob(const std::vector<float>& hbuf, void** blob, char* err) {
    const size_t bytes = hbuf.size() * sizeof(float);
    const bool fresh = !*blob;
    if (fresh && hipMalloc(blob, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail_to(err, HE_ENOMEM, "hipMalloc of the packed weights failed (no HIP device?)");
    }
    if (hipMemcpy(*blob, hbuf.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        if (fresh) (void)hipFree(*blob);
        return fail_to(err, HE_EHIP, "upload of the packed weights failed");
    }
    return HE_OK;
}

// a new ha_actor / ha_policy around the uploaded blob; its p is the caller's to fill
template <class H>
ha_status create_handle(const std::vector<float>& hbuf, H** out) {
    H* a = new (std::nothrow) H();   // value-initialised: no message, no blob
    if (!a) return fail_to(nullptr, HE_ENOMEM, "host allocation failed");
    const ha_status st = upload_blob(hbuf, &a->blob, nullptr);
    if (st != HE_OK) delete a;
    else *out = a;
    return st;
}

// one network's HOST tensors, torch layout; w3 is [n_out][64]
struct HostNet {
    const float *w_ih, *w_hh, *b_ih, *b_hh, *w1, *b1, *w2, *b2, *w3, *b3;
    int n_out;
    bool complete() const { return w_ih && w_hh && b_ih && b_hh && w1 && b1 && w2 && b2 && w3 && b3; }
};

template <class W>   // ha_weights or ha_policy_weights
HostNet actor_net(const W* w) {
    return {w->w_ih, w->w_hh, w->b_ih, w->b_hh, w->w1, w->b1, w->w2, w->b2, w->w3, w->b3, kAct};
}
HostNet critic_net(const ha_policy_weights* w) {
    return {w->c_w_ih, w->c_w_hh, w->c_b_ih, w->c_b_hh, w->v1, w->vb1, w->v2, w->vb2, w->v3, w->vb3, 1};
}

// The header fields ha_weights and ha_policy_weights share: n_lstm_layers, the four dimensions,
// activation and the mean / var pairing.  layers, what, built: the words their messages differ in;
// rest: the caller's own finding (squash, a NULL tensor) or NULL, reported where it always stood,
// after the activation.
template <class W>
ha_status check_header(const W* w, char* err, const char* layers, const char* what, const char* built,
                       const char* rest) {
    char m[200];
    if (w->n_lstm_layers != 1) {
        snprintf(m, sizeof m, "n_lstm_layers = %d: %s", w->n_lstm_layers, layers);
        return fail_to(err, HE_ESHAPE, m);
    }
    if (w->obs_dim != kObs || w->hidden != kHid || w->mlp_width != kMlp || w->act_dim != kAct) {
        snprintf(m, sizeof m, "%s shape obs %d / lstm %d / mlp %d / action %d: only %s is built", what, w->obs_dim,
                 w->hidden, w->mlp_width, w->act_dim, built);
        return fail_to(err, HE_ESHAPE, m);
    }
    if (w->activation != HA_ACT_TANH && w->activation != HA_ACT_RELU) return fail_to(err, HE_EINVAL, "unknown activation");
    if (rest) return fail_to(err, HE_EINVAL, rest);
    if ((w->obs_mean == nullptr) != (w->obs_var == nullptr))
        return fail_to(err, HE_EINVAL, "obs_mean and obs_var come together");
    return HE_OK;
}

ha_status check_weights(const ha_weights* w, ha_actor* a) {
    if (!w) return fail(a, HE_EINVAL, "weights is NULL");
    if (w->abi_version != HA_ABI_VERSION) return fail(a, HE_EINVAL, "ha_weights.abi_version mismatch");
    const char* rest = w->squash != HA_SQUASH_CLIP && w->squash != HA_SQUASH_TANH ? "unknown squash"
                       : !actor_net(w).complete()                                 ? "an actor tensor is NULL"
                                                                                  : nullptr;
    return check_header(w, a ? a->err : nullptr, "this actor has one LSTM layer", "actor", "13 / 128 / 64 / 2", rest);
}

ha_status check_policy_weights(const ha_policy_weights* w, ha_policy* a) {
    if (!w) return fail(a, HE_EINVAL, "weights is NULL");
    if (w->abi_version != HA_POLICY_ABI_VERSION) return fail(a, HE_EINVAL, "ha_policy_weights.abi_version mismatch");
    const char* rest = !actor_net(w).complete() || !w->log_std ? "an actor tensor (or log_std) is NULL"
                       : !critic_net(w).complete()             ? "a critic tensor is NULL"
                                                               : nullptr;
    return check_header(w, a ? a->err : nullptr, "actor and critic have one LSTM layer each", "policy",
                        "13 / 128 / 64-64 / 2 actions / 1 value", rest);
}

// W[j][k] of the gate product over [x | h | 0]
inline float gate_w(const HostNet& w, int j, int k) {
    return k < kObs ? w.w_ih[j * kObs + k] : (k < kKx ? w.w_hh[j * kHid + (k - kObs)] : 0.0f);
}

// one packed network: float4-aligned sections, in floats
constexpr size_t o_wg = 0, n_wg = (size_t)4 * kStepsG * 64 * 4;
constexpr size_t o_bg = o_wg + n_wg, o_w1 = o_bg + kGates, o_b1 = o_w1 + (size_t)kMlp * kHid;
constexpr size_t o_w2 = o_b1 + kMlp, o_b2 = o_w2 + (size_t)kMlp * kMlp, o_w3 = o_b2 + kMlp;
constexpr size_t o_b3 = o_w3 + kAct * kMlp, kNetFloats = o_b3 + 4;
constexpr size_t kStatFloats = 2 * 3 * kObs;   // [3][13] doubles
static_assert(kNetFloats % 4 == 0, "the next section stays 16-byte aligned");

void pack_net(const HostNet& w, float* dst) {
    for (int ug = 0; ug < 4; ++ug)
        for (int s = 0; s < kStepsG; ++s)
            for (int l = 0; l < 64; ++l)
                for (int g = 0; g < 4; ++g)
                    dst[o_wg + (((size_t)ug * kStepsG + s) * 64 + l) * 4 + g] =
                        gate_w(w, g * kHid + ug * 32 + (l & 31), 2 * s + (l >> 5));
    for (int j = 0; j < kGates; ++j) dst[o_bg + j] = w.b_ih[j] + w.b_hh[j];
    for (int rt = 0; rt < 2; ++rt)
        for (int l = 0; l < 64; ++l) {
            for (int s = 0; s < kHid / 2; ++s)
                dst[o_w1 + ((size_t)rt * (kHid / 2) + s) * 64 + l] = w.w1[(rt * 32 + (l & 31)) * kHid + 2 * s + (l >> 5)];
            for (int s = 0; s < kMlp / 2; ++s)
                dst[o_w2 + ((size_t)rt * (kMlp / 2) + s) * 64 + l] = w.w2[(rt * 32 + (l & 31)) * kMlp + 2 * s + (l >> 5)];
        }
    memcpy(dst + o_b1, w.b1, kMlp * sizeof(float));
    memcpy(dst + o_b2, w.b2, kMlp * sizeof(float));
    memcpy(dst + o_w3, w.w3, (size_t)w.n_out * kMlp * sizeof(float));
    memcpy(dst + o_b3, w.b3, w.n_out * sizeof(float));
}

Net net_at(const float* d) {
    return {(const float4*)(d + o_wg), d + o_bg, d + o_w1, d + o_b1, d + o_w2, d + o_b2, d + o_w3, d + o_b3};
}

// [3][13] mean, sd = sqrt(var + eps), RN(1 / sd) at an 8-byte aligned dst
void pack_stats(const double* mean, const double* var, double epsilon, float* dst) {
    double stt[3 * kObs];
    for (int k = 0; k < kObs; ++k) {
        stt[k] = mean[k];
        stt[kObs + k] = sqrt(var[k] + epsilon);
        stt[2 * kObs + k] = 1.0 / stt[kObs + k];
    }
    memcpy(dst, stt, sizeof stt);
}

// the host's gate operand [x | h, zeroed when fresh | 0]
void host_xh(const float* x, const float* h, bool fresh, float* xh) {
    for (int k = 0; k < kObs; ++k) xh[k] = x[k];
    for (int u = 0; u < kHid; ++u) xh[kObs + u] = fresh ? 0.0f : h[u];
    xh[kKx] = 0.0f;
}

// THE gate chain of the contract on the host: the four pre-activations of unit u, each from
// b_ih + b_hh through fmaf over k = 0 .. kKp - 1 of xh
void host_gates(const HostNet& w, const float* xh, int u, float* pre) {
    for (int g = 0; g < 4; ++g) {
        const int j = g * kHid + u;
        float acc = w.b_ih[j] + w.b_hh[j];
        for (int k = 0; k < kKp; ++k) acc = fmaf(gate_w(w, j, k), xh[k], acc);
        pre[g] = acc;
    }
}

// Contract step 2 on the host: sd = sqrt(var + eps) and y = RN(1 / sd) once, then env(): env e's obs
// into x[kObs], and into obs_norm_out's row e where that is given
struct HostNorm {
    const double* mean;   // NULL: the obs are used as they come
    double sd[kObs], y[kObs], clip;
    bool has_clip;
    HostNorm(const double* obs_mean, const double* obs_var, double epsilon, bool has_clip_, double clip_obs)
        : mean(obs_mean), clip(clip_obs), has_clip(has_clip_) {
        for (int k = 0; mean && k < kObs; ++k) {
            sd[k] = sqrt(obs_var[k] + epsilon);
            y[k] = 1.0 / sd[k];
        }
    }
    void env(const float* obs, int64_t e, float* x, float* obs_norm_out) const {
        for (int k = 0; k < kObs; ++k) {
            float v = obs[e * kObs + k];
            if (mean) v = norm_obs(v, mean[k], sd[k], y[k], has_clip, clip);
            if (obs_norm_out) obs_norm_out[e * kObs + k] = v;
            x[k] = v;
        }
    }
};

// Contract steps 1, 3-5 for one env on the host: x is the (normalised) obs; h, c are read unless
// fresh and written when write_state; a2 receives the last hidden layer.
void host_net_env(const HostNet& w, const float* x, bool fresh, float* h, float* c, bool write_state, bool relu,
                  float* a2) {
    float xh[kKp], hn[kHid], cn[kHid], a1[kMlp], pre[4];
    host_xh(x, h, fresh, xh);
    for (int u = 0; u < kHid; ++u) {
        host_gates(w, xh, u, pre);
        float cv = fresh ? 0.0f : c[u];
        hn[u] = cell_update(pre[0], pre[1], pre[2], pre[3], &cv);
        cn[u] = cv;
    }
    if (write_state) {
        memcpy(h, hn, sizeof hn);
        memcpy(c, cn, sizeof cn);
    }
    for (int j = 0; j < kMlp; ++j) {
        float acc = w.b1[j];
        for (int k = 0; k < kHid; ++k) acc = fmaf(w.w1[j * kHid + k], hn[k], acc);
        a1[j] = mlp_act(acc, relu);
    }
    for (int j = 0; j < kMlp; ++j) {
        float acc = w.b2[j];
        for (int k = 0; k < kMlp; ++k) acc = fmaf(w.w2[j * kMlp + k], a1[k], acc);
        a2[j] = mlp_act(acc, relu);
    }
}

inline float host_head(const HostNet& w, int j, const float* a2) {
    float m = w.b3[j];
    for (int k = 0; k < kMlp; ++k) m = fmaf(w.w3[j * kMlp + k], a2[k], m);
    return m;
}

// the blob of a policy: [actor | critic | log_std, std | statistics]
constexpr size_t o_ls = 2 * kNetFloats, o_pst = o_ls + 4, kPolicyFloats = o_pst + kStatFloats;

void pack_policy(const ha_policy_weights* w, float* dst) {
    pack_net(actor_net(w), dst);
    pack_net(critic_net(w), dst + kNetFloats);
    for (int j = 0; j < kAct; ++j) {
        dst[o_ls + j] = w->log_std[j];
        dst[o_ls + kAct + j] = policy_std(w->log_std[j]);
    }
    if (w->obs_mean) pack_stats(w->obs_mean, w->obs_var, w->epsilon, dst + o_pst);
}

void policy_params(const ha_policy_weights* w, const float* d, PolicyParams* p) {
    memset(p, 0, sizeof *p);
    p->pi = net_at(d);
    p->vf = net_at(d + kNetFloats);
    p->ls = d + o_ls;
    p->stats = w->obs_mean ? (const double*)(d + o_pst) : nullptr;
    p->clip = w->clip_obs;
    p->has_clip = w->has_clip;
    p->relu = w->activation == HA_ACT_RELU;
}

ha_status check_gae(int64_t n, int64_t K, double gamma, double gae_lambda, const void* rewards, const void* values,
                    const void* episode_starts, const void* last_values, const void* last_dones,
                    const void* advantages, const void* returns) {
    if (n < 1 || K < 1) return fail_to(nullptr, HE_EINVAL, "n and K must be >= 1");
    if (!(gamma == gamma) || !(gae_lambda == gae_lambda)) return fail_to(nullptr, HE_EINVAL, "gamma / gae_lambda is NaN");
    if (!rewards || !values || !episode_starts || !last_values || !last_dones || !advantages || !returns)
        return fail_to(nullptr, HE_EINVAL, "a GAE buffer is NULL");
    return HE_OK;
}

// ---------------------------------------------------------------- the LSTM over a stored sequence
// lstm_seq_fwd_kernel / lstm_seq_bwd_kernel (ha_lstm_seq_forward / _backward, contract F1-F2 and
// B1-B4): grid (tiles, n_nets), a workgroup of 4 waves owns 32 envs of one network for ALL L steps.
//   forward   net_tile's gate section per step; c stays in registers, h' goes to the OTHER half of a
//             double-buffered xh (zeroed where the next step starts an episode) beside the next
//             step's x, so one barrier per step orders the B-operand reads against the writes.
//   backward  the cell backward in registers on the forward's (unit, env) ownership; d_gates[t] to
//             HBM and to LDS as dg[u][env]; dh_rec = W_hh^T d_gates as ONE accumulator per wave
//             (output units 32 w .. 32 w + 31) over 256 k-steps of 32x32x2: the k-ordered chain over
//             u = 0 .. 511.  Two barriers per step (dg written / dg read).
// The weights arrive as device tensors in torch layout and are packed into the workspace by a small
// kernel in front of each launch: [wg | bg | wt] per network, wg / bg as pack_net's, wt[w][s][lane] =
// w_hh[2 s + (lane >> 5)][32 w + (lane & 31)].
constexpr int kStepsB = kGates / 2;   // 256 k-steps of the recurrent gradient
constexpr size_t kSeqBg = n_wg, kSeqWt = kSeqBg + kGates, kSeqNetFloats = kSeqWt + (size_t)4 * kStepsB * 64;
static_assert(kSeqBg % 4 == 0 && kSeqWt % 4 == 0 && kSeqNetFloats % 4 == 0, "16-byte aligned sections");

struct SeqPackParams {
    const float* w_ih[2];
    const float* w_hh[2];
    const float* b_ih[2];
    const float* b_hh[2];
    float* ws;
};

struct SeqFwdParams {
    int64_t L, B;
    const float* x;
    const uint8_t* start;
    ha_lstm_seq_net net[2];
    const float* ws;
};

struct SeqBwdParams {
    int64_t L, B;
    const uint8_t* start;
    ha_lstm_seq_bwd net[2];
    const float* ws;
};

// grid (blocks, n_nets): the forward's sections
__global__ __launch_bounds__(256) void lstm_seq_pack_fwd_kernel(const SeqPackParams p) {
    const bool second = blockIdx.y != 0;
    const float* __restrict__ w_ih = second ? p.w_ih[1] : p.w_ih[0];
    const float* __restrict__ w_hh = second ? p.w_hh[1] : p.w_hh[0];
    const float* __restrict__ b_ih = second ? p.b_ih[1] : p.b_ih[0];
    const float* __restrict__ b_hh = second ? p.b_hh[1] : p.b_hh[0];
    float* dst = p.ws + (second ? kSeqNetFloats : 0);
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < kSeqWt; idx += gridDim.x * 256) {
        float v;
        if (idx < kSeqBg) {
            const int g = idx & 3, l = (idx >> 2) & 63;
            const int rest = idx >> 8, ug = rest / kStepsG, s = rest - ug * kStepsG;
            const int j = g * kHid + ug * 32 + (l & 31), k = 2 * s + (l >> 5);
            v = k < kObs ? w_ih[j * kObs + k] : (k < kKx ? w_hh[j * kHid + (k - kObs)] : 0.0f);
        } else {
            const int j = idx - kSeqBg;
            v = b_ih[j] + b_hh[j];
        }
        dst[idx] = v;
    }
}

// grid (blocks, n_nets): the backward's section, W_hh transposed in fragment order
__global__ __launch_bounds__(256) void lstm_seq_pack_bwd_kernel(const SeqPackParams p) {
    const bool second = blockIdx.y != 0;
    const float* __restrict__ w_hh = second ? p.w_hh[1] : p.w_hh[0];
    float* dst = p.ws + (second ? kSeqNetFloats : 0) + kSeqWt;
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < 4u * kStepsB * 64; idx += gridDim.x * 256) {
        const int l = idx & 63, s = (idx >> 6) & (kStepsB - 1), w = idx >> 14;
        dst[idx] = w_hh[(2 * s + (l >> 5)) * kHid + w * 32 + (l & 31)];
    }
}

struct SeqTile {
    float xh[2][kKp][kLd];   // 37,488 B: step t reads [t & 1] and fills [(t + 1) & 1]
};

__global__ __launch_bounds__(kThreads, 2) void lstm_seq_fwd_kernel(const SeqFwdParams p) {
    __shared__ SeqTile t;
    const int tid = threadIdx.x;
    const int64_t B = p.B, L = p.L;
    const int64_t e0 = (int64_t)blockIdx.x * kTile;
    const bool second = blockIdx.y != 0;
    const ha_lstm_seq_net nt = second ? p.net[1] : p.net[0];
    const float* ws = p.ws + (second ? kSeqNetFloats : 0);
    const float* __restrict__ bg = ws + kSeqBg;
    const uint8_t* __restrict__ start = p.start;
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    const int64_t e = e0 + col;
    const bool valid = e < B;
    const int nx = (int)((B - e0 < kTile ? B - e0 : kTile) * kObs);   // the tile's x of one step: contiguous
    const int el0 = tid / kObs, k0 = tid - el0 * kObs;
    const int el1 = (tid + kThreads) / kObs, k1 = (tid + kThreads) - el1 * kObs;

    // ---- step 0's operand: [x[0] | h0, zeroed at a start | 0]; the padding row of both halves
    {
        const float* x0 = p.x + e0 * kObs;
        t.xh[0][k0][el0] = tid < nx ? x0[tid] : 0.0f;
        if (tid + kThreads < kTile * kObs) t.xh[0][k1][el1] = tid + kThreads < nx ? x0[tid + kThreads] : 0.0f;
        for (int idx = tid; idx < kTile * kHid; idx += kThreads) {
            const int el = idx >> 7, u = idx & (kHid - 1);
            float v = 0.0f;
            if (e0 + el < B && !start[e0 + el]) v = nt.h0[(e0 + el) * kHid + u];
            t.xh[0][kObs + u][el] = v;
        }
        if (tid < 2 * kTile) t.xh[tid >> 5][kKx][tid & 31] = 0.0f;
    }
    float cc[16];
    {
        const bool fresh = valid && start[e] != 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (valid && !fresh) cv = *(const float4*)(nt.c0 + e * kHid + wave * 32 + 8 * q + 4 * hi);
            cc[4 * q + 0] = cv.x; cc[4 * q + 1] = cv.y; cc[4 * q + 2] = cv.z; cc[4 * q + 3] = cv.w;
        }
    }
    __syncthreads();

    const float4* wp = (const float4*)ws + (size_t)wave * kStepsG * 64 + lane;
    for (int64_t ts = 0; ts < L; ++ts) {
        const int cur = (int)(ts & 1), nxt = cur ^ 1;
        const bool more = ts + 1 < L;
        // the next step's x and start flag: issued now, used after the gate product
        float xv0 = 0.0f, xv1 = 0.0f;
        bool nfresh = false;
        if (more) {
            const float* xn = p.x + ((ts + 1) * B + e0) * kObs;
            if (tid < nx) xv0 = xn[tid];
            if (tid + kThreads < nx) xv1 = xn[tid + kThreads];
            nfresh = valid && start[(ts + 1) * B + e] != 0;
        }
        // weights and bias are re-read every step (L2 hits): loop-invariant loads hoisted out of
        // the step loop would sit in registers and spill
        const float* bgs = bg;
        const float4* wps = wp;
        asm volatile("" : "+s"(bgs), "+v"(wps));
        f32x16 acc[4];   // net_tile's gate product: a shared inline moves both code objects, so there are two copies
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b = *(const float4*)(bgs + g * kHid + wave * 32 + 8 * q + 4 * hi);
                acc[g][4 * q + 0] = b.x; acc[g][4 * q + 1] = b.y; acc[g][4 * q + 2] = b.z; acc[g][4 * q + 3] = b.w;
            }
#pragma unroll 4
        for (int s = 0; s < kStepsG; ++s) {
            const float4 w = wps[s * 64];
            const float b = t.xh[cur][2 * s + hi][col];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, b, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, b, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, b, acc[3], 0, 0, 0);
        }
        // ---- cell update in registers; h', c', gates leave as 16-byte lines
        const int64_t row = ts * B + e;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = wave * 32 + 8 * q + 4 * hi;
            float hv[4], gt[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * q + j;
                hv[j] = cell_forward(acc[0][r], acc[1][r], acc[2][r], acc[3][r], &cc[r], gt[j]);
                if (more) t.xh[nxt][kObs + u + j][col] = nfresh ? 0.0f : hv[j];
            }
            if (valid) {
                *(float4*)(nt.h + row * kHid + u) = make_float4(hv[0], hv[1], hv[2], hv[3]);
                *(float4*)(nt.c + row * kHid + u) = make_float4(cc[4 * q], cc[4 * q + 1], cc[4 * q + 2], cc[4 * q + 3]);
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *(float4*)(nt.gates + (row * 4 + g) * kHid + u) = make_float4(gt[0][g], gt[1][g], gt[2][g], gt[3][g]);
            }
            if (nfresh) cc[4 * q] = cc[4 * q + 1] = cc[4 * q + 2] = cc[4 * q + 3] = 0.0f;
        }
        if (more) {
            t.xh[nxt][k0][el0] = xv0;
            if (tid + kThreads < kTile * kObs) t.xh[nxt][k1][el1] = xv1;
        }
        __syncthreads();
    }
}

struct SeqBwdTile {
    float dg[kGates][kLd];   // 67,584 B: d_gates[t] of the tile, the B operand of the recurrent gradient
};

__global__ __launch_bounds__(kThreads, 2) void lstm_seq_bwd_kernel(const SeqBwdParams p) {
    __shared__ SeqBwdTile t;
    const int tid = threadIdx.x;
    const int64_t B = p.B, L = p.L;
    const int64_t e0 = (int64_t)blockIdx.x * kTile;
    const bool second = blockIdx.y != 0;
    const ha_lstm_seq_bwd nt = second ? p.net[1] : p.net[0];
    const uint8_t* __restrict__ start = p.start;
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    const int64_t e = e0 + col;
    const bool valid = e < B;
    const float* __restrict__ wt = p.ws + (second ? kSeqNetFloats : 0) + kSeqWt + (size_t)wave * kStepsB * 64 + lane;

    float dc[16], dhr[16], cur[16];   // the carries, and c[t] on its way down
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 cv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (valid) cv = *(const float4*)(nt.c + ((L - 1) * B + e) * kHid + wave * 32 + 8 * q + 4 * hi);
        cur[4 * q + 0] = cv.x; cur[4 * q + 1] = cv.y; cur[4 * q + 2] = cv.z; cur[4 * q + 3] = cv.w;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dc[r] = dhr[r] = 0.0f;

    for (int64_t ts = L - 1; ts >= 0; --ts) {
        const int64_t row = ts * B + e;
        const bool fresh = valid && start[row] != 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = wave * 32 + 8 * q + 4 * hi;
            const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float4 dh4 = z4, pv4 = z4, g4[4] = {z4, z4, z4, z4};
            if (valid) {
                dh4 = *(const float4*)(nt.d_h + row * kHid + u);
                pv4 = ts > 0 ? *(const float4*)(nt.c + (row - B) * kHid + u) : *(const float4*)(nt.c0 + e * kHid + u);
#pragma unroll
                for (int g = 0; g < 4; ++g) g4[g] = *(const float4*)(nt.gates + (row * 4 + g) * kHid + u);
            }
            const float dhv[4] = {dh4.x, dh4.y, dh4.z, dh4.w}, pv[4] = {pv4.x, pv4.y, pv4.z, pv4.w};
            const float gi[4] = {g4[0].x, g4[0].y, g4[0].z, g4[0].w}, gf[4] = {g4[1].x, g4[1].y, g4[1].z, g4[1].w};
            const float gg[4] = {g4[2].x, g4[2].y, g4[2].z, g4[2].w}, go[4] = {g4[3].x, g4[3].y, g4[3].z, g4[3].w};
            float d[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 4 * q + j;
                const float dh = dhv[j] + dhr[r];
                const float dcn = cell_backward(gi[j], gf[j], gg[j], go[j], cur[r], fresh ? 0.0f : pv[j], dh, dc[r], d[j]);
                dc[r] = fresh ? 0.0f : dcn;
                cur[r] = pv[j];
#pragma unroll
                for (int g = 0; g < 4; ++g) t.dg[g * kHid + u + j][col] = d[j][g];
            }
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *(float4*)(nt.d_gates + (row * 4 + g) * kHid + u) = make_float4(d[0][g], d[1][g], d[2][g], d[3][g]);
            }
        }
        if (ts == 0) break;   // h0 receives no gradient
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 8
        for (int s = 0; s < kStepsB; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[s * 64], t.dg[2 * s + hi][col], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) dhr[r] = fresh ? 0.0f : acc[r];
        __syncthreads();
    }
}

ha_status check_seq(int64_t n_nets, int64_t L, int64_t B) {
    char m[200];
    if (n_nets != 1 && n_nets != 2) {
        snprintf(m, sizeof m, "n_nets = %lld: one network or the actor / critic pair", (long long)n_nets);
        return fail_to(nullptr, HE_ESHAPE, m);
    }
    if (L < 1 || B < 1 || B > ((int64_t)1 << 30) || L > ((int64_t)1 << 30)) {
        snprintf(m, sizeof m, "sequence of L = %lld steps x B = %lld envs: both must be in [1, 2^30]", (long long)L,
                 (long long)B);
        return fail_to(nullptr, HE_ESHAPE, m);
    }
    return HE_OK;
}

inline bool bad_ptr(const void* q, uintptr_t mask) { return !q || (((uintptr_t)q) & mask); }

ha_status check_workspace(const void* workspace) {
    return bad_ptr(workspace, 15u) ? fail_to(nullptr, HE_EINVAL, "workspace must be non-NULL and 16-byte aligned") : HE_OK;
}

ha_status check_seq_fwd(int64_t n_nets, int64_t L, int64_t B, const void* x, const void* starts,
                        const ha_lstm_seq_net* nets, uintptr_t mask) {
    const ha_status st = check_seq(n_nets, L, B);
    if (st != HE_OK) return st;
    if (!nets) return fail_to(nullptr, HE_EINVAL, "nets is NULL");
    if (bad_ptr(x, mask) || bad_ptr(starts, mask))
        return fail_to(nullptr, HE_EINVAL, "x and episode_starts must be non-NULL and 16-byte aligned");
    for (int64_t k = 0; k < n_nets; ++k) {
        const ha_lstm_seq_net& n = nets[k];
        if (bad_ptr(n.w_ih, mask) || bad_ptr(n.w_hh, mask) || bad_ptr(n.b_ih, mask) || bad_ptr(n.b_hh, mask) ||
            bad_ptr(n.h0, mask) || bad_ptr(n.c0, mask) || bad_ptr(n.h, mask) || bad_ptr(n.c, mask) ||
            bad_ptr(n.gates, mask))
            return fail_to(nullptr, HE_EINVAL, "a tensor of ha_lstm_seq_net is NULL or not 16-byte aligned");
    }
    return HE_OK;
}

ha_status check_seq_bwd(int64_t n_nets, int64_t L, int64_t B, const void* starts, const ha_lstm_seq_bwd* nets,
                        uintptr_t mask) {
    const ha_status st = check_seq(n_nets, L, B);
    if (st != HE_OK) return st;
    if (!nets) return fail_to(nullptr, HE_EINVAL, "nets is NULL");
    if (bad_ptr(starts, mask)) return fail_to(nullptr, HE_EINVAL, "episode_starts must be non-NULL and 16-byte aligned");
    for (int64_t k = 0; k < n_nets; ++k) {
        const ha_lstm_seq_bwd& n = nets[k];
        if (bad_ptr(n.w_hh, mask) || bad_ptr(n.c0, mask) || bad_ptr(n.c, mask) || bad_ptr(n.gates, mask) ||
            bad_ptr(n.d_h, mask) || bad_ptr(n.d_gates, mask))
            return fail_to(nullptr, HE_EINVAL, "a tensor of ha_lstm_seq_bwd is NULL or not 16-byte aligned");
    }
    return HE_OK;
}

// ---------------------------------------------------------------- the LSTM's weight gradients
// lstm_wgrad_kernel / lstm_wgrad_reduce_kernel (ha_lstm_seq_weight_grads, contract W1-W4).
//   lstm_wgrad_kernel   grid (chunks, 4 groups of 128 gate rows, n_nets), 4 waves.  Wave w owns gate
//             rows u0 = 128 group + 32 w .. u0 + 31 against all of z, padded to five 32-column tiles:
//             five f32 accumulators D[u][column], independent, so the instruction's 64-cycle
//             dependent latency is covered.  The MFMA's k is the ROW index: lane l feeds
//             A = dg[r + (l >> 5)][u0 + (l & 31)] straight from global (a coalesced pair of 128-byte
//             lines per k-step, shared by the five tiles) and B = z[r + (l >> 5)][32 n + (l & 31)]
//             from LDS, so a block's 64 k-steps are W1's chain over its 128 rows.  z is built per
//             workgroup in LDS in sub-blocks of 32 rows, double-buffered, in the column order
//             [h_prev 128 | x 13 | 1 | 0 x 18] (16-byte stores of h; the chain runs over rows, so the
//             column order is free): the next sub-block's x, h (row r - B, or h0), start flags and A
//             operands are loaded before the current one's 80 MFMAs and stored after them, one
//             barrier per sub-block.  Rows past R load from row R - 1 and are replaced by +0: the
//             padding terms of W1.  After each block the accumulators are added into 80 f64
//             registers a lane (W2; v_add_f64 is IEEE) and zeroed; the chunk's p_c goes to the
//             workspace as [512][142] f64.
//   lstm_wgrad_reduce_kernel   one thread per output adds its p_c over the chunks in order and
//             rounds once (W3, W4).
constexpr int kWgSub = 32;                  // rows of a staged sub-block: 16 k-steps
constexpr int kWgSteps = kWgSub / 2;
constexpr int kWgTiles = 5;                 // 32-column tiles of z
constexpr int kWgCols = 32 * kWgTiles;      // 160
constexpr int kWgXcol = kHid;               // z's LDS columns: h_prev at 0, x at 128, the ones column at 141
constexpr int64_t kWgChunkRows = (int64_t)HA_WGRAD_BLOCK * HA_WGRAD_CHUNK;
constexpr size_t kWgPartial = (size_t)kGates * kKp;   // f64 of one chunk's p_c
static_assert(HA_WGRAD_BLOCK % kWgSub == 0 && HA_WGRAD_BLOCK >= kWgSub && HA_WGRAD_CHUNK >= 1, "whole sub-blocks");
static_assert(kKp <= kWgCols && kWgSub * kHid == 4 * 4 * kThreads && kWgSub * kObs <= 2 * kThreads, "staging passes");

struct WgradParams {
    int64_t R, B, n_chunks;
    const float* x;
    const uint8_t* start;
    ha_lstm_seq_wgrad net[2];
    double* ws;
};

struct WgradTile {
    float z[2][kWgSub][kWgCols];   // 40,960 B
};

// one sub-block's loads, held in registers across the MFMAs of the sub-block before it: raw values from
// clamped addresses (rows past R read row R - 1); wgrad_store / wgrad_operands replace them by +0.
// Nothing here depends on a loaded value, so no load is waited for before the MFMAs.
struct WgradStage {
    float4 h[4];
    float x[2];
    float a[kWgSteps];
    uint8_t fresh[4];
};

// the last in-range row of the sub-block at rb, relative to rb: 31 when it is whole, negative past R
__device__ __forceinline__ int wgrad_last_row(int64_t rb, int64_t R) {
    const int64_t lim = R - 1 - rb;
    return (int)(lim < kWgSub - 1 ? lim : kWgSub - 1);
}

// aoff = (lane >> 5) 512 + u0 + (lane & 31): the lane's part of its A operand's address
__device__ __forceinline__ void wgrad_load(WgradStage& st, const WgradParams& p, const ha_lstm_seq_wgrad& nt,
                                           int64_t rb, int tid, unsigned aoff) {
    const int64_t B = p.B;
    const int lim = wgrad_last_row(rb, p.R);
    if (lim == kWgSub - 1 && rb >= B) {
        // a whole sub-block past the first step: wave-uniform bases, the lane's part a 32-bit offset
        const float* hb = nt.h + (rb - B) * kHid;
        const uint8_t* eb = p.start + rb;
        const float* xb = p.x + rb * kObs;
        const float* ab = nt.d_gates + rb * kGates;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            st.h[i] = *(const float4*)(hb + i * 4 * kThreads + 4u * (unsigned)tid);
            st.fresh[i] = eb[i * (kThreads >> 5) + ((unsigned)tid >> 5)];
        }
        st.x[0] = xb[(unsigned)tid];
        st.x[1] = xb[(unsigned)tid < kWgSub * kObs - kThreads ? kThreads + (unsigned)tid : 0u];
#pragma unroll
        for (int s = 0; s < kWgSteps; ++s) st.a[s] = (ab + 2 * s * kGates)[aoff];
        return;
    }
    const int hi = (int)(aoff >> 9);
    const int xlim = lim * kObs + kObs - 1;   // the last in-range element of x relative to rb's first
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * kThreads, row = idx >> 5;
        const int64_t r = rb + (row < lim ? row : lim);
        const float* src = r >= B ? nt.h + (r - B) * kHid : nt.h0 + r * kHid;
        st.h[i] = *(const float4*)(src + 4 * (idx & 31));
        st.fresh[i] = p.start[r];
    }
    const float* xb = p.x + rb * kObs;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + i * kThreads;
        st.x[i] = xb[idx < xlim ? idx : xlim];
    }
    const float* ab = nt.d_gates + rb * kGates + (aoff & 511u);
#pragma unroll
    for (int s = 0; s < kWgSteps; ++s) {
        const int row = 2 * s + hi;
        st.a[s] = ab[(row < lim ? row : lim) * kGates];
    }
}

__device__ __forceinline__ void wgrad_store(float (*z)[kWgCols], const WgradStage& st, int64_t rb, int64_t R, int tid) {
    const int lim = wgrad_last_row(rb, R);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * kThreads, row = idx >> 5;
        const bool keep = (row <= lim) & (st.fresh[i] == 0);
        const float4 v = st.h[i];
        *(float4*)&z[row][4 * (idx & 31)] = make_float4(keep ? v.x : 0.0f, keep ? v.y : 0.0f, keep ? v.z : 0.0f, keep ? v.w : 0.0f);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + i * kThreads;
        if (idx < kWgSub * kObs) {
            const int row = idx / kObs;
            z[row][kWgXcol + (idx - row * kObs)] = row <= lim ? st.x[i] : 0.0f;
        }
    }
    if (tid < kWgSub) z[tid][kWgXcol + kObs] = tid <= lim ? 1.0f : 0.0f;
}

// the A operands of the sub-block at rb
__device__ __forceinline__ void wgrad_operands(float* ac, const WgradStage& st, int64_t rb, int64_t R, int hi) {
    const int lim = wgrad_last_row(rb, R);
#pragma unroll
    for (int s = 0; s < kWgSteps; ++s) ac[s] = 2 * s + hi <= lim ? st.a[s] : 0.0f;
}

__global__ __launch_bounds__(kThreads) void lstm_wgrad_kernel(const WgradParams p) {
    __shared__ WgradTile t;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    const bool second = blockIdx.z != 0;
    const ha_lstm_seq_wgrad nt = second ? p.net[1] : p.net[0];
    const int64_t R = p.R;
    const int64_t r0 = (int64_t)blockIdx.x * kWgChunkRows;   // the chunk's first row (< R)
    const int64_t rows = R - r0 < kWgChunkRows ? R - r0 : kWgChunkRows;
    const int n_sub = (int)((rows + HA_WGRAD_BLOCK - 1) / HA_WGRAD_BLOCK) * (HA_WGRAD_BLOCK / kWgSub);
    const int u0 = (int)blockIdx.y * kHid + wave * 32;
    const unsigned aoff = (unsigned)(hi * kGates + u0 + col);

    // the zero columns of both halves, and the first sub-block
    for (int idx = tid; idx < 2 * kWgSub * (kWgCols - kKp); idx += kThreads) {
        const int rw = idx / (kWgCols - kKp);
        t.z[rw >> 5][rw & 31][kKp + (idx - rw * (kWgCols - kKp))] = 0.0f;
    }
    WgradStage st;
    wgrad_load(st, p, nt, r0, tid, aoff);
    wgrad_store(t.z[0], st, r0, R, tid);
    float ac[kWgSteps];
    wgrad_operands(ac, st, r0, R, hi);
    __syncthreads();

    f32x16 acc[kWgTiles];
    double d[kWgTiles][16];
#pragma unroll
    for (int n = 0; n < kWgTiles; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[n][r] = 0.0f;
            d[n][r] = 0.0;
        }

    for (int sb = 0; sb < n_sub; ++sb) {
        const bool more = sb + 1 < n_sub;
        const int64_t rn = r0 + (int64_t)(sb + 1) * kWgSub;
        if (more) wgrad_load(st, p, nt, rn, tid, aoff);
        __builtin_amdgcn_sched_barrier(0);   // the loads are issued before the MFMAs, their uses come after
        const float* zb = &t.z[sb & 1][hi][col];
#pragma unroll
        for (int s = 0; s < kWgSteps; ++s) {
#pragma unroll
            for (int n = 0; n < kWgTiles; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[s], zb[2 * s * kWgCols + 32 * n], acc[n], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
            wgrad_store(t.z[(sb + 1) & 1], st, rn, R, tid);
            wgrad_operands(ac, st, rn, R, hi);
        }
        __syncthreads();
        if ((sb & (HA_WGRAD_BLOCK / kWgSub - 1)) == HA_WGRAD_BLOCK / kWgSub - 1) {   // a block is complete: W2
#pragma unroll
            for (int n = 0; n < kWgTiles; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    d[n][r] += (double)acc[n][r];
                    acc[n][r] = 0.0f;
                }
        }
    }

    // p_c[u][k]: tile n < 4 holds k = 13 + 32 n + col, tile 4 the x columns and the bias column
    double* out = p.ws + ((size_t)(second ? p.n_chunks : 0) + blockIdx.x) * kWgPartial;
#pragma unroll
    for (int n = 0; n < kWgTiles; ++n) {
        const int k = n < 4 ? kObs + 32 * n + col : (col < kObs ? col : (col == kObs ? kKx : -1));
        if (k < 0) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(size_t)(u0 + (r & 3) + 8 * (r >> 2) + 4 * hi) * kKp + k] = d[n][r];
    }
}

// grid (blocks of 256 outputs, n_nets)
__global__ __launch_bounds__(256) void lstm_wgrad_reduce_kernel(const WgradParams p) {
    const unsigned idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= kWgPartial) return;
    const bool second = blockIdx.y != 0;
    const ha_lstm_seq_wgrad nt = second ? p.net[1] : p.net[0];
    const double* __restrict__ src = p.ws + (size_t)(second ? p.n_chunks : 0) * kWgPartial + idx;
    double total = 0.0;
    for (int64_t c = 0; c < p.n_chunks; ++c) total += src[c * kWgPartial];
    const float v = (float)total;
    const int u = idx / kKp, k = idx - u * kKp;
    if (k < kObs) nt.d_w_ih[u * kObs + k] = v;
    else if (k < kKx) nt.d_w_hh[u * kHid + (k - kObs)] = v;
    else nt.d_b[u] = v;
}

// one row's terms of W1 for every (u, k): s[u][k] = fmaf(dg[u], z[k], s[u][k]).  fmaf is correctly
// rounded whether libm computes it or the CPU's FMA unit; where the CPU has one, the second copy
// lets the k loop run on it eight wide (the same bits, an order of magnitude sooner).
#define HA_WGRAD_ROW_BODY                                                   \
    for (int u = 0; u < kGates; ++u) {                                      \
        const float a = dg[u];                                              \
        float* su = s + (size_t)u * kKp;                                    \
        for (int k = 0; k < kKp; ++k) su[k] = __builtin_fmaf(a, z[k], su[k]); \
    }
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define HA_WGRAD_FMA_COPY 1
__attribute__((target("avx2,fma"))) void wgrad_row_fma(const float* __restrict__ dg, const float* __restrict__ z,
                                                       float* __restrict__ s) {
    HA_WGRAD_ROW_BODY
}
#endif
void wgrad_row(const float* __restrict__ dg, const float* __restrict__ z, float* __restrict__ s) {
#ifdef HA_WGRAD_FMA_COPY
    static const bool fma_unit = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    if (fma_unit) return wgrad_row_fma(dg, z, s);
#endif
    HA_WGRAD_ROW_BODY
}
#undef HA_WGRAD_ROW_BODY

int64_t wgrad_chunks(int64_t L, int64_t B) { return (L * B + kWgChunkRows - 1) / kWgChunkRows; }

ha_status check_wgrad(int64_t n_nets, int64_t L, int64_t B, const void* x, const void* starts,
                      const ha_lstm_seq_wgrad* nets, uintptr_t mask) {
    ha_status st = check_seq(n_nets, L, B);
    if (st != HE_OK) return st;
    if (wgrad_chunks(L, B) > 0x7fffffffll) {
        char m[200];
        snprintf(m, sizeof m, "L B = %lld rows: more than 2^31 - 1 chunks of %lld rows", (long long)(L * B),
                 (long long)kWgChunkRows);
        return fail_to(nullptr, HE_ESHAPE, m);
    }
    if (!nets) return fail_to(nullptr, HE_EINVAL, "nets is NULL");
    if (!x || bad_ptr(starts, mask))
        return fail_to(nullptr, HE_EINVAL, "x must be non-NULL, episode_starts non-NULL and 16-byte aligned");
    for (int64_t k = 0; k < n_nets; ++k) {
        const ha_lstm_seq_wgrad& n = nets[k];
        if (bad_ptr(n.d_gates, mask) || bad_ptr(n.h, mask) || bad_ptr(n.h0, mask) || bad_ptr(n.d_w_ih, mask) ||
            bad_ptr(n.d_w_hh, mask) || bad_ptr(n.d_b, mask))
            return fail_to(nullptr, HE_EINVAL, "a tensor of ha_lstm_seq_wgrad is NULL or not 16-byte aligned");
    }
    return HE_OK;
}

// ---------------------------------------------------------------- a policy's blob from device tensors
// policy_pack_kernel (ha_policy_refresh): pack_policy's layout written from the 21 tensors where they
// stand on the device, grid-stride over the blob's floats up to the statistics; then the tensors
// themselves, flat in ha_policy_weights' order, behind the blob (ha_policy_download).
constexpr int kPolicyTensors = 21;
constexpr size_t kSnapFloats = HA_POLICY_TENSOR_FLOATS;
constexpr int kTensorFloats[kPolicyTensors] = {
    kGates * kObs, kGates * kHid, kGates, kGates, kMlp * kHid, kMlp, kMlp * kMlp, kMlp, kAct * kMlp, kAct, kAct,
    kGates * kObs, kGates * kHid, kGates, kGates, kMlp * kHid, kMlp, kMlp * kMlp, kMlp, kMlp, 1};

struct PolicyPackParams {
    const float* t[kPolicyTensors];   // w_ih w_hh b_ih b_hh w1 b1 w2 b2 w3 b3 log_std, then the critic's ten
    int32_t off[kPolicyTensors + 1];  // where each begins in the flat copy
    float* blob;
    float* snap;
};

// float `i` of one packed network (pack_net's layout) from its tensors in torch layout
HE_HD float packed_net_float(unsigned i, const float* __restrict__ w_ih,
                                                  const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                  const float* __restrict__ b_hh, const float* __restrict__ w1,
                                                  const float* __restrict__ b1, const float* __restrict__ w2,
                                                  const float* __restrict__ b2, const float* __restrict__ w3,
                                                  const float* __restrict__ b3, unsigned n_out) {
    if (i < o_bg) {
        const int g = i & 3, l = (i >> 2) & 63;
        const int rest = i >> 8, ug = rest / kStepsG, s = rest - ug * kStepsG;
        const int j = g * kHid + ug * 32 + (l & 31), k = 2 * s + (l >> 5);
        return k < kObs ? w_ih[j * kObs + k] : (k < kKx ? w_hh[j * kHid + (k - kObs)] : 0.0f);
    }
    if (i < o_w1) return b_ih[i - o_bg] + b_hh[i - o_bg];
    if (i < o_b1) {
        const unsigned q = i - o_w1, l = q & 63, rt = q >> 12, s = (q >> 6) & (kHid / 2 - 1);
        return w1[(rt * 32 + (l & 31)) * kHid + 2 * s + (l >> 5)];
    }
    if (i < o_w2) return b1[i - o_b1];
    if (i < o_b2) {
        const unsigned q = i - o_w2, l = q & 63, rt = q >> 11, s = (q >> 6) & (kMlp / 2 - 1);
        return w2[(rt * 32 + (l & 31)) * kMlp + 2 * s + (l >> 5)];
    }
    if (i < o_w3) return b2[i - o_b2];
    if (i < o_b3) return i - o_w3 < n_out * kMlp ? w3[i - o_w3] : 0.0f;
    return i - o_b3 < n_out ? b3[i - o_b3] : 0.0f;
}
static_assert(kHid / 2 == 64 && kMlp / 2 == 32, "the shifts of packed_net_float");

__global__ __launch_bounds__(256) void policy_pack_kernel(const PolicyPackParams p) {
    const unsigned first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (unsigned idx = first; idx < o_ls + 2 * kAct; idx += stride) {
        float v;
        if (idx < kNetFloats)
            v = packed_net_float(idx, p.t[0], p.t[1], p.t[2], p.t[3], p.t[4], p.t[5], p.t[6], p.t[7], p.t[8], p.t[9], kAct);
        else if (idx < o_ls)
            v = packed_net_float(idx - kNetFloats, p.t[11], p.t[12], p.t[13], p.t[14], p.t[15], p.t[16], p.t[17],
                                 p.t[18], p.t[19], p.t[20], 1);
        else
            v = idx < o_ls + kAct ? p.t[10][idx - o_ls] : policy_std(p.t[10][idx - o_ls - kAct]);
        p.blob[idx] = v;
    }
#pragma unroll
    for (int k = 0; k < kPolicyTensors; ++k) {
        const float* __restrict__ src = p.t[k];
        float* dst = p.snap + p.off[k];
        const unsigned n = p.off[k + 1] - p.off[k];
        for (unsigned i = first; i < n; i += stride) dst[i] = src[i];
    }
}

// ---------------------------------------------------------------- the optimizer step (contract O1-O5)
// opt_norm_kernel: one workgroup per block of 256 elements, the f64 tree of O1 in LDS, s_b to the
// workspace.  opt_adam_kernel: the same grid; every thread adds the s_b in order (the same loads and
// adds in every lane of every workgroup: the same bits), then updates its element.  The tensors and
// the first block of each travel in the kernel's arguments.
struct AdamParams {
    ha_adam_tensor t[HA_OPT_MAX_TENSORS];
    int32_t first[HA_OPT_MAX_TENSORS + 1];   // first[k]: the first block of tensor k; first[n]: all blocks
    int32_t n;
    AdamConsts k;
    double* partial;
    float* norm_out;
};

// the tensor of block b: the last k with first[k] <= b (wave-uniform)
__device__ __forceinline__ int adam_tensor_of(const AdamParams& p, int b) {
    int k = 0;
    while (k + 1 < p.n && p.first[k + 1] <= b) ++k;
    return k;
}

__global__ __launch_bounds__(HA_OPT_BLOCK) void opt_norm_kernel(const AdamParams p) {
    __shared__ double q[HA_OPT_BLOCK];
    const int b = blockIdx.x, tid = threadIdx.x, k = adam_tensor_of(p, b);
    const int64_t i = (int64_t)(b - p.first[k]) * HA_OPT_BLOCK + tid;
    const float g = i < p.t[k].numel ? p.t[k].grad[i] : 0.0f;
    q[tid] = (double)g * (double)g;
    for (int off = HA_OPT_BLOCK / 2; off >= 1; off >>= 1) {
        __syncthreads();
        if (tid < off) q[tid] = q[tid] + q[tid + off];
    }
    if (tid == 0) p.partial[b] = q[0];
}

__global__ __launch_bounds__(HA_OPT_BLOCK) void opt_adam_kernel(const AdamParams p) {
    const int b = blockIdx.x, tid = threadIdx.x, k = adam_tensor_of(p, b);
    const int nb = p.first[p.n];
    const double* __restrict__ partial = p.partial;
    double total = 0.0;
    for (int j = 0; j < nb; ++j) total = total + partial[j];
    float norm;
    const float c = adam_clip(total, p.k, &norm);
    if (b == 0 && tid == 0 && p.norm_out) *p.norm_out = norm;
    const int64_t i = (int64_t)(b - p.first[k]) * HA_OPT_BLOCK + tid;
    if (i >= p.t[k].numel) return;
    float pv = p.t[k].param[i], m = p.t[k].exp_avg[i], v = p.t[k].exp_avg_sq[i];
    adam_element(p.t[k].grad[i], c, p.k, &pv, &m, &v);
    p.t[k].param[i] = pv;
    p.t[k].exp_avg[i] = m;
    p.t[k].exp_avg_sq[i] = v;
}

// The checks of ha_adam_step / ha_host_adam_step; fills first[] and the constants (hy and k NULL: the
// shapes alone, for the workspace's size).
ha_status check_adam(int64_t n, const ha_adam_tensor* ts, const ha_adam_hyper* hy, int32_t* first, AdamConsts* k) {
    char m[200];
    if (n < 1 || n > HA_OPT_MAX_TENSORS) {
        snprintf(m, sizeof m, "n_tensors = %lld: 1 to %d tensors a call", (long long)n, HA_OPT_MAX_TENSORS);
        return fail_to(nullptr, HE_ESHAPE, m);
    }
    if (!ts) return fail_to(nullptr, HE_EINVAL, "tensors is NULL");
    int64_t blocks = 0;
    for (int64_t j = 0; j < n; ++j) {
        if (ts[j].numel < 1) {
            snprintf(m, sizeof m, "tensor %lld has numel %lld", (long long)j, (long long)ts[j].numel);
            return fail_to(nullptr, HE_ESHAPE, m);
        }
        first[j] = (int32_t)blocks;
        blocks += (ts[j].numel - 1) / HA_OPT_BLOCK + 1;
        if (blocks > HA_OPT_MAX_BLOCKS) {
            snprintf(m, sizeof m, "more than %d blocks of %d elements in one call", HA_OPT_MAX_BLOCKS, HA_OPT_BLOCK);
            return fail_to(nullptr, HE_ESHAPE, m);
        }
    }
    first[n] = (int32_t)blocks;
    if (!hy) return k ? fail_to(nullptr, HE_EINVAL, "hyper is NULL") : HE_OK;   // (the workspace's size needs none)
    for (int64_t j = 0; j < n; ++j)
        if (!ts[j].param || !ts[j].grad || !ts[j].exp_avg || !ts[j].exp_avg_sq)
            return fail_to(nullptr, HE_EINVAL, "a tensor pointer is NULL");
    const double inf = __builtin_inf();
    if (hy->t < 1) return fail_to(nullptr, HE_EINVAL, "t is the 1-based step count");
    if (!(hy->lr > -inf && hy->lr < inf) || !(hy->eps >= 0.0 && hy->eps < inf))
        return fail_to(nullptr, HE_EINVAL, "lr must be finite, eps finite and >= 0");
    if (!(hy->beta1 >= 0.0 && hy->beta1 < 1.0) || !(hy->beta2 >= 0.0 && hy->beta2 < 1.0))
        return fail_to(nullptr, HE_EINVAL, "beta1 and beta2 must be in [0, 1)");
    k->b1 = (float)hy->beta1;
    k->b2 = (float)hy->beta2;
    k->a1 = (float)(1.0 - hy->beta1);
    k->a2 = (float)(1.0 - hy->beta2);
    k->ss = (float)(hy->lr / (1.0 - pow(hy->beta1, (double)hy->t)));
    k->bc2s = (float)sqrt(1.0 - pow(hy->beta2, (double)hy->t));
    k->eps = (float)hy->eps;
    k->clip = hy->max_grad_norm > 0.0 && hy->max_grad_norm < inf;
    k->max_norm = k->clip ? (float)hy->max_grad_norm : 0.0f;
    return HE_OK;
}

// ---------------------------------------------------------------- the PPO loss (contract L1-L6)
// One workgroup of 256 per block of HA_LOSS_BLOCK rows; lane i owns rows i, i + 256, ... of its block
// (L1), so a wave's load is 256 consecutive bytes of each array.  The blocks' sums go to the workspace
// as f64, [sum A | sum (A - mean)^2 | pol | val | ent | kl | clipped][block]; the launch after reads them:
//   loss_mean_kernel    s_b of L2.
//   loss_spread_kernel  every workgroup adds the s_b of L2 in block order (loss_totals: the same adds
//                       everywhere, the same bits) and forms its s_b of L3.
//   loss_rows_kernel    both lists' totals (lanes 0 and 1, one chain each), the row's loads in flight
//                       meanwhile; loss_row per row, the gradients stored, the five s_b of L5 through one
//                       tree.
//   loss_stats_kernel   one workgroup: lane l < 7 adds list l in block order, lane 0 forms the statistics.
// The serial totals bound a large call, as O2 bounds ha_adam_step: HA_LOSS_MAX_BLOCKS is the cap.
constexpr int kLossLanes = 256, kLossPerLane = HA_LOSS_BLOCK / kLossLanes, kLossLists = 7, kLossStage = 512;
static_assert(HA_LOSS_BLOCK % kLossLanes == 0 && kLossPerLane >= 1, "whole rows a lane");
static_assert((int64_t)HA_LOSS_BLOCK * HA_LOSS_MAX_BLOCKS >= (int64_t)256 * 16384, "a 256 x 16,384 buffer is one call");

struct LossParams {
    ha_ppo_loss_io io;
    LossConsts k;
    int64_t n;
    int32_t nb;
    double* ws;   // [kLossLists][nb]
};

// the tree of O1 over NQ lists of 256 lane sums at once; q[j][0] is list j's s_b (read by lane 0)
template <int NQ>
__device__ __forceinline__ void loss_tree(double (*q)[kLossLanes], int tid) {
    for (int off = kLossLanes / 2; off >= 1; off >>= 1) {
        __syncthreads();
        if (tid < off) {
#pragma unroll
            for (int j = 0; j < NQ; ++j) q[j][tid] = q[j][tid] + q[j][tid + off];
        }
    }
}

// L1's totals of NL lists of nb block sums that lie nb apart from `lists`: the blocks' sums are staged in
// LDS kLossStage blocks at a time by all lanes (coalesced loads, no chain of load latencies), and lane
// l < NL adds list l from 0.0 in block order.  Every workgroup makes the same adds in the same order:
// the same bits.  On return (after a barrier) tot[l] holds list l's total.
template <int NL>
__device__ __forceinline__ void loss_totals(const double* __restrict__ lists, int nb, int tid, double* stage,
                                            double* tot) {
    double t = 0.0;
    for (int j0 = 0; j0 < nb; j0 += kLossStage) {
        const int cnt = nb - j0 < kLossStage ? nb - j0 : kLossStage;
        __syncthreads();   // the chunk before is consumed (and, the first time, LDS of the caller's is free)
        for (int j = tid; j < cnt; j += kLossLanes) {
#pragma unroll
            for (int l = 0; l < NL; ++l) stage[j * NL + l] = lists[(int64_t)l * nb + j0 + j];
        }
        __syncthreads();
        if (tid < NL) {
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) t = t + stage[j * NL + tid];
        }
    }
    if (tid < NL) tot[tid] = t;
    __syncthreads();
}

__global__ __launch_bounds__(kLossLanes) void loss_mean_kernel(const LossParams p) {
    __shared__ double q[1][kLossLanes];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ adv = p.io.advantages;
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < kLossPerLane; ++m) {
        const int64_t i = (int64_t)b * HA_LOSS_BLOCK + m * kLossLanes + tid;
        s = s + (i < p.n ? (double)adv[i] : 0.0);
    }
    q[0][tid] = s;
    loss_tree<1>(q, tid);
    if (tid == 0) p.ws[b] = q[0][0];
}

__global__ __launch_bounds__(kLossLanes) void loss_spread_kernel(const LossParams p) {
    __shared__ double q[1][kLossLanes];
    __shared__ double stage[kLossStage];
    __shared__ double tot[1];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ adv = p.io.advantages;
    float a[kLossPerLane];
#pragma unroll
    for (int m = 0; m < kLossPerLane; ++m) {
        const int64_t i = (int64_t)b * HA_LOSS_BLOCK + m * kLossLanes + tid;
        a[m] = i < p.n ? adv[i] : 0.0f;
    }
    loss_totals<1>(p.ws, p.nb, tid, stage, tot);
    const double mean = tot[0] / p.k.n;
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < kLossPerLane; ++m) {
        const int64_t i = (int64_t)b * HA_LOSS_BLOCK + m * kLossLanes + tid;
        const double dev = (double)a[m] - mean;
        s = s + (i < p.n ? dev * dev : 0.0);
    }
    q[0][tid] = s;
    loss_tree<1>(q, tid);
    if (tid == 0) p.ws[p.nb + b] = q[0][0];
}

__global__ __launch_bounds__(kLossLanes) void loss_rows_kernel(const LossParams p) {
    __shared__ double q[5][kLossLanes];
    __shared__ double stage[2 * kLossStage];
    __shared__ double tot[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const ha_ppo_loss_io& io = p.io;
    float v[kLossPerLane], lp[kLossPerLane], en[kLossPerLane], ol[kLossPerLane], ad[kLossPerLane], re[kLossPerLane],
        ov[kLossPerLane];
#pragma unroll
    for (int m = 0; m < kLossPerLane; ++m) {
        const int64_t i = (int64_t)b * HA_LOSS_BLOCK + m * kLossLanes + tid;
        const bool in = i < p.n;
        v[m] = in ? io.values[i] : 0.0f;
        lp[m] = in ? io.log_prob[i] : 0.0f;
        en[m] = in ? io.entropy[i] : 0.0f;
        ol[m] = in ? io.old_log_prob[i] : 0.0f;
        ad[m] = in ? io.advantages[i] : 0.0f;
        re[m] = in ? io.returns[i] : 0.0f;
        ov[m] = (in && p.k.clip_vf) ? io.old_values[i] : 0.0f;
    }
    double mean = 0.0, den = 1.0;
    if (p.k.normalize) {
        loss_totals<2>(p.ws, p.nb, tid, stage, tot);
        mean = tot[0] / p.k.n;
        den = loss_std(tot[1], p.k.n) + 1e-8;
    }
    const double ge = -p.k.ent_coef;
    const float d_ent = (float)(ge / p.k.n);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int m = 0; m < kLossPerLane; ++m) {
        const int64_t i = (int64_t)b * HA_LOSS_BLOCK + m * kLossLanes + tid;
        const bool in = i < p.n;
        float d_v, d_lp;
        const LossTerms t = loss_row(v[m], lp[m], en[m], ol[m], ad[m], re[m], ov[m], mean, den, p.k, &d_v, &d_lp);
        s[0] = s[0] + (in ? t.pol : 0.0);
        s[1] = s[1] + (in ? t.val : 0.0);
        s[2] = s[2] + (in ? t.ent : 0.0);
        s[3] = s[3] + (in ? t.kl : 0.0);
        s[4] = s[4] + (in ? t.clipped : 0.0);
        if (in) {
            io.d_values[i] = d_v;
            io.d_log_prob[i] = d_lp;
            io.d_entropy[i] = d_ent;
        }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) q[j][tid] = s[j];
    loss_tree<5>(q, tid);
    if (tid < 5) p.ws[(int64_t)(2 + tid) * p.nb + b] = q[tid][0];
}

__global__ __launch_bounds__(kLossLanes) void loss_stats_kernel(const LossParams p) {
    __shared__ double stage[kLossLists * kLossStage];
    __shared__ double tot[kLossLists];
    const int tid = threadIdx.x;
    if (p.k.normalize)
        loss_totals<kLossLists>(p.ws, p.nb, tid, stage, tot);
    else
        loss_totals<kLossLists - 2>(p.ws + 2 * (int64_t)p.nb, p.nb, tid, stage, tot + 2);
    if (tid == 0) {
        const double mean = p.k.normalize ? tot[0] / p.k.n : 0.0;
        const double sd = p.k.normalize ? loss_std(tot[1], p.k.n) : 1.0;
        loss_stats(tot + 2, mean, sd, p.k, p.io.stats);
    }
}

// The checks of ha_ppo_loss / ha_host_ppo_loss; fills the constants (io, hy and k NULL: n_rows alone,
// for the workspace's size).
ha_status check_loss(int64_t n, const ha_ppo_loss_io* io, const ha_ppo_loss_hyper* hy, LossConsts* k) {
    char m[200];
    if (n < 1 || n > (int64_t)HA_LOSS_BLOCK * HA_LOSS_MAX_BLOCKS) {
        snprintf(m, sizeof m, "n_rows = %lld: 1 to %lld rows a call (%d blocks of %d)", (long long)n,
                 (long long)HA_LOSS_BLOCK * HA_LOSS_MAX_BLOCKS, HA_LOSS_MAX_BLOCKS, HA_LOSS_BLOCK);
        return fail_to(nullptr, HE_ESHAPE, m);
    }
    if (!k) return HE_OK;
    if (!io || !hy) return fail_to(nullptr, HE_EINVAL, "io or hyper is NULL");
    if (n == 1 && hy->normalize_advantage)
        return fail_to(nullptr, HE_ESHAPE, "n_rows = 1 with normalize_advantage: the unbiased std needs two rows");
    const double inf = __builtin_inf();
    if (!(hy->clip_range >= 0.0 && hy->clip_range < inf))
        return fail_to(nullptr, HE_EINVAL, "clip_range must be finite and >= 0");
    const bool clip_vf = hy->clip_range_vf > 0.0;
    if (clip_vf && !io->old_values) return fail_to(nullptr, HE_EINVAL, "clip_range_vf > 0 needs old_values");
    const void* ptrs[] = {io->values,  io->log_prob, io->entropy,    io->old_log_prob, io->advantages,
                          io->returns, io->d_values, io->d_log_prob, io->d_entropy,    io->stats};
    uintptr_t bits = clip_vf ? (uintptr_t)io->old_values : 0;
    for (const void* q : ptrs) {
        if (!q) return fail_to(nullptr, HE_EINVAL, "a pointer of io is NULL");
        bits |= (uintptr_t)q;
    }
    if (bits & 3u) return fail_to(nullptr, HE_EINVAL, "the pointers of io must be 4-byte aligned");
    k->c = hy->clip_range;
    k->lo = 1.0 - k->c;
    k->hi = 1.0 + k->c;
    k->cv = clip_vf ? hy->clip_range_vf : 0.0;
    k->ent_coef = hy->ent_coef;
    k->vf_coef = hy->vf_coef;
    k->vf2 = 2.0 * hy->vf_coef;
    k->n = (double)n;
    k->normalize = hy->normalize_advantage != 0;
    k->clip_vf = clip_vf;
    return HE_OK;
}

// L1 on the host over rows [0, n): term(row) in f64, a short last block padded with +0
template <class F>
double loss_sum_host(int64_t n, F term) {
    double total = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += HA_LOSS_BLOCK) {
        double q[kLossLanes];
        for (int i = 0; i < kLossLanes; ++i) {
            double s = 0.0;
            for (int m = 0; m < kLossPerLane; ++m) {
                const int64_t r = b0 + m * kLossLanes + i;
                s = s + (r < n ? term(r) : 0.0);
            }
            q[i] = s;
        }
        for (int off = kLossLanes / 2; off >= 1; off >>= 1)
            for (int i = 0; i < off; ++i) q[i] = q[i] + q[i + off];
        total = total + q[0];
    }
    return total;
}

// ---------------------------------------------------------------- the PPO heads (contract H1-H6)
// heads_pack_kernel / heads_fwd_kernel / heads_bwd_kernel / heads_lsd_kernel (ha_ppo_heads_forward /
// _backward).  A tile is 64 rows: two halves of 32, the MFMA's columns.  The four waves of a workgroup are
// (32-output slice, row half) pairs, and a workgroup keeps the A fragments of its slices resident over all
// the tiles it walks, read once from the workspace: 64 + 32 floats a lane in the backward's registers;
// in the forward, whose f64 activations need the registers, 32 there and layer 1's in LDS.
//   pack      the weights change with every optimizer step: W1, W2 in mlp_slice's fragment order, their
//             transposes in the same order (wt[o][s][lane] = W[2 s + (lane >> 5)][32 o + (lane & 31)]), and
//             log_std with std = policy_std(log_std).
//   forward   grid (groups of tiles, 2), y = actor / critic.  h of the tile to LDS as [half][k][row] at
//             kLd; layer 1 and layer 2 one accumulator each from the bias (mlp_slice's chain), a1 and a2
//             to LDS for the next product (over h, which layer 1 has read by then) and to HBM as 16-byte
//             lines from the accumulator's own layout; the head chain and H2 / H3 on the VALU, one lane
//             pair a row.  Layer 1's fragments stay in LDS, layer 2's in registers.
//   backward  grid (blocks of HA_LOSS_BLOCK rows, 2): a workgroup walks the 16 tiles of its block.  H4 and
//             H6's terms one lane a row (the terms wait in LDS for the block's tree); d_a2, d_z2 on the
//             VALU; d_z2, d_z1 through LDS as [half][u][row], the B operand of W2^T and W1^T with u as k,
//             accumulators from +0; d_h as 16-byte lines.  The actor's workgroup ends with L1's lane sums
//             and tree over its block and writes the two s_b; heads_lsd_kernel adds them in block order.
constexpr int kHRows = 64;                                  // rows of a tile
constexpr int kHTiles = HA_LOSS_BLOCK / kHRows;            // tiles of one block of L1
constexpr size_t kHw1p = 0, kHw2p = kHw1p + (size_t)kMlp * kHid, kHw1t = kHw2p + (size_t)kMlp * kMlp;
constexpr size_t kHw2t = kHw1t + (size_t)kMlp * kHid, kHeadsNetFloats = kHw2t + (size_t)kMlp * kMlp;
constexpr size_t kHls = 2 * kHeadsNetFloats, kHpart = kHls + 4;   // log_std[2], std[2]; then f64 [2][blocks]
static_assert(kHeadsNetFloats % 4 == 0 && (kHpart * sizeof(float)) % 16 == 0, "aligned sections");
static_assert(HA_LOSS_BLOCK % kHRows == 0 && kHRows == 2 * kTile, "whole tiles a block, two MFMA halves a tile");

struct HeadsNetW {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    int n_out;
};

inline HeadsNetW heads_net(const ha_ppo_heads_weights* w, bool critic) {
    return critic ? HeadsNetW{w->v1, w->vb1, w->v2, w->vb2, w->v3, w->vb3, 1}
                  : HeadsNetW{w->w1, w->b1, w->w2, w->b2, w->w3, w->b3, kAct};
}

struct HeadsPackParams {
    const float* w1[2];
    const float* w2[2];
    const float* log_std;
    float* ws;
};

struct HeadsFwdParams {
    int64_t n;
    int32_t relu, tiles_per_wg;
    ha_ppo_heads_fwd io;
    HeadsNetW net[2];
    const float* ws;
};

struct HeadsBwdParams {
    int64_t n;
    int32_t relu, nb;
    ha_ppo_heads_bwd io;
    HeadsNetW net[2];
    const float* ws;
    double* part;   // [2][nb]
};

// grid (blocks, 2): one network's four sections; the first thread pair of the grid adds log_std, std
__global__ __launch_bounds__(256) void heads_pack_kernel(const HeadsPackParams p) {
    const bool critic = blockIdx.y != 0;
    const float* __restrict__ w1 = critic ? p.w1[1] : p.w1[0];
    const float* __restrict__ w2 = critic ? p.w2[1] : p.w2[0];
    float* dst = p.ws + (critic ? kHeadsNetFloats : 0);
    for (unsigned idx = blockIdx.x * 256 + threadIdx.x; idx < kHeadsNetFloats; idx += gridDim.x * 256) {
        const int l = idx & 63, m = l & 31, hi = l >> 5;
        float v;
        if (idx < kHw2p) {          // [2][64][64]
            const int s = (idx >> 6) & 63, rt = idx >> 12;
            v = w1[(rt * 32 + m) * kHid + 2 * s + hi];
        } else if (idx < kHw1t) {   // [2][32][64]
            const unsigned i = idx - kHw2p;
            const int s = (i >> 6) & 31, rt = i >> 11;
            v = w2[(rt * 32 + m) * kMlp + 2 * s + hi];
        } else if (idx < kHw2t) {   // [4][32][64]
            const unsigned i = idx - kHw1t;
            const int s = (i >> 6) & 31, ot = i >> 11;
            v = w1[(2 * s + hi) * kHid + ot * 32 + m];
        } else {                    // [2][32][64]
            const unsigned i = idx - kHw2t;
            const int s = (i >> 6) & 31, ot = i >> 11;
            v = w2[(2 * s + hi) * kMlp + ot * 32 + m];
        }
        dst[idx] = v;
    }
    if (!critic && blockIdx.x == 0 && threadIdx.x < kAct) {
        const float ls = p.log_std[threadIdx.x];
        p.ws[kHls + threadIdx.x] = ls;
        p.ws[kHls + kAct + threadIdx.x] = policy_std(ls);
    }
}

struct HeadsFwdTile {
    float h[2][kHid][kLd];       // 33,792 B; once layer 1 has read h, a2 takes its rows 0 .. 63 and a1 its rows 64 .. 127
    float w1[2][kHid / 2][64];   // 32,768 B: layer 1's A fragments, both slices
    float w3[kAct * kMlp];
    float b1[kMlp], b2[kMlp];    // the small tensors once, not a pointer each through the tile loop
    float b3[4], ls[4];          // b3; log_std[2], std[2]
};

// the accumulator's registers from 16 consecutive-by-four biases: register 4 q + j is output 8 q + 4 hi + j
__device__ __forceinline__ void heads_bias(const float* b, int hi, float* out) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *(const float4*)(b + 8 * q + 4 * hi);
        out[4 * q + 0] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
    }
}

// act(acc) of one 32 x 32 product to LDS as out[unit][col] and, where the row exists, to HBM as four
// 16-byte lines of row `dst` (the row's 64 floats; o0 the slice's first unit)
__device__ __forceinline__ void heads_act_store(const f32x16& acc, float (*out)[kLd], float* dst, int o0, int col,
                                                int hi, bool relu) {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[o0 + (r & 3) + 8 * (r >> 2) + 4 * hi][col] = acc[r];
    // the lane's own 16 values back from LDS, four at a time in a rolled loop: the f64 temporaries of four
    // activations, not of sixteen, stand beside the resident fragments
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        const int u = o0 + 8 * q + 4 * hi;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = mlp_act(out[u + j][col], relu);
            out[u + j][col] = o[j];
        }
        if (dst) *(float4*)(dst + u) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

__global__ __launch_bounds__(kThreads, 2) void heads_fwd_kernel(const HeadsFwdParams p) {
    __shared__ HeadsFwdTile t;
    const int tid = threadIdx.x;
    const bool critic = blockIdx.y != 0;
    const bool relu = p.relu != 0;
    const HeadsNetW nw = critic ? p.net[1] : p.net[0];
    const float* __restrict__ ws = p.ws + (critic ? kHeadsNetFloats : 0);
    const float* __restrict__ h = critic ? p.io.h_vf : p.io.h_pi;
    float* a1o = critic ? p.io.a1_vf : p.io.a1_pi;
    float* a2o = critic ? p.io.a2_vf : p.io.a2_pi;
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    const int rt = wave & 1, rh = wave >> 1;   // output slice, row half

    // ---- the wave's A fragments and biases, resident over its tiles
    float w2r[kMlp / 2];
    {
        const float* w2p = ws + kHw2p + (size_t)rt * (kMlp / 2) * 64 + lane;
#pragma unroll
        for (int s = 0; s < kMlp / 2; ++s) w2r[s] = w2p[s * 64];
        for (int i = tid; i < kMlp * kHid; i += kThreads) (&t.w1[0][0][0])[i] = ws[kHw1p + i];
    }
    if (tid < nw.n_out * kMlp) t.w3[tid] = nw.w3[tid];
    if (tid < kMlp) t.b1[tid] = nw.b1[tid], t.b2[tid] = nw.b2[tid];
    if (tid < nw.n_out) t.b3[tid] = nw.b3[tid];
    if (tid < 4) t.ls[tid] = p.ws[kHls + tid];

    const int n = (int)p.n;   // at most 2^22 rows: 32-bit row arithmetic
    const int ntiles = (n + kHRows - 1) / kHRows;
    int tile = (int)blockIdx.x * p.tiles_per_wg;
    const int end = tile + p.tiles_per_wg < ntiles ? tile + p.tiles_per_wg : ntiles;
    for (; tile < end; ++tile) {
        const int r0 = tile * kHRows;
        // ---- stage h: a wave loads 8 rows x 128 B a pass; rows past n are zero columns
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
            const int row = (tid & 7) + 8 * it, k4 = ((tid >> 3) & 7) + 8 * wave;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r0 + row < n) v = *(const float4*)(h + (size_t)(r0 + row) * kHid + 4 * k4);
            float(*dst)[kLd] = t.h[row >> 5];
            dst[4 * k4 + 0][row & 31] = v.x;
            dst[4 * k4 + 1][row & 31] = v.y;
            dst[4 * k4 + 2][row & 31] = v.z;
            dst[4 * k4 + 3][row & 31] = v.w;
        }
        __syncthreads();
        const int r = r0 + rh * 32 + col;
        const bool valid = r < n;
        // ---- layer 1
        {
            float bias[16];
            heads_bias(t.b1 + rt * 32, hi, bias);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = bias[i];
#pragma unroll
            for (int s = 0; s < kHid / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t.w1[rt][s][lane], t.h[rh][2 * s + hi][col], acc, 0, 0, 0);
            __syncthreads();   // every wave has read h
            heads_act_store(acc, t.h[rh] + kMlp, valid ? a1o + (size_t)r * kMlp : nullptr, rt * 32, col, hi, relu);
        }
        __syncthreads();
        // ---- layer 2
        {
            float bias[16];
            heads_bias(t.b2 + rt * 32, hi, bias);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = bias[i];
#pragma unroll
            for (int s = 0; s < kMlp / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[s], t.h[rh][kMlp + 2 * s + hi][col], acc, 0, 0, 0);
            heads_act_store(acc, t.h[rh], valid ? a2o + (size_t)r * kMlp : nullptr, rt * 32, col, hi, relu);
        }
        __syncthreads();
        // ---- the head: lane pair (2 el, 2 el + 1) = the two outputs of row el (waves 0 and 1)
        if (tid < kHRows * kAct) {
            const int el = tid >> 1, j = tid & 1;
            const int re = r0 + el;
            const float(*a2)[kLd] = t.h[el >> 5];
            if (critic) {
                if (j == 0) {
                    const float v = head_chain(t.w3, t.b3[0], a2, el & 31);
                    if (re < n) p.io.values[re] = v;
                }
            } else {
                const float m = head_chain(t.w3 + j * kMlp, t.b3[j], a2, el & 31);
                const float mo = __shfl_xor(m, 1);
                if (j == 0 && re < n) {
                    const float mean[kAct] = {m, mo};
                    const float2 av = *(const float2*)(p.io.actions + (size_t)re * kAct);
                    const float a[kAct] = {av.x, av.y};
                    const float* ls = t.ls;
                    *(float2*)(p.io.mean + (size_t)re * kAct) = make_float2(m, mo);
                    p.io.log_prob[re] = heads_log_prob(a, mean, ls, ls + kAct);
                    p.io.entropy[re] = heads_entropy(ls);
                }
            }
        }
        __syncthreads();   // a2 is read before the next tile's h lands on it
    }
}

struct HeadsBwdTile {
    float dz2[2][kMlp][kLd];   // 16,896 B
    float dz1[2][kMlp][kLd];   // 16,896 B
    float dout[kHRows][kAct];
    float w3[kAct * kMlp];
    double term[kAct][HA_LOSS_BLOCK];   // 16,384 B: H6's terms of the block's rows
    double q[kAct][kLossLanes];
};

__global__ __launch_bounds__(kThreads, 2) void heads_bwd_kernel(const HeadsBwdParams p) {
    __shared__ HeadsBwdTile t;
    const int tid = threadIdx.x;
    const bool critic = blockIdx.y != 0;
    const bool relu = p.relu != 0;
    const HeadsNetW nw = critic ? p.net[1] : p.net[0];
    const float* __restrict__ ws = p.ws + (critic ? kHeadsNetFloats : 0);
    const float* __restrict__ a1i = critic ? p.io.a1_vf : p.io.a1_pi;
    const float* __restrict__ a2i = critic ? p.io.a2_vf : p.io.a2_pi;
    float* dz1o = critic ? p.io.d_z1_vf : p.io.d_z1_pi;
    float* dz2o = critic ? p.io.d_z2_vf : p.io.d_z2_pi;
    float* dho = critic ? p.io.d_h_vf : p.io.d_h_pi;
    const int wave = tid >> 6, lane = tid & 63;
    const int col = lane & 31, hi = lane >> 5;
    const int ot = wave & 1, rh = wave >> 1;   // W2^T: output slice ot; W1^T: slices 2 ot, 2 ot + 1
    const int n_out = nw.n_out;

    float w2r[kMlp / 2], w1r[2][kMlp / 2];
    {
        const float* w2t = ws + kHw2t + (size_t)ot * (kMlp / 2) * 64 + lane;
        const float* w1t = ws + kHw1t + (size_t)(2 * ot) * (kMlp / 2) * 64 + lane;
#pragma unroll
        for (int s = 0; s < kMlp / 2; ++s) {
            w2r[s] = w2t[s * 64];
            w1r[0][s] = w1t[s * 64];
            w1r[1][s] = w1t[(kMlp / 2 + s) * 64];
        }
    }
    if (tid < n_out * kMlp) t.w3[tid] = nw.w3[tid];
    else if (tid < kAct * kMlp) t.w3[tid] = 0.0f;

    const int64_t b0 = (int64_t)blockIdx.x * HA_LOSS_BLOCK;
    for (int ti = 0; ti < kHTiles; ++ti) {
        const int64_t r0 = b0 + (int64_t)ti * kHRows;
        if (r0 >= p.n) break;
        // ---- H4 and H6's terms: one lane a row
        if (tid < kHRows) {
            const int64_t re = r0 + tid;
            float d0 = 0.0f, d1 = 0.0f;
            if (critic) {
                if (re < p.n) d0 = p.io.d_values[re];
            } else {
                double t0 = 0.0, t1 = 0.0;
                if (re < p.n) {
                    const float* ls = p.ws + kHls;
                    const float2 av = *(const float2*)(p.io.actions + re * kAct);
                    const float2 mv = *(const float2*)(p.io.mean + re * kAct);
                    const float dlp = p.io.d_log_prob[re], den = p.io.d_entropy[re];
                    const double z0 = gauss_z(av.x, mv.x, ls[kAct]), z1 = gauss_z(av.y, mv.y, ls[kAct + 1]);
                    d0 = heads_d_mean(dlp, z0, ls[kAct]);
                    d1 = heads_d_mean(dlp, z1, ls[kAct + 1]);
                    t0 = heads_lsd_term(dlp, z0, den);
                    t1 = heads_lsd_term(dlp, z1, den);
                    *(float2*)(p.io.d_mean + re * kAct) = make_float2(d0, d1);
                }
                t.term[0][ti * kHRows + tid] = t0;
                t.term[1][ti * kHRows + tid] = t1;
            }
            t.dout[tid][0] = d0;
            t.dout[tid][1] = d1;
        }
        __syncthreads();
        // ---- d_a2 and d_z2 on the VALU: a wave takes 16 rows x 64 B of a2 a pass
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = (lane & 15) + 16 * it, k4 = (lane >> 4) + 4 * wave;
            const int64_t re = r0 + row;
            float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (re < p.n) av = *(const float4*)(a2i + re * kMlp + 4 * k4);
            const float a[4] = {av.x, av.y, av.z, av.w};
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.0f;
                for (int o = 0; o < n_out; ++o) s = fmaf(t.dout[row][o], t.w3[o * kMlp + 4 * k4 + j], s);
                d[j] = act_backward(s, a[j], relu);
                t.dz2[row >> 5][4 * k4 + j][row & 31] = d[j];
            }
            if (re < p.n) *(float4*)(dz2o + re * kMlp + 4 * k4) = make_float4(d[0], d[1], d[2], d[3]);
        }
        __syncthreads();
        const int64_t r = r0 + rh * 32 + col;
        const bool valid = r < p.n;
        // ---- d_a1 = W2^T d_z2, d_z1
        {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int s = 0; s < kMlp / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[s], t.dz2[rh][2 * s + hi][col], acc, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int u = ot * 32 + 8 * q + 4 * hi;
                float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (valid) av = *(const float4*)(a1i + r * kMlp + u);
                const float a[4] = {av.x, av.y, av.z, av.w};
                float d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    d[j] = act_backward(acc[4 * q + j], a[j], relu);
                    t.dz1[rh][u + j][col] = d[j];
                }
                if (valid) *(float4*)(dz1o + r * kMlp + u) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
        __syncthreads();
        // ---- d_h = W1^T d_z1: two output slices a wave
        {
            f32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
#pragma unroll
            for (int s = 0; s < kMlp / 2; ++s) {
                const float b = t.dz1[rh][2 * s + hi][col];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1r[0][s], b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1r[1][s], b, acc1, 0, 0, 0);
            }
            if (valid) {
                float* dst = dho + r * kHid + (2 * ot) * 32 + 4 * hi;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    *(float4*)(dst + 8 * q) = make_float4(acc0[4 * q], acc0[4 * q + 1], acc0[4 * q + 2], acc0[4 * q + 3]);
                    *(float4*)(dst + 32 + 8 * q) = make_float4(acc1[4 * q], acc1[4 * q + 1], acc1[4 * q + 2], acc1[4 * q + 3]);
                }
            }
        }
    }
    if (critic) return;
    // ---- H6: L1's lane sums and tree over the block's terms
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kAct; ++j) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < kLossPerLane; ++m) {
            const int i = m * kLossLanes + tid;
            s = s + (b0 + i < p.n ? t.term[j][i] : 0.0);
        }
        t.q[j][tid] = s;
    }
    loss_tree<kAct>(t.q, tid);
    if (tid < kAct) p.part[(int64_t)tid * p.nb + blockIdx.x] = t.q[tid][0];
}

// one workgroup: the blocks' sums of H6 in block order, rounded once
__global__ __launch_bounds__(kLossLanes) void heads_lsd_kernel(const double* __restrict__ part, int nb, float* d_log_std) {
    __shared__ double stage[kAct * kLossStage];
    __shared__ double tot[kAct];
    const int tid = threadIdx.x;
    loss_totals<kAct>(part, nb, tid, stage, tot);
    if (tid < kAct) d_log_std[tid] = (float)tot[tid];
}

// The checks of the four ha_ppo_heads entry points: m16 / m8 are the alignment masks of the [R][128],
// [R][64] and weight arrays and of the [R][2] arrays (3 on the host).  ptrs16 / ptrs8 / ptrs4 end at n16 ...
ha_status check_heads_rows(int64_t n) {
    char m[200];
    if (n < 1 || n > (int64_t)HA_LOSS_BLOCK * HA_LOSS_MAX_BLOCKS) {
        snprintf(m, sizeof m, "n_rows = %lld: 1 to %lld rows a call (%d blocks of %d)", (long long)n,
                 (long long)HA_LOSS_BLOCK * HA_LOSS_MAX_BLOCKS, HA_LOSS_MAX_BLOCKS, HA_LOSS_BLOCK);
        return fail_to(nullptr, HE_ESHAPE, m);
    }
    return HE_OK;
}

ha_status check_heads(int64_t n, const ha_ppo_heads_weights* w, const void* io, uintptr_t m16, uintptr_t m8,
                      const void* const* p16, int n16, const void* const* p8, int n8, const void* const* p4, int n4) {
    const ha_status st = check_heads_rows(n);
    if (st != HE_OK) return st;
    if (!w || !io) return fail_to(nullptr, HE_EINVAL, "weights or io is NULL");
    if (w->activation != HA_ACT_TANH && w->activation != HA_ACT_RELU) return fail_to(nullptr, HE_EINVAL, "unknown activation");
    const void* big[] = {w->w1, w->b1, w->w2, w->b2, w->w3, w->v1, w->vb1, w->v2, w->vb2, w->v3};
    const void* small[] = {w->b3, w->log_std, w->vb3};
    for (const void* q : big)
        if (bad_ptr(q, m16)) return fail_to(nullptr, HE_EINVAL, "a weight tensor is NULL or not 16-byte aligned");
    for (const void* q : small)
        if (bad_ptr(q, 3u)) return fail_to(nullptr, HE_EINVAL, "b3, vb3 or log_std is NULL or not 4-byte aligned");
    for (int i = 0; i < n16; ++i)
        if (bad_ptr(p16[i], m16)) return fail_to(nullptr, HE_EINVAL, "a [R][128] or [R][64] array of io is NULL or not 16-byte aligned");
    for (int i = 0; i < n8; ++i)
        if (bad_ptr(p8[i], m8)) return fail_to(nullptr, HE_EINVAL, "a [R][2] array of io is NULL or not 8-byte aligned");
    for (int i = 0; i < n4; ++i)
        if (bad_ptr(p4[i], 3u)) return fail_to(nullptr, HE_EINVAL, "a per-row array of io is NULL or not 4-byte aligned");
    return HE_OK;
}

ha_status check_heads_fwd(int64_t n, const ha_ppo_heads_weights* w, const ha_ppo_heads_fwd* io, uintptr_t m16, uintptr_t m8) {
    if (!io) return check_heads(n, w, nullptr, m16, m8, nullptr, 0, nullptr, 0, nullptr, 0);
    const void* p16[] = {io->h_pi, io->h_vf, io->a1_pi, io->a2_pi, io->a1_vf, io->a2_vf};
    const void* p8[] = {io->actions, io->mean};
    const void* p4[] = {io->values, io->log_prob, io->entropy};
    return check_heads(n, w, io, m16, m8, p16, 6, p8, 2, p4, 3);
}

ha_status check_heads_bwd(int64_t n, const ha_ppo_heads_weights* w, const ha_ppo_heads_bwd* io, uintptr_t m16, uintptr_t m8) {
    if (!io) return check_heads(n, w, nullptr, m16, m8, nullptr, 0, nullptr, 0, nullptr, 0);
    const void* p16[] = {io->a1_pi, io->a2_pi, io->a1_vf, io->a2_vf, io->d_h_pi, io->d_h_vf,
                         io->d_z1_pi, io->d_z2_pi, io->d_z1_vf, io->d_z2_vf};
    const void* p8[] = {io->actions, io->mean, io->d_mean};
    const void* p4[] = {io->d_values, io->d_log_prob, io->d_entropy, io->d_log_std};
    return check_heads(n, w, io, m16, m8, p16, 10, p8, 3, p4, 4);
}

ha_status heads_pack(const ha_ppo_heads_weights* w, void* workspace, void* stream) {
    HeadsPackParams pp;
    pp.w1[0] = w->w1, pp.w1[1] = w->v1, pp.w2[0] = w->w2, pp.w2[1] = w->v2;
    pp.log_std = w->log_std;
    pp.ws = (float*)workspace;
    return launch(nullptr, heads_pack_kernel, dim3(24, 2), dim3(256), stream, "heads_pack_kernel", pp);
}

// H1 for one network and row on the host: the two layers into a1, a2
void host_heads_mlp(const HeadsNetW& w, const float* h, bool relu, float* a1, float* a2) {
    for (int j = 0; j < kMlp; ++j) {
        float acc = w.b1[j];
        for (int k = 0; k < kHid; ++k) acc = fmaf(w.w1[j * kHid + k], h[k], acc);
        a1[j] = mlp_act(acc, relu);
    }
    for (int j = 0; j < kMlp; ++j) {
        float acc = w.b2[j];
        for (int k = 0; k < kMlp; ++k) acc = fmaf(w.w2[j * kMlp + k], a1[k], acc);
        a2[j] = mlp_act(acc, relu);
    }
}

// H5 for one network and row on the host, from the head's gradient d_out[n_out]
void host_heads_mlp_bwd(const HeadsNetW& w, const float* d_out, const float* a1, const float* a2, bool relu, float* d_z1,
                        float* d_z2, float* d_h) {
    for (int k = 0; k < kMlp; ++k) {
        float s = 0.0f;
        for (int j = 0; j < w.n_out; ++j) s = fmaf(d_out[j], w.w3[j * kMlp + k], s);
        d_z2[k] = act_backward(s, a2[k], relu);
    }
    for (int k = 0; k < kMlp; ++k) {
        float s = 0.0f;
        for (int u = 0; u < kMlp; ++u) s = fmaf(d_z2[u], w.w2[u * kMlp + k], s);
        d_z1[k] = act_backward(s, a1[k], relu);
    }
    for (int k = 0; k < kHid; ++k) {
        float s = 0.0f;
        for (int u = 0; u < kMlp; ++u) s = fmaf(d_z1[u], w.w1[u * kHid + k], s);
        d_h[k] = s;
    }
}

}  // namespace

extern "C" {

const char* ha_version(void) { return "libhedgeactor 1 (gfx950, v_mfma_f32_32x32x2_f32)"; }

const char* ha_last_error(const ha_actor* actor) { return actor ? actor->err : g_err; }

const char* ha_policy_last_error(const ha_policy* policy) { return policy ? policy->err : g_err; }

ha_status ha_create(const ha_weights* w, ha_actor** out) {
    if (!out) return fail_to(nullptr, HE_EINVAL, "out is NULL");
    *out = nullptr;
    ha_status st = check_weights(w, nullptr);
    if (st != HE_OK) return st;
    const size_t o_st = kNetFloats;   // stats: doubles, 8-byte aligned (o_st even)
    const size_t total = o_st + kStatFloats;
    std::vector<float> hbuf(total, 0.0f);
    pack_net(actor_net(w), hbuf.data());
    if (w->obs_mean) pack_stats(w->obs_mean, w->obs_var, w->epsilon, &hbuf[o_st]);
    st = create_handle(hbuf, out);
    if (st != HE_OK) return st;
    const float* d = (const float*)(*out)->blob;
    Params& p = (*out)->p;
    memset(&p, 0, sizeof p);
    p.net = net_at(d);
    p.stats = w->obs_mean ? (const double*)(d + o_st) : nullptr;
    p.clip = w->clip_obs;
    p.has_clip = w->has_clip;
    p.relu = w->activation == HA_ACT_RELU;
    p.tanh_squash = w->squash == HA_SQUASH_TANH;
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
    return launch(actor->err, actor_kernel, dim3(grid), dim3(kThreads), stream, "actor_kernel", p);
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
    return launch(actor->err, accumulate_kernel, dim3(grid), dim3(256), stream, "accumulate_kernel", n, env_id_offset, in,
                  terminated, sums, records, capacity, count);
}

ha_status ha_host_step(const ha_weights* w, int64_t n, const float* obs, const uint8_t* episode_start, float* h,
                       float* c, float* actions, float* mean_out, float* obs_norm_out) {
    ha_status st = check_weights(w, nullptr);
    if (st != HE_OK) return st;
    if (n < 1 || !obs || !episode_start || !h || !c || !actions)
        return fail_to(nullptr, HE_EINVAL, "bad argument");
    const HostNorm norm(w->obs_mean, w->obs_var, w->epsilon, w->has_clip != 0, w->clip_obs);
    const bool relu = w->activation == HA_ACT_RELU, tsq = w->squash == HA_SQUASH_TANH;
    const HostNet net = actor_net(w);
    for (int64_t e = 0; e < n; ++e) {
        float x[kObs], a2[kMlp];
        norm.env(obs, e, x, obs_norm_out);
        host_net_env(net, x, episode_start[e] != 0, h + e * kHid, c + e * kHid, true, relu, a2);
        for (int j = 0; j < kAct; ++j) {
            const float m = host_head(net, j, a2);
            if (mean_out) mean_out[e * kAct + j] = m;
            actions[e * kAct + j] = squash_action(m, tsq);
        }
    }
    return HE_OK;
}

ha_status ha_policy_create(const ha_policy_weights* w, ha_policy** out) {
    if (!out) return fail_to(nullptr, HE_EINVAL, "out is NULL");
    *out = nullptr;
    ha_status st = check_policy_weights(w, nullptr);
    if (st != HE_OK) return st;
    std::vector<float> hbuf(kPolicyFloats + kSnapFloats, 0.0f);   // the tail: ha_policy_refresh's copy of the tensors
    pack_policy(w, hbuf.data());
    st = create_handle(hbuf, out);
    if (st == HE_OK) policy_params(w, (const float*)(*out)->blob, &(*out)->p);
    return st;
}

ha_status ha_policy_destroy(ha_policy* policy) {
    if (!policy) return HE_EINVAL;
    if (policy->blob) (void)hipFree(policy->blob);
    delete policy;
    return HE_OK;
}

ha_status ha_policy_update(ha_policy* policy, const ha_policy_weights* w) {
    if (!policy) return HE_EINVAL;
    ha_status st = check_policy_weights(w, policy);
    if (st != HE_OK) return st;
    std::vector<float> hbuf(kPolicyFloats, 0.0f);
    pack_policy(w, hbuf.data());
    // steps already enqueued read the old tensors to their end
    if (hipDeviceSynchronize() != hipSuccess) return fail(policy, HE_EHIP, "hipDeviceSynchronize failed");
    st = upload_blob(hbuf, &policy->blob, policy->err);
    if (st == HE_OK) policy_params(w, (const float*)policy->blob, &policy->p);
    policy->refreshed = false;
    return st;
}

ha_status ha_policy_refresh(ha_policy* policy, const ha_policy_weights* w_dev, void* stream) {
    if (!policy) return HE_EINVAL;
    ha_policy_weights w;   // the statistics are the handle's: the pointers of w_dev are not looked at
    if (w_dev) {
        w = *w_dev;
        w.obs_mean = w.obs_var = nullptr;
    }
    ha_status st = check_policy_weights(w_dev ? &w : nullptr, policy);
    if (st != HE_OK) return st;
    PolicyPackParams p;
    const float* t[kPolicyTensors] = {w.w_ih,   w.w_hh,   w.b_ih,   w.b_hh,   w.w1, w.b1,  w.w2, w.b2,  w.w3, w.b3, w.log_std,
                                      w.c_w_ih, w.c_w_hh, w.c_b_ih, w.c_b_hh, w.v1, w.vb1, w.v2, w.vb2, w.v3, w.vb3};
    p.off[0] = 0;
    for (int k = 0; k < kPolicyTensors; ++k) {
        if (((uintptr_t)t[k]) & 3u) return fail(policy, HE_EINVAL, "the tensors must be 4-byte aligned");
        p.t[k] = t[k];
        p.off[k + 1] = p.off[k] + kTensorFloats[k];
    }
    p.blob = (float*)policy->blob;
    p.snap = p.blob + kPolicyFloats;
    st = launch(policy->err, policy_pack_kernel, dim3(512), dim3(256), stream, "policy_pack_kernel", p);
    if (st == HE_OK) policy->refreshed = true;
    return st;
}

ha_status ha_policy_download(ha_policy* policy, float* out, void* stream) {
    if (!policy) return HE_EINVAL;
    if (!out) return fail(policy, HE_EINVAL, "out is NULL");
    if (!policy->refreshed)
        return fail(policy, HE_ESTATE, "no ha_policy_refresh since the handle's tensors last came from the host");
    if (hipMemcpyAsync(out, (const float*)policy->blob + kPolicyFloats, kSnapFloats * sizeof(float),
                       hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return fail(policy, HE_EHIP, "download of the refreshed tensors failed");
    return HE_OK;
}

ha_status ha_policy_step(ha_policy* policy, int64_t n, int64_t env_id_offset, uint64_t seed, uint64_t step_index,
                         int32_t deterministic, int32_t write_state, const float* obs, const uint8_t* episode_start,
                         float* h_pi, float* c_pi, float* h_vf, float* c_vf, float* actions, float* env_actions,
                         float* values, float* log_probs, float* mean_out, float* obs_norm_out, void* stream) {
    if (!policy) return HE_EINVAL;
    if (n < 1 || n > ((int64_t)1 << 30)) return fail(policy, HE_EINVAL, "n must be in [1, 2^30]");
    if (env_id_offset < 0) return fail(policy, HE_EINVAL, "env_id_offset must be >= 0");
    if (!obs || !episode_start || !h_pi || !c_pi || !h_vf || !c_vf || !actions || !env_actions || !values || !log_probs)
        return fail(policy, HE_EINVAL, "a required buffer is NULL");
    if ((((uintptr_t)h_pi) | ((uintptr_t)c_pi) | ((uintptr_t)h_vf) | ((uintptr_t)c_vf)) & 15u)
        return fail(policy, HE_EINVAL, "the LSTM states must be 16-byte aligned");
    if ((((uintptr_t)actions) | ((uintptr_t)env_actions) | ((uintptr_t)mean_out)) & 7u)
        return fail(policy, HE_EINVAL, "actions, env_actions and mean_out must be 8-byte aligned");
    PolicyParams p = policy->p;
    p.n = n;
    p.goff = env_id_offset;
    p.seed = seed;
    p.step_index = step_index;
    p.deterministic = deterministic != 0;
    p.write_state = write_state != 0;
    p.obs = obs;
    p.start = episode_start;
    p.h_pi = h_pi;
    p.c_pi = c_pi;
    p.h_vf = h_vf;
    p.c_vf = c_vf;
    p.actions = actions;
    p.env_actions = env_actions;
    p.values = values;
    p.log_probs = log_probs;
    p.mean_out = mean_out;
    p.obs_norm_out = obs_norm_out;
    const unsigned grid = (unsigned)((n + kTile - 1) / kTile);
    return launch(policy->err, policy_step_kernel, dim3(grid, 2), dim3(kThreads), stream, "policy_step_kernel", p);
}

ha_status ha_gae(int64_t n, int64_t K, double gamma, double gae_lambda, const float* rewards, const float* values,
                 const uint8_t* episode_starts, const float* last_values, const uint8_t* last_dones,
                 float* advantages, float* returns, void* stream) {
    ha_status st = check_gae(n, K, gamma, gae_lambda, rewards, values, episode_starts, last_values, last_dones,
                             advantages, returns);
    if (st != HE_OK) return st;
    if (n > ((int64_t)1 << 30)) return fail_to(nullptr, HE_EINVAL, "n must be <= 2^30");
    const unsigned grid = (unsigned)((n + 255) / 256);
    return launch(nullptr, gae_kernel, dim3(grid), dim3(256), stream, "gae_kernel", n, K, (float)gamma,
                  (float)(gamma * gae_lambda), rewards, values, episode_starts, last_values, last_dones, advantages,
                  returns);
}

ha_status ha_host_policy_step(const ha_policy_weights* w, int64_t n, int64_t env_id_offset, uint64_t seed,
                              uint64_t step_index, int32_t deterministic, int32_t write_state, const float* obs,
                              const uint8_t* episode_start, float* h_pi, float* c_pi, float* h_vf, float* c_vf,
                              float* actions, float* env_actions, float* values, float* log_probs, float* mean_out,
                              float* obs_norm_out) {
    ha_status st = check_policy_weights(w, nullptr);
    if (st != HE_OK) return st;
    if (n < 1 || env_id_offset < 0 || !obs || !episode_start || !h_pi || !c_pi || !h_vf || !c_vf || !actions ||
        !env_actions || !values || !log_probs)
        return fail_to(nullptr, HE_EINVAL, "bad argument");
    const HostNorm norm(w->obs_mean, w->obs_var, w->epsilon, w->has_clip != 0, w->clip_obs);
    const bool relu = w->activation == HA_ACT_RELU;
    const HostNet pi = actor_net(w), vf = critic_net(w);
    const float stdv[kAct] = {policy_std(w->log_std[0]), policy_std(w->log_std[1])};
    for (int64_t e = 0; e < n; ++e) {
        float x[kObs], a2[kMlp], mean[kAct];
        norm.env(obs, e, x, obs_norm_out);
        const bool fresh = episode_start[e] != 0;
        host_net_env(pi, x, fresh, h_pi + e * kHid, c_pi + e * kHid, write_state != 0, relu, a2);
        for (int j = 0; j < kAct; ++j) {
            mean[j] = host_head(pi, j, a2);
            if (mean_out) mean_out[e * kAct + j] = mean[j];
        }
        host_net_env(vf, x, fresh, h_vf + e * kHid, c_vf + e * kHid, write_state != 0, relu, a2);
        values[e] = host_head(vf, 0, a2);
        sample_action(mean, w->log_std, stdv, seed, step_index, (uint64_t)(env_id_offset + e), deterministic != 0,
                      actions + e * kAct, env_actions + e * kAct, log_probs + e);
    }
    return HE_OK;
}

ha_status ha_host_gae(int64_t n, int64_t K, double gamma, double gae_lambda, const float* rewards,
                      const float* values, const uint8_t* episode_starts, const float* last_values,
                      const uint8_t* last_dones, float* advantages, float* returns) {
    ha_status st = check_gae(n, K, gamma, gae_lambda, rewards, values, episode_starts, last_values, last_dones,
                             advantages, returns);
    if (st != HE_OK) return st;
    const float g32 = (float)gamma, gl32 = (float)(gamma * gae_lambda);
    for (int64_t e = 0; e < n; ++e)
        gae_env(e, n, K, g32, gl32, rewards, values, episode_starts, last_values, last_dones, advantages, returns);
    return HE_OK;
}

size_t ha_lstm_seq_workspace_bytes(int64_t n_nets) {
    return (n_nets == 1 || n_nets == 2) ? (size_t)n_nets * kSeqNetFloats * sizeof(float) : 0;
}

ha_status ha_lstm_seq_forward(int64_t n_nets, int64_t L, int64_t B, const float* x, const uint8_t* episode_starts,
                              const ha_lstm_seq_net* nets, void* workspace, void* stream) {
    ha_status st = check_seq_fwd(n_nets, L, B, x, episode_starts, nets, 15u);
    if (st == HE_OK) st = check_workspace(workspace);
    if (st != HE_OK) return st;
    SeqPackParams pk = {};
    SeqFwdParams p = {};
    for (int64_t k = 0; k < n_nets; ++k) {
        pk.w_ih[k] = nets[k].w_ih;
        pk.w_hh[k] = nets[k].w_hh;
        pk.b_ih[k] = nets[k].b_ih;
        pk.b_hh[k] = nets[k].b_hh;
        p.net[k] = nets[k];
    }
    pk.ws = (float*)workspace;
    p.L = L;
    p.B = B;
    p.x = x;
    p.start = episode_starts;
    p.ws = (const float*)workspace;
    st = launch(nullptr, lstm_seq_pack_fwd_kernel, dim3(72, (unsigned)n_nets), dim3(256), stream,
                "lstm_seq_pack_fwd_kernel", pk);
    if (st != HE_OK) return st;
    const unsigned grid = (unsigned)((B + kTile - 1) / kTile);
    return launch(nullptr, lstm_seq_fwd_kernel, dim3(grid, (unsigned)n_nets), dim3(kThreads), stream,
                  "lstm_seq_fwd_kernel", p);
}

ha_status ha_lstm_seq_backward(int64_t n_nets, int64_t L, int64_t B, const uint8_t* episode_starts,
                               const ha_lstm_seq_bwd* nets, void* workspace, void* stream) {
    ha_status st = check_seq_bwd(n_nets, L, B, episode_starts, nets, 15u);
    if (st == HE_OK) st = check_workspace(workspace);
    if (st != HE_OK) return st;
    SeqPackParams pk = {};
    SeqBwdParams p = {};
    for (int64_t k = 0; k < n_nets; ++k) {
        pk.w_hh[k] = nets[k].w_hh;
        p.net[k] = nets[k];
    }
    pk.ws = (float*)workspace;
    p.L = L;
    p.B = B;
    p.start = episode_starts;
    p.ws = (const float*)workspace;
    st = launch(nullptr, lstm_seq_pack_bwd_kernel, dim3(64, (unsigned)n_nets), dim3(256), stream,
                "lstm_seq_pack_bwd_kernel", pk);
    if (st != HE_OK) return st;
    const unsigned grid = (unsigned)((B + kTile - 1) / kTile);
    return launch(nullptr, lstm_seq_bwd_kernel, dim3(grid, (unsigned)n_nets), dim3(kThreads), stream,
                  "lstm_seq_bwd_kernel", p);
}

ha_status ha_host_lstm_seq_forward(int64_t n_nets, int64_t L, int64_t B, const float* x,
                                   const uint8_t* episode_starts, const ha_lstm_seq_net* nets) {
    const ha_status st = check_seq_fwd(n_nets, L, B, x, episode_starts, nets, 0u);
    if (st != HE_OK) return st;
    for (int64_t k = 0; k < n_nets; ++k) {
        const ha_lstm_seq_net& n = nets[k];
        const HostNet w = {n.w_ih, n.w_hh, n.b_ih, n.b_hh, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
        for (int64_t e = 0; e < B; ++e) {
            float h[kHid], c[kHid], hn[kHid], xh[kKp];
            memcpy(h, n.h0 + e * kHid, sizeof h);
            memcpy(c, n.c0 + e * kHid, sizeof c);
            for (int64_t t = 0; t < L; ++t) {
                const int64_t row = t * B + e;
                const bool fresh = episode_starts[row] != 0;
                host_xh(x + row * kObs, h, fresh, xh);
                for (int u = 0; u < kHid; ++u) {
                    float pre[4], gt[4];
                    host_gates(w, xh, u, pre);
                    float cv = fresh ? 0.0f : c[u];
                    hn[u] = cell_forward(pre[0], pre[1], pre[2], pre[3], &cv, gt);
                    c[u] = cv;
                    for (int g = 0; g < 4; ++g) n.gates[(row * 4 + g) * kHid + u] = gt[g];
                }
                memcpy(h, hn, sizeof h);
                memcpy(n.h + row * kHid, h, sizeof h);
                memcpy(n.c + row * kHid, c, sizeof c);
            }
        }
    }
    return HE_OK;
}

ha_status ha_host_lstm_seq_backward(int64_t n_nets, int64_t L, int64_t B, const uint8_t* episode_starts,
                                    const ha_lstm_seq_bwd* nets) {
    const ha_status st = check_seq_bwd(n_nets, L, B, episode_starts, nets, 0u);
    if (st != HE_OK) return st;
    std::vector<float> dgv(kGates);
    float* dg = dgv.data();
    for (int64_t k = 0; k < n_nets; ++k) {
        const ha_lstm_seq_bwd& n = nets[k];
        for (int64_t e = 0; e < B; ++e) {
            float dc[kHid], dhr[kHid];
            for (int u = 0; u < kHid; ++u) dc[u] = dhr[u] = 0.0f;
            for (int64_t t = L - 1; t >= 0; --t) {
                const int64_t row = t * B + e;
                const bool fresh = episode_starts[row] != 0;
                const float* cp = t > 0 ? n.c + (row - B) * kHid : n.c0 + e * kHid;
                const float* gt = n.gates + row * 4 * kHid;
                for (int u = 0; u < kHid; ++u) {
                    const float dh = n.d_h[row * kHid + u] + dhr[u];
                    float d[4];
                    const float dcn = cell_backward(gt[u], gt[kHid + u], gt[2 * kHid + u], gt[3 * kHid + u],
                                                    n.c[row * kHid + u], fresh ? 0.0f : cp[u], dh, dc[u], d);
                    dc[u] = fresh ? 0.0f : dcn;
                    for (int g = 0; g < 4; ++g) dg[g * kHid + u] = d[g];
                }
                memcpy(n.d_gates + row * 4 * kHid, dg, kGates * sizeof(float));
                if (t == 0) break;
                for (int j = 0; j < kHid; ++j) {
                    float acc = 0.0f;
                    for (int u = 0; u < kGates; ++u) acc = fmaf(dg[u], n.w_hh[u * kHid + j], acc);
                    dhr[j] = fresh ? 0.0f : acc;
                }
            }
        }
    }
    return HE_OK;
}

size_t ha_lstm_seq_weight_grads_workspace_bytes(int64_t n_nets, int64_t L, int64_t B) {
    if ((n_nets != 1 && n_nets != 2) || L < 1 || B < 1 || L > ((int64_t)1 << 30) || B > ((int64_t)1 << 30)) return 0;
    const int64_t chunks = wgrad_chunks(L, B);
    return chunks > 0x7fffffffll ? 0 : (size_t)n_nets * (size_t)chunks * kWgPartial * sizeof(double);
}

ha_status ha_lstm_seq_weight_grads(int64_t n_nets, int64_t L, int64_t B, const float* x,
                                   const uint8_t* episode_starts, const ha_lstm_seq_wgrad* nets, void* workspace,
                                   void* stream) {
    ha_status st = check_wgrad(n_nets, L, B, x, episode_starts, nets, 15u);
    if (st == HE_OK) st = check_workspace(workspace);
    if (st != HE_OK) return st;
    WgradParams p = {};
    for (int64_t k = 0; k < n_nets; ++k) p.net[k] = nets[k];
    p.R = L * B;
    p.B = B;
    p.n_chunks = wgrad_chunks(L, B);
    p.x = x;
    p.start = episode_starts;
    p.ws = (double*)workspace;
    st = launch(nullptr, lstm_wgrad_kernel, dim3((unsigned)p.n_chunks, kGates / kHid, (unsigned)n_nets), dim3(kThreads),
                stream, "lstm_wgrad_kernel", p);
    if (st != HE_OK) return st;
    return launch(nullptr, lstm_wgrad_reduce_kernel, dim3((unsigned)((kWgPartial + 255) / 256), (unsigned)n_nets),
                  dim3(256), stream, "lstm_wgrad_reduce_kernel", p);
}

ha_status ha_host_lstm_seq_weight_grads(int64_t n_nets, int64_t L, int64_t B, const float* x,
                                        const uint8_t* episode_starts, const ha_lstm_seq_wgrad* nets) {
    ha_status st = check_wgrad(n_nets, L, B, x, episode_starts, nets, 0u);
    if (st != HE_OK) return st;
    const int64_t R = L * B, chunks = wgrad_chunks(L, B);
    std::vector<float> sv(kWgPartial);
    std::vector<double> pv(kWgPartial), tv(kWgPartial);
    float* s = sv.data();
    const float zeros[kGates] = {0.0f};
    for (int64_t k = 0; k < n_nets; ++k) {
        const ha_lstm_seq_wgrad& n = nets[k];
        for (size_t i = 0; i < kWgPartial; ++i) tv[i] = 0.0;
        for (int64_t c = 0; c < chunks; ++c) {
            for (size_t i = 0; i < kWgPartial; ++i) pv[i] = 0.0;
            const int64_t c0 = c * kWgChunkRows, c1 = c0 + kWgChunkRows < R ? c0 + kWgChunkRows : R;
            for (int64_t b0 = c0; b0 < c1; b0 += HA_WGRAD_BLOCK) {
                for (size_t i = 0; i < kWgPartial; ++i) s[i] = 0.0f;
                for (int64_t r = b0; r < b0 + HA_WGRAD_BLOCK; ++r) {   // W1, the padding terms included
                    float z[kKp];
                    if (r < R) {
                        const bool fresh = episode_starts[r] != 0;
                        const float* hp = r >= B ? n.h + (r - B) * kHid : n.h0 + r * kHid;
                        for (int i = 0; i < kObs; ++i) z[i] = x[r * kObs + i];
                        for (int u = 0; u < kHid; ++u) z[kObs + u] = fresh ? 0.0f : hp[u];
                        z[kKx] = 1.0f;
                    } else {
                        for (int i = 0; i < kKp; ++i) z[i] = 0.0f;
                    }
                    wgrad_row(r < R ? n.d_gates + r * kGates : zeros, z, s);
                }
                for (size_t i = 0; i < kWgPartial; ++i) pv[i] += (double)s[i];   // W2
            }
            for (size_t i = 0; i < kWgPartial; ++i) tv[i] += pv[i];   // W3
        }
        for (int u = 0; u < kGates; ++u) {   // W4
            for (int i = 0; i < kObs; ++i) n.d_w_ih[u * kObs + i] = (float)tv[(size_t)u * kKp + i];
            for (int j = 0; j < kHid; ++j) n.d_w_hh[u * kHid + j] = (float)tv[(size_t)u * kKp + kObs + j];
            n.d_b[u] = (float)tv[(size_t)u * kKp + kKx];
        }
    }
    return HE_OK;
}

size_t ha_adam_workspace_bytes(int64_t n_tensors, const ha_adam_tensor* tensors) {
    int32_t first[HA_OPT_MAX_TENSORS + 1];
    if (check_adam(n_tensors, tensors, nullptr, first, nullptr) != HE_OK) return 0;
    return (size_t)first[n_tensors] * sizeof(double);
}

ha_status ha_adam_step(int64_t n_tensors, const ha_adam_tensor* tensors, const ha_adam_hyper* hyper, void* workspace,
                       void* stream) {
    AdamParams p;
    ha_status st = check_adam(n_tensors, tensors, hyper, p.first, &p.k);
    if (st != HE_OK) return st;
    if (!workspace || (((uintptr_t)workspace) & 7u))
        return fail_to(nullptr, HE_EINVAL, "workspace must be non-NULL and 8-byte aligned");
    uintptr_t bits = (uintptr_t)hyper->grad_norm_out;
    for (int64_t j = 0; j < n_tensors; ++j) {
        p.t[j] = tensors[j];
        bits |= (uintptr_t)tensors[j].param | (uintptr_t)tensors[j].grad | (uintptr_t)tensors[j].exp_avg |
                (uintptr_t)tensors[j].exp_avg_sq;
    }
    if (bits & 3u) return fail_to(nullptr, HE_EINVAL, "the tensors and grad_norm_out must be 4-byte aligned");
    for (int64_t j = n_tensors; j < HA_OPT_MAX_TENSORS; ++j) {
        p.t[j] = ha_adam_tensor{nullptr, nullptr, nullptr, nullptr, 0};
        p.first[j + 1] = p.first[n_tensors];
    }
    p.n = (int32_t)n_tensors;
    p.partial = (double*)workspace;
    p.norm_out = hyper->grad_norm_out;
    const dim3 grid((unsigned)p.first[n_tensors]), block(HA_OPT_BLOCK);
    st = launch(nullptr, opt_norm_kernel, grid, block, stream, "opt_norm_kernel", p);
    if (st != HE_OK) return st;
    return launch(nullptr, opt_adam_kernel, grid, block, stream, "opt_adam_kernel", p);
}

ha_status ha_host_adam_step(int64_t n_tensors, const ha_adam_tensor* tensors, const ha_adam_hyper* hyper) {
    int32_t first[HA_OPT_MAX_TENSORS + 1];
    AdamConsts k;
    const ha_status st = check_adam(n_tensors, tensors, hyper, first, &k);
    if (st != HE_OK) return st;
    double total = 0.0;   // O1, O2
    for (int64_t j = 0; j < n_tensors; ++j)
        for (int64_t i0 = 0; i0 < tensors[j].numel; i0 += HA_OPT_BLOCK) {
            double q[HA_OPT_BLOCK];
            for (int i = 0; i < HA_OPT_BLOCK; ++i) {
                const float g = i0 + i < tensors[j].numel ? tensors[j].grad[i0 + i] : 0.0f;
                q[i] = (double)g * (double)g;
            }
            for (int off = HA_OPT_BLOCK / 2; off >= 1; off >>= 1)
                for (int i = 0; i < off; ++i) q[i] = q[i] + q[i + off];
            total = total + q[0];
        }
    float norm;   // O3, O4
    const float c = adam_clip(total, k, &norm);
    if (hyper->grad_norm_out) *hyper->grad_norm_out = norm;
    for (int64_t j = 0; j < n_tensors; ++j) {   // O5
        const ha_adam_tensor& t = tensors[j];
        for (int64_t i = 0; i < t.numel; ++i) adam_element(t.grad[i], c, k, t.param + i, t.exp_avg + i, t.exp_avg_sq + i);
    }
    return HE_OK;
}

size_t ha_ppo_loss_workspace_bytes(int64_t n_rows) {
    if (check_loss(n_rows, nullptr, nullptr, nullptr) != HE_OK) return 0;
    return (size_t)((n_rows - 1) / HA_LOSS_BLOCK + 1) * kLossLists * sizeof(double);
}

ha_status ha_ppo_loss(int64_t n_rows, const ha_ppo_loss_io* io, const ha_ppo_loss_hyper* hyper, void* workspace,
                      void* stream) {
    LossParams p;
    ha_status st = check_loss(n_rows, io, hyper, &p.k);
    if (st != HE_OK) return st;
    if (!workspace || (((uintptr_t)workspace) & 7u))
        return fail_to(nullptr, HE_EINVAL, "workspace must be non-NULL and 8-byte aligned");
    p.io = *io;
    p.n = n_rows;
    p.nb = (int32_t)((n_rows - 1) / HA_LOSS_BLOCK + 1);
    p.ws = (double*)workspace;
    const dim3 grid((unsigned)p.nb), block(kLossLanes);
    if (p.k.normalize) {
        st = launch(nullptr, loss_mean_kernel, grid, block, stream, "loss_mean_kernel", p);
        if (st != HE_OK) return st;
        st = launch(nullptr, loss_spread_kernel, grid, block, stream, "loss_spread_kernel", p);
        if (st != HE_OK) return st;
    }
    st = launch(nullptr, loss_rows_kernel, grid, block, stream, "loss_rows_kernel", p);
    if (st != HE_OK) return st;
    return launch(nullptr, loss_stats_kernel, dim3(1), block, stream, "loss_stats_kernel", p);
}

ha_status ha_host_ppo_loss(int64_t n_rows, const ha_ppo_loss_io* io, const ha_ppo_loss_hyper* hyper) {
    LossConsts k;
    const ha_status st = check_loss(n_rows, io, hyper, &k);
    if (st != HE_OK) return st;
    std::vector<LossTerms> t;
    try {
        t.resize((size_t)n_rows);
    } catch (const std::bad_alloc&) {
        return fail_to(nullptr, HE_ENOMEM, "out of host memory");
    }
    double mean = 0.0, sd = 1.0, den = 1.0;
    if (k.normalize) {   // L2, L3
        const float* adv = io->advantages;
        mean = loss_sum_host(n_rows, [&](int64_t r) { return (double)adv[r]; }) / k.n;
        const double ssq = loss_sum_host(n_rows, [&](int64_t r) {
            const double dev = (double)adv[r] - mean;
            return dev * dev;
        });
        sd = loss_std(ssq, k.n);
        den = sd + 1e-8;
    }
    const double ge = -k.ent_coef;
    const float d_ent = (float)(ge / k.n);
    for (int64_t r = 0; r < n_rows; ++r) {   // L4, L6
        t[(size_t)r] = loss_row(io->values[r], io->log_prob[r], io->entropy[r], io->old_log_prob[r], io->advantages[r],
                                io->returns[r], k.clip_vf ? io->old_values[r] : 0.0f, mean, den, k, io->d_values + r,
                                io->d_log_prob + r);
        io->d_entropy[r] = d_ent;
    }
    const double tot[5] = {loss_sum_host(n_rows, [&](int64_t r) { return t[(size_t)r].pol; }),
                           loss_sum_host(n_rows, [&](int64_t r) { return t[(size_t)r].val; }),
                           loss_sum_host(n_rows, [&](int64_t r) { return t[(size_t)r].ent; }),
                           loss_sum_host(n_rows, [&](int64_t r) { return t[(size_t)r].kl; }),
                           loss_sum_host(n_rows, [&](int64_t r) { return t[(size_t)r].clipped; })};
    loss_stats(tot, k.normalize ? mean : 0.0, sd, k, io->stats);   // L5
    return HE_OK;
}

size_t ha_ppo_heads_workspace_bytes(int64_t n_rows) {
    if (check_heads_rows(n_rows) != HE_OK) return 0;
    return kHpart * sizeof(float) + (size_t)((n_rows - 1) / HA_LOSS_BLOCK + 1) * kAct * sizeof(double);
}

ha_status ha_ppo_heads_forward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_fwd* io,
                               void* workspace, void* stream) {
    ha_status st = check_heads_fwd(n_rows, weights, io, 15u, 7u);
    if (st != HE_OK) return st;
    st = check_workspace(workspace);
    if (st != HE_OK) return st;
    st = heads_pack(weights, workspace, stream);
    if (st != HE_OK) return st;
    HeadsFwdParams p;
    p.n = n_rows;
    p.relu = weights->activation == HA_ACT_RELU;
    p.io = *io;
    p.net[0] = heads_net(weights, false);
    p.net[1] = heads_net(weights, true);
    p.ws = (const float*)workspace;
    // enough workgroups to fill the device twice over, then up to a block's tiles each
    const int64_t ntiles = (n_rows - 1) / kHRows + 1;
    const int64_t per = ntiles / 512;
    p.tiles_per_wg = (int32_t)(per < 1 ? 1 : (per > kHTiles ? kHTiles : per));
    const dim3 grid((unsigned)((ntiles - 1) / p.tiles_per_wg + 1), 2);
    return launch(nullptr, heads_fwd_kernel, grid, dim3(kThreads), stream, "heads_fwd_kernel", p);
}

ha_status ha_ppo_heads_backward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_bwd* io,
                                void* workspace, void* stream) {
    ha_status st = check_heads_bwd(n_rows, weights, io, 15u, 7u);
    if (st != HE_OK) return st;
    st = check_workspace(workspace);
    if (st != HE_OK) return st;
    st = heads_pack(weights, workspace, stream);
    if (st != HE_OK) return st;
    HeadsBwdParams p;
    p.n = n_rows;
    p.relu = weights->activation == HA_ACT_RELU;
    p.nb = (int32_t)((n_rows - 1) / HA_LOSS_BLOCK + 1);
    p.io = *io;
    p.net[0] = heads_net(weights, false);
    p.net[1] = heads_net(weights, true);
    p.ws = (const float*)workspace;
    p.part = (double*)((float*)workspace + kHpart);
    st = launch(nullptr, heads_bwd_kernel, dim3((unsigned)p.nb, 2), dim3(kThreads), stream, "heads_bwd_kernel", p);
    if (st != HE_OK) return st;
    return launch(nullptr, heads_lsd_kernel, dim3(1), dim3(kLossLanes), stream, "heads_lsd_kernel", (const double*)p.part,
                  (int)p.nb, io->d_log_std);
}

ha_status ha_host_ppo_heads_forward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_fwd* io) {
    const ha_status st = check_heads_fwd(n_rows, weights, io, 3u, 3u);
    if (st != HE_OK) return st;
    const bool relu = weights->activation == HA_ACT_RELU;
    const HeadsNetW pi = heads_net(weights, false), vf = heads_net(weights, true);
    const float* ls = weights->log_std;
    const float stdv[kAct] = {policy_std(ls[0]), policy_std(ls[1])};
    const float ent = heads_entropy(ls);
    for (int64_t r = 0; r < n_rows; ++r) {
        float* a2 = io->a2_pi + r * kMlp;
        host_heads_mlp(pi, io->h_pi + r * kHid, relu, io->a1_pi + r * kMlp, a2);
        float mean[kAct];
        for (int j = 0; j < kAct; ++j) {
            float m = pi.b3[j];
            for (int k = 0; k < kMlp; ++k) m = fmaf(pi.w3[j * kMlp + k], a2[k], m);
            mean[j] = io->mean[r * kAct + j] = m;
        }
        io->log_prob[r] = heads_log_prob(io->actions + r * kAct, mean, ls, stdv);
        io->entropy[r] = ent;
        a2 = io->a2_vf + r * kMlp;
        host_heads_mlp(vf, io->h_vf + r * kHid, relu, io->a1_vf + r * kMlp, a2);
        float v = vf.b3[0];
        for (int k = 0; k < kMlp; ++k) v = fmaf(vf.w3[k], a2[k], v);
        io->values[r] = v;
    }
    return HE_OK;
}

ha_status ha_host_ppo_heads_backward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_bwd* io) {
    const ha_status st = check_heads_bwd(n_rows, weights, io, 3u, 3u);
    if (st != HE_OK) return st;
    const bool relu = weights->activation == HA_ACT_RELU;
    const HeadsNetW pi = heads_net(weights, false), vf = heads_net(weights, true);
    const float* ls = weights->log_std;
    const float stdv[kAct] = {policy_std(ls[0]), policy_std(ls[1])};
    for (int64_t r = 0; r < n_rows; ++r) {   // H4, H5
        float d_mean[kAct];
        for (int j = 0; j < kAct; ++j) {
            const double z = gauss_z(io->actions[r * kAct + j], io->mean[r * kAct + j], stdv[j]);
            d_mean[j] = io->d_mean[r * kAct + j] = heads_d_mean(io->d_log_prob[r], z, stdv[j]);
        }
        host_heads_mlp_bwd(pi, d_mean, io->a1_pi + r * kMlp, io->a2_pi + r * kMlp, relu, io->d_z1_pi + r * kMlp,
                           io->d_z2_pi + r * kMlp, io->d_h_pi + r * kHid);
        host_heads_mlp_bwd(vf, io->d_values + r, io->a1_vf + r * kMlp, io->a2_vf + r * kMlp, relu, io->d_z1_vf + r * kMlp,
                           io->d_z2_vf + r * kMlp, io->d_h_vf + r * kHid);
    }
    for (int j = 0; j < kAct; ++j)   // H6
        io->d_log_std[j] = (float)loss_sum_host(n_rows, [&](int64_t r) {
            const double z = gauss_z(io->actions[r * kAct + j], io->mean[r * kAct + j], stdv[j]);
            return heads_lsd_term(io->d_log_prob[r], z, io->d_entropy[r]);
        });
    return HE_OK;
}

}  // extern "C"

