/*
 * hedge_actor.h -- C ABI of libhedgeactor: the actor of an SB3 RecurrentPPO checkpoint
 * (sb3_contrib RecurrentActorCriticPolicy: obs 13 -> LSTM 128 -> Linear 64 -> Linear 64 ->
 * Linear 2) evaluated for N device-resident envs in one HIP kernel on MI355X (gfx950), and
 * the per-episode sums of a closed-loop evaluation around he_step.
 *
 * Conventions (as hedge_env.h): plain C types, every entry point returns an ha_status (the
 * he_status values), the last failure's message is ha_last_error(handle), no C++ exception
 * crosses the boundary.  ha_step / ha_accumulate take DEVICE pointers the caller owns and
 * only enqueue work on `stream` (an opaque hipStream_t): no host synchronisation, no
 * allocation.  ha_host_step is the same arithmetic compiled for the host, over HOST
 * pointers; it needs no GPU.
 *
 * Arithmetic contract, per env e, in this order (restated from sb3_contrib
 * RecurrentActorCriticPolicy.predict / _process_sequence as train_ppo_v2.py:478 uses it, and
 * from quantconnect/model_wrapper.py:111-204):
 *   1. episode_start[e] != 0: h[e,:] = c[e,:] = 0.
 *   2. with statistics: x = f32(clip((f64(obs) - mean) / sqrt(var + epsilon), -clip, clip)),
 *      f64 throughout, rounded once; no clip when has_clip = 0.  Without: x = obs.
 *   3. gates i, f, g, o (torch order): pre[j] = a k-ordered chain of f32 fmaf starting from
 *      b_ih[j] + b_hh[j] (one f32 add), k = 0..12 over W_ih[j,k] x[k], then k = 0..127 over
 *      W_hh[j,k] h[k], then one zero-weight padding term.  v_mfma_f32_32x32x2_f32 computes
 *      exactly this chain.
 *   4. i, f, o = f32(sigmoid_f64(pre)), g = f32(tanh_f64(pre));
 *      c' = f32(f32(f c) + f32(i g)); h' = f32(o f32(tanh_f64(c'))).
 *   5. two layers a = act(chain(bias; W in)), act = tanh (f32(tanh_f64)) or relu; then
 *      mean = chain(action_net).
 *   6. action = clip(mean, -1, 1) (HA_SQUASH_CLIP) or clip(f32(tanh_f64(mean)), -1, 1).
 */
#ifndef HEDGE_ACTOR_H
#define HEDGE_ACTOR_H

#include <stddef.h>
#include <stdint.h>

#include "hedge_env.h" /* he_episode_record, HE_OBS_DIM, the status values */

#ifdef __cplusplus
extern "C" {
#endif

#define HA_ABI_VERSION 1
#define HA_OBS_DIM 13
#define HA_HIDDEN 128
#define HA_MLP 64
#define HA_ACT_DIM 2

typedef int32_t ha_status; /* HE_OK, HE_EINVAL, HE_ESHAPE, HE_EHIP, HE_ENOMEM, HE_ESTATE */

typedef enum ha_activation { HA_ACT_TANH = 0, HA_ACT_RELU = 1 } ha_activation;
typedef enum ha_squash { HA_SQUASH_CLIP = 0, HA_SQUASH_TANH = 1 } ha_squash;

/* The actor: HOST pointers to the 11 f32 tensors of the checkpoint's state dict (row-major,
 * torch layout) and to the optional f64 observation statistics. */
typedef struct ha_weights {
    int32_t abi_version;   /* HA_ABI_VERSION */
    int32_t obs_dim;       /* 13 */
    int32_t hidden;        /* 128 */
    int32_t n_lstm_layers; /* 1 */
    int32_t mlp_width;     /* 64 */
    int32_t act_dim;       /* 2 */
    int32_t activation;    /* ha_activation */
    int32_t squash;        /* ha_squash */
    int32_t has_clip;      /* 0: no clip of the normalised obs (clip_obs=None) */
    int32_t reserved;
    double clip_obs;
    double epsilon;
    const float* w_ih;     /* lstm_actor.weight_ih_l0 [512][13]  */
    const float* w_hh;     /* lstm_actor.weight_hh_l0 [512][128] */
    const float* b_ih;     /* lstm_actor.bias_ih_l0   [512]      */
    const float* b_hh;     /* lstm_actor.bias_hh_l0   [512]      */
    const float* w1;       /* mlp_extractor.policy_net.0.weight [64][128] */
    const float* b1;       /* mlp_extractor.policy_net.0.bias   [64]      */
    const float* w2;       /* mlp_extractor.policy_net.2.weight [64][64]  */
    const float* b2;       /* mlp_extractor.policy_net.2.bias   [64]      */
    const float* w3;       /* action_net.weight [2][64] */
    const float* b3;       /* action_net.bias   [2]     */
    const float* log_std;  /* [2]; not used by the deterministic action, may be NULL */
    const double* obs_mean; /* [13] or NULL: both NULL = no normalisation */
    const double* obs_var;  /* [13] or NULL */
} ha_weights;

typedef struct ha_actor ha_actor;

/* Running sums of one env's current episode (ha_accumulate): s[] in he_episode_record's
 * order (reward, pnl, abs_pnl, cost, pnl_penalty, cost_penalty, per_share_pnl). */
typedef struct ha_episode_sums {
    double s[7];
    int64_t length;
} ha_episode_sums;

const char* ha_version(void);
/* The last failure's message on `actor`; NULL = the last failed ha_create / ha_host_step of
 * this thread. */
const char* ha_last_error(const ha_actor* actor);

/* Checks the shapes (anything but 13 / 128 / 1 layer / 64 / 2 is HE_ESHAPE), uploads the
 * tensors to the current device and packs them in the kernel's fragment order. */
ha_status ha_create(const ha_weights* w, ha_actor** out);
ha_status ha_destroy(ha_actor* actor);

/* One actor step of n envs.  obs [n][13], episode_start [n] u8, h / c [n][128] updated in
 * place, actions [n][2] out; mean_out [n][2] (the pre-squash mean) and obs_norm_out [n][13]
 * (the normalised obs x) may be NULL. */
ha_status ha_step(ha_actor* actor, int64_t n, const float* obs, const uint8_t* episode_start, float* h, float* c,
                  float* actions, float* mean_out, float* obs_norm_out, void* stream);

/* Adds one he_step's info columns (f64 [n] each) to sums[n] in step order; where
 * terminated[e] != 0 appends one he_episode_record (env_id = env_id_offset + e) at
 * records[atomicAdd(count, 1)] while that index is < capacity, then clears sums[e]. */
ha_status ha_accumulate(ha_actor* actor, int64_t n, int64_t env_id_offset, const double* reward_step,
                        const double* step_pnl_total, const double* raw_pnl_deviation_abs,
                        const double* transaction_costs_total, const double* reward_pnl_component,
                        const double* transaction_cost_penalty, const double* per_share_step_pnl,
                        const uint8_t* terminated, ha_episode_sums* sums, he_episode_record* records,
                        int64_t capacity, unsigned long long* count, void* stream);

/* ha_step's arithmetic on the host, HOST pointers, straight from the unpacked tensors. */
ha_status ha_host_step(const ha_weights* w, int64_t n, const float* obs, const uint8_t* episode_start, float* h,
                       float* c, float* actions, float* mean_out, float* obs_norm_out);

#ifdef __cplusplus
}
#endif
#endif /* HEDGE_ACTOR_H */
