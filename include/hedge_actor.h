/*
 * hedge_actor.h -- C ABI of libhedgeactor: the actor of an SB3 RecurrentPPO checkpoint
 * (sb3_contrib RecurrentActorCriticPolicy: obs 13 -> LSTM 128 -> Linear 64 -> Linear 64 ->
 * Linear 2) evaluated for N device-resident envs in one HIP kernel on MI355X (gfx950), the
 * per-episode sums of a closed-loop evaluation around he_step, and the training side: actor,
 * critic, action sampling and log-probability of a rollout step in one launch, GAE, and for the
 * PPO update both LSTMs over a stored sequence with per-step resets, forward and backward, their
 * weight gradients, the MLP heads after them with the log-probability and the entropy, forward and
 * backward, the PPO loss with its gradients, the gradient-norm clip with Adam's step, and the re-packing
 * of a policy's handle from the updated device tensors.
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
 *
 * Rollout collection (ha_policy_step, ha_gae: what sb3_contrib RecurrentPPO.collect_rollouts
 * computes per step, and SB3 2.6.0 RolloutBuffer.compute_returns_and_advantage after it;
 * restated, SB3 is not a dependency).  Per env e:
 *   P1. steps 1-5 with the actor's tensors and h_pi / c_pi give mean[2]: for the same tensors
 *       the bits of ha_step's mean_out.
 *   P2. steps 1-5 with the critic's LSTM (lstm_critic) and MLP (value_net, the same
 *       activation) on the same normalised obs and the critic's own h_vf / c_vf give a2[64];
 *       value = chain(vb3; v3 a2), the k-ordered fmaf chain of 64 terms.
 *   P3. std[j] = f32(exp_f64(f64(log_std[j]))).
 *   P4. noise: one Philox4x32-10 block, counter (lo(step_index), hi(step_index), lo(g), hi(g))
 *       with g = env_id_offset + e, key (lo(seed), hi(seed)): the env's own layout, so the
 *       caller passes a seed distinct from the env's.  u1 = u01(x0, x1), u2 = u01(x2, x3),
 *       (z0, z1) = box_muller(u1, u2) in f64, eps[j] = f32(z_j).  Nothing depends on how the
 *       envs are split over calls or ranks.
 *   P5. a[j] = deterministic ? mean[j] : fmaf(std[j], eps[j], mean[j]);
 *       env_action[j] = clip(a[j], -1, 1).
 *   P6. log_prob = f32(sum_j ((-0.5 z_j^2 - f64(log_std[j])) - 0.9189385332046727)), f64, j in
 *       order from 0, with z_j = (f64(a[j]) - f64(mean[j])) / f64(std[j]):
 *       torch.distributions.Normal(mean, std).log_prob(a).sum(-1), rounded once.
 *   P7. GAE, f32 throughout, no contraction; g32 = f32(gamma), gl32 = f32(gamma gae_lambda)
 *       (the product in f64).  last = 0; for k = K-1 .. 0:
 *         nnt   = 1 - f32(last_dones)          at k = K-1, else 1 - f32(episode_starts[k+1])
 *         nv    = last_values                  at k = K-1, else values[k+1]
 *         delta = ((rewards[k] + ((g32 nv) nnt)) - values[k])
 *         last  = delta + ((gl32 nnt) last)
 *         advantages[k] = last; returns[k] = last + values[k]
 *       The env never truncates an episode (it ends by `terminated` only), so SB3's time-out
 *       bootstrap (reward += gamma V(terminal_obs)) has no counterpart here.
 *
 * The LSTM over a stored sequence, forward and backward (ha_lstm_seq_forward / _backward: what
 * sb3_contrib's _process_sequence computes inside evaluate_actions, one LSTM call per time step
 * with the state zeroed at episode_starts, and autograd's backward of it; restated).  Arrays are
 * laid out [L][B][...] (SB3's (buffer_size, n_envs, ...)); per env e and network:
 *   F1. the state before step 0 is (h0[e], c0[e]); for t = 0 .. L-1 steps 1, 3 and 4 above with
 *       x = x[t][e] (already normalised) and episode_start = episode_starts[t][e]: the reset, the
 *       142-term k-ordered fmaf gate chains from b_ih + b_hh, cell_update.  h[t], c[t] are the
 *       state after step t: for the same tensors and inputs the bits that t + 1 successive
 *       ha_policy_step / ha_host_policy_step calls leave in h_pi, c_pi (h_vf, c_vf).
 *   F2. gates[t][e][0..3][u] = the post-activation i, f, g, o of unit u at step t (f32), the
 *       values step 4 forms on its way to c' and h'.
 *   B1. the carries dh_rec[128] and dc[128] start at 0; t runs from L-1 down to 0.  h0, c0 and x
 *       receive no gradient (SB3 stores the states of a rollout as constants).
 *   B2. per unit u, with (i, f, g, o) = gates[t], c_prev = 0 where episode_starts[t], else
 *       c[t-1] (c0 at t = 0), and tc = f32(tanh_f64(c[t])); every operation one f32 rounding, the
 *       products in the order written, no contraction:
 *         dh  = d_h[t] + dh_rec
 *         dct = ((dh o) (1 - tc tc)) + dc
 *         d_gates[t] = { (dct g) (i (1 - i)), (dct c_prev) (f (1 - f)), (dct i) (1 - g g),
 *                        (dh tc) (o (1 - o)) }
 *   B3. dc = episode_starts[t] ? 0 : dct f.
 *   B4. dh_rec[j] = episode_starts[t] ? 0 : the k-ordered f32 fmaf chain from 0 over
 *       u = 0 .. 511 (torch's gate rows: i, f, g, o blocks of 128) of d_gates[t][u] w_hh[u][j].
 *       v_mfma_f32_32x32x2_f32 over K = 512 in one accumulator computes exactly this chain.
 *
 * The weight gradients (ha_lstm_seq_weight_grads: dW_ih = d_gates^T x, dW_hh = d_gates^T h_prev,
 * db_ih = db_hh = sum d_gates, sums over the L B rows of d_gates).  Per network, rows r = t B + e
 * for r in [0, R), R = L B; dg[r][u] = d_gates[t][e][u], u = 0 .. 511 in torch's row order;
 * z[r][k], k = 0 .. 141: x[t][e][k] for k < 13; h_prev[t][e][k - 13] for 13 <= k < 141, with
 * h_prev = 0 where episode_starts[t][e], else h[t-1][e] (h0[e] at t = 0); 1.0 at k = 141 (the bias
 * column).
 *   W1. block sum: the rows are cut into blocks of HA_WGRAD_BLOCK consecutive rows.  s_b[u][k] is
 *       the f32 fmaf chain from +0 over the block's rows in ascending order,
 *       s = fmaf(dg[r][u], z[r][k], s); a short last block is continued with terms
 *       fmaf(+0, +0, s) up to the full block (part of the contract: both builds may pad).
 *       v_mfma_f32_32x32x2_f32 with the row index as its k computes exactly this chain.
 *   W2. chunk sum: HA_WGRAD_CHUNK consecutive blocks form a chunk; p_c[u][k] is the f64 sum from
 *       0.0 of f64(s_b[u][k]) over the chunk's blocks in ascending order.
 *   W3. total[u][k] is the f64 sum from 0.0 of p_c[u][k] over ascending chunks.
 *   W4. outputs, each rounded once from f64 to f32: d_w_ih[u][k] = total[u][k] for k < 13,
 *       d_w_hh[u][j] = total[u][13 + j], d_b[u] = total[u][141] (the value of db_ih and db_hh).
 *   Nothing in W1-W4 depends on the grid, the CU count or the number of networks per call.
 *
 * The optimizer step (ha_adam_step: torch.nn.utils.clip_grad_norm_ over every tensor of the call, then
 * torch.optim.Adam's step without weight decay and amsgrad; restated).  The tensors t = 0 .. n - 1 of
 * the call in the caller's order, g the gradient, m = exp_avg, v = exp_avg_sq, p the parameter:
 *   O1. sum of squares per block: each tensor is cut into blocks of HA_OPT_BLOCK = 256 consecutive
 *       elements, a short last block padded with +0.  Element i of a block contributes q_i =
 *       f64(g_i) f64(g_i) (exact in f64); the 256 values are added in f64 by a fixed tree: q_i +=
 *       q_(i + 128) for i < 128, then q_i += q_(i + 64) for i < 64, ... q_0 += q_1.  s_b = q_0.
 *   O2. total = the f64 sum from 0.0 of s_b over the blocks in (tensor, block) order.
 *   O3. norm = f32(sqrt(total)), the f64 square root correctly rounded, then rounded to f32.
 *   O4. with a clip (max_grad_norm > 0 and finite): q = f32(max_grad_norm) / (norm + 1e-6f) in f32,
 *       c = q < 1 ? q : 1.  Without: c = 1.  g' = g c, one f32 multiply (by 1 where nothing clips, as
 *       torch multiplies).
 *   O5. per element in f32, every operation rounded once, no fmaf, no contraction, in the order
 *       written; b1 = f32(beta1), b2 = f32(beta2), a1 = f32(1 - beta1), a2 = f32(1 - beta2), ss =
 *       f32(lr / (1 - beta1^t)), bc2s = f32(sqrt(1 - beta2^t)), e = f32(eps), each formed on the host
 *       in f64 (pow, sqrt of libm) and rounded once, t the 1-based count of this step:
 *         m <- (b1 m) + (a1 g')
 *         v <- (b2 v) + (a2 (g' g'))
 *         denom = (sqrtf(v) / bc2s) + e
 *         p <- p - (ss (m / denom))
 *       f32 / and sqrtf are correctly rounded on the device (-fhip-fp32-correctly-rounded-divide-sqrt).
 *   Nothing in O1-O5 depends on the grid; a tensor cut at a multiple of 256 elements into two tensors
 *   standing where it stood gives the same blocks, hence the same bits.
 *
 * The PPO loss (ha_ppo_loss: sb3_contrib 2.6.0 RecurrentPPO.train's loss for one minibatch of N rows
 * without padding, its six statistics and its gradients with respect to values, log_prob and entropy in
 * closed form; restated).  Everything in f64 from the f32 inputs, every operation rounded once, in the
 * order written, no contraction; c = clip_range, cv = clip_range_vf.  Per row i: v = values, lp =
 * log_prob, ent = entropy, old_lp, A = advantages, ret = returns, old_v = old_values.
 *   L1. a sum: the rows are cut into blocks of HA_LOSS_BLOCK consecutive rows, a short last block
 *       padded with terms +0.  Lane i of 256 adds the terms of its rows i, i + 256, ... of the block
 *       from 0.0 in ascending order: q_i.  Then the tree of O1: q_i += q_(i + 128) for i < 128, ...
 *       q_0 += q_1; s_b = q_0.  The total is the f64 sum from 0.0 of s_b over the blocks in order.
 *       Every sum below is this sum.
 *   L2. mean = sum f64(A_i) / N.
 *   L3. with normalize_advantage: std = sqrt(sum (f64(A_i) - mean)^2 / (N - 1)) (unbiased) and
 *       A'_i = (f64(A_i) - mean) / (std + 1e-8).  Without: A'_i = f64(A_i), and the statistics report
 *       mean 0, std 1.  f64 / and sqrt are correctly rounded, as in O3.
 *   L4. per row: d = f64(lp) - f64(old_lp) (exact), r = he::exp_k(d), lo = 1 - c, hi = 1 + c,
 *       rc = r < lo ? lo : (r > hi ? hi : r); s1 = A' r, s2 = A' rc, pol = s2 < s1 ? s2 : s1;
 *       active = (A' >= 0) ? (r < hi) : (r > lo).
 *       vp = f64(v) and pass = true without a value clip (cv <= 0); with one, dv = f64(v) - f64(old_v),
 *       vp = f64(old_v) + (dv < -cv ? -cv : (dv > cv ? cv : dv)), pass = |dv| <= cv (torch.clamp passes
 *       gradient on the closed interval).
 *       e = f64(ret) - vp, val = e e, kl = (r - 1) - d, clipped = |r - 1| > c (1.0 or 0.0).
 *   L5. policy = -(sum pol) / N, value = sum val / N, entropy_loss = -(sum f64(ent)) / N,
 *       loss = (policy + ent_coef entropy_loss) + vf_coef value, approx_kl = sum kl / N,
 *       clip_fraction = sum clipped / N.  stats = { loss, policy, value, entropy_loss, approx_kl,
 *       clip_fraction, mean, std }, each rounded once to f32.
 *   L6. d_log_prob_i = active ? -(A' r) / N : +0; d_values_i = pass ? -((2 vf_coef) e) / N : +0;
 *       d_entropy_i = -ent_coef / N; each rounded once to f32.
 *   Nothing in L1-L6 depends on the grid.
 *
 * The PPO heads (ha_ppo_heads_forward / _backward: what evaluate_actions computes after the LSTMs, the two
 * 64-64 MLPs, action_net, value_net, the Gaussian log-probability of the stored action and the entropy,
 * and autograd's backward of it down to the LSTMs' outputs; restated).  Rows r = 0 .. R - 1, h_pi[r] and
 * h_vf[r] of 128 each; every row is independent of the others except in H6.  f32, one rounding per
 * operation, no contraction, unless it says f64.
 *   H1. per network a1 = act(chain(b1; W1 h)), a2 = act(chain(b2; W2 a1)): step 5 with mlp_act.  Actor:
 *       mean[j] = chain(b3[j]; w3[j] a2).  Critic: value = chain(vb3; v3 a2).  A chain is the k-ordered
 *       fmaf chain from the bias: for the same tensors and the same h the bits of ha_policy_step's
 *       mean_out and values.
 *   H2. std[j] = f32(exp_f64(f64(log_std[j]))) (P3); log_prob is P6 with a = the row's stored action.
 *   H3. entropy = f32(sum_j ((0.5 + 0.9189385332046727) + f64(log_std[j]))), f64, j in order from 0.
 *   H4. z_j as in P6; d_mean[j] = f32(f64(d_log_prob) (z_j / f64(std[j]))), f64.  The critic's head
 *       gradient is d_values.
 *   H5. per network, d_out the head's gradient (d_mean[2], or d_values):
 *         d_a2[k] = the fmaf chain from +0 over the head's rows j in order of d_out[j] w3[j][k]
 *         d_z2[k] = d_a2[k] (1 - a2[k] a2[k]) for tanh; a2[k] > 0 ? d_a2[k] : +0 for relu
 *         d_a1[k] = the fmaf chain from +0 over u = 0 .. 63 of d_z2[u] W2[u][k]; d_z1 from d_a1, a1 likewise
 *         d_h[k], k = 0 .. 127 = the fmaf chain from +0 over u = 0 .. 63 of d_z1[u] W1[u][k]
 *       v_mfma_f32_32x32x2_f32 with u as its k computes exactly these chains (as B4).
 *   H6. d_log_std[j] = f32(sum_r (f64(d_log_prob_r) (z_rj z_rj - 1) + f64(d_entropy_r))), f64, the sum
 *       of L1 over the rows (blocks of HA_LOSS_BLOCK, the same lane ownership and tree), R <= 2^22.
 *   Nothing in H1-H6 depends on the grid.
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

/* ---- rollout collection: actor + critic + sampling in one launch, and GAE ---- */
#define HA_POLICY_ABI_VERSION 1

/* Actor and critic of the checkpoint: HOST pointers, torch layout.  log_std is required. */
typedef struct ha_policy_weights {
    int32_t abi_version;   /* HA_POLICY_ABI_VERSION */
    int32_t obs_dim;       /* 13 */
    int32_t hidden;        /* 128, actor and critic */
    int32_t n_lstm_layers; /* 1 */
    int32_t mlp_width;     /* 64 */
    int32_t act_dim;       /* 2 */
    int32_t activation;    /* ha_activation, both MLPs */
    int32_t has_clip;
    double clip_obs;
    double epsilon;
    const double* obs_mean; /* [13] or NULL: both NULL = no normalisation */
    const double* obs_var;
    const float* w_ih;     /* the actor, as ha_weights */
    const float* w_hh;
    const float* b_ih;
    const float* b_hh;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* w3;
    const float* b3;
    const float* log_std;  /* [2] */
    const float* c_w_ih;   /* lstm_critic.weight_ih_l0 [512][13]  */
    const float* c_w_hh;   /* lstm_critic.weight_hh_l0 [512][128] */
    const float* c_b_ih;   /* lstm_critic.bias_ih_l0   [512]      */
    const float* c_b_hh;   /* lstm_critic.bias_hh_l0   [512]      */
    const float* v1;       /* mlp_extractor.value_net.0.weight [64][128] */
    const float* vb1;      /* mlp_extractor.value_net.0.bias   [64]      */
    const float* v2;       /* mlp_extractor.value_net.2.weight [64][64]  */
    const float* vb2;      /* mlp_extractor.value_net.2.bias   [64]      */
    const float* v3;       /* value_net.weight [1][64] */
    const float* vb3;      /* value_net.bias   [1]     */
} ha_policy_weights;

typedef struct ha_policy ha_policy;

/* The last failure's message on `policy`; NULL = the last failed ha_policy_create /
 * ha_host_policy_step / ha_host_gae / ha_gae of this thread. */
const char* ha_policy_last_error(const ha_policy* policy);

/* As ha_create / ha_destroy: anything but 13 / 128 x 1 layer / 64-64 / 2 actions / 1 value is
 * HE_ESHAPE with a message; both networks are packed in ha_create's fragment order. */
ha_status ha_policy_create(const ha_policy_weights* w, ha_policy** out);
ha_status ha_policy_destroy(ha_policy* policy);

/* Re-packs and re-uploads every tensor and statistic of an existing handle (a training loop
 * changes them after each rollout).  SYNCHRONISES: it waits for the device to go idle, so no
 * step in flight reads half-written weights, and copies synchronously.  Not capturable. */
ha_status ha_policy_update(ha_policy* policy, const ha_policy_weights* w);

/* The 21 tensors of a policy, flat: w_ih ... log_std, c_w_ih ... vb3 in ha_policy_weights' order. */
#define HA_POLICY_TENSOR_FLOATS 171461

/* ha_policy_update's re-packing from DEVICE tensors, on the stream: the 21 tensor pointers of w_dev
 * are DEVICE pointers (f32, torch layout, 4-byte aligned; an optimizer's parameters as they stand
 * when the launch runs).  One launch of policy_pack_kernel writes the handle's packed networks, b_ih +
 * b_hh (one f32 add), log_std and std = f32(exp_f64(log_std)): bit for bit what ha_policy_update
 * uploads for the same values.  The same launch copies the 21 tensors into a buffer of the handle
 * (ha_policy_download).  obs_mean / obs_var of w_dev are ignored: statistics, clip, epsilon and
 * activation stay as ha_policy_create or the last ha_policy_update set them; the other fields are
 * checked as ha_policy_create checks them (HE_ESHAPE, HE_EINVAL; a NULL handle or tensor HE_EINVAL),
 * before the launch.  Stream-ordered: no host synchronisation, no copy call, no allocation, capturable.
 * A step enqueued later on the same stream reads the new tensors, one enqueued earlier the old; work
 * on OTHER streams that reads the handle or writes the tensors is the caller's to order (an event). */
ha_status ha_policy_refresh(ha_policy* policy, const ha_policy_weights* w_dev, void* stream);

/* The tensors the last ha_policy_refresh read, to HOST memory: out [HA_POLICY_TENSOR_FLOATS], flat in
 * ha_policy_weights' order.  Copies on `stream` and WAITS for that stream.  HE_ESTATE when no refresh
 * has run since ha_policy_create or the last ha_policy_update (the caller's host tensors are current). */
ha_status ha_policy_download(ha_policy* policy, float* out, void* stream);

/* One collection step of n envs (contract P1-P6), one launch, DEVICE pointers, no host
 * synchronisation.  obs [n][13], episode_start [n] u8; h_pi, c_pi, h_vf, c_vf [n][128] are
 * updated in place (16-byte aligned) unless write_state = 0, which computes every output and
 * stores no state: SB3's predict_values call for last_values.  Out: actions [n][2] unclipped
 * (what the buffer stores), env_actions [n][2] clipped to +-1 (what the env is fed), values
 * [n], log_probs [n]; mean_out [n][2] and obs_norm_out [n][13] may be NULL. */
ha_status ha_policy_step(ha_policy* policy, int64_t n, int64_t env_id_offset, uint64_t seed, uint64_t step_index,
                         int32_t deterministic, int32_t write_state, const float* obs, const uint8_t* episode_start,
                         float* h_pi, float* c_pi, float* h_vf, float* c_vf, float* actions, float* env_actions,
                         float* values, float* log_probs, float* mean_out, float* obs_norm_out, void* stream);

/* Contract P7 over DEVICE arrays laid out [K][n] (SB3's (buffer_size, n_envs)): one thread per
 * env walks k from K-1 down to 0, every access coalesced over the env index. */
ha_status ha_gae(int64_t n, int64_t K, double gamma, double gae_lambda, const float* rewards, const float* values,
                 const uint8_t* episode_starts, const float* last_values, const uint8_t* last_dones,
                 float* advantages, float* returns, void* stream);

/* The same arithmetic on the host, HOST pointers, straight from the unpacked tensors. */
ha_status ha_host_policy_step(const ha_policy_weights* w, int64_t n, int64_t env_id_offset, uint64_t seed,
                              uint64_t step_index, int32_t deterministic, int32_t write_state, const float* obs,
                              const uint8_t* episode_start, float* h_pi, float* c_pi, float* h_vf, float* c_vf,
                              float* actions, float* env_actions, float* values, float* log_probs, float* mean_out,
                              float* obs_norm_out);
ha_status ha_host_gae(int64_t n, int64_t K, double gamma, double gae_lambda, const float* rewards,
                      const float* values, const uint8_t* episode_starts, const float* last_values,
                      const uint8_t* last_dones, float* advantages, float* returns);

/* ---- the LSTM over a stored sequence with per-step resets, forward and backward (F1-F2, B1-B4) ---- */

/* One network of ha_lstm_seq_forward.  The weights are read in torch layout as they stand when
 * the call runs on the stream (an optimizer step changes them in place): w_ih [512][13], w_hh
 * [512][128], b_ih, b_hh [512]; h0, c0 [B][128] in; h, c [L][B][128] and gates [L][B][4][128] out. */
typedef struct ha_lstm_seq_net {
    const float* w_ih;
    const float* w_hh;
    const float* b_ih;
    const float* b_hh;
    const float* h0;
    const float* c0;
    float* h;
    float* c;
    float* gates;
} ha_lstm_seq_net;

/* One network of ha_lstm_seq_backward: w_hh [512][128], c0 [B][128], the forward's c [L][B][128]
 * and gates [L][B][4][128], d_h [L][B][128] (the loss's gradient of every h[t]) in; d_gates
 * [L][B][4][128] out (the gradient of the pre-activations, rows in torch's order i, f, g, o). */
typedef struct ha_lstm_seq_bwd {
    const float* w_hh;
    const float* c0;
    const float* c;
    const float* gates;
    const float* d_h;
    float* d_gates;
} ha_lstm_seq_bwd;

/* Bytes of the workspace both calls take for n_nets (1 or 2) networks, 0 for any other count:
 * the weights packed in the kernels' fragment order.  Each call packs what it reads from the
 * tensors it is given (one small launch before the sequence kernel), so the workspace carries
 * nothing from call to call and one workspace serves forward and backward in stream order. */
size_t ha_lstm_seq_workspace_bytes(int64_t n_nets);

/* n_nets = 1 or 2 networks (`nets` is a HOST array of structs holding DEVICE pointers) over the
 * same x [L][B][13] and episode_starts [L][B] u8: one launch over a grid of (tiles of 32 envs,
 * n_nets), each workgroup walking all L steps of its tile.  Every pointer is a DEVICE pointer,
 * 16-byte aligned; stream-ordered, no host synchronisation, no allocation.  n_nets other than 1
 * or 2, L or B < 1 or B > 2^30 is HE_ESHAPE; a NULL or misaligned pointer HE_EINVAL; the message
 * is ha_policy_last_error(NULL). */
ha_status ha_lstm_seq_forward(int64_t n_nets, int64_t L, int64_t B, const float* x, const uint8_t* episode_starts,
                              const ha_lstm_seq_net* nets, void* workspace, void* stream);
ha_status ha_lstm_seq_backward(int64_t n_nets, int64_t L, int64_t B, const uint8_t* episode_starts,
                               const ha_lstm_seq_bwd* nets, void* workspace, void* stream);

/* The same arithmetic on the host, HOST pointers (no alignment asked), no workspace. */
ha_status ha_host_lstm_seq_forward(int64_t n_nets, int64_t L, int64_t B, const float* x,
                                   const uint8_t* episode_starts, const ha_lstm_seq_net* nets);
ha_status ha_host_lstm_seq_backward(int64_t n_nets, int64_t L, int64_t B, const uint8_t* episode_starts,
                                    const ha_lstm_seq_bwd* nets);

/* ---- the LSTM's weight gradients from d_gates (W1-W4) ---- */
#define HA_WGRAD_BLOCK 128 /* rows of one f32 fmaf chain (W1) */
#define HA_WGRAD_CHUNK 64  /* blocks of one f64 partial (W2): 8,192 rows a chunk */

/* One network of ha_lstm_seq_weight_grads: the backward's d_gates [L][B][4][128], the forward's h
 * [L][B][128] and its h0 [B][128] in; d_w_ih [512][13], d_w_hh [512][128], d_b [512] out. */
typedef struct ha_lstm_seq_wgrad {
    const float* d_gates;
    const float* h;
    const float* h0;
    float* d_w_ih;
    float* d_w_hh;
    float* d_b;
} ha_lstm_seq_wgrad;

/* Bytes of the workspace ha_lstm_seq_weight_grads takes: the chunks' f64 partials p_c, [512][142]
 * per chunk and network.  0 for n_nets other than 1 or 2 or a shape the call refuses.  The
 * workspace carries nothing from call to call. */
size_t ha_lstm_seq_weight_grads_workspace_bytes(int64_t n_nets, int64_t L, int64_t B);

/* W1-W4 for n_nets = 1 or 2 networks over the same x [L][B][13] and episode_starts [L][B] u8: two
 * launches, one workgroup per (chunk, 128 gate rows, network) forming p_c, then one thread per
 * output adding the chunks in order.  DEVICE pointers, 16-byte aligned but for x (52-byte rows);
 * stream-ordered, no host synchronisation, no allocation.  The checks of ha_lstm_seq_forward, made
 * before anything is launched; also HE_ESHAPE when L B has more than 2^31 - 1 chunks.  The message
 * is ha_policy_last_error(NULL). */
ha_status ha_lstm_seq_weight_grads(int64_t n_nets, int64_t L, int64_t B, const float* x,
                                   const uint8_t* episode_starts, const ha_lstm_seq_wgrad* nets, void* workspace,
                                   void* stream);

/* The same arithmetic on the host, HOST pointers (no alignment asked), no workspace. */
ha_status ha_host_lstm_seq_weight_grads(int64_t n_nets, int64_t L, int64_t B, const float* x,
                                        const uint8_t* episode_starts, const ha_lstm_seq_wgrad* nets);

/* ---- the optimizer step: gradient-norm clip + Adam over a list of tensors (O1-O5) ---- */
#define HA_OPT_BLOCK 256         /* elements of one block of O1 */
#define HA_OPT_MAX_TENSORS 64
#define HA_OPT_MAX_BLOCKS 4096   /* blocks of one call: 2^20 elements in whole blocks; the policy's 21
                                    tensors make 677.  Every workgroup adds all the blocks' sums (O2). */

/* One tensor of the call: numel f32 elements each, contiguous.  grad is read, never written. */
typedef struct ha_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} ha_adam_tensor;

typedef struct ha_adam_hyper {
    double lr, beta1, beta2, eps;
    double max_grad_norm; /* <= 0, +inf or NaN: no clip */
    int64_t t;            /* the 1-based count of this step: the host knows it without reading the device */
    float* grad_norm_out; /* [1] or NULL: norm of O3, before the clip, as clip_grad_norm_ returns it */
} ha_adam_hyper;

/* Bytes of ha_adam_step's workspace: one f64 per block, the s_b of O1.  0 for a list the call
 * refuses.  The workspace carries nothing from call to call. */
size_t ha_adam_workspace_bytes(int64_t n_tensors, const ha_adam_tensor* tensors);

/* O1-O5 over `tensors`, a HOST array of structs of DEVICE pointers (4-byte aligned; the workspace 8):
 * two launches, opt_norm_kernel with one workgroup per block writing s_b, then opt_adam_kernel, where
 * every workgroup adds the s_b in O2's order (all of them get the same bits), updates its own block
 * and the first writes grad_norm_out (a DEVICE pointer).  No atomics, no waiting between workgroups;
 * stream-ordered, no host synchronisation, no allocation.  Before any launch: n_tensors outside
 * [1, HA_OPT_MAX_TENSORS], a numel < 1 or more than HA_OPT_MAX_BLOCKS blocks in all is HE_ESHAPE; a
 * NULL pointer, t < 1, lr or eps not finite, eps < 0 or a beta outside [0, 1) HE_EINVAL.  The message
 * is ha_policy_last_error(NULL). */
ha_status ha_adam_step(int64_t n_tensors, const ha_adam_tensor* tensors, const ha_adam_hyper* hyper, void* workspace,
                       void* stream);

/* The same arithmetic on the host, HOST pointers throughout, no workspace. */
ha_status ha_host_adam_step(int64_t n_tensors, const ha_adam_tensor* tensors, const ha_adam_hyper* hyper);

/* ---- the PPO loss: statistics and the gradients of values, log_prob, entropy (L1-L6) ---- */
#define HA_LOSS_BLOCK 1024       /* rows of one block of L1: four rows a lane of 256 */
#define HA_LOSS_MAX_BLOCKS 4096  /* blocks of one call: 2^22 rows, a 256 x 16,384 buffer as one minibatch */

typedef struct ha_ppo_loss_hyper {
    double clip_range;
    double clip_range_vf; /* <= 0 or NaN: no value clip */
    double ent_coef;
    double vf_coef;
    int32_t normalize_advantage;
} ha_ppo_loss_hyper;

/* DEVICE pointers (HOST pointers for ha_host_ppo_loss), n_rows f32 each, 4-byte aligned. */
typedef struct ha_ppo_loss_io {
    const float* values;
    const float* log_prob;
    const float* entropy;
    const float* old_log_prob;
    const float* advantages;
    const float* returns;
    const float* old_values; /* required iff clip_range_vf > 0, else ignored (may be NULL) */
    float* d_values;
    float* d_log_prob;
    float* d_entropy;
    float* stats;            /* [8]: loss, policy_gradient_loss, value_loss, entropy_loss, approx_kl,
                                clip_fraction, adv_mean, adv_std (0, 1 without normalisation) */
} ha_ppo_loss_io;

/* Bytes of ha_ppo_loss's workspace: seven f64 per block (the s_b of L2's, L3's and L5's five sums).
 * 0 for an n_rows the call refuses.  The workspace carries nothing from call to call. */
size_t ha_ppo_loss_workspace_bytes(int64_t n_rows);

/* L1-L6 over n_rows rows, one workgroup of 256 per block of HA_LOSS_BLOCK rows.  With normalisation four
 * launches: loss_mean_kernel writes each block's sum of A, loss_spread_kernel (every workgroup adds
 * those in block order: the same bits everywhere) each block's sum of squared deviations,
 * loss_rows_kernel the three gradients and each block's five sums, loss_stats_kernel (one workgroup)
 * the eight statistics.  Without normalisation the last two alone.  No atomics, no waiting between
 * workgroups: kernel boundaries are the only grid-wide ordering.  Stream-ordered: no host
 * synchronisation, no copy call, no allocation; the workspace (8-byte aligned) is the caller's.  Before
 * any launch: n_rows outside [1, HA_LOSS_BLOCK HA_LOSS_MAX_BLOCKS], or n_rows = 1 with
 * normalize_advantage (an unbiased std of one row), is HE_ESHAPE; a NULL or misaligned pointer, a
 * missing old_values when clip_range_vf > 0, a clip_range that is negative or not finite HE_EINVAL.
 * The message is ha_policy_last_error(NULL). */
ha_status ha_ppo_loss(int64_t n_rows, const ha_ppo_loss_io* io, const ha_ppo_loss_hyper* hyper, void* workspace,
                      void* stream);

/* The same arithmetic on the host (L1-L6 taken literally), HOST pointers, no workspace. */
ha_status ha_host_ppo_loss(int64_t n_rows, const ha_ppo_loss_io* io, const ha_ppo_loss_hyper* hyper);

/* ---- the PPO heads: MLPs, action / value heads, log-probability, entropy, and their backward (H1-H6) ---- */

/* The 13 tensors after the LSTMs, DEVICE pointers (HOST pointers for ha_host_ppo_heads_*), f32, torch
 * layout, read as they stand when the call runs on the stream.  w1, w2, w3, b1, b2 and their critic
 * counterparts 16-byte aligned, b3, vb3 and log_std 4-byte. */
typedef struct ha_ppo_heads_weights {
    const float* w1;       /* mlp_extractor.policy_net.0.weight [64][128] */
    const float* b1;       /* mlp_extractor.policy_net.0.bias   [64]      */
    const float* w2;       /* mlp_extractor.policy_net.2.weight [64][64]  */
    const float* b2;       /* mlp_extractor.policy_net.2.bias   [64]      */
    const float* w3;       /* action_net.weight [2][64] */
    const float* b3;       /* action_net.bias   [2]     */
    const float* log_std;  /* [2] */
    const float* v1;       /* mlp_extractor.value_net.0.weight [64][128] */
    const float* vb1;      /* mlp_extractor.value_net.0.bias   [64]      */
    const float* v2;       /* mlp_extractor.value_net.2.weight [64][64]  */
    const float* vb2;      /* mlp_extractor.value_net.2.bias   [64]      */
    const float* v3;       /* value_net.weight [1][64] */
    const float* vb3;      /* value_net.bias   [1]     */
    int32_t activation;    /* ha_activation, both MLPs */
} ha_ppo_heads_weights;

/* The forward's rows.  [R][128], [R][64]: 16-byte aligned; [R][2]: 8-byte; [R]: 4-byte. */
typedef struct ha_ppo_heads_fwd {
    const float* h_pi;     /* [R][128] the actor LSTM's output */
    const float* h_vf;     /* [R][128] the critic LSTM's */
    const float* actions;  /* [R][2] the stored (unclipped) actions */
    float* values;         /* [R] out */
    float* log_prob;       /* [R] out */
    float* entropy;        /* [R] out */
    float* mean;           /* [R][2] out, saved for the backward */
    float* a1_pi;          /* [R][64] out, saved for the backward: the actor's first hidden layer */
    float* a2_pi;          /* [R][64] its second */
    float* a1_vf;          /* [R][64] the critic's */
    float* a2_vf;
} ha_ppo_heads_fwd;

/* The backward's rows, alignment as ha_ppo_heads_fwd; d_log_std 4-byte. */
typedef struct ha_ppo_heads_bwd {
    const float* d_values;   /* [R] ha_ppo_loss's three gradients */
    const float* d_log_prob;
    const float* d_entropy;
    const float* actions;    /* [R][2] */
    const float* mean;       /* [R][2] the forward's */
    const float* a1_pi;      /* [R][64] the forward's */
    const float* a2_pi;
    const float* a1_vf;
    const float* a2_vf;
    float* d_h_pi;           /* [R][128] out */
    float* d_h_vf;
    float* d_z1_pi;          /* [R][64] out: the gradients of the pre-activations (the weight gradients' input) */
    float* d_z2_pi;
    float* d_z1_vf;
    float* d_z2_vf;
    float* d_mean;           /* [R][2] out */
    float* d_log_std;        /* [2] out */
} ha_ppo_heads_bwd;

/* Bytes of the workspace both calls take: both networks' weights in the kernels' fragment order (W1, W2
 * and their transposes), log_std with std, and two f64 per block of HA_LOSS_BLOCK rows (H6's s_b).  0 for
 * an n_rows the calls refuse.  Each call packs what it reads (heads_pack_kernel in front), so the
 * workspace carries nothing from call to call. */
size_t ha_ppo_heads_workspace_bytes(int64_t n_rows);

/* H1-H3 over n_rows rows: heads_pack_kernel, then heads_fwd_kernel over a grid of (groups of 64-row
 * tiles, 2), y = actor / critic, a workgroup keeping its slice of the weights in registers over its tiles.
 * H4-H6: heads_pack_kernel, heads_bwd_kernel over a grid of (blocks of HA_LOSS_BLOCK rows, 2), each actor
 * workgroup writing its block's two sums of H6, then heads_lsd_kernel (one workgroup) adding them in block
 * order.  No atomics, no waiting between workgroups: kernel boundaries are the only grid-wide ordering.
 * Stream-ordered: no host synchronisation, no copy call, no allocation; capturable; the workspace (16-byte
 * aligned) is the caller's.  Before any launch: n_rows outside [1, HA_LOSS_BLOCK HA_LOSS_MAX_BLOCKS] is
 * HE_ESHAPE; a NULL or misaligned pointer or an unknown activation HE_EINVAL.  The message is
 * ha_policy_last_error(NULL).  A refused call writes nothing. */
ha_status ha_ppo_heads_forward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_fwd* io,
                               void* workspace, void* stream);
ha_status ha_ppo_heads_backward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_bwd* io,
                                void* workspace, void* stream);

/* The same arithmetic on the host (H1-H6 taken literally), HOST pointers (4-byte aligned), no workspace. */
ha_status ha_host_ppo_heads_forward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_fwd* io);
ha_status ha_host_ppo_heads_backward(int64_t n_rows, const ha_ppo_heads_weights* weights, const ha_ppo_heads_bwd* io);

#ifdef __cplusplus
}
#endif
#endif /* HEDGE_ACTOR_H */
