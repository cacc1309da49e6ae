// ha_math.h -- the scalar arithmetic of the RecurrentPPO actor (include/hedge_actor.h,
// "Arithmetic contract"), its rollout policy (sampling, log-probability), GAE, the optimizer step, the
// PPO loss and the PPO heads, shared by the HIP kernels (__device__) and the ha_host_* entry points (__host__):
// one implementation, so the two agree bit for bit.  The library is compiled with
// -ffp-contract=off; f64 + - * / are IEEE on both sides and he::exp_k is host / device identical.
#pragma once

#include "he_math.h"

namespace ha {

constexpr int kObs = 13;
constexpr int kHid = 128;
constexpr int kGates = 4 * kHid;
constexpr int kMlp = 64;
constexpr int kAct = 2;
constexpr int kKx = kObs + kHid;   // 141: the gate chain's terms [x | h]
constexpr int kKp = kKx + 1;       // + one zero-weight term: whole 32x32x2 k-steps

// 1 / (1 + e^-x) in f64
HE_HD double sigmoid_f64(double x) { return 1.0 / (1.0 + he::exp_k(-x)); }

// tanh in f64: (1 - e) / (1 + e) with e = e^(-2|x|), the sign restored; below 2^-13 the
// odd series x (1 - x^2 / 3) (next term 2 x^5 / 15 < 2^-54 relative), where 1 - e would cancel
HE_HD double tanh_f64(double x) {
    const double ax = fabs(x);
    if (ax < 0x1p-13) return x * (1.0 - (x * x) * (1.0 / 3.0));
    if (!(ax < 20.0)) return (x != x) ? x : (x < 0.0 ? -1.0 : 1.0);   // 1 - 2 e^-40 rounds to 1
    const double e = he::exp_k(-2.0 * ax);
    const double t = (1.0 - e) / (1.0 + e);
    return x < 0.0 ? -t : t;
}

HE_HD float sigmoidf_r(float x) { return (float)sigmoid_f64((double)x); }
HE_HD float tanhf_r(float x) { return (float)tanh_f64((double)x); }

// x = f32(clip((f64(obs) - mean) / sd, -clip, clip)), sd = sqrt(var + eps) and y = RN(1 / sd)
// made on the host; the quotient by he::div_by (correctly rounded: the f64 division's bits)
HE_HD float norm_obs(float o, double mean, double sd, double y, bool has_clip, double clip) {
    double q = he::div_by((double)o - mean, sd, y);
    if (has_clip) q = q < -clip ? -clip : (q > clip ? clip : q);
    return (float)q;
}

// the LSTM cell from the four pre-activations: c' into *c, the four activations into gate[i, f, g, o]
// (contract F2), returns h'
HE_HD float cell_forward(float pi, float pf, float pg, float po, float* c, float* gate) {
    const float i = sigmoidf_r(pi), f = sigmoidf_r(pf), o = sigmoidf_r(po);
    const float g = tanhf_r(pg);
    const float fc = f * *c;
    const float ig = i * g;
    const float cn = fc + ig;
    *c = cn;
    gate[0] = i, gate[1] = f, gate[2] = g, gate[3] = o;
    return o * tanhf_r(cn);
}

// cell_forward without the activations
HE_HD float cell_update(float pi, float pf, float pg, float po, float* c) {
    float gate[4];
    return cell_forward(pi, pf, pg, po, c, gate);
}

// Contract B2-B3 for one (unit, env) at one step: the gradient of the four pre-activations into
// dgate[i, f, g, o]; returns dct f, the cell carry of the step before (the caller zeroes it at an
// episode start).  One f32 rounding per line.
HE_HD float cell_backward(float i, float f, float g, float o, float ct, float c_prev, float dh, float dc,
                          float* dgate) {
    const float tc = tanhf_r(ct);
    const float tc2 = tc * tc;
    const float omt = 1.0f - tc2;
    const float dho = dh * o;
    const float dhc = dho * omt;
    const float dct = dhc + dc;
    const float i1 = 1.0f - i;
    const float ii = i * i1;
    const float f1 = 1.0f - f;
    const float ff = f * f1;
    const float g2 = g * g;
    const float gg = 1.0f - g2;
    const float o1 = 1.0f - o;
    const float oo = o * o1;
    const float dg_i = dct * g;
    const float dg_f = dct * c_prev;
    const float dg_g = dct * i;
    const float dg_o = dh * tc;
    dgate[0] = dg_i * ii;
    dgate[1] = dg_f * ff;
    dgate[2] = dg_g * gg;
    dgate[3] = dg_o * oo;
    return dct * f;
}

HE_HD float mlp_act(float x, bool relu) { return relu ? (x > 0.0f ? x : (x != x ? x : 0.0f)) : tanhf_r(x); }

HE_HD float squash_action(float mean, bool tanh_squash) {
    const float a = tanh_squash ? tanhf_r(mean) : mean;
    return he::np_clipf(a, -1.0f, 1.0f);
}

// ---------------------------------------------------------------- the rollout policy (ha_policy_step)
// std = f32(exp(f64(log_std)))
HE_HD float policy_std(float log_std) { return (float)he::exp_k((double)log_std); }

// Contract P6's z_j and the term of action j in the log-probability (the loop of sample_action and of
// heads_log_prob): one f64 rounding per line
HE_HD double gauss_z(float a, float mean, float stdv) { return ((double)a - (double)mean) / (double)stdv; }
HE_HD double log_prob_term(double z, float log_std) {
    const double zz = z * z;
    const double t = -0.5 * zz;
    const double u = t - (double)log_std;
    return u - 0.9189385332046727;
}

// Contract steps 4-6: the diagonal-Gaussian sample of env g at step_index, its clipped form and
// its log-probability.  One Philox block per (seed, step_index, g): nothing depends on how the
// envs are split over calls.
HE_HD void sample_action(const float* mean, const float* log_std, const float* stdv, uint64_t seed,
                         uint64_t step_index, uint64_t g, bool deterministic, float* a, float* env_a,
                         float* log_prob) {
    float eps[kAct] = {0.0f, 0.0f};
    if (!deterministic) {
        he::u32x4 ctr;
        ctr.x = (uint32_t)step_index;
        ctr.y = (uint32_t)(step_index >> 32);
        ctr.z = (uint32_t)g;
        ctr.w = (uint32_t)(g >> 32);
        const he::u32x4 r = he::philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
        double z0, z1;
        he::box_muller(he::u01(r.x, r.y), he::u01(r.z, r.w), &z0, &z1);
        eps[0] = (float)z0;
        eps[1] = (float)z1;
    }
    double lp = 0.0;
    for (int j = 0; j < kAct; ++j) {
        a[j] = deterministic ? mean[j] : fmaf(stdv[j], eps[j], mean[j]);
        env_a[j] = he::np_clipf(a[j], -1.0f, 1.0f);
        lp = lp + log_prob_term(gauss_z(a[j], mean[j], stdv[j]), log_std[j]);
    }
    *log_prob = (float)lp;
}

// Contract step 7 for env e: SB3's compute_returns_and_advantage in f32, k = K-1 .. 0; every
// array is [K][n], so a wave of consecutive e reads consecutive addresses.
HE_HD void gae_env(int64_t e, int64_t n, int64_t K, float g32, float gl32, const float* rewards,
                   const float* values, const uint8_t* episode_starts, const float* last_values,
                   const uint8_t* last_dones, float* advantages, float* returns) {
    float last = 0.0f;
    float nv = last_values[e];
    float nnt = 1.0f - (float)last_dones[e];
    for (int64_t k = K - 1; k >= 0; --k) {
        const int64_t i = k * n + e;
        const float v = values[i];
        const float gv = g32 * nv;
        const float gvn = gv * nnt;
        const float rg = rewards[i] + gvn;
        const float delta = rg - v;
        const float gn = gl32 * nnt;
        const float gl = gn * last;
        last = delta + gl;
        advantages[i] = last;
        returns[i] = last + v;
        nv = v;
        nnt = 1.0f - (float)episode_starts[i];
    }
}

// ---------------------------------------------------------------- the optimizer step (ha_adam_step)
// the constants of contract O4-O5, formed once on the host
struct AdamConsts {
    float b1, b2, a1, a2, ss, bc2s, eps, max_norm;
    int clip;
};

// Contract O3-O4: the norm from the f64 total, the coefficient every gradient is multiplied by
HE_HD float adam_clip(double total, const AdamConsts& k, float* norm_out) {
    const float norm = (float)sqrt(total);
    *norm_out = norm;
    if (!k.clip) return 1.0f;
    const float d = norm + 1e-6f;
    const float q = k.max_norm / d;
    return q < 1.0f ? q : 1.0f;
}

// Contract O5 for one element: one f32 rounding per line
HE_HD void adam_element(float g, float c, const AdamConsts& k, float* p, float* m, float* v) {
    const float gc = g * c;
    const float m1 = k.b1 * *m;
    const float m2 = k.a1 * gc;
    const float mn = m1 + m2;
    const float gg = gc * gc;
    const float v1 = k.b2 * *v;
    const float v2 = k.a2 * gg;
    const float vn = v1 + v2;
    const float sq = sqrtf(vn);
    const float sb = sq / k.bc2s;
    const float den = sb + k.eps;
    const float r = mn / den;
    const float u = k.ss * r;
    *m = mn;
    *v = vn;
    *p = *p - u;
}

// ---------------------------------------------------------------- the PPO loss (ha_ppo_loss)
// the constants of contract L4-L6, formed once on the host
struct LossConsts {
    double c, lo, hi, cv, ent_coef, vf_coef, vf2, n;   // lo = 1 - c, hi = 1 + c, vf2 = 2 vf_coef, n = f64(N)
    int normalize, clip_vf;
};

// Contract L3: the spread of the advantages from the sum of squared deviations
HE_HD double loss_std(double ssq, double n) {
    const double var = ssq / (n - 1.0);
    return sqrt(var);
}

// the five terms of L5's sums
struct LossTerms {
    double pol, val, ent, kl, clipped;
};

// Contract L3 (the row's A'), L4 and L6 for one row; den = std + 1e-8.  One f64 rounding per line.
HE_HD LossTerms loss_row(float v, float lp, float ent, float old_lp, float adv, float ret, float old_v, double mean,
                         double den, const LossConsts& k, float* d_v, float* d_lp) {
    double a = (double)adv;
    if (k.normalize) {
        const double dev = a - mean;
        a = dev / den;
    }
    const double d = (double)lp - (double)old_lp;
    const double r = he::exp_k(d);
    const double rc = r < k.lo ? k.lo : (r > k.hi ? k.hi : r);
    const double s1 = a * r;
    const double s2 = a * rc;
    const bool active = (a >= 0.0) ? (r < k.hi) : (r > k.lo);
    double vp = (double)v;
    bool pass = true;
    if (k.clip_vf) {
        const double dv = (double)v - (double)old_v;
        const double cl = dv < -k.cv ? -k.cv : (dv > k.cv ? k.cv : dv);
        vp = (double)old_v + cl;
        pass = fabs(dv) <= k.cv;
    }
    const double e = (double)ret - vp;
    const double r1 = r - 1.0;
    LossTerms t;
    t.pol = s2 < s1 ? s2 : s1;
    t.val = e * e;
    t.ent = (double)ent;
    t.kl = r1 - d;
    t.clipped = fabs(r1) > k.c ? 1.0 : 0.0;
    const double gl = -s1;
    const double ge = k.vf2 * e;
    const double gv = -ge;
    *d_lp = active ? (float)(gl / k.n) : 0.0f;
    *d_v = pass ? (float)(gv / k.n) : 0.0f;
    return t;
}

// Contract L5 from the five totals, mean and std: the eight statistics, each rounded once
HE_HD void loss_stats(const double* tot, double mean, double sd, const LossConsts& k, float* stats) {
    const double policy = -tot[0] / k.n;
    const double value = tot[1] / k.n;
    const double entropy = -tot[2] / k.n;
    const double pe = k.ent_coef * entropy;
    const double l1 = policy + pe;
    const double vv = k.vf_coef * value;
    stats[0] = (float)(l1 + vv);
    stats[1] = (float)policy;
    stats[2] = (float)value;
    stats[3] = (float)entropy;
    stats[4] = (float)(tot[3] / k.n);
    stats[5] = (float)(tot[4] / k.n);
    stats[6] = (float)mean;
    stats[7] = (float)sd;
}

// ---------------------------------------------------------------- the PPO heads (ha_ppo_heads_*)
// Contract H2: the log-probability of the stored action a[2] under Normal(mean, std), P6's sum
HE_HD float heads_log_prob(const float* a, const float* mean, const float* log_std, const float* stdv) {
    double lp = 0.0;
    for (int j = 0; j < kAct; ++j) lp = lp + log_prob_term(gauss_z(a[j], mean[j], stdv[j]), log_std[j]);
    return (float)lp;
}

// Contract H3: the entropy of the diagonal Gaussian, the same for every row
HE_HD float heads_entropy(const float* log_std) {
    double e = 0.0;
    for (int j = 0; j < kAct; ++j) {
        const double t = (0.5 + 0.9189385332046727) + (double)log_std[j];
        e = e + t;
    }
    return (float)e;
}

// Contract H4: the gradient of mean[j] from the row's d_log_prob and z_j
HE_HD float heads_d_mean(float d_lp, double z, float stdv) {
    const double q = z / (double)stdv;
    return (float)((double)d_lp * q);
}

// Contract H6's term of one row for action j
HE_HD double heads_lsd_term(float d_lp, double z, float d_ent) {
    const double zz = z * z;
    const double zm = zz - 1.0;
    const double p = (double)d_lp * zm;
    return p + (double)d_ent;
}

// Contract H5: the gradient of a pre-activation from that of the activation a = act(z)
HE_HD float act_backward(float d_a, float a, bool relu) {
    if (relu) return a > 0.0f ? d_a : 0.0f;
    const float aa = a * a;
    const float om = 1.0f - aa;
    return d_a * om;
}

}  // namespace ha
