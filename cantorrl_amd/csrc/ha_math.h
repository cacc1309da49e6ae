// ha_math.h -- the scalar arithmetic of the RecurrentPPO actor (include/hedge_actor.h,
// "Arithmetic contract"), shared by the HIP kernel (__device__) and ha_host_step (__host__):
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

// the LSTM cell from the four pre-activations: c' into *c, returns h'
HE_HD float cell_update(float pi, float pf, float pg, float po, float* c) {
    const float i = sigmoidf_r(pi), f = sigmoidf_r(pf), o = sigmoidf_r(po);
    const float g = tanhf_r(pg);
    const float fc = f * *c;
    const float ig = i * g;
    const float cn = fc + ig;
    *c = cn;
    return o * tanhf_r(cn);
}

HE_HD float mlp_act(float x, bool relu) { return relu ? (x > 0.0f ? x : (x != x ? x : 0.0f)) : tanhf_r(x); }

HE_HD float squash_action(float mean, bool tanh_squash) {
    const float a = tanh_squash ? tanhf_r(mean) : mean;
    return he::np_clipf(a, -1.0f, 1.0f);
}

}  // namespace ha
