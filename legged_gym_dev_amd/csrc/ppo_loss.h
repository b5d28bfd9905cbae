// The row arithmetic of the PPO minibatch loss (rsl_rl PPO.update), once, for the four kernels of ppo_kernels.hip that evaluate it:
// k_loss, k_head_fused<32|64> and k_head_net<128, NA>; and the layout of the per-row sums they and k_head_finish<128> reduce.
//
// Everything here takes scalars by value and returns a small struct by value: no PpoDev &, no out-parameters, no pointer into a
// kernel's register arrays.  k_head_net<128, 12> sits on the register count that gives three workgroups per CU, and a helper that
// reaches into the caller's state through a reference cost it 12 bytes of scratch.  Operand paths, staging,
// reductions and the scaling of d loss / d value stay with each kernel.
#pragma once
#include "ppo_device.h"

// ---- the per-row sums: part[] of every loss kernel, the tail of a k_head_net scratch row ----
enum : int {
    PPO_SUM_DSTD = 0,                                  // [0 .. MA)   d loss / d sigma
    PPO_SUM_DBIAS_ACTOR = LG_PPO_MAX_A,                // [MA .. 2MA) actor head bias gradient (= column sums of d loss / d mu)
    PPO_SUM_DBIAS_CRITIC = 2 * LG_PPO_MAX_A,           // critic head bias gradient (= sum of d loss / d value)
    PPO_SUM_KL,                                        // KL(old || new)
    PPO_SUM_VLOSS,                                     // value loss
    PPO_SUM_SLOSS,                                     // surrogate loss
    PPO_NSUMS
};
// a per-action slot past the task's action count carries nothing
__device__ __forceinline__ bool ppo_sum_live(int k, int A) { return k >= PPO_SUM_DBIAS_CRITIC || (k % LG_PPO_MAX_A) < A; }
// the sums that need mu only (k_head_net's actor workgroups); the other two need V only
__device__ __forceinline__ bool ppo_sum_of_actor(int k) { return k < PPO_SUM_DBIAS_CRITIC || k == PPO_SUM_KL || k == PPO_SUM_SLOSS; }
// where sum k is accumulated; b_a / b_c: flat offsets of the two head biases
__device__ __forceinline__ float *ppo_sum_dest(const PpoDev &P, int k, int64_t b_a, int64_t b_c) {
    if (k < PPO_SUM_DBIAS_ACTOR) return &P.grads[P.off_std + k];
    if (k < PPO_SUM_DBIAS_CRITIC) return &P.grads[b_a + (k - PPO_SUM_DBIAS_ACTOR)];
    if (k == PPO_SUM_DBIAS_CRITIC) return &P.grads[b_c];
    if (k == PPO_SUM_KL) return &P.grads[P.num_params];                 // the KL sum rides in the grad buffer tail
    if (k == PPO_SUM_VLOSS) return &P.loss_acc[0];
    return &P.loss_acc[1];
}

// ---- Gaussian terms in reciprocal form (the fused heads; k_loss keeps its own, in division form) ----
// per-action constants (row independent), so that the per-row loss needs no log and no division
struct PpoGauss { float so2, i2s2, is2, is, lgs, klc; };   // sigma_old^2, 1/(2 s^2), 1/s^2, 1/s, ln s + ln sqrt(2 pi), ln(s / s_old + 1e-5) - 1/2
__device__ __forceinline__ PpoGauss ppo_gauss(float sg, float so) {
    return {so * so, 1.0f / (2.0f * sg * sg), 1.0f / (sg * sg), 1.0f / sg, logf(sg) + 0.9189385332046727f, logf(sg / so + 1.e-5f) - 0.5f};
}
// one action's term of the log-prob; d = action - mu
__device__ __forceinline__ float ppo_lp_term(float d, float i2s2, float lgs) { return -(d * d) * i2s2 - lgs; }
// one action's term of KL(old || new); mo = old mean, m = new mean
__device__ __forceinline__ float ppo_kl_term(float mo, float m, float so2, float i2s2, float klc) { return klc + (so2 + (mo - m) * (mo - m)) * i2s2; }
__device__ __forceinline__ float ppo_dmu(float dl_dlp, float d, float is2) { return dl_dlp * d * is2; }
// ent = entropy_coef / R: the entropy bonus's pull on sigma
__device__ __forceinline__ float ppo_dstd(float dl_dlp, float d, float is2, float is, float ent) {
    return dl_dlp * (d * d * is2 * is - is) - ent * is;
}

// ---- surrogate: importance ratio, its clip, and which of the two branches carries the gradient ----
struct PpoSurrogate { float dl_dlp, s1, s2; };             // d loss / d log-prob (already / R); the row's loss is fmaxf(s1, s2)
__device__ __forceinline__ PpoSurrogate ppo_surrogate(float clip, float lp, float lp_old, float adv, float invR) {
    const float ratio = expf(lp - lp_old);
    const float rc = fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
    const float s1 = -adv * ratio, s2 = -adv * rc;
    return {(s1 >= s2 ? -adv : 0.0f) * ratio * invR, s1, s2};          // torch.max ties: see DESIGN.md
}

// ---- value loss: clipped (three-way: which square is larger, or a tie) or plain ----
struct PpoValue { float lv, dv; };                         // dv = d lv / d v, UNSCALED: value_coef / R is applied by the caller, in its own order
__device__ __forceinline__ PpoValue ppo_value(int clipped_value, float clip, float v, float v_old, float ret) {
    float lv, dv;
    if (clipped_value) {
        const float dvv = v - v_old;
        const float vc = v_old + fminf(fmaxf(dvv, -clip), clip);
        const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
        const float inside = (dvv >= -clip && dvv <= clip) ? 1.0f : 0.0f;
        lv = fmaxf(l1, l2);
        if (l1 > l2) dv = 2.0f * (v - ret);
        else if (l1 < l2) dv = 2.0f * (vc - ret) * inside;
        else dv = (v - ret) + (vc - ret) * inside;
    } else {
        lv = (ret - v) * (ret - v);
        dv = 2.0f * (v - ret);
    }
    return {lv, dv};
}
