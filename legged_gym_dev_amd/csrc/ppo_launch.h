// The launchers of the PPO kernels (ppo_kernels.hip, ppo_gemm.hip, ppo_mlp_fused.hip, ppo_rnn.hip), as the learner's host side
// (ppo_sched.hip, ppo_api.hip) calls them.  The defining files include this header too: a definition that drifts from its
// declaration here does not compile.
#pragma once
#include "ppo_device.h"
#include "ppo_mlp_args.h"
#include "ppo_rnn.h"

extern "C" {
// ppo_gemm.hip
void ppok_gemm_fwd(const GemmArgs *g, int nz, hipStream_t s);
void ppok_gemm_dx(const GemmArgs *g, int nz, hipStream_t s);
void ppok_gemm_dw(const GemmArgs *g, int nz, hipStream_t s);
// ppo_mlp_fused.hip
int ppok_mlp_fwd(const MlpArgs *g, const PpoDev *P, hipStream_t s);
int ppok_mlp_supported(const MlpArgs *g);
int64_t ppok_mlp_frag_elems(int K, int N);
void ppok_mlp_frag_build(const MlpArgs *g, hipStream_t s);
// ppo_kernels.hip
void ppok_sync_planes(const PpoDev *P, hipStream_t s);
void ppok_act_sample(const PpoDev *P, const float *obs, const float *cobs, const float *mu, const float *val, int t,
                     int64_t cnt, int inject, hipStream_t s);
void ppok_process_step(const PpoDev *P, const float *rew, const uint8_t *dones, const uint8_t *tos, int t, hipStream_t s);
void ppok_gae(const PpoDev *P, const float *last_values, hipStream_t s);
void ppok_det_fold(const PpoDev *P, hipStream_t s);
void ppok_adv_normalize(const PpoDev *P, hipStream_t s);
void ppok_gather(const PpoDev *P, int mb, hipStream_t s);
void ppok_randperm(const PpoDev *P, int n, uint64_t update_idx, hipStream_t s);
void ppok_loss(const PpoDev *P, const float *mu, const float *v, float *dmu, float *dval, hipStream_t s);
int ppok_step(const PpoDev *P, int par, const PpoDev *G, int gather_mb, hipStream_t s);
size_t ppok_head_part_floats();
int ppok_head_fused(const PpoDev *P, int H3, const float *xa, const float *xc, float *dza, float *dzc, int64_t w_a, int64_t b_a,
                    int64_t w_c, int64_t b_c, int64_t b_prev_a, int64_t b_prev_c, hipStream_t s);
// ppo_rnn.hip
void ppok_lstm_fwd(const RnnStepArgs *a, int nz, hipStream_t s);
void ppok_lstm_bwd(const RnnBwdArgs *a, int nz, hipStream_t s);
void ppok_lstm_bias_grad(const PpoDev *P, const RnnBiasArgs *a, hipStream_t s);
void ppok_lstm_reset(float *h0, float *c0, float *h1, float *c1, const uint8_t *done, int N, int H, hipStream_t s);
}
