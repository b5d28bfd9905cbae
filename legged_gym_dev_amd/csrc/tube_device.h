// Device-side struct of the tube-model trainer (tube_kernels.hip, plan_kernels.hip, tube_api.hip, plan_api.hip).
#pragma once
#include "lg_device.h"
#include "../../include/legged_hip.h"

#define LG_TUBE_ROWS 32                 // rows per workgroup tile of k_tube_rows
#define LG_TUBE_THREADS 256
#define LG_TUBE_ROLLOUT_LDS (144 * 1024) // k_tube_rollout keeps the weights in LDS where weights + tile fit this (a CU has 160 KiB)
#define LG_TUBE_RING_MAX 1024           // floats of output history per sequence of k_tube_rollout_window, ((taps-1) dN + 1) * fb at most:
                                        // the largest model's 16-row tile (36 KiB) plus 16 such rings (64 KiB) fits LG_TUBE_ROLLOUT_LDS
#define LG_TUBE_MAX_LIN 5               // num_layers (<= 4) hidden Linear layers + the output Linear

struct TubeSplit {                      // one side of random_split, device memory owned by the caller
    const float *x, *y, *v;             // flat: data (rows, in), target (rows, out).  horizon: w (rows, T), z (rows, T, nz), v (rows, T, m)
    int64_t rows;
};

struct TubeDev {                        // passed by value to kernels
    int in_dim, out_dim, units, layers, act, loss, horizon;
    int H_fwd, H_rev, T, nz, m;         // horizon dataset: padded time length T, z / v widths
    float alpha, delta, sp_beta;
    uint64_t seed;
    int64_t num_params, slab_ld;        // slab row: num_params gradients + the loss sum, padded to slab_ld
    int64_t off_w[LG_TUBE_MAX_LIN], off_b[LG_TUBE_MAX_LIN];
    int din[LG_TUBE_MAX_LIN], dout[LG_TUBE_MAX_LIN];
    float *params, *wt;                 // wt: every weight matrix transposed ([k][j], same offsets), for the forward's coalesced reads
    float *grads, *adam_m, *adam_v;
    float *slab;                        // (workgroups, slab_ld) per-workgroup partial gradients of one step
    float *evpart;                      // (workgroups, 4) per-workgroup partial eval sums
    float *normpart;                    // per-block sums of g^2 of k_tube_adam
    uint32_t *done_ctr;                 // k_tube_adam's last-block counter (returns to 0 after every launch)
    float *log;                         // (log_cap, 4): loss, lr after the step, grad_norm, rows
    float *eval;                        // 4: loss, fraction fw > w, mean |w - fw| where fw > w, rows
    int32_t *starts;                    // horizon window start per row of the last step / eval
    int32_t *perm;
    int64_t log_cap;
    // level-conditioned tube (lg_tube_cfg.level_input), appended: the fields above keep their offsets
    int level_input;                    // 1: the last input column is the row's level, drawn per row in [level_lo, level_hi)
    float level_lo, level_hi;
    float *levels;                      // level per row of the last step / eval
};

// columns of a horizon handle's item built from z of width nz and v of width m; a conditioned handle's last column is the level
inline int64_t window_dim(const TubeDev &D, int32_t nz, int32_t m) {
    return D.H_rev + (int64_t)nz + (int64_t)(D.H_rev + D.H_fwd) * m + (D.level_input ? 1 : 0);
}

struct TubeMember {                     // one model of a sweep (lg_tube_sweep); the kernels index a device array of these by blockIdx.y
    TubeDev dev;                        // its own buffers, alpha / delta / activation / seed / level range; the shape is the same in every member
    double lr0, gamma;                  // its Adam rate and StepLR schedule
    int64_t step_size;
};

extern "C" {
// tube_kernels.hip
size_t tubek_lds_bytes(const TubeDev *D);
int tubek_init();
void tubek_step(const TubeDev *D, const TubeSplit *S, const int32_t *rows, int64_t count, uint64_t key, float norm, hipStream_t s);
void tubek_adam(const TubeDev *D, int nwg, int64_t t, double lr0, double gamma, int64_t step_size, float norm, int64_t rows,
                hipStream_t s);
void tubek_eval(const TubeDev *D, const TubeSplit *S, const int32_t *rows, uint64_t key, float norm, float level, hipStream_t s);
void tubek_wt(const TubeDev *D, hipStream_t s);
void tubek_perm(const TubeDev *D, int n, uint64_t epoch, hipStream_t s);
void tubek_iota(int32_t *p, int64_t n, hipStream_t s);
void tubek_step_sweep(const TubeMember *M, int K, const TubeDev *D0, const TubeSplit *S, const int32_t *rows, int64_t pos, int64_t count,
                      uint64_t key, float norm, hipStream_t s);
void tubek_adam_sweep(const TubeMember *M, int K, const TubeDev *D0, int nwg, int64_t t, float norm, int64_t rows, hipStream_t s);
void tubek_eval_sweep(const TubeMember *M, int K, const TubeDev *D0, const TubeSplit *S, const int32_t *rows, uint64_t key, float norm,
                      float level, hipStream_t s);
void tubek_predict_levels(const TubeDev *D, const float *x, const int32_t *rows, int64_t count, const float *levels, int n_levels,
                          float *o, hipStream_t s);
void tubek_predict_windows_levels(const TubeDev *D, const float *w, const float *z, const float *v, const int32_t *env,
                                  const int32_t *start, int T, int nz, int m, int64_t count, const float *levels, int n_levels,
                                  float *o, hipStream_t s);
void tubek_perm_sweep(const TubeMember *M, int K, int n, uint64_t epoch, hipStream_t s);
void tubek_predict(const TubeDev *D, const float *x, const float *y, const float *v, const int32_t *rows, const int32_t *env,
                   const int32_t *start, int T, int nz, int m, int64_t count, float *o, hipStream_t s);
void tubek_rollout(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, const uint8_t *reseed, float *o, hipStream_t s);
void tubek_rollout_window(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, int taps, int dN, int stride,
                          const uint8_t *reseed, float *o, hipStream_t s);
}
