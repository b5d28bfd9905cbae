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
