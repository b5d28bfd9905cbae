// Device-side struct of the empirical observation normalisation (obsnorm_kernels.hip, obsnorm_api.hip; legged_hip.h lg_obs_norm_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/legged_hip.h"

#define LG_ON_WAVES 4                                       // waves per workgroup: wave w takes rows w, w + 4, ... of the row block
#define LG_ON_THREADS (LG_ON_WAVES * LG_OBS_NORM_COLS)      // lane = column of the column block (LG_OBS_NORM_COLS = the wave's 64 lanes)

struct ObsNormProb {                    // one row kind: the actor's or the critic's
    const float *x;                     // (n, W), the caller's
    float *y;                           // (n, W), the caller's or the handle's own
    const float *st_in;                 // (3, W) mean | var | std: the state this compute starts from
    float *st_out;                      // (3, W): the other copy, written by the row-block-0 workgroups of a training compute
    double2 *slab;                      // (row blocks, W) of (S1, S2) = sums of (x - k_j) and (x - k_j)^2 over the block's rows
    double rate;                        // n / count after this update
    float eps;
    int W, update;                      // update: 0 frozen (st_out and slab unused)
};

struct ObsNormDev {                     // passed by value; blockIdx.z picks the problem
    ObsNormProb p[2];
    long long n;                        // rows, the same for both problems
    int nrb;                            // row blocks of LG_OBS_NORM_ROWS = gridDim.x
};

extern "C" {
void obsnormk_stats(const ObsNormDev *D, int num, hipStream_t st);
void obsnormk_apply(const ObsNormDev *D, int num, hipStream_t st);
}
