// Device-side struct of the actor's observation history (obshist_kernels.hip, obshist_api.hip; legged_hip.h lg_obs_hist_*).
#pragma once
#include "lg_device.h"
#include "../../include/legged_hip.h"

#define LG_OH_TILE 16                   // envs per workgroup, as the post-step and the privileged row
#define LG_OH_THREADS 256               // lanes along (env, obs column) of the tile

struct ObsHistDev {                     // passed by value to the kernel: the range table comes as kernel arguments
    float *row;                         // (n, W), the handle's own: [obs_t | sel(obs_t-1) | ... | sel(obs_t-H+1)]
    const int64_t *marks;               // (n), the handle's own: the number of the compute that reinitialises the env (see epoch)
    // the env's, borrowed for this launch
    const float *obs;                   // (n, O)
    const uint8_t *reset;               // (n), the step's dones
    int64_t epoch;                      // the number of this compute, 1-based: env i is marked iff marks[i] == epoch
    int n, O, W, H, S, num_ranges, reset_mode;
    int32_t lo[LG_OBS_HIST_MAX_RANGES], hi[LG_OBS_HIST_MAX_RANGES];
    int32_t pos[LG_OBS_HIST_MAX_RANGES];      // selected columns before range r
};

extern "C" {
void obshistk_launch(const ObsHistDev *D, hipStream_t st);
void obshistk_mark(int64_t *marks, const int32_t *ids, int n, int num_envs, int64_t epoch, hipStream_t st);
}
