// Device-side struct of the privileged observations (privobs_kernels.hip, privobs_api.hip; legged_hip.h lg_priv_obs_*).
#pragma once
#include "lg_device.h"
#include "../../include/legged_hip.h"

#define LG_PO_TILE 16                   // envs per workgroup, as the post-step tile
#define LG_PO_THREADS 256               // 16 lanes per env: a flat row (58 entries) is four trips, a rough one (250) sixteen

struct PrivTermDev { int32_t kind, off, width; float scale; };

struct PrivObsDev {                     // passed by value to the kernel: the term table and every constant come as kernel arguments
    float *out;                         // (n, W), the handle's own
    // the env's, borrowed for this launch
    const float *root, *dof, *cf, *torques, *actions, *commands, *trajectory, *base_lin_vel, *base_ang_vel, *projected_gravity;
    const float *measured_heights, *friction, *base_mass_delta, *material, *feet_air_time;
    const int64_t *episode_length;
    int n, W, O, A, B, F, NP, H, traj_N /*0: the velocity-command env*/, num_terms;
    float clip, inv_max_len;
    float s_lin_vel, s_ang_vel, s_dof_pos, s_dof_vel, s_height, s_traj[2];
    int32_t feet_idx[LG_MAX_FEET], pen_idx[LG_MAX_PEN];
    float default_dof_pos[LG_MAX_DOF];
    PrivTermDev terms[LG_PRIV_MAX_TERMS];
};

extern "C" {
void privobsk_launch(const PrivObsDev *D, hipStream_t st);
}
