// Device-side struct of the ROM-on-ROM simulator (romsim_kernels.hip, romsim_api.hip).
#pragma once
#include "lg_device.h"
#include "../../include/legged_hip.h"

#define LG_RS_LANES LG_WAVE             // one env per lane, one wave per workgroup: 8192 envs spread over 128 CUs' worth of waves
#define LG_RS_VWIN (2 * (LG_TRAJ_MAX_PTS - 1))      // floats of the input window
#define LG_RS_LDS_STRIDE (2 * LG_TRAJ_MAX_PTS + 1 + LG_RS_VWIN)     // state window (LG_TG_WIN, lg_traj.h) + input window; odd

struct RomSimDev {                      // passed by value to kernels
    const DevParams *P;                 // what the laws of lg_traj.h read: buf.tg_state / tg_traj / trajectory / inject_uniforms, K,
                                        // cfg.traj, cfg.dt, cfg.seed, cfg.env_offset, cb, tg_kind, tg_wsamp; nothing else is filled in
    float *root, *v_traj, *obs, *act;
    int32_t *n_resample, *overrun;
    int n, inject, R, rand_dist;
    float dt, Kp, Kd, llh;
    float vel_min[2], vel_max[2], acc_min[2], acc_max[2];
    float noise_lo[4], noise_hi[4], max_dist[2];
};
