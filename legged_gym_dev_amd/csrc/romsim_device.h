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

extern "C" {
void romsimk_reset(const RomSimDev *D, int64_t epoch, int construct, hipStream_t st);
void romsimk_step(const RomSimDev *D, int64_t epoch, const float *actions, hipStream_t st);
void romsimk_policy(const RomSimDev *D, const float *obs, float *out, int64_t rows, hipStream_t st);
void romsimk_collect(const RomSimDev *D, int64_t epoch, int construct, int T, int max_sub, float *z, float *v, float *pz,
                     uint8_t *done, float *x, hipStream_t st);
void romsimk_plan_track(const RomSimDev *D, const float *z, const float *v, const float *x0, int64_t B, int N, int S, float rom_dt,
                        float *pz, float *wt, float *x, float *u, hipStream_t st);
}
