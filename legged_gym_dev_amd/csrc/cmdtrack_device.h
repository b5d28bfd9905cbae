// Device-side struct of the command tracker (cmdtrack_kernels.hip, cmdtrack_api.hip; legged_hip.h lg_cmdtrack_*).
#pragma once
#include "lg_device.h"
#include "../../include/legged_hip.h"

#define LG_CT_LANES LG_WAVE             // one env per lane, one wave per workgroup, as the ROM simulator
#define LG_CT_STATE 8                   // floats per env of lg_cmdtrack_buffers.state: z 2, v 2, u 3, 1 unused

struct CmdTrackDev {                    // passed by value to the kernel
    const DevParams *P;                 // the TRACKER's own: what the laws of lg_traj.h read (buf.tg_state / inject_uniforms, K, cfg.traj,
                                        // cfg.seed, cfg.env_offset, tg_wsamp), as RomSimDev.P; nothing else is filled in
    float *state;                       // (n, LG_CT_STATE)
    int32_t *n_resample, *overrun;      // (n) each
    const float *plan;                  // (n, LG_PLAN_MAX_N, 2)
    // the env's, borrowed for this launch
    const float *root, *dof;
    float *obs;
    const uint8_t *reset;
    int n, num_obs, A, kind, track_yaw, inject, R, cmd_col, n_nodes, x_n;
    float rom_dt;
    float Kp[9], u_min[3], u_max[3], cmd_scale[3];
};

extern "C" {
void cmdtrackk_launch(const CmdTrackDev *D, const lg_cmdtrack_rec *rec, int t, int64_t epoch, int construct, hipStream_t st);
}
