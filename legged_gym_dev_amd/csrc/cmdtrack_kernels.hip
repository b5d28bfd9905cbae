// Command tracker: ROM trajectories tracked by a velocity-command policy -- the loop of the reference's
// deep_tube_learning/data_collection_velocity.py:84-156 ("DV") with SingleInt2D (trajopt/rom_dynamics.py "RD":182-199), the
// TrajectoryGenerator (RD:441-616) and quat2yaw / yaw2rot / wrap_angles (deep_tube_learning/utils.py:82-105).
//
// One lane per env, workgroups of one wave, ONE launch per env step: the record of the step the env just made, the ROM step, the
// next ROM input (drawn from the generator or read from the env's plan) and the next command, written over the command columns
// of the observation.  A few dozen dependent flops on a handful of floats per env; in torch it is 25-odd launches and several
// host reads.  fp32, one rounding per operation (fp contract off), as lg_traj.h and romsim_kernels.hip.  The generator's laws are
// those of lg_traj.h (tg_resample, tg_input), used as they are and driven the way the ROM simulator drives them: the hold time
// checked on EVERY evaluation, the draws keyed by the env's own resample count.  Every store is a plain C++ store into the env's own
// rows: no atomics, no LDS, and an env's outputs depend neither on its lane nor on the number of envs.
#include "cmdtrack_device.h"
#include "lg_traj.h"

// TrajectoryGenerator.resample (RD:510-520) of env i, keyed by the env's own resample count (romsim_kernels.hip rs_resample).
// Injected: block r of the env's row; a missing block is counted per env (lg_cmdtrack_inject_status) and the last one read again.
__device__ inline void ct_resample(const CmdTrackDev &D, int i, int64_t epoch) {
    const int r = D.n_resample[i];
    int slot0 = 0;
    if (D.inject) {
        int b = r;
        if (b >= D.R) { D.overrun[i] = D.overrun[i] + 1; b = D.R - 1; }
        slot0 = LG_RS_NRESET + b * LG_TG_NDRAW;
    }
    tg_resample(D.P, tg_par_cfg(D.P), i, slot0, (epoch << 32) | (int64_t)(uint32_t)(r + 1), D.inject);
    D.n_resample[i] = r + 1;
}

// get_input_t (RD:560-566) + the stationary mask (RD:580)
__device__ inline void ct_input(const CmdTrackDev &D, int i, float tt, int64_t epoch, float v[2]) {
    const float *s = D.P->buf.tg_state + (size_t)i * LG_TG_STRIDE;
    if (tt > s[LG_TG_T_FINAL]) ct_resample(D, i, epoch);
    tg_input(D.P, i, tt, v);
}

// TrajectoryGenerator.reset(z) (RD:592-605) without its window, which nothing here reads: the clocks restart at -N rom_dt, one
// resample, and the N evaluations of the pre-roll, each of which may resample again
__device__ inline void ct_gen_reset(const CmdTrackDev &D, int i, int64_t epoch, int construct) {
#pragma clang fp contract(off)
    const DevParams *P = D.P;
    const lg_traj_cfg &t = P->cfg.traj;
    float *s = P->buf.tg_state + (size_t)i * LG_TG_STRIDE;
    if (construct) {                                               // RD:495, once per tracker
        for (int q = 0; q < LG_TG_STRIDE; ++q) s[q] = 0.0f;
#pragma unroll
        for (int d = 0; d < 2; ++d)
            s[LG_TG_RAMP_V1 + d] = (t.v_max[d] - t.v_min[d]) * tg_uni(P, i, LG_RS_SLOT_RAMP + d, epoch << 32, D.inject) + t.v_min[d];
    }
    s[LG_TG_K] = -(float)(t.N * t.dN);
    s[LG_TG_T] = s[LG_TG_K] * t.rom_dt;
    s[LG_TG_T_FINAL] = s[LG_TG_K] * t.rom_dt;
    D.n_resample[i] = 0;
    ct_resample(D, i, epoch);
    float tt = s[LG_TG_T], k = s[LG_TG_K], v[2] = {0.0f, 0.0f};
    for (int it = 0; it < t.N * t.dN; ++it) {
        ct_input(D, i, tt, epoch, v);
        k += 1.0f;
        tt += t.rom_dt;
    }
    s[LG_TG_V] = v[0]; s[LG_TG_V + 1] = v[1];
    s[LG_TG_K] = k;
    s[LG_TG_T] = tt;
}

// wrap_angles: ((a + pi) mod 2 pi) - pi with Python's floor mod (fmod, then the divisor added to a negative remainder)
__device__ __forceinline__ float ct_wrap(float a) {
#pragma clang fp contract(off)
    const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
    float m = fmodf(a + pi, two_pi);
    if (m < 0.0f) m = m + two_pi;
    return m - pi;
}

// The ROM input of step t and the command it gives at the robot's pose (DV:112-141); both go into the env's state row, the
// command into obs (DV:144)
__device__ inline void ct_command(const CmdTrackDev &D, int i, int t, int64_t epoch, const float z[2], const float *__restrict__ root) {
#pragma clang fp contract(off)
    float v[2] = {0.0f, 0.0f};
    if (D.kind == LG_TG_KIND_RANDOM) ct_input(D, i, (float)t * D.rom_dt, epoch, v);
    else if (t < D.n_nodes) { v[0] = D.plan[((size_t)i * LG_PLAN_MAX_N + t) * 2]; v[1] = D.plan[((size_t)i * LG_PLAN_MAX_N + t) * 2 + 1]; }
    const float qx = root[3], qy = root[4], qz = root[5], qw = root[6];
    const float yaw = atan2f(2.0f * (qx * qy + qw * qz), ((qw * qw + qx * qx) - qy * qy) - qz * qz);
    const float c = cosf(yaw), s = sinf(yaw);
    const float e0 = z[0] - root[0], e1 = z[1] - root[1];
    const float e2 = D.track_yaw ? ct_wrap(atan2f(v[1], v[0]) - yaw) : 0.0f;
    const float el[3] = {c * e0 + s * e1, (-s) * e0 + c * e1, e2};
    const float vl[3] = {c * v[0] + s * v[1], (-s) * v[0] + c * v[1], 0.0f};
    float *st = D.state + (size_t)i * LG_CT_STATE;
    st[2] = v[0]; st[3] = v[1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float kp = (D.Kp[3 * j] * el[0] + D.Kp[3 * j + 1] * el[1]) + D.Kp[3 * j + 2] * el[2];
        const float u = fminf(fmaxf(vl[j] + kp, D.u_min[j]), D.u_max[j]);
        st[4 + j] = u;
        D.obs[(size_t)i * D.num_obs + D.cmd_col + j] = u * D.cmd_scale[j];
    }
}

// row r of pz_x (and x): the robot as the env left it; x in get_state()'s layout (base pose 7, joint positions, base twist 6,
// joint velocities), as k_traj_record writes it
__device__ inline void ct_robot_row(const CmdTrackDev &D, const lg_cmdtrack_rec &R, int i, int r, const float *__restrict__ root) {
    const size_t o = ((size_t)i * (R.T + 1) + r) * 2;
    R.pz_x[o] = root[0]; R.pz_x[o + 1] = root[1];
    if (R.x) {
        const int A = D.A;
        float *x = R.x + ((size_t)i * (R.T + 1) + r) * D.x_n;
        const float *d = D.dof + (size_t)i * A * 2;
        for (int k = 0; k < 7; ++k) x[k] = root[k];
        for (int a = 0; a < A; ++a) x[7 + a] = d[2 * a];
        for (int k = 0; k < 6; ++k) x[7 + A + k] = root[7 + k];
        for (int a = 0; a < A; ++a) x[13 + A + a] = d[2 * a + 1];
    }
}

// t < 0: the begin.  Otherwise the record of env step t (DV:149-156) and, if t + 1 < T, command t + 1.
__global__ __launch_bounds__(LG_CT_LANES) void k_cmdtrack(CmdTrackDev D, lg_cmdtrack_rec R, int t, int64_t epoch, int construct) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * LG_CT_LANES + threadIdx.x;
    if (i >= D.n) return;
    const float *root = D.root + (size_t)i * 13;
    float *st = D.state + (size_t)i * LG_CT_STATE;
    const size_t r1 = (size_t)i * (R.T + 1), r0 = (size_t)i * R.T;
    float z[2];
    if (t < 0) {
        if (D.kind == LG_TG_KIND_RANDOM) ct_gen_reset(D, i, epoch, construct);
        z[0] = root[0]; z[1] = root[1];
        R.z[r1 * 2] = z[0]; R.z[r1 * 2 + 1] = z[1];
        ct_robot_row(D, R, i, 0, root);
    } else {
        const bool done = D.reset[i] != 0;
        const float v0 = st[2], v1 = st[3];
        R.done[r0 + t] = done ? 1 : 0;
        R.v[(r0 + t) * 2] = v0; R.v[(r0 + t) * 2 + 1] = v1;
        if (R.u) {
#pragma unroll
            for (int j = 0; j < 3; ++j) R.u[(r0 + t) * 3 + j] = st[4 + j];
        }
        z[0] = st[0] + D.rom_dt * v0; z[1] = st[1] + D.rom_dt * v1;            // SingleInt2D.f
        if (done) { z[0] = root[0]; z[1] = root[1]; }                          // DV:155: a reset env restarts with zero tracking error
        R.z[(r1 + t + 1) * 2] = z[0]; R.z[(r1 + t + 1) * 2 + 1] = z[1];
        ct_robot_row(D, R, i, t + 1, root);
    }
    st[0] = z[0]; st[1] = z[1];
    if (t + 1 < R.T) ct_command(D, i, t + 1, epoch, z, root);
}

extern "C" void cmdtrackk_launch(const CmdTrackDev *D, const lg_cmdtrack_rec *rec, int t, int64_t epoch, int construct, hipStream_t st) {
    hipLaunchKernelGGL(k_cmdtrack, dim3((D->n + LG_CT_LANES - 1) / LG_CT_LANES), dim3(LG_CT_LANES), 0, st, *D, *rec, t, epoch, construct);
}
