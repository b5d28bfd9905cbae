// ROM-on-ROM simulator: the reference's CustomSim (deep_tube_learning/custom_sim.py, "CS") with its TrajectoryGenerator /
// SingleInt2D / DoubleInt2D (trajopt/rom_dynamics.py, "RD"), the DoubleSingleTracking law (deep_tube_learning/controllers.py:80-92,
// "CT") and the collection loop of deep_tube_learning/data_collection_trajectory.py:111-149 ("DC").
//
// One lane per env, workgroups of one wave.  An env step is a few dozen dependent flops on a handful of floats: in torch it is a
// hundred-odd launches, here the whole epoch -- reset, 2 T env steps, T records -- is ONE launch with the time loop inside
// (k_romsim_collect), as k_tube_rollout does for the tube model.  Reset, step and collect run the same device functions, every
// one of them with one rounding per torch op (fp contract off), so an env's records from the fused launch equal reset + repeated
// step bit for bit, whatever its lane or the number of envs.  The generator's laws are those of lg_traj.h (tg_resample, tg_input,
// tg_window_step, tg_window_interpolate), used as they are; what this simulator adds to them: the hold-time check on EVERY
// evaluation of the input (RD:561-562; the reset loop included, RD:604-605 -- hold times below N rom_dt are legal here), the
// window of inputs v_trajectory (RD:505,586-587) and the per-env resample count that keys the draws.
// The two windows live in LDS for the length of a launch (odd stride between lanes), the generator row stays in HBM where the
// lg_traj.h functions read it.  Everything written to memory is a plain C++ store.
#include "romsim_device.h"
#include "lg_traj.h"

// one reset draw (legged_hip.h LG_RS_SLOT_*): event 0 of the epoch
__device__ __forceinline__ float rs_uni(const RomSimDev &D, int i, int slot, int64_t epoch) {
    return tg_uni(D.P, i, slot, epoch << 32, D.inject);
}

// TrajectoryGenerator.resample (RD:510-520) of env i, keyed by the env's own resample count.  Injected: block r of the env's
// row; a missing block is counted (lg_romsim_inject_status) and the last one read again.
__device__ inline void rs_resample(const RomSimDev &D, int i, int64_t epoch) {
    const int r = D.n_resample[i];
    int slot0 = 0;
    if (D.inject) {
        int b = r;
        if (b >= D.R) { atomicAdd(D.overrun, 1); b = D.R - 1; }
        slot0 = LG_RS_NRESET + b * LG_TG_NDRAW;
    }
    tg_resample(D.P, tg_par_cfg(D.P), i, slot0, (epoch << 32) | (int64_t)(uint32_t)(r + 1), D.inject);
    D.n_resample[i] = r + 1;
}

// get_input_t (RD:560-566) + the stationary mask (RD:580): the hold time is checked on every evaluation
__device__ inline void rs_input(const RomSimDev &D, int i, float tt, int64_t epoch, float v[2]) {
    const float *s = D.P->buf.tg_state + (size_t)i * LG_TG_STRIDE;
    if (tt > s[LG_TG_T_FINAL]) rs_resample(D, i, epoch);
    tg_input(D.P, i, tt, v);
}

// RD:586-587: shift the input window by one point and append v
__device__ inline void rs_vwindow_step(const DevParams *P, float *__restrict__ vw, const float v[2]) {
    const int n2 = 2 * (P->cfg.traj.N * P->cfg.traj.dN);
    for (int p = 0; p < n2 - 2; ++p) vw[p] = vw[p + 2];
    vw[n2 - 2] = v[0]; vw[n2 - 1] = v[1];
}
__device__ inline void rs_vwindow_load(const RomSimDev &D, int i, float *__restrict__ vw) {
    const int n2 = 2 * (D.P->cfg.traj.N * D.P->cfg.traj.dN);
    for (int p = 0; p < n2; ++p) vw[p] = D.v_traj[(size_t)i * n2 + p];
}
__device__ inline void rs_vwindow_store(const RomSimDev &D, int i, const float *__restrict__ vw) {
    const int n2 = 2 * (D.P->cfg.traj.N * D.P->cfg.traj.dN);
    for (int p = 0; p < n2; ++p) D.v_traj[(size_t)i * n2 + p] = vw[p];
}

// CT:87-92 with DoubleInt2D.clip_v_z (RD:244-250): min with the upper bound first, then max with the lower
__device__ inline void rs_controller(const RomSimDev &D, const float o[LG_RS_NOBS], float a[2]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float u = D.Kp * (o[4 + d] - o[d]) + D.Kd * (o[6 + d] - o[2 + d]);
        const float hi = fminf(D.acc_max[d], (D.vel_max[d] - o[2 + d]) / D.dt);
        const float lo = fmaxf(D.acc_min[d], (D.vel_min[d] - o[2 + d]) / D.dt);
        a[d] = fmaxf(fminf(u, hi), lo);
    }
}

// CustomSim.step (CS:71-75) + get_observations (CS:95-100).  x: root_states of the env; w / vw: its windows.
__device__ inline void rs_env_step(const RomSimDev &D, int i, int64_t epoch, float *__restrict__ w, float *__restrict__ vw,
                                   float x[4], const float a[2], float o[LG_RS_NOBS]) {
#pragma clang fp contract(off)      // one rounding per torch op: the event comparisons below must agree with the reference
    const DevParams *P = D.P;
    const lg_traj_cfg &t = P->cfg.traj;
    // DoubleInt2D.f (RD:224-225): the 4 x 4 matmul written out
    const float px = x[0] + D.dt * x[2], py = x[1] + D.dt * x[3];
    x[2] = x[2] + D.dt * a[0]; x[3] = x[3] + D.dt * a[1];
    x[0] = px; x[1] = py;
    // traj_gen.step() (RD:568-590): the ROM steps where t >= k rom_dt - 1e-5; the input is evaluated for every env
    float *s = P->buf.tg_state + (size_t)i * LG_TG_STRIDE;
    const float tt = s[LG_TG_T];
    float v[2];
    rs_input(D, i, tt, epoch, v);
    float k = s[LG_TG_K];
    if (tt >= k * t.rom_dt - 1e-5f) { tg_window_step(P, w, v); rs_vwindow_step(P, vw, v); k += 1.0f; }
    const float tn = tt + P->cfg.dt;
    s[LG_TG_V] = v[0]; s[LG_TG_V + 1] = v[1];
    s[LG_TG_K] = k;
    s[LG_TG_T] = tn;
    tg_window_interpolate(P, i, w, tn, k);                         // CS:74 trajectory = get_trajectory()
    const float *tr = P->buf.trajectory + (size_t)i * t.N * 2;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = x[d];
    o[4] = tr[0]; o[5] = tr[1];
    o[6] = vw[2]; o[7] = vw[3];                                    // v_trajectory[:, 1, :]
}

// CustomSim.reset_idx (CS:87-93) with reset_traj (CS:80-85) and TrajectoryGenerator.reset_idx (RD:595-605)
__device__ inline void rs_reset(const RomSimDev &D, int i, int64_t epoch, int construct, float *__restrict__ w,
                                float *__restrict__ vw, float x[4], float o[LG_RS_NOBS]) {
#pragma clang fp contract(off)
    const DevParams *P = D.P;
    const lg_traj_cfg &t = P->cfg.traj;
    float *s = P->buf.tg_state + (size_t)i * LG_TG_STRIDE;
    if (construct) {                                               // RD:495, once per simulator
        for (int q = 0; q < LG_TG_STRIDE; ++q) s[q] = 0.0f;
#pragma unroll
        for (int d = 0; d < 2; ++d) s[LG_TG_RAMP_V1 + d] = (t.v_max[d] - t.v_min[d]) * rs_uni(D, i, LG_RS_SLOT_RAMP + d, epoch) + t.v_min[d];
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = (D.noise_hi[d] - D.noise_lo[d]) * rs_uni(D, i, LG_RS_SLOT_ROOT + d, epoch) + D.noise_lo[d];
    float z0[2] = {x[0], x[1]};                                    // rom.proj_z
    if (D.rand_dist && rs_uni(D, i, LG_RS_SLOT_MASK, epoch) > D.llh) {
#pragma unroll
        for (int d = 0; d < 2; ++d) z0[d] += (D.max_dist[d] - (-D.max_dist[d])) * rs_uni(D, i, LG_RS_SLOT_DIST + d, epoch) + (-D.max_dist[d]);
    }
    const int npts = t.N * t.dN + 1;
    for (int p = 0; p < 2 * (npts - 1); ++p) { w[p] = 0.0f; vw[p] = 0.0f; }
    w[2 * (npts - 1)] = z0[0]; w[2 * (npts - 1) + 1] = z0[1];
    s[LG_TG_K] = -(float)(t.N * t.dN);
    s[LG_TG_T] = s[LG_TG_K] * t.rom_dt;
    s[LG_TG_T_FINAL] = s[LG_TG_K] * t.rom_dt;
    D.n_resample[i] = 0;
    rs_resample(D, i, epoch);
    float tt = s[LG_TG_T], k = s[LG_TG_K], v[2] = {0.0f, 0.0f};
    for (int it = 0; it < t.N * t.dN; ++it) {                      // step_rom_idx(idx, increment_rom_time=True)
        rs_input(D, i, tt, epoch, v);
        tg_window_step(P, w, v);
        rs_vwindow_step(P, vw, v);
        k += 1.0f;
        tt += t.rom_dt;
    }
    s[LG_TG_V] = v[0]; s[LG_TG_V + 1] = v[1];
    s[LG_TG_K] = k;
    s[LG_TG_T] = tt;
    const float zero[2] = {0.0f, 0.0f};
    rs_env_step(D, i, epoch, w, vw, x, zero, o);                   // CS:93
}

// the env's state leaves the launch: root_states, observation, last action, both windows
__device__ inline void rs_store(const RomSimDev &D, int i, const float *__restrict__ w, const float *__restrict__ vw, const float x[4],
                                const float a[2], const float o[LG_RS_NOBS]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) D.root[(size_t)i * 4 + d] = x[d];
#pragma unroll
    for (int d = 0; d < LG_RS_NOBS; ++d) D.obs[(size_t)i * LG_RS_NOBS + d] = o[d];
    D.act[(size_t)i * 2] = a[0]; D.act[(size_t)i * 2 + 1] = a[1];
    tg_window_store(D.P, i, w);
    rs_vwindow_store(D, i, vw);
}

__global__ __launch_bounds__(LG_RS_LANES) void k_romsim_reset(RomSimDev D, int64_t epoch, int construct) {
    __shared__ float lds[LG_RS_LANES * LG_RS_LDS_STRIDE];
    const int i = blockIdx.x * LG_RS_LANES + threadIdx.x;
    if (i >= D.n) return;
    float *w = lds + threadIdx.x * LG_RS_LDS_STRIDE, *vw = w + LG_TG_WIN;
    float x[4], o[LG_RS_NOBS];
    const float zero[2] = {0.0f, 0.0f};
    rs_reset(D, i, epoch, construct, w, vw, x, o);
    rs_store(D, i, w, vw, x, zero, o);
}

__global__ __launch_bounds__(LG_RS_LANES) void k_romsim_step(RomSimDev D, int64_t epoch, const float *__restrict__ actions) {
    __shared__ float lds[LG_RS_LANES * LG_RS_LDS_STRIDE];
    const int i = blockIdx.x * LG_RS_LANES + threadIdx.x;
    if (i >= D.n) return;
    float *w = lds + threadIdx.x * LG_RS_LDS_STRIDE, *vw = w + LG_TG_WIN;
    float x[4], o[LG_RS_NOBS], a[2];
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = D.root[(size_t)i * 4 + d];
#pragma unroll
    for (int d = 0; d < LG_RS_NOBS; ++d) o[d] = D.obs[(size_t)i * LG_RS_NOBS + d];
    if (actions) { a[0] = actions[(size_t)i * 2]; a[1] = actions[(size_t)i * 2 + 1]; }
    else rs_controller(D, o, a);
    tg_window_load(D.P, i, w);
    rs_vwindow_load(D, i, vw);
    rs_env_step(D, i, epoch, w, vw, x, a, o);
    rs_store(D, i, w, vw, x, a, o);
}

__global__ __launch_bounds__(256) void k_romsim_policy(RomSimDev D, const float *__restrict__ obs, float *__restrict__ out, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    float o[LG_RS_NOBS], a[2];
#pragma unroll
    for (int d = 0; d < LG_RS_NOBS; ++d) o[d] = obs[i * LG_RS_NOBS + d];
    rs_controller(D, o, a);
    out[i * 2] = a[0]; out[i * 2 + 1] = a[1];
}

// DC:111-149.  max_sub bounds the env steps of one record (ceil(rom_dt / dt) + 2: k advances within that many, the bound only
// keeps a broken clock from spinning).  A lane's record stores are 8 bytes at a stride of (T + 1) 8: per-env rows, as the
// reference lays them out.
__global__ __launch_bounds__(LG_RS_LANES) void k_romsim_collect(RomSimDev D, int64_t epoch, int construct, int T, int max_sub,
                                                                float *__restrict__ z, float *__restrict__ v, float *__restrict__ pz,
                                                                uint8_t *__restrict__ done, float *__restrict__ xo) {
    __shared__ float lds[LG_RS_LANES * LG_RS_LDS_STRIDE];
    const int i = blockIdx.x * LG_RS_LANES + threadIdx.x;
    if (i >= D.n) return;
    float *w = lds + threadIdx.x * LG_RS_LDS_STRIDE, *vw = w + LG_TG_WIN;
    float x[4], o[LG_RS_NOBS], a[2] = {0.0f, 0.0f};
    rs_reset(D, i, epoch, construct, w, vw, x, o);
    const float *s = D.P->buf.tg_state + (size_t)i * LG_TG_STRIDE;
    const size_t r1 = (size_t)i * (T + 1), r0 = (size_t)i * T;
    z[r1 * 2] = w[0]; z[r1 * 2 + 1] = w[1];                        // DC:116: the raw window's point 0
    pz[r1 * 2] = x[0]; pz[r1 * 2 + 1] = x[1];
    if (xo) {
#pragma unroll
        for (int d = 0; d < 4; ++d) xo[r1 * 4 + d] = x[d];
    }
    for (int t = 0; t < T; ++t) {
        const float k0 = s[LG_TG_K];
        for (int it = 0; it < max_sub && s[LG_TG_K] == k0; ++it) {
            rs_controller(D, o, a);
            rs_env_step(D, i, epoch, w, vw, x, a, o);
        }
        v[(r0 + t) * 2] = s[LG_TG_V]; v[(r0 + t) * 2 + 1] = s[LG_TG_V + 1];
        z[(r1 + t + 1) * 2] = o[4]; z[(r1 + t + 1) * 2 + 1] = o[5];
        pz[(r1 + t + 1) * 2] = x[0]; pz[(r1 + t + 1) * 2 + 1] = x[1];
        if (xo) {
#pragma unroll
            for (int d = 0; d < 4; ++d) xo[(r1 + t + 1) * 4 + d] = x[d];
        }
        done[r0 + t] = 0;
    }
    rs_store(D, i, w, vw, x, a, o);
}

// Track B prescribed plans: the loop of deep_tube_learning/evaluation/
// evaluate_tube_simple_oneshot_on_mpc_traj.py:75-88 ("MT") with S model steps per node.  One lane per plan, as k_romsim_collect has
// one per env; the law is rs_controller and the model the DoubleInt2D.f lines of rs_env_step, one rounding per op.  Nothing of the
// simulator's own state is read or written: D supplies Kp, Kd, the bounds and the model dt.
__global__ __launch_bounds__(LG_RS_LANES) void k_plan_track(RomSimDev D, const float *__restrict__ z, const float *__restrict__ v,
                                                            const float *__restrict__ x0, int64_t B, int N, int S, float rom_dt,
                                                            float *__restrict__ pz, float *__restrict__ wt, float *__restrict__ xo,
                                                            float *__restrict__ uo) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * LG_RS_LANES + threadIdx.x;
    if (i >= B) return;
    const float *zi = z + i * (N + 1) * 2, *vi = v + i * N * 2;
    float x[4], o[LG_RS_NOBS], a[2];
    if (x0) {
#pragma unroll
        for (int d = 0; d < 4; ++d) x[d] = x0[i * 4 + d];
    } else { x[0] = zi[0]; x[1] = zi[1]; x[2] = 0.0f; x[3] = 0.0f; }
    const int64_t r1 = i * (N + 1);
    for (int t = 0; t <= N; ++t) {
        // the record of node t: proj_z (MT:88) and the error norm (MT:90), sqrtf of the squares summed in column order
        const float ex = x[0] - zi[2 * t], ey = x[1] - zi[2 * t + 1];
        float s2 = 0.0f;
        s2 = s2 + ex * ex; s2 = s2 + ey * ey;
        pz[(r1 + t) * 2] = x[0]; pz[(r1 + t) * 2 + 1] = x[1];
        wt[r1 + t] = sqrtf(s2);
        if (xo) {
#pragma unroll
            for (int d = 0; d < 4; ++d) xo[(r1 + t) * 4 + d] = x[d];
        }
        if (t == N) break;
        const int tf = t + 1 < N ? t + 1 : N - 1;                   // MT:80
        const float za[2] = {zi[2 * t], zi[2 * t + 1]}, zb[2] = {zi[2 * t + 2], zi[2 * t + 3]};
        for (int s = 0; s < S; ++s) {
            const float frac = ((float)s * D.dt) / rom_dt;
#pragma unroll
            for (int d = 0; d < 4; ++d) o[d] = x[d];
            o[4] = za[0] + (zb[0] - za[0]) * frac; o[5] = za[1] + (zb[1] - za[1]) * frac;
            o[6] = vi[2 * tf]; o[7] = vi[2 * tf + 1];
            rs_controller(D, o, a);                                 // MT:81
            // DoubleInt2D.f (RD:224-225), as rs_env_step writes it out
            const float px = x[0] + D.dt * x[2], py = x[1] + D.dt * x[3];
            x[2] = x[2] + D.dt * a[0]; x[3] = x[3] + D.dt * a[1];
            x[0] = px; x[1] = py;
            if (uo) { uo[(i * N * S + (int64_t)t * S + s) * 2] = a[0]; uo[(i * N * S + (int64_t)t * S + s) * 2 + 1] = a[1]; }
        }
    }
}

extern "C" {
void romsimk_plan_track(const RomSimDev *D, const float *z, const float *v, const float *x0, int64_t B, int N, int S, float rom_dt,
                        float *pz, float *wt, float *x, float *u, hipStream_t st) {
    hipLaunchKernelGGL(k_plan_track, dim3((unsigned)((B + LG_RS_LANES - 1) / LG_RS_LANES)), dim3(LG_RS_LANES), 0, st, *D, z, v, x0, B, N,
                       S, rom_dt, pz, wt, x, u);
}
void romsimk_reset(const RomSimDev *D, int64_t epoch, int construct, hipStream_t st) {
    hipLaunchKernelGGL(k_romsim_reset, dim3((D->n + LG_RS_LANES - 1) / LG_RS_LANES), dim3(LG_RS_LANES), 0, st, *D, epoch, construct);
}
void romsimk_step(const RomSimDev *D, int64_t epoch, const float *actions, hipStream_t st) {
    hipLaunchKernelGGL(k_romsim_step, dim3((D->n + LG_RS_LANES - 1) / LG_RS_LANES), dim3(LG_RS_LANES), 0, st, *D, epoch, actions);
}
void romsimk_policy(const RomSimDev *D, const float *obs, float *out, int64_t rows, hipStream_t st) {
    hipLaunchKernelGGL(k_romsim_policy, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *D, obs, out, rows);
}
void romsimk_collect(const RomSimDev *D, int64_t epoch, int construct, int T, int max_sub, float *z, float *v, float *pz,
                     uint8_t *done, float *x, hipStream_t st) {
    hipLaunchKernelGGL(k_romsim_collect, dim3((D->n + LG_RS_LANES - 1) / LG_RS_LANES), dim3(LG_RS_LANES), 0, st, *D, epoch, construct,
                       T, max_sub, z, v, pz, done, x);
}
}
