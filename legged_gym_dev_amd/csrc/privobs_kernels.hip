// Privileged observations: the critic's own row, gathered from the env's buffers in ONE launch after the step (legged_hip.h
// lg_priv_obs_*; the buffer of the reference's base_task.py:62-79 / legged_robot.py:100-104, which nothing there fills).
//
// Memory- and launch-bound: at 4096 envs a row of a few dozen to a few hundred floats, read once and written once, no Philox and no
// reward work.  A workgroup owns LG_PO_TILE envs and walks the row term by term -- the term comes from the kernel arguments, so the
// branch on its kind is uniform over the whole workgroup -- and inside a term lanes run along (env, column) of the tile: the
// source rows of a tile are contiguous in every env buffer, so the loads coalesce, and the stores fill each env's segment of the
// (n, W) row in order.  fp32, one rounding per operation (fp contract off), so the row can be restated bit for bit.  Plain loads
// and stores only: no LDS, no atomics, and an env's row depends neither on its lane nor on the number of envs.
#include "privobs_device.h"

// every entry: raw * scale, clipped as obs is (legged_robot.py:100-103)
__device__ __forceinline__ void po_put(const PrivObsDev &D, float *__restrict__ seg, int e, int j, float scale, float raw) {
#pragma clang fp contract(off)
    seg[(size_t)e * D.W + j] = clampf(raw * scale, -D.clip, D.clip);
}

// lanes over (env, column) of one segment of width w: idx -> env e of the tile, column j
#define PO_SEG(w) for (int idx = threadIdx.x, e = idx / (w), j = idx - e * (w); idx < nE * (w); idx += LG_PO_THREADS, e = idx / (w), j = idx - e * (w))

// The observation before noise, with the expressions of the post-step's phase O (env_kernels.hip) operation for operation:
// base_lin_vel, base_ang_vel, projected_gravity, commands[:3] | (trajectory - root xy) obs_scale; (q - default) s, qdot s, actions
__device__ inline void po_obs_state(const PrivObsDev &D, float *__restrict__ seg, int env0, int nE, float scale) {
#pragma clang fp contract(off)
    const int A = D.A, ob = D.traj_N ? 9 + 2 * D.traj_N : 12;
    PO_SEG(ob) {
        const int i = env0 + e, k = j;
        float v;
        if (k < 9) {
            const float *src = k < 3 ? D.base_lin_vel : k < 6 ? D.base_ang_vel : D.projected_gravity;
            v = src[3 * (size_t)i + k % 3] * (k < 3 ? D.s_lin_vel : k < 6 ? D.s_ang_vel : 1.0f);
        } else if (D.traj_N) {
            v = (D.trajectory[(size_t)i * 2 * D.traj_N + (k - 9)] - D.root[(size_t)i * 13 + ((k - 9) & 1)]) * D.s_traj[(k - 9) & 1];
        } else {
            v = D.commands[(size_t)i * 4 + k - 9] * (k == 11 ? D.s_ang_vel : D.s_lin_vel);
        }
        po_put(D, seg, e, k, scale, v);
    }
    PO_SEG(A) {
        const int i = env0 + e;
        const float2 st = reinterpret_cast<const float2 *>(D.dof)[(size_t)i * A + j];
        const float act = D.actions[(size_t)i * A + j];
        po_put(D, seg, e, ob + j, scale, (st.x - D.default_dof_pos[j]) * D.s_dof_pos);
        po_put(D, seg, e, ob + A + j, scale, st.y * D.s_dof_vel);
        po_put(D, seg, e, ob + 2 * A + j, scale, act);
    }
}

// the height block: clip(root_z - 0.5 - measured_heights, -1, 1) s (legged_robot.py:222-224)
__device__ inline void po_heights(const PrivObsDev &D, float *__restrict__ seg, int env0, int nE, float scale) {
#pragma clang fp contract(off)
    const int H = D.H;
    PO_SEG(H) {
        const int i = env0 + e;
        const float hv = D.measured_heights[(size_t)i * H + j], rz = D.root[(size_t)i * 13 + 2];
        po_put(D, seg, e, j, scale, clampf(rz - 0.5f - hv, -1.0f, 1.0f) * D.s_height);
    }
}

// a per-env buffer of w floats per env, as it is
__device__ inline void po_copy(const PrivObsDev &D, float *__restrict__ seg, int env0, int nE, float scale, const float *__restrict__ src, int w) {
    PO_SEG(w) po_put(D, seg, e, j, scale, src[(size_t)env0 * w + idx]);
}

__global__ __launch_bounds__(LG_PO_THREADS) void k_priv_obs(PrivObsDev D) {
#pragma clang fp contract(off)
    const int env0 = (int)blockIdx.x * LG_PO_TILE;
    const int nE = min(LG_PO_TILE, D.n - env0);
    for (int t = 0; t < D.num_terms; ++t) {
        const PrivTermDev T = D.terms[t];
        float *seg = D.out + (size_t)env0 * D.W + T.off;
        switch (T.kind) {
        case LG_PRIV_OBS:
            po_obs_state(D, seg, env0, nE, T.scale);
            if (D.H > 0) po_heights(D, seg + (D.O - D.H), env0, nE, T.scale);
            break;
        case LG_PRIV_FRICTION: po_copy(D, seg, env0, nE, T.scale, D.friction, 1); break;
        case LG_PRIV_BASE_MASS: po_copy(D, seg, env0, nE, T.scale, D.base_mass_delta, 1); break;
        case LG_PRIV_MATERIAL: po_copy(D, seg, env0, nE, T.scale, D.material, 4); break;
        case LG_PRIV_FEET_AIR_TIME: po_copy(D, seg, env0, nE, T.scale, D.feet_air_time, D.F); break;
        case LG_PRIV_TORQUES: po_copy(D, seg, env0, nE, T.scale, D.torques, D.A); break;
        case LG_PRIV_HEIGHTS: po_heights(D, seg, env0, nE, T.scale); break;
        case LG_PRIV_FEET_CONTACT_FORCES: {
            const int w = 3 * D.F;
            PO_SEG(w) po_put(D, seg, e, j, T.scale, D.cf[((size_t)(env0 + e) * D.B + D.feet_idx[j / 3]) * 3 + j % 3]);
            break;
        }
        case LG_PRIV_FEET_CONTACT: {
            const int w = D.F;
            PO_SEG(w) po_put(D, seg, e, j, T.scale, D.cf[((size_t)(env0 + e) * D.B + D.feet_idx[j]) * 3 + 2] > 1.0f ? 1.0f : 0.0f);
            break;
        }
        case LG_PRIV_BODY_CONTACT: {
            const int w = D.NP;
            PO_SEG(w) {
                const float *f = D.cf + ((size_t)(env0 + e) * D.B + D.pen_idx[j]) * 3;
                const float fx = f[0], fy = f[1], fz = f[2];
                po_put(D, seg, e, j, T.scale, fx * fx + fy * fy + fz * fz > 0.01f ? 1.0f : 0.0f);
            }
            break;
        }
        case LG_PRIV_EPISODE_PROGRESS: {
            PO_SEG(1) po_put(D, seg, e, j, T.scale, (float)D.episode_length[env0 + e] * D.inv_max_len);
            break;
        }
        default: break;                                            // lg_priv_obs_check admits no other kind
        }
    }
}

extern "C" void privobsk_launch(const PrivObsDev *D, hipStream_t st) {
    hipLaunchKernelGGL(k_priv_obs, dim3((D->n + LG_PO_TILE - 1) / LG_PO_TILE), dim3(LG_PO_THREADS), 0, st, *D);
}
