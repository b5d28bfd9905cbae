// A fleet builds its own scenes on the device: for every robot the obstacle list of lg_plan_scenes -- its
// static obstacles advanced to the call's time, then its nearest neighbours as discs of radius `separation` that move with the
// neighbour's velocity.  One launch, no atomics, nothing read back.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "fleet_device.h"

// One lane per robot, one wave per workgroup: FLEET_NT robots walk over all P candidates, staged through LDS FLEET_CH positions at a
// time (a lane loads FLEET_CH / FLEET_NT of them), every lane reading the same candidate at the same time (an LDS broadcast).  A lane
// keeps its LG_PLAN_MAX_OBS best (d2, q) sorted ascending in registers -- the slots are indexed by unrolled loops alone, so there is
// no scratch -- and inserts a candidate by carrying it down the list, swapping wherever it orders before the slot.
constexpr int FLEET_NT = 64, FLEET_CH = 256;
static_assert(FLEET_CH % FLEET_NT == 0, "a lane loads whole positions of a chunk");

struct FleetDev {                       // passed by value
    lg_fleet_cfg cfg;
    const float *pos, *vel, *static_obs, *static_vel;
    const int32_t *n_static;
    float t;
    float *obs, *obs_vel;
    int32_t *n_obs;
    int64_t P;
};

__global__ void __launch_bounds__(FLEET_NT) k_fleet_scenes(FleetDev F) {
#pragma clang fp contract(off)
    __shared__ float cand[FLEET_CH * 2];
    constexpr int M = LG_PLAN_MAX_OBS;
    const int tid = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * FLEET_NT + tid;
    const bool on = p < F.P;
    const float px = on ? F.pos[p * 2] : 0.f, py = on ? F.pos[p * 2 + 1] : 0.f;
    const float s2 = F.cfg.sense_radius * F.cfg.sense_radius;
    float bd[M];
    int bq[M];
#pragma unroll
    for (int j = 0; j < M; ++j) { bd[j] = INFINITY; bq[j] = INT_MAX; }
    int found = 0;
    for (int64_t q0 = 0; q0 < F.P; q0 += FLEET_CH) {
        const int nc = (int)(F.P - q0 < FLEET_CH ? F.P - q0 : FLEET_CH);
        __syncthreads();                // the walk over the chunk before is done
        for (int e = tid; e < nc * 2; e += FLEET_NT) cand[e] = F.pos[q0 * 2 + e];
        __syncthreads();
        if (!on) continue;
        for (int c = 0; c < nc; ++c) {
            const float dx = cand[2 * c] - px, dy = cand[2 * c + 1] - py;
            float cd = dx * dx + dy * dy;
            int cq = (int)(q0 + c);
            if (!(cd <= s2) || !(cd < INFINITY) || (int64_t)cq == p) continue;      // a NaN or infinite d2 never passes
            found += found < M;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const bool before = cd < bd[j] || (cd == bd[j] && cq < bq[j]);
                const float td = bd[j];
                const int tq = bq[j];
                bd[j] = before ? cd : td; bq[j] = before ? cq : tq;
                cd = before ? td : cd; cq = before ? tq : cq;
            }
        }
    }
    if (!on) return;
    int ns = F.static_obs && F.n_static ? F.n_static[p] : 0;
    ns = ns < 0 ? 0 : (ns > M ? M : ns);
    int room = F.cfg.max_neighbours < M - ns ? F.cfg.max_neighbours : M - ns;
    room = room < 0 ? 0 : room;
    const int nn = found < room ? found : room;
    float *o = F.obs + p * (3 * M), *ov = F.obs_vel + p * (2 * M);
    for (int i = 0; i < M; ++i) {       // the static part; zeros in every slot past it
        float cx = 0.f, cy = 0.f, r = 0.f, ux = 0.f, uy = 0.f;
        if (i < ns) {
            const float *so = F.static_obs + p * (3 * M) + 3 * i;
            cx = so[0]; cy = so[1]; r = so[2];
            if (F.static_vel) {
                ux = F.static_vel[p * (2 * M) + 2 * i]; uy = F.static_vel[p * (2 * M) + 2 * i + 1];
                const float mx = ux * F.t, my = uy * F.t;
                cx = cx + mx; cy = cy + my;
            }
        }
        o[3 * i] = cx; o[3 * i + 1] = cy; o[3 * i + 2] = r;
        ov[2 * i] = ux; ov[2 * i + 1] = uy;
    }
#pragma unroll
    for (int j = 0; j < M; ++j) {       // the neighbours in (d2, q) order behind it: ns + j < M where j < nn
        if (j < nn) {
            const int64_t q = bq[j];
            const int i = ns + j;
            o[3 * i] = F.pos[q * 2]; o[3 * i + 1] = F.pos[q * 2 + 1]; o[3 * i + 2] = F.cfg.separation;
            ov[2 * i] = F.vel[q * 2]; ov[2 * i + 1] = F.vel[q * 2 + 1];
        }
    }
    F.n_obs[p] = ns + nn;
}

extern "C" void fleetk_scenes(const lg_fleet_cfg *cfg, const float *pos, const float *vel, int64_t P, const float *static_obs,
                              const float *static_vel, const int32_t *n_static, float t, float *obs, float *obs_vel, int32_t *n_obs,
                              hipStream_t s) {
    FleetDev F;
    F.cfg = *cfg; F.pos = pos; F.vel = vel; F.static_obs = static_obs; F.static_vel = static_vel; F.n_static = n_static; F.t = t;
    F.obs = obs; F.obs_vel = obs_vel; F.n_obs = n_obs; F.P = P;
    hipLaunchKernelGGL(k_fleet_scenes, dim3((unsigned)((P + FLEET_NT - 1) / FLEET_NT)), dim3(FLEET_NT), 0, s, F);
}
