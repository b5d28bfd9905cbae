// The launch of fleet_kernels.hip, as fleet_api.hip calls it (legged_hip.h lg_plan_fleet_scenes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/legged_hip.h"

extern "C" {
void fleetk_scenes(const lg_fleet_cfg *cfg, const float *pos, const float *vel, int64_t P, const float *static_obs, const float *static_vel,
                   const int32_t *n_static, float t, float *obs, float *obs_vel, int32_t *n_obs, hipStream_t s);
}
