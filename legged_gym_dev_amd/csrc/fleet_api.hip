// C-ABI (include/legged_hip.h, lg_plan_fleet_scenes) of the fleet's scenes: the argument checks, which are
// host code and come before a device is touched, and the one launch of fleet_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "fleet_device.h"
#include "lg_internal.h"

extern "C" {
int lg_plan_fleet_scenes(const lg_fleet_cfg *cfg, const float *pos, const float *vel, int64_t P, const float *static_obs,
                         const float *static_vel, const int32_t *n_static, float t, float *obs, float *obs_vel, int32_t *n_obs,
                         void *stream) {
    std::string e;
    if (!cfg) e = "cfg is null";
    else if (!(cfg->separation >= 0.f) || !std::isfinite(cfg->separation)) e = "separation must be finite and not negative";
    else if (!(cfg->sense_radius >= 0.f) || !std::isfinite(cfg->sense_radius)) e = "sense_radius must be finite and not negative";
    else if (cfg->max_neighbours < 0 || cfg->max_neighbours > LG_PLAN_MAX_OBS)
        e = "max_neighbours = " + std::to_string(cfg->max_neighbours) + " must lie in 0.." + std::to_string(LG_PLAN_MAX_OBS);
    else if (P < 1 || P > INT32_MAX) e = "P = " + std::to_string(P) + " must be 1..2^31-1";
    else if (!pos || !vel || !obs || !obs_vel || !n_obs) e = "missing array (pos, vel, obs, obs_vel and n_obs are required)";
    else if ((static_obs == nullptr) != (n_static == nullptr)) e = "static_obs and n_static are given together or not at all";
    else if (static_vel && !static_obs) e = "static_vel is given without static_obs";
    else if (!std::isfinite(t)) e = "t must be finite";
    if (!e.empty()) { lg_set_error("lg_plan_fleet_scenes: " + e); return -1; }
    fleetk_scenes(cfg, pos, vel, P, static_obs, static_vel, n_static, t, obs, obs_vel, n_obs, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_fleet_scenes: launch failed"), -3);
}
}
