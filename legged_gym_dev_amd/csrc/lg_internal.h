// What one source file of the library defines for the others: same library, not in the header (include/legged_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/legged_hip.h"

struct DevParams;                       // lg_device.h
struct TubeDev;                         // tube_device.h

// env_api.hip: the calling thread's message, what lg_last_error returns
void lg_set_error(const std::string &s);

extern "C" {
// env_api.hip: the env's stream and host-side parameters, for the handles that borrow its buffers for a call
hipStream_t lg_internal_stream(lg_ctx *c);
const DevParams *lg_internal_host_params(lg_ctx *c);
// env_api.hip: env side of the learner's fused rollout epilogue (lg_ppo_attach_env)
void lg_internal_defer_finalize(lg_ctx *c, int on);
int lg_internal_finalize_pending(lg_ctx *c);
const DevParams *lg_internal_take_finalize(lg_ctx *c, int64_t *counter);
// tube_api.hip: all the planner reads of a tube handle.  Null for a null handle
const TubeDev *lg_internal_tube_dev(const lg_tube *t);
// comm_api.cpp: the learner's overlapped per-layer gradient reduction
hipStream_t lg_comm_stream_(lg_comm *c);
hipEvent_t lg_comm_event_(lg_comm *c);
int lg_comm_group_allreduce_(lg_comm *c, float *const *bufs, const int64_t *counts, int n, hipStream_t s);
}
