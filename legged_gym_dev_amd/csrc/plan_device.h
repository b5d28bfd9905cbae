// Argument structs of the planner launchers (plan_kernels.hip), filled by tube_api.hip; every array a device pointer.
#pragma once
#include "tube_device.h"

struct PlanArgs {                       // what every planner launch takes; a launch reads the outputs its kernel has and no others
    const float *z0, *v, *e, *v_prev, *w0, *offset;     // v: (B, N, 2) the plans (the sampling planner draws its own)
    float level;                        // 0 where the handle takes none
    float *cost, *min_clear, *fw, *z, *w;
    int32_t *worst_node, *n_viol;
    const lg_plan_scenes *scenes;       // per-plan scenes, or null
};

struct PlanGradArgs {                   // one launch of k_plan_grad
    PlanArgs plan;                      // cost and min_clear optional; the outputs past them are not written
    float *v;                           // plan.v where the step writes it (step), else unused
    float *J, *grad, *pen;              // J required; the rest optional
    float *m, *s, *best_J, *best_v, *hist;     // Adam moments (step); elite and history row (optional)
    int32_t *n_bad;
    int step, reset;                    // step: the optimiser tail runs; reset: moments, elite and n_bad start afresh
    float lr, beta1, beta2, eps, bc1, bc2;     // bc = 1 - beta^t of the launch's step index t, rounded once from double
    float rho_g, rho_w, rho_z;
};

extern "C" {
// plan_kernels.hip.  D: the handle's TubeDev, or null for an analytic kind
int64_t tubek_plan_score(const TubeDev *D, const lg_plan_problem *prob, const PlanArgs *A, int64_t B, hipStream_t s);
int64_t tubek_plan_score_step(const TubeDev *D, const lg_plan_problem *prob, const PlanArgs *A, int64_t B, hipStream_t s);
void tubek_plan_mppi_candidates(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const float *vbar, int64_t P_, float *out,
                                hipStream_t s);
int64_t tubek_plan_sample_score(const TubeDev *D, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const PlanArgs *A, int64_t P_,
                                const float *vbar, float *J, float *pen, hipStream_t s);
int64_t tubek_plan_sample_score_step(const TubeDev *D, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const PlanArgs *A,
                                     int64_t P_, const float *vbar, float *J, float *pen, hipStream_t s);
void tubek_plan_mppi_update(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, int reset, int64_t P_, float *vbar,
                            const float *J, float *best_J, float *best_v, float *hist, int32_t *n_bad, hipStream_t s);
int64_t tubek_plan_grad(const TubeDev *D, const lg_plan_problem *prob, const PlanGradArgs *A, int64_t B, hipStream_t s);
int64_t tubek_plan_step_bytes(const TubeDev *D, const lg_plan_problem *prob);
}
