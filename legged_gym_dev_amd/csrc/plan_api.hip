// C-ABI (include/legged_hip.h, lg_plan_* and lg_mppi_*) of the planners on a tube.  The entries launch plan_kernels.hip through the
// argument structs of plan_device.h; an lg_plan_call says what every launch reads, and plan_args() is where it becomes PlanArgs.
// lg_plan_check / lg_plan_score: plans scored against a one-shot horizon handle or an analytic tube (k_plan_score).
// The same entry points take the one-step kind LG_PLAN_TUBE_NN_STEP (k_plan_score_step, k_plan_sample_score_step; section 10.13).
// lg_mppi_check / lg_plan_mppi*: the sampling planner on top of it (k_plan_sample_score, k_plan_mppi_update).
// lg_plan_grad_check / lg_plan_grad / lg_plan_descend*: the gradient planner (k_plan_grad).
// lg_plan_scenes_check: per-plan scenes (section 10.14).  Of a tube handle only its TubeDev is read.
#include <cmath>
#include <cstring>
#include <string>

#include "plan_device.h"
#include "lg_internal.h"

// ---------------------------------------------------------------- plans against a tube
// Taps of a one-step handle: with I' = input_dim minus the level column, I' = 1 + 2 T (not recursive) or
// 3 T (recursive); 0 where I' fits the form asked for in no T >= 1.
static int plan_step_taps(const TubeDev &D, int recursive) {
    const int Ip = D.in_dim - (D.level_input ? 1 : 0);
    if (recursive) return Ip >= 3 && Ip % 3 == 0 ? Ip / 3 : 0;
    return Ip >= 3 && (Ip - 1) % 2 == 0 ? (Ip - 1) / 2 : 0;
}
// the envelope of LG_PLAN_TUBE_NN_STEP beyond the problem's own fields
static std::string plan_step_reason(const lg_plan_problem *q, const TubeDev *t, int32_t has_level) {
    if (!t) return "tube_kind nn_step needs a tube handle";
    const TubeDev &D = *t;
    if (D.horizon) return "the tube handle is a horizon handle (lg_tube_cfg.horizon): nn_step rolls a flat one-step tube along the plan";
    if (D.out_dim != 1) return "the handle's output_dim = " + std::to_string(D.out_dim) + " must be 1: nn_step rolls a scalar tube";
    if (q->recursive != 0 && q->recursive != 1) return "recursive = " + std::to_string(q->recursive) + " must be 0 or 1";
    const int T = plan_step_taps(D, q->recursive);
    if (!T)
        return "the handle's input_dim = " + std::to_string(D.in_dim) + (D.level_input ? " (one of them the level)" : "") + " with recursive = " +
               std::to_string(q->recursive) + " is not " + (q->recursive ? "3 T" : "1 + 2 T") + (D.level_input ? " + 1" : "") +
               " for any T >= 1 (the ROM is SingleInt2D: no state columns past the position)";
    if (q->H_rev < 0 || q->H_rev > LG_PLAN_STEP_MAX_HREV || q->H_rev < T - 1)
        return "H_rev = " + std::to_string(q->H_rev) + " must be 0.." + std::to_string(LG_PLAN_STEP_MAX_HREV) + " and at least T - 1 = " +
               std::to_string(T - 1) + ": the delayed taps of node 0 come from e and v_prev";
    if (tubek_plan_step_bytes(&D, q) > (int64_t)LG_TUBE_ROLLOUT_LDS)
        return "the tile of input_dim = " + std::to_string(D.in_dim) + ", " + std::to_string(D.units) + " units, H_rev = " +
               std::to_string(q->H_rev) + " and N = " + std::to_string(q->N) + " does not fit the dynamic LDS ceiling";
    if (has_level && !D.level_input) return "level is given, but the handle is not level-conditioned (lg_tube_cfg.level_input)";
    if (!has_level && D.level_input) return "level is missing: the handle is level-conditioned (lg_tube_cfg.level_input)";
    return "";
}

// why a problem, with the handle it is asked with, lies outside the envelope; empty inside it
static std::string plan_reason(const lg_plan_problem *q, const TubeDev *t, int32_t has_level) {
    if (q->N < 1 || q->N > LG_PLAN_MAX_N) return "N = " + std::to_string(q->N) + " must be 1.." + std::to_string(LG_PLAN_MAX_N);
    if (q->n_obs < 0 || q->n_obs > LG_PLAN_MAX_OBS) return "n_obs = " + std::to_string(q->n_obs) + " must be 0.." + std::to_string(LG_PLAN_MAX_OBS);
    if (!(q->dt > 0.f)) return "dt must be positive";
    for (int i = 0; i < q->n_obs; ++i)
        if (!(q->obs_r[i] >= 0.f)) return "obs_r[" + std::to_string(i) + "] is negative";
    if (q->tube_kind < LG_PLAN_TUBE_NN || q->tube_kind > LG_PLAN_TUBE_NN_STEP)
        return "tube_kind must be nn (0), l1, l2, l1_rolling, l2_rolling (1..4) or nn_step (5)";
    if ((q->tube_kind == LG_PLAN_TUBE_L1_ROLLING || q->tube_kind == LG_PLAN_TUBE_L2_ROLLING) && q->window_size < 1)
        return "window_size must be at least 1 for a rolling tube_kind";
    if (q->tube_kind == LG_PLAN_TUBE_NN_STEP) return plan_step_reason(q, t, has_level);
    if (q->tube_kind != LG_PLAN_TUBE_NN) return has_level ? "level is given, but an analytic tube_kind has none" : "";
    if (!t) return "tube_kind nn needs a tube handle";
    const TubeDev &D = *t;
    if (!D.horizon) return "the tube handle is not a horizon handle (lg_tube_cfg.horizon): a plan is scored by a one-shot tube";
    if (D.H_fwd != q->N) return "the handle's H_fwd = " + std::to_string(D.H_fwd) + " differs from N = " + std::to_string(q->N);
    if (D.H_rev != q->H_rev) return "the handle's H_rev = " + std::to_string(D.H_rev) + " differs from the problem's H_rev = " + std::to_string(q->H_rev);
    if (window_dim(D, 0, 2) != D.in_dim)
        return "nz must be 0: the handle's input_dim = " + std::to_string(D.in_dim) + " is not H_rev + 2 (H_rev + H_fwd)" +
               (D.level_input ? " + 1" : "") + " (the ROM is SingleInt2D: no state columns past the position)";
    if (has_level && !D.level_input) return "level is given, but the handle is not level-conditioned (lg_tube_cfg.level_input)";
    if (!has_level && D.level_input) return "level is missing: the handle is level-conditioned (lg_tube_cfg.level_input)";
    return "";
}

// The handle's TubeDev where the problem's kind reads one (plan_reason has then seen it is there), else null.
static const TubeDev *plan_dev(const lg_plan_problem *prob, const lg_tube *tube) {
    return prob->tube_kind == LG_PLAN_TUBE_NN || prob->tube_kind == LG_PLAN_TUBE_NN_STEP ? lg_internal_tube_dev(tube) : nullptr;
}

// the one new refusal of an entry that takes an lg_plan_call
static bool no_call(const lg_plan_call *call, const char *who) {
    if (!call) lg_set_error(std::string(who) + ": null argument");
    return !call;
}

// what every planner launch takes, from the call and the plans v (null where the kernel draws its own); the caller adds the outputs
// its kernel has
static PlanArgs plan_args(const lg_plan_call *call, const float *v) {
    PlanArgs A;
    memset(&A, 0, sizeof(A));
    A.z0 = call->z0; A.v = v; A.e = call->e; A.v_prev = call->v_prev; A.w0 = call->w0; A.offset = call->offset;
    A.level = call->has_level ? call->level : 0.f;
    A.scenes = call->scenes;
    return A;
}

extern "C" {

int lg_plan_check(const lg_plan_problem *prob, const lg_tube *tube, int32_t has_level) {
    const std::string e = plan_reason(prob, lg_internal_tube_dev(tube), has_level);
    if (!e.empty()) { lg_set_error("lg_plan: " + e); return -1; }
    return 0;
}

// Per-plan scenes.
int lg_plan_scenes_check(const lg_plan_scenes *sc, int64_t count) {
    std::string e;
    if (sc->S < 1) e = "S = " + std::to_string(sc->S) + " must be at least 1";
    else if (sc->S != count)
        e = "S = " + std::to_string(sc->S) + " differs from the call's count of plans or instances = " + std::to_string(count);
    else if (sc->obs && !sc->n_obs) e = "obs is given without n_obs";
    else if (!sc->obs && sc->n_obs) e = "n_obs is given without obs";
    else if (!sc->goal && !sc->obs) e = "goal, obs and n_obs are all NULL: the scenes say nothing (pass NULL scenes)";
    else if (sc->vel && !sc->obs) e = "vel is given without obs: a velocity belongs to an obstacle slot of the scenes' own";
    if (!e.empty()) { lg_set_error("lg_plan_scenes: " + e); return -1; }
    return 0;
}

int lg_plan_score(lg_tube *tube, const lg_plan_problem *prob, const lg_plan_call *call, const float *v, float *cost, float *min_clear,
                  int32_t *worst_node, int32_t *n_viol, float *fw, float *z, float *w) {
    if (no_call(call, "lg_plan_score")) return -1;
    const int64_t B = call->count;
    if (lg_plan_check(prob, tube, call->has_level)) return -1;
    if (B < 1 || B > INT32_MAX) { lg_set_error("lg_plan_score: B must be 1..2^31-1"); return -1; }
    if (call->scenes && lg_plan_scenes_check(call->scenes, B)) return -1;
    if (!call->z0 || !v || !cost || !min_clear || !worst_node || !n_viol) {
        lg_set_error("lg_plan_score: missing array (z0, v, cost, min_clear, worst_node and n_viol are required)"); return -1;
    }
    PlanArgs A = plan_args(call, v);
    A.cost = cost; A.min_clear = min_clear; A.worst_node = worst_node; A.n_viol = n_viol; A.fw = fw; A.z = z; A.w = w;
    const TubeDev *D = plan_dev(prob, tube);
    const hipStream_t st = (hipStream_t)call->stream;
    const int64_t rc = prob->tube_kind == LG_PLAN_TUBE_NN_STEP ? tubek_plan_score_step(D, prob, &A, B, st) : tubek_plan_score(D, prob, &A, B, st);
    if (rc < 0) { lg_set_error("lg_plan_score: hipFuncSetAttribute failed"); return -2; }
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_score: launch failed"), -3);
}

// ---------------------------------------------------------------- sampling planner on a tube
static std::string mppi_reason(const lg_mppi_cfg *c, int64_t P) {
    if (c->K < 32 || c->K > LG_MPPI_MAX_K || c->K % 32) return "K = " + std::to_string(c->K) + " must be a multiple of 32 in 32.." + std::to_string(LG_MPPI_MAX_K);
    if (c->iters < 1) return "iters = " + std::to_string(c->iters) + " must be at least 1";
    if (!(c->sigma > 0.f)) return "sigma must be positive";
    if (!(c->sigma_decay > 0.f && c->sigma_decay <= 1.f)) return "sigma_decay must lie in (0, 1]";
    if (!(c->lambda > 0.f)) return "lambda must be positive";
    if (!(c->rho_g >= 0.f)) return "rho_g must not be negative";
    if (!(c->rho_w >= 0.f)) return "rho_w must not be negative";
    if (!(c->rho_z >= 0.f)) return "rho_z must not be negative";
    if (P < 1) return "P = " + std::to_string(P) + " must be at least 1";
    if (P * c->K > INT32_MAX) return "P * K = " + std::to_string(P * c->K) + " must not exceed 2^31 - 1";
    return "";
}

int lg_mppi_check(const lg_mppi_cfg *cfg, const lg_plan_problem *prob, const lg_tube *tube, int32_t has_level, int64_t P) {
    if (lg_plan_check(prob, tube, has_level)) return -1;
    const std::string e = mppi_reason(cfg, P);
    if (!e.empty()) { lg_set_error("lg_mppi: " + e); return -1; }
    return 0;
}

int lg_plan_mppi_candidates(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int32_t it, const float *vbar, int64_t P, float *out,
                            void *stream) {
    lg_plan_problem q = *prob;          // the tube is not read: the analytic envelope of the problem is what counts here
    q.tube_kind = LG_PLAN_TUBE_L1;
    if (lg_mppi_check(cfg, &q, nullptr, 0, P)) return -1;
    if (it < 0) { lg_set_error("lg_plan_mppi_candidates: it must not be negative"); return -1; }
    if (P * cfg->K * (int64_t)prob->N > INT32_MAX) { lg_set_error("lg_plan_mppi_candidates: P * K * N must not exceed 2^31 - 1"); return -1; }
    if (!vbar || !out) { lg_set_error("lg_plan_mppi_candidates: missing array"); return -1; }
    tubek_plan_mppi_candidates(prob, cfg, it, vbar, P, out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_mppi_candidates: launch failed"), -3);
}

int lg_plan_mppi_step(lg_tube *tube, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, const lg_plan_call *call, int32_t it, int32_t what,
                      int32_t reset_best, float *vbar, float *J, float *cost, float *min_clear, float *pen, float *best_J, float *best_v,
                      float *hist_row, int32_t *n_bad) {
    if (no_call(call, "lg_plan_mppi_step")) return -1;
    const int64_t P = call->count;
    if (lg_mppi_check(cfg, prob, tube, call->has_level, P)) return -1;
    if (call->scenes && lg_plan_scenes_check(call->scenes, P)) return -1;
    if (it < 0) { lg_set_error("lg_plan_mppi_step: it must not be negative"); return -1; }
    if (!(what & 3)) { lg_set_error("lg_plan_mppi_step: what must name the score (1), the update (2) or both (3)"); return -1; }
    if (!vbar || !J || ((what & 1) && !call->z0) || ((what & 2) && (!best_J || !best_v || !n_bad))) {
        lg_set_error("lg_plan_mppi_step: missing array (vbar and J; z0 for the score; best_J, best_v and n_bad for the update)"); return -1;
    }
    const hipStream_t st = (hipStream_t)call->stream;
    if (what & 1) {
        PlanArgs A = plan_args(call, nullptr);
        A.cost = cost; A.min_clear = min_clear;
        const TubeDev *D = plan_dev(prob, tube);
        const int64_t rc = prob->tube_kind == LG_PLAN_TUBE_NN_STEP ? tubek_plan_sample_score_step(D, prob, cfg, it, &A, P, vbar, J, pen, st)
                                                                   : tubek_plan_sample_score(D, prob, cfg, it, &A, P, vbar, J, pen, st);
        if (rc < 0) { lg_set_error("lg_plan_mppi_step: hipFuncSetAttribute failed"); return -2; }
    }
    if (what & 2) tubek_plan_mppi_update(prob, cfg, it, reset_best, P, vbar, J, best_J, best_v, hist_row, n_bad, st);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_mppi_step: launch failed"), -3);
}

int lg_plan_mppi(lg_tube *tube, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, const lg_plan_call *call, float *vbar,
                 float *J_scratch, float *best_J, float *best_v, float *hist, int32_t *n_bad) {
    if (no_call(call, "lg_plan_mppi")) return -1;
    const int64_t P = call->count;
    if (lg_mppi_check(cfg, prob, tube, call->has_level, P)) return -1;
    if (call->scenes && lg_plan_scenes_check(call->scenes, P)) return -1;
    for (int32_t it = 0; it < cfg->iters; ++it) {
        const int rc = lg_plan_mppi_step(tube, prob, cfg, call, it, 3, it == 0, vbar, J_scratch, nullptr, nullptr, nullptr, best_J, best_v,
                                         hist ? hist + (int64_t)it * P * 2 : nullptr, n_bad);
        if (rc) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------- gradient planner on a tube
static std::string grad_reason(const lg_grad_cfg *c, int64_t B) {
    if (c->iters < 1) return "iters = " + std::to_string(c->iters) + " must be at least 1";
    if (!(c->lr > 0.f)) return "lr must be positive";
    if (!(c->beta1 >= 0.f && c->beta1 < 1.f)) return "beta1 must lie in [0, 1)";
    if (!(c->beta2 >= 0.f && c->beta2 < 1.f)) return "beta2 must lie in [0, 1)";
    if (!(c->eps > 0.f)) return "eps must be positive";
    if (!(c->rho_g >= 0.f)) return "rho_g must not be negative";
    if (!(c->rho_w >= 0.f)) return "rho_w must not be negative";
    if (!(c->rho_z >= 0.f)) return "rho_z must not be negative";
    if (B < 1) return "B = " + std::to_string(B) + " must be at least 1";
    if (B > INT32_MAX) return "B = " + std::to_string(B) + " must not exceed 2^31 - 1";
    return "";
}

int lg_plan_grad_check(const lg_grad_cfg *cfg, const lg_plan_problem *prob, const lg_tube *tube, int32_t has_level, int64_t B) {
    if (prob->tube_kind == LG_PLAN_TUBE_NN_STEP) {
        lg_set_error("lg_plan_grad: tube_kind nn_step has no gradient planner: reverse mode through N chained MLP passes is not built "
                     "(plan with lg_plan_mppi)");
        return -1;
    }
    if (lg_plan_check(prob, tube, has_level)) return -1;
    const std::string e = grad_reason(cfg, B);
    if (!e.empty()) { lg_set_error("lg_plan_grad: " + e); return -1; }
    return 0;
}

static void grad_args(PlanGradArgs *A, const lg_grad_cfg *cfg, const PlanArgs &plan, float *J, float *grad, float *cost, float *min_clear,
                      float *pen) {
    memset(A, 0, sizeof(*A));
    A->plan = plan;
    A->plan.cost = cost; A->plan.min_clear = min_clear;
    A->J = J; A->grad = grad; A->pen = pen;
    A->lr = cfg->lr; A->beta1 = cfg->beta1; A->beta2 = cfg->beta2; A->eps = cfg->eps; A->bc1 = 1.f; A->bc2 = 1.f;
    A->rho_g = cfg->rho_g; A->rho_w = cfg->rho_w; A->rho_z = cfg->rho_z;
}

int lg_plan_grad(lg_tube *tube, const lg_plan_problem *prob, const lg_grad_cfg *cfg, const lg_plan_call *call, const float *v, float *J,
                 float *grad, float *cost, float *min_clear, float *pen) {
    if (no_call(call, "lg_plan_grad")) return -1;
    const int64_t B = call->count;
    if (lg_plan_grad_check(cfg, prob, tube, call->has_level, B)) return -1;
    if (call->scenes && lg_plan_scenes_check(call->scenes, B)) return -1;
    if (!call->z0 || !v || !J || !grad) { lg_set_error("lg_plan_grad: missing array (z0, v, J and grad are required)"); return -1; }
    PlanGradArgs A;
    grad_args(&A, cfg, plan_args(call, v), J, grad, cost, min_clear, pen);
    if (tubek_plan_grad(plan_dev(prob, tube), prob, &A, B, (hipStream_t)call->stream) < 0) {
        lg_set_error("lg_plan_grad: hipFuncSetAttribute failed"); return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_grad: launch failed"), -3);
}

int lg_plan_descend_step(lg_tube *tube, const lg_plan_problem *prob, const lg_grad_cfg *cfg, const lg_plan_call *call, int32_t it,
                         int32_t what, int32_t reset, float *v, float *J, float *grad, float *cost, float *min_clear, float *pen, float *m,
                         float *s, float *best_J, float *best_v, float *hist_row, int32_t *n_bad) {
    if (no_call(call, "lg_plan_descend_step")) return -1;
    const int64_t B = call->count;
    if (lg_plan_grad_check(cfg, prob, tube, call->has_level, B)) return -1;
    if (call->scenes && lg_plan_scenes_check(call->scenes, B)) return -1;
    if (it < 0) { lg_set_error("lg_plan_descend_step: it must not be negative"); return -1; }
    if (what != 1 && what != 3) {
        lg_set_error("lg_plan_descend_step: what must be the evaluation (1) or the evaluation and the step (3): the step is fused into "
                     "the launch that makes the gradient");
        return -1;
    }
    if (!call->z0 || !v || !J || !best_J || !best_v || !n_bad || ((what & 2) && (!m || !s))) {
        lg_set_error("lg_plan_descend_step: missing array (z0, v, J, best_J, best_v and n_bad; m and s for the step)"); return -1;
    }
    PlanGradArgs A;
    grad_args(&A, cfg, plan_args(call, v), J, grad, cost, min_clear, pen);
    A.v = v;
    A.m = m; A.s = s; A.best_J = best_J; A.best_v = best_v; A.hist = hist_row; A.n_bad = n_bad;
    A.step = (what & 2) != 0; A.reset = reset != 0;
    A.bc1 = (float)(1.0 - std::pow((double)cfg->beta1, (double)it + 1.0));     // step index t = it + 1
    A.bc2 = (float)(1.0 - std::pow((double)cfg->beta2, (double)it + 1.0));
    if (tubek_plan_grad(plan_dev(prob, tube), prob, &A, B, (hipStream_t)call->stream) < 0) {
        lg_set_error("lg_plan_descend_step: hipFuncSetAttribute failed"); return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_descend_step: launch failed"), -3);
}

int lg_plan_descend(lg_tube *tube, const lg_plan_problem *prob, const lg_grad_cfg *cfg, const lg_plan_call *call, float *v,
                    float *J_scratch, float *m, float *s, float *best_J, float *best_v, float *hist, int32_t *n_bad) {
    if (no_call(call, "lg_plan_descend")) return -1;
    const int64_t B = call->count;
    if (lg_plan_grad_check(cfg, prob, tube, call->has_level, B)) return -1;
    if (call->scenes && lg_plan_scenes_check(call->scenes, B)) return -1;
    for (int32_t it = 0; it <= cfg->iters; ++it) {  // iters stepping launches, then the evaluation of the last iterate
        const int rc = lg_plan_descend_step(tube, prob, cfg, call, it, it < cfg->iters ? 3 : 1, it == 0, v, J_scratch, nullptr, nullptr,
                                            nullptr, nullptr, m, s, best_J, best_v, hist ? hist + (int64_t)it * B * 2 : nullptr, n_bad);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
