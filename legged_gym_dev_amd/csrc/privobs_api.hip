// C-ABI (include/legged_hip.h, lg_priv_obs_*) of the privileged observations: the term table resolved to offsets and widths, the
// handle's own (num_envs, W) buffer, and the one launch of privobs_kernels.hip.  The handle keeps no pointer into the env: compute
// borrows the env's buffers and stream for its own call, and leaves a deferred step epilogue (lg_finalize.h) where it is -- the
// epilogue touches no state the kernel reads.  Nothing here waits for the device except create (the zero fill) and destroy.
#include <cmath>
#include <cstring>
#include <string>

#include "privobs_device.h"
#include "lg_internal.h"

struct lg_priv_obs {
    PrivObsDev dev;                     // the env's pointers in it are filled per call
    float *out = nullptr;
    int n = 0, B = 0, measure_heights = 0, traj_N = 0;     // the env's dimensions at creation: every later env must have them
};

static const char *const KIND_NAME[LG_PRIV_NUM_KINDS] = {"obs", "friction", "base_mass", "material", "feet_contact_forces", "feet_contact",
                                                         "feet_air_time", "body_contact", "torques", "heights", "episode_progress"};

static int kind_width(int kind, int O, int A, int F, int NP, int H) {
    switch (kind) {
    case LG_PRIV_OBS: return O;
    case LG_PRIV_FRICTION: case LG_PRIV_BASE_MASS: case LG_PRIV_EPISODE_PROGRESS: return 1;
    case LG_PRIV_MATERIAL: return 4;
    case LG_PRIV_FEET_CONTACT_FORCES: return 3 * F;
    case LG_PRIV_FEET_CONTACT: case LG_PRIV_FEET_AIR_TIME: return F;
    case LG_PRIV_BODY_CONTACT: return NP;
    case LG_PRIV_TORQUES: return A;
    case LG_PRIV_HEIGHTS: return H;
    }
    return -1;
}

// the kernel indexes contact_forces rows with the env's feet_idx / pen_idx
static bool body_rows_ok(const lg_cfg &c, const char *who) {
    bool ok = c.num_feet >= 0 && c.num_feet <= LG_MAX_FEET && c.num_pen >= 0 && c.num_pen <= LG_MAX_PEN;
    for (int f = 0; ok && f < c.num_feet; ++f) ok = c.feet_idx[f] >= 0 && c.feet_idx[f] < c.num_bodies;
    for (int b = 0; ok && b < c.num_pen; ++b) ok = c.pen_idx[b] >= 0 && c.pen_idx[b] < c.num_bodies;
    if (!ok) lg_set_error(std::string(who) + ": the env's feet_idx / pen_idx do not lie within its num_bodies");
    return ok;
}

// the env of this call: its dimensions must be those of the env the handle was created for
static const DevParams *env_of(lg_priv_obs *p, lg_ctx *env, const char *who) {
    if (!p || !env) { lg_set_error(std::string(who) + ": null argument"); return nullptr; }
    const DevParams *E = lg_internal_host_params(env);
    const lg_cfg &c = E->cfg;
    const PrivObsDev &D = p->dev;
    if (c.num_envs != p->n || c.num_obs != D.O || c.num_actions != D.A || c.num_bodies != p->B || c.num_feet != D.F || c.num_pen != D.NP ||
        (c.measure_heights ? c.num_height_points : 0) != D.H || (c.measure_heights != 0) != (p->measure_heights != 0) || (c.traj.enabled ? c.traj.N : 0) != p->traj_N) {
        lg_set_error(std::string(who) + ": the env is not the one the handle was created for (num_envs, num_obs, num_actions, the body "
                     "counts, the height scan or the trajectory window differ)");
        return nullptr;
    }
    return E;
}

extern "C" {

int lg_priv_obs_check(const lg_priv_cfg *c, int32_t num_obs, int32_t num_actions, int32_t num_feet, int32_t num_pen,
                      int32_t num_height_points, int32_t measure_heights, int32_t *width) {
    std::string e;
    auto S = [](long long v) { return std::to_string(v); };
    long long W = 0;
    if (!c) e = "cfg is null";
    else if (c->num_terms < 1 || c->num_terms > LG_PRIV_MAX_TERMS)
        e = "num_terms = " + S(c->num_terms) + " must lie in 1.." + S(LG_PRIV_MAX_TERMS);
    else if (num_obs < 1 || num_actions < 1 || num_actions > LG_MAX_DOF || num_feet < 0 || num_feet > LG_MAX_FEET || num_pen < 0 ||
             num_pen > LG_MAX_PEN || num_height_points < 0)
        e = "the env's dimensions (num_obs, num_actions, num_feet, num_pen, num_height_points) are out of range";
    for (int t = 0; e.empty() && t < c->num_terms; ++t) {
        const int k = c->terms[t].kind;
        const std::string at = "terms[" + S(t) + "]";
        if (k < 0 || k >= LG_PRIV_NUM_KINDS) { e = at + ".kind = " + S(k) + " is not a term (LG_PRIV_*: 0.." + S(LG_PRIV_NUM_KINDS - 1) + ")"; break; }
        for (int u = 0; u < t; ++u)
            if (c->terms[u].kind == k) e = at + ".kind: the term '" + KIND_NAME[k] + "' appears twice (also terms[" + S(u) + "])";
        if (!e.empty()) break;
        if (!std::isfinite(c->terms[t].scale)) { e = at + ".scale is not finite"; break; }
        if (k == LG_PRIV_HEIGHTS && !measure_heights) { e = at + ".kind: 'heights' needs an env with measure_heights"; break; }
        const int w = kind_width(k, num_obs, num_actions, num_feet, num_pen, measure_heights ? num_height_points : 0);
        if (w < 1) { e = at + ".kind: the term '" + KIND_NAME[k] + "' has no entries on this env"; break; }
        W += w;
    }
    if (e.empty() && W > LG_PRIV_MAX_WIDTH) e = "width = " + S(W) + " exceeds LG_PRIV_MAX_WIDTH = " + S(LG_PRIV_MAX_WIDTH);
    if (e.empty()) { if (width) *width = (int32_t)W; return 0; }
    lg_set_error("lg_priv_obs: " + e);
    return -1;
}

int lg_priv_obs_destroy(lg_priv_obs *p) {
    if (!p) return 0;
    (void)hipDeviceSynchronize();
    if (p->out) (void)hipFree(p->out);
    delete p;
    return 0;
}

int lg_priv_obs_create(lg_ctx *env, const lg_priv_cfg *cfg, lg_priv_obs **out) {
    if (!env || !out) { lg_set_error("lg_priv_obs_create: null argument"); return -1; }
    *out = nullptr;
    const DevParams *E = lg_internal_host_params(env);
    const lg_cfg &c = E->cfg;
    int32_t W = 0;
    if (lg_priv_obs_check(cfg, c.num_obs, c.num_actions, c.num_feet, c.num_pen, c.num_height_points, c.measure_heights, &W)) return -1;
    const int H = c.measure_heights ? c.num_height_points : 0;
    if (!body_rows_ok(c, "lg_priv_obs_create")) return -1;
    if (c.num_obs != 9 + (c.traj.enabled ? 2 * c.traj.N : 3) + 3 * c.num_actions + H) {
        lg_set_error("lg_priv_obs_create: num_obs is not 9 + commands | trajectory + 3 num_actions + height points"); return -1;
    }
    lg_priv_obs *p = new lg_priv_obs();
    p->n = c.num_envs; p->B = c.num_bodies; p->measure_heights = c.measure_heights; p->traj_N = c.traj.enabled ? c.traj.N : 0;
    PrivObsDev &D = p->dev;
    memset(&D, 0, sizeof(D));
    D.n = p->n; D.W = W; D.O = c.num_obs; D.A = c.num_actions; D.B = c.num_bodies; D.F = c.num_feet; D.NP = c.num_pen;
    D.H = H; D.traj_N = p->traj_N; D.num_terms = cfg->num_terms;
    int off = 0;
    for (int t = 0; t < cfg->num_terms; ++t) {
        const int w = kind_width(cfg->terms[t].kind, D.O, D.A, D.F, D.NP, H);
        D.terms[t] = PrivTermDev{cfg->terms[t].kind, off, w, cfg->terms[t].scale};
        off += w;
    }
    const size_t bytes = (size_t)p->n * W * sizeof(float);
    if (hipMalloc((void **)&p->out, bytes) != hipSuccess || hipMemset(p->out, 0, bytes) != hipSuccess) {
        lg_set_error("hipMalloc failed in lg_priv_obs_create"); lg_priv_obs_destroy(p); return -100;
    }
    D.out = p->out;
    *out = p;
    return 0;
}

int lg_priv_obs_buffer(lg_priv_obs *p, float **out, int32_t *width) {
    if (!p || !out) { lg_set_error("lg_priv_obs_buffer: null argument"); return -1; }
    *out = p->out;
    if (width) *width = p->dev.W;
    return 0;
}

int lg_priv_obs_compute(lg_priv_obs *p, lg_ctx *env) {
    const DevParams *E = env_of(p, env, "lg_priv_obs_compute");
    if (!E) return -1;
    const lg_cfg &c = E->cfg;
    const lg_buffers &b = E->buf;
    if (!body_rows_ok(c, "lg_priv_obs_compute")) return -1;
    PrivObsDev D = p->dev;
    D.root = b.root_states; D.dof = b.dof_state; D.cf = b.contact_forces; D.torques = b.torques; D.actions = b.actions;
    D.commands = b.commands; D.trajectory = b.trajectory; D.base_lin_vel = b.base_lin_vel; D.base_ang_vel = b.base_ang_vel;
    D.projected_gravity = b.projected_gravity; D.measured_heights = b.measured_heights; D.friction = b.friction;
    D.base_mass_delta = b.base_mass_delta; D.material = b.material; D.feet_air_time = b.feet_air_time; D.episode_length = b.episode_length;
    // the env's constants as they stand now (legged_robot.py:100-103 reads clip_observations at every step)
    D.clip = c.clip_obs;
    D.inv_max_len = (float)(1.0 / (double)c.max_episode_length);
    D.s_lin_vel = c.obs_scale_lin_vel; D.s_ang_vel = c.obs_scale_ang_vel; D.s_dof_pos = c.obs_scale_dof_pos;
    D.s_dof_vel = c.obs_scale_dof_vel; D.s_height = c.obs_scale_height;
    D.s_traj[0] = c.traj.obs_scale[0]; D.s_traj[1] = c.traj.obs_scale[1];
    for (int f = 0; f < D.F; ++f) D.feet_idx[f] = c.feet_idx[f];
    for (int q = 0; q < D.NP; ++q) D.pen_idx[q] = c.pen_idx[q];
    for (int a = 0; a < D.A; ++a) D.default_dof_pos[a] = c.default_dof_pos[a];
    privobsk_launch(&D, lg_internal_stream(env));
    if (hipGetLastError() != hipSuccess) { lg_set_error("lg_priv_obs_compute: launch failed"); return -3; }
    return 0;
}

}  // extern "C"
