// C-ABI (include/legged_hip.h, lg_cmdtrack_*) of the command tracker: the tracker's own state in HBM (ROM state and command in
// force, generator rows, plans, injected draws), the DevParams the generator laws of lg_traj.h read, and the one launch of
// cmdtrack_kernels.hip.  The tracker keeps no pointer into the env: an entry borrows the env's buffers and stream for its own call.
// Nothing here waits for the device except lg_cmdtrack_inject (when it reallocates), lg_cmdtrack_inject_status and
// lg_cmdtrack_destroy.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cmdtrack_device.h"
#include "lg_internal.h"

struct lg_cmdtrack {
    lg_cmdtrack_cfg cfg;
    CmdTrackDev dev;                    // the env's pointers in it are filled per call and cleared after it
    DevParams *hp = nullptr;            // host copy (heap: DevParams is tens of KiB), device copy in dev.P
    DevParams *dp = nullptr;
    float *plan = nullptr;
    int n = 0, num_obs = 0, A = 0;      // the env's dimensions at creation: every later env must have them
    float dt = 0.f;
    int64_t epoch = 0;                  // of the last begin
    int begun = 0, constructed = 0, T = 0;
};

static bool calloc_dev(void **q, size_t bytes) {
    *q = nullptr;
    if (bytes == 0) bytes = 4;
    return hipMalloc(q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess;
}

static int push_params(lg_cmdtrack *p) {
    if (hipMemcpy(p->dp, p->hp, sizeof(DevParams), hipMemcpyHostToDevice) != hipSuccess) {
        lg_set_error("lg_cmdtrack: copying the parameters to the device failed");
        return -100;
    }
    return 0;
}

// the env of this call: its dimensions must be those of the env the tracker was created for
static const DevParams *env_of(lg_cmdtrack *p, lg_ctx *env, const char *who) {
    if (!p || !env) { lg_set_error(std::string(who) + ": null argument"); return nullptr; }
    const DevParams *E = lg_internal_host_params(env);
    if (E->cfg.num_envs != p->n || E->cfg.num_obs != p->num_obs || E->cfg.num_actions != p->A || E->cfg.dt != p->dt || E->cfg.traj.enabled) {
        lg_set_error(std::string(who) + ": the env is not the one the tracker was created for (num_envs, num_obs, num_actions or dt differ)");
        return nullptr;
    }
    return E;
}

extern "C" {

int lg_cmdtrack_check(const lg_cmdtrack_cfg *c, const lg_cmdtrack_rec *r, int32_t env_traj, int32_t num_obs, int32_t env_x_n) {
    std::string e;
    auto S = [](long long v) { return std::to_string(v); };
    if (!c) e = "cfg is null";
    else if (env_traj) e = "the env is a trajectory env: its observation has no command columns (collect_trajectory_data.py serves it)";
    else if (c->kind != LG_TG_KIND_RANDOM && c->kind != LG_TG_KIND_PLAN)
        e = "kind = " + S(c->kind) + " must be LG_TG_KIND_RANDOM (0) or LG_TG_KIND_PLAN (4)";
    else if (c->cmd_col < 0 || c->cmd_col + 3 > num_obs)
        e = "cmd_col = " + S(c->cmd_col) + ": cmd_col .. cmd_col + 2 must lie within the num_obs = " + S(num_obs) + " observations";
    else if (c->x_n != 0 && c->x_n != env_x_n) e = "x_n = " + S(c->x_n) + " must be 0 or the env's " + S(env_x_n);
    if (e.empty()) {
        for (int j = 0; j < 9 && e.empty(); ++j)
            if (!std::isfinite(c->Kp[j])) e = "Kp[" + S(j) + "] is not finite";
        for (int j = 0; j < 3 && e.empty(); ++j) {
            if (!(c->u_min[j] <= c->u_max[j])) e = "u_min[" + S(j) + "] exceeds u_max[" + S(j) + "] (or one is not a number)";
            else if (!std::isfinite(c->cmd_scale[j])) e = "cmd_scale[" + S(j) + "] is not finite";
        }
    }
    if (e.empty() && c->kind == LG_TG_KIND_RANDOM) {
        if (c->weight_sampler != LG_TG_WSAMP_UNIFORM && c->weight_sampler != LG_TG_WSAMP_NO_RAMP)
            e = "weight_sampler = " + S(c->weight_sampler) + " must be LG_TG_WSAMP_UNIFORM (0) or LG_TG_WSAMP_NO_RAMP (1)";
        else if (c->tg_N < 1 || c->tg_N > LG_TRAJ_MAX_PTS - 1) e = "tg_N = " + S(c->tg_N) + " must lie in 1.." + S(LG_TRAJ_MAX_PTS - 1);
        else if (!(c->t_low > 0.f) || !(c->t_high >= c->t_low)) e = "t_low / t_high must satisfy 0 < t_low <= t_high";
        else
            for (int d = 0; d < 2 && e.empty(); ++d)
                if (!(c->rom_v_min[d] <= c->rom_v_max[d])) e = "rom_v_min[" + S(d) + "] exceeds rom_v_max[" + S(d) + "] (or one is not a number)";
    }
    if (e.empty() && r) {
        if (r->T < 1) e = "T = " + S(r->T) + " must be at least 1";
        else if (!r->z) e = "z is null";
        else if (!r->v) e = "v is null";
        else if (!r->pz_x) e = "pz_x is null";
        else if (!r->done) e = "done is null";
        else if (r->x && c->x_n == 0) e = "x is given but x_n = 0";
    }
    if (e.empty()) return 0;
    lg_set_error("lg_cmdtrack: " + e);
    return -1;
}

int lg_cmdtrack_destroy(lg_cmdtrack *p) {
    if (!p) return 0;
    (void)hipDeviceSynchronize();
    if (p->hp) {
        lg_buffers &b = p->hp->buf;
        for (void *q : {(void *)b.tg_state, (void *)b.inject_uniforms})
            if (q) (void)hipFree(q);
        delete p->hp;
    }
    for (void *q : {(void *)p->dp, (void *)p->dev.state, (void *)p->dev.n_resample, (void *)p->dev.overrun, (void *)p->plan})
        if (q) (void)hipFree(q);
    delete p;
    return 0;
}

int lg_cmdtrack_create(lg_ctx *env, const lg_cmdtrack_cfg *cfg, lg_cmdtrack **out) {
    if (!env || !out) { lg_set_error("lg_cmdtrack_create: null argument"); return -1; }
    *out = nullptr;
    const DevParams *E = lg_internal_host_params(env);
    if (lg_cmdtrack_check(cfg, nullptr, E->cfg.traj.enabled, E->cfg.num_obs, 13 + 2 * E->cfg.num_actions)) return -1;
    lg_cmdtrack *p = new lg_cmdtrack();
    p->cfg = *cfg;
    p->n = E->cfg.num_envs; p->num_obs = E->cfg.num_obs; p->A = E->cfg.num_actions; p->dt = E->cfg.dt;
    p->hp = new DevParams();
    memset(p->hp, 0, sizeof(DevParams));
    DevParams &H = *p->hp;
    const int n = p->n;
    // the fields the lg_traj.h laws read (and only those), as lg_romsim_create fills them
    lg_traj_cfg &t = H.cfg.traj;
    t.enabled = 1; t.N = cfg->kind == LG_TG_KIND_RANDOM ? cfg->tg_N : 1; t.dN = 1; t.rom_dt = E->cfg.dt;
    t.t_low = cfg->t_low; t.t_high = cfg->t_high; t.freq_low = cfg->freq_low; t.freq_high = cfg->freq_high;
    t.prob_stationary = cfg->prob_stationary;
    for (int d = 0; d < 2; ++d) { t.v_min[d] = cfg->rom_v_min[d]; t.v_max[d] = cfg->rom_v_max[d]; }
    H.cfg.num_envs = n; H.cfg.dt = E->cfg.dt; H.cfg.seed = cfg->seed; H.cfg.env_offset = E->cfg.env_offset;
    for (int d = 0; d < 2; ++d) { H.cb.v_min[d] = t.v_min[d]; H.cb.v_max[d] = t.v_max[d]; }
    H.cb.t_low = t.t_low; H.cb.t_high = t.t_high;
    H.tg_kind = LG_TG_KIND_RANDOM; H.tg_wsamp = cfg->weight_sampler;
    H.K = LG_RS_NRESET;
    CmdTrackDev &D = p->dev;
    memset(&D, 0, sizeof(D));
    bool ok = calloc_dev((void **)&p->dp, sizeof(DevParams)) && calloc_dev((void **)&D.state, (size_t)n * LG_CT_STATE * 4) &&
              calloc_dev((void **)&H.buf.tg_state, (size_t)n * LG_TG_STRIDE * 4) && calloc_dev((void **)&D.n_resample, (size_t)n * 4) &&
              calloc_dev((void **)&D.overrun, (size_t)n * 4) && calloc_dev((void **)&p->plan, (size_t)n * LG_PLAN_MAX_N * 2 * 4);
    if (!ok) { lg_set_error("hipMalloc failed in lg_cmdtrack_create"); lg_cmdtrack_destroy(p); return -100; }
    D.P = p->dp; D.plan = p->plan;
    D.n = n; D.num_obs = p->num_obs; D.A = p->A; D.kind = cfg->kind; D.track_yaw = cfg->track_yaw != 0; D.cmd_col = cfg->cmd_col;
    D.x_n = cfg->x_n; D.rom_dt = E->cfg.dt;
    for (int j = 0; j < 9; ++j) D.Kp[j] = cfg->Kp[j];
    for (int j = 0; j < 3; ++j) { D.u_min[j] = cfg->u_min[j]; D.u_max[j] = cfg->u_max[j]; D.cmd_scale[j] = cfg->cmd_scale[j]; }
    if (push_params(p)) { lg_cmdtrack_destroy(p); return -100; }
    *out = p;
    return 0;
}

int lg_cmdtrack_get_buffers(lg_cmdtrack *p, lg_cmdtrack_buffers *out) {
    if (!p || !out) { lg_set_error("lg_cmdtrack_get_buffers: null argument"); return -1; }
    const lg_buffers &b = p->hp->buf;
    out->state = p->dev.state; out->tg_state = b.tg_state; out->plan = p->plan; out->inject = b.inject_uniforms;
    out->n_resample = p->dev.n_resample; out->inject_overrun = p->dev.overrun;
    out->inject_K = b.inject_uniforms ? p->hp->K : 0;
    return 0;
}

int lg_cmdtrack_set_plans(lg_cmdtrack *p, lg_ctx *env, const float *v, int32_t n_nodes) {
    if (!env_of(p, env, "lg_cmdtrack_set_plans")) return -1;
    if (p->cfg.kind != LG_TG_KIND_PLAN) { lg_set_error("lg_cmdtrack_set_plans: the tracker's kind is not LG_TG_KIND_PLAN"); return -1; }
    if (n_nodes < 0 || n_nodes > LG_PLAN_MAX_N) {
        lg_set_error("lg_cmdtrack_set_plans: n_nodes = " + std::to_string(n_nodes) + " must lie in 0.." + std::to_string(LG_PLAN_MAX_N)); return -1;
    }
    if (n_nodes > 0 && !v) { lg_set_error("lg_cmdtrack_set_plans: v is null with n_nodes > 0"); return -1; }
    if (n_nodes > 0 && hipMemcpy2DAsync(p->plan, (size_t)LG_PLAN_MAX_N * 8, v, (size_t)n_nodes * 8, (size_t)n_nodes * 8, (size_t)p->n,
                                        hipMemcpyDeviceToDevice, lg_internal_stream(env)) != hipSuccess) {
        lg_set_error("lg_cmdtrack_set_plans: the copy failed"); return -100;
    }
    p->dev.n_nodes = n_nodes;
    return 0;
}

int lg_cmdtrack_inject(lg_cmdtrack *p, int enable, int32_t R) {
    if (!p) { lg_set_error("lg_cmdtrack_inject: null argument"); return -1; }
    if (!enable) { p->dev.inject = 0; return 0; }
    if (R < 1 || R > 4096) { lg_set_error("lg_cmdtrack_inject: R must be 1..4096 (a begin resamples once)"); return -1; }
    DevParams &H = *p->hp;
    if (!H.buf.inject_uniforms || p->dev.R != R) {
        (void)hipDeviceSynchronize();
        if (H.buf.inject_uniforms) (void)hipFree(H.buf.inject_uniforms);
        H.K = LG_RS_NRESET + R * LG_TG_NDRAW;
        if (!calloc_dev((void **)&H.buf.inject_uniforms, (size_t)p->n * H.K * 4)) {
            H.buf.inject_uniforms = nullptr; p->dev.inject = 0; p->dev.R = 0;
            lg_set_error("hipMalloc failed in lg_cmdtrack_inject"); return -100;
        }
        p->dev.R = R;
        if (push_params(p)) return -100;
    }
    p->dev.inject = 1;
    return 0;
}

int lg_cmdtrack_inject_status(lg_cmdtrack *p) {
    if (!p) { lg_set_error("lg_cmdtrack_inject_status: null argument"); return -1; }
    std::vector<int32_t> h((size_t)p->n);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), p->dev.overrun, (size_t)p->n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        lg_set_error("lg_cmdtrack_inject_status: reading the counts failed"); return -100;
    }
    long long total = 0;
    for (int32_t c : h) total += c;
    if (total == 0) return 0;
    (void)hipMemset(p->dev.overrun, 0, (size_t)p->n * 4);
    lg_set_error("lg_cmdtrack: " + std::to_string(total) + " generator resample(s) found the injected draws used up (R = " +
                 std::to_string(p->dev.R) + " blocks per env): give more blocks to lg_cmdtrack_inject");
    return -1;
}

static int launch(lg_cmdtrack *p, lg_ctx *env, const DevParams *E, const lg_cmdtrack_rec *rec, int t, const char *who) {
    if (lg_finalize(env)) return -1;                               // as every env entry
    CmdTrackDev D = p->dev;
    D.root = E->buf.root_states; D.dof = E->buf.dof_state; D.obs = E->buf.obs; D.reset = E->buf.reset;
    cmdtrackk_launch(&D, rec, t, p->epoch, t < 0 && !p->constructed, lg_internal_stream(env));
    if (hipGetLastError() != hipSuccess) { lg_set_error(std::string(who) + ": launch failed"); return -3; }
    return 0;
}

int lg_cmdtrack_begin(lg_cmdtrack *p, lg_ctx *env, const lg_cmdtrack_rec *rec, int64_t epoch) {
    const DevParams *E = env_of(p, env, "lg_cmdtrack_begin");
    if (!E) return -1;
    if (!rec) { lg_set_error("lg_cmdtrack_begin: rec is null"); return -1; }
    if (lg_cmdtrack_check(&p->cfg, rec, 0, p->num_obs, 13 + 2 * p->A)) return -1;
    if (epoch < 0 || epoch >= ((int64_t)1 << 31)) { lg_set_error("lg_cmdtrack_begin: epoch must be 0..2^31-1"); return -1; }
    p->epoch = epoch;
    const int rc = launch(p, env, E, rec, -1, "lg_cmdtrack_begin");
    if (rc) return rc;
    if (p->cfg.kind == LG_TG_KIND_RANDOM) p->constructed = 1;
    p->begun = 1; p->T = rec->T;
    return 0;
}

int lg_cmdtrack_step(lg_cmdtrack *p, lg_ctx *env, const lg_cmdtrack_rec *rec, int32_t t) {
    const DevParams *E = env_of(p, env, "lg_cmdtrack_step");
    if (!E) return -1;
    if (!rec) { lg_set_error("lg_cmdtrack_step: rec is null"); return -1; }
    if (lg_cmdtrack_check(&p->cfg, rec, 0, p->num_obs, 13 + 2 * p->A)) return -1;
    if (!p->begun || rec->T != p->T) { lg_set_error("lg_cmdtrack_step: no lg_cmdtrack_begin with this T came before"); return -1; }
    if (t < 0 || t >= rec->T) { lg_set_error("lg_cmdtrack_step: t = " + std::to_string(t) + " must lie in 0.." + std::to_string(rec->T - 1)); return -1; }
    return launch(p, env, E, rec, t, "lg_cmdtrack_step");
}

}  // extern "C"
