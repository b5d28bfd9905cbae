// C-ABI (include/legged_hip.h, lg_romsim_*) of the ROM-on-ROM simulator: buffers in HBM, the DevParams the generator laws of
// lg_traj.h read, the Philox epoch, and the launches of romsim_kernels.hip.  Nothing here waits for the device except
// lg_romsim_inject_status and lg_romsim_destroy.
// lg_plan_track: prescribed plans tracked under the handle's law and bounds (k_plan_track).
#include <cmath>
#include <cstring>
#include <string>

#include "romsim_device.h"
#include "lg_internal.h"

struct lg_romsim {
    lg_romsim_cfg cfg;
    RomSimDev dev;
    DevParams *hp = nullptr;            // host copy (heap: DevParams is tens of KiB), device copy in dev.P
    DevParams *dp = nullptr;
    uint8_t *done = nullptr;
    hipStream_t stream = nullptr;
    int64_t epoch = 0;                  // resets made so far
    int constructed = 0;
    int max_sub = 0;
};

static bool ralloc(void **q, size_t bytes) {
    *q = nullptr;
    if (bytes == 0) bytes = 4;
    return hipMalloc(q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess;
}

static int push_params(lg_romsim *p) {
    // ordered after the launches already on the stream, before the next one
    if (hipMemcpyAsync(p->dp, p->hp, sizeof(DevParams), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess) {
        lg_set_error("lg_romsim: copying the parameters to the device failed");
        return -100;
    }
    return 0;
}

extern "C" {

int lg_romsim_check_cfg(const lg_romsim_cfg *c) {
    std::string e;
    if (c->model_cls != 0) e = "model.cls must be DoubleInt2D";
    else if (c->rom_cls != 0) e = "rom.cls must be SingleInt2D";
    else if (c->controller_cls != 0) e = "controller must be DoubleSingleTracking";
    else if (c->generator_cls != LG_TG_KIND_RANDOM) e = "trajectory_generator.cls must be TrajectoryGenerator (the Zero / Square / Circle generators are not supported on this simulator)";
    else if (c->t_samp_cls != 0) e = "trajectory_generator.t_samp_cls must be UniformSampleHoldDT";
    else if (c->weight_sampler != LG_TG_WSAMP_UNIFORM && c->weight_sampler != LG_TG_WSAMP_NO_RAMP)
        e = "trajectory_generator.weight_samp_cls must be UniformWeightSampler or UniformWeightSamplerNoRamp";
    else if (c->dN != 1) e = "trajectory_generator.dN must be 1";
    else if (c->N < 2 || c->N > LG_TRAJ_MAX_PTS - 1) e = "trajectory_generator.N must be 2.." + std::to_string(LG_TRAJ_MAX_PTS - 1) + " (N = 1 has no v_trajectory[:, 1])";
    else if (!(c->model_dt > 0.f) || !(c->model_dt <= c->rom_dt)) e = "model.dt must satisfy 0 < model.dt <= rom.dt";
    else if (c->num_envs < 1) e = "num_envs must be positive";
    else if (!(c->t_low > 0.f) || !(c->t_high >= c->t_low)) e = "trajectory_generator.t_low / t_high must satisfy 0 < t_low <= t_high";
    if (!e.empty()) { lg_set_error("lg_romsim: " + e); return -1; }
    return 0;
}

int lg_romsim_create(const lg_romsim_cfg *cfg, lg_romsim **out) {
    *out = nullptr;
    if (lg_romsim_check_cfg(cfg)) return -1;
    lg_romsim *p = new lg_romsim();
    p->cfg = *cfg;
    p->hp = new DevParams();
    memset(p->hp, 0, sizeof(DevParams));
    DevParams &H = *p->hp;
    const int n = cfg->num_envs, npts = cfg->N * cfg->dN + 1;
    // the fields the lg_traj.h laws read (and only those)
    lg_traj_cfg &t = H.cfg.traj;
    t.enabled = 1; t.N = cfg->N; t.dN = cfg->dN; t.rom_dt = cfg->rom_dt;
    t.t_low = cfg->t_low; t.t_high = cfg->t_high; t.freq_low = cfg->freq_low; t.freq_high = cfg->freq_high;
    t.prob_stationary = cfg->prob_stationary;
    for (int d = 0; d < 2; ++d) { t.v_min[d] = cfg->rom_v_min[d]; t.v_max[d] = cfg->rom_v_max[d]; }
    H.cfg.num_envs = n; H.cfg.dt = cfg->model_dt; H.cfg.seed = cfg->seed; H.cfg.env_offset = cfg->env_offset;
    for (int d = 0; d < 2; ++d) { H.cb.v_min[d] = t.v_min[d]; H.cb.v_max[d] = t.v_max[d]; }
    H.cb.t_low = t.t_low; H.cb.t_high = t.t_high;
    H.tg_kind = LG_TG_KIND_RANDOM; H.tg_wsamp = cfg->weight_sampler;
    H.K = LG_RS_NRESET;
    RomSimDev &D = p->dev;
    memset(&D, 0, sizeof(D));
    bool ok = ralloc((void **)&p->dp, sizeof(DevParams)) && ralloc((void **)&D.root, (size_t)n * 4 * 4) &&
              ralloc((void **)&H.buf.tg_state, (size_t)n * LG_TG_STRIDE * 4) && ralloc((void **)&H.buf.tg_traj, (size_t)n * npts * 2 * 4) &&
              ralloc((void **)&D.v_traj, (size_t)n * (npts - 1) * 2 * 4) && ralloc((void **)&H.buf.trajectory, (size_t)n * cfg->N * 2 * 4) &&
              ralloc((void **)&D.obs, (size_t)n * LG_RS_NOBS * 4) && ralloc((void **)&D.act, (size_t)n * 2 * 4) &&
              ralloc((void **)&p->done, (size_t)n) && ralloc((void **)&D.n_resample, (size_t)n * 4) && ralloc((void **)&D.overrun, 4);
    if (!ok) { lg_set_error("hipMalloc failed in lg_romsim_create"); lg_romsim_destroy(p); return -100; }
    D.P = p->dp;
    D.n = n; D.inject = 0; D.R = 0; D.rand_dist = cfg->randomize_rom_distance;
    D.dt = cfg->model_dt; D.Kp = cfg->Kp; D.Kd = cfg->Kd; D.llh = cfg->zero_rom_dist_llh;
    for (int d = 0; d < 2; ++d) {
        D.vel_min[d] = cfg->model_z_min[2 + d]; D.vel_max[d] = cfg->model_z_max[2 + d];
        D.acc_min[d] = cfg->model_v_min[d]; D.acc_max[d] = cfg->model_v_max[d];
        D.max_dist[d] = cfg->max_rom_dist[d];
    }
    for (int d = 0; d < 4; ++d) { D.noise_lo[d] = cfg->noise_lo[d]; D.noise_hi[d] = cfg->noise_hi[d]; }
    p->max_sub = (int)std::ceil((double)cfg->rom_dt / (double)cfg->model_dt) + 2;
    if (push_params(p)) { lg_romsim_destroy(p); return -100; }
    *out = p;
    return 0;
}

int lg_romsim_destroy(lg_romsim *p) {
    if (!p) return 0;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    else (void)hipDeviceSynchronize();
    RomSimDev &D = p->dev;
    if (p->hp) {
        lg_buffers &b = p->hp->buf;
        for (void *q : {(void *)b.tg_state, (void *)b.tg_traj, (void *)b.trajectory, (void *)b.inject_uniforms})
            if (q) (void)hipFree(q);
        delete p->hp;
    }
    for (void *q : {(void *)p->dp, (void *)D.root, (void *)D.v_traj, (void *)D.obs, (void *)D.act, (void *)p->done,
                    (void *)D.n_resample, (void *)D.overrun})
        if (q) (void)hipFree(q);
    delete p;
    return 0;
}

int lg_romsim_set_stream(lg_romsim *p, void *stream) { p->stream = (hipStream_t)stream; return 0; }

int lg_romsim_get_buffers(lg_romsim *p, lg_romsim_buffers *out) {
    const RomSimDev &D = p->dev;
    const lg_buffers &b = p->hp->buf;
    out->root_states = D.root; out->tg_state = b.tg_state; out->tg_traj = b.tg_traj; out->v_traj = D.v_traj;
    out->trajectory = b.trajectory; out->obs = D.obs; out->actions = D.act; out->done = p->done;
    out->inject = b.inject_uniforms; out->n_resample = D.n_resample; out->inject_overrun = D.overrun;
    out->inject_K = b.inject_uniforms ? p->hp->K : 0;
    return 0;
}

int lg_romsim_set_epoch(lg_romsim *p, int64_t epoch) {
    if (epoch < 0 || epoch >= ((int64_t)1 << 31)) { lg_set_error("lg_romsim_set_epoch: epoch must be 0..2^31-1"); return -1; }
    p->epoch = epoch;
    return 0;
}
int64_t lg_romsim_get_epoch(lg_romsim *p) { return p->epoch; }

int lg_romsim_inject(lg_romsim *p, int enable, int32_t R, int constructed) {
    if (!enable) { p->dev.inject = 0; return 0; }
    if (R < 1 || R > 4096) { lg_set_error("lg_romsim_inject: R must be 1..4096 (a reset resamples once)"); return -1; }
    DevParams &H = *p->hp;
    if (!H.buf.inject_uniforms || p->dev.R != R) {
        if (p->stream) (void)hipStreamSynchronize(p->stream);
        else (void)hipDeviceSynchronize();
        if (H.buf.inject_uniforms) (void)hipFree(H.buf.inject_uniforms);
        H.K = LG_RS_NRESET + R * LG_TG_NDRAW;
        if (!ralloc((void **)&H.buf.inject_uniforms, (size_t)p->cfg.num_envs * H.K * 4)) {
            H.buf.inject_uniforms = nullptr; p->dev.inject = 0; p->dev.R = 0;
            lg_set_error("hipMalloc failed in lg_romsim_inject"); return -100;
        }
        p->dev.R = R;
        if (push_params(p)) return -100;
    }
    p->dev.inject = 1;
    if (constructed) p->constructed = 1;
    return 0;
}

int lg_romsim_inject_status(lg_romsim *p) {
    int32_t n = 0;
    if (hipMemcpyAsync(&n, p->dev.overrun, 4, hipMemcpyDeviceToHost, p->stream) != hipSuccess ||
        hipStreamSynchronize(p->stream) != hipSuccess) { lg_set_error("lg_romsim_inject_status: reading the count failed"); return -100; }
    if (n == 0) return 0;
    (void)hipMemsetAsync(p->dev.overrun, 0, 4, p->stream);
    lg_set_error("lg_romsim: " + std::to_string(n) + " generator resample(s) found the injected draws used up (R = " +
                 std::to_string(p->dev.R) + " blocks per env): give more blocks to lg_romsim_inject");
    return -1;
}

int lg_romsim_reset(lg_romsim *p, const int32_t *ids, int n) {
    (void)ids;
    if (n != p->cfg.num_envs) {
        lg_set_error("lg_romsim_reset: a partial reset is refused (CustomSim resets all envs at once); n must equal num_envs");
        return -1;
    }
    ++p->epoch;
    romsimk_reset(&p->dev, p->epoch, !p->constructed, p->stream);
    p->constructed = 1;
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_romsim_reset: launch failed"), -3);
}

int lg_romsim_step(lg_romsim *p, const float *actions) {
    romsimk_step(&p->dev, p->epoch, actions, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_romsim_step: launch failed"), -3);
}

int lg_romsim_policy(lg_romsim *p, const float *obs, float *out, int64_t rows) {
    if (rows < 1 || rows > INT32_MAX) { lg_set_error("lg_romsim_policy: rows must be 1..2^31-1"); return -1; }
    if (!obs || !out) { lg_set_error("lg_romsim_policy: missing array"); return -1; }
    romsimk_policy(&p->dev, obs, out, rows, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_romsim_policy: launch failed"), -3);
}

int lg_romsim_collect(lg_romsim *p, int32_t T, float *z, float *v, float *pz_x, uint8_t *done, float *x) {
    if (T < 1) { lg_set_error("lg_romsim_collect: T must be at least 1"); return -1; }
    if (!z || !v || !pz_x || !done) { lg_set_error("lg_romsim_collect: missing array (z, v, pz_x and done are required)"); return -1; }
    ++p->epoch;
    romsimk_collect(&p->dev, p->epoch, !p->constructed, T, p->max_sub, z, v, pz_x, done, x, p->stream);
    p->constructed = 1;
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_romsim_collect: launch failed"), -3);
}

// DESIGN.md section 10.9.  The handle's epoch, generator state and buffers are not touched.
int lg_plan_track(lg_romsim *p, const float *z, const float *v, const float *x0, int64_t B, int32_t N, int32_t S, float rom_dt,
                  float *pz_x, float *w_true, float *x, float *u) {
    if (B < 1 || B > INT32_MAX) { lg_set_error("lg_plan_track: B must be 1..2^31-1"); return -1; }
    if (N < 1 || N > LG_PLAN_MAX_N) { lg_set_error("lg_plan_track: N must be 1.." + std::to_string(LG_PLAN_MAX_N)); return -1; }
    if (S < 1 || S > 8) { lg_set_error("lg_plan_track: S must be 1..8"); return -1; }
    if (!(rom_dt > 0.f) || !(std::fabs((double)S * (double)p->cfg.model_dt - (double)rom_dt) <= 1e-6 * (double)rom_dt)) {
        lg_set_error("lg_plan_track: S * model_dt = " + std::to_string(S) + " * " + std::to_string(p->cfg.model_dt) +
                     " differs from rom_dt = " + std::to_string(rom_dt) + " (the ROM step must be a whole number S of model steps)");
        return -1;
    }
    if (!z || !v || !pz_x || !w_true) { lg_set_error("lg_plan_track: missing array (z, v, pz_x and w_true are required)"); return -1; }
    romsimk_plan_track(&p->dev, z, v, x0, B, N, S, rom_dt, pz_x, w_true, x, u, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_plan_track: launch failed"), -3);
}

}  // extern "C"
