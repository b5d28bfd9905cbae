// C-ABI (include/legged_hip.h, lg_obs_hist_*) of the actor's observation history: the range table resolved to positions, the
// handle's own (num_envs, W) row and its marks, and the one launch of obshist_kernels.hip.  As lg_priv_obs, the handle keeps no
// pointer into the env: compute and mark borrow the env's buffers and stream for their own call and leave a deferred step epilogue
// (lg_finalize.h) where it is -- the epilogue touches neither obs nor reset.  Nothing here waits for the device except create and
// destroy.
#include <cstring>
#include <string>

#include "obshist_device.h"
#include "lg_internal.h"

struct lg_obs_hist {
    ObsHistDev dev;                     // the env's pointers and the epoch in it are filled per call
    float *row = nullptr;
    int64_t *marks = nullptr;
    int64_t computes = 0;               // computes enqueued so far: a mark made now is meant for compute number computes + 1
};

// the env of this call: its dimensions must be those of the env the handle was created for
static const DevParams *env_of(lg_obs_hist *h, lg_ctx *env, const char *who) {
    if (!h || !env) { lg_set_error(std::string(who) + ": null argument"); return nullptr; }
    const DevParams *E = lg_internal_host_params(env);
    if (E->cfg.num_envs != h->dev.n || E->cfg.num_obs != h->dev.O) {
        lg_set_error(std::string(who) + ": the env is not the one the handle was created for (num_envs or num_obs differ)");
        return nullptr;
    }
    return E;
}

extern "C" {

int lg_obs_hist_check(const lg_obs_hist_cfg *c, int32_t num_obs, int32_t *width) {
    std::string e;
    auto S = [](long long v) { return std::to_string(v); };
    long long sel = 0;
    if (!c) e = "cfg is null";
    else if (num_obs < 1) e = "num_obs = " + S(num_obs) + " must be positive";
    else if (c->length < 2 || c->length > LG_OBS_HIST_MAX_LENGTH)
        e = "length = " + S(c->length) + " must lie in 2.." + S(LG_OBS_HIST_MAX_LENGTH);
    else if (c->num_ranges < 0 || c->num_ranges > LG_OBS_HIST_MAX_RANGES)
        e = "num_ranges = " + S(c->num_ranges) + " must lie in 0.." + S(LG_OBS_HIST_MAX_RANGES) + " (0: every column)";
    else if (c->reset_mode != LG_OBS_HIST_REPEAT && c->reset_mode != LG_OBS_HIST_ZERO)
        e = "reset_mode = " + S(c->reset_mode) + " is neither LG_OBS_HIST_REPEAT (0) nor LG_OBS_HIST_ZERO (1)";
    for (int r = 0; e.empty() && r < c->num_ranges; ++r) {
        const long long lo = c->lo[r], hi = c->hi[r];
        const std::string at = "[" + S(r) + "]";
        if (lo < 0) e = "lo" + at + " = " + S(lo) + " is negative";
        else if (lo >= hi) e = "lo" + at + " = " + S(lo) + " is not below hi" + at + " = " + S(hi) + " (ranges are half-open [lo, hi))";
        else if (hi > num_obs) e = "hi" + at + " = " + S(hi) + " exceeds num_obs = " + S(num_obs);
        else if (r > 0 && lo < c->hi[r - 1])
            e = "lo" + at + " = " + S(lo) + " lies below hi[" + S(r - 1) + "] = " + S(c->hi[r - 1]) + ": ranges must ascend and not overlap";
        sel += hi - lo;
    }
    if (e.empty()) {
        if (c->num_ranges == 0) sel = num_obs;
        const long long W = num_obs + (long long)(c->length - 1) * sel;
        if (W > LG_OBS_HIST_MAX_WIDTH)
            e = "width = num_obs + (length - 1) * selected = " + S(num_obs) + " + " + S(c->length - 1) + " * " + S(sel) + " = " + S(W) +
                " exceeds LG_OBS_HIST_MAX_WIDTH = " + S(LG_OBS_HIST_MAX_WIDTH);
        else { if (width) *width = (int32_t)W; return 0; }
    }
    lg_set_error("lg_obs_hist: " + e);
    return -1;
}

int lg_obs_hist_destroy(lg_obs_hist *h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    if (h->row) (void)hipFree(h->row);
    if (h->marks) (void)hipFree(h->marks);
    delete h;
    return 0;
}

int lg_obs_hist_create(lg_ctx *env, const lg_obs_hist_cfg *cfg, lg_obs_hist **out) {
    if (!env || !out) { lg_set_error("lg_obs_hist_create: null argument"); return -1; }
    *out = nullptr;
    const DevParams *E = lg_internal_host_params(env);
    int32_t W = 0;
    if (lg_obs_hist_check(cfg, E->cfg.num_obs, &W)) return -1;
    lg_obs_hist *h = new lg_obs_hist();
    ObsHistDev &D = h->dev;
    memset(&D, 0, sizeof(D));
    D.n = E->cfg.num_envs; D.O = E->cfg.num_obs; D.W = W; D.H = cfg->length; D.num_ranges = cfg->num_ranges; D.reset_mode = cfg->reset_mode;
    int pos = 0;
    for (int r = 0; r < cfg->num_ranges; ++r) {
        D.lo[r] = cfg->lo[r]; D.hi[r] = cfg->hi[r]; D.pos[r] = pos;
        pos += cfg->hi[r] - cfg->lo[r];
    }
    D.S = cfg->num_ranges ? pos : D.O;
    const size_t bytes = (size_t)D.n * W * sizeof(float);
    if (hipMalloc((void **)&h->row, bytes) != hipSuccess || hipMemset(h->row, 0, bytes) != hipSuccess ||
        hipMalloc((void **)&h->marks, (size_t)D.n * sizeof(int64_t)) != hipSuccess) {
        lg_set_error("hipMalloc failed in lg_obs_hist_create"); lg_obs_hist_destroy(h); return -100;
    }
    D.row = h->row; D.marks = h->marks;
    // every env starts marked: the first compute initialises every row
    obshistk_mark(h->marks, nullptr, D.n, D.n, 1, lg_internal_stream(env));
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(lg_internal_stream(env)) != hipSuccess) {
        lg_set_error("lg_obs_hist_create: launch failed"); lg_obs_hist_destroy(h); return -3;
    }
    *out = h;
    return 0;
}

int lg_obs_hist_buffer(lg_obs_hist *h, void **out, int32_t *width) {
    if (!h || !out) { lg_set_error("lg_obs_hist_buffer: null argument"); return -1; }
    *out = h->row;
    if (width) *width = h->dev.W;
    return 0;
}

int lg_obs_hist_mark(lg_obs_hist *h, lg_ctx *env, const int32_t *ids, int32_t n) {
    const DevParams *E = env_of(h, env, "lg_obs_hist_mark");
    if (!E) return -1;
    if (!ids) n = h->dev.n;
    if (n < 0 || n > h->dev.n) { lg_set_error("lg_obs_hist_mark: n = " + std::to_string(n) + " must lie in 0..num_envs"); return -1; }
    if (n == 0) return 0;
    obshistk_mark(h->marks, ids, n, h->dev.n, h->computes + 1, lg_internal_stream(env));
    if (hipGetLastError() != hipSuccess) { lg_set_error("lg_obs_hist_mark: launch failed"); return -3; }
    return 0;
}

int lg_obs_hist_compute(lg_obs_hist *h, lg_ctx *env) {
    const DevParams *E = env_of(h, env, "lg_obs_hist_compute");
    if (!E) return -1;
    ObsHistDev D = h->dev;
    D.obs = E->buf.obs; D.reset = E->buf.reset;
    D.epoch = h->computes + 1;
    obshistk_launch(&D, lg_internal_stream(env));
    if (hipGetLastError() != hipSuccess) { lg_set_error("lg_obs_hist_compute: launch failed"); return -3; }
    h->computes = D.epoch;              // only now do the marks made for this compute lapse: the next one carries the next number
    return 0;
}

}  // extern "C"
