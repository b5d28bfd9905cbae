// C-ABI (include/legged_hip.h, lg_obs_norm_*) of the empirical observation normalisation: the handle's two state copies, slab and
// output, the row counter and the `until` rule on the host, and the one or two launches of obsnorm_kernels.hip.  The handle keeps no
// pointer into an env or a learner: x, y and the stream are the caller's for the call.  Nothing here waits for the device except
// create, get_state, set_state and destroy.
#include <cmath>
#include <string>
#include <vector>

#include "obsnorm_device.h"
#include "lg_internal.h"

struct lg_obs_norm {
    lg_obs_norm_cfg cfg;
    int64_t max_rows = 0, count = 0;
    float *state = nullptr;             // (2, 3, W): two copies of mean | var | std
    int cur = 0;                        // the copy that holds the state; a training compute writes the other and flips
    double2 *slab = nullptr;            // (ceil(max_rows / LG_OBS_NORM_ROWS), W)
    float *y = nullptr;                 // (max_rows, W)
};

static int refuse(const std::string &s) { lg_set_error("lg_obs_norm: " + s); return -1; }
static std::string S(long long v) { return std::to_string(v); }

extern "C" {

int lg_obs_norm_check(const lg_obs_norm_cfg *c) {
    if (!c) return refuse("cfg is null");
    if (c->width < 1 || c->width > LG_OBS_NORM_MAX_WIDTH)
        return refuse("width = " + S(c->width) + " must lie in 1.." + S(LG_OBS_NORM_MAX_WIDTH) + " (LG_OBS_NORM_MAX_WIDTH)");
    if (!std::isfinite(c->eps) || !(c->eps > 0.0f)) return refuse("eps = " + std::to_string(c->eps) + " must be finite and positive");
    if (c->until < -1) return refuse("until = " + S(c->until) + " must be -1 (never stop) or a row count >= 0");
    return 0;
}

int lg_obs_norm_destroy(lg_obs_norm *h) {
    if (!h) return 0;
    (void)hipDeviceSynchronize();
    if (h->state) (void)hipFree(h->state);
    if (h->slab) (void)hipFree(h->slab);
    if (h->y) (void)hipFree(h->y);
    delete h;
    return 0;
}

// mean | var | std of `width` columns each into copy `cur`; waits for the device
static int write_state(lg_obs_norm *h, const float *mean, const float *var) {
    const int W = h->cfg.width;
    std::vector<float> st(3 * (size_t)W);
    for (int j = 0; j < W; ++j) { st[j] = mean ? mean[j] : 0.0f; st[W + j] = var ? var[j] : 1.0f; st[2 * W + j] = sqrtf(st[W + j]); }
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(h->state + (size_t)h->cur * 3 * W, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        lg_set_error("lg_obs_norm: copying the state to the device failed");
        return -100;
    }
    return 0;
}

int lg_obs_norm_create(const lg_obs_norm_cfg *cfg, int64_t max_rows, lg_obs_norm **out) {
    if (!out) return refuse("create: out is null");
    *out = nullptr;
    if (lg_obs_norm_check(cfg)) return -1;
    if (max_rows < 1 || max_rows > (int64_t)1 << 31) return refuse("create: max_rows = " + S(max_rows) + " must lie in 1..2^31");
    lg_obs_norm *h = new lg_obs_norm();
    h->cfg = *cfg;
    h->max_rows = max_rows;
    const size_t W = (size_t)cfg->width, nrb = (size_t)((max_rows + LG_OBS_NORM_ROWS - 1) / LG_OBS_NORM_ROWS);
    const size_t ybytes = (size_t)max_rows * W * sizeof(float);
    if (hipMalloc((void **)&h->state, 2 * 3 * W * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&h->slab, nrb * W * sizeof(double2)) != hipSuccess || hipMalloc((void **)&h->y, ybytes) != hipSuccess ||
        hipMemset(h->state, 0, 2 * 3 * W * sizeof(float)) != hipSuccess || hipMemset(h->y, 0, ybytes) != hipSuccess) {
        lg_set_error("lg_obs_norm: hipMalloc failed in create");
        lg_obs_norm_destroy(h);
        return -100;
    }
    if (int rc = write_state(h, nullptr, nullptr)) { lg_obs_norm_destroy(h); return rc; }
    *out = h;
    return 0;
}

int lg_obs_norm_buffer(lg_obs_norm *h, void **y, int32_t *width) {
    if (!h || !y) return refuse("buffer: null argument");
    *y = h->y;
    if (width) *width = h->cfg.width;
    return 0;
}

int lg_obs_norm_compute(lg_obs_norm *const *h, const float *const *x, float *const *y, int32_t num, int64_t n, int32_t update,
                        void *stream) {
    if (num != 1 && num != 2) return refuse("compute: num = " + S(num) + " must be 1 or 2");
    if (!h || !x) return refuse("compute: null argument");
    if (n < 1) return refuse("compute: n = " + S(n) + " must be positive");
    const int64_t nrb = (n + LG_OBS_NORM_ROWS - 1) / LG_OBS_NORM_ROWS;
    if (nrb > 0x7fffffff) return refuse("compute: n = " + S(n) + " exceeds 2^31 - 1 row blocks of " + S(LG_OBS_NORM_ROWS));
    if (num == 2 && h[0] && h[0] == h[1]) return refuse("compute: the two handles of a pair are the same one");
    ObsNormDev D = {};
    D.n = n;
    D.nrb = (int)nrb;
    bool any = false;
    for (int i = 0; i < num; ++i) {
        const std::string at = "[" + S(i) + "]";
        lg_obs_norm *g = h[i];
        if (!g || !x[i]) return refuse("compute: h" + at + " or x" + at + " is null");
        float *yi = y ? y[i] : nullptr;
        if (yi == x[i]) return refuse("compute: y" + at + " == x" + at + ": normalising in place is not supported");
        if (!yi && n > g->max_rows)
            return refuse("compute: n = " + S(n) + " exceeds max_rows = " + S(g->max_rows) + " of the handle's own buffer; pass y" + at);
        if (update && n > g->max_rows)
            return refuse("compute: a training compute of n = " + S(n) + " rows exceeds max_rows = " + S(g->max_rows) + " (the slab)");
        const bool up = update && !(g->cfg.until >= 0 && g->count >= g->cfg.until);
        const size_t W = (size_t)g->cfg.width;
        ObsNormProb &P = D.p[i];
        P.x = x[i];
        P.y = yi ? yi : g->y;
        P.st_in = g->state + (size_t)g->cur * 3 * W;
        P.st_out = g->state + (size_t)(g->cur ^ 1) * 3 * W;
        P.slab = g->slab;
        P.rate = up ? (double)n / (double)(g->count + n) : 0.0;
        P.eps = g->cfg.eps;
        P.W = (int)W;
        P.update = up ? 1 : 0;
        any = any || up;
    }
    hipStream_t st = (hipStream_t)stream;
    if (any) obsnormk_stats(&D, num, st);
    obsnormk_apply(&D, num, st);
    if (hipGetLastError() != hipSuccess) { lg_set_error("lg_obs_norm: compute: launch failed"); return -3; }
    for (int i = 0; i < num; ++i)
        if (D.p[i].update) { h[i]->count += n; h[i]->cur ^= 1; }
    return 0;
}

int lg_obs_norm_get_state(lg_obs_norm *h, float *mean, float *var, float *std, int64_t *count) {
    if (!h) return refuse("get_state: null handle");
    const size_t W = (size_t)h->cfg.width;
    const float *st = h->state + (size_t)h->cur * 3 * W;
    float *dst[3] = {mean, var, std};
    if (hipDeviceSynchronize() != hipSuccess) { lg_set_error("lg_obs_norm: get_state: the device reports an error"); return -100; }
    for (int k = 0; k < 3; ++k)
        if (dst[k] && hipMemcpy(dst[k], st + k * W, W * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            lg_set_error("lg_obs_norm: get_state: copying the state to the host failed");
            return -100;
        }
    if (count) *count = h->count;
    return 0;
}

int lg_obs_norm_set_state(lg_obs_norm *h, const float *mean, const float *var, int64_t count) {
    if (!h || !mean || !var) return refuse("set_state: null argument");
    if (count < 0) return refuse("set_state: count = " + S(count) + " is negative");
    for (int j = 0; j < h->cfg.width; ++j) {
        if (!std::isfinite(mean[j])) return refuse("set_state: mean[" + S(j) + "] = " + std::to_string(mean[j]) + " is not finite");
        if (!std::isfinite(var[j]) || var[j] < 0.0f)
            return refuse("set_state: var[" + S(j) + "] = " + std::to_string(var[j]) + " must be finite and not negative");
    }
    if (int rc = write_state(h, mean, var)) return rc;
    h->count = count;
    return 0;
}

}  // extern "C"
