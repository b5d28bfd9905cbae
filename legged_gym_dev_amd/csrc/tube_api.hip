// C-ABI (include/legged_hip.h, lg_tube_*) of the tube-model trainer: parameter / optimiser / slab allocation in HBM, epoch
// permutation, the two launches of a training step, the eval launch, and the inference entries: predict, window prediction and
// the closed-loop roll-outs, single-tap and windowed, and the level entries of a level-conditioned model, flat or horizon (tube_kernels.hip).  lg_tube_sweep_*: K such trainers of one shape on one
// dataset, stepped by the same two launches with the members along grid y.
// The planner entries, which read a handle's TubeDev and nothing else of it (lg_internal_tube_dev), are plan_api.hip's.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "tube_device.h"
#include "lg_internal.h"

struct TubeCaps {                       // rows that a model's data-sized buffers hold
    int64_t starts = 0, perm = 0, evpart = 0, levels = 0;
};

struct lg_tube {
    lg_tube_cfg cfg;
    TubeDev dev;
    TubeSplit split[2];                 // train, test
    hipStream_t stream = nullptr;
    int64_t t = 0;                      // Adam steps taken
    int64_t pos = 0;                    // rows of the epoch permutation consumed
    int64_t eval_count = 0;
    TubeCaps caps;
    int64_t eval_rows_cap = 0;
    int32_t *eval_rows = nullptr;
};

struct lg_tube_sweep {
    std::vector<lg_tube_cfg> cfg;       // per member
    std::vector<TubeMember> mem;        // host copy of the member array
    std::vector<TubeCaps> caps;
    TubeMember *dmem = nullptr;         // device copy, what the kernels index by blockIdx.y
    TubeSplit split[2];                 // shared by all members
    hipStream_t stream = nullptr;
    int64_t t = 0, pos = 0, eval_count = 0;   // the members step together
    int64_t eval_rows_cap = 0;
    int32_t *eval_rows = nullptr;
};

static bool talloc(void **q, size_t bytes) {
    *q = nullptr;
    if (bytes == 0) bytes = 4;
    return hipMalloc(q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess;
}

static float loss_norm(const lg_tube_cfg &c, int64_t rows) {
    return (float)(c.loss == LG_TUBE_LOSS_VECTOR ? rows : rows * (int64_t)c.output_dim);
}

// why a configuration lies outside the supported envelope; empty inside it
static std::string cfg_reason(const lg_tube_cfg *c) {
    if (c->num_units < 16 || c->num_units > LG_TUBE_MAX_UNITS || c->num_units % 16) return "num_units must be 16..128 in steps of 16";
    if (c->num_layers < 1 || c->num_layers > 4) return "num_layers must be 1..4";
    if (c->input_dim < 1 || c->input_dim > LG_TUBE_MAX_IN) return "input_dim must be 1..256";
    if (c->output_dim < 1 || c->output_dim > LG_TUBE_MAX_OUT) return "output_dim must be 1..64";
    if (c->activation < 0 || c->activation > 3) return "activation must be relu, softplus, tanh or elu";
    if (c->loss < 0 || c->loss > 2) return "loss must be scalar (0), vector (1) or mse (2)";
    if (c->batch_size < 1) return "batch_size must be positive";
    if (c->step_size < 1) return "step_size must be positive";
    if (c->horizon && (c->H_rev < 0 || c->H_fwd < 1 || c->output_dim != c->H_fwd)) return "horizon dataset: output_dim must equal H_fwd";
    if (c->activation == LG_TUBE_ACT_SOFTPLUS && !(c->softplus_beta > 0.f)) return "softplus_beta must be positive";
    if (c->level_input != 0 && c->level_input != 1) return "level_input must be 0 or 1";
    if (c->level_input) {
        if (c->loss == LG_TUBE_LOSS_MSE) return "level_input needs a tube loss (scalar or vector): the mse loss has no level";
        if (c->horizon && c->H_rev < 1) return "level_input with horizon = 1 needs H_rev >= 1: an item without a past error has no error history (use a flat level kind)";
        if (c->input_dim < 2) return "level_input: input_dim counts the level column and must be at least 2";
        if (!(c->level_lo >= 0.f && c->level_lo < c->level_hi && c->level_hi <= 1.f)) return "level range must satisfy 0 <= level_lo < level_hi <= 1";
    }
    return "";
}

// One model's device struct and the buffers whose size the configuration fixes; false on a failed allocation (the caller frees).
static bool dev_init(const lg_tube_cfg *cfg, TubeDev &D) {
    memset(&D, 0, sizeof(D));
    D.in_dim = cfg->input_dim; D.out_dim = cfg->output_dim; D.units = cfg->num_units; D.layers = cfg->num_layers;
    D.act = cfg->activation; D.loss = cfg->loss; D.horizon = cfg->horizon; D.H_fwd = cfg->H_fwd; D.H_rev = cfg->H_rev;
    D.alpha = cfg->alpha; D.delta = cfg->delta; D.sp_beta = cfg->activation == LG_TUBE_ACT_SOFTPLUS ? cfg->softplus_beta : 1.f;
    D.seed = cfg->seed;
    D.level_input = cfg->level_input; D.level_lo = cfg->level_lo; D.level_hi = cfg->level_hi;
    int64_t off = 0;
    for (int li = 0; li <= D.layers; ++li) {        // state-dict order: layers.{2 li}.weight (out, in), layers.{2 li}.bias
        D.din[li] = li == 0 ? D.in_dim : D.units;
        D.dout[li] = li == D.layers ? D.out_dim : D.units;
        D.off_w[li] = off; off += (int64_t)D.din[li] * D.dout[li];
        D.off_b[li] = off; off += D.dout[li];
    }
    D.num_params = off;
    D.slab_ld = (off + 1 + 63) / 64 * 64;
    D.log_cap = 65536;
    const int64_t nwg = (cfg->batch_size + LG_TUBE_ROWS - 1) / LG_TUBE_ROWS;
    return talloc((void **)&D.params, off * 4) && talloc((void **)&D.wt, off * 4) && talloc((void **)&D.grads, off * 4) &&
           talloc((void **)&D.adam_m, off * 4) && talloc((void **)&D.adam_v, off * 4) &&
           talloc((void **)&D.slab, (size_t)nwg * D.slab_ld * 4) && talloc((void **)&D.normpart, 1024 * 4) &&
           talloc((void **)&D.done_ctr, 4) && talloc((void **)&D.log, (size_t)D.log_cap * 16) && talloc((void **)&D.eval, 16);
}

static void dev_free(TubeDev &D) {
    for (void *q : {(void *)D.params, (void *)D.wt, (void *)D.grads, (void *)D.adam_m, (void *)D.adam_v, (void *)D.slab,
                    (void *)D.evpart, (void *)D.normpart, (void *)D.done_ctr, (void *)D.log, (void *)D.eval, (void *)D.starts,
                    (void *)D.perm, (void *)D.levels})
        if (q) (void)hipFree(q);
}

// what is wrong with a split handed to set_data (null: nothing); a horizon split's T, nz, m are taken into D
static const char *data_reason(TubeDev &D, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T, int32_t nz,
                               int32_t m) {
    if (which != 0 && which != 1) return "which must be 0 (train) or 1 (test)";
    if (rows < 1 || rows > INT32_MAX) return "rows must be 1..2^31-1";
    if (!x || (!D.horizon && !y) || (D.horizon && ((nz && !y) || (m && !v)))) return "missing array";
    if (D.horizon) {
        if (nz < 0 || m < 0 || window_dim(D, nz, m) != D.in_dim)
            return D.level_input ? "input_dim != H_rev + nz + (H_rev + H_fwd) * m + 1 (the level column)" : "input_dim != H_rev + nz + (H_rev + H_fwd) * m";
        if (T - D.H_fwd - 1 <= D.H_rev) return "T - H_fwd - 1 must exceed H_rev";
        if ((D.T && D.T != T) || (D.nz && D.nz != nz) || (D.m && D.m != m)) return "train and test splits differ in T, nz or m";
        D.T = T; D.nz = nz; D.m = m;
    }
    return nullptr;
}

// grow one model's starts / perm / evpart to a split of `rows` rows; false on a failed allocation
static bool data_alloc(TubeDev &D, TubeCaps &c, int which, int64_t rows, int64_t batch_size) {
    const int64_t need = rows > batch_size ? rows : batch_size;
    if (need > c.starts) {
        if (D.starts) (void)hipFree(D.starts);
        if (!talloc((void **)&D.starts, need * 4)) { D.starts = nullptr; c.starts = 0; return false; }
        c.starts = need;
    }
    if (D.level_input && need > c.levels) {
        if (D.levels) (void)hipFree(D.levels);
        if (!talloc((void **)&D.levels, need * 4)) { D.levels = nullptr; c.levels = 0; return false; }
        c.levels = need;
    }
    if (which == 0 && rows > c.perm) {
        if (D.perm) (void)hipFree(D.perm);
        if (!talloc((void **)&D.perm, rows * 4)) { D.perm = nullptr; c.perm = 0; return false; }
        c.perm = rows;
    }
    if (which == 1 && rows > c.evpart) {
        if (D.evpart) (void)hipFree(D.evpart);
        if (!talloc((void **)&D.evpart, (rows + LG_TUBE_ROWS - 1) / LG_TUBE_ROWS * 16)) { D.evpart = nullptr; c.evpart = 0; return false; }
        c.evpart = rows;
    }
    return true;
}

// the test split's row list 0..rows-1, grown on demand
static bool eval_rows_alloc(int32_t **eval_rows, int64_t *cap, int64_t rows, hipStream_t stream) {
    if (rows > *cap) {
        if (*eval_rows) (void)hipFree(*eval_rows);
        if (!talloc((void **)eval_rows, rows * 4)) { *eval_rows = nullptr; *cap = 0; return false; }
        *cap = rows;
    }
    tubek_iota(*eval_rows, rows, stream);
    return true;
}

static void fill_buffers(const TubeDev &D, const TubeCaps &c, int64_t t, lg_tube_buffers *out) {
    out->params = D.params; out->grads = D.grads; out->adam_m = D.adam_m; out->adam_v = D.adam_v;
    out->log = D.log; out->eval = D.eval; out->starts = D.starts; out->perm = D.perm;
    out->num_params = D.num_params; out->log_cap = D.log_cap; out->starts_cap = c.starts; out->perm_cap = c.perm;
    out->step = t;
    out->levels = D.levels; out->levels_cap = c.levels;
}

static int fill_layout(const TubeDev &D, int64_t *offsets, int64_t *shapes, int max_entries, const char *who) {
    const int n = 2 * (D.layers + 1);
    if (max_entries < n) { lg_set_error(std::string(who) + ": max_entries too small"); return -1; }
    for (int li = 0; li <= D.layers; ++li) {
        offsets[2 * li] = D.off_w[li]; shapes[4 * li] = D.dout[li]; shapes[4 * li + 1] = D.din[li];
        offsets[2 * li + 1] = D.off_b[li]; shapes[4 * li + 2] = D.dout[li]; shapes[4 * li + 3] = 0;
    }
    return n;
}

extern "C" {

int lg_tube_check_cfg(const lg_tube_cfg *c) {
    const std::string e = cfg_reason(c);
    if (!e.empty()) { lg_set_error("lg_tube: " + e); return -1; }
    return 0;
}

int lg_tube_create(const lg_tube_cfg *cfg, lg_tube **out) {
    *out = nullptr;
    if (lg_tube_check_cfg(cfg)) return -1;
    if (tubek_init()) { lg_set_error("lg_tube_create: hipFuncSetAttribute failed"); return -2; }
    lg_tube *p = new lg_tube();
    p->cfg = *cfg;
    const bool ok = dev_init(cfg, p->dev);
    if (!ok) { lg_set_error("hipMalloc failed in lg_tube_create"); lg_tube_destroy(p); return -100; }
    *out = p;
    return 0;
}

int lg_tube_destroy(lg_tube *p) {
    if (!p) return 0;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    else (void)hipDeviceSynchronize();
    dev_free(p->dev);
    if (p->eval_rows) (void)hipFree(p->eval_rows);
    delete p;
    return 0;
}

int lg_tube_set_stream(lg_tube *p, void *stream) { p->stream = (hipStream_t)stream; return 0; }

// for plan_api.hip (lg_internal.h)
const TubeDev *lg_internal_tube_dev(const lg_tube *p) { return p ? &p->dev : nullptr; }

int lg_tube_get_buffers(lg_tube *p, lg_tube_buffers *out) {
    fill_buffers(p->dev, p->caps, p->t, out);
    return 0;
}

int lg_tube_param_layout(lg_tube *p, int64_t *offsets, int64_t *shapes, int max_entries) {
    return fill_layout(p->dev, offsets, shapes, max_entries, "lg_tube_param_layout");
}

int lg_tube_params_changed(lg_tube *p) { tubek_wt(&p->dev, p->stream); return 0; }

int lg_tube_set_step(lg_tube *p, int64_t t) {
    if (t < 0) { lg_set_error("lg_tube_set_step: negative step"); return -1; }
    p->t = t;
    return 0;
}

int lg_tube_set_data(lg_tube *p, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T, int32_t nz,
                     int32_t m) {
    TubeDev &D = p->dev;
    if (const char *e = data_reason(D, which, x, y, v, rows, T, nz, m)) { lg_set_error(std::string("lg_tube_set_data: ") + e); return -1; }
    p->split[which] = TubeSplit{x, y, v, rows};
    if (!data_alloc(D, p->caps, which, rows, p->cfg.batch_size) ||
        (which == 1 && !eval_rows_alloc(&p->eval_rows, &p->eval_rows_cap, rows, p->stream))) {
        lg_set_error("hipMalloc failed"); return -100;
    }
    return 0;
}

int lg_tube_begin_epoch(lg_tube *p, int64_t epoch) {
    if (!p->split[0].rows) { lg_set_error("lg_tube_begin_epoch: no training data (lg_tube_set_data)"); return -1; }
    tubek_perm(&p->dev, (int)p->split[0].rows, (uint64_t)epoch, p->stream);
    p->pos = 0;
    return 0;
}

int lg_tube_step(lg_tube *p, const int32_t *rows, int64_t count) {
    if (!p->split[0].rows) { lg_set_error("lg_tube_step: no training data (lg_tube_set_data)"); return -1; }
    if (count < 1 || count > p->cfg.batch_size) { lg_set_error("lg_tube_step: count must be 1..batch_size"); return -1; }
    const int32_t *r = rows;
    if (!r) {
        if (p->pos + count > p->split[0].rows) { lg_set_error("lg_tube_step: the epoch's permutation is used up (lg_tube_begin_epoch)"); return -1; }
        r = p->dev.perm + p->pos;
        p->pos += count;
    }
    const float norm = loss_norm(p->cfg, count);
    ++p->t;
    tubek_step(&p->dev, &p->split[0], r, count, (uint64_t)p->t, norm, p->stream);
    tubek_adam(&p->dev, (int)((count + LG_TUBE_ROWS - 1) / LG_TUBE_ROWS), p->t, (double)p->cfg.lr, (double)p->cfg.gamma,
               (int64_t)p->cfg.step_size, norm, count, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_step: launch failed"), -3);
}

int lg_tube_eval(lg_tube *p) {
    const TubeSplit &S = p->split[1];
    if (!S.rows) { lg_set_error("lg_tube_eval: no test data (lg_tube_set_data with which = 1)"); return -1; }
    const uint64_t key = 0x8000000000000000ull | (uint64_t)p->eval_count++;
    tubek_eval(&p->dev, &S, p->eval_rows, key, loss_norm(p->cfg, S.rows), -1.f, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_eval: launch failed"), -3);
}

int lg_tube_eval_level(lg_tube *p, float level) {
    const TubeSplit &S = p->split[1];
    if (!p->dev.level_input) { lg_set_error("lg_tube_eval_level: the handle is not level-conditioned (lg_tube_cfg.level_input)"); return -1; }
    if (!(level >= 0.f && level <= 1.f)) { lg_set_error("lg_tube_eval_level: level must lie in 0..1"); return -1; }
    if (!S.rows) { lg_set_error("lg_tube_eval_level: no test data (lg_tube_set_data with which = 1)"); return -1; }
    tubek_eval(&p->dev, &S, p->eval_rows, 0, loss_norm(p->cfg, S.rows), level, p->stream);     // nothing is drawn: no key
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_eval_level: launch failed"), -3);
}

// ---------------------------------------------------------------- inference: reads params / wt, changes neither
int lg_tube_predict(lg_tube *p, const float *x, const int32_t *rows, int64_t count, float *out) {
    if (p->dev.horizon) { lg_set_error("lg_tube_predict: a horizon handle predicts windows (lg_tube_predict_windows)"); return -1; }
    if (count < 1) { lg_set_error("lg_tube_predict: count must be positive"); return -1; }
    if (!x || !out) { lg_set_error("lg_tube_predict: missing array"); return -1; }
    tubek_predict(&p->dev, x, nullptr, nullptr, rows, nullptr, nullptr, 0, 0, 0, count, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict: launch failed"), -3);
}

int lg_tube_predict_levels(lg_tube *p, const float *x, const int32_t *rows, int64_t count, const float *levels, int32_t n_levels,
                           float *out) {
    if (!p->dev.level_input) { lg_set_error("lg_tube_predict_levels: the handle is not level-conditioned (lg_tube_cfg.level_input)"); return -1; }
    if (count < 1) { lg_set_error("lg_tube_predict_levels: count must be positive"); return -1; }
    if (n_levels < 1 || n_levels > LG_TUBE_MAX_LEVELS) { lg_set_error("lg_tube_predict_levels: n_levels must be 1..64"); return -1; }
    if (!x || !levels || !out) { lg_set_error("lg_tube_predict_levels: missing array"); return -1; }
    tubek_predict_levels(&p->dev, x, rows, count, levels, n_levels, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict_levels: launch failed"), -3);
}

// what is wrong with a window query on a horizon handle (null: nothing)
static const char *windows_reason(const TubeDev &D, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz,
                                  int32_t m, const int32_t *env, const int32_t *start, int64_t count, const float *out) {
    if (count < 1 || n < 1) return "n and count must be positive";
    if (nz < 0 || m < 0 || window_dim(D, nz, m) != D.in_dim)
        return D.level_input ? "input_dim != H_rev + nz + (H_rev + H_fwd) * m + 1 (the level column)" : "input_dim != H_rev + nz + (H_rev + H_fwd) * m";
    if (T < D.H_rev + D.H_fwd) return "T is shorter than H_rev + H_fwd";
    if (!w || (nz && !z) || (m && !v) || !env || !start || !out) return "missing array";
    return nullptr;
}

int lg_tube_predict_windows(lg_tube *p, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz, int32_t m,
                            const int32_t *env, const int32_t *start, int64_t count, float *out) {
    const TubeDev &D = p->dev;
    if (!D.horizon) { lg_set_error("lg_tube_predict_windows: a flat handle predicts rows (lg_tube_predict)"); return -1; }
    if (D.level_input) {
        lg_set_error("lg_tube_predict_windows: the handle is level-conditioned (lg_tube_cfg.level_input): a window has no level, use "
                     "lg_tube_predict_windows_levels");
        return -1;
    }
    if (const char *e = windows_reason(D, w, z, v, n, T, nz, m, env, start, count, out)) {
        lg_set_error(std::string("lg_tube_predict_windows: ") + e); return -1;
    }
    tubek_predict(&p->dev, w, z, v, nullptr, env, start, T, nz, m, count, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict_windows: launch failed"), -3);
}

int lg_tube_predict_windows_levels(lg_tube *p, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz,
                                   int32_t m, const int32_t *env, const int32_t *start, int64_t count, const float *levels,
                                   int32_t n_levels, float *out) {
    const TubeDev &D = p->dev;
    const char *e = nullptr;
    if (!D.level_input) e = "the handle is not level-conditioned (lg_tube_cfg.level_input)";
    else if (!D.horizon) e = "not a horizon handle (lg_tube_cfg.horizon): a flat handle predicts rows (lg_tube_predict_levels)";
    else if (n_levels < 1 || n_levels > LG_TUBE_MAX_LEVELS) e = "n_levels must be 1..64";
    else if (!levels) e = "missing array";
    else e = windows_reason(D, w, z, v, n, T, nz, m, env, start, count, out);
    if (e) { lg_set_error(std::string("lg_tube_predict_windows_levels: ") + e); return -1; }
    tubek_predict_windows_levels(&p->dev, w, z, v, env, start, T, nz, m, count, levels, n_levels, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict_windows_levels: launch failed"), -3);
}

int lg_tube_rollout(lg_tube *p, const float *x, int64_t n_seq, int32_t T, int32_t fb, const uint8_t *reseed, float *out) {
    const TubeDev &D = p->dev;
    if (D.horizon) { lg_set_error("lg_tube_rollout: a horizon handle has no closed loop (lg_tube_predict_windows)"); return -1; }
    if (n_seq < 1 || T < 1) { lg_set_error("lg_tube_rollout: n_seq and T must be positive"); return -1; }
    if (n_seq > INT32_MAX / 16) { lg_set_error("lg_tube_rollout: n_seq must be below 2^27"); return -1; }
    if (fb < 0 || fb > D.in_dim || fb > D.out_dim) { lg_set_error("lg_tube_rollout: fb must be 0..min(input_dim, output_dim)"); return -1; }
    if (!x || !out) { lg_set_error("lg_tube_rollout: missing array"); return -1; }
    tubek_rollout(&p->dev, x, n_seq, T, fb, reseed, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_rollout: launch failed"), -3);
}

int lg_tube_rollout_window(lg_tube *p, const float *x, int64_t n_seq, int32_t T, int32_t fb, int32_t taps, int32_t dN, int32_t stride,
                           const uint8_t *reseed, float *out) {
    const TubeDev &D = p->dev;
    const char *e = nullptr;
    if (D.horizon) e = "a horizon handle has no closed loop (lg_tube_predict_windows)";
    else if (n_seq < 1 || T < 1) e = "n_seq and T must be positive";
    else if (n_seq > INT32_MAX / 16) e = "n_seq must be below 2^27";
    else if (fb < 1 || taps < 1 || dN < 1) e = "fb, taps and dN must be at least 1";
    else if (fb > D.out_dim) e = "fb must not exceed output_dim";
    else if (taps > 1 && stride < fb) e = "stride must be at least fb";
    else if ((int64_t)(taps - 1) * (taps > 1 ? stride : 0) + fb > D.in_dim) e = "(taps - 1) * stride + fb must not exceed input_dim";
    else if (((int64_t)(taps - 1) * dN + 1) * fb > LG_TUBE_RING_MAX) e = "the ring ((taps - 1) * dN + 1) * fb must not exceed 1024 floats per sequence";
    else if (!x || !out) e = "missing array";
    if (e) { lg_set_error(std::string("lg_tube_rollout_window: ") + e); return -1; }
    tubek_rollout_window(&p->dev, x, n_seq, T, fb, taps, dN, taps > 1 ? stride : D.in_dim, reseed, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_rollout_window: launch failed"), -3);
}

// ---------------------------------------------------------------- sweep: K trainers of one shape on one dataset
static int sweep_upload(lg_tube_sweep *s) {       // the device copy of the member array follows the host copy
    if (hipMemcpyAsync(s->dmem, s->mem.data(), s->mem.size() * sizeof(TubeMember), hipMemcpyHostToDevice, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess) {
        lg_set_error("lg_tube_sweep: copying the member array failed"); return -3;
    }
    return 0;
}

static bool sweep_member(const lg_tube_sweep *s, int32_t k, const char *who) {
    if (k >= 0 && k < (int32_t)s->mem.size()) return true;
    lg_set_error(std::string(who) + ": member " + std::to_string(k) + " is outside 0.." + std::to_string(s->mem.size() - 1));
    return false;
}

int lg_tube_sweep_create(const lg_tube_cfg *cfgs, int32_t K, lg_tube_sweep **out) {
    *out = nullptr;
    if (K < 1 || K > LG_TUBE_SWEEP_MAX) {
        lg_set_error("lg_tube_sweep_create: K = " + std::to_string(K) + " must be 1.." + std::to_string(LG_TUBE_SWEEP_MAX)); return -1;
    }
    for (int k = 0; k < K; ++k) {
        const std::string e = cfg_reason(cfgs + k);
        if (!e.empty()) { lg_set_error("lg_tube_sweep_create: member " + std::to_string(k) + ": " + e); return -1; }
    }
    for (int k = 1; k < K; ++k) {
        const lg_tube_cfg &a = cfgs[0], &b = cfgs[k];
        const char *f = a.input_dim != b.input_dim ? "input_dim" : a.output_dim != b.output_dim ? "output_dim"
                      : a.num_units != b.num_units ? "num_units" : a.num_layers != b.num_layers ? "num_layers"
                      : a.loss != b.loss ? "loss" : a.horizon != b.horizon ? "horizon" : a.H_fwd != b.H_fwd ? "H_fwd"
                      : a.H_rev != b.H_rev ? "H_rev" : a.batch_size != b.batch_size ? "batch_size"
                      : a.level_input != b.level_input ? "level_input" : nullptr;
        if (f) {
            lg_set_error(std::string("lg_tube_sweep_create: ") + f + " differs between member 0 and member " + std::to_string(k) +
                         " (the members of a sweep share it)");
            return -1;
        }
    }
    if (tubek_init()) { lg_set_error("lg_tube_sweep_create: hipFuncSetAttribute failed"); return -2; }
    lg_tube_sweep *s = new lg_tube_sweep();
    s->cfg.assign(cfgs, cfgs + K);
    s->mem.resize(K);
    s->caps.resize(K);
    for (int k = 0; k < K; ++k) memset(&s->mem[k], 0, sizeof(TubeMember));
    bool ok = talloc((void **)&s->dmem, (size_t)K * sizeof(TubeMember));
    for (int k = 0; ok && k < K; ++k) {
        ok = dev_init(cfgs + k, s->mem[k].dev);
        s->mem[k].lr0 = cfgs[k].lr; s->mem[k].gamma = cfgs[k].gamma; s->mem[k].step_size = cfgs[k].step_size;
    }
    if (!ok) {
        lg_set_error("hipMalloc failed in lg_tube_sweep_create (a sweep of " + std::to_string(K) + " members takes " + std::to_string(K) +
                     " times a single trainer's memory)");
        lg_tube_sweep_destroy(s);
        return -100;
    }
    if (sweep_upload(s)) { lg_tube_sweep_destroy(s); return -3; }
    *out = s;
    return 0;
}

int lg_tube_sweep_destroy(lg_tube_sweep *s) {
    if (!s) return 0;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    else (void)hipDeviceSynchronize();
    for (TubeMember &m : s->mem) dev_free(m.dev);
    if (s->dmem) (void)hipFree(s->dmem);
    if (s->eval_rows) (void)hipFree(s->eval_rows);
    delete s;
    return 0;
}

int lg_tube_sweep_set_stream(lg_tube_sweep *s, void *stream) { s->stream = (hipStream_t)stream; return 0; }

int lg_tube_sweep_get_buffers(lg_tube_sweep *s, int32_t k, lg_tube_buffers *out) {
    if (!sweep_member(s, k, "lg_tube_sweep_get_buffers")) return -1;
    fill_buffers(s->mem[k].dev, s->caps[k], s->t, out);
    return 0;
}

int lg_tube_sweep_param_layout(lg_tube_sweep *s, int64_t *offsets, int64_t *shapes, int max_entries) {
    return fill_layout(s->mem[0].dev, offsets, shapes, max_entries, "lg_tube_sweep_param_layout");
}

// one k_tube_wt launch per member asked for (K launches for k = -1): initialisation and checkpoint loads, not the step
int lg_tube_sweep_params_changed(lg_tube_sweep *s, int32_t k) {
    if (k != -1 && !sweep_member(s, k, "lg_tube_sweep_params_changed")) return -1;
    for (int32_t i = k < 0 ? 0 : k; i < (k < 0 ? (int32_t)s->mem.size() : k + 1); ++i) tubek_wt(&s->mem[i].dev, s->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_sweep_params_changed: launch failed"), -3);
}

int lg_tube_sweep_set_step(lg_tube_sweep *s, int64_t t) {
    if (t < 0) { lg_set_error("lg_tube_sweep_set_step: negative step"); return -1; }
    s->t = t;
    return 0;
}

int lg_tube_sweep_set_data(lg_tube_sweep *s, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T,
                           int32_t nz, int32_t m) {
    // every member is asked: data_reason also records a horizon split's T / nz / m in that member's TubeDev (the members share the
    // shape, so they all give the same verdict)
    for (size_t k = 0; k < s->mem.size(); ++k)
        if (const char *e = data_reason(s->mem[k].dev, which, x, y, v, rows, T, nz, m)) {
            lg_set_error(std::string("lg_tube_sweep_set_data: ") + e); return -1;
        }
    s->split[which] = TubeSplit{x, y, v, rows};
    bool ok = true;
    for (size_t k = 0; ok && k < s->mem.size(); ++k) ok = data_alloc(s->mem[k].dev, s->caps[k], which, rows, s->cfg[k].batch_size);
    ok = ok && (which != 1 || eval_rows_alloc(&s->eval_rows, &s->eval_rows_cap, rows, s->stream));
    const int rc = sweep_upload(s);                 // also after a failure: the array must not keep a freed pointer
    if (!ok) { lg_set_error("hipMalloc failed in lg_tube_sweep_set_data"); return -100; }
    return rc;
}

int lg_tube_sweep_begin_epoch(lg_tube_sweep *s, int64_t epoch) {
    if (!s->split[0].rows) { lg_set_error("lg_tube_sweep_begin_epoch: no training data (lg_tube_sweep_set_data)"); return -1; }
    tubek_perm_sweep(s->dmem, (int)s->mem.size(), (int)s->split[0].rows, (uint64_t)epoch, s->stream);
    s->pos = 0;
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_sweep_begin_epoch: launch failed"), -3);
}

int lg_tube_sweep_step(lg_tube_sweep *s, const int32_t *rows, int64_t count) {
    if (!s->split[0].rows) { lg_set_error("lg_tube_sweep_step: no training data (lg_tube_sweep_set_data)"); return -1; }
    if (count < 1 || count > s->cfg[0].batch_size) { lg_set_error("lg_tube_sweep_step: count must be 1..batch_size"); return -1; }
    int64_t pos = 0;
    if (!rows) {
        if (s->pos + count > s->split[0].rows) {
            lg_set_error("lg_tube_sweep_step: the epoch's permutation is used up (lg_tube_sweep_begin_epoch)"); return -1;
        }
        pos = s->pos;
        s->pos += count;
    }
    const float norm = loss_norm(s->cfg[0], count);
    const int K = (int)s->mem.size();
    ++s->t;
    tubek_step_sweep(s->dmem, K, &s->mem[0].dev, &s->split[0], rows, pos, count, (uint64_t)s->t, norm, s->stream);
    tubek_adam_sweep(s->dmem, K, &s->mem[0].dev, (int)((count + LG_TUBE_ROWS - 1) / LG_TUBE_ROWS), s->t, norm, count, s->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_sweep_step: launch failed"), -3);
}

int lg_tube_sweep_eval(lg_tube_sweep *s) {
    const TubeSplit &S = s->split[1];
    if (!S.rows) { lg_set_error("lg_tube_sweep_eval: no test data (lg_tube_sweep_set_data with which = 1)"); return -1; }
    const uint64_t key = 0x8000000000000000ull | (uint64_t)s->eval_count++;
    tubek_eval_sweep(s->dmem, (int)s->mem.size(), &s->mem[0].dev, &S, s->eval_rows, key, loss_norm(s->cfg[0], S.rows), -1.f, s->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_sweep_eval: launch failed"), -3);
}

int lg_tube_sweep_eval_level(lg_tube_sweep *s, float level) {
    const TubeSplit &S = s->split[1];
    if (!s->mem[0].dev.level_input) { lg_set_error("lg_tube_sweep_eval_level: the sweep is not level-conditioned (lg_tube_cfg.level_input)"); return -1; }
    if (!(level >= 0.f && level <= 1.f)) { lg_set_error("lg_tube_sweep_eval_level: level must lie in 0..1"); return -1; }
    if (!S.rows) { lg_set_error("lg_tube_sweep_eval_level: no test data (lg_tube_sweep_set_data with which = 1)"); return -1; }
    tubek_eval_sweep(s->dmem, (int)s->mem.size(), &s->mem[0].dev, &S, s->eval_rows, 0, loss_norm(s->cfg[0], S.rows), level, s->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_sweep_eval_level: launch failed"), -3);
}

}  // extern "C"
