// C-ABI (include/legged_hip.h, lg_tube_*) of the tube-model trainer: parameter / optimiser / slab allocation in HBM, epoch
// permutation, the two launches of a training step, the eval launch, and the inference entries: predict, window prediction and
// the closed-loop roll-outs, single-tap and windowed, and the level entries of a level-conditioned model, flat or horizon (tube_kernels.hip).
// One trainer, TubeTrainer: K models of one shape on one dataset, stepped by the same two launches.  lg_tube is K = 1 and
// lg_tube_sweep_* any K; every training operation is written once (trainer_*) and the entries of both families forward to it
// with their name, which the error texts carry.
// The K == 1 rule: one member is launched through the by-value kernels (k_tube_rows, k_tube_adam, ...: TubeDev in the kernel
// arguments), K > 1 through the member-array kernels (*_sweep, the members along grid y).  The two sets compute the same bits; the
// member-array set measured 1.2 us per step slower at K = 1 on the level-conditioned default config.
// Waiting: with K > 1, create and set_data copy the member array to the device and wait for the handle's stream; nothing else
// waits, and with one member nothing does.
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

struct TubeTrainer {
    std::vector<lg_tube_cfg> cfg;       // per member
    std::vector<TubeMember> mem;        // host copy of the member array; mem[0].dev is what inference and the planner read
    std::vector<TubeCaps> caps;
    TubeMember *dmem = nullptr;         // device copy, what the member-array kernels index by blockIdx.y (K > 1)
    TubeSplit split[2];                 // train, test; shared by all members
    hipStream_t stream = nullptr;
    int64_t t = 0;                      // Adam steps taken; the members step together
    int64_t pos = 0;                    // rows of the epoch permutation consumed
    int64_t eval_count = 0;
    int64_t eval_rows_cap = 0;
    int32_t *eval_rows = nullptr;
};
struct lg_tube : TubeTrainer {};        // K = 1
struct lg_tube_sweep : TubeTrainer {};

// what an entry's error texts take from its family: the prefix of its name and what it calls its handle
struct Family { const char *prefix, *noun; };
static const Family SINGLE{"lg_tube", "handle"}, SWEEP{"lg_tube_sweep", "sweep"};

static std::string entry(const Family &f, const char *fn) { return std::string(f.prefix) + "_" + fn; }
static int refuse(const Family &f, const char *fn, const std::string &why, int rc = -1) {
    lg_set_error(entry(f, fn) + ": " + why);
    return rc;
}
static int launched(const Family &f, const char *fn) { return hipGetLastError() == hipSuccess ? 0 : refuse(f, fn, "launch failed", -3); }

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

// ---------------------------------------------------------------- the trainer: every operation once, for both families
static int trainer_upload(TubeTrainer &T, const Family &f) {   // the device copy of the member array follows the host copy
    if (T.mem.size() == 1) return 0;    // one member goes to its kernels by value: nothing reads the device copy
    if (hipMemcpyAsync(T.dmem, T.mem.data(), T.mem.size() * sizeof(TubeMember), hipMemcpyHostToDevice, T.stream) != hipSuccess ||
        hipStreamSynchronize(T.stream) != hipSuccess) {
        lg_set_error(std::string(f.prefix) + ": copying the member array failed"); return -3;
    }
    return 0;
}

static bool trainer_member(const TubeTrainer &T, const Family &f, const char *fn, int32_t k) {
    if (k >= 0 && k < (int32_t)T.mem.size()) return true;
    refuse(f, fn, "member " + std::to_string(k) + " is outside 0.." + std::to_string(T.mem.size() - 1));
    return false;
}

template <class H>
static int trainer_destroy(H *p) {
    if (!p) return 0;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    else (void)hipDeviceSynchronize();
    for (TubeMember &m : p->mem) dev_free(m.dev);
    if (p->dmem) (void)hipFree(p->dmem);
    if (p->eval_rows) (void)hipFree(p->eval_rows);
    delete p;
    return 0;
}

// cfgs: K configurations that the caller has checked
template <class H>
static int trainer_create(const Family &f, const lg_tube_cfg *cfgs, int32_t K, H **out) {
    if (tubek_init()) return refuse(f, "create", "hipFuncSetAttribute failed", -2);
    H *p = new H();
    p->cfg.assign(cfgs, cfgs + K);
    p->mem.resize(K);                   // zeroed: a member that dev_init never reached frees nothing
    p->caps.resize(K);
    bool ok = talloc((void **)&p->dmem, (size_t)K * sizeof(TubeMember));
    for (int k = 0; ok && k < K; ++k) {
        ok = dev_init(cfgs + k, p->mem[k].dev);
        p->mem[k].lr0 = cfgs[k].lr; p->mem[k].gamma = cfgs[k].gamma; p->mem[k].step_size = cfgs[k].step_size;
    }
    if (!ok) {
        std::string e = "hipMalloc failed in " + entry(f, "create");
        if (&f == &SWEEP) e += " (a sweep of " + std::to_string(K) + " members takes " + std::to_string(K) + " times a single trainer's memory)";
        lg_set_error(e);
        trainer_destroy(p);
        return -100;
    }
    if (trainer_upload(*p, f)) { trainer_destroy(p); return -3; }
    *out = p;
    return 0;
}

static int trainer_get_buffers(TubeTrainer &T, const Family &f, int32_t k, lg_tube_buffers *out) {
    if (!trainer_member(T, f, "get_buffers", k)) return -1;
    fill_buffers(T.mem[k].dev, T.caps[k], T.t, out);
    return 0;
}

// one k_tube_wt launch per member asked for (K launches for k = -1): initialisation and checkpoint loads, not the step
static int trainer_params_changed(TubeTrainer &T, const Family &f, int32_t k) {
    if (k != -1 && !trainer_member(T, f, "params_changed", k)) return -1;
    for (int32_t i = k < 0 ? 0 : k; i < (k < 0 ? (int32_t)T.mem.size() : k + 1); ++i) tubek_wt(&T.mem[i].dev, T.stream);
    return launched(f, "params_changed");
}

static int trainer_set_step(TubeTrainer &T, const Family &f, int64_t t) {
    if (t < 0) return refuse(f, "set_step", "negative step");
    T.t = t;
    return 0;
}

static int trainer_set_data(TubeTrainer &T, const Family &f, int which, const float *x, const float *y, const float *v, int64_t rows,
                            int32_t Tn, int32_t nz, int32_t m) {
    // every member is asked: data_reason also records a horizon split's T / nz / m in that member's TubeDev (the members share the
    // shape, so they all give the same verdict)
    for (TubeMember &mb : T.mem)
        if (const char *e = data_reason(mb.dev, which, x, y, v, rows, Tn, nz, m)) return refuse(f, "set_data", e);
    T.split[which] = TubeSplit{x, y, v, rows};
    bool ok = true;
    for (size_t k = 0; ok && k < T.mem.size(); ++k) ok = data_alloc(T.mem[k].dev, T.caps[k], which, rows, T.cfg[k].batch_size);
    ok = ok && (which != 1 || eval_rows_alloc(&T.eval_rows, &T.eval_rows_cap, rows, T.stream));
    const int rc = trainer_upload(T, f);            // also after a failure: the array must not keep a freed pointer
    if (!ok) { lg_set_error("hipMalloc failed in " + entry(f, "set_data")); return -100; }
    return rc;
}

static int trainer_begin_epoch(TubeTrainer &T, const Family &f, int64_t epoch) {
    if (!T.split[0].rows) return refuse(f, "begin_epoch", "no training data (" + entry(f, "set_data") + ")");
    if (T.mem.size() == 1) tubek_perm(&T.mem[0].dev, (int)T.split[0].rows, (uint64_t)epoch, T.stream);
    else tubek_perm_sweep(T.dmem, (int)T.mem.size(), (int)T.split[0].rows, (uint64_t)epoch, T.stream);
    T.pos = 0;
    return launched(f, "begin_epoch");
}

static int trainer_step(TubeTrainer &T, const Family &f, const int32_t *rows, int64_t count) {
    if (!T.split[0].rows) return refuse(f, "step", "no training data (" + entry(f, "set_data") + ")");
    if (count < 1 || count > T.cfg[0].batch_size) return refuse(f, "step", "count must be 1..batch_size");
    int64_t pos = 0;
    if (!rows) {                        // each member's own permutation, from the shared position
        if (T.pos + count > T.split[0].rows) return refuse(f, "step", "the epoch's permutation is used up (" + entry(f, "begin_epoch") + ")");
        pos = T.pos;
        T.pos += count;
    }
    const float norm = loss_norm(T.cfg[0], count);
    const int K = (int)T.mem.size(), nwg = (int)((count + LG_TUBE_ROWS - 1) / LG_TUBE_ROWS);
    const TubeDev &D0 = T.mem[0].dev;
    ++T.t;
    if (K == 1) {                       // the K == 1 rule (top of the file)
        tubek_step(&D0, &T.split[0], rows ? rows : D0.perm + pos, count, (uint64_t)T.t, norm, T.stream);
        tubek_adam(&D0, nwg, T.t, T.cfg[0].lr, T.cfg[0].gamma, (int64_t)T.cfg[0].step_size, norm, count, T.stream);
    } else {
        tubek_step_sweep(T.dmem, K, &D0, &T.split[0], rows, pos, count, (uint64_t)T.t, norm, T.stream);
        tubek_adam_sweep(T.dmem, K, &D0, nwg, T.t, norm, count, T.stream);
    }
    return launched(f, "step");
}

// level < 0: lg_tube_eval, one drawn level per row of a level_input handle; 0..1: lg_tube_eval_level
static int trainer_eval(TubeTrainer &T, const Family &f, const char *fn, float level) {
    const TubeSplit &S = T.split[1];
    if (!S.rows) return refuse(f, fn, "no test data (" + entry(f, "set_data") + " with which = 1)");
    const uint64_t key = level < 0.f ? 0x8000000000000000ull | (uint64_t)T.eval_count++ : 0;   // a fixed level draws nothing: no key
    const float norm = loss_norm(T.cfg[0], S.rows);
    if (T.mem.size() == 1) tubek_eval(&T.mem[0].dev, &S, T.eval_rows, key, norm, level, T.stream);
    else tubek_eval_sweep(T.dmem, (int)T.mem.size(), &T.mem[0].dev, &S, T.eval_rows, key, norm, level, T.stream);
    return launched(f, fn);
}

static int trainer_eval_level(TubeTrainer &T, const Family &f, float level) {
    if (!T.mem[0].dev.level_input) return refuse(f, "eval_level", std::string("the ") + f.noun + " is not level-conditioned (lg_tube_cfg.level_input)");
    if (!(level >= 0.f && level <= 1.f)) return refuse(f, "eval_level", "level must lie in 0..1");
    return trainer_eval(T, f, "eval_level", level);
}

extern "C" {

int lg_tube_check_cfg(const lg_tube_cfg *c) {
    const std::string e = cfg_reason(c);
    if (!e.empty()) { lg_set_error("lg_tube: " + e); return -1; }
    return 0;
}

int lg_tube_create(const lg_tube_cfg *cfg, lg_tube **out) {
    *out = nullptr;
    return lg_tube_check_cfg(cfg) ? -1 : trainer_create(SINGLE, cfg, 1, out);
}
int lg_tube_destroy(lg_tube *p) { return trainer_destroy(p); }
int lg_tube_set_stream(lg_tube *p, void *stream) { p->stream = (hipStream_t)stream; return 0; }
int lg_tube_get_buffers(lg_tube *p, lg_tube_buffers *out) { return trainer_get_buffers(*p, SINGLE, 0, out); }
int lg_tube_param_layout(lg_tube *p, int64_t *offsets, int64_t *shapes, int max_entries) {
    return fill_layout(p->mem[0].dev, offsets, shapes, max_entries, "lg_tube_param_layout");
}
int lg_tube_params_changed(lg_tube *p) { return trainer_params_changed(*p, SINGLE, 0); }
int lg_tube_set_step(lg_tube *p, int64_t t) { return trainer_set_step(*p, SINGLE, t); }
int lg_tube_set_data(lg_tube *p, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T, int32_t nz,
                     int32_t m) {
    return trainer_set_data(*p, SINGLE, which, x, y, v, rows, T, nz, m);
}
int lg_tube_begin_epoch(lg_tube *p, int64_t epoch) { return trainer_begin_epoch(*p, SINGLE, epoch); }
int lg_tube_step(lg_tube *p, const int32_t *rows, int64_t count) { return trainer_step(*p, SINGLE, rows, count); }
int lg_tube_eval(lg_tube *p) { return trainer_eval(*p, SINGLE, "eval", -1.f); }
int lg_tube_eval_level(lg_tube *p, float level) { return trainer_eval_level(*p, SINGLE, level); }

// for plan_api.hip (lg_internal.h)
const TubeDev *lg_internal_tube_dev(const lg_tube *p) { return p ? &p->mem[0].dev : nullptr; }

// ---------------------------------------------------------------- inference: reads params / wt, changes neither
int lg_tube_predict(lg_tube *p, const float *x, const int32_t *rows, int64_t count, float *out) {
    if (p->mem[0].dev.horizon) { lg_set_error("lg_tube_predict: a horizon handle predicts windows (lg_tube_predict_windows)"); return -1; }
    if (count < 1) { lg_set_error("lg_tube_predict: count must be positive"); return -1; }
    if (!x || !out) { lg_set_error("lg_tube_predict: missing array"); return -1; }
    tubek_predict(&p->mem[0].dev, x, nullptr, nullptr, rows, nullptr, nullptr, 0, 0, 0, count, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict: launch failed"), -3);
}

int lg_tube_predict_levels(lg_tube *p, const float *x, const int32_t *rows, int64_t count, const float *levels, int32_t n_levels,
                           float *out) {
    if (!p->mem[0].dev.level_input) { lg_set_error("lg_tube_predict_levels: the handle is not level-conditioned (lg_tube_cfg.level_input)"); return -1; }
    if (count < 1) { lg_set_error("lg_tube_predict_levels: count must be positive"); return -1; }
    if (n_levels < 1 || n_levels > LG_TUBE_MAX_LEVELS) { lg_set_error("lg_tube_predict_levels: n_levels must be 1..64"); return -1; }
    if (!x || !levels || !out) { lg_set_error("lg_tube_predict_levels: missing array"); return -1; }
    tubek_predict_levels(&p->mem[0].dev, x, rows, count, levels, n_levels, out, p->stream);
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
    const TubeDev &D = p->mem[0].dev;
    if (!D.horizon) { lg_set_error("lg_tube_predict_windows: a flat handle predicts rows (lg_tube_predict)"); return -1; }
    if (D.level_input) {
        lg_set_error("lg_tube_predict_windows: the handle is level-conditioned (lg_tube_cfg.level_input): a window has no level, use "
                     "lg_tube_predict_windows_levels");
        return -1;
    }
    if (const char *e = windows_reason(D, w, z, v, n, T, nz, m, env, start, count, out)) {
        lg_set_error(std::string("lg_tube_predict_windows: ") + e); return -1;
    }
    tubek_predict(&p->mem[0].dev, w, z, v, nullptr, env, start, T, nz, m, count, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict_windows: launch failed"), -3);
}

int lg_tube_predict_windows_levels(lg_tube *p, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz,
                                   int32_t m, const int32_t *env, const int32_t *start, int64_t count, const float *levels,
                                   int32_t n_levels, float *out) {
    const TubeDev &D = p->mem[0].dev;
    const char *e = nullptr;
    if (!D.level_input) e = "the handle is not level-conditioned (lg_tube_cfg.level_input)";
    else if (!D.horizon) e = "not a horizon handle (lg_tube_cfg.horizon): a flat handle predicts rows (lg_tube_predict_levels)";
    else if (n_levels < 1 || n_levels > LG_TUBE_MAX_LEVELS) e = "n_levels must be 1..64";
    else if (!levels) e = "missing array";
    else e = windows_reason(D, w, z, v, n, T, nz, m, env, start, count, out);
    if (e) { lg_set_error(std::string("lg_tube_predict_windows_levels: ") + e); return -1; }
    tubek_predict_windows_levels(&p->mem[0].dev, w, z, v, env, start, T, nz, m, count, levels, n_levels, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict_windows_levels: launch failed"), -3);
}

int lg_tube_rollout(lg_tube *p, const float *x, int64_t n_seq, int32_t T, int32_t fb, const uint8_t *reseed, float *out) {
    const TubeDev &D = p->mem[0].dev;
    if (D.horizon) { lg_set_error("lg_tube_rollout: a horizon handle has no closed loop (lg_tube_predict_windows)"); return -1; }
    if (n_seq < 1 || T < 1) { lg_set_error("lg_tube_rollout: n_seq and T must be positive"); return -1; }
    if (n_seq > INT32_MAX / 16) { lg_set_error("lg_tube_rollout: n_seq must be below 2^27"); return -1; }
    if (fb < 0 || fb > D.in_dim || fb > D.out_dim) { lg_set_error("lg_tube_rollout: fb must be 0..min(input_dim, output_dim)"); return -1; }
    if (!x || !out) { lg_set_error("lg_tube_rollout: missing array"); return -1; }
    tubek_rollout(&p->mem[0].dev, x, n_seq, T, fb, reseed, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_rollout: launch failed"), -3);
}

int lg_tube_rollout_window(lg_tube *p, const float *x, int64_t n_seq, int32_t T, int32_t fb, int32_t taps, int32_t dN, int32_t stride,
                           const uint8_t *reseed, float *out) {
    const TubeDev &D = p->mem[0].dev;
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
    tubek_rollout_window(&p->mem[0].dev, x, n_seq, T, fb, taps, dN, taps > 1 ? stride : D.in_dim, reseed, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_rollout_window: launch failed"), -3);
}

// ---------------------------------------------------------------- sweep: the same trainer with K members
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
    return trainer_create(SWEEP, cfgs, K, out);
}
int lg_tube_sweep_destroy(lg_tube_sweep *s) { return trainer_destroy(s); }
int lg_tube_sweep_set_stream(lg_tube_sweep *s, void *stream) { s->stream = (hipStream_t)stream; return 0; }
int lg_tube_sweep_get_buffers(lg_tube_sweep *s, int32_t k, lg_tube_buffers *out) { return trainer_get_buffers(*s, SWEEP, k, out); }
int lg_tube_sweep_param_layout(lg_tube_sweep *s, int64_t *offsets, int64_t *shapes, int max_entries) {
    return fill_layout(s->mem[0].dev, offsets, shapes, max_entries, "lg_tube_sweep_param_layout");
}
int lg_tube_sweep_params_changed(lg_tube_sweep *s, int32_t k) { return trainer_params_changed(*s, SWEEP, k); }
int lg_tube_sweep_set_step(lg_tube_sweep *s, int64_t t) { return trainer_set_step(*s, SWEEP, t); }
int lg_tube_sweep_set_data(lg_tube_sweep *s, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T,
                           int32_t nz, int32_t m) {
    return trainer_set_data(*s, SWEEP, which, x, y, v, rows, T, nz, m);
}
int lg_tube_sweep_begin_epoch(lg_tube_sweep *s, int64_t epoch) { return trainer_begin_epoch(*s, SWEEP, epoch); }
int lg_tube_sweep_step(lg_tube_sweep *s, const int32_t *rows, int64_t count) { return trainer_step(*s, SWEEP, rows, count); }
int lg_tube_sweep_eval(lg_tube_sweep *s) { return trainer_eval(*s, SWEEP, "eval", -1.f); }
int lg_tube_sweep_eval_level(lg_tube_sweep *s, float level) { return trainer_eval_level(*s, SWEEP, level); }

}  // extern "C"
