// C-ABI (include/legged_hip.h, lg_tube_*) of the tube-model trainer: parameter / optimiser / slab allocation in HBM, epoch
// permutation, the two launches of a training step, the eval launch, and the inference entries: predict, window prediction and
// the closed-loop roll-outs, single-tap and windowed (tube_kernels.hip).
#include <cmath>
#include <cstring>
#include <string>

#include "tube_device.h"
#include "../../include/legged_hip.h"

void lg_set_error(const std::string &s);

extern "C" {
size_t tubek_lds_bytes(const TubeDev *D);
int tubek_init();
void tubek_step(const TubeDev *D, const TubeSplit *S, const int32_t *rows, int64_t count, uint64_t key, float norm, hipStream_t s);
void tubek_adam(const TubeDev *D, int nwg, int64_t t, double lr0, double gamma, int64_t step_size, float norm, int64_t rows,
                hipStream_t s);
void tubek_eval(const TubeDev *D, const TubeSplit *S, const int32_t *rows, uint64_t key, float norm, hipStream_t s);
void tubek_wt(const TubeDev *D, hipStream_t s);
void tubek_perm(const TubeDev *D, int n, uint64_t epoch, hipStream_t s);
void tubek_iota(int32_t *p, int64_t n, hipStream_t s);
void tubek_predict(const TubeDev *D, const float *x, const float *y, const float *v, const int32_t *rows, const int32_t *env,
                   const int32_t *start, int T, int nz, int m, int64_t count, float *o, hipStream_t s);
void tubek_rollout(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, const uint8_t *reseed, float *o, hipStream_t s);
void tubek_rollout_window(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, int taps, int dN, int stride,
                          const uint8_t *reseed, float *o, hipStream_t s);
}

struct lg_tube {
    lg_tube_cfg cfg;
    TubeDev dev;
    TubeSplit split[2];                 // train, test
    hipStream_t stream = nullptr;
    int64_t t = 0;                      // Adam steps taken
    int64_t pos = 0;                    // rows of the epoch permutation consumed
    int64_t eval_count = 0;
    int64_t starts_cap = 0, eval_rows_cap = 0, perm_cap = 0;
    int32_t *eval_rows = nullptr;
};

static bool talloc(void **q, size_t bytes) {
    *q = nullptr;
    if (bytes == 0) bytes = 4;
    return hipMalloc(q, bytes) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess;
}

static float loss_norm(const lg_tube *p, int64_t rows) {
    return (float)(p->cfg.loss == LG_TUBE_LOSS_VECTOR ? rows : rows * (int64_t)p->cfg.output_dim);
}

extern "C" {

int lg_tube_check_cfg(const lg_tube_cfg *c) {
    std::string e;
    if (c->num_units < 16 || c->num_units > LG_TUBE_MAX_UNITS || c->num_units % 16) e = "num_units must be 16..128 in steps of 16";
    else if (c->num_layers < 1 || c->num_layers > 4) e = "num_layers must be 1..4";
    else if (c->input_dim < 1 || c->input_dim > LG_TUBE_MAX_IN) e = "input_dim must be 1..256";
    else if (c->output_dim < 1 || c->output_dim > LG_TUBE_MAX_OUT) e = "output_dim must be 1..64";
    else if (c->activation < 0 || c->activation > 3) e = "activation must be relu, softplus, tanh or elu";
    else if (c->loss < 0 || c->loss > 2) e = "loss must be scalar (0), vector (1) or mse (2)";
    else if (c->batch_size < 1) e = "batch_size must be positive";
    else if (c->step_size < 1) e = "step_size must be positive";
    else if (c->horizon && (c->H_rev < 0 || c->H_fwd < 1 || c->output_dim != c->H_fwd)) e = "horizon dataset: output_dim must equal H_fwd";
    else if (c->activation == LG_TUBE_ACT_SOFTPLUS && !(c->softplus_beta > 0.f)) e = "softplus_beta must be positive";
    if (!e.empty()) { lg_set_error("lg_tube: " + e); return -1; }
    return 0;
}

int lg_tube_create(const lg_tube_cfg *cfg, lg_tube **out) {
    *out = nullptr;
    if (lg_tube_check_cfg(cfg)) return -1;
    if (tubek_init()) { lg_set_error("lg_tube_create: hipFuncSetAttribute failed"); return -2; }
    lg_tube *p = new lg_tube();
    p->cfg = *cfg;
    TubeDev &D = p->dev;
    memset(&D, 0, sizeof(D));
    D.in_dim = cfg->input_dim; D.out_dim = cfg->output_dim; D.units = cfg->num_units; D.layers = cfg->num_layers;
    D.act = cfg->activation; D.loss = cfg->loss; D.horizon = cfg->horizon; D.H_fwd = cfg->H_fwd; D.H_rev = cfg->H_rev;
    D.alpha = cfg->alpha; D.delta = cfg->delta; D.sp_beta = cfg->activation == LG_TUBE_ACT_SOFTPLUS ? cfg->softplus_beta : 1.f;
    D.seed = cfg->seed;
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
    bool ok = talloc((void **)&D.params, off * 4) && talloc((void **)&D.wt, off * 4) && talloc((void **)&D.grads, off * 4) &&
              talloc((void **)&D.adam_m, off * 4) && talloc((void **)&D.adam_v, off * 4) &&
              talloc((void **)&D.slab, (size_t)nwg * D.slab_ld * 4) && talloc((void **)&D.normpart, 1024 * 4) &&
              talloc((void **)&D.done_ctr, 4) && talloc((void **)&D.log, (size_t)D.log_cap * 16) && talloc((void **)&D.eval, 16);
    if (!ok) { lg_set_error("hipMalloc failed in lg_tube_create"); lg_tube_destroy(p); return -100; }
    *out = p;
    return 0;
}

int lg_tube_destroy(lg_tube *p) {
    if (!p) return 0;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    else (void)hipDeviceSynchronize();
    TubeDev &D = p->dev;
    for (void *q : {(void *)D.params, (void *)D.wt, (void *)D.grads, (void *)D.adam_m, (void *)D.adam_v, (void *)D.slab,
                    (void *)D.evpart, (void *)D.normpart, (void *)D.done_ctr, (void *)D.log, (void *)D.eval, (void *)D.starts,
                    (void *)D.perm, (void *)p->eval_rows})
        if (q) (void)hipFree(q);
    delete p;
    return 0;
}

int lg_tube_set_stream(lg_tube *p, void *stream) { p->stream = (hipStream_t)stream; return 0; }

int lg_tube_get_buffers(lg_tube *p, lg_tube_buffers *out) {
    const TubeDev &D = p->dev;
    out->params = D.params; out->grads = D.grads; out->adam_m = D.adam_m; out->adam_v = D.adam_v;
    out->log = D.log; out->eval = D.eval; out->starts = D.starts; out->perm = D.perm;
    out->num_params = D.num_params; out->log_cap = D.log_cap; out->starts_cap = p->starts_cap; out->perm_cap = p->perm_cap;
    out->step = p->t;
    return 0;
}

int lg_tube_param_layout(lg_tube *p, int64_t *offsets, int64_t *shapes, int max_entries) {
    const TubeDev &D = p->dev;
    const int n = 2 * (D.layers + 1);
    if (max_entries < n) { lg_set_error("lg_tube_param_layout: max_entries too small"); return -1; }
    for (int li = 0; li <= D.layers; ++li) {
        offsets[2 * li] = D.off_w[li]; shapes[4 * li] = D.dout[li]; shapes[4 * li + 1] = D.din[li];
        offsets[2 * li + 1] = D.off_b[li]; shapes[4 * li + 2] = D.dout[li]; shapes[4 * li + 3] = 0;
    }
    return n;
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
    if (which != 0 && which != 1) { lg_set_error("lg_tube_set_data: which must be 0 (train) or 1 (test)"); return -1; }
    if (rows < 1 || rows > INT32_MAX) { lg_set_error("lg_tube_set_data: rows must be 1..2^31-1"); return -1; }
    if (!x || (!D.horizon && !y) || (D.horizon && ((nz && !y) || (m && !v)))) { lg_set_error("lg_tube_set_data: missing array"); return -1; }
    if (D.horizon) {
        if (D.H_rev + nz + (D.H_rev + D.H_fwd) * m != D.in_dim) {
            lg_set_error("lg_tube_set_data: input_dim != H_rev + nz + (H_rev + H_fwd) * m"); return -1;
        }
        if (T - D.H_fwd - 1 <= D.H_rev) { lg_set_error("lg_tube_set_data: T - H_fwd - 1 must exceed H_rev"); return -1; }
        if ((D.T && D.T != T) || (D.nz && D.nz != nz) || (D.m && D.m != m)) {
            lg_set_error("lg_tube_set_data: train and test splits differ in T, nz or m"); return -1;
        }
        D.T = T; D.nz = nz; D.m = m;
    }
    p->split[which] = TubeSplit{x, y, v, rows};
    const int64_t need = rows > p->cfg.batch_size ? rows : p->cfg.batch_size;
    if (need > p->starts_cap) {
        if (D.starts) (void)hipFree(D.starts);
        if (!talloc((void **)&D.starts, need * 4)) { D.starts = nullptr; p->starts_cap = 0; lg_set_error("hipMalloc failed"); return -100; }
        p->starts_cap = need;
    }
    if (which == 0 && rows > p->perm_cap) {
        if (D.perm) (void)hipFree(D.perm);
        if (!talloc((void **)&D.perm, rows * 4)) { D.perm = nullptr; p->perm_cap = 0; lg_set_error("hipMalloc failed"); return -100; }
        p->perm_cap = rows;
    }
    if (which == 1) {
        const int64_t nwg = (rows + LG_TUBE_ROWS - 1) / LG_TUBE_ROWS;
        if (rows > p->eval_rows_cap) {
            if (p->eval_rows) (void)hipFree(p->eval_rows);
            if (D.evpart) (void)hipFree(D.evpart);
            D.evpart = nullptr;
            if (!talloc((void **)&p->eval_rows, rows * 4) || !talloc((void **)&D.evpart, nwg * 16)) {
                p->eval_rows_cap = 0; lg_set_error("hipMalloc failed"); return -100;
            }
            p->eval_rows_cap = rows;
        }
        tubek_iota(p->eval_rows, rows, p->stream);
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
    const float norm = loss_norm(p, count);
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
    tubek_eval(&p->dev, &S, p->eval_rows, key, loss_norm(p, S.rows), p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_eval: launch failed"), -3);
}

// ---------------------------------------------------------------- inference: reads params / wt, changes neither
int lg_tube_predict(lg_tube *p, const float *x, const int32_t *rows, int64_t count, float *out) {
    if (p->dev.horizon) { lg_set_error("lg_tube_predict: a horizon handle predicts windows (lg_tube_predict_windows)"); return -1; }
    if (count < 1) { lg_set_error("lg_tube_predict: count must be positive"); return -1; }
    if (!x || !out) { lg_set_error("lg_tube_predict: missing array"); return -1; }
    tubek_predict(&p->dev, x, nullptr, nullptr, rows, nullptr, nullptr, 0, 0, 0, count, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict: launch failed"), -3);
}

int lg_tube_predict_windows(lg_tube *p, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz, int32_t m,
                            const int32_t *env, const int32_t *start, int64_t count, float *out) {
    const TubeDev &D = p->dev;
    if (!D.horizon) { lg_set_error("lg_tube_predict_windows: a flat handle predicts rows (lg_tube_predict)"); return -1; }
    if (count < 1 || n < 1) { lg_set_error("lg_tube_predict_windows: n and count must be positive"); return -1; }
    if (nz < 0 || m < 0 || D.H_rev + nz + (D.H_rev + D.H_fwd) * m != D.in_dim) {
        lg_set_error("lg_tube_predict_windows: input_dim != H_rev + nz + (H_rev + H_fwd) * m"); return -1;
    }
    if (T < D.H_rev + D.H_fwd) { lg_set_error("lg_tube_predict_windows: T is shorter than H_rev + H_fwd"); return -1; }
    if (!w || (nz && !z) || (m && !v) || !env || !start || !out) { lg_set_error("lg_tube_predict_windows: missing array"); return -1; }
    tubek_predict(&p->dev, w, z, v, nullptr, env, start, T, nz, m, count, out, p->stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_predict_windows: launch failed"), -3);
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

}  // extern "C"
