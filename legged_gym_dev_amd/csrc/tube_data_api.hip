// C-ABI (include/legged_hip.h, lg_tube_rows_* and lg_tube_horizon_build) of the device dataset builder: the envelope check and the
// widths are host code, callable without a GPU; the builds queue the launches of tube_data_kernels.hip on the given stream and
// wait for nothing.
#include <string>

#include "lg_internal.h"
#include "tube_data_device.h"

static const int64_t TD_MAX_T = (int64_t)1 << 24;

static int64_t rows_input_dim(const lg_tube_rows_spec *s) {
    if (s->kind == LG_TUBE_ROWS_SCALAR)
        return s->recursive ? (int64_t)s->N * (1 + (s->n - 2) + s->m) : 1 + (int64_t)s->N * ((s->n - 2) + s->m);
    return (int64_t)s->N * (2 * s->n + s->m);
}

static int64_t rows_chunks(const lg_tube_rows_spec *s) { return (int64_t)s->n_env * ((s->T + TD_CHUNK - 1) / TD_CHUNK); }

extern "C" {

int lg_tube_rows_check(const lg_tube_rows_spec *s) {
    std::string e;
    if (s->kind < LG_TUBE_ROWS_SCALAR || s->kind > LG_TUBE_ROWS_ERROR) e = "kind must be 0 (scalar), 1 (vector) or 2 (error dynamics)";
    else if (s->n < 2 || s->n > 6) e = "n (the width of z) must be 2..6";
    else if (s->m < 1 || s->m > 4) e = "m (the width of v) must be 1..4";
    else if (s->N < 1 || s->N > LG_TUBE_MAX_IN) e = "N must be 1.." + std::to_string(LG_TUBE_MAX_IN);
    else if (s->dN < 1 || s->dN > TD_MAX_T) e = "dN must be 1..2^24";
    else if (s->recursive != 0 && s->recursive != 1) e = "recursive must be 0 or 1";
    else if (s->recursive && s->kind != LG_TUBE_ROWS_SCALAR) e = "recursive is a flag of the scalar kind";
    else if (s->T < 1 || s->T > TD_MAX_T) e = "T must be 1..2^24";
    else if (s->n_env < 1) e = "n_env must be positive";
    else if (rows_chunks(s) * TD_CHUNK > INT32_MAX) e = "n_env x T (rounded up to whole 64-step chunks) must stay below 2^31";
    else if (s->compact != 0 && s->compact != 1) e = "compact must be 0 or 1";
    else if (s->mark_last_env != 0 && s->mark_last_env != 1) e = "mark_last_env must be 0 or 1";
    else if (s->epoch_envs < 1 || s->n_env % s->epoch_envs != 0) e = "epoch_envs must be positive and divide n_env";
    else if (rows_input_dim(s) > LG_TUBE_MAX_IN)
        e = "input_dim = " + std::to_string(rows_input_dim(s)) + " exceeds " + std::to_string(LG_TUBE_MAX_IN) + " (the model envelope)";
    if (!e.empty()) { lg_set_error("lg_tube_rows: " + e); return -1; }
    return 0;
}

int lg_tube_rows_dims(const lg_tube_rows_spec *s, int32_t *input_dim, int32_t *output_dim) {
    if (lg_tube_rows_check(s)) return -1;
    if (input_dim) *input_dim = (int32_t)rows_input_dim(s);
    if (output_dim) *output_dim = s->kind == LG_TUBE_ROWS_SCALAR ? 1 : s->n;
    return 0;
}

int64_t lg_tube_rows_workspace(const lg_tube_rows_spec *s) {
    if (lg_tube_rows_check(s)) return -1;
    return s->compact ? rows_chunks(s) * 12 : 0;      // offs int64[chunks], then counts int32[chunks]
}

int lg_tube_rows_build(const lg_tube_rows_spec *s, const float *z, const float *pz_x, const float *v, const uint8_t *done,
                       float *data, float *target, int64_t *n_rows, void *workspace, void *stream) {
    if (lg_tube_rows_check(s)) return -1;
    if (!z || !pz_x || !v || !data || !target || !n_rows) { lg_set_error("lg_tube_rows_build: missing array"); return -1; }
    if (s->compact && (!done || !workspace)) { lg_set_error("lg_tube_rows_build: compact = 1 needs done and the workspace"); return -1; }
    if (s->compact && ((uintptr_t)workspace & 7)) { lg_set_error("lg_tube_rows_build: the workspace must be 8-byte aligned"); return -1; }
    TubeRowsP P;
    P.z = z; P.pz = pz_x; P.v = v; P.done = done; P.data = data; P.target = target; P.n_rows = n_rows; P.offs = nullptr;
    P.nchunks = rows_chunks(s);
    P.n_env = s->n_env; P.T = s->T; P.cpe = (s->T + TD_CHUNK - 1) / TD_CHUNK;
    P.kind = s->kind; P.N = s->N; P.dN = s->dN; P.recursive = s->recursive; P.n = s->n; P.m = s->m;
    P.compact = s->compact; P.mark = s->mark_last_env; P.epoch_envs = s->epoch_envs;
    P.I = (int32_t)rows_input_dim(s);
    const bool scalar = s->kind == LG_TUBE_ROWS_SCALAR;
    P.O = scalar ? 1 : s->n;
    P.L = scalar ? (s->recursive ? 1 : 0) : s->n;
    P.nz = scalar ? s->n - 2 : s->n;
    P.zoff = scalar ? 2 : 0;
    P.bw = P.L + P.nz + s->m;
    int64_t *offs = (int64_t *)workspace;
    int32_t *counts = s->compact ? (int32_t *)(offs + P.nchunks) : nullptr;
    tubedatak_rows(&P, counts, offs, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_rows_build: launch failed"), -3);
}

int lg_tube_horizon_build(const float *z, const float *pz_x, const float *v, int64_t n_env, int32_t T, int32_t n, int32_t m,
                          int32_t H_rev, float *w, float *z_no_pos, float *v_pad, void *stream) {
    std::string e;
    if (n < 2 || n > 6) e = "n (the width of z) must be 2..6";
    else if (m < 1 || m > 4) e = "m (the width of v) must be 1..4";
    else if (T < 1 || T > TD_MAX_T) e = "T must be 1..2^24";
    else if (H_rev < 0 || H_rev > TD_MAX_T) e = "H_rev must be 0..2^24";
    else if (n_env < 1 || n_env > INT32_MAX) e = "n_env must be 1..2^31-1";
    else if (!z || !pz_x || !v || !w || !v_pad || (n > 2 && !z_no_pos)) e = "missing array";
    if (!e.empty()) { lg_set_error("lg_tube_horizon_build: " + e); return -1; }
    tubedatak_horizon(z, pz_x, v, n_env, T, n, m, H_rev, w, z_no_pos, v_pad, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_tube_horizon_build: launch failed"), -3);
}

}  // extern "C"
