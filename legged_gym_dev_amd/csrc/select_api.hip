// C-ABI (include/legged_hip.h, lg_select_*) of the batched k-th selection and its grouped form: the envelope checks and the
// workspace sizes are host code, callable without a GPU; lg_select_kth and lg_select_kth_grouped queue one clear of the workspace
// and the four passes of select_kernels.hip on the given stream and wait for nothing.
#include <string>

#include "lg_internal.h"
#include "select_device.h"

static bool refuse(const char *who, const std::string &e) {
    if (!e.empty()) lg_set_error(std::string(who) + ": " + e);
    return !e.empty();
}

static bool select_envelope(int32_t B, int32_t R) {
    std::string e;
    if (B < 1 || B > 4096) e = "B must be 1..4096";
    else if (R < 1 || R > SEL_MAX_R) e = "R must be 1.." + std::to_string(SEL_MAX_R);
    return !refuse("lg_select", e);
}

static int32_t group_tile(int32_t R) { return SELG_BINS / R; }      // R <= SEL_MAX_R <= SELG_BINS: at least one group

static bool grouped_envelope(int32_t B, int32_t G, int32_t R) {
    std::string e;
    if (B < 1 || B > 4096) e = "B must be 1..4096";
    else if (G < 1 || G > LG_SELECT_MAX_GROUPS) e = "G must be 1.." + std::to_string(LG_SELECT_MAX_GROUPS);
    else if (R < 1 || R > SEL_MAX_R) e = "R must be 1.." + std::to_string(SEL_MAX_R);
    else if ((int64_t)B * G * R > 65536) e = "B G R must be at most 65536";
    return !refuse("lg_select_grouped", e);
}

// What both entries ask of the rows and the workspace; group NULL: the entry has none.  missing: one of the entry's arrays is NULL.
static bool rows_ok(const char *who, int64_t n, int64_t ld, bool missing, const float *values, const int32_t *group, const void *workspace) {
    std::string e;
    if (n < 1 || n > INT32_MAX) e = "n must be 1..2^31-1";
    else if (ld < n) e = "ld must be at least n";
    else if (missing) e = "missing array";
    else if ((uintptr_t)values & 3) e = "values must be 4-byte aligned";
    else if ((uintptr_t)group & 3) e = "group must be 4-byte aligned";
    else if ((uintptr_t)workspace & 7) e = "the workspace must be 8-byte aligned";
    return !refuse(who, e);
}

// The workspace of `sets` selection states and `counters` counters: bins, prefix, rank left, counters.  Returns its bytes; with P
// it also points P's four arrays into the workspace.
template <class Params>
static int64_t lay_out(int64_t sets, int64_t counters, void *workspace = nullptr, Params *P = nullptr) {
    const int64_t prefix = sets * 256, rem = prefix + sets, ctr = rem + sets, words = ctr + counters;
    if (P) {
        P->hist = (uint32_t *)workspace;
        P->prefix = P->hist + prefix;
        P->rem = P->hist + rem;
        P->ctr = P->hist + ctr;
    }
    return (words * 4 + 7) / 8 * 8;
}

static int64_t tiles_of(int32_t G, int32_t R) { return (G + group_tile(R) - 1) / group_tile(R); }

// Clear the workspace -- whatever an earlier call with another shape left here: the passes need zero bins and counters -- and
// queue the four passes.
template <class Params>
static int run(const char *who, void (*passes)(const Params *, hipStream_t), const Params &P, void *workspace, int64_t bytes, void *stream) {
    if (hipMemsetAsync(workspace, 0, (size_t)bytes, (hipStream_t)stream) != hipSuccess) {
        lg_set_error(std::string(who) + ": clearing the workspace failed");
        return -3;
    }
    passes(&P, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error(std::string(who) + ": launch failed"), -3);
}

extern "C" {

int64_t lg_select_workspace(int32_t B, int32_t R) {
    return select_envelope(B, R) ? lay_out<SelectP>((int64_t)B * R, B) : -1;
}

int lg_select_kth(const float *values, int64_t ld, int32_t B, int64_t n, const uint8_t *keep, const int64_t *ranks, int32_t R,
                  float *out, int64_t *n_kept, void *workspace, void *stream) {
    const char *who = "lg_select_kth";
    if (!select_envelope(B, R) || !rows_ok(who, n, ld, !values || !ranks || !out || !n_kept || !workspace, values, nullptr, workspace))
        return -1;
    SelectP P;
    P.values = values; P.keep = keep; P.ranks = ranks; P.out = out; P.n_kept = n_kept;
    P.ld = ld; P.n = n; P.nchunks = 0; P.B = B; P.R = R;
    return run(who, selectk_run, P, workspace, lay_out((int64_t)B * R, B, workspace, &P), stream);
}

int32_t lg_select_chunk(void) { return SEL_CHUNK; }

int32_t lg_select_group_tile(int32_t R) {
    if (R < 1 || R > SEL_MAX_R) { lg_set_error("lg_select_grouped: R must be 1.." + std::to_string(SEL_MAX_R)); return -1; }
    return group_tile(R);
}

int64_t lg_select_grouped_workspace(int32_t B, int32_t G, int32_t R) {
    return grouped_envelope(B, G, R) ? lay_out<SelectGP>((int64_t)B * G * R, B * tiles_of(G, R)) : -1;
}

int lg_select_kth_grouped(const float *values, int64_t ld, int32_t B, int64_t n, const int32_t *group, int32_t G,
                          const int64_t *cov_num, const int64_t *cov_den, int32_t R, float *out, int64_t *counts, int64_t *ranks,
                          void *workspace, void *stream) {
    const char *who = "lg_select_kth_grouped";
    if (!grouped_envelope(B, G, R) || !rows_ok(who, n, ld, !values || !group || !cov_num || !cov_den || !out || !counts || !ranks || !workspace,
                                               values, group, workspace))
        return -1;
    SelectGP P;
    std::string e;
    for (int r = 0; r < SEL_MAX_R && e.empty(); ++r) {
        P.num[r] = r < R ? cov_num[r] : 1;
        P.den[r] = r < R ? cov_den[r] : 2;
        if (P.den[r] > INT32_MAX) e = "cov_den[" + std::to_string(r) + "] must be at most 2^31-1";
        else if (P.num[r] < 1) e = "cov_num[" + std::to_string(r) + "] must be at least 1";
        else if (P.num[r] >= P.den[r]) e = "cov_num[" + std::to_string(r) + "] must be below cov_den: a coverage lies inside (0, 1)";
    }
    if (refuse(who, e)) return -1;
    P.values = values; P.group = group; P.out = out; P.counts = counts; P.ranks = ranks;
    P.ld = ld; P.n = n; P.nchunks = 0; P.B = B; P.G = G; P.R = R; P.gt = group_tile(R);
    return run(who, selectg_run, P, workspace, lay_out((int64_t)B * G * R, B * tiles_of(G, R), workspace, &P), stream);
}

}  // extern "C"
