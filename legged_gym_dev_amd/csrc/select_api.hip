// C-ABI (include/legged_hip.h, lg_select_*) of the batched k-th selection and its grouped form: the envelope checks and the
// workspace sizes are host code, callable without a GPU; lg_select_kth and lg_select_kth_grouped queue one clear of the workspace
// and the four passes of select_kernels.hip / select_grouped_kernels.hip on the given stream and wait for nothing.
#include <string>

#include "../../include/legged_hip.h"
#include "select_device.h"

void lg_set_error(const std::string &s);

static bool select_envelope(int32_t B, int32_t R) {
    std::string e;
    if (B < 1 || B > 4096) e = "B must be 1..4096";
    else if (R < 1 || R > SEL_MAX_R) e = "R must be 1.." + std::to_string(SEL_MAX_R);
    if (!e.empty()) { lg_set_error("lg_select: " + e); return false; }
    return true;
}

static int32_t group_tile(int32_t R) { return SELG_BINS / R; }      // R <= SEL_MAX_R <= SELG_BINS: at least one group

static bool grouped_envelope(int32_t B, int32_t G, int32_t R) {
    std::string e;
    if (B < 1 || B > 4096) e = "B must be 1..4096";
    else if (G < 1 || G > LG_SELECT_MAX_GROUPS) e = "G must be 1.." + std::to_string(LG_SELECT_MAX_GROUPS);
    else if (R < 1 || R > SEL_MAX_R) e = "R must be 1.." + std::to_string(SEL_MAX_R);
    else if ((int64_t)B * G * R > 65536) e = "B G R must be at most 65536";
    if (!e.empty()) { lg_set_error("lg_select_grouped: " + e); return false; }
    return true;
}

extern "C" {

int64_t lg_select_workspace(int32_t B, int32_t R) {
    if (!select_envelope(B, R)) return -1;
    const int64_t words = (int64_t)B * R * 256 + 2 * (int64_t)B * R + B;     // bins, prefix, rank left, counter
    return (words * 4 + 7) / 8 * 8;
}

int lg_select_kth(const float *values, int64_t ld, int32_t B, int64_t n, const uint8_t *keep, const int64_t *ranks, int32_t R,
                  float *out, int64_t *n_kept, void *workspace, void *stream) {
    if (!select_envelope(B, R)) return -1;
    std::string e;
    if (n < 1 || n > INT32_MAX) e = "n must be 1..2^31-1";
    else if (ld < n) e = "ld must be at least n";
    else if (!values || !ranks || !out || !n_kept || !workspace) e = "missing array";
    else if ((uintptr_t)values & 3) e = "values must be 4-byte aligned";
    else if ((uintptr_t)workspace & 7) e = "the workspace must be 8-byte aligned";
    if (!e.empty()) { lg_set_error("lg_select_kth: " + e); return -1; }
    SelectP P;
    P.values = values; P.keep = keep; P.ranks = ranks; P.out = out; P.n_kept = n_kept;
    P.hist = (uint32_t *)workspace;
    P.prefix = P.hist + (size_t)B * R * 256;
    P.rem = P.prefix + (size_t)B * R;
    P.ctr = P.rem + (size_t)B * R;
    P.ld = ld; P.n = n; P.nchunks = 0; P.B = B; P.R = R;
    // whatever an earlier call with another (B, R) left here: the passes need zero bins and counters
    if (hipMemsetAsync(workspace, 0, (size_t)lg_select_workspace(B, R), (hipStream_t)stream) != hipSuccess) {
        lg_set_error("lg_select_kth: clearing the workspace failed");
        return -3;
    }
    selectk_run(&P, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_select_kth: launch failed"), -3);
}

int32_t lg_select_chunk(void) { return SEL_CHUNK; }

int32_t lg_select_group_tile(int32_t R) {
    if (R < 1 || R > SEL_MAX_R) { lg_set_error("lg_select_grouped: R must be 1.." + std::to_string(SEL_MAX_R)); return -1; }
    return group_tile(R);
}

int64_t lg_select_grouped_workspace(int32_t B, int32_t G, int32_t R) {
    if (!grouped_envelope(B, G, R)) return -1;
    const int64_t sets = (int64_t)B * G * R, gt = group_tile(R), tiles = (G + gt - 1) / gt;
    const int64_t words = sets * 256 + 2 * sets + B * tiles;                 // bins, prefix, rank left, counters
    return (words * 4 + 7) / 8 * 8;
}

int lg_select_kth_grouped(const float *values, int64_t ld, int32_t B, int64_t n, const int32_t *group, int32_t G,
                          const int64_t *cov_num, const int64_t *cov_den, int32_t R, float *out, int64_t *counts, int64_t *ranks,
                          void *workspace, void *stream) {
    if (!grouped_envelope(B, G, R)) return -1;
    std::string e;
    if (n < 1 || n > INT32_MAX) e = "n must be 1..2^31-1";
    else if (ld < n) e = "ld must be at least n";
    else if (!values || !group || !cov_num || !cov_den || !out || !counts || !ranks || !workspace) e = "missing array";
    else if ((uintptr_t)values & 3) e = "values must be 4-byte aligned";
    else if ((uintptr_t)group & 3) e = "group must be 4-byte aligned";
    else if ((uintptr_t)workspace & 7) e = "the workspace must be 8-byte aligned";
    SelectGP P;
    for (int r = 0; r < SEL_MAX_R && e.empty(); ++r) {
        P.num[r] = r < R ? cov_num[r] : 1;
        P.den[r] = r < R ? cov_den[r] : 2;
        if (P.den[r] > INT32_MAX) e = "cov_den[" + std::to_string(r) + "] must be at most 2^31-1";
        else if (P.num[r] < 1) e = "cov_num[" + std::to_string(r) + "] must be at least 1";
        else if (P.num[r] >= P.den[r]) e = "cov_num[" + std::to_string(r) + "] must be below cov_den: a coverage lies inside (0, 1)";
    }
    if (!e.empty()) { lg_set_error("lg_select_kth_grouped: " + e); return -1; }
    const size_t sets = (size_t)B * G * R;
    P.values = values; P.group = group; P.out = out; P.counts = counts; P.ranks = ranks;
    P.hist = (uint32_t *)workspace;
    P.prefix = P.hist + sets * 256;
    P.rem = P.prefix + sets;
    P.ctr = P.rem + sets;
    P.ld = ld; P.n = n; P.nchunks = 0; P.B = B; P.G = G; P.R = R; P.gt = group_tile(R);
    // whatever an earlier call with another (B, G, R) left here: the passes need zero bins and counters
    if (hipMemsetAsync(workspace, 0, (size_t)lg_select_grouped_workspace(B, G, R), (hipStream_t)stream) != hipSuccess) {
        lg_set_error("lg_select_kth_grouped: clearing the workspace failed");
        return -3;
    }
    selectg_run(&P, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : (lg_set_error("lg_select_kth_grouped: launch failed"), -3);
}

}  // extern "C"
