// C-ABI (include/legged_hip.h, lg_select_*) of the batched k-th selection: the envelope check and the workspace size are host code,
// callable without a GPU; lg_select_kth queues one clear of the workspace and the four passes of select_kernels.hip on the given
// stream and waits for nothing.
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

}  // extern "C"
