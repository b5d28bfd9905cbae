// What lg_select_kth hands to the kernels of select_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SEL_THREADS 256
#define SEL_CHUNK 4096              // elements per step of a workgroup's walk: four 16-byte loads per thread
#define SEL_MAX_R 8
#define SEL_COPIES 16               // copies of pass one's LDS histogram, one per lane % 16
#define SEL_GRID 2048               // workgroups a pass aims at: eight per CU
#define SEL_ROW_MAX 256             // and at most this many per batch row: each adds its bins to the row's global bins

struct SelectP {
    const float *values;
    const uint8_t *keep;            // NULL: every element takes part
    const int64_t *ranks;
    float *out;
    int64_t *n_kept;
    uint32_t *hist;                 // (B, R, 256) bins; zero between the passes
    uint32_t *prefix;               // (B, R) the digits fixed so far, in place
    uint32_t *rem;                  // (B, R) the rank left inside the prefix; 0: the rank is outside 1..n_kept
    uint32_t *ctr;                  // (B) workgroups of the row that have finished the pass
    int64_t ld, n, nchunks;         // nchunks: SEL_CHUNK pieces of a row, counted from the 16-byte boundary below its start
    int32_t B, R;
};

extern "C" {
void selectk_run(const SelectP *P, hipStream_t st);      // the four passes
}
