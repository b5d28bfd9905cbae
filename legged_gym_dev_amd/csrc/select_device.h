// What lg_select_kth and lg_select_kth_grouped hand to the kernels of select_kernels.hip and select_grouped_kernels.hip, and the
// order-preserving key both count on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SEL_THREADS 256
#define SEL_CHUNK 4096              // elements per step of a workgroup's walk: four 16-byte loads per thread
#define SEL_MAX_R 8
#define SEL_COPIES 16               // copies of pass one's LDS histogram, one per lane % 16
#define SEL_GRID 2048               // workgroups a pass aims at: eight per CU
#define SEL_ROW_MAX 256             // and at most this many per batch row: each adds its bins to the row's global bins
#define SELG_BINS 32                // grouped: 256-bin LDS histograms of a workgroup, 32 KiB: four workgroups per CU

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

struct SelectGP {
    const float *values;
    const int32_t *group;           // (n) shared by the rows; outside 0..G-1: the element takes no part
    float *out;                     // (B, G, R)
    int64_t *counts;                // (G)
    int64_t *ranks;                 // (G, R)
    uint32_t *hist;                 // (B, G, R, 256) bins; zero between the passes; pass one uses the bins of rank 0 for every rank
    uint32_t *prefix;               // (B, G, R)
    uint32_t *rem;                  // (B, G, R); 0: the rank is above the group's count
    uint32_t *ctr;                  // (B, tiles) workgroups of the (row, tile) that have finished the pass
    int64_t num[SEL_MAX_R], den[SEL_MAX_R];      // the coverages, by value: the rank is computed on the device
    int64_t ld, n, nchunks;
    int32_t B, G, R, gt;            // gt: groups of a tile, lg_select_group_tile(R)
};

extern "C" {
void selectk_run(const SelectP *P, hipStream_t st);      // the four passes
void selectg_run(const SelectGP *P, hipStream_t st);     // the four passes of the grouped selection
}

// The key.  u = the float's bits; every NaN -> 0xffffffff (above +inf, whose key is 0xff800000; no other float maps there);
// -0.0 -> +0.0; then u ^ 0x80000000 for u >= 0 and ~u for u < 0.  The way back gives +0.0 for the zero and the canonical quiet NaN.
__device__ __forceinline__ uint32_t sel_key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

__device__ __forceinline__ float sel_value(uint32_t key) {
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
