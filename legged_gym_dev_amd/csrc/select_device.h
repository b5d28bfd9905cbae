// What lg_select_kth and lg_select_kth_grouped hand to the two kernels of select_kernels.hip, and what both kernels share: the
// order-preserving key, the walk over a row, the scan of 256 bins, the ticket that finds the last workgroup and the update that
// fixes a digit (DESIGN.md sections 10.6 and 10.7).
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
// -0.0 -> +0.0; then u ^ 0x80000000 for u >= 0 and ~u for u < 0.  Unsigned order of the keys is IEEE order of the floats with the
// NaNs on top, which is where torch.sort leaves them.  The way back gives +0.0 for the zero and the canonical quiet NaN.
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

// Elements between the 16-byte boundary at or below p and p.
__device__ __forceinline__ int64_t sel_mis(const void *p) { return (int64_t)(((uintptr_t)p >> 2) & 3u); }

// What sel_walk_row reads beside the values.  quad(i): the data of elements i .. i + 3 in one load where the address allows;
// elem(q, e): element e of a quad; one(i): the datum of element i alone; part(d): false where the datum alone drops the element.
struct SelKeep {                    // lg_select_kth's keep bytes: the datum is non-zero where the element takes part
    const uint8_t *keep;            // NULL: every element does
    typedef uint32_t Quad;          // four bytes, element e in bits 8 e .. 8 e + 7
    __device__ __forceinline__ Quad quad(int64_t i) const {
        if (!keep) return 0x01010101u;
        const uint8_t *kp = keep + i;
        if (((uintptr_t)kp & 3u) == 0) return *reinterpret_cast<const uint32_t *>(kp);
        return (uint32_t)kp[0] | ((uint32_t)kp[1] << 8) | ((uint32_t)kp[2] << 16) | ((uint32_t)kp[3] << 24);
    }
    static __device__ __forceinline__ uint32_t elem(Quad q, int e) { return q & (0xffu << (8 * e)); }
    __device__ __forceinline__ uint32_t one(int64_t i) const { return keep ? keep[i] : 1u; }
    static __device__ __forceinline__ bool part(uint32_t d) { return d != 0u; }
};

struct SelGroup {                   // lg_select_kth_grouped's group ids
    const int32_t *group;
    bool aligned;                   // sel_mis(group) == sel_mis(row): group + i is 16-byte aligned wherever row + i is
    typedef int4 Quad;
    __device__ __forceinline__ Quad quad(int64_t i) const {
        const int32_t *gp = group + i;
        return aligned ? *reinterpret_cast<const int4 *>(gp) : make_int4(gp[0], gp[1], gp[2], gp[3]);
    }
    static __device__ __forceinline__ int32_t elem(Quad q, int e) { return e == 0 ? q.x : e == 1 ? q.y : e == 2 ? q.z : q.w; }
    __device__ __forceinline__ int32_t one(int64_t i) const { return group[i]; }
    static __device__ __forceinline__ bool part(int32_t) { return true; }       // the kernel tests the id against its tile
};

// The walk.  A 256-thread workgroup walks chunks of SEL_CHUNK consecutive elements of one row of n, chunk blockIdx.x,
// blockIdx.x + gridDim.x, ...; chunks are counted from the 16-byte boundary at or below the row's first element, so that every
// interior load is one aligned 16-byte load whatever the row's address is; the groups of four that straddle the row's two ends
// are read element by element.  take(value, side datum) is called once per element of the row that Side::part does not drop.
// All loads of a chunk, values and side data, are issued before the first take: eight 16-byte loads in flight per lane.
template <class Side, class Take>
__device__ __forceinline__ void sel_walk_row(const float *__restrict__ row, int64_t n, int64_t nchunks, const Side &side, Take &&take) {
    const int64_t mis = sel_mis(row), end = mis + n;
    constexpr int ITEMS = SEL_CHUNK / (SEL_THREADS * 4);
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t j0 = c * SEL_CHUNK + threadIdx.x * 4;
        float4 v[ITEMS];
        typename Side::Quad s[ITEMS];
        bool full[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int64_t j = j0 + (int64_t)k * SEL_THREADS * 4;
            full[k] = j >= mis && j + 4 <= end;
            if (full[k]) {
                v[k] = *reinterpret_cast<const float4 *>(row + (j - mis));
                s[k] = side.quad(j - mis);
            }
        }
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (full[k]) {
                if (Side::part(Side::elem(s[k], 0))) take(v[k].x, Side::elem(s[k], 0));
                if (Side::part(Side::elem(s[k], 1))) take(v[k].y, Side::elem(s[k], 1));
                if (Side::part(Side::elem(s[k], 2))) take(v[k].z, Side::elem(s[k], 2));
                if (Side::part(Side::elem(s[k], 3))) take(v[k].w, Side::elem(s[k], 3));
            } else {
                const int64_t j = j0 + (int64_t)k * SEL_THREADS * 4;
                for (int e = 0; e < 4; ++e) {
                    const int64_t i = j + e - mis;
                    if (i < 0 || i >= n) continue;
                    const auto d = side.one(i);
                    if (Side::part(d)) take(row[i], d);              // the value is not loaded for a datum that drops it
                }
            }
        }
    }
}

// The ticket (the pattern of tube_adam_block.inl).  Every workgroup of a row (or of a (row, tile)) calls this after it has added
// its bins to the global ones; true in the workgroup that draws the last ticket, which then sees what all the others added
// (through agent-scope atomic loads).  last: one bool of LDS.
__device__ __forceinline__ bool sel_last_workgroup(uint32_t *ctr, bool *last) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) *last = atomicAdd(ctr, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!*last) return false;
    __threadfence();
    return true;
}

// The scan of 256 bins, thread d holding the count c of bin d: the counts below bin d (excl), up to and including it (incl) and
// of all bins (total).  An inclusive scan over the wave, then the four wave totals through wsum (SEL_THREADS / 64 words of LDS).
// Every thread of the workgroup calls it, and wsum is rewritten by the next call: a __syncthreads() lies between two calls.
__device__ __forceinline__ void sel_scan_bins(uint32_t c, uint32_t *wsum, uint32_t &excl, uint32_t &incl, uint32_t &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
        if (w < wv) base += wsum[w];
        total += wsum[w];
    }
    incl = base + x;
    excl = incl - c;
}

// After a scan: the bins partition the counted elements, so for a rank want inside 1..total exactly one thread owns the bin that
// holds it.  That thread puts its bin into the prefix as this pass's digit (the top one when FIRST), takes the count below the bin
// off the rank, and after the last digit writes the value of the key.  want 0: the rank is outside, nobody writes.
template <bool FIRST>
__device__ __forceinline__ void sel_fix_digit(uint32_t want, uint32_t excl, uint32_t incl, int shift, uint32_t *pre, uint32_t *rem, float *out) {
    if (want == 0u || excl >= want || want > incl) return;
    const uint32_t p = FIRST ? (uint32_t)threadIdx.x << 24 : *pre | ((uint32_t)threadIdx.x << shift);
    *pre = p;
    *rem = want - excl;
    if (!FIRST && shift == 0) *out = sel_value(p);
}
