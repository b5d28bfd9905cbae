// Batched exact k-th smallest, plain (lg_select_kth) and grouped (lg_select_kth_grouped; section 10.7):
// most-significant-digit radix select on the order-preserving uint32 key of the float, 8 bits per pass, four passes, one launch
// each.  A pass of either kernel: a workgroup walks its share of one batch row (sel_walk_row) and counts the digits of the
// elements that take part in 256-bin LDS histograms, adds its non-zero bins to the global bins with integer atomics and draws a
// ticket (sel_last_workgroup); the workgroup that draws the last one scans the bins (sel_scan_bins), fixes the digit that holds
// each rank and takes the count below it off the rank (sel_fix_digit), and clears bins and counter for the next launch.  After the
// fourth pass the prefix is the key and the same workgroup writes out.  Counts are integers: the result does not depend on the
// order in which workgroups arrive, and no float is ever added.  The shared pieces are described in select_device.h.
#include "select_device.h"

// Grid (workgroups per row, B).  Each kept element adds one to the LDS bin of its digit, once per rank whose prefix its higher
// digits equal.  Pass one has no prefix, so one histogram serves every rank; tube scores have one sign and a few binades, so nearly
// every lane of a wave hits the same one or two bins there, and the pass keeps SEL_COPIES copies of its histogram, lane l adding
// to copy l % SEL_COPIES (consecutive words, different banks), and sums them at the end.  The workgroups per row are capped
// (sel_run) because every one of them adds up to 256 R words to the same 256 R addresses, and that many-adders-one-line traffic,
// not the reads, set the time of the first version of this kernel.
template <bool FIRST>
__global__ __launch_bounds__(SEL_THREADS) void k_select_pass(SelectP P, int shift) {
    constexpr int NL = FIRST ? SEL_COPIES * 256 : SEL_MAX_R * 256;
    __shared__ uint32_t lh[NL];
    __shared__ uint32_t wsum[SEL_THREADS / 64];
    __shared__ bool last;
    const int tid = threadIdx.x, b = blockIdx.y, R = P.R, nh = FIRST ? 1 : R;
    uint32_t *__restrict__ gh = P.hist + (size_t)b * R * 256;
    uint32_t *__restrict__ gpre = P.prefix + (size_t)b * R, *__restrict__ grem = P.rem + (size_t)b * R;

    uint32_t pre[SEL_MAX_R];                           // the rank's prefix above this pass's digit; no key has more than 24 bits there
#pragma unroll
    for (int r = 0; r < SEL_MAX_R; ++r) pre[r] = (!FIRST && r < R && grem[r] != 0u) ? gpre[r] >> (shift + 8) : 0xffffffffu;
    for (int i = tid; i < (FIRST ? NL : nh * 256); i += SEL_THREADS) lh[i] = 0u;
    __syncthreads();

    sel_walk_row(P.values + (int64_t)b * P.ld, P.n, P.nchunks, SelKeep{P.keep}, [&](float f, uint32_t) {
        const uint32_t key = sel_key(f);
        if (FIRST) atomicAdd(&lh[(key >> 24) * SEL_COPIES + (tid & (SEL_COPIES - 1))], 1u);
        else {
            const uint32_t hi = key >> (shift + 8), d = (key >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < SEL_MAX_R; ++r)
                if (hi == pre[r]) atomicAdd(&lh[r * 256 + d], 1u);
        }
    });
    __syncthreads();
    if (FIRST) {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < SEL_COPIES; ++k) c += lh[tid * SEL_COPIES + k];
        if (c) atomicAdd(&gh[tid], c);
    } else {
        for (int i = tid; i < nh * 256; i += SEL_THREADS) {
            const uint32_t c = lh[i];
            if (c) atomicAdd(&gh[i], c);
        }
    }
    if (!sel_last_workgroup(P.ctr + b, &last)) return;

    // the row's last workgroup: thread d owns bin d
    for (int r = 0; r < R; ++r) {
        // the rank inside this histogram; 0: outside 1..n_kept.  Read by every thread before the scan's barrier; written after it
        uint32_t want = FIRST ? 0u : grem[r];
        uint32_t excl, incl, total;
        sel_scan_bins(__hip_atomic_load(gh + (FIRST ? 0 : r) * 256 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), wsum, excl, incl, total);
        if (FIRST) {
            const int64_t k = P.ranks[(size_t)b * R + r];
            want = (k >= 1 && k <= (int64_t)total) ? (uint32_t)k : 0u;
            if (tid == 0) {
                if (b == 0 && r == 0) *P.n_kept = (int64_t)total;
                if (want == 0u) { grem[r] = 0u; gpre[r] = 0u; P.out[(size_t)b * R + r] = __uint_as_float(0x7f800000u); }
            }
        }
        sel_fix_digit<FIRST>(want, excl, incl, shift, gpre + r, grem + r, P.out + (size_t)b * R + r);
        __syncthreads();                               // wsum is rewritten by the next rank
    }
    for (int i = tid; i < nh * 256; i += SEL_THREADS) __hip_atomic_store(gh + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) atomicExch(P.ctr + b, 0u);
}

// Grid (workgroups per row, B, tiles): k_select_pass with (group, digit) as the counted key, and each group's conformal rank
// ceil((count + 1) num / den) computed on the device between the first count and the selection.  The workgroup reads the group
// ids beside the values and counts the groups of tile blockIdx.z only, gt = lg_select_group_tile(R) consecutive groups: elements
// of other groups, and ids outside 0..G-1, are read and skipped.  Pass one keeps one 256-bin LDS histogram per group of the tile
// (no prefix exists yet, and it serves every rank); passes two to four one per (group, rank).  SELG_BINS histograms, 32 KiB, is
// what a workgroup has.  Neighbouring elements belong to different groups in the layouts this serves (the age of a step, element
// index mod the horizon), so pass one needs no copies of its histograms.  The ticket is that of the (row, tile).  In pass one the
// last workgroup writes counts and ranks (from row 0; they are the same for every row), and marks a rank above the count as +inf.
template <bool FIRST>
__global__ __launch_bounds__(SEL_THREADS) void k_select_grouped_pass(SelectGP P, int shift) {
    __shared__ uint32_t lh[SELG_BINS * 256];
    __shared__ uint32_t lpre[SELG_BINS];               // the prefix of (group of the tile, rank) above this pass's digit
    __shared__ uint32_t wsum[SEL_THREADS / 64];
    __shared__ bool last;
    const int tid = threadIdx.x, b = blockIdx.y, R = P.R, G = P.G;
    const int g0 = blockIdx.z * P.gt, ng = min(P.gt, G - g0);      // the tile's groups g0 .. g0 + ng - 1; ng R <= SELG_BINS
    const int nh = FIRST ? ng : ng * R;
    const size_t s0 = ((size_t)b * G + g0) * R;                    // (row, first group of the tile, rank 0)
    uint32_t *__restrict__ gh = P.hist + s0 * 256;
    uint32_t *__restrict__ gpre = P.prefix + s0, *__restrict__ grem = P.rem + s0;
    uint32_t *__restrict__ ctr = P.ctr + (size_t)b * gridDim.z + blockIdx.z;

    if (!FIRST && tid < ng * R) lpre[tid] = grem[tid] != 0u ? gpre[tid] >> (shift + 8) : 0xffffffffu;   // no key has more than 24 bits there
    for (int i = tid; i < nh * 256; i += SEL_THREADS) lh[i] = 0u;
    __syncthreads();

    const float *__restrict__ row = P.values + (int64_t)b * P.ld;
    sel_walk_row(row, P.n, P.nchunks, SelGroup{P.group, sel_mis(P.group) == sel_mis(row)}, [&](float f, int32_t gid) {
        const uint32_t gi = (uint32_t)(gid - g0);
        if (gi >= (uint32_t)ng) return;
        const uint32_t key = sel_key(f);
        if (FIRST) atomicAdd(&lh[gi * 256 + (key >> 24)], 1u);
        else {
            const uint32_t hi = key >> (shift + 8), d = (key >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < SEL_MAX_R; ++r)
                if (r < R && hi == lpre[gi * R + r]) atomicAdd(&lh[(gi * R + r) * 256 + d], 1u);
        }
    });
    __syncthreads();
    for (int i = tid; i < nh * 256; i += SEL_THREADS) {
        const uint32_t c = lh[i];                      // pass one: histogram i >> 8 is group g0 + (i >> 8), kept in the bins of its rank 0
        if (c) atomicAdd(&gh[FIRST ? (size_t)(i >> 8) * R * 256 + (i & 255) : (size_t)i], c);
    }
    if (!sel_last_workgroup(ctr, &last)) return;

    // the last workgroup of the (row, tile): thread d owns bin d
    for (int h = 0; h < nh; ++h) {
        const int gi = FIRST ? h : h / R, g = g0 + gi;
        const uint32_t left = FIRST ? 0u : grem[h];    // read by every thread before the scan's barrier; written after it
        uint32_t excl, incl, total;
        sel_scan_bins(__hip_atomic_load(gh + (size_t)(FIRST ? h * R : h) * 256 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), wsum, excl, incl, total);
        if (FIRST) {
            if (tid == 0 && b == 0) P.counts[g] = (int64_t)total;
            for (int r = 0; r < R; ++r) {
                const size_t s = (size_t)gi * R + r;   // past s0
                const int64_t k = (((int64_t)total + 1) * P.num[r] + P.den[r] - 1) / P.den[r];     // >= 1; below 2^62
                const uint32_t want = k <= (int64_t)total ? (uint32_t)k : 0u;
                if (tid == 0) {
                    if (b == 0) P.ranks[(size_t)g * R + r] = k;
                    if (want == 0u) { grem[s] = 0u; gpre[s] = 0u; P.out[s0 + s] = __uint_as_float(0x7f800000u); }
                }
                sel_fix_digit<true>(want, excl, incl, shift, gpre + s, grem + s, P.out + s0 + s);
            }
        } else sel_fix_digit<false>(left, excl, incl, shift, gpre + h, grem + h, P.out + s0 + h);
        __syncthreads();                               // wsum is rewritten by the next histogram
    }
    for (int h = 0; h < nh; ++h)
        __hip_atomic_store(gh + (size_t)(FIRST ? h * R : h) * 256 + tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) atomicExch(ctr, 0u);
}

// The four passes on a grid of (workgroups per row, B, tiles): about SEL_GRID workgroups in all, at most SEL_ROW_MAX adders per
// (row, tile), and no more than the row has chunks.
template <class Params>
static void sel_run(void (*first)(Params, int), void (*next)(Params, int), Params p, int64_t tiles, hipStream_t st) {
    p.nchunks = (p.n + 3 + SEL_CHUNK - 1) / SEL_CHUNK;
    int64_t per_row = (SEL_GRID + p.B * tiles - 1) / (p.B * tiles);
    if (per_row > SEL_ROW_MAX) per_row = SEL_ROW_MAX;
    if (per_row > p.nchunks) per_row = p.nchunks;
    const dim3 grid((unsigned)per_row, (unsigned)p.B, (unsigned)tiles);
    hipLaunchKernelGGL(first, grid, dim3(SEL_THREADS), 0, st, p, 24);
    for (int shift = 16; shift >= 0; shift -= 8) hipLaunchKernelGGL(next, grid, dim3(SEL_THREADS), 0, st, p, shift);
}

extern "C" {

void selectk_run(const SelectP *P, hipStream_t st) { sel_run(k_select_pass<true>, k_select_pass<false>, *P, 1, st); }

void selectg_run(const SelectGP *P, hipStream_t st) {
    sel_run(k_select_grouped_pass<true>, k_select_grouped_pass<false>, *P, (P->G + P->gt - 1) / P->gt, st);
}

}  // extern "C"
