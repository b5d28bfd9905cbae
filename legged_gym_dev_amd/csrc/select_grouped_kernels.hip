// Grouped exact k-th smallest (lg_select_kth_grouped): the radix select of select_kernels.hip -- the same
// order-preserving key, 8 bits per pass, four launches, integer counting only -- with (group, digit) as the counted key, and each
// group's conformal rank ceil((count + 1) num / den) computed on the device between the first count and the selection.
//
// A pass.  Grid (workgroups per row, B, tiles): a 256-thread workgroup walks chunks of SEL_CHUNK elements of batch row
// blockIdx.y exactly as k_select_pass does (chunks counted from the 16-byte boundary at or below the row's start, aligned float4
// loads inside, element-wise ends) and reads the group ids beside the values, one aligned 16-byte load per four elements where
// the address of group allows.  It counts the groups of tile blockIdx.z only, gt = lg_select_group_tile(R) consecutive groups:
// elements of other groups, and ids outside 0..G-1, are read and skipped.  Pass one keeps one 256-bin LDS histogram per group of
// the tile (no prefix exists yet, and it serves every rank); passes two to four one per (group, rank), an element adding to those
// ranks whose prefix its higher digits equal.  SELG_BINS histograms, 32 KiB, is what a workgroup has.  Neighbouring elements
// belong to different groups in the layouts this serves (the age of a step, element index mod the horizon), so pass one needs no
// copies of its histograms.  The workgroup adds its non-zero bins to the global bins of (row, group, rank) and draws a ticket from
// the counter of its (row, tile); the one that draws the last (the pattern of tube_adam_block.inl) scans the bins of every (group,
// rank) of the tile.  In pass one it writes counts and ranks (from row 0; they are the same for every row), and marks a rank above
// the count as +inf; in every pass it fixes the digit that holds the rank, takes the count below it off the rank, and clears bins
// and counter for the next launch.  After the fourth pass the prefix is the key and it writes out.
#include "select_device.h"

template <bool FIRST>
__global__ __launch_bounds__(SEL_THREADS) void k_select_grouped_pass(SelectGP P, int shift) {
    __shared__ uint32_t lh[SELG_BINS * 256];
    __shared__ uint32_t lpre[SELG_BINS];               // the prefix of (group of the tile, rank) above this pass's digit
    __shared__ uint32_t wsum[SEL_THREADS / 64];
    __shared__ bool last;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, R = P.R, G = P.G;
    const int g0 = blockIdx.z * P.gt, ng = min(P.gt, G - g0);      // the tile's groups g0 .. g0 + ng - 1; ng R <= SELG_BINS
    const int nh = FIRST ? ng : ng * R;
    const size_t s0 = ((size_t)b * G + g0) * R;                    // (row, first group of the tile, rank 0)
    uint32_t *__restrict__ gh = P.hist + s0 * 256;
    uint32_t *__restrict__ gpre = P.prefix + s0, *__restrict__ grem = P.rem + s0;
    uint32_t *__restrict__ ctr = P.ctr + (size_t)b * gridDim.z + blockIdx.z;

    if (!FIRST && tid < ng * R) lpre[tid] = grem[tid] != 0u ? gpre[tid] >> (shift + 8) : 0xffffffffu;   // no key has more than 24 bits there
    for (int i = tid; i < nh * 256; i += SEL_THREADS) lh[i] = 0u;
    __syncthreads();

    auto take = [&](float f, int32_t gid) {
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
    };

    const float *__restrict__ row = P.values + (int64_t)b * P.ld;
    const int64_t mis = (int64_t)(((uintptr_t)row >> 2) & 3u);   // elements between the 16-byte boundary below the row and its start
    const bool galign = (int64_t)(((uintptr_t)P.group >> 2) & 3u) == mis;     // group + (j - mis) is 16-byte aligned where row + (j - mis) is
    const int64_t lo = mis, end = mis + P.n;
    constexpr int ITEMS = SEL_CHUNK / (SEL_THREADS * 4);
  for (int64_t c = blockIdx.x; c < P.nchunks; c += gridDim.x) {
    const int64_t j0 = c * SEL_CHUNK + tid * 4;
    float4 v[ITEMS];
    int4 g4[ITEMS];
    bool full[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t j = j0 + (int64_t)k * SEL_THREADS * 4;
        full[k] = j >= lo && j + 4 <= end;
        if (full[k]) {
            v[k] = *reinterpret_cast<const float4 *>(row + (j - mis));
            const int32_t *gp = P.group + (j - mis);
            if (galign) g4[k] = *reinterpret_cast<const int4 *>(gp);
            else g4[k] = make_int4(gp[0], gp[1], gp[2], gp[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        if (full[k]) {
            take(v[k].x, g4[k].x);
            take(v[k].y, g4[k].y);
            take(v[k].z, g4[k].z);
            take(v[k].w, g4[k].w);
        } else {
            const int64_t j = j0 + (int64_t)k * SEL_THREADS * 4;
            for (int e = 0; e < 4; ++e) {
                const int64_t i = j + e - mis;
                if (i >= 0 && i < P.n) take(row[i], P.group[i]);
            }
        }
    }
  }
    __syncthreads();
    for (int i = tid; i < nh * 256; i += SEL_THREADS) {
        const uint32_t c = lh[i];                      // pass one: histogram i >> 8 is group g0 + (i >> 8), kept in the bins of its rank 0
        if (c) atomicAdd(&gh[FIRST ? (size_t)(i >> 8) * R * 256 + (i & 255) : (size_t)i], c);
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) last = atomicAdd(ctr, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();

    // the last workgroup of the (row, tile): thread d owns bin d
    for (int h = 0; h < nh; ++h) {
        const int gi = FIRST ? h : h / R, g = g0 + gi;
        const uint32_t left = FIRST ? 0u : grem[h];    // read by every thread before the barrier below; written after it
        const uint32_t c = __hip_atomic_load(gh + (size_t)(FIRST ? h * R : h) * 256 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t x = c;                                // inclusive scan over the wave, then the four wave totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        uint32_t base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SEL_THREADS / 64; ++w) {
            if (w < wv) base += wsum[w];
            total += wsum[w];
        }
        const uint32_t incl = base + x, excl = incl - c;
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
                if (want != 0u && excl < want && want <= incl) {   // one thread: the bins partition the group's elements
                    gpre[s] = (uint32_t)tid << 24;
                    grem[s] = want - excl;
                }
            }
        } else if (left != 0u && excl < left && left <= incl) {
            const uint32_t p = gpre[h] | ((uint32_t)tid << shift);
            gpre[h] = p;
            grem[h] = left - excl;
            if (shift == 0) P.out[s0 + h] = sel_value(p);
        }
        __syncthreads();                               // wsum is rewritten by the next histogram
    }
    for (int h = 0; h < nh; ++h)
        __hip_atomic_store(gh + (size_t)(FIRST ? h * R : h) * 256 + tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) atomicExch(ctr, 0u);
}

extern "C" {

void selectg_run(const SelectGP *P, hipStream_t st) {
    SelectGP p = *P;
    p.nchunks = (p.n + 3 + SEL_CHUNK - 1) / SEL_CHUNK;
    const int64_t tiles = (p.G + p.gt - 1) / p.gt;
    int64_t per_row = (SEL_GRID + p.B * tiles - 1) / (p.B * tiles);     // about SEL_GRID workgroups in all, at most SEL_ROW_MAX adders per (row, tile)
    if (per_row > SEL_ROW_MAX) per_row = SEL_ROW_MAX;
    if (per_row > p.nchunks) per_row = p.nchunks;
    const dim3 grid((unsigned)per_row, (unsigned)p.B, (unsigned)tiles);
    hipLaunchKernelGGL(k_select_grouped_pass<true>, grid, dim3(SEL_THREADS), 0, st, p, 24);
    for (int shift = 16; shift >= 0; shift -= 8) hipLaunchKernelGGL(k_select_grouped_pass<false>, grid, dim3(SEL_THREADS), 0, st, p, shift);
}

}  // extern "C"
