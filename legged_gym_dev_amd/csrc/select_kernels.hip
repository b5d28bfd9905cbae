// Batched exact k-th smallest (lg_select_kth): most-significant-digit radix select on the order-preserving
// uint32 key of the float, 8 bits per pass, four passes, one launch each.
//
// The key.  u = the float's bits; every NaN -> 0xffffffff (above +inf, whose key is 0xff800000; no other float maps there);
// -0.0 -> +0.0; then u ^ 0x80000000 for u >= 0 and ~u for u < 0.  Unsigned order of the keys is IEEE order of the floats with the
// NaNs on top, which is where torch.sort leaves them.  The way back gives +0.0 for the zero and the canonical quiet NaN.
//
// A pass.  Grid (workgroups per row, B): a 256-thread workgroup walks chunks of SEL_CHUNK consecutive elements of one batch row,
// chunk c, c + gridDim.x, ...; chunks are counted from the 16-byte boundary at or below the row's first element, so that every
// interior load is one aligned 16-byte load whatever b ld is; the groups of four that straddle the row's ends are read element by
// element.  Each kept element adds one to the LDS bin of its digit, once per rank whose prefix its higher digits equal.  Pass one
// has no prefix, so one histogram serves every rank; tube scores have one sign and a few binades, so nearly every lane of a wave
// hits the same one or two bins there, and the pass keeps SEL_COPIES copies of its histogram, lane l adding to copy l % SEL_COPIES
// (consecutive words, different banks), and sums them at the end.  The workgroup then adds its non-zero bins to the row's global
// bins with integer atomics -- the workgroups per row are capped (selectk_run) because every one of them adds up to 256 R words
// to the same 256 R addresses, and that many-adders-one-line traffic, not the reads, set the time of the first version of this
// kernel -- and draws a ticket from the row's counter;
// the workgroup that draws the last one -- the pattern of tube_adam_block.inl -- scans the 256 bins of every rank, fixes the
// digit that holds the rank, takes the count below it off the rank, and clears bins and counter for the next launch.  After the
// fourth pass the prefix is the key and the same workgroup writes out.  Counts are integers: the result does not depend on the
// order in which workgroups arrive, and no float is ever added.
#include "select_device.h"

template <bool FIRST>
__global__ __launch_bounds__(SEL_THREADS) void k_select_pass(SelectP P, int shift) {
    constexpr int NL = FIRST ? SEL_COPIES * 256 : SEL_MAX_R * 256;
    __shared__ uint32_t lh[NL];
    __shared__ uint32_t wsum[SEL_THREADS / 64];
    __shared__ bool last;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, R = P.R, nh = FIRST ? 1 : R;
    uint32_t *__restrict__ gh = P.hist + (size_t)b * R * 256;
    uint32_t *__restrict__ gpre = P.prefix + (size_t)b * R, *__restrict__ grem = P.rem + (size_t)b * R;

    uint32_t pre[SEL_MAX_R];                           // the rank's prefix above this pass's digit; no key has more than 24 bits there
#pragma unroll
    for (int r = 0; r < SEL_MAX_R; ++r) pre[r] = (!FIRST && r < R && grem[r] != 0u) ? gpre[r] >> (shift + 8) : 0xffffffffu;
    for (int i = tid; i < (FIRST ? NL : nh * 256); i += SEL_THREADS) lh[i] = 0u;
    __syncthreads();

    auto take = [&](float f) {
        const uint32_t key = sel_key(f);
        if (FIRST) atomicAdd(&lh[(key >> 24) * SEL_COPIES + (tid & (SEL_COPIES - 1))], 1u);
        else {
            const uint32_t hi = key >> (shift + 8), d = (key >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < SEL_MAX_R; ++r)
                if (hi == pre[r]) atomicAdd(&lh[r * 256 + d], 1u);
        }
    };

    const float *__restrict__ row = P.values + (int64_t)b * P.ld;
    const int64_t mis = (int64_t)(((uintptr_t)row >> 2) & 3u);   // elements between the 16-byte boundary below the row and its start
    const int64_t lo = mis, end = mis + P.n;
    constexpr int ITEMS = SEL_CHUNK / (SEL_THREADS * 4);
  for (int64_t c = blockIdx.x; c < P.nchunks; c += gridDim.x) {
    const int64_t j0 = c * SEL_CHUNK + tid * 4;
    float4 v[ITEMS];
    uint32_t k4[ITEMS];                                // the four keep bytes; 0x01010101 without a mask
    bool full[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int64_t j = j0 + (int64_t)k * SEL_THREADS * 4;
        full[k] = j >= lo && j + 4 <= end;
        k4[k] = 0x01010101u;
        if (full[k]) {
            v[k] = *reinterpret_cast<const float4 *>(row + (j - mis));
            if (P.keep) {
                const uint8_t *kp = P.keep + (j - mis);
                if (((uintptr_t)kp & 3u) == 0) k4[k] = *reinterpret_cast<const uint32_t *>(kp);
                else k4[k] = (uint32_t)kp[0] | ((uint32_t)kp[1] << 8) | ((uint32_t)kp[2] << 16) | ((uint32_t)kp[3] << 24);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        if (full[k]) {
            if (k4[k] & 0x000000ffu) take(v[k].x);
            if (k4[k] & 0x0000ff00u) take(v[k].y);
            if (k4[k] & 0x00ff0000u) take(v[k].z);
            if (k4[k] & 0xff000000u) take(v[k].w);
        } else {
            const int64_t j = j0 + (int64_t)k * SEL_THREADS * 4;
            for (int e = 0; e < 4; ++e) {
                const int64_t i = j + e - mis;
                if (i >= 0 && i < P.n && (!P.keep || P.keep[i] != 0)) take(row[i]);
            }
        }
    }
  }
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
    __threadfence();
    __syncthreads();
    if (tid == 0) last = atomicAdd(P.ctr + b, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();

    // the row's last workgroup: thread d owns bin d
    for (int r = 0; r < R; ++r) {
        const uint32_t left = FIRST ? 0u : grem[r];    // read by every thread before the barrier below; written after it
        const uint32_t c = __hip_atomic_load(gh + (FIRST ? 0 : r) * 256 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
        uint32_t want;                                 // the rank inside this histogram; 0: outside 1..n_kept
        if (FIRST) {
            const int64_t k = P.ranks[(size_t)b * R + r];
            want = (k >= 1 && k <= (int64_t)total) ? (uint32_t)k : 0u;
            if (tid == 0) {
                if (b == 0 && r == 0) *P.n_kept = (int64_t)total;
                if (want == 0u) { grem[r] = 0u; gpre[r] = 0u; P.out[(size_t)b * R + r] = __uint_as_float(0x7f800000u); }
            }
        } else want = left;
        if (want != 0u && excl < want && want <= incl) {       // one thread: the bins partition the counted elements
            const uint32_t p = (FIRST ? 0u : gpre[r]) | ((uint32_t)tid << shift);
            gpre[r] = p;
            grem[r] = want - excl;
            if (shift == 0) P.out[(size_t)b * R + r] = sel_value(p);
        }
        __syncthreads();                               // wsum is rewritten by the next rank
    }
    for (int i = tid; i < nh * 256; i += SEL_THREADS) __hip_atomic_store(gh + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) atomicExch(P.ctr + b, 0u);
}

extern "C" {

void selectk_run(const SelectP *P, hipStream_t st) {
    SelectP p = *P;
    p.nchunks = (p.n + 3 + SEL_CHUNK - 1) / SEL_CHUNK;
    int64_t per_row = (SEL_GRID + p.B - 1) / p.B;      // about SEL_GRID workgroups in all, at most SEL_ROW_MAX adders per row
    if (per_row > SEL_ROW_MAX) per_row = SEL_ROW_MAX;
    if (per_row > p.nchunks) per_row = p.nchunks;
    const dim3 grid((unsigned)per_row, (unsigned)p.B);
    hipLaunchKernelGGL(k_select_pass<true>, grid, dim3(SEL_THREADS), 0, st, p, 24);
    for (int shift = 16; shift >= 0; shift -= 8) hipLaunchKernelGGL(k_select_pass<false>, grid, dim3(SEL_THREADS), 0, st, p, shift);
}

}  // extern "C"
