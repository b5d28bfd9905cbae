// Tube datasets built on the device (lg_tube_rows_build, lg_tube_horizon_build): the rows of tube/data.py
// -- the reference's deep_tube_learning/datasets.py -- from an epoch of records (z, pz_x, v, done) without leaving HBM.
//
// The rule.  Per (env e, step t), t in 0..T-1, a base row b[e, t] of z[e, t], pz_x[e, t], v[e, t]:
//     scalar, recursive      (w, z[2:], v)         w = |pz_x - z| (2-norm)
//     scalar, not recursive  (z[2:], v)            and one column w[e, t] in front of the whole window
//     vector                 (|pz_x - z|, z, v)
//     error dynamics         (pz_x - z, z, v)
// Block i < N of row (e, t) is b[e, src], src = (T-1 - i dN) - (T-1 - t) dN, when src >= 0, else b[e, 0] with its v columns
// zeroed (get_slice: every dN-th sample counted back from the end of the episode, the front padded with the first sample).  The
// target is the leading quantity at t + 1.  The norm is sqrtf of the squares summed in column order, one rounding per operation:
// what np.linalg.norm computes in float32.
//
// Compaction (compact = 1) drops the rows whose step is done, keeping (env, time) order.  It is stable and uses no atomics:
//     k_tube_rows_count   one wave per 64-step chunk of one env: ballot, popcount -> counts[chunk]
//     k_tube_rows_scan    one workgroup: exclusive scan of counts -> offs[chunk] (int64), n_rows
//     k_tube_rows_build   one workgroup per tile of 4 consecutive chunks.  Chunks are ordered (env, time), so a tile's kept rows are
//                         one contiguous span of `data`: the waves resolve slot -> rank with a ballot, leave (e, t) per rank in LDS,
//                         then all 256 threads walk the span element by element -- thread k writes elements k, k + 256, ... -- so a
//                         wave's stores cover 64 consecutive floats whatever input_dim is.  The target span is written the same way.
// The three are separate launches on the caller's stream; no workgroup waits for another.
#include "tube_data_device.h"

#define TD_TILE 4                   // chunks per build workgroup
#define TD_THREADS (TD_CHUNK * TD_TILE)
#define TD_SCAN_THREADS 1024
#define TD_SCAN_ITEMS 8
#define TD_LEADW 0x80000000u        // column table: the single w column of a non-recursive scalar row

__device__ __forceinline__ float td_err_norm(const float *__restrict__ z, const float *__restrict__ pz, int64_t row, int n) {
#pragma clang fp contract(off)
    const float *a = pz + row * n, *b = z + row * n;
    float s = 0.f;
    for (int k = 0; k < n; ++k) {
        const float d = a[k] - b[k];
        s = s + d * d;
    }
    return sqrtf(s);
}

// the leading quantity, column k, of record row `row` = e (T+1) + step
__device__ __forceinline__ float td_lead(const TubeRowsP &P, int64_t row, int k) {
#pragma clang fp contract(off)
    if (P.kind == 0) return td_err_norm(P.z, P.pz, row, P.n);
    const float d = P.pz[row * P.n + k] - P.z[row * P.n + k];
    return P.kind == 1 ? fabsf(d) : d;
}

__device__ __forceinline__ bool td_keep(const TubeRowsP &P, int e, int t) {
    if (t >= P.T) return false;
    if (!P.compact) return true;
    if (P.mark && e % P.epoch_envs == P.epoch_envs - 1) return false;
    return P.done[(int64_t)e * P.T + t] == 0;
}

__global__ __launch_bounds__(TD_THREADS) void k_tube_rows_count(TubeRowsP P, int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * TD_TILE + (threadIdx.x >> 6);
    if (c >= P.nchunks) return;                       // wave-uniform
    const int e = (int)(c / P.cpe), t = (int)(c - (int64_t)e * P.cpe) * TD_CHUNK + lane;
    const unsigned long long b = __ballot(td_keep(P, e, t));
    if (lane == 0) counts[c] = __popcll(b);
}

__global__ __launch_bounds__(TD_SCAN_THREADS) void k_tube_rows_scan(const int32_t *__restrict__ counts, int64_t nchunks,
                                                                    int64_t *__restrict__ offs, int64_t *__restrict__ n_rows) {
    __shared__ int wsum[TD_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < nchunks; base += (int64_t)TD_SCAN_THREADS * TD_SCAN_ITEMS) {
        const int64_t i0 = base + (int64_t)tid * TD_SCAN_ITEMS;
        int c[TD_SCAN_ITEMS], s = 0;
#pragma unroll
        for (int k = 0; k < TD_SCAN_ITEMS; ++k) {
            c[k] = i0 + k < nchunks ? counts[i0 + k] : 0;
            s += c[k];
        }
        int x = s;                                     // inclusive scan over the wave, then over the 16 wave totals
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        if (wv == 0) {
            int w = lane < TD_SCAN_THREADS / 64 ? wsum[lane] : 0;
#pragma unroll
            for (int d = 1; d < TD_SCAN_THREADS / 64; d <<= 1) {
                const int y = __shfl_up(w, d);
                if (lane >= d) w += y;
            }
            if (lane < TD_SCAN_THREADS / 64) wsum[lane] = w;
        }
        __syncthreads();
        int64_t o = carry + (x - s) + (wv ? wsum[wv - 1] : 0);
        carry += wsum[TD_SCAN_THREADS / 64 - 1];
#pragma unroll
        for (int k = 0; k < TD_SCAN_ITEMS; ++k) {
            if (i0 + k < nchunks) offs[i0 + k] = o;
            o += c[k];
        }
        __syncthreads();                               // wsum is rewritten by the next round
    }
    if (tid == 0) *n_rows = carry;
}

__global__ __launch_bounds__(TD_THREADS) void k_tube_rows_build(TubeRowsP P) {
    __shared__ int s_cnt[TD_TILE], s_e[TD_THREADS], s_t[TD_THREADS];
    __shared__ uint32_t s_tab[256];                    // per column: block << 16 | column of the block, or TD_LEADW
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * TD_TILE, c = c0 + wv;
    int e = 0, t = 0;
    bool keep = false;
    if (c < P.nchunks) {
        e = (int)(c / P.cpe);
        t = (int)(c - (int64_t)e * P.cpe) * TD_CHUNK + lane;
        keep = td_keep(P, e, t);
    }
    const unsigned long long b = __ballot(keep);
    const int rank = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wv] = __popcll(b);
    if (tid < P.I) {
        const bool lead = P.kind == 0 && !P.recursive;
        const int q = tid - (lead ? 1 : 0);
        s_tab[tid] = lead && tid == 0 ? TD_LEADW : ((uint32_t)(q / P.bw) << 16) | (uint32_t)(q % P.bw);
    }
    __syncthreads();
    int rel = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TD_TILE; ++w) {
        if (w < wv) rel += s_cnt[w];
        total += s_cnt[w];
    }
    if (keep) { s_e[rel + rank] = e; s_t[rel + rank] = t; }
    __syncthreads();
    int64_t row0;                                      // the tile's first destination row
    if (P.compact) row0 = P.offs[c0];
    else {
        const int e0 = (int)(c0 / P.cpe);
        row0 = (int64_t)e0 * P.T + (c0 - (int64_t)e0 * P.cpe) * TD_CHUNK;
        if (blockIdx.x == 0 && tid == 0) *P.n_rows = (int64_t)P.n_env * P.T;
    }
    const int T = P.T, n = P.n, m = P.m;
    {   // data: total x I floats from row0 I
        float *__restrict__ dst = P.data + row0 * P.I;
        const int nel = total * P.I, qs = TD_THREADS / P.I, rs = TD_THREADS % P.I;
        int r = tid / P.I, col = tid % P.I;
        for (int j = tid; j < nel; j += TD_THREADS) {
            const int re = s_e[r], rt = s_t[r];
            const uint32_t tab = s_tab[col];
            float val;
            if (tab & TD_LEADW) val = td_err_norm(P.z, P.pz, (int64_t)re * (T + 1) + rt, n);
            else {
                const int i = (int)(tab >> 16), cc = (int)(tab & 0xffffu);
                const int64_t src = ((int64_t)(T - 1) - (int64_t)i * P.dN) - (int64_t)(T - 1 - rt) * P.dN;
                const bool pad = src < 0;
                const int64_t s = pad ? 0 : src, row = (int64_t)re * (T + 1) + s;
                if (cc < P.L) val = td_lead(P, row, cc);
                else if (cc < P.L + P.nz) val = P.z[row * n + P.zoff + (cc - P.L)];
                else val = pad ? 0.f : P.v[((int64_t)re * T + s) * m + (cc - P.L - P.nz)];
            }
            dst[j] = val;
            col += rs; r += qs;
            if (col >= P.I) { col -= P.I; ++r; }
        }
    }
    {   // target: total x O floats from row0 O, the leading quantity one step ahead
        float *__restrict__ dst = P.target + row0 * P.O;
        const int nel = total * P.O, qs = TD_THREADS / P.O, rs = TD_THREADS % P.O;
        int r = tid / P.O, col = tid % P.O;
        for (int j = tid; j < nel; j += TD_THREADS) {
            dst[j] = td_lead(P, (int64_t)s_e[r] * (T + 1) + s_t[r] + 1, col);
            col += rs; r += qs;
            if (col >= P.O) { col -= P.O; ++r; }
        }
    }
}

// ScalarHorizonTubeDataset.from_folder's arrays: S = n_env (T + H) slots (e, tp); the record step is max(tp - H, 0).  One flat index
// over the three outputs, each written contiguously: w [0, S), z_no_pos [S, S + S nz), v_pad after it.
__global__ __launch_bounds__(256) void k_tube_horizon_build(const float *__restrict__ z, const float *__restrict__ pz,
                                                            const float *__restrict__ v, int64_t n_env, int T, int n, int m, int H,
                                                            float *__restrict__ w, float *__restrict__ znp, float *__restrict__ vpad) {
    const int nz = n - 2, Tp = T + H;
    const int64_t S = n_env * Tp, total = S * (1 + nz + m);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        int64_t slot;
        int k, seg;
        if (g < S) { slot = g; k = 0; seg = 0; }
        else if (g < S + S * nz) { slot = (g - S) / nz; k = (int)((g - S) - slot * nz); seg = 1; }
        else { const int64_t q = g - S - S * nz; slot = q / m; k = (int)(q - slot * m); seg = 2; }
        const int64_t e = slot / Tp;
        const int tp = (int)(slot - e * Tp), s = tp < H ? 0 : tp - H;
        if (seg == 0) w[slot] = td_err_norm(z, pz, e * (T + 1) + s, n);
        else if (seg == 1) znp[slot * nz + k] = z[(e * (T + 1) + s) * n + 2 + k];
        else vpad[slot * m + k] = tp < H ? 0.f : v[(e * T + s) * m + k];
    }
}

extern "C" {

void tubedatak_rows(const TubeRowsP *P, int32_t *counts, int64_t *offs, hipStream_t st) {
    TubeRowsP p = *P;
    const unsigned grid = (unsigned)((p.nchunks + TD_TILE - 1) / TD_TILE);
    if (p.compact) {
        p.offs = offs;
        hipLaunchKernelGGL(k_tube_rows_count, dim3(grid), dim3(TD_THREADS), 0, st, p, counts);
        hipLaunchKernelGGL(k_tube_rows_scan, dim3(1), dim3(TD_SCAN_THREADS), 0, st, counts, p.nchunks, offs, p.n_rows);
    }
    hipLaunchKernelGGL(k_tube_rows_build, dim3(grid), dim3(TD_THREADS), 0, st, p);
}

void tubedatak_horizon(const float *z, const float *pz, const float *v, int64_t n_env, int T, int n, int m, int H, float *w,
                       float *znp, float *vpad, hipStream_t st) {
    const int64_t total = n_env * (int64_t)(T + H) * (1 + (n - 2) + m);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_tube_horizon_build, dim3((unsigned)blocks), dim3(256), 0, st, z, pz, v, n_env, T, n, m, H, w, znp, vpad);
}

}  // extern "C"
