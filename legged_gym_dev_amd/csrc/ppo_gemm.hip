// GEMM layer of the PPO update and rollout: fp32 GEMMs with fused epilogues for the ActorCritic forward, input gradient and weight
// gradient, on the split-bf16 mainloops (ppo_split_bf16.h) and the LDS-DMA forward (ppo_gemm_glds.h), plus the fp32-input MFMA
// reference the tests compare them against.  Entry points: ppok_gemm_fwd / _dx / _dw and the ppok_debug_* hooks.
#include <cstring>
#include <type_traits>

#include "ppo_launch.h"
#include "ppo_split_bf16.h"

// XCD-aware workgroup -> tile map.  The 8 XCDs of an MI355X have private L2s and workgroups are dealt to them round-robin by
// linear workgroup id, so neighbouring ids -- the column tiles of one row block, the output tiles of one reduction slice --
// land on 8 different L2s and each fetches its own copy of the operand rows they share.  remap(l) regroups the ids so that
// the `inner` workgroups that share operand rows get the same XCD: XCD c owns outer indices c, c + 8, ...
__device__ __forceinline__ void xcd_tile(int lin, int inner, int outer, int &o, int &i) {
    if ((outer & 7) == 0) {
        const int c = lin & 7, j = lin >> 3;
        o = c + 8 * (j / inner);
        i = j % inner;
    } else {
        o = lin / inner;
        i = lin % inner;
    }
}

// ------------------------------------------------------------------------------------------------
// C[M,N] = opA(A) . opB(B), K = reduction length.  A_RC: A stored [m][k] (reduction contiguous),
// else [k][m].  B_RC: B stored [n][k], else [k][n].  4 waves as 2x2, each TM x TN tiles of 32x32
// computed with v_mfma_f32_32x32x2_f32 (exact fp32, A/B one VGPR per lane: lane l holds
// A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]).
// LDS tiles keep the global layout (so the global->LDS copy is a straight 16-byte move) with a
// one-float row pad; fragments are ds_read_b32 with lanes on consecutive rows/columns, which is
// bank-conflict free in both layouts and far below the LDS rate at 64 cycles per fp32 MFMA.
// EPI 0: C = act(acc + bias[n]), act = g.elu code (forward, nn.Linear + activation; 0 on the head layer)
// EPI 1: C = acc * act'(aux[m][n]); colsum[n] += sum_m C   (input gradient + bias gradient below)
// EPI 2: C += acc via float atomics, reduction split over blockIdx.y   (weight gradient)
#define BK 32

// Prologue of the GEMM kernels: the workgroup's problem z = blockIdx.z and its M x N output in BM x BN tiles.  The launch grid is
// sized for the largest problem of the launch: false for the workgroups past this problem's tiles.
// A kernel that remaps its workgroups over this problem's own tiles (xcd_tile on tiles_n x tiles_m) tests the raw blockIdx.x, as
// gemm_tiles does.  One that remaps over the whole GRID (k_gemm_dw_t: the grid's tiles x its reduction slices) takes gemm_problem and
// tests the REMAPPED tile: that map is a bijection on the grid only, not on the smaller problem's share of it.
struct GemmTiles { int z, M, N, K, tiles_n, tiles_m; };
template <int BM, int BN>
__device__ __forceinline__ void gemm_problem(const GemmArgs &g, GemmTiles &t) {
    t.z = blockIdx.z;
    t.M = g.M[t.z]; t.N = g.N[t.z]; t.K = g.K[t.z];
    t.tiles_n = (t.N + BN - 1) / BN; t.tiles_m = (t.M + BM - 1) / BM;
}
template <int BM, int BN>
__device__ __forceinline__ bool gemm_tiles(const GemmArgs &g, GemmTiles &t) {
    gemm_problem<BM, BN>(g, t);
    return (int)blockIdx.x < t.tiles_n * t.tiles_m;
}
// reduction range of slice `slice` when the launch splits K into gridDim.y slices of whole k-tiles; false when it is empty
__device__ __forceinline__ bool k_slice(int K, int slice, int &k_begin, int &k_end) {
    const int per = ((K + gridDim.y - 1) / gridDim.y + BK - 1) / BK * BK;
    k_begin = slice * per;
    k_end = min(K, k_begin + per);
    return k_begin < k_end;
}

template <bool RC, int ROWS, bool VEC, bool KSEQ = false, int NT = 256, bool FULL = false>
__device__ __forceinline__ void stage_load(const float *__restrict__ src, int ld, int row0, int red0, int nrows, int nred,
                                           float4 (&regs)[ROWS * BK / 4 / NT], unsigned &mask) {
    constexpr int NV = ROWS * BK / 4 / NT;
    const int tid = threadIdx.x & (NT - 1);      // index inside the group of NT threads that stages this tile (= threadIdx.x unless
                                                 // the workgroup holds two such groups: k_gemm_pp)
    const int row_lim = RC ? nrows : nred, col_lim = RC ? nred : nrows;
    mask = 0u;                          // bit v: regs[v] is in range (applied at stage_store, so that nothing
                                        // consumes the loaded data -- and waits on it -- before the MFMA block)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int idx = tid + v * NT;
        int r, c;                       // r: index along the tile's non-contiguous dim, c: float4 along the contiguous one
        if (RC) { c = idx & (BK / 4 - 1); r = idx / (BK / 4); }
        else if (KSEQ) { c = tid & (ROWS / 4 - 1); r = NV * (tid / (ROWS / 4)) + v; }   // NV consecutive k per thread
        else { c = idx & (ROWS / 4 - 1); r = idx / (ROWS / 4); }
        const int grow = RC ? row0 + r : red0 + r;        // global row
        const int gcol = RC ? red0 + 4 * c : row0 + 4 * c;
        if (FULL) {                     // tile entirely in range (workgroup-uniform): no clamps, no mask
            regs[v] = *reinterpret_cast<const float4 *>(src + (size_t)grow * ld + gcol);
            mask = ~0u;
        } else if (VEC) {
            // branch-free: every lane loads 16 B from a clamped (always valid) address and zeroes it by
            // select when out of range -- a guarded load makes hipcc wait vmcnt(0) per element.
            // VEC implies col_lim % 4 == 0, so a float4 is entirely inside or entirely outside.
            const int rc_ = min(grow, row_lim - 1), cc_ = min(gcol, col_lim - 4);
            regs[v] = *reinterpret_cast<const float4 *>(src + (size_t)rc_ * ld + cc_);
            mask |= (grow < row_lim && gcol < col_lim) ? (1u << v) : 0u;
        } else {
            const int rc_ = min(grow, row_lim - 1);
            const float *p = src + (size_t)rc_ * ld;
            const bool rin = grow < row_lim;
            float e[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cc_ = min(gcol + q, col_lim - 1);
                const float x = p[cc_];
                e[q] = (rin && gcol + q < col_lim) ? x : 0.f;
            }
            regs[v] = make_float4(e[0], e[1], e[2], e[3]);
            mask |= 1u << v;
        }
    }
}
template <bool RC, int ROWS>
__device__ __forceinline__ void stage_store(float *__restrict__ lds, const float4 (&regs_in)[ROWS * BK / 4 / 256], unsigned mask) {
    constexpr int NV = ROWS * BK / 4 / 256;
    const int tid = threadIdx.x;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        int idx = tid + v * 256;
        const bool in = (mask >> v) & 1u;
        float4 regs[1];
        regs[0] = make_float4(in ? regs_in[v].x : 0.f, in ? regs_in[v].y : 0.f, in ? regs_in[v].z : 0.f, in ? regs_in[v].w : 0.f);
        if (RC) {                       // lds[r][BK+1]
            int c = idx & (BK / 4 - 1), r = idx / (BK / 4);
            float *d = lds + r * (BK + 1) + 4 * c;
            d[0] = regs[0].x; d[1] = regs[0].y; d[2] = regs[0].z; d[3] = regs[0].w;
        } else {                        // lds[k][ROWS+4]
            int c = idx & (ROWS / 4 - 1), r = idx / (ROWS / 4);
            *reinterpret_cast<float4 *>(lds + r * (ROWS + 4) + 4 * c) = regs[0];
        }
    }
}
template <bool RC, int ROWS>
__device__ __forceinline__ float frag(const float *__restrict__ lds, int row, int k) {
    return RC ? lds[row * (BK + 1) + k] : lds[k * (ROWS + 4) + row];
}
template <bool RC, int ROWS>
constexpr int tile_floats() { return RC ? ROWS * (BK + 1) : BK * (ROWS + 4); }

template <bool A_RC, bool B_RC, int TM, int TN, bool VEC>
__device__ __forceinline__ void gemm_mainloop(const float *__restrict__ A, const float *__restrict__ B, int lda, int ldb, int m0, int n0,
                                              int M, int N, int k_begin, int k_end, float *__restrict__ lds, int wm, int wn, int li, int lk,
                                              f32x16 (&acc)[TM][TN]) {
    constexpr int BM = 64 * TM, BN = 64 * TN;
    constexpr int AF = tile_floats<A_RC, BM>(), BF = tile_floats<B_RC, BN>();
    float4 ra[BM * BK / 4 / 256], rb[BN * BK / 4 / 256];
    unsigned ma, mb_;
    stage_load<A_RC, BM, VEC>(A, lda, m0, k_begin, M, k_end, ra, ma);
    stage_load<B_RC, BN, VEC>(B, ldb, n0, k_begin, N, k_end, rb, mb_);
    stage_store<A_RC, BM>(lds, ra, ma);
    stage_store<B_RC, BN>(lds + AF, rb, mb_);
    __syncthreads();
    for (int k0 = k_begin; k0 < k_end; k0 += BK) {
        const bool more = k0 + BK < k_end;
        if (more) {
            stage_load<A_RC, BM, VEC>(A, lda, m0, k0 + BK, M, k_end, ra, ma);
            stage_load<B_RC, BN, VEC>(B, ldb, n0, k0 + BK, N, k_end, rb, mb_);
        }
        const float *as = lds, *bs = as + AF;
        // fragments are fetched one group (GS k-steps) ahead of the MFMAs that consume them, so the
        // LDS latency is paid once per k-tile instead of once per k-step
        constexpr int GS = 4, NG = BK / 2 / GS;
        float av[2][GS][TM], bv[2][GS][TN];
#pragma unroll
        for (int s = 0; s < GS; ++s) {
#pragma unroll
            for (int a = 0; a < TM; ++a) av[0][s][a] = frag<A_RC, BM>(as, wm + 32 * a + li, 2 * s + lk);
#pragma unroll
            for (int b = 0; b < TN; ++b) bv[0][s][b] = frag<B_RC, BN>(bs, wn + 32 * b + li, 2 * s + lk);
        }
#pragma unroll
        for (int gq = 0; gq < NG; ++gq) {
            if (gq + 1 < NG) {
#pragma unroll
                for (int s = 0; s < GS; ++s) {
                    const int ks = 2 * ((gq + 1) * GS + s) + lk;
#pragma unroll
                    for (int a = 0; a < TM; ++a) av[(gq + 1) & 1][s][a] = frag<A_RC, BM>(as, wm + 32 * a + li, ks);
#pragma unroll
                    for (int b = 0; b < TN; ++b) bv[(gq + 1) & 1][s][b] = frag<B_RC, BN>(bs, wn + 32 * b + li, ks);
                }
            }
#pragma unroll
            for (int s = 0; s < GS; ++s)
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[gq & 1][s][a], bv[gq & 1][s][b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();                         // every wave is done reading before the tile is refilled
        if (more) {
            stage_store<A_RC, BM>(lds, ra, ma);
            stage_store<B_RC, BN>(lds + AF, rb, mb_);
        }
        __syncthreads();
    }
}


// ------------------------------------------------------------------------------------------------
// Split-bf16 ("bf16x6") mainloop: the same fp32 GEMM computed on the bf16 matrix cores, which on gfx950 run 16x the fp32-input
// MFMA rate, with the split and the six term products of ppo_split_bf16.h.  6 bf16 MFMAs of 32 cycles replace 8 fp32 MFMAs of 64
// per 32x32x16 block: 2.67x the MFMA-bound rate at fp32 accuracy (tests/test_hip_ppo.py checks both paths against float64).
//
// LDS image per operand: 3 planes [physical row][32 bf16 + 16 B pad] (80-B rows: a 5-slot stride
// keeps the 16-lane groups of ds_read_b128 on distinct 16-B slots).  Logical row r lives at
// physical row (r&3)*(ROWS/4+4) + (r>>2): the operand whose reduction dimension is NOT contiguous
// in memory arrives as float4s along the rows, and this places the four rows of one float4 in
// four different bank phases while fragment reads (32 consecutive rows) stay conflict-free.
#define X6_ROWB 80
template <int ROWS>
__device__ __forceinline__ int x6_prow(int r) { return (r & 3) * (ROWS / 4 + 4) + (r >> 2); }
template <int ROWS>
constexpr int x6_plane_bytes() { return (ROWS + 16) * X6_ROWB; }

template <bool RC, int ROWS, int NT, bool FULL = false>
__device__ __forceinline__ void stage_store_x6(unsigned char *__restrict__ lds, const float4 (&regs)[ROWS * BK / 4 / NT], unsigned mask) {
    constexpr int NV = ROWS * BK / 4 / NT;
    constexpr int PL = x6_plane_bytes<ROWS>();
    const int tid = threadIdx.x & (NT - 1);
    if constexpr (RC) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int idx = tid + v * NT;
            const int c = idx & (BK / 4 - 1), r = idx / (BK / 4);
            const bool in = FULL || ((mask >> v) & 1u);
            const float x0 = in ? regs[v].x : 0.f, x1 = in ? regs[v].y : 0.f, x2 = in ? regs[v].z : 0.f, x3 = in ? regs[v].w : 0.f;
            uint32_t h0, m0, l0, h1, m1, l1;
            split2(x0, x1, h0, m0, l0);
            split2(x2, x3, h1, m1, l1);
            unsigned char *d = lds + x6_prow<ROWS>(r) * X6_ROWB + 8 * c;
            *reinterpret_cast<uint2 *>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2 *>(d + PL) = make_uint2(m0, m1);
            *reinterpret_cast<uint2 *>(d + 2 * PL) = make_uint2(l0, l1);
        }
    } else {
        // regs[v] = rows 4c..4c+3 at k = NV*kg + v (stage_load KSEQ mapping)
        const int c = tid & (ROWS / 4 - 1), kg = tid / (ROWS / 4);
        float e[4][NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const bool in = FULL || ((mask >> v) & 1u);
            e[0][v] = in ? regs[v].x : 0.f; e[1][v] = in ? regs[v].y : 0.f;
            e[2][v] = in ? regs[v].z : 0.f; e[3][v] = in ? regs[v].w : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned char *d = lds + (q * (ROWS / 4 + 4) + c) * X6_ROWB + 2 * NV * kg;
            if (NV == 4) {
                uint32_t h0, m0, l0, h1, m1, l1;
                split2(e[q][0], e[q][1], h0, m0, l0);
                split2(e[q][2 % NV], e[q][3 % NV], h1, m1, l1);
                *reinterpret_cast<uint2 *>(d) = make_uint2(h0, h1);
                *reinterpret_cast<uint2 *>(d + PL) = make_uint2(m0, m1);
                *reinterpret_cast<uint2 *>(d + 2 * PL) = make_uint2(l0, l1);
            } else {
                static_assert(NV == 4 || NV == 2, "tile/threads combination");
                uint32_t h0, m0, l0;
                split2(e[q][0], e[q][1 % NV], h0, m0, l0);
                *reinterpret_cast<uint32_t *>(d) = h0;
                *reinterpret_cast<uint32_t *>(d + PL) = m0;
                *reinterpret_cast<uint32_t *>(d + 2 * PL) = l0;
            }
        }
    }
}

// B operand already split (weight planes kept by the optimiser step): the tile is three [ROWS][32] bf16 images,
// staged as plain 16-byte copies -- no conversion work in the loop.  Chunk c of a tile: plane c / (ROWS*4),
// row (c / 4) % ROWS, 16-byte quarter c % 4 of the row's 64 bytes.
template <int ROWS, int NT>
__device__ __forceinline__ void stage_load_pl(const uint16_t *__restrict__ src, int64_t pl_stride, int ld, int row0, int red0, int nrows,
                                              int nred, uint4 (&regs)[ROWS * 12 / NT], unsigned &mask) {
    constexpr int NV = ROWS * 12 / NT;
    mask = 0u;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (threadIdx.x & (NT - 1)) + v * NT;
        const int pl = c / (ROWS * 4), r = (c >> 2) % ROWS, q = c & 3;
        const int grow = row0 + r, gk = red0 + 8 * q;
        const int rc_ = min(grow, nrows - 1), kc_ = min(gk, nred - 8);      // nred % 8 == 0 (checked by the launcher)
        regs[v] = *reinterpret_cast<const uint4 *>(src + pl * pl_stride + (size_t)rc_ * ld + kc_);
        mask |= (grow < nrows && gk < nred) ? (1u << v) : 0u;
    }
}
template <int ROWS, int NT>
__device__ __forceinline__ void stage_store_pl(unsigned char *__restrict__ lds, const uint4 (&regs)[ROWS * 12 / NT], unsigned mask) {
    constexpr int NV = ROWS * 12 / NT;
    constexpr int PL = x6_plane_bytes<ROWS>();
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (threadIdx.x & (NT - 1)) + v * NT;
        const int pl = c / (ROWS * 4), r = (c >> 2) % ROWS, q = c & 3;
        const bool in = (mask >> v) & 1u;
        const uint4 x = in ? regs[v] : make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4 *>(lds + pl * PL + x6_prow<ROWS>(r) * X6_ROWB + 16 * q) = x;
    }
}

// B operand from the SAME weight planes when the reduction runs over the planes' ROWS (input gradient: dz . W with W [k][n],
// n contiguous): the k-tile is staged as it lies in memory -- [32 k-rows][BN n-columns] bf16 per plane, plain 16-byte copies --
// and the fragments (8 consecutive k for one n per lane) come out of gfx950's transposing LDS read, two
// ds_read_b64_tr_b16 (4 k x 16 n each per 16-lane group) per operand.  Image: 8-row x 32-column subtiles of 512 B with the
// chunk XOR of cdna_hip_programming.md T10 image (a): off(row, ch) = GRP (row>>3) + 512 (ch>>2) + 64 (row&7) +
// 16 ((ch&3) ^ ((row>>2)&3)), ch = 16-byte chunk of the row, GRP = 512 BN/32 -- conflict-free for both the b128 stores'
// rows and the transposed reads.
// Subtile stride PLT_SUB = 512 + 64 bytes: with subtiles exactly 512 B apart the 4 (stores of 16 B: 16 lanes, stores of 8 B: 32
// lanes) subtiles one k-row spans fall on the SAME 16 banks -- a 4-way conflict on every staging store (SQ_LDS_BANK_CONFLICT = 17 % of the LDS
// cycles of the input-gradient kernel, 29-33 % of the weight-gradient kernels': profiles/r03_kernel_clocks.txt).  The 64-byte pad rotates
// them onto the four quarters of the bank row; a transposed read stays inside one subtile and is unaffected.
constexpr int PLT_SUB = 576;
template <int BN>
__device__ __forceinline__ int plt_off(int row, int ch) {
    return (BN / 32 * PLT_SUB) * (row >> 3) + PLT_SUB * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}
template <int BN>
constexpr int plt_plane_bytes() { return BK / 8 * (BN / 32) * PLT_SUB; }

template <int BN, int NT>
__device__ __forceinline__ void stage_load_plt(const uint16_t *__restrict__ src, int64_t pl_stride, int ld, int n0, int red0, int ncols,
                                               int nred, uint4 (&regs)[BK * BN / 8 * 3 / NT], unsigned &mask) {
    constexpr int CPR = BN / 8, NV = BK * CPR * 3 / NT;         // chunks per row; chunks per thread
    mask = 0u;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (threadIdx.x & (NT - 1)) + v * NT;
        const int pl = c / (BK * CPR), k = (c / CPR) % BK, ch = c % CPR;
        const int gk = red0 + k, gn = n0 + 8 * ch;
        const int kc_ = min(gk, nred - 1), nc_ = min(gn, ncols - 8);      // ncols % 8 == 0 (checked by the launcher)
        regs[v] = *reinterpret_cast<const uint4 *>(src + pl * pl_stride + (size_t)kc_ * ld + nc_);
        mask |= (gk < nred && gn < ncols) ? (1u << v) : 0u;
    }
}
template <int BN, int NT>
__device__ __forceinline__ void stage_store_plt(unsigned char *__restrict__ lds, const uint4 (&regs)[BK * BN / 8 * 3 / NT], unsigned mask) {
    constexpr int CPR = BN / 8, NV = BK * CPR * 3 / NT;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = (threadIdx.x & (NT - 1)) + v * NT;
        const int pl = c / (BK * CPR), k = (c / CPR) % BK, ch = c % CPR;
        const bool in = (mask >> v) & 1u;
        const uint4 x = in ? regs[v] : make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4 *>(lds + pl * plt_plane_bytes<BN>() + plt_off<BN>(k, ch)) = x;
    }
}

template <bool A_RC, bool B_RC, int TM, int TN, int WGM, int WGN, bool VEC, bool FULL = false, int B_PL = 0>
__device__ __forceinline__ void gemm_mainloop_x6(const float *__restrict__ A, const float *__restrict__ B, int lda, int ldb, int m0, int n0,
                                                 int M, int N, int k_begin, int k_end, unsigned char *__restrict__ lds, int wm, int wn, int li,
                                                 int lk, f32x16 (&acc)[TM][TN], const uint16_t *__restrict__ Bpl = nullptr,
                                                 int64_t pl_stride = 0) {
    constexpr int BM = 32 * TM * WGM, BN = 32 * TN * WGN, NT = 64 * WGM * WGN;
    constexpr int APL = x6_plane_bytes<BM>(), BPL = B_PL == 2 ? plt_plane_bytes<BN>() : x6_plane_bytes<BN>();
    constexpr int NVA = BM * BK / 4 / NT, NVB = BN * BK / 4 / NT;
    // two register sets: the global loads of k-tile t+2 are issued before the MFMAs of tile t, and tile t+1 (already
    // landed) is split and stored after them -- one full iteration to cover the L2/HBM latency.
    // Measured and not kept: two LDS stages (the split + store of tile t+1 to the other stage, overlapping the MFMAs of tile t), NEUTRAL
    // for the 64x64 configuration (12.5 vs 13.1 us per rollout GEMM), as was a prefetch distance of 4: those launches are bound by
    // their fixed cost (~7 us for a K = 48 or K = 128 layer) and were replaced by the one-launch forward of ppo_mlp_fused.hip.
    constexpr int PD = 2;
    constexpr int NVP = B_PL ? BN * 12 / NT : 1;                 // 16-byte chunks of a plane k-tile per thread (either plane layout)
    struct Regs { float4 a[NVA], b[NVB]; uint4 p[NVP]; unsigned ma = 0, mb = 0; };
    Regs R[PD];
    unsigned char *lds_b = lds + 3 * APL;
    auto load_tile = [&](Regs &r, int k) {
        stage_load<A_RC, BM, VEC, true, NT, FULL>(A, lda, m0, k, M, k_end, r.a, r.ma);
        if constexpr (B_PL == 2) stage_load_plt<BN, NT>(Bpl, pl_stride, ldb, n0, k, N, k_end, r.p, r.mb);
        else if constexpr (B_PL == 1) stage_load_pl<BN, NT>(Bpl, pl_stride, ldb, n0, k, N, k_end, r.p, r.mb);
        else stage_load<B_RC, BN, VEC, true, NT, FULL>(B, ldb, n0, k, N, k_end, r.b, r.mb);
    };
    auto store_tile = [&](Regs &r) {
        stage_store_x6<A_RC, BM, NT, FULL>(lds, r.a, r.ma);
        if constexpr (B_PL == 2) stage_store_plt<BN, NT>(lds_b, r.p, r.mb);
        else if constexpr (B_PL == 1) stage_store_pl<BN, NT>(lds_b, r.p, r.mb);
        else stage_store_x6<B_RC, BN, NT, FULL>(lds_b, r.b, r.mb);
    };
    load_tile(R[0], k_begin);
#pragma unroll
    for (int d = 1; d < PD; ++d)
        if (k_begin + d * BK < k_end) load_tile(R[d], k_begin + d * BK);
    store_tile(R[0]);
    lds_barrier();
    // fragment of tile a, plane p, k-step s: base + a*8*X6_ROWB (32 logical rows = 8 physical) + p*PL + s*32
    const unsigned char *fa = lds + x6_prow<BM>(wm + li) * X6_ROWB + 16 * lk;
    const unsigned char *fb = lds_b + x6_prow<BN>(wn + li) * X6_ROWB + 16 * lk;
    // transposed-read bases of this lane (B_PL == 2): group g = lane >> 4 takes n-columns 16 (g & 1) .. +15 and k-rows
    // 8 (g >> 1) + 4 h .. +3 of a k-step; lane 4 q + p of the group addresses row q, half-chunk p (T10)
    const int tg = (threadIdx.x >> 4) & 3, tq = (threadIdx.x >> 2) & 3, tp = threadIdx.x & 3;
    const unsigned char *ft[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
        ft[h] = lds_b + (BN / 32 * PLT_SUB) * (tg >> 1) + PLT_SUB * (wn / 32) + 64 * (4 * h + tq) +
                16 * ((2 * (tg & 1) + (tp >> 1)) ^ (2 * (tg >> 1) + h)) + 8 * (tp & 1);
    auto read_b = [&](int b, int p, int s) -> bf16x8 {
        if constexpr (B_PL == 2) {
            const int o = PLT_SUB * b + p * BPL + (BN / 32 * PLT_SUB) * 2 * s;
            return lds_read_tr_frag(ft[0] + o, ft[1] + o);
        } else {
            return *reinterpret_cast<const bf16x8 *>(fb + b * 8 * X6_ROWB + p * BPL + s * 32);
        }
    };

    // one k-tile: x = the set holding tile k0 + BK (stored to LDS after the MFMAs), y = the set tile k0 + PD BK is loaded into.
    // Measured and not kept: a steady-state loop with the prefetch and the store unconditional.  hipcc counts s_waitcnt vmcnt per
    // path and takes the minimum where paths join, so behind the guarded prefetch the store of tile k0 + BK waits for loads issued a
    // few hundred cycles earlier (vmcnt(3)..(0) instead of (8)..(5) in the ISA); without the join it does not, and measures the same
    // (profiles/r03_ab.txt: the other resident workgroup covers the wait).
    auto body = [&](int k0, Regs &x, Regs &y) {
        if (k0 + PD * BK < k_end) load_tile(y, k0 + PD * BK);
        bf16x8 av[2][TM][3], bv[2][TN][3];
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int p = 0; p < 3; ++p) av[0][a][p] = *reinterpret_cast<const bf16x8 *>(fa + a * 8 * X6_ROWB + p * APL);
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int p = 0; p < 3; ++p) bv[0][b][p] = read_b(b, p, 0);
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            if (s + 1 < BK / 16) {
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        av[(s + 1) & 1][a][p] = *reinterpret_cast<const bf16x8 *>(fa + a * 8 * X6_ROWB + p * APL + (s + 1) * 32);
#pragma unroll
                for (int b = 0; b < TN; ++b)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        bv[(s + 1) & 1][b][p] = read_b(b, p, s + 1);
            }
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = mfma_x6(av[s & 1][a], bv[s & 1][b], acc[a][b]);
        }
        lds_barrier();                         // every wave is done reading before the tile is refilled
        if (k0 + BK < k_end) store_tile(x);
        lds_barrier();
    };
    for (int k0 = k_begin; k0 < k_end; k0 += PD * BK) {
#pragma unroll
        for (int d = 0; d < PD; ++d)
            if (d == 0 || k0 + d * BK < k_end) body(k0 + d * BK, R[(d + 1) % PD], R[d]);
    }
}

// Epilogue of the GEMM kernels.  acc[a][b][r]: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).  ACT: 1 = ELU and 0 = none
// are compiled in (the reference's configurations); -1 = the activation code g.elu is switched on per element.
template <int EPI, int TM, int TN, int BM, int BN, int ACT>
__device__ __forceinline__ void gemm_epilogue_act(const GemmArgs &g, int z, int M, int N, int m0, int n0, int wm, int wn, int li, int lk, int ldc,
                                              f32x16 (&acc)[TM][TN]) {
    float *__restrict__ C = g.C[z];
    const bool interior = (m0 + BM <= M) && (n0 + BN <= N);     // workgroup-uniform
    const int elu = g.elu;                                      // activation code (workgroup-uniform)
    if (interior) {
        // unguarded path: loads of the epilogue operand are issued as one batch (no per-element branch,
        // which would serialise them behind s_waitcnt vmcnt(0)), then compute + store
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const int n = n0 + wn + 32 * b + li;
            float csum = 0.f;
            const float bias = (EPI == 0 && g.bias[z]) ? g.bias[z][n] : 0.f;
#pragma unroll
            for (int a = 0; a < TM; ++a) {
                const int mb = m0 + wm + 32 * a + 4 * lk;
                float aux[16];
                if (EPI == 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        aux[r] = g.aux[z][(size_t)(mb + (r & 3) + 8 * (r >> 2)) * g.ldaux[z] + n];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float *cp = &C[(size_t)(mb + (r & 3) + 8 * (r >> 2)) * ldc + n];
                    float v = acc[a][b][r];
                    if (EPI == 0) {
                        v += bias;
                        v = (ACT == 1 ? (v > 0.f ? v : __expf(v) - 1.0f) : ACT == 0 ? v : act_fwd(elu, v));
                        *cp = v;
                    } else if (EPI == 1) {
                        v *= (ACT == 1 ? (aux[r] > 0.f ? 1.0f : aux[r] + 1.0f) : ACT == 0 ? 1.0f : act_bwd(elu, aux[r]));
                        *cp = v;
                        csum += v;
                    } else {
                        acc_add(g, cp, v);
                    }
                }
            }
            if (EPI == 1 && g.colsum[z]) {
                csum += __shfl_xor(csum, 32);
                if (lk == 0) acc_add(g, &g.colsum[z][n], csum);
            }
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int n = n0 + wn + 32 * b + li;
        float csum = 0.f;
        const float bias = (EPI == 0 && g.bias[z] && n < N) ? g.bias[z][n] : 0.f;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (m < M && n < N) {
                    float v = acc[a][b][r];
                    if (EPI == 0) {
                        v += bias;
                        v = (ACT == 1 ? (v > 0.f ? v : __expf(v) - 1.0f) : ACT == 0 ? v : act_fwd(elu, v));
                        C[(size_t)m * ldc + n] = v;
                    } else if (EPI == 1) {
                        const float act = g.aux[z][(size_t)m * g.ldaux[z] + n];
                        v *= (ACT == 1 ? (act > 0.f ? 1.0f : act + 1.0f) : ACT == 0 ? 1.0f : act_bwd(elu, act));
                        C[(size_t)m * ldc + n] = v;
                        csum += v;
                    } else {
                        acc_add(g, &C[(size_t)m * ldc + n], v);
                    }
                }
            }
        if (EPI == 1 && g.colsum[z]) {
            csum += __shfl_xor(csum, 32);
            if (lk == 0 && n < N) acc_add(g, &g.colsum[z][n], csum);
        }
    }
}
// gemm_epilogue_act with the activation specialised on the workgroup-uniform code g.elu (EPI 2 has none).  A macro rather than a
// function: behind one more inlined call level hipcc orders the epilogue's loads and bounds tests differently.
#define GEMM_EPILOGUE(EPI, TM, TN, BM, BN, ...)                                                                                \
    do {                                                                                                                       \
        if (EPI == 2 || g.elu == 1) gemm_epilogue_act<EPI, TM, TN, BM, BN, 1>(__VA_ARGS__);                                    \
        else if (g.elu == 0) gemm_epilogue_act<EPI, TM, TN, BM, BN, 0>(__VA_ARGS__);                                           \
        else gemm_epilogue_act<EPI, TM, TN, BM, BN, -1>(__VA_ARGS__);                                                          \
    } while (0)

// Split-bf16 forward (EPI 0) and input gradient (EPI 1): WGM x WGN waves, each TM x TN tiles of 32x32.  B from fp32 B (B_PL 0) or
// from the weight planes (B_PL 1, 2: gemm_mainloop_x6).
template <bool A_RC, bool B_RC, int EPI, int TM, int TN, int WGM = 2, int WGN = 2, int B_PL = 0>
__global__ void __launch_bounds__(64 * WGM * WGN, WGM * WGN == 8 ? 4 : 2) k_gemm(GemmArgs g) {
    static_assert(EPI != 2, "weight gradients: k_gemm_dw_t");
    static_assert(B_PL == 0 || (B_PL == 1) == B_RC, "weight planes: [n][k] planes as the reduction-contiguous operand (1), the same "
                  "planes read along their rows through the transposing LDS read (2)");
    constexpr int BM = 32 * TM * WGM, BN = 32 * TN * WGN;
    GemmTiles t;
    if (!gemm_tiles<BM, BN>(g, t)) return;
    const int z = t.z, M = t.M, N = t.N;
    int tm, tn;
    xcd_tile((int)blockIdx.x, t.tiles_n, t.tiles_m, tm, tn);      // the column tiles of a row block share the A rows: one XCD
    const int m0 = tm * BM, n0 = tn * BN;
    const int k_begin = 0, k_end = t.K;
    const float *__restrict__ A = g.A[z];
    const float *__restrict__ B = g.B[z];
    const int lda = g.lda[z], ldb = g.ldb[z], ldc = g.ldc[z];
    // 16-byte path: aligned rows and a contiguous-dimension limit that no float4 straddles
    const bool a_vec = (lda & 3) == 0 && ((uintptr_t)A & 15) == 0 && (((A_RC ? k_end : M) & 3) == 0) && (A_RC ? k_end : M) >= 4;
    const bool b_vec = (ldb & 3) == 0 && ((uintptr_t)B & 15) == 0 && (((B_RC ? k_end : N) & 3) == 0) && (B_RC ? k_end : N) >= 4;

    constexpr int LDS_BYTES = 3 * (x6_plane_bytes<BM>() + (B_PL == 2 ? plt_plane_bytes<BN>() : x6_plane_bytes<BN>()));
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = (wave / WGN) * 32 * TM, wn = (wave % WGN) * 32 * TN;
    const int li = lane & 31, lk = lane >> 5;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // whole tile in range in all three dimensions (workgroup-uniform): staging without clamps and masks
    const bool full = a_vec && b_vec && m0 + BM <= M && n0 + BN <= N && ((k_end - k_begin) % BK) == 0;
    if (B_PL) {
        const bool fullp = a_vec && m0 + BM <= M && n0 + BN <= N && ((k_end - k_begin) % BK) == 0;
        if (fullp) gemm_mainloop_x6<A_RC, B_RC, TM, TN, WGM, WGN, true, true, B_PL>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds_raw, wm, wn, li, lk, acc, g.Bpl[z], g.pl_stride);
        else if (a_vec) gemm_mainloop_x6<A_RC, B_RC, TM, TN, WGM, WGN, true, false, B_PL>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds_raw, wm, wn, li, lk, acc, g.Bpl[z], g.pl_stride);
        else gemm_mainloop_x6<A_RC, B_RC, TM, TN, WGM, WGN, false, false, B_PL>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds_raw, wm, wn, li, lk, acc, g.Bpl[z], g.pl_stride);
    } else
    if (full) gemm_mainloop_x6<A_RC, B_RC, TM, TN, WGM, WGN, true, true>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds_raw, wm, wn, li, lk, acc);
    else if (a_vec && b_vec) gemm_mainloop_x6<A_RC, B_RC, TM, TN, WGM, WGN, true>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds_raw, wm, wn, li, lk, acc);
    else gemm_mainloop_x6<A_RC, B_RC, TM, TN, WGM, WGN, false>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds_raw, wm, wn, li, lk, acc);

    GEMM_EPILOGUE(EPI, TM, TN, BM, BN, g, z, M, N, m0, n0, wm, wn, li, lk, ldc, acc);
}

// The fp32-input MFMA reference (ppok_debug_set_x6(0)), what the tests compare the split-bf16 kernels against: gemm_mainloop with
// 64x64 tiles on 2x2 waves and one LDS buffer.  Its sums do not depend on the tile shape: every output adds the same MFMAs in
// the same k order.  EPI 2 splits the reduction over gridDim.y slices.
template <bool A_RC, bool B_RC, int EPI>
__global__ void __launch_bounds__(256, 1) k_gemm_ref(GemmArgs g) {
    constexpr int BM = 64, BN = 64;
    GemmTiles t;
    if (!gemm_tiles<BM, BN>(g, t)) return;
    const int z = t.z, M = t.M, N = t.N;
    const int m0 = (blockIdx.x / t.tiles_n) * BM, n0 = (blockIdx.x % t.tiles_n) * BN;
    int k_begin = 0, k_end = t.K;
    if (EPI == 2 && !k_slice(t.K, blockIdx.y, k_begin, k_end)) return;
    const float *__restrict__ A = g.A[z];
    const float *__restrict__ B = g.B[z];
    const int lda = g.lda[z], ldb = g.ldb[z];
    const bool a_vec = (lda & 3) == 0 && ((uintptr_t)A & 15) == 0 && (((A_RC ? k_end : M) & 3) == 0) && (A_RC ? k_end : M) >= 4;
    const bool b_vec = (ldb & 3) == 0 && ((uintptr_t)B & 15) == 0 && (((B_RC ? k_end : N) & 3) == 0) && (B_RC ? k_end : N) >= 4;
    __shared__ __attribute__((aligned(16))) float lds[tile_floats<A_RC, BM>() + tile_floats<B_RC, BN>()];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, li = lane & 31, lk = lane >> 5;
    f32x16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
    if (a_vec && b_vec) gemm_mainloop<A_RC, B_RC, 1, 1, true>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds, wm, wn, li, lk, acc);
    else gemm_mainloop<A_RC, B_RC, 1, 1, false>(A, B, lda, ldb, m0, n0, M, N, k_begin, k_end, lds, wm, wn, li, lk, acc);
    GEMM_EPILOGUE(EPI, 1, 1, BM, BN, g, z, M, N, m0, n0, wm, wn, li, lk, g.ldc[z], acc);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient dW[M][N] += A^T . B over a slice of the minibatch rows, A = dz [k][m], B = act [k][n], both with the
// REDUCTION index as the row index in memory.  Both k-tiles are staged the way they lie in HBM -- [32 k-rows][BM | BN columns],
// float4 along the rows, split into the three bf16 planes on the way (8-byte LDS stores, consecutive lanes on consecutive
// half-chunks) -- and every operand fragment (8 consecutive k of one column per lane) comes out of the transposing LDS read,
// as in the input-gradient kernel.  The k_gemm<false,false,2,...> path it replaces transposed while staging: 4-byte stores
// scattered over four physical rows per float4, 4-way bank conflicts, 2.7 us per k-tile with a CU to itself.
template <int ROWS, int NT>
__device__ __forceinline__ void stage_store_x6t(unsigned char *__restrict__ lds, const float4 (&regs)[ROWS * BK / 4 / NT], unsigned mask) {
    constexpr int NV = ROWS * BK / 4 / NT, PL = plt_plane_bytes<ROWS>();
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int idx = threadIdx.x + v * NT;
        const int c = idx & (ROWS / 4 - 1), r = idx / (ROWS / 4);          // float4 c of k-row r (stage_load<false,...> mapping)
        const bool in = (mask >> v) & 1u;
        const float x0 = in ? regs[v].x : 0.f, x1 = in ? regs[v].y : 0.f, x2 = in ? regs[v].z : 0.f, x3 = in ? regs[v].w : 0.f;
        uint32_t h0, m0, l0, h1, m1, l1;
        split2(x0, x1, h0, m0, l0);
        split2(x2, x3, h1, m1, l1);
        unsigned char *d = lds + plt_off<ROWS>(r, c >> 1) + 8 * (c & 1);
        *reinterpret_cast<uint2 *>(d) = make_uint2(h0, h1);
        *reinterpret_cast<uint2 *>(d + PL) = make_uint2(m0, m1);
        *reinterpret_cast<uint2 *>(d + 2 * PL) = make_uint2(l0, l1);
    }
}

// PD: k-tiles of global loads in flight per workgroup (register sets).  3 and 4 measured no faster for the first layer's thin
// gradient (42.8 / 56.9 vs 42.4 us: the fourth set costs a workgroup per CU) and slower for the 128 x 128 tiles (spills at 128 VGPRs);
// neither were 128 x 64 tiles or 96 reduction slices for that launch (profiles/r03_ab.txt).
template <int TM, int TN, int WGM, int WGN, int PD = 2>
__global__ void __launch_bounds__(64 * WGM * WGN, WGM * WGN == 8 ? 4 : 2) k_gemm_dw_t(GemmArgs g) {
    constexpr int BM = 32 * TM * WGM, BN = 32 * TN * WGN, NT = 64 * WGM * WGN;
    constexpr int APL = plt_plane_bytes<BM>(), BPL = plt_plane_bytes<BN>();
    constexpr int NVA = BM * BK / 4 / NT, NVB = BN * BK / 4 / NT;
    GemmTiles t;
    gemm_problem<BM, BN>(g, t);
    const int z = t.z, M = t.M, N = t.N;
    int slice, tile;                                               // the output tiles of one reduction slice share its rows: one XCD
    xcd_tile((int)(blockIdx.x + gridDim.x * blockIdx.y), (int)gridDim.x, (int)gridDim.y, slice, tile);
    if (tile >= t.tiles_n * t.tiles_m) return;                     // gridDim.x = the tiles of the launch's LARGEST problem
    const int m0 = (tile / t.tiles_n) * BM, n0 = (tile % t.tiles_n) * BN;
    int k_begin, k_end;
    if (!k_slice(t.K, slice, k_begin, k_end)) return;
    const float *__restrict__ A = g.A[z];
    const float *__restrict__ B = g.B[z];
    const int lda = g.lda[z], ldb = g.ldb[z], ldc = g.ldc[z];
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * (APL + BPL)];
    unsigned char *lds_b = lds + 3 * APL;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = (wave / WGN) * 32 * TM, wn = (wave % WGN) * 32 * TN;
    const int li = lane & 31, lk = lane >> 5;
    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // transposed-read bases (T10): group tg = lane >> 4 takes columns 16 (tg & 1) .. +15 and k-rows 8 (tg >> 1) + 4 h .. +3
    const int tg = (threadIdx.x >> 4) & 3, tq = (threadIdx.x >> 2) & 3, tp = threadIdx.x & 3;
    const unsigned char *fa[2], *fb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int lane_off = 64 * (4 * h + tq) + 16 * ((2 * (tg & 1) + (tp >> 1)) ^ (2 * (tg >> 1) + h)) + 8 * (tp & 1);
        fa[h] = lds + (BM / 32 * PLT_SUB) * (tg >> 1) + PLT_SUB * (wm / 32) + lane_off;
        fb[h] = lds_b + (BN / 32 * PLT_SUB) * (tg >> 1) + PLT_SUB * (wn / 32) + lane_off;
    }
    auto frag = [&](const unsigned char *const (&f)[2], int o) { return lds_read_tr_frag(f[0] + o, f[1] + o); };
    const bool a_vec = (lda & 3) == 0 && ((uintptr_t)A & 15) == 0 && (M & 3) == 0 && M >= 4;
    const bool b_vec = (ldb & 3) == 0 && ((uintptr_t)B & 15) == 0 && (N & 3) == 0 && N >= 4;
    // The whole k-loop once per load form (16-byte loads for both operands, or the element-wise fallback): with the choice as a
    // branch INSIDE the loop hipcc's s_waitcnt insertion lost track of the prefetched registers across the join -- in a
    // steady-state loop form (see gemm_mainloop_x6) the split read a register set with no vmcnt wait at all (wrong sums), in the
    // guarded form it waited for everything.
    auto run = [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        float4 ra[PD][NVA], rb[PD][NVB];
        unsigned ma[PD], mb[PD];
    #pragma unroll
        for (int d = 0; d < PD; ++d) { ma[d] = 0u; mb[d] = 0u; }
        auto load = [&](int k0, float4 (&xa)[NVA], float4 (&xb)[NVB], unsigned &xma, unsigned &xmb) {
            stage_load<false, BM, VEC, false, NT>(A, lda, m0, k0, M, k_end, xa, xma);
            stage_load<false, BN, VEC, false, NT>(B, ldb, n0, k0, N, k_end, xb, xmb);
        };
    #pragma unroll
        for (int d = 0; d < PD; ++d)
            if (d == 0 || k_begin + d * BK < k_end) load(k_begin + d * BK, ra[d], rb[d], ma[d], mb[d]);
        stage_store_x6t<BM, NT>(lds, ra[0], ma[0]);
        stage_store_x6t<BN, NT>(lds_b, rb[0], mb[0]);
        lds_barrier();
        // one k-tile (in LDS; its register set c is free): loads of tile + PD into set c, MFMAs, then the next tile (set n) to LDS
        auto body = [&](int k0, float4 (&ca)[NVA], float4 (&cb)[NVB], unsigned &cma, unsigned &cmb, float4 (&na)[NVA], float4 (&nb)[NVB],
                        unsigned &nma, unsigned &nmb) {
            if (k0 + PD * BK < k_end) load(k0 + PD * BK, ca, cb, cma, cmb);
    #pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
                bf16x8 av[TM][3], bv[TN][3];
    #pragma unroll
                for (int a = 0; a < TM; ++a)
    #pragma unroll
                    for (int p = 0; p < 3; ++p) av[a][p] = frag(fa, PLT_SUB * a + p * APL + (BM / 32 * PLT_SUB) * 2 * s);
    #pragma unroll
                for (int b = 0; b < TN; ++b)
    #pragma unroll
                    for (int p = 0; p < 3; ++p) bv[b][p] = frag(fb, PLT_SUB * b + p * BPL + (BN / 32 * PLT_SUB) * 2 * s);
    #pragma unroll
                for (int a = 0; a < TM; ++a)
    #pragma unroll
                    for (int b = 0; b < TN; ++b) acc[a][b] = mfma_x6(av[a], bv[b], acc[a][b]);
            }
            lds_barrier();
            if (k0 + BK < k_end) {
                stage_store_x6t<BM, NT>(lds, na, nma);
                stage_store_x6t<BN, NT>(lds_b, nb, nmb);
            }
            lds_barrier();
        };
        for (int k0 = k_begin; k0 < k_end; k0 += PD * BK) {
    #pragma unroll
            for (int d = 0; d < PD; ++d)
                if (d == 0 || k0 + d * BK < k_end)
                    body(k0 + d * BK, ra[d], rb[d], ma[d], mb[d], ra[(d + 1) % PD], rb[(d + 1) % PD], ma[(d + 1) % PD], mb[(d + 1) % PD]);
        }
    };
    if (a_vec && b_vec) run(std::true_type{});
    else run(std::false_type{});
    // nstore: columns past it are products with the zero pad columns of the padded observations -- computed, not stored
    GEMM_EPILOGUE(2, TM, TN, BM, BN, g, z, M, g.nstore[z] ? g.nstore[z] : N, m0, n0, wm, wn, li, lk, ldc, acc);
}

static int g_gemm_x6 = 1;     // split-bf16 kernels (fp32 accuracy on the bf16 matrix cores); 0 = k_gemm_ref, the reference of the tests
extern "C" void ppok_debug_set_x6(int v) { g_gemm_x6 = v != 0; }

#include "ppo_gemm_glds.h"

// Launch shape of every launcher: the largest problem of the launch, its 64 x 64 and 128 x 128 tile counts, and whether it takes
// the 128 x 128 tiles -- when those alone (times the reduction slices) fill the chip and both dimensions exceed one small tile.
struct GemmShape { int maxM, maxN; unsigned small_tiles, big_tiles; bool big; };
// What a launcher launched: the kernel (GK_*: the codes ppok_debug_gemm_args reports) and the reduction slices of the launch.
enum { GK_GEMM_SMALL = 1, GK_GEMM_BIG, GK_PL1_SMALL, GK_PL1_BIG, GK_PL2_SMALL, GK_PL2_BIG, GK_GLDS, GK_DW_SMALL, GK_DW_BIG, GK_REF };
struct GemmLaunch { int kernel, slices; };
static GemmShape gemm_shape(const GemmArgs &g, int nz, int splits) {
    GemmShape sh{0, 0, 0, 0, false};
    for (int z = 0; z < nz; ++z) { sh.maxM = g.M[z] > sh.maxM ? g.M[z] : sh.maxM; sh.maxN = g.N[z] > sh.maxN ? g.N[z] : sh.maxN; }
    const long big_tiles = (long)((sh.maxM + 127) / 128) * ((sh.maxN + 127) / 128);
    sh.small_tiles = (unsigned)(((sh.maxM + 63) / 64) * ((sh.maxN + 63) / 64));
    sh.big_tiles = (unsigned)big_tiles;
    sh.big = big_tiles * splits >= 192 && sh.maxN > 64 && sh.maxM > 64;
    return sh;
}

// Whether the weight planes can stand in for B: 16-byte aligned rows, and `chunked` -- the planes' dimension the staging reads in
// 16-byte pieces: K for the forward (reduction-contiguous planes), N for the input gradient (planes read along their rows) -- a
// whole number of 8-element chunks.
static bool planes_ok(const GemmArgs &g, int nz, int (GemmArgs::*chunked)[2]) {
    if (!g_gemm_x6) return false;
    for (int z = 0; z < nz; ++z) {
        const int d = (g.*chunked)[z];
        if (!g.Bpl[z] || (g.ldb[z] & 7) || (d & 7) || d < 8 || ((uintptr_t)g.Bpl[z] & 15) || (g.pl_stride & 7)) return false;
    }
    return true;
}

// forward (EPI 0) and input gradient (EPI 1) with B = pre-split weight planes: PL 1 reduction-contiguous, PL 2 read along their rows
template <int EPI, bool B_RC = true, int PL = 1>
static GemmLaunch launch_gemm_pl(const GemmArgs &g, int nz, hipStream_t s) {
    const GemmShape sh = gemm_shape(g, nz, 1);
    // LDS-DMA forward (ppo_gemm_glds.h): 40 KB workgroups, up to four per CU -- update -2.6 % (profiles/r04_ab.txt)
    if (EPI == 0 && sh.maxM > 64 && glds_ok(g, nz)) {
        dim3 grid((unsigned)(((sh.maxM + GLDS_BM - 1) / GLDS_BM) * (sh.maxN / GLDS_BN)), 1, nz);
        hipLaunchKernelGGL(k_gemm_glds, grid, dim3(256), 0, s, g);
        return {GK_GLDS, 1};
    }
    if (sh.big) hipLaunchKernelGGL((k_gemm<true, B_RC, EPI, 2, 1, 2, 4, PL>), dim3(sh.big_tiles, 1, nz), dim3(512), 0, s, g);
    else hipLaunchKernelGGL((k_gemm<true, B_RC, EPI, 1, 1, 2, 2, PL>), dim3(sh.small_tiles, 1, nz), dim3(256), 0, s, g);
    return {(PL == 1 ? GK_PL1_SMALL : GK_PL2_SMALL) + (sh.big ? 1 : 0), 1};
}

// fp32 operands in memory, split-bf16: 128x128 tiles on 8 waves (2x4, each 64x32); small problems (rollout forward on 4096 rows,
// heads) use 64x64 tiles on 4 waves to fill more CUs
template <bool A_RC, bool B_RC, int EPI>
static GemmLaunch launch_gemm(const GemmArgs &g, int nz, hipStream_t s) {
    const GemmShape sh = gemm_shape(g, nz, 1);
    if (sh.big) hipLaunchKernelGGL((k_gemm<A_RC, B_RC, EPI, 2, 1, 2, 4>), dim3(sh.big_tiles, 1, nz), dim3(512), 0, s, g);
    else hipLaunchKernelGGL((k_gemm<A_RC, B_RC, EPI, 1, 1>), dim3(sh.small_tiles, 1, nz), dim3(256), 0, s, g);
    return {sh.big ? GK_GEMM_BIG : GK_GEMM_SMALL, 1};
}
template <bool A_RC, bool B_RC, int EPI>
static GemmLaunch launch_gemm_ref(const GemmArgs &g, int nz, int splits, hipStream_t s) {
    hipLaunchKernelGGL((k_gemm_ref<A_RC, B_RC, EPI>), dim3(gemm_shape(g, nz, splits).small_tiles, splits, nz), dim3(256), 0, s, g);
    return {GK_REF, splits};
}

// weight gradients over `splits` reduction slices: k_gemm_dw_t on the split-bf16 path, the fp32-input reference otherwise
static GemmLaunch launch_gemm_dw(const GemmArgs &g, int nz, int splits, hipStream_t s) {
    if (!g_gemm_x6) {                          // the reference's store guard is its N: compute the true width only
        GemmArgs gt = g;
        for (int z = 0; z < nz; ++z) if (g.nstore[z]) gt.N[z] = g.nstore[z];
        return launch_gemm_ref<false, false, 2>(gt, nz, splits, s);
    }
    const GemmShape sh = gemm_shape(g, nz, splits);
    if (sh.big) hipLaunchKernelGGL((k_gemm_dw_t<2, 1, 2, 4>), dim3(sh.big_tiles, splits, nz), dim3(512), 0, s, g);
    else hipLaunchKernelGGL((k_gemm_dw_t<1, 1, 2, 2>), dim3(sh.small_tiles, splits, nz), dim3(256), 0, s, g);
    return {sh.big ? GK_DW_BIG : GK_DW_SMALL, splits};
}
// Reduction slices of a weight-gradient launch: about 384 workgroups per net over (output tiles x slices), counted with the tile
// each problem alone would get (128 x 128 when both dimensions exceed 64) -- swept 64..384 inside the update (side stream beside
// the input-gradient chain): 0.637 / 0.585 / 0.597 / 0.574 / 0.560 ms per minibatch at 64 / 128 / 192 / 256 / 384.  At least 256
// rows per slice, so the split-K float atomics (slices x output floats) stay well below the MFMA time, and from 8 slices on whole
// groups of 8: one slice per XCD (xcd_tile).
static int dw_splits(const GemmArgs &g, int nz) {
    long tiles = 0;
    int rows = 0;
    for (int z = 0; z < nz; ++z) {
        const int tile = (g.M[z] > 64 && g.N[z] > 64) ? 128 : 64;
        const long t = (long)((g.M[z] + tile - 1) / tile) * ((g.N[z] + tile - 1) / tile);
        tiles = t > tiles ? t : tiles;
        rows = g.K[z] > rows ? g.K[z] : rows;
    }
    int splits = (int)((384 + tiles - 1) / tiles);
    const int max_splits = rows / 256 > 0 ? rows / 256 : 1;
    if (splits > max_splits) splits = max_splits;
    if (splits >= 8) splits &= ~7;
    if (splits < 1) splits = 1;
    return splits;
}

// g->Bpl (optional): bf16 planes of W [n_out][n_in] kept by the optimiser step; the caller passes both B (fp32 W) and Bpl,
// whichever path is eligible is taken.  Forward: the planes are the reduction-contiguous operand.  Input gradient: the
// SAME planes, reduced over their rows through the transposing LDS read (no second image of W^T to keep current).
static GemmLaunch gemm_fwd(const GemmArgs *g, int nz, hipStream_t s) {
    GemmArgs gp = *g;                          // the plane path's view of the reduction dimension (padded first layer, ppo_device.h)
    for (int z = 0; z < nz; ++z) {
        if (g->Kpl[z]) gp.K[z] = g->Kpl[z];
        if (g->ldbpl[z]) gp.ldb[z] = g->ldbpl[z];
    }
    if (planes_ok(gp, nz, &GemmArgs::K)) return launch_gemm_pl<0>(gp, nz, s);
    if (g_gemm_x6) return launch_gemm<true, true, 0>(*g, nz, s);
    return launch_gemm_ref<true, true, 0>(*g, nz, 1, s);
}
static GemmLaunch gemm_dx(const GemmArgs *g, int nz, hipStream_t s) {
    if (planes_ok(*g, nz, &GemmArgs::N)) return launch_gemm_pl<1, false, 2>(*g, nz, s);
    if (g_gemm_x6) return launch_gemm<true, false, 1>(*g, nz, s);
    return launch_gemm_ref<true, false, 1>(*g, nz, 1, s);
}
// Host-side trace of what the three entry points launched, for tests/test_hip_ppo_update.py: per launch {kind 0 / 1 / 2 = forward / input
// gradient / weight gradient, nz, kernel (GK_*), reduction slices} as the launcher itself returned them, in launch order.  The first
// GEMM_TRACE_CAP launches since the last read are kept, later ones dropped; ppok_debug_gemm_trace copies up to `cap` entries (4 ints
// each) to `out`, clears the trace and returns how many it held.  Host code only; not synchronised (one learner per process in the tests).
#define GEMM_TRACE_CAP 64
static int g_gemm_trace[GEMM_TRACE_CAP][4];
static int g_gemm_trace_n = 0;
static void gemm_trace(int kind, int nz, const GemmLaunch &l) {
    if (g_gemm_trace_n < 0 || g_gemm_trace_n >= GEMM_TRACE_CAP) return;
    int *e = g_gemm_trace[g_gemm_trace_n++];
    e[0] = kind; e[1] = nz; e[2] = l.kernel; e[3] = l.slices;
}
extern "C" int ppok_debug_gemm_trace(int *out, int cap) {
    const int n = g_gemm_trace_n < GEMM_TRACE_CAP ? g_gemm_trace_n : GEMM_TRACE_CAP;
    for (int k = 0; out && k < n && k < cap; ++k) memcpy(out + 4 * k, g_gemm_trace[k], sizeof(g_gemm_trace[k]));
    g_gemm_trace_n = 0;
    return n;
}
extern "C" void ppok_gemm_fwd(const GemmArgs *g, int nz, hipStream_t s) { gemm_trace(0, nz, gemm_fwd(g, nz, s)); }
extern "C" void ppok_gemm_dx(const GemmArgs *g, int nz, hipStream_t s) { gemm_trace(1, nz, gemm_dx(g, nz, s)); }
extern "C" void ppok_gemm_dw(const GemmArgs *g, int nz, hipStream_t s) { gemm_trace(2, nz, launch_gemm_dw(*g, nz, dw_splits(*g, nz), s)); }

// Debug entry that launches what the product launches (tests/test_hip_ppo_gemm.py): kind 0 / 1 / 2 = forward / input gradient / weight
// gradient on the caller's GemmArgs as it stands -- nz problems, every field as given.  kind 2: splits = 0 takes the product's own
// dw_splits, a positive value forces that many reduction slices.  info[0] = the kernel the launcher chose (GK_*), info[1] = the
// reduction slices, both as reported by the launcher itself.  Returns 0, or -1 for an unknown kind / nz.
extern "C" int ppok_debug_gemm_args(const GemmArgs *g, int nz, int kind, int splits, void *stream, int *info) {
    if (!g || nz < 1 || nz > 2 || kind < 0 || kind > 2 || splits < 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    const GemmLaunch l = kind == 0 ? gemm_fwd(g, nz, s) : kind == 1 ? gemm_dx(g, nz, s) : launch_gemm_dw(*g, nz, splits ? splits : dw_splits(*g, nz), s);
    if (info) { info[0] = l.kernel; info[1] = l.slices; }
    return 0;
}
extern "C" int ppok_debug_gemm_args_size() { return (int)sizeof(GemmArgs); }

// Debug / microbenchmark entry (tools/gemm_bench.py): C[M,N] = A . B with the layouts of `mode`
// (0: A[m][k] B[n][k] forward; 1: A[m][k] B[k][n] input-gradient; 2: A[k][m] B[k][n] weight-gradient over `splits` reduction
// slices, C zeroed by caller).
extern "C" void ppok_debug_gemm(const float *A, const float *B, float *C, int M, int N, int K, int mode, int splits, void *stream) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A[0] = A; g.B[0] = B; g.C[0] = C; g.M[0] = M; g.N[0] = N; g.K[0] = K; g.ldc[0] = N;
    if (mode == 0) { g.lda[0] = K; g.ldb[0] = K; ppok_gemm_fwd(&g, 1, (hipStream_t)stream); }                 // no planes: k_gemm
    else if (mode == 1) { g.lda[0] = K; g.ldb[0] = N; g.aux[0] = C; g.ldaux[0] = N; g.elu = 1; ppok_gemm_dx(&g, 1, (hipStream_t)stream); }
    else { g.lda[0] = M; g.ldb[0] = N; launch_gemm_dw(g, 1, splits, (hipStream_t)stream); }
}

// Debug entry for the weight-plane operand paths: W [rows][cols] fp32 is split into its three bf16 planes (caller-provided
// scratch of 3 x plane_stride uint16, plane_stride = rows * cols rounded up to 8), then
//   mode 0: C[M][rows] = A[M][cols] . W^T   (forward: planes as the reduction-contiguous operand)
//   mode 1: C[M][cols] = A[M][rows] . W     (input gradient: the same planes through the transposing LDS read)
__global__ void __launch_bounds__(256) k_debug_split(const float *__restrict__ W, uint16_t *__restrict__ pl, int64_t n, int64_t stride) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        uint32_t h, m, l;
        split2(W[k], 0.f, h, m, l);
        pl[k] = (uint16_t)h; pl[stride + k] = (uint16_t)m; pl[2 * stride + k] = (uint16_t)l;
    }
}
extern "C" int ppok_debug_gemm_planes(const float *A, const float *W, float *C, uint16_t *planes, int64_t plane_stride, int M, int rows,
                                      int cols, int mode, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_debug_split, dim3(256), dim3(256), 0, s, W, planes, (int64_t)rows * cols, plane_stride);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A[0] = A; g.B[0] = W; g.C[0] = C; g.M[0] = M; g.Bpl[0] = planes; g.pl_stride = plane_stride; g.ldb[0] = cols;
    if (mode == 0) {
        g.N[0] = rows; g.K[0] = cols; g.lda[0] = cols; g.ldc[0] = rows;
        if (!planes_ok(g, 1, &GemmArgs::K)) return -1;
        launch_gemm_pl<0>(g, 1, s);
    } else {
        g.N[0] = cols; g.K[0] = rows; g.lda[0] = rows; g.ldc[0] = cols; g.aux[0] = C; g.ldaux[0] = cols; g.elu = 0;
        if (!planes_ok(g, 1, &GemmArgs::N)) return -1;
        launch_gemm_pl<1, false, 2>(g, 1, s);
    }
    return 0;
}
