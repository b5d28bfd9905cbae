// Tube-model trainer kernels (deep_tube_learning's train_tube.py on the device).
//
// Model: the reference MLP -- Linear, activation, repeated num_layers times, then a final Linear.  One training step is two launches
// (for a sweep of K models of one shape the same two, k_tube_rows_sweep / k_tube_adam_sweep, with the members along grid y):
//   k_tube_rows<true>  every workgroup owns LG_TUBE_ROWS rows of the minibatch: gathers them (through the epoch permutation or an
//                      explicit row list; for the horizon dataset it draws the window start and builds input / target in place),
//                      runs the forward pass with every hidden activation kept in LDS, the loss and its gradient, the backward
//                      pass, and writes its partial weight / bias gradients and loss sum to its own slab row;
//   k_tube_adam        sums the slab rows in workgroup order (fixed order: bit-reproducible without atomics), applies
//                      torch.optim.Adam (defaults) at the StepLR rate of the step, and logs loss, lr and gradient norm on the device.
// A level-conditioned model (lg_tube_cfg.level_input) runs the same two launches with the tile's LEVEL flag
// set -- on flat rows and on horizon windows alike (section 10.8) -- and k_tube_predict_levels evaluates many levels of a row, or
// of a window, in one launch.
// Plain fp32 FMA over LDS tiles: at 16..128 units the matrices are far too small for MFMA to matter.
#include "tube_mlp.h"

constexpr int R = LG_TUBE_ROWS, NT = LG_TUBE_THREADS, RB = LG_TUBE_RB;   // the tile, under the names the kernels use

// the pinball residual of ScalarTubeLoss / VectorTubeLoss: l = alpha r where r = w - fw > 0, else (1 - alpha) |r|; dl/dfw
// (torch.where routes the gradient to the branch taken; |r|'s gradient at r = 0 is 0)
__device__ __forceinline__ float tube_pinball(float alpha, float w, float fw, float *dl) {
    const float r = w - fw;
    if (r > 0.f) { *dl = -alpha; return alpha * r; }
    *dl = r < 0.f ? (1.f - alpha) : 0.f;
    return (1.f - alpha) * fabsf(r);
}
// HuberLoss(delta)(l, 0) of one element and its derivative in l (|l| = delta takes the linear branch, as torch does)
__device__ __forceinline__ float tube_huber(float delta, float l, float *dh) {
    const float a = fabsf(l);
    *dh = fminf(fmaxf(l, -delta), delta);
    return a < delta ? 0.5f * a * a : delta * (a - 0.5f * delta);
}

// Window start of row `pos` of a draw: uniform over [H_rev, T - H_fwd - 1), Philox keyed by (seed, draw key, row position).
template <class Dev>                    // TubeDev, or a sweep kernel's TubeDevView
__device__ __forceinline__ int tube_window(const Dev &D, uint64_t key, int64_t pos) {
    uint32_t c[4] = {(uint32_t)pos, (uint32_t)key, (uint32_t)(key >> 32), 0x7ab3e5u ^ (uint32_t)(pos >> 32)};
    philox4x32((uint32_t)D.seed, (uint32_t)(D.seed >> 32), c);
    const uint32_t range = (uint32_t)(D.T - D.H_fwd - 1 - D.H_rev);
    return D.H_rev + (int)(((uint64_t)c[0] * range) >> 32);
}

// Level of row `pos` of a draw on a level-conditioned model: uniform over [level_lo, level_hi), from the same Philox key as
// tube_window -- (seed, draw key, row position) -- under a domain constant of its own, so the two draws never coincide.  It depends
// on (seed, key, pos) alone: not on the tile, the batch size or the sweep.  The one fp32 formula: u = 24 bits / 2^24, fmaf(hi - lo, u, lo).
template <class Dev>
__device__ __forceinline__ float tube_level(const Dev &D, uint64_t key, int64_t pos) {
    uint32_t c[4] = {(uint32_t)pos, (uint32_t)key, (uint32_t)(key >> 32), 0x1e7e1c0du ^ (uint32_t)(pos >> 32)};
    philox4x32((uint32_t)D.seed, (uint32_t)(D.seed >> 32), c);
    const float u = (float)(c[0] >> 8) * (1.f / 16777216.f);
    return fmaf(D.level_hi - D.level_lo, u, D.level_lo);
}

// One tile of rows: gather, forward, loss (+ backward into the slab row when TRAIN, eval partial sums otherwise).
// rows: row ids of the batch (position base + r); count: rows in the batch; norm: the loss's divisor (elements or rows).
// The body is tube_rows_tile.inl, included by k_tube_rows (D in the kernel arguments) and k_tube_rows_sweep (D in the member array):
// as a device function it inlined into k_tube_rows with a different schedule, and the single kernel is to stay as it was.
// LEVEL: the level-conditioned tile (tube_rows_tile.inl); `level` >= 0 fixes every row's level, < 0 draws it.
template <bool TRAIN, bool LEVEL>
__global__ void __launch_bounds__(NT) k_tube_rows(TubeDev D, TubeSplit S, const int32_t *rows, int64_t count, uint64_t key, float norm,
                                                  float level) {
#include "tube_rows_tile.inl"
}

// Member blockIdx.y of a sweep's device array.  The array is read-only for the whole launch, and it is read through the constant
// address space: the loads are scalar, and the compiler takes the pointers stored in it for global ones (global_load /
// global_store), where pointers loaded from global memory are generic and every weight load and slab store would be a flat access.
#define TUBE_CONST __attribute__((address_space(4)))
__device__ __forceinline__ const TUBE_CONST TubeMember &tube_member(const TubeMember *M) { return ((const TUBE_CONST TubeMember *)M)[blockIdx.y]; }

// What k_tube_rows_sweep / k_tube_adam_sweep hold of their member's TubeDev, under TubeDev's field names.  The single kernels get
// their TubeDev in the kernel arguments: loads the compiler knows to be invariant, so a field read inside a loop (D.horizon in the
// gather, D.act after every dot product, D.layers per parameter of the Adam loop) costs nothing there.  Read from the member array
// in place, the same field was loaded again in every iteration, with a wait that also drains the loop's LDS reads.  So every scalar
// and pointer is read once, at kernel entry, into registers; the per-layer tables stay in the array and are read per layer.
struct TubeDevView {
    int in_dim, out_dim, units, layers, act, loss, horizon;
    int H_fwd, H_rev, T, nz, m;
    float alpha, delta, sp_beta;
    uint64_t seed;
    int64_t num_params, slab_ld;
    const TUBE_CONST int64_t *off_w, *off_b;
    const TUBE_CONST int *din, *dout;
    float *params, *wt, *grads, *adam_m, *adam_v, *slab, *evpart, *normpart;
    uint32_t *done_ctr;
    float *log, *eval;
    int32_t *starts, *perm;
    int64_t log_cap;
    float level_lo, level_hi;
    float *levels;
    __device__ __forceinline__ TubeDevView(const TUBE_CONST TubeDev &d)
        : in_dim(d.in_dim), out_dim(d.out_dim), units(d.units), layers(d.layers), act(d.act), loss(d.loss), horizon(d.horizon),
          H_fwd(d.H_fwd), H_rev(d.H_rev), T(d.T), nz(d.nz), m(d.m), alpha(d.alpha), delta(d.delta), sp_beta(d.sp_beta), seed(d.seed),
          num_params(d.num_params), slab_ld(d.slab_ld), off_w(d.off_w), off_b(d.off_b), din(d.din), dout(d.dout), params(d.params),
          wt(d.wt), grads(d.grads), adam_m(d.adam_m), adam_v(d.adam_v), slab(d.slab), evpart(d.evpart), normpart(d.normpart),
          done_ctr(d.done_ctr), log(d.log), eval(d.eval), starts(d.starts), perm(d.perm), log_cap(d.log_cap), level_lo(d.level_lo),
          level_hi(d.level_hi), levels(d.levels) {}
};

// The same tile for member blockIdx.y of a sweep (grid = (tiles, K)).  rows: a row list shared by all members, or null: the
// member's own epoch permutation from position pos.
template <bool TRAIN, bool LEVEL>
__global__ void __launch_bounds__(NT) k_tube_rows_sweep(const TubeMember *__restrict__ M, TubeSplit S, const int32_t *rows, int64_t pos,
                                                        int64_t count, uint64_t key, float norm, float level) {
    const TubeDevView D(tube_member(M).dev);
    if (!rows) rows = D.perm + pos;
#include "tube_rows_tile.inl"
}

// transposed copy of every weight matrix (after the host wrote params)
__global__ void k_tube_wt(TubeDev D) {
    for (int li = 0; li <= D.layers; ++li) {
        const int K = D.din[li], N = D.dout[li];
        for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < N * K; e += gridDim.x * blockDim.x) {
            const int j = e / K, k = e - j * K;
            D.wt[D.off_w[li] + (int64_t)k * N + j] = D.params[D.off_w[li] + e];
        }
    }
}

// Reduce the nwg slab rows in order, torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no weight decay) at StepLR's rate,
// log [loss, lr after the step, grad_norm, rows] at slot (t - 1) % log_cap.  t: Adam's step count after this step (>= 1).
// The body is tube_adam_block.inl, for the same reason as tube_rows_tile.inl.
__global__ void __launch_bounds__(256) k_tube_adam(TubeDev D, int nwg, int64_t t, double lr0, double gamma, int64_t step_size,
                                                   float norm, int64_t rows) {
#include "tube_adam_block.inl"
}

// member blockIdx.y of a sweep: its own slab, moments, rate schedule, counter and log (grid = (blocks, K))
__global__ void __launch_bounds__(256) k_tube_adam_sweep(const TubeMember *__restrict__ M, int nwg, int64_t t, float norm, int64_t rows) {
    const TUBE_CONST TubeMember &m = tube_member(M);
    const TubeDevView D(m.dev);
    const double lr0 = m.lr0, gamma = m.gamma;
    const int64_t step_size = m.step_size;
#include "tube_adam_block.inl"
}

// the eval's per-workgroup sums, in workgroup order
__device__ __forceinline__ void tube_eval_finish_block(const TubeDev &D, int nwg, float norm, float elems) {
    __shared__ float red[4][256];
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int w = threadIdx.x; w < nwg; w += 256)
        for (int q = 0; q < 4; ++q) a[q] += D.evpart[(size_t)w * 4 + q];
    for (int q = 0; q < 4; ++q) red[q][threadIdx.x] = a[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int q = 0; q < 4; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        D.eval[0] = red[0][0] / norm;
        D.eval[1] = red[1][0] / elems;
        D.eval[2] = red[2][0] / red[1][0];            // torch: mean of an empty selection is nan
        D.eval[3] = red[3][0];
    }
}

__global__ void __launch_bounds__(256) k_tube_eval_finish(TubeDev D, int nwg, float norm, float elems) {
    tube_eval_finish_block(D, nwg, norm, elems);
}

__global__ void __launch_bounds__(256) k_tube_eval_finish_sweep(const TubeMember *__restrict__ M, int nwg, float norm, float elems) {
    tube_eval_finish_block((const TubeDev &)tube_member(M).dev, nwg, norm, elems);
}

__device__ __forceinline__ void tube_perm_entry(const TubeDev &D, int n, int half_bits, uint64_t epoch) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    D.perm[i] = (int32_t)feistel_perm(D.seed, epoch ^ 0x7475626500000000ull, n, half_bits, (uint32_t)i);
}

__global__ void __launch_bounds__(256) k_tube_perm(TubeDev D, int n, int half_bits, uint64_t epoch) { tube_perm_entry(D, n, half_bits, epoch); }

__global__ void __launch_bounds__(256) k_tube_perm_sweep(const TubeMember *__restrict__ M, int n, int half_bits, uint64_t epoch) {
    tube_perm_entry((const TubeDev &)tube_member(M).dev, n, half_bits, epoch);
}

__global__ void k_tube_iota(int32_t *p, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = (int32_t)i;
}

// ------------------------------------------------------------------ inference: predict and the closed-loop roll-out
// out[i] = MLP(item i).  Flat: item i = x[rows ? rows[i] : i].  Horizon: the ScalarHorizonTubeDataset item at (env[i], start[i])
// of the arrays in G (the caller guarantees H_rev <= start and start + H_fwd <= T).  No loss, no slab; weights through wt.
struct TubeGather {
    const float *x, *y, *v;             // flat: x (n, in).  horizon: w (n, T), z (n, T, nz), v (n, T, m)
    const int32_t *rows, *env, *start;
    int T, nz, m;
};
// element c of the window item at (s, t0) of w, z, v: [w[t0-Hr : t0], z[t0], v[t0-Hr : ..]]
__device__ __forceinline__ float tube_window_item(const TubeGather &G, int Hr, int64_t s, int t0, int c) {
    if (c < Hr) return G.x[s * G.T + t0 - Hr + c];
    if (c < Hr + G.nz) return G.y[(s * G.T + t0) * G.nz + (c - Hr)];
    const int q = c - Hr - G.nz, tt = q / G.m;
    return G.v[(s * G.T + t0 - Hr + tt) * G.m + (q - tt * G.m)];
}

__global__ void __launch_bounds__(NT) k_tube_predict(TubeDev D, TubeGather G, int64_t count, float *o) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, I = D.in_dim, O = D.out_dim, U = D.units, L = D.layers;
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds, *H0 = X + R * I, *H1 = H0 + R * U;
    for (int e = tid; e < R * I; e += NT) {
        const int r = e / I, c = e - r * I;
        float x = 0.f;
        if (r < nr) {
            if (!D.horizon) {
                const int64_t s = G.rows ? (int64_t)G.rows[base + r] : base + r;
                x = G.x[s * I + c];
            } else {
                x = tube_window_item(G, D.H_rev, G.env[base + r], G.start[base + r], c);
            }
        }
        X[e] = x;
    }
    __syncthreads();
    const float *in = tube_hidden<R, RB, NT>(tid, D, X, D.wt, D.params, H0, H1);
    tube_layer<R, RB, NT, true>(tid, D.din[L], O, in, D.wt + D.off_w[L], D.params + D.off_b[L], D.act, D.sp_beta, nullptr, o + base * O, O, nr);
}

// out[i][l] = MLP([x row of item i, levels[l]]) for a level-conditioned model: R rows per workgroup, gathered as in k_tube_predict
// from x (n, I - 1) -- or, WINDOW, as k_tube_predict's horizon branch gathers the item at (env[i], start[i]) of w, z, v: the I - 1
// shared columns [w[t0-H_rev : t0], z[t0], v[t0-H_rev : t0+H_fwd]] (k_tube_predict_windows_levels is that instantiation).
// The first layer is split: per (row, unit) the chain over the I - 1 shared columns -- acc = 0, fmaf over k
// ascending, tube_layer's order -- is computed once into A; per level the unit is finished with the chain's last link
// fmaf(level, w[I-1][j], acc), the bias and the activation, and the remaining layers run through tube_layer.  The level is the
// last k of the first layer, so every out[i][l] equals k_tube_predict on the row with the level appended, bit for bit.
// Dynamic LDS: X (R, I - 1), A (R, U), H0, H1 (R, U).  o: (count, n_levels, O).
template <bool WINDOW>
__global__ void __launch_bounds__(NT) k_tube_predict_levels(TubeDev D, TubeGather G, int64_t count, const float *levels, int n_levels,
                                                            float *o) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, I = D.in_dim, Ix = I - 1, O = D.out_dim, U = D.units, L = D.layers;
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds, *A = X + R * Ix, *H0 = A + R * U, *H1 = H0 + R * U;
    for (int e = tid; e < R * Ix; e += NT) {
        const int r = e / Ix, c = e - r * Ix;
        float x = 0.f;
        if (r < nr) {
            if (!WINDOW) {
                const int64_t s = G.rows ? (int64_t)G.rows[base + r] : base + r;
                x = G.x[s * Ix + c];
            } else {
                x = tube_window_item(G, D.H_rev, G.env[base + r], G.start[base + r], c);
            }
        }
        X[e] = x;
    }
    __syncthreads();
    const float *w0 = D.wt + D.off_w[0], *b0 = D.params + D.off_b[0];
    for (int e = tid; e < U * (R / RB); e += NT) {
        const int j = e % U, r0 = (e / U) * RB;
        float acc[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) acc[q] = 0.f;
#pragma unroll 8
        for (int k = 0; k < Ix; ++k) {
            const float wv = w0[k * U + j];
#pragma unroll
            for (int q = 0; q < RB; ++q) acc[q] = fmaf(X[(r0 + q) * Ix + k], wv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) A[(r0 + q) * U + j] = acc[q];
    }
    __syncthreads();
    for (int l = 0; l < n_levels; ++l) {
        const float lv = levels[l];
        for (int e = tid; e < R * U; e += NT) {
            const int j = e % U;
            const float z = fmaf(lv, w0[Ix * U + j], A[e]) + b0[j];
            H0[e] = tube_act(D.act, z, D.sp_beta);
        }
        __syncthreads();
        const float *in = H0;
        int64_t ow = D.off_b[0] + U;    // off_w[1]; the hidden layers are U x U and packed weight, bias, weight, ... (dev_init)
        for (int li = 1; li < L; ++li) {
            float *out = li & 1 ? H1 : H0;
            tube_layer<R, RB, NT, false>(tid, U, U, in, D.wt + ow, D.params + ow + U * U, D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
            ow += U * U + U;
        }
        tube_layer<R, RB, NT, true>(tid, U, O, in, D.wt + ow, D.params + ow + U * O, D.act, D.sp_beta, nullptr,
                                    o + (base * n_levels + l) * O, (int64_t)n_levels * O, nr);
        __syncthreads();                // the next level rewrites H0, which the last layer may still read
    }
}

// Closed loop over time: a workgroup owns RT sequences and walks t = 0..T-1 itself; the carried output of the tile stays in LDS.
// Step t: X = x[s, t] with its leading fb columns replaced by the previous output unless t == 0 or reseed[s, t]; forward; store.
// The teacher row and the reseed flag of step t + 1 are loaded into registers before step t's layers run, so their latency
// hides behind the chain.  WLDS: the transposed weights and the biases are staged to LDS once (params' own offsets).
#define TUBE_RO_PRE 16                  // teacher elements a thread holds for the next step: RT * LG_TUBE_MAX_IN / NT_ at most
template <int RT, int NT_, bool WLDS>
__global__ void __launch_bounds__(NT_) k_tube_rollout(TubeDev D, const float *x, int64_t n_seq, int T, int fb, const uint8_t *reseed,
                                                      float *o) {
    constexpr int RB_ = RT < 4 ? RT : 4;
    static_assert(RT * LG_TUBE_MAX_IN <= TUBE_RO_PRE * NT_ && RT <= NT_, "tile shape");
    extern __shared__ float lds[];
    const int tid = threadIdx.x, I = D.in_dim, O = D.out_dim, U = D.units, L = D.layers;
    const int64_t base = (int64_t)blockIdx.x * RT;
    const int nr = (int)(n_seq - base < RT ? n_seq - base : RT);
    float *W = lds;
    float *X = W + (WLDS ? D.num_params : 0), *H0 = X + RT * I, *H1 = H0 + RT * U, *F = H1 + RT * U;
    int *fresh = (int *)(F + RT * O);   // (RT) 1: the row takes the teacher's columns this step
    if (WLDS) {
        for (int64_t p = tid; p < D.num_params; p += NT_) W[p] = D.wt[p];
        __syncthreads();
        for (int li = 0; li <= L; ++li)
            for (int j = tid; j < D.dout[li]; j += NT_) W[D.off_b[li] + j] = D.params[D.off_b[li] + j];
    }
    const float *wsrc = WLDS ? W : D.wt, *bsrc = WLDS ? W : D.params;
    const int nq = (RT * I + NT_ - 1) / NT_;
    // element e = tid + q NT_ of the (RT, I) tile: its offset in x at t = 0 and, for a fed-back column, row * 64 + column (else -1).
    // Elements past the tile repeat its last one and rows past the batch read sequence n_seq - 1; neither is stored.
    int64_t poff[TUBE_RO_PRE];
    int pfb[TUBE_RO_PRE];
    float pre[TUBE_RO_PRE];
    int pfresh = 1;
#pragma unroll
    for (int q = 0; q < TUBE_RO_PRE; ++q) {
        int e = tid + q * NT_;
        const bool live = e < RT * I;
        e = live ? e : RT * I - 1;
        const int r = e / I, c = e - r * I;
        poff[q] = (r < nr ? base + r : n_seq - 1) * T * I + c;
        pfb[q] = live ? (c < fb ? r * 64 + c : -1) : -2;
    }
    auto fetch = [&](int t) {
#pragma unroll
        for (int q = 0; q < TUBE_RO_PRE; ++q)
            if (q < nq) pre[q] = x[poff[q] + (int64_t)t * I];
        if (tid < RT) pfresh = reseed && tid < nr && reseed[(base + tid) * T + t];
    };
    fetch(0);
    if (tid < RT) fresh[tid] = 1;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int q = 0; q < TUBE_RO_PRE; ++q) {
            if (q < nq && pfb[q] != -2) {
                const int fbi = pfb[q];
                X[tid + q * NT_] = fbi >= 0 && !fresh[fbi >> 6] ? F[(fbi >> 6) * O + (fbi & 63)] : pre[q];
            }
        }
        if (t + 1 < T) fetch(t + 1);
        __syncthreads();
        const float *in = X;
        for (int li = 0; li < L; ++li) {
            float *out = li & 1 ? H1 : H0;
            tube_layer<RT, RB_, NT_, false>(tid, D.din[li], U, in, wsrc + D.off_w[li], bsrc + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
        }
        tube_layer<RT, RB_, NT_, true>(tid, D.din[L], O, in, wsrc + D.off_w[L], bsrc + D.off_b[L], D.act, D.sp_beta, F,
                                       o + (base * T + t) * O, (int64_t)T * O, nr);
        if (tid < RT) fresh[tid] = pfresh;
        __syncthreads();
    }
}

// The closed loop of a windowed model: the input row is `taps` blocks of `stride` columns, block i the
// dataset row delayed by i * dN steps, and the leading fb columns of EVERY block are fed back -- block i takes out[s, t-1-i*dN]
// where that step lies after the row's last seed (t == 0 or reseed[s, t']), the teacher's column otherwise.  k_tube_rollout's
// shapes and step; added to it are a ring of the tile's own last depth = (taps-1) * dN + 1 outputs (fb floats each) per row and
// a per-row count of the steps since the seed, both in LDS.  The ring slot of out[t-1] is written from F during step t's input
// build; the delayed taps read slots of lag >= 1 in the same phase, which are other slots because lag < depth.  Tap 0 reads F.
// A fed-back element is lag << 10 | row << 6 | column (lag < depth <= LG_TUBE_RING_MAX = 1024, row < 16, column < 64).
template <int RT, int NT_, bool WLDS>
__global__ void __launch_bounds__(NT_) k_tube_rollout_window(TubeDev D, const float *x, int64_t n_seq, int T, int fb, int taps, int dN,
                                                             int stride, const uint8_t *reseed, float *o) {
    constexpr int RB_ = RT < 4 ? RT : 4;
    static_assert(RT * LG_TUBE_MAX_IN <= TUBE_RO_PRE * NT_ && RT <= NT_ && RT <= 16, "tile shape");
    extern __shared__ float lds[];
    const int tid = threadIdx.x, I = D.in_dim, O = D.out_dim, U = D.units, L = D.layers;
    const int depth = (taps - 1) * dN + 1;
    const int64_t base = (int64_t)blockIdx.x * RT;
    const int nr = (int)(n_seq - base < RT ? n_seq - base : RT);
    float *W = lds;
    float *X = W + (WLDS ? D.num_params : 0), *H0 = X + RT * I, *H1 = H0 + RT * U, *F = H1 + RT * U;
    float *ring = F + RT * O;           // (RT, depth, fb): slot t % depth of row r holds out[r, t, 0:fb]
    int *age = (int *)(ring + RT * depth * fb);   // (RT) steps since the row's seed: 0 at t == 0 and at a reseed
    if (WLDS) {
        for (int64_t p = tid; p < D.num_params; p += NT_) W[p] = D.wt[p];
        __syncthreads();
        for (int li = 0; li <= L; ++li)
            for (int j = tid; j < D.dout[li]; j += NT_) W[D.off_b[li] + j] = D.params[D.off_b[li] + j];
    }
    const float *wsrc = WLDS ? W : D.wt, *bsrc = WLDS ? W : D.params;
    const int nq = (RT * I + NT_ - 1) / NT_;
    // as in k_tube_rollout; pfb: the fed-back element's code (above), -1 a teacher-only column, -2 past the tile
    int64_t poff[TUBE_RO_PRE];
    int pfb[TUBE_RO_PRE];
    float pre[TUBE_RO_PRE];
    int pfresh = 1;
#pragma unroll
    for (int q = 0; q < TUBE_RO_PRE; ++q) {
        int e = tid + q * NT_;
        const bool live = e < RT * I;
        e = live ? e : RT * I - 1;
        const int r = e / I, c = e - r * I;
        const int tap = taps > 1 ? c / stride : 0, cc = c - tap * stride;
        poff[q] = (r < nr ? base + r : n_seq - 1) * T * I + c;
        pfb[q] = live ? (tap < taps && cc < fb ? (tap * dN) << 10 | r << 6 | cc : -1) : -2;
    }
    auto fetch = [&](int t) {
#pragma unroll
        for (int q = 0; q < TUBE_RO_PRE; ++q)
            if (q < nq) pre[q] = x[poff[q] + (int64_t)t * I];
        if (tid < RT) pfresh = reseed && tid < nr && reseed[(base + tid) * T + t];
    };
    fetch(0);
    if (tid < RT) age[tid] = 0;
    __syncthreads();
    int head = -1;                      // (t - 1) % depth: the slot of out[t-1]
    for (int t = 0; t < T; ++t) {
        if (t > 0) {
            head = head + 1 == depth ? 0 : head + 1;
            for (int e = tid; e < RT * fb; e += NT_) {
                const int r = e / fb, c = e - r * fb;
                ring[(r * depth + head) * fb + c] = F[r * O + c];
            }
        }
#pragma unroll
        for (int q = 0; q < TUBE_RO_PRE; ++q) {
            if (q < nq && pfb[q] != -2) {
                const int code = pfb[q];
                float v = pre[q];
                if (code >= 0) {
                    const int r = (code >> 6) & 15, c = code & 63, lag = code >> 10;
                    if (age[r] > lag) {
                        const int slot = head - lag + (head < lag ? depth : 0);
                        v = lag ? ring[(r * depth + slot) * fb + c] : F[r * O + c];
                    }
                }
                X[tid + q * NT_] = v;
            }
        }
        if (t + 1 < T) fetch(t + 1);
        __syncthreads();
        const float *in = X;
        for (int li = 0; li < L; ++li) {
            float *out = li & 1 ? H1 : H0;
            tube_layer<RT, RB_, NT_, false>(tid, D.din[li], U, in, wsrc + D.off_w[li], bsrc + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
        }
        tube_layer<RT, RB_, NT_, true>(tid, D.din[L], O, in, wsrc + D.off_w[L], bsrc + D.off_b[L], D.act, D.sp_beta, F,
                                       o + (base * T + t) * O, (int64_t)T * O, nr);
        if (tid < RT) age[tid] = pfresh ? 0 : age[tid] + 1;
        __syncthreads();
    }
}

// LDS of a roll-out tile in floats, without the weights
static size_t tubek_rollout_acts(const TubeDev *D, int rt) { return (size_t)rt * (D->in_dim + 2 * D->units + D->out_dim + 1); }
// rows per workgroup from the batch: the smallest tile that keeps the launch within about two workgroups per CU of the chip's 256
static int tubek_rollout_tile(int64_t n_seq) { return n_seq <= 256 ? 1 : n_seq <= 2048 ? 4 : 16; }
// weights go to LDS where weights + tile fit LG_TUBE_ROLLOUT_LDS
// (ring: the floats of a windowed roll-out's output ring per row, 0 for the single-tap kernel)
static int tubek_rollout_wlds(const TubeDev *D, int rt, int ring = 0) {
    return sizeof(float) * (D->num_params + tubek_rollout_acts(D, rt) + (size_t)rt * ring) <= LG_TUBE_ROLLOUT_LDS;
}

template <int RT, int NT_>
static void rollout_launch(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, const uint8_t *reseed, float *o, hipStream_t s) {
    const int nwg = (int)((n_seq + RT - 1) / RT);
    const bool wl = tubek_rollout_wlds(D, RT);
    const size_t bytes = sizeof(float) * (tubek_rollout_acts(D, RT) + (wl ? D->num_params : 0));
    if (wl) hipLaunchKernelGGL((k_tube_rollout<RT, NT_, true>), dim3(nwg), dim3(NT_), bytes, s, *D, x, n_seq, T, fb, reseed, o);
    else hipLaunchKernelGGL((k_tube_rollout<RT, NT_, false>), dim3(nwg), dim3(NT_), bytes, s, *D, x, n_seq, T, fb, reseed, o);
}

template <int RT, int NT_>
static void rollout_window_launch(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, int taps, int dN, int stride,
                                  const uint8_t *reseed, float *o, hipStream_t s) {
    const int nwg = (int)((n_seq + RT - 1) / RT), ring = ((taps - 1) * dN + 1) * fb;
    const bool wl = tubek_rollout_wlds(D, RT, ring);
    const size_t bytes = sizeof(float) * (tubek_rollout_acts(D, RT) + (size_t)RT * ring + (wl ? D->num_params : 0));
    if (wl) hipLaunchKernelGGL((k_tube_rollout_window<RT, NT_, true>), dim3(nwg), dim3(NT_), bytes, s, *D, x, n_seq, T, fb, taps, dN, stride, reseed, o);
    else hipLaunchKernelGGL((k_tube_rollout_window<RT, NT_, false>), dim3(nwg), dim3(NT_), bytes, s, *D, x, n_seq, T, fb, taps, dN, stride, reseed, o);
}

extern "C" {
void tubek_rollout_window(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, int taps, int dN, int stride,
                          const uint8_t *reseed, float *o, hipStream_t s) {
    switch (tubek_rollout_tile(n_seq)) {
    case 1: rollout_window_launch<1, 64>(D, x, n_seq, T, fb, taps, dN, stride, reseed, o, s); break;
    case 4: rollout_window_launch<4, 64>(D, x, n_seq, T, fb, taps, dN, stride, reseed, o, s); break;
    default: rollout_window_launch<16, 256>(D, x, n_seq, T, fb, taps, dN, stride, reseed, o, s); break;
    }
}
void tubek_rollout(const TubeDev *D, const float *x, int64_t n_seq, int T, int fb, const uint8_t *reseed, float *o, hipStream_t s) {
    switch (tubek_rollout_tile(n_seq)) {
    case 1: rollout_launch<1, 64>(D, x, n_seq, T, fb, reseed, o, s); break;
    case 4: rollout_launch<4, 64>(D, x, n_seq, T, fb, reseed, o, s); break;
    default: rollout_launch<16, 256>(D, x, n_seq, T, fb, reseed, o, s); break;
    }
}
void tubek_predict(const TubeDev *D, const float *x, const float *y, const float *v, const int32_t *rows, const int32_t *env,
                   const int32_t *start, int T, int nz, int m, int64_t count, float *o, hipStream_t s) {
    const TubeGather G{x, y, v, rows, env, start, T, nz, m};
    const size_t bytes = sizeof(float) * (size_t)R * (D->in_dim + 2 * D->units);
    hipLaunchKernelGGL(k_tube_predict, dim3((unsigned)((count + R - 1) / R)), dim3(NT), bytes, s, *D, G, count, o);
}

void tubek_predict_levels(const TubeDev *D, const float *x, const int32_t *rows, int64_t count, const float *levels, int n_levels,
                          float *o, hipStream_t s) {
    const TubeGather G{x, nullptr, nullptr, rows, nullptr, nullptr, 0, 0, 0};
    const size_t bytes = sizeof(float) * (size_t)R * (D->in_dim - 1 + 3 * D->units);
    hipLaunchKernelGGL(k_tube_predict_levels<false>, dim3((unsigned)((count + R - 1) / R)), dim3(NT), bytes, s, *D, G, count, levels,
                       n_levels, o);
}
// k_tube_predict_windows_levels: the same tile with the window gather
void tubek_predict_windows_levels(const TubeDev *D, const float *w, const float *z, const float *v, const int32_t *env,
                                  const int32_t *start, int T, int nz, int m, int64_t count, const float *levels, int n_levels,
                                  float *o, hipStream_t s) {
    const TubeGather G{w, z, v, nullptr, env, start, T, nz, m};
    const size_t bytes = sizeof(float) * (size_t)R * (D->in_dim - 1 + 3 * D->units);
    hipLaunchKernelGGL(k_tube_predict_levels<true>, dim3((unsigned)((count + R - 1) / R)), dim3(NT), bytes, s, *D, G, count, levels,
                       n_levels, o);
}

size_t tubek_lds_bytes(const TubeDev *D) {
    return sizeof(float) * (size_t)R * (D->in_dim + D->layers * D->units + 2 * D->out_dim + 2 * D->units);
}
int tubek_init() {
    const int lim = (int)(sizeof(float) * R * (LG_TUBE_MAX_IN + 4 * LG_TUBE_MAX_UNITS + 2 * LG_TUBE_MAX_OUT + 2 * LG_TUBE_MAX_UNITS));
    for (const void *f : {(const void *)k_tube_rows<true, false>, (const void *)k_tube_rows<false, false>,
                          (const void *)k_tube_rows<true, true>, (const void *)k_tube_rows<false, true>,
                          (const void *)k_tube_rows_sweep<true, false>, (const void *)k_tube_rows_sweep<false, false>,
                          (const void *)k_tube_rows_sweep<true, true>, (const void *)k_tube_rows_sweep<false, true>})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lim) != hipSuccess) return -1;
    const int plim = (int)(sizeof(float) * R * (LG_TUBE_MAX_IN + 2 * LG_TUBE_MAX_UNITS));
    if (hipFuncSetAttribute((const void *)k_tube_predict, hipFuncAttributeMaxDynamicSharedMemorySize, plim) != hipSuccess) return -1;
    const int llim = (int)(sizeof(float) * R * (LG_TUBE_MAX_IN - 1 + 3 * LG_TUBE_MAX_UNITS));
    for (const void *f : {(const void *)k_tube_predict_levels<false>, (const void *)k_tube_predict_levels<true>})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, llim) != hipSuccess) return -1;
    for (const void *f : {(const void *)k_tube_rollout<1, 64, true>, (const void *)k_tube_rollout<1, 64, false>,
                          (const void *)k_tube_rollout<4, 64, true>, (const void *)k_tube_rollout<4, 64, false>,
                          (const void *)k_tube_rollout<16, 256, true>, (const void *)k_tube_rollout<16, 256, false>,
                          (const void *)k_tube_rollout_window<1, 64, true>, (const void *)k_tube_rollout_window<1, 64, false>,
                          (const void *)k_tube_rollout_window<4, 64, true>, (const void *)k_tube_rollout_window<4, 64, false>,
                          (const void *)k_tube_rollout_window<16, 256, true>, (const void *)k_tube_rollout_window<16, 256, false>})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LG_TUBE_ROLLOUT_LDS) != hipSuccess) return -1;
    return 0;
}
void tubek_step(const TubeDev *D, const TubeSplit *S, const int32_t *rows, int64_t count, uint64_t key, float norm, hipStream_t s) {
    const int nwg = (int)((count + R - 1) / R);
    if (D->level_input) hipLaunchKernelGGL((k_tube_rows<true, true>), dim3(nwg), dim3(NT), tubek_lds_bytes(D), s, *D, *S, rows, count, key, norm, -1.f);
    else hipLaunchKernelGGL((k_tube_rows<true, false>), dim3(nwg), dim3(NT), tubek_lds_bytes(D), s, *D, *S, rows, count, key, norm, -1.f);
}
void tubek_adam(const TubeDev *D, int nwg, int64_t t, double lr0, double gamma, int64_t step_size, float norm, int64_t rows,
                hipStream_t s) {
    int blocks = (int)((D->num_params + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_tube_adam, dim3(blocks), dim3(256), 0, s, *D, nwg, t, lr0, gamma, step_size, norm, rows);
}
// level: a level-conditioned model's fixed level (lg_tube_eval_level), or negative: one drawn per row
void tubek_eval(const TubeDev *D, const TubeSplit *S, const int32_t *rows, uint64_t key, float norm, float level, hipStream_t s) {
    const int nwg = (int)((S->rows + R - 1) / R);
    if (D->level_input) hipLaunchKernelGGL((k_tube_rows<false, true>), dim3(nwg), dim3(NT), tubek_lds_bytes(D), s, *D, *S, rows, S->rows, key, norm, level);
    else hipLaunchKernelGGL((k_tube_rows<false, false>), dim3(nwg), dim3(NT), tubek_lds_bytes(D), s, *D, *S, rows, S->rows, key, norm, level);
    hipLaunchKernelGGL(k_tube_eval_finish, dim3(1), dim3(256), 0, s, *D, nwg, norm, (float)(S->rows * (int64_t)D->out_dim));
}
// ---- sweep: the same launches with the members along grid y.  M: device array of K members; D0: member 0's host copy (the shape).
void tubek_step_sweep(const TubeMember *M, int K, const TubeDev *D0, const TubeSplit *S, const int32_t *rows, int64_t pos, int64_t count,
                      uint64_t key, float norm, hipStream_t s) {
    const int nwg = (int)((count + R - 1) / R);
    if (D0->level_input) hipLaunchKernelGGL((k_tube_rows_sweep<true, true>), dim3(nwg, K), dim3(NT), tubek_lds_bytes(D0), s, M, *S, rows, pos, count, key, norm, -1.f);
    else hipLaunchKernelGGL((k_tube_rows_sweep<true, false>), dim3(nwg, K), dim3(NT), tubek_lds_bytes(D0), s, M, *S, rows, pos, count, key, norm, -1.f);
}
void tubek_adam_sweep(const TubeMember *M, int K, const TubeDev *D0, int nwg, int64_t t, float norm, int64_t rows, hipStream_t s) {
    int blocks = (int)((D0->num_params + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_tube_adam_sweep, dim3(blocks, K), dim3(256), 0, s, M, nwg, t, norm, rows);
}
void tubek_eval_sweep(const TubeMember *M, int K, const TubeDev *D0, const TubeSplit *S, const int32_t *rows, uint64_t key, float norm,
                      float level, hipStream_t s) {
    const int nwg = (int)((S->rows + R - 1) / R);
    if (D0->level_input) hipLaunchKernelGGL((k_tube_rows_sweep<false, true>), dim3(nwg, K), dim3(NT), tubek_lds_bytes(D0), s, M, *S, rows, (int64_t)0, S->rows, key, norm, level);
    else hipLaunchKernelGGL((k_tube_rows_sweep<false, false>), dim3(nwg, K), dim3(NT), tubek_lds_bytes(D0), s, M, *S, rows, (int64_t)0, S->rows, key, norm, level);
    hipLaunchKernelGGL(k_tube_eval_finish_sweep, dim3(1, K), dim3(256), 0, s, M, nwg, norm, (float)(S->rows * (int64_t)D0->out_dim));
}
void tubek_perm_sweep(const TubeMember *M, int K, int n, uint64_t epoch, hipStream_t s) {
    int bits = 2;
    while ((1ll << bits) < n) ++bits;
    bits += bits & 1;
    hipLaunchKernelGGL(k_tube_perm_sweep, dim3((n + 255) / 256, K), dim3(256), 0, s, M, n, bits / 2, epoch);
}
void tubek_wt(const TubeDev *D, hipStream_t s) { hipLaunchKernelGGL(k_tube_wt, dim3(64), dim3(256), 0, s, *D); }
void tubek_perm(const TubeDev *D, int n, uint64_t epoch, hipStream_t s) {
    int bits = 2;
    while ((1ll << bits) < n) ++bits;
    bits += bits & 1;
    hipLaunchKernelGGL(k_tube_perm, dim3((n + 255) / 256), dim3(256), 0, s, *D, n, bits / 2, epoch);
}
void tubek_iota(int32_t *p, int64_t n, hipStream_t s) { hipLaunchKernelGGL(k_tube_iota, dim3(256), dim3(256), 0, s, p, n); }
}
