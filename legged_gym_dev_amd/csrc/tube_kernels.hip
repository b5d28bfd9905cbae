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
#include <cstring>

#include "tube_device.h"

// lg_plan_problem.R, read before R becomes the tile's row count below
__device__ __forceinline__ const float *plan_input_cost(const lg_plan_problem &p) { return p.R; }

#define R LG_TUBE_ROWS
#define NT LG_TUBE_THREADS
#define RB 4                            // rows per thread in the forward / input-gradient loops (one weight load, RB FMAs)

__device__ __forceinline__ float tube_act(int act, float x, float beta) {
    switch (act) {
    case LG_TUBE_ACT_RELU: return x > 0.f ? x : 0.f;
    case LG_TUBE_ACT_SOFTPLUS: return x * beta > 20.f ? x : log1pf(expf(x * beta)) / beta;   // torch: threshold 20
    case LG_TUBE_ACT_TANH: return tanhf(x);
    default: return x > 0.f ? x : expm1f(x);                                              // ELU, alpha 1
    }
}
// derivative from the activation's output h (what LDS keeps); torch's tie rules: ReLU'(0) = 0, ELU'(0) = exp(0) = 1
__device__ __forceinline__ float tube_act_grad(int act, float h, float beta) {
    switch (act) {
    case LG_TUBE_ACT_RELU: return h > 0.f ? 1.f : 0.f;
    case LG_TUBE_ACT_SOFTPLUS: return h * beta > 20.f ? 1.f : -expm1f(-h * beta);   // sigmoid(beta x) = 1 - exp(-beta h)
    case LG_TUBE_ACT_TANH: return 1.f - h * h;
    default: return h > 0.f ? 1.f : h + 1.f;
    }
}

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
// One Linear layer of a tile of RT rows, shared by k_tube_predict and every k_tube_rollout shape.  Each output is the same chain
// as in k_tube_rows -- acc = 0, fmaf over k = 0..K-1 in order, + bias, activation -- whatever RT, RB or the weights' address
// space, so a row's result does not depend on the tile it sits in.  w: the layer's transposed weights [k][j]; b: its bias.
// Hidden layers write the activated output to `out` (LDS, (RT, N)); the LAST one writes the raw output to `out` (LDS, may be
// null) and to g[r * gld + j] for the rows r < nr.
template <int RT, int RB_, int NT_, bool LAST>
__device__ __forceinline__ void tube_layer(int tid, int K, int N, const float *in, const float *w, const float *b, int act, float beta,
                                           float *out, float *g, int64_t gld, int nr) {
    for (int e = tid; e < N * (RT / RB_); e += NT_) {
        const int j = e % N, r0 = (e / N) * RB_;
        float acc[RB_];
#pragma unroll
        for (int q = 0; q < RB_; ++q) acc[q] = 0.f;
#pragma unroll 8                        // eight operand loads in flight per wait: a lone wave per SIMD has nothing else to hide LDS latency behind
        for (int k = 0; k < K; ++k) {
            const float wv = w[k * N + j];
#pragma unroll
            for (int q = 0; q < RB_; ++q) acc[q] = fmaf(in[(r0 + q) * K + k], wv, acc[q]);
        }
        const float bj = b[j];
#pragma unroll
        for (int q = 0; q < RB_; ++q) {
            const float z = acc[q] + bj;
            if (LAST) {
                if (out) out[(r0 + q) * N + j] = z;
                if (r0 + q < nr) g[(int64_t)(r0 + q) * gld + j] = z;
            } else {
                out[(r0 + q) * N + j] = tube_act(act, z, beta);
            }
        }
    }
}

// out[i] = MLP(item i).  Flat: item i = x[rows ? rows[i] : i].  Horizon: the ScalarHorizonTubeDataset item at (env[i], start[i])
// of the arrays in G (the caller guarantees H_rev <= start and start + H_fwd <= T).  No loss, no slab; weights through wt.
struct TubeGather {
    const float *x, *y, *v;             // flat: x (n, in).  horizon: w (n, T), z (n, T, nz), v (n, T, m)
    const int32_t *rows, *env, *start;
    int T, nz, m;
};

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
                const int64_t s = G.env[base + r];
                const int t0 = G.start[base + r];
                if (c < D.H_rev) x = G.x[s * G.T + t0 - D.H_rev + c];
                else if (c < D.H_rev + G.nz) x = G.y[(s * G.T + t0) * G.nz + (c - D.H_rev)];
                else {
                    const int q = c - D.H_rev - G.nz, tt = q / G.m;
                    x = G.v[(s * G.T + t0 - D.H_rev + tt) * G.m + (q - tt * G.m)];
                }
            }
        }
        X[e] = x;
    }
    __syncthreads();
    const float *in = X;
    for (int li = 0; li < L; ++li) {
        float *out = li & 1 ? H1 : H0;
        tube_layer<R, RB, NT, false>(tid, D.din[li], U, in, D.wt + D.off_w[li], D.params + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
        __syncthreads();
        in = out;
    }
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
                const int64_t s = G.env[base + r];
                const int t0 = G.start[base + r];
                if (c < D.H_rev) x = G.x[s * G.T + t0 - D.H_rev + c];
                else if (c < D.H_rev + G.nz) x = G.y[(s * G.T + t0) * G.nz + (c - D.H_rev)];
                else {
                    const int q = c - D.H_rev - G.nz, tt = q / G.m;
                    x = G.v[(s * G.T + t0 - D.H_rev + tt) * G.m + (q - tt * G.m)];
                }
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

// ------------------------------------------------------------------ plans against a tube
// Score R plans per workgroup: the one-shot tube of every plan through tube_layer (or an analytic tube), then one lane per plan
// walks the plan's nodes -- ROM state, tube, clearance, cost, counts -- in one fixed-order chain.  The reference's definitions:
// trajopt/tube_trajopt.py ("TT") oneshot_nn_tube_dyn :561-568, the analytic tubes :489-540, the obstacle constraint :59-97, the
// objective :41-56,206-212; SingleInt2D.f is trajopt/rom_dynamics.py:192.
struct PlanDev {                        // passed by value
    lg_plan_problem p;
    const float *z0, *v, *e, *v_prev, *w0, *offset;
    float *cost, *min_clear, *fw, *z, *w;
    int32_t *worst_node, *n_viol;
    float level;
    int Hr, I;                          // columns of the tile's item: Hr past errors, 2 (Hr + N) inputs, (level); analytic kinds: Hr = 0
    const float *sc_goal, *sc_obs;      // lg_plan_scenes (section 10.14): read by the <SC = true> kernels alone
    const int32_t *sc_n;
};

#define PLAN_ZS(N) ((((N) + 1) * 3) | 1)    // floats of a plan's (z, w) nodes in LDS: odd, so that the lanes' rows fall on different banks

// sum((d @ M) * d) of a 2-vector, M row-major (TT:56)
__device__ __forceinline__ float plan_quad(const float *M, float d0, float d1) {
#pragma clang fp contract(off)
    return (d0 * M[0] + d1 * M[2]) * d0 + (d0 * M[1] + d1 * M[3]) * d1;
}

// The scene a walk runs against: the goal, the obstacle list and its length, read through one accessor.
// PlanSceneProb: the call's one scene in the by-value problem -- uniform reads, the code of the entries without scenes.
// PlanSceneRow: a row of PLAN_SCN floats in LDS, [goal x, y, (cx, cy, r) x LG_PLAN_MAX_OBS, count]; the stride is odd, so the 32
// walking lanes read different banks.  plan_scene_stage fills the rows of a tile before its first barrier.
#define PLAN_SCN (3 + 3 * LG_PLAN_MAX_OBS)
static_assert(PLAN_SCN == 27 && (PLAN_SCN & 1), "a scene row: 2 + 24 + 1 floats, an odd stride");
struct PlanSceneProb {
    const lg_plan_problem &p;
    __device__ __forceinline__ int n() const { return p.n_obs; }
    __device__ __forceinline__ float cx(int i) const { return p.obs_c[i][0]; }
    __device__ __forceinline__ float cy(int i) const { return p.obs_c[i][1]; }
    __device__ __forceinline__ float r(int i) const { return p.obs_r[i]; }
    __device__ __forceinline__ float gx() const { return p.goal[0]; }
    __device__ __forceinline__ float gy() const { return p.goal[1]; }
};
struct PlanSceneRow {
    const float *s;
    __device__ __forceinline__ int n() const { return (int)s[PLAN_SCN - 1]; }
    __device__ __forceinline__ float cx(int i) const { return s[2 + 3 * i]; }
    __device__ __forceinline__ float cy(int i) const { return s[3 + 3 * i]; }
    __device__ __forceinline__ float r(int i) const { return s[4 + 3 * i]; }
    __device__ __forceinline__ float gx() const { return s[0]; }
    __device__ __forceinline__ float gy() const { return s[1]; }
};
// Rows 0 .. rows - 1 of SCN take scenes s0, s0 + 1, ..; rows at and past nr are zeros with a zero count.  A part the scenes leave
// out (goal, or obs and n_obs) comes from the problem; n_obs[s] is clamped into 0 .. LG_PLAN_MAX_OBS and slots past it are not read.
__device__ __forceinline__ void plan_scene_stage(const PlanDev &P, float *SCN, int64_t s0, int rows, int nr, int tid) {
    for (int e = tid; e < rows * PLAN_SCN; e += NT) {
        const int r = e / PLAN_SCN, c = e - r * PLAN_SCN;
        float x = 0.f;
        if (r < nr) {
            const int64_t s = s0 + r;
            if (c < 2) x = P.sc_goal ? P.sc_goal[s * 2 + c] : P.p.goal[c];
            else {
                int n = P.sc_n ? P.sc_n[s] : P.p.n_obs;
                n = n < 0 ? 0 : (n > LG_PLAN_MAX_OBS ? LG_PLAN_MAX_OBS : n);
                const int q = c - 2, i = q / 3, k = q - 3 * i;
                if (c == PLAN_SCN - 1) x = (float)n;
                else if (i < n) x = P.sc_obs ? P.sc_obs[s * (3 * LG_PLAN_MAX_OBS) + q] : (k < 2 ? P.p.obs_c[i][k] : P.p.obs_r[i]);
            }
        }
        SCN[e] = x;
    }
}

// One lane's walk over a plan's nodes, shared by k_plan_score and k_plan_sample_score: the analytic tube (where the kind is one), the
// ROM nodes, the tube nodes, clearance, cost and counts in one fixed-order chain, every operation rounded on its own.  vr: the plan's
// inputs (N, 2) in the lane's item; fw (N): the MLP's tube values, or written here for an analytic kind; zw: PLAN_ZS floats of nodes.
// PEN adds the three hinge sums of the sampling planner (section 10.10), each its own chain over the nodes in ascending order:
// pen_g += max(0, -g) per obstacle, pen_w += max(0, w - w_max), pen_z += max(0, z_d - z_max_d) + max(0, z_min_d - z_d) per axis d.
struct PlanWalk {
    float cost, minc, pen_g, pen_w, pen_z;
    int worst, nv_g, nv_v, nv_z, nv_w;
};
template <bool PEN, class SN>
__device__ __forceinline__ PlanWalk plan_walk(const lg_plan_problem &p, const SN &sn, bool nn, const float *vr, float *fw, float *zw, float zx, float zy,
                                              float wk, const float *offset) {
#pragma clang fp contract(off)
    const int N = p.N;
    if (!nn) {
        const bool l1 = p.tube_kind == LG_PLAN_TUBE_L1 || p.tube_kind == LG_PLAN_TUBE_L1_ROLLING;
        for (int k = 0; k < N; ++k) {
            const float vx = vr[2 * k], vy = vr[2 * k + 1];
            fw[k] = p.scaling * (l1 ? fabsf(vx) + fabsf(vy) : vx * vx + vy * vy);
        }
        if (p.tube_kind == LG_PLAN_TUBE_L1_ROLLING || p.tube_kind == LG_PLAN_TUBE_L2_ROLLING) {
            for (int k = N - 1; k >= 0; --k) {  // descending: fw[k] reads the plain values at and before k only
                const int k0 = k - p.window_size + 1 > 0 ? k - p.window_size + 1 : 0;
                float s = 0.f;
                for (int i = k0; i <= k; ++i) s = s + fw[i];
                fw[k] = s / (float)(k - k0 + 1);
            }
        }
    }
    PlanWalk W;
    W.cost = 0.f; W.minc = INFINITY; W.pen_g = 0.f; W.pen_w = 0.f; W.pen_z = 0.f;
    W.worst = -1; W.nv_g = 0; W.nv_v = 0; W.nv_z = 0; W.nv_w = 0;
    const int n_obs = sn.n();
    const float gx = sn.gx(), gy = sn.gy();
    for (int k = 0; k <= N; ++k) {
        zw[3 * k] = zx; zw[3 * k + 1] = zy; zw[3 * k + 2] = wk;
        bool hit = false;
        for (int i = 0; i < n_obs; ++i) {
            const float dx = zx - sn.cx(i), dy = zy - sn.cy(i), rr = sn.r(i) + wk;
            const float g = (dx * dx + dy * dy) - rr * rr;
            if (g < W.minc) { W.minc = g; W.worst = k; }
            hit = hit || g < 0.f;
            if (PEN) W.pen_g = W.pen_g + fmaxf(0.f, -g);
        }
        W.nv_g += hit;
        W.nv_z += zx < p.rom_z_min[0] || zx > p.rom_z_max[0] || zy < p.rom_z_min[1] || zy > p.rom_z_max[1];
        W.nv_w += wk > p.w_max;
        if (PEN) {
            W.pen_w = W.pen_w + fmaxf(0.f, wk - p.w_max);
            W.pen_z = W.pen_z + (fmaxf(0.f, zx - p.rom_z_max[0]) + fmaxf(0.f, p.rom_z_min[0] - zx));
            W.pen_z = W.pen_z + (fmaxf(0.f, zy - p.rom_z_max[1]) + fmaxf(0.f, p.rom_z_min[1] - zy));
        }
        W.cost = W.cost + plan_quad(k < N ? p.Q : p.Qf, zx - gx, zy - gy);
        const float vx = k < N ? vr[2 * k] : 0.f, vy = k < N ? vr[2 * k + 1] : 0.f;
        if (k < N) {
            W.nv_v += vx < p.rom_v_min[0] || vx > p.rom_v_max[0] || vy < p.rom_v_min[1] || vy > p.rom_v_max[1];
            W.cost = W.cost + plan_quad(plan_input_cost(p), vx, vy);
        }
        W.cost = W.cost + (wk * p.Qw) * wk;
        if (k < N) {
            zx = zx + p.dt * vx; zy = zy + p.dt * vy;          // SingleInt2D.f
            wk = offset ? fw[k] + offset[k] : fw[k];
        }
    }
    return W;
}

// The tile's items: the ScalarHorizonTubeDataset item at start = H_rev of w = e, z = none, v = cat(v_prev, v) of plans base .. base + nr - 1,
// straight into X (R, I); rows past nr are zeros.  Shared by k_plan_score and k_plan_grad.
__device__ __forceinline__ void plan_gather(const PlanDev &P, float *X, int64_t base, int nr, int tid) {
    const int N = P.p.N, I = P.I, Hr = P.Hr;
    for (int e = tid; e < R * I; e += NT) {
        const int r = e / I, c = e - r * I;
        float x = 0.f;
        if (r < nr) {
            const int64_t b = base + r;
            if (c < Hr) x = P.e ? P.e[b * Hr + c] : 0.f;
            else if (c < Hr + 2 * (Hr + N)) {
                const int q = c - Hr, tt = q >> 1, d = q & 1;
                if (tt < Hr) x = P.v_prev ? P.v_prev[(b * Hr + tt) * 2 + d] : 0.f;
                else x = P.v[(b * N + (tt - Hr)) * 2 + d];
            } else x = P.level;
        }
        X[e] = x;
    }
}

// Dynamic LDS: X (R, I) the items -- for an analytic kind the plan's inputs alone --, H0, H1 (R, U) (NN kind), FW (R, N), ZW (R, PLAN_ZS),
// and with SC the scenes SCN (R, PLAN_SCN): row r walks against scene base + r.
template <bool SC>
__global__ void __launch_bounds__(NT) k_plan_score(TubeDev D, PlanDev P, int64_t count) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, I = P.I, Hr = P.Hr;
    const bool nn = P.p.tube_kind == LG_PLAN_TUBE_NN;
    const int U = nn ? D.units : 0, L = D.layers, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds, *H0 = X + R * I, *H1 = H0 + R * U, *FW = H1 + R * U, *ZW = FW + R * N, *SCN = ZW + R * ZS;
    plan_gather(P, X, base, nr, tid);
    if (SC) plan_scene_stage(P, SCN, base, R, nr, tid);
    __syncthreads();
    if (nn) {
        const float *in = X;
        for (int li = 0; li < L; ++li) {
            float *out = li & 1 ? H1 : H0;
            tube_layer<R, RB, NT, false>(tid, D.din[li], U, in, D.wt + D.off_w[li], D.params + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
        }
        tube_layer<R, RB, NT, true>(tid, D.din[L], N, in, D.wt + D.off_w[L], D.params + D.off_b[L], D.act, D.sp_beta, FW,
                                    P.fw ? P.fw + base * N : nullptr, N, P.fw ? nr : 0);
        __syncthreads();
    }
    if (tid < nr) {
        const int64_t b = base + tid;
        const float *vr = X + tid * I + 3 * Hr;
        const float w0 = P.w0 ? P.w0[b] : 0.f;
        const PlanWalk W = SC ? plan_walk<false>(P.p, PlanSceneRow{SCN + tid * PLAN_SCN}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[b * 2],
                                                 P.z0[b * 2 + 1], w0, P.offset)
                              : plan_walk<false>(P.p, PlanSceneProb{P.p}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[b * 2], P.z0[b * 2 + 1],
                                                 w0, P.offset);
        P.cost[b] = W.cost; P.min_clear[b] = W.minc; P.worst_node[b] = W.worst;
        P.n_viol[b * 4] = W.nv_g; P.n_viol[b * 4 + 1] = W.nv_v; P.n_viol[b * 4 + 2] = W.nv_z; P.n_viol[b * 4 + 3] = W.nv_w;
    }
    if (!P.z && !P.w && (nn || !P.fw)) return;
    __syncthreads();
    for (int e = tid; e < nr * (N + 1); e += NT) {
        const int r = e / (N + 1), k = e - r * (N + 1);
        const float *zw = ZW + r * ZS + 3 * k;
        const int64_t o = (base + r) * (N + 1) + k;
        if (P.z) { P.z[o * 2] = zw[0]; P.z[o * 2 + 1] = zw[1]; }
        if (P.w) P.w[o] = zw[2];
    }
    if (!nn && P.fw)
        for (int e = tid; e < nr * N; e += NT) P.fw[base * N + e] = FW[e];
}

// ------------------------------------------------------------------ sampling planner on a tube (MPPI)
// One iteration is two launches: k_plan_sample_score draws K candidates around every instance's mean plan and scores them with
// k_plan_score's own tile; k_plan_mppi_update folds them into the new mean by softmin weights.  No candidate is stored: both kernels
// regenerate it from Philox through mppi_candidate.
struct MppiDev {                        // passed by value
    const float *vbar_in;               // (P, N, 2) mean plans read by the launch
    float *vbar;                        // the same array, written by the update
    float *J, *pen, *best_J, *best_v, *hist;
    int32_t *n_bad;
    uint64_t seed;
    uint32_t inst0, it;                 // instance id of instance 0, iteration
    int K, N, reset;
    float sigma_it, lambda, rho_g, rho_w, rho_z;
    float v_min[2], v_max[2];
};

// Candidate j of instance id `inst` at iteration `it`, node k: clip(vbar + sigma_it eps, v_min, v_max), every operation rounded on its
// own.  eps = one Philox4x32-10 block keyed by the call's seed at counter (inst, it, j, node | tag): Box-Muller on its first two words,
// the cosine branch for x and the sine branch for y; u1 in (0, 1], the angle 2 pi u2 taken as sincospi(2 u2).  Candidate 0 is the
// mean plan itself.  The only place a candidate is made: k_plan_sample_score, k_plan_mppi_update and k_plan_mppi_candidates call it.
__device__ __forceinline__ void mppi_candidate(const MppiDev &M, uint32_t inst, int j, int k, float bx, float by, float *vx, float *vy) {
#pragma clang fp contract(off)
    float x = bx, y = by;
    if (j != 0) {
        uint32_t c[4] = {inst, M.it, (uint32_t)j, 0x4d500000u | (uint32_t)k};
        philox4x32((uint32_t)M.seed, (uint32_t)(M.seed >> 32), c);
        const float u1 = ((float)(c[0] >> 8) + 1.0f) * (1.0f / 16777216.0f), u2 = (float)(c[1] >> 8) * (1.0f / 16777216.0f);
        const float r = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        x = bx + M.sigma_it * (r * cs);
        y = by + M.sigma_it * (r * sn);
    }
    *vx = fminf(fmaxf(x, M.v_min[0]), M.v_max[0]);
    *vy = fminf(fmaxf(y, M.v_min[1]), M.v_max[1]);
}

// for tests and tools: the (P, K, N, 2) candidates of one iteration, one thread per (instance, candidate, node)
__global__ void __launch_bounds__(NT) k_plan_mppi_candidates(MppiDev M, int64_t count, float *out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= count) return;
    const int k = (int)(i % M.N);
    const int64_t g = i / M.N;
    const int p = (int)(g / M.K), j = (int)(g - (int64_t)p * M.K);
    const float *vb = M.vbar_in + ((int64_t)p * M.N + k) * 2;
    mppi_candidate(M, M.inst0 + (uint32_t)p, j, k, vb[0], vb[1], out + i * 2, out + i * 2 + 1);
}

// k_plan_score's tile -- R candidates per workgroup, the same LDS layout -- with the plan columns of the item drawn in place instead
// of gathered: tile t holds candidates 32 (t mod K/32) .. + 31 of instance t / (K/32) (K is a multiple of R), so one z0, e, v_prev,
// w0 serves the tile.  The layers and the lane's walk are k_plan_score's.  J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z.
// P.cost, P.min_clear and M.pen (P, K, 3) are optional here.  No atomics; a candidate depends on (seed, instance id, it, j) alone.
// With SC the tile's instance has a scene of its own: one row SCN (PLAN_SCN) behind ZW, which every walking lane reads.
template <bool SC>
__global__ void __launch_bounds__(NT) k_plan_sample_score(TubeDev D, PlanDev P, MppiDev M) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, I = P.I, Hr = P.Hr;
    const bool nn = P.p.tube_kind == LG_PLAN_TUBE_NN;
    const int U = nn ? D.units : 0, L = D.layers, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int pi = (int)(base / M.K), j0 = (int)(base - (int64_t)pi * M.K);
    float *X = lds, *H0 = X + R * I, *H1 = H0 + R * U, *FW = H1 + R * U, *ZW = FW + R * N, *SCN = ZW + R * ZS;
    if (SC) plan_scene_stage(P, SCN, pi, 1, 1, tid);
    for (int e = tid; e < R * I; e += NT) {         // the columns beside the plan: the instance's e, v_prev and the level
        const int r = e / I, c = e - r * I;
        if (c < Hr) X[e] = P.e ? P.e[(int64_t)pi * Hr + c] : 0.f;
        else if (c < 3 * Hr) X[e] = P.v_prev ? P.v_prev[(int64_t)pi * Hr * 2 + (c - Hr)] : 0.f;
        else if (c >= Hr + 2 * (Hr + N)) X[e] = P.level;
    }
    for (int q = tid; q < R * N; q += NT) {         // the plan: one Philox block per (candidate, node)
        const int r = q / N, k = q - r * N;
        const float *vb = M.vbar_in + ((int64_t)pi * N + k) * 2;
        float *x = X + r * I + 3 * Hr + 2 * k;
        mppi_candidate(M, M.inst0 + (uint32_t)pi, j0 + r, k, vb[0], vb[1], x, x + 1);
    }
    __syncthreads();
    if (nn) {
        const float *in = X;
        for (int li = 0; li < L; ++li) {
            float *out = li & 1 ? H1 : H0;
            tube_layer<R, RB, NT, false>(tid, D.din[li], U, in, D.wt + D.off_w[li], D.params + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
        }
        tube_layer<R, RB, NT, true>(tid, D.din[L], N, in, D.wt + D.off_w[L], D.params + D.off_b[L], D.act, D.sp_beta, FW, nullptr, N, 0);
        __syncthreads();
    }
    if (tid < R) {
#pragma clang fp contract(off)
        const int64_t b = base + tid;
        const float *vr = X + tid * I + 3 * Hr;
        const float w0 = P.w0 ? P.w0[pi] : 0.f;
        const PlanWalk W = SC ? plan_walk<true>(P.p, PlanSceneRow{SCN}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[pi * 2], P.z0[pi * 2 + 1],
                                                w0, P.offset)
                              : plan_walk<true>(P.p, PlanSceneProb{P.p}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[pi * 2],
                                                P.z0[pi * 2 + 1], w0, P.offset);
        M.J[b] = ((W.cost + M.rho_g * W.pen_g) + M.rho_w * W.pen_w) + M.rho_z * W.pen_z;
        if (P.cost) P.cost[b] = W.cost;
        if (P.min_clear) P.min_clear[b] = W.minc;
        if (M.pen) { M.pen[b * 3] = W.pen_g; M.pen[b * 3 + 1] = W.pen_w; M.pen[b * 3 + 2] = W.pen_z; }
    }
}

// The softmin update, one workgroup per instance.  Dynamic LDS: K floats, J then the weights.
//   1. Jmin and its first index over the finite J: thread t scans j = t, t + 256, .. ascending, then a halving tree over the threads
//      that prefers the smaller value and, on a tie, the smaller index.
//   2. weight_j = expf(-(J_j - Jmin) / lambda), 0 for a non-finite J.
//   3. Every sum over the candidates has one order, fixed by K alone: MPPI_CH = 64 chunks, chunk c adding j = c, c + 64, .. ascending
//      from 0, then a halving tree over the chunks (c += c + 32, 16, .. 1).  The weights' sum S takes it on threads 0..63; the
//      weighted sums take it MPPI_NB = 4 nodes at a time -- thread t is chunk t / 4 of node k0 + t % 4 and accumulates x and y of its
//      candidates, regenerated by mppi_candidate -- so a thread makes K / 64 Philox blocks per pass and ceil(N / 4) passes, at P = 1 too.
//      A candidate of weight 0 is skipped: it adds +0 to a sum that is not -0.
//   4. vbar[k] = sum / S.  With no finite J the mean stays and n_bad counts the iteration.  The elite: where Jmin < best_J (or at a
//      reset) best_J and best_v take the arg-min candidate; a reset without a finite J leaves best_J = inf and best_v = the mean.
//      hist = (J of candidate 0, Jmin).
#define MPPI_CH 64
#define MPPI_NB (NT / MPPI_CH)
__device__ __forceinline__ bool mppi_finite(float x) { return fabsf(x) < INFINITY; }
__global__ void __launch_bounds__(NT) k_plan_mppi_update(MppiDev M) {
#pragma clang fp contract(off)
    extern __shared__ float wl[];
    __shared__ float red[NT * 2];
    __shared__ int redi[NT];
    const int tid = threadIdx.x, p = blockIdx.x, K = M.K, N = M.N;
    const float *J = M.J + (int64_t)p * K;
    float m = INFINITY;
    int mi = -1;
    for (int j = tid; j < K; j += NT) {
        const float x = J[j];
        wl[j] = x;
        if (mppi_finite(x) && (mi < 0 || x < m)) { m = x; mi = j; }
    }
    red[tid] = m; redi[tid] = mi;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const float b = red[tid + h];
            const int bi = redi[tid + h], ai = redi[tid];
            if (bi >= 0 && (ai < 0 || b < red[tid] || (b == red[tid] && bi < ai))) { red[tid] = b; redi[tid] = bi; }
        }
        __syncthreads();
    }
    const float Jmin = red[0];
    const int best = redi[0];
    const float J0 = wl[0], bJ = M.best_J[p];
    const bool improved = best >= 0 && (M.reset || Jmin < bJ);
    __syncthreads();
    for (int j = tid; j < K; j += NT) {
        const float x = wl[j];
        wl[j] = mppi_finite(x) ? expf(-(x - Jmin) / M.lambda) : 0.f;
    }
    __syncthreads();
    const int c = tid / MPPI_NB, n = tid - c * MPPI_NB;
    if (tid < MPPI_CH) {
        float s = 0.f;
        for (int j = tid; j < K; j += MPPI_CH) s = s + wl[j];
        red[tid] = s;
    }
    __syncthreads();
    for (int h = MPPI_CH / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    const float S = red[0];
    __syncthreads();
    const uint32_t inst = M.inst0 + (uint32_t)p;
    for (int k0 = 0; k0 < N; k0 += MPPI_NB) {
        const int k = k0 + n;
        const bool on = k < N;
        float bx = 0.f, by = 0.f, ax = 0.f, ay = 0.f;
        if (on) {
            const float *vb = M.vbar_in + ((int64_t)p * N + k) * 2;
            bx = vb[0]; by = vb[1];
            for (int j = c; j < K; j += MPPI_CH) {
                const float w = wl[j];
                if (w == 0.f) continue;
                float vx, vy;
                mppi_candidate(M, inst, j, k, bx, by, &vx, &vy);
                ax = ax + w * vx; ay = ay + w * vy;
            }
        }
        red[tid * 2] = ax; red[tid * 2 + 1] = ay;
        __syncthreads();
        for (int h = MPPI_CH / 2; h > 0; h >>= 1) {
            if (c < h) {
                red[tid * 2] = red[tid * 2] + red[(tid + h * MPPI_NB) * 2];
                red[tid * 2 + 1] = red[tid * 2 + 1] + red[(tid + h * MPPI_NB) * 2 + 1];
            }
            __syncthreads();
        }
        if (c == 0 && on) {
            const int64_t o = ((int64_t)p * N + k) * 2;
            if (improved) mppi_candidate(M, inst, best, k, bx, by, M.best_v + o, M.best_v + o + 1);
            else if (M.reset) { M.best_v[o] = bx; M.best_v[o + 1] = by; }
            if (best >= 0) { M.vbar[o] = red[tid * 2] / S; M.vbar[o + 1] = red[tid * 2 + 1] / S; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (improved) M.best_J[p] = Jmin;
        else if (M.reset) M.best_J[p] = INFINITY;
        if (M.hist) { M.hist[p * 2] = J0; M.hist[p * 2 + 1] = Jmin; }
        const int bad = best < 0;
        M.n_bad[p] = M.reset ? bad : M.n_bad[p] + bad;
    }
}

// ------------------------------------------------------------------ plans against a one-step tube
// LG_PLAN_TUBE_NN_STEP: the flat scalar tube MLP rolled node by node along the plan, w[k+1] = fw(w[k], v[k], ..) (the reference's
// trajopt/old/rom_tube_planning.py:106-107), inside the scoring tile.  A workgroup owns R plans as k_plan_score does and keeps their
// history in LDS: per plan a line of inputs -- v_prev, then the plan, so the lane's walk still reads (N, 2) contiguous inputs -- and
// a line of tube values e, w0, fw[0..N-1].  Per node it builds the (R, I) rows from the two lines, runs the L + 1 layers through
// tube_layer -- the chains of k_tube_rollout, so fw carries that kernel's bits -- and the last layer appends fw[k] to the w lines.
// The lines' strides are odd, so the 32 walking lanes fall on different banks.
#define PLAN_STEP_VS(Hr, N) ((2 * ((Hr) + (N))) | 1)
#define PLAN_STEP_WS(Hr, N) (((Hr) + (N) + 1) | 1)
#define PLAN_STEP_PRE 4                 // row elements whose source a thread keeps in registers: R * 32 columns / NT
constexpr size_t plan_step_floats(int I, int U, int Hr, int N, bool scenes) {   // the tile without the weights
    return (size_t)R * (PLAN_STEP_VS(Hr, N) + PLAN_STEP_WS(Hr, N) + I + 2 * U + PLAN_ZS(N) + (scenes ? PLAN_SCN : 0));
}
struct PlanStepTile {
    float *W, *V, *WL, *X, *H0, *H1, *ZW, *SCN;         // SCN (R, PLAN_SCN): the tile's scenes, kernels with SC alone
    int VS, WS;
};
__device__ __forceinline__ PlanStepTile plan_step_tile(float *lds, const TubeDev &D, const PlanDev &P, bool wlds) {
    PlanStepTile S;
    S.VS = PLAN_STEP_VS(P.Hr, P.p.N); S.WS = PLAN_STEP_WS(P.Hr, P.p.N);
    S.W = lds;
    S.V = lds + (wlds ? D.num_params : 0);
    S.WL = S.V + R * S.VS; S.X = S.WL + R * S.WS; S.H0 = S.X + R * P.I; S.H1 = S.H0 + R * D.units; S.ZW = S.H1 + R * D.units;
    S.SCN = S.ZW + R * PLAN_ZS(P.p.N);
    return S;
}
// Element (r, c) of the row tile: where node 0 reads it, as a float offset from the V lines (the w lines follow them) with bit 30
// set where the source advances 2 floats per node (an input column) instead of 1 (a tube column); -1 for the level column, which
// is written once.  Tap i of node k is step k - i: the input at V[2 (Hr + k - i)], the tube value at WL[Hr + k - i] (Hr >= T - 1).
__device__ __forceinline__ int plan_step_src(int r, int c, int Ix, bool rec, int Hr, int VS, int WS) {
    if (c >= Ix) return -1;
    int tap, col;                       // col 0: the tube value; 1, 2: the input's x, y
    if (rec) { tap = c / 3; col = c - tap * 3; }
    else if (c == 0) { tap = 0; col = 0; }
    else { tap = (c - 1) >> 1; col = 1 + ((c - 1) & 1); }
    return col == 0 ? R * VS + r * WS + Hr - tap : (1 << 30) | (r * VS + 2 * (Hr - tap) + col - 1);
}
// The node loop of a tile whose V and w lines are filled up to node 0 (no barrier needed before the call): fw[k] of every row lands
// in its w line at Hr + 1 + k.  WLDS: the transposed weights and the biases are staged to LDS once, as in k_tube_rollout.
template <bool WLDS>
__device__ __forceinline__ void plan_step_roll(const TubeDev &D, const PlanDev &P, const PlanStepTile &S, int tid) {
    const int N = P.p.N, I = P.I, Hr = P.Hr, U = D.units, L = D.layers, Ix = I - (D.level_input ? 1 : 0);
    const bool rec = P.p.recursive != 0;
    if (WLDS) {
        for (int64_t p = tid; p < D.num_params; p += NT) S.W[p] = D.wt[p];
        __syncthreads();
        for (int li = 0; li <= L; ++li)
            for (int j = tid; j < D.dout[li]; j += NT) S.W[D.off_b[li] + j] = D.params[D.off_b[li] + j];
    }
    const float *wsrc = WLDS ? S.W : D.wt, *bsrc = WLDS ? S.W : D.params;
    int src[PLAN_STEP_PRE];
#pragma unroll
    for (int q = 0; q < PLAN_STEP_PRE; ++q) {
        const int e = tid + q * NT;
        src[q] = e < R * I ? plan_step_src(e / I, e % I, Ix, rec, Hr, S.VS, S.WS) : -1;
    }
    if (D.level_input)
        for (int r = tid; r < R; r += NT) S.X[r * I + I - 1] = P.level;
    __syncthreads();
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int q = 0; q < PLAN_STEP_PRE; ++q)
            if (src[q] >= 0) S.X[tid + q * NT] = S.V[(src[q] & 0x3fffffff) + k * (1 + (src[q] >> 30))];
        for (int e = tid + PLAN_STEP_PRE * NT; e < R * I; e += NT) {     // rows wider than 32 columns: the source per element
            const int sc = plan_step_src(e / I, e % I, Ix, rec, Hr, S.VS, S.WS);
            if (sc >= 0) S.X[e] = S.V[(sc & 0x3fffffff) + k * (1 + (sc >> 30))];
        }
        __syncthreads();
        const float *in = S.X;
        for (int li = 0; li < L; ++li) {
            float *out = li & 1 ? S.H1 : S.H0;
            tube_layer<R, RB, NT, false>(tid, D.din[li], U, in, wsrc + D.off_w[li], bsrc + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
        }
        tube_layer<R, RB, NT, true>(tid, D.din[L], 1, in, wsrc + D.off_w[L], bsrc + D.off_b[L], D.act, D.sp_beta, nullptr,
                                    S.WL + Hr + 1 + k, S.WS, R);
        __syncthreads();
    }
}

// k_plan_score for the one-step kind.  Dynamic LDS: (W the parameters), V (R, VS), WL (R, WS), X (R, I), H0, H1 (R, U), ZW (R, PLAN_ZS),
// (SCN (R, PLAN_SCN) the scenes).
template <bool WLDS, bool SC>
__global__ void __launch_bounds__(NT) k_plan_score_step(TubeDev D, PlanDev P, int64_t count) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, Hr = P.Hr, ZS = PLAN_ZS(N), VC = 2 * (Hr + N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    const PlanStepTile S = plan_step_tile(lds, D, P, WLDS);
    for (int e = tid; e < R * VC; e += NT) {            // rows past nr are zeros
        const int r = e / VC, c = e - r * VC;
        float x = 0.f;
        if (r < nr) {
            const int64_t b = base + r;
            if (c < 2 * Hr) x = P.v_prev ? P.v_prev[b * 2 * Hr + c] : 0.f;
            else x = P.v[b * 2 * N + (c - 2 * Hr)];
        }
        S.V[r * S.VS + c] = x;
    }
    for (int e = tid; e < R * (Hr + 1); e += NT) {
        const int r = e / (Hr + 1), c = e - r * (Hr + 1);
        float x = 0.f;
        if (r < nr) {
            const int64_t b = base + r;
            if (c < Hr) x = P.e ? P.e[b * Hr + c] : 0.f;
            else x = P.w0 ? P.w0[b] : 0.f;
        }
        S.WL[r * S.WS + c] = x;
    }
    if (SC) plan_scene_stage(P, S.SCN, base, R, nr, tid);
    plan_step_roll<WLDS>(D, P, S, tid);
    if (tid < nr) {
        const int64_t b = base + tid;
        const float *vr = S.V + tid * S.VS + 2 * Hr;
        float *fw = S.WL + tid * S.WS + Hr + 1;
        const PlanWalk W = SC ? plan_walk<false>(P.p, PlanSceneRow{S.SCN + tid * PLAN_SCN}, true, vr, fw, S.ZW + tid * ZS, P.z0[b * 2],
                                                 P.z0[b * 2 + 1], S.WL[tid * S.WS + Hr], P.offset)
                              : plan_walk<false>(P.p, PlanSceneProb{P.p}, true, vr, fw, S.ZW + tid * ZS, P.z0[b * 2], P.z0[b * 2 + 1],
                                                 S.WL[tid * S.WS + Hr], P.offset);
        P.cost[b] = W.cost; P.min_clear[b] = W.minc; P.worst_node[b] = W.worst;
        P.n_viol[b * 4] = W.nv_g; P.n_viol[b * 4 + 1] = W.nv_v; P.n_viol[b * 4 + 2] = W.nv_z; P.n_viol[b * 4 + 3] = W.nv_w;
    }
    if (P.fw)
        for (int e = tid; e < nr * N; e += NT) {
            const int r = e / N, k = e - r * N;
            P.fw[base * N + e] = S.WL[r * S.WS + Hr + 1 + k];
        }
    if (!P.z && !P.w) return;
    __syncthreads();
    for (int e = tid; e < nr * (N + 1); e += NT) {
        const int r = e / (N + 1), k = e - r * (N + 1);
        const float *zw = S.ZW + r * ZS + 3 * k;
        const int64_t o = (base + r) * (N + 1) + k;
        if (P.z) { P.z[o * 2] = zw[0]; P.z[o * 2 + 1] = zw[1]; }
        if (P.w) P.w[o] = zw[2];
    }
}

// k_plan_sample_score for the one-step kind: the same tile with the plan columns drawn in place; tile t holds candidates of one
// instance, whose v_prev, e and w0 every row shares.  J is formed by k_plan_sample_score's expression.
template <bool WLDS, bool SC>
__global__ void __launch_bounds__(NT) k_plan_sample_score_step(TubeDev D, PlanDev P, MppiDev M) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, Hr = P.Hr, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int pi = (int)(base / M.K), j0 = (int)(base - (int64_t)pi * M.K);
    const PlanStepTile S = plan_step_tile(lds, D, P, WLDS);
    for (int e = tid; e < R * 2 * Hr; e += NT) {
        const int r = e / (2 * Hr), c = e - r * (2 * Hr);
        S.V[r * S.VS + c] = P.v_prev ? P.v_prev[(int64_t)pi * Hr * 2 + c] : 0.f;
    }
    for (int q = tid; q < R * N; q += NT) {         // the plan: one Philox block per (candidate, node)
        const int r = q / N, k = q - r * N;
        const float *vb = M.vbar_in + ((int64_t)pi * N + k) * 2;
        float *x = S.V + r * S.VS + 2 * Hr + 2 * k;
        mppi_candidate(M, M.inst0 + (uint32_t)pi, j0 + r, k, vb[0], vb[1], x, x + 1);
    }
    for (int e = tid; e < R * (Hr + 1); e += NT) {
        const int r = e / (Hr + 1), c = e - r * (Hr + 1);
        S.WL[r * S.WS + c] = c < Hr ? (P.e ? P.e[(int64_t)pi * Hr + c] : 0.f) : (P.w0 ? P.w0[pi] : 0.f);
    }
    if (SC) plan_scene_stage(P, S.SCN, pi, 1, 1, tid);
    plan_step_roll<WLDS>(D, P, S, tid);
    if (tid < R) {
#pragma clang fp contract(off)
        const int64_t b = base + tid;
        const float *vr = S.V + tid * S.VS + 2 * Hr;
        float *fw = S.WL + tid * S.WS + Hr + 1;
        const float w0 = P.w0 ? P.w0[pi] : 0.f;
        const PlanWalk W = SC ? plan_walk<true>(P.p, PlanSceneRow{S.SCN}, true, vr, fw, S.ZW + tid * ZS, P.z0[pi * 2], P.z0[pi * 2 + 1], w0,
                                                P.offset)
                              : plan_walk<true>(P.p, PlanSceneProb{P.p}, true, vr, fw, S.ZW + tid * ZS, P.z0[pi * 2], P.z0[pi * 2 + 1], w0,
                                                P.offset);
        M.J[b] = ((W.cost + M.rho_g * W.pen_g) + M.rho_w * W.pen_w) + M.rho_z * W.pen_z;
        if (P.cost) P.cost[b] = W.cost;
        if (P.min_clear) P.min_clear[b] = W.minc;
        if (M.pen) { M.pen[b * 3] = W.pen_g; M.pen[b * 3 + 1] = W.pen_w; M.pen[b * 3 + 2] = W.pen_z; }
    }
}

// ------------------------------------------------------------------ gradient planner on a tube
// J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z of R plans per workgroup and dJ/dv of every plan by a reverse sweep in the
// same workgroup, with projected Adam and the elite fused behind it.  No atomics; a plan's outputs depend on its own row alone.
//
// One Linear layer backwards for a tile of R rows, in place: h (R, K) holds the layer's activated input and takes
// dIn[r][k] = act'(h[r][k]) * sum_j delta[r][j] W[j][k], W = the layer's weights as the parameters keep them ([j][k], lanes across k),
// each sum one fmaf chain from 0 with j ascending.  No thread reads another's h, so in place needs no second buffer.
__device__ __forceinline__ void tube_layer_back(int tid, int K, int No, const float *delta, const float *w, float *h, int act, float beta) {
    for (int e = tid; e < K * (R / RB); e += NT) {
        const int k = e % K, r0 = (e / K) * RB;
        float acc[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) acc[q] = 0.f;
#pragma unroll 8
        for (int j = 0; j < No; ++j) {
            const float wv = w[j * K + k];
#pragma unroll
            for (int q = 0; q < RB; ++q) acc[q] = fmaf(delta[(r0 + q) * No + j], wv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) h[(r0 + q) * K + k] = tube_act_grad(act, h[(r0 + q) * K + k], beta) * acc[q];
    }
}

// plan_walk in reverse, one lane per plan, every operation rounded on its own.  zw: the nodes plan_walk left; vr: the plan's inputs.
// Nodes k = N..1 (z0 and w0 get no gradient).  Per node the local adjoints, each one chain in this order: the state (goal) term
// d (M + M'), then per obstacle i ascending where g < 0 strictly (the hinge max(0, -g); g recomputed by plan_walk's own expression)
// -rho_g 2 (z - c_i) for z and +rho_g 2 (r_i + w) for w, then +-rho_z where a state bound is passed strictly; for w: 2 Qw w first,
// rho_w where w > w_max last.  a = sum_{j >= k} dJ/dz_j, nodes descending.  Left behind: dfw[k-1] = dJ/dw_k = dJ/dfw[k-1] (the
// offset is a constant), and in the slots of node k, zw[3k + d], dJ/dv[k-1][d] = v (R + R') + dt a, without the tube's part.
// Analytic kinds then add the tube's part in the same lane, steps i ascending: db = dJ/dfw[i], or for a rolling kind the window's
// transposed mean sum_{k = i..min(i + window - 1, N - 1)} dJ/dfw[k] / (k - k0(k) + 1), k ascending from 0; times scaling sign(v)
// (l1, 0 at 0) or (2 scaling) v (l2).
template <class SN>
__device__ __forceinline__ void plan_walk_back(const lg_plan_problem &p, const SN &sn, bool nn, const float *vr, float *dfw, float *zw, float rho_g,
                                               float rho_w, float rho_z) {
#pragma clang fp contract(off)
    const int N = p.N;
    const float *Ri = plan_input_cost(p);
    const int n_obs = sn.n();
    const float gx = sn.gx(), gy = sn.gy();
    float ax = 0.f, ay = 0.f;
    for (int k = N; k >= 1; --k) {
        const float zx = zw[3 * k], zy = zw[3 * k + 1], wk = zw[3 * k + 2];
        const float *M = k < N ? p.Q : p.Qf;
        const float d0 = zx - gx, d1 = zy - gy;
        float lx = (M[0] + M[0]) * d0 + (M[1] + M[2]) * d1;
        float ly = (M[1] + M[2]) * d0 + (M[3] + M[3]) * d1;
        float lw = (2.f * p.Qw) * wk;
        for (int i = 0; i < n_obs; ++i) {
            const float dx = zx - sn.cx(i), dy = zy - sn.cy(i), rr = sn.r(i) + wk;
            const float g = (dx * dx + dy * dy) - rr * rr;
            if (g < 0.f) {
                lx = lx - rho_g * (2.f * dx);
                ly = ly - rho_g * (2.f * dy);
                lw = lw + rho_g * (2.f * rr);
            }
        }
        if (zx - p.rom_z_max[0] > 0.f) lx = lx + rho_z;
        if (p.rom_z_min[0] - zx > 0.f) lx = lx - rho_z;
        if (zy - p.rom_z_max[1] > 0.f) ly = ly + rho_z;
        if (p.rom_z_min[1] - zy > 0.f) ly = ly - rho_z;
        if (wk - p.w_max > 0.f) lw = lw + rho_w;
        ax = ax + lx; ay = ay + ly;
        dfw[k - 1] = lw;
        const float vx = vr[2 * (k - 1)], vy = vr[2 * (k - 1) + 1];
        zw[3 * k] = ((Ri[0] + Ri[0]) * vx + (Ri[1] + Ri[2]) * vy) + p.dt * ax;
        zw[3 * k + 1] = ((Ri[1] + Ri[2]) * vx + (Ri[3] + Ri[3]) * vy) + p.dt * ay;
    }
    if (nn) return;
    const bool l1 = p.tube_kind == LG_PLAN_TUBE_L1 || p.tube_kind == LG_PLAN_TUBE_L1_ROLLING;
    const bool rolling = p.tube_kind == LG_PLAN_TUBE_L1_ROLLING || p.tube_kind == LG_PLAN_TUBE_L2_ROLLING;
    const int ws = p.window_size < N ? p.window_size : N;
    for (int i = 0; i < N; ++i) {
        float db = dfw[i];
        if (rolling) {
            const int k1 = i + ws - 1 < N - 1 ? i + ws - 1 : N - 1;
            db = 0.f;
            for (int k = i; k <= k1; ++k) {
                const int k0 = k - ws + 1 > 0 ? k - ws + 1 : 0;
                db = db + dfw[k] / (float)(k - k0 + 1);
            }
        }
        const float vx = vr[2 * i], vy = vr[2 * i + 1];
        const float tx = l1 ? p.scaling * (float)((vx > 0.f) - (vx < 0.f)) : (2.f * p.scaling) * vx;
        const float ty = l1 ? p.scaling * (float)((vy > 0.f) - (vy < 0.f)) : (2.f * p.scaling) * vy;
        zw[3 * (i + 1)] = zw[3 * (i + 1)] + db * tx;
        zw[3 * (i + 1) + 1] = zw[3 * (i + 1) + 1] + db * ty;
    }
}

// Dynamic LDS: X (R, I) the items as in k_plan_score, H_l (R, U) per hidden layer l (every activated output is kept for the reverse
// sweep), FW (R, N): the tube values, then dJ/dfw in place, ZW (R, PLAN_ZS): the nodes, then per row [J, elite flag, bad flag] in node
// 0's slots and dJ/dv[k][d] in slot 3 (k + 1) + d.
//   1. gather, tube_layer per layer, plan_walk<true>: k_plan_sample_score's forward, so J and its parts are that kernel's bits.
//   2. plan_walk_back in the lane that walked the plan.
//   3. NN kind: delta of the output layer = dJ/dfw; tube_layer_back per hidden layer, last to first, in place over H_l; of the first
//      layer's input gradient only the 2 N plan columns are formed -- sum_j delta_0[r][j] W_0[j][3 H_rev + c], one fmaf chain from 0,
//      j ascending -- and dJ/dv = (the lane's term) + (that sum).
//   4. the lane: bad = J or some dJ/dv not finite; hist = (J, max |dJ/dv|); the elite takes the plan evaluated where J is finite and
//      (reset or J < best_J), before any step; n_bad counts the steps refused.
//   5. per plan element, coalesced: grad out, best_v, and with `step` Adam on (m, s) and the projection clip(v, v_min, v_max),
//      every operation rounded on its own: m = beta1 m + (1 - beta1) g; s = beta2 s + ((1 - beta2) g) g;
//      v = clip(v - lr (m / bc1) / (sqrt(s / bc2) + eps)).  A bad plan keeps v, m and s.
struct GradDev {                        // passed by value
    float *v, *J, *grad, *pen, *m, *s, *best_J, *best_v, *hist;
    int32_t *n_bad;
    int step, reset;
    float lr, beta1, beta2, eps, bc1, bc2, rho_g, rho_w, rho_z;
    float v_min[2], v_max[2];
};

template <bool SC>                      // SC: the scenes SCN (R, PLAN_SCN) follow ZW; both walks of row r read scene base + r
__global__ void __launch_bounds__(NT) k_plan_grad(TubeDev D, PlanDev P, GradDev G, int64_t count) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, I = P.I, Hr = P.Hr;
    const bool nn = P.p.tube_kind == LG_PLAN_TUBE_NN;
    const int U = nn ? D.units : 0, L = nn ? D.layers : 0, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds, *H = X + R * I, *FW = H + R * U * L, *ZW = FW + R * N, *SCN = ZW + R * ZS;
    plan_gather(P, X, base, nr, tid);
    if (SC) plan_scene_stage(P, SCN, base, R, nr, tid);
    __syncthreads();
    if (nn) {
        const float *in = X;
        for (int li = 0; li < L; ++li) {
            float *out = H + li * R * U;
            tube_layer<R, RB, NT, false>(tid, D.din[li], U, in, D.wt + D.off_w[li], D.params + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
            __syncthreads();
            in = out;
        }
        tube_layer<R, RB, NT, true>(tid, D.din[L], N, in, D.wt + D.off_w[L], D.params + D.off_b[L], D.act, D.sp_beta, FW, nullptr, N, 0);
        __syncthreads();
    }
    if (tid < nr) {
#pragma clang fp contract(off)
        const int64_t b = base + tid;
        float *zw = ZW + tid * ZS;
        const float *vr = X + tid * I + 3 * Hr;
        const float w0 = P.w0 ? P.w0[b] : 0.f;
        const PlanSceneRow row{SCN + tid * PLAN_SCN};
        const PlanWalk W = SC ? plan_walk<true>(P.p, row, nn, vr, FW + tid * N, zw, P.z0[b * 2], P.z0[b * 2 + 1], w0, P.offset)
                              : plan_walk<true>(P.p, PlanSceneProb{P.p}, nn, vr, FW + tid * N, zw, P.z0[b * 2], P.z0[b * 2 + 1], w0, P.offset);
        const float J = ((W.cost + G.rho_g * W.pen_g) + G.rho_w * W.pen_w) + G.rho_z * W.pen_z;
        G.J[b] = J;
        if (P.cost) P.cost[b] = W.cost;
        if (P.min_clear) P.min_clear[b] = W.minc;
        if (G.pen) { G.pen[b * 3] = W.pen_g; G.pen[b * 3 + 1] = W.pen_w; G.pen[b * 3 + 2] = W.pen_z; }
        if (SC) plan_walk_back(P.p, row, nn, vr, FW + tid * N, zw, G.rho_g, G.rho_w, G.rho_z);
        else plan_walk_back(P.p, PlanSceneProb{P.p}, nn, vr, FW + tid * N, zw, G.rho_g, G.rho_w, G.rho_z);
        zw[0] = J;
    }
    __syncthreads();
    if (nn) {
        const float *delta = FW;
        int No = N;
        for (int li = L; li >= 1; --li) {           // layer li: U inputs (hidden layer li - 1's output), No outputs
            float *h = H + (li - 1) * R * U;
            tube_layer_back(tid, U, No, delta, D.params + D.off_w[li], h, D.act, D.sp_beta);
            __syncthreads();
            delta = h; No = U;
        }
        const float *w0 = D.params + D.off_w[0] + 3 * Hr;
        for (int e = tid; e < 2 * N * (R / RB); e += NT) {
            const int c = e % (2 * N), r0 = (e / (2 * N)) * RB;
            float acc[RB];
#pragma unroll
            for (int q = 0; q < RB; ++q) acc[q] = 0.f;
#pragma unroll 8
            for (int j = 0; j < No; ++j) {
                const float wv = w0[j * I + c];
#pragma unroll
                for (int q = 0; q < RB; ++q) acc[q] = fmaf(delta[(r0 + q) * No + j], wv, acc[q]);
            }
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                float *g = ZW + (r0 + q) * ZS + 3 * ((c >> 1) + 1) + (c & 1);
                if (r0 + q < nr) *g = *g + acc[q];
            }
        }
        __syncthreads();
    }
    if (tid < nr) {
        const int64_t b = base + tid;
        float *zw = ZW + tid * ZS;
        const float J = zw[0];
        bool fin = mppi_finite(J);
        float gmax = 0.f;
        for (int k = 1; k <= N; ++k) {
            const float gx = zw[3 * k], gy = zw[3 * k + 1];
            fin = fin && mppi_finite(gx) && mppi_finite(gy);
            gmax = fmaxf(gmax, fmaxf(fabsf(gx), fabsf(gy)));
        }
        bool improved = false;
        if (G.best_J) {
            improved = mppi_finite(J) && (G.reset || J < G.best_J[b]);
            if (improved) G.best_J[b] = J;
            else if (G.reset) G.best_J[b] = INFINITY;
        }
        if (G.n_bad) G.n_bad[b] = (G.reset ? 0 : G.n_bad[b]) + (G.step && !fin ? 1 : 0);
        if (G.hist) { G.hist[b * 2] = J; G.hist[b * 2 + 1] = gmax; }
        zw[1] = improved ? 1.f : 0.f;
        zw[2] = fin ? 0.f : 1.f;
    }
    __syncthreads();
    for (int e = tid; e < nr * 2 * N; e += NT) {
#pragma clang fp contract(off)
        const int r = e / (2 * N), c = e - r * 2 * N, d = c & 1;
        const float *zw = ZW + r * ZS;
        const float g = zw[3 * ((c >> 1) + 1) + d], v = X[r * I + 3 * Hr + c];
        const bool bad = zw[2] != 0.f;
        const int64_t o = base * 2 * N + e;
        if (G.grad) G.grad[o] = g;
        if (G.best_v && (G.reset || zw[1] != 0.f)) G.best_v[o] = v;     // a reset without a finite J: best_J = inf, best_v = the plan
        if (G.step) {
            float m = G.reset ? 0.f : G.m[o], s = G.reset ? 0.f : G.s[o];
            if (!bad) {
                m = G.beta1 * m + (1.f - G.beta1) * g;
                s = G.beta2 * s + ((1.f - G.beta2) * g) * g;
                const float x = v - (G.lr * (m / G.bc1)) / (sqrtf(s / G.bc2) + G.eps);
                G.v[o] = fminf(fmaxf(x, G.v_min[d]), G.v_max[d]);
            }
            if (G.reset || !bad) { G.m[o] = m; G.s[o] = s; }
        }
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

// Per-plan scenes: sc = null launches the instantiation without them, the code of the entries before
// scenes; otherwise the <SC = true> one, whose tile carries R scene rows (one row in the sampling kernels, within the same budget).
constexpr size_t PLAN_SCN_BYTES = sizeof(float) * (size_t)R * PLAN_SCN;
static void plan_scenes_dev(PlanDev *P, const lg_plan_scenes *sc) {
    if (!sc) return;
    P->sc_goal = sc->goal; P->sc_obs = sc->obs; P->sc_n = sc->n_obs;
}
// the dynamic LDS ceiling of kernel f, set once per device, not per launch
static int plan_ceiling(const void *f, bool *set) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev < 0 || dev >= 64 || !set[dev]) {
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LG_TUBE_ROLLOUT_LDS) != hipSuccess) return -1;
        if (dev >= 0 && dev < 64) set[dev] = true;
    }
    return 0;
}

// k_plan_score.  D: the horizon handle's TubeDev, or null for an analytic kind.  Returns the dynamic LDS of the launch in bytes, or
// -1 where the kernel's ceiling cannot be set.  The reference shape (130 inputs, 128 units, N = 50) takes 74 KiB, past k_tube_predict's
// own 64 KiB, so the ceiling is the roll-out kernels'; the largest shape of the envelope stays below it:
static_assert(sizeof(float) * R * (LG_TUBE_MAX_IN + 2 * LG_TUBE_MAX_UNITS + LG_PLAN_MAX_N + PLAN_ZS(LG_PLAN_MAX_N) + PLAN_SCN) <= LG_TUBE_ROLLOUT_LDS,
              "k_plan_score: the envelope's largest tile set must fit the dynamic LDS ceiling");
int64_t tubek_plan_score(const TubeDev *D, const lg_plan_problem *prob, const float *z0, const float *v, const float *e,
                         const float *v_prev, const float *w0, const float *offset, float level, int64_t B, float *cost,
                         float *min_clear, int32_t *worst_node, int32_t *n_viol, float *fw, float *z, float *w,
                         const lg_plan_scenes *sc, hipStream_t s) {
    PlanDev P;
    memset(&P, 0, sizeof(P));
    plan_scenes_dev(&P, sc);
    TubeDev T;
    memset(&T, 0, sizeof(T));
    if (D) T = *D;
    const bool nn = prob->tube_kind == LG_PLAN_TUBE_NN;
    P.p = *prob;
    P.z0 = z0; P.v = v; P.e = nn ? e : nullptr; P.v_prev = nn ? v_prev : nullptr; P.w0 = w0; P.offset = offset;
    P.cost = cost; P.min_clear = min_clear; P.worst_node = worst_node; P.n_viol = n_viol; P.fw = fw; P.z = z; P.w = w;
    P.level = level;
    P.Hr = nn ? prob->H_rev : 0;
    P.I = nn ? T.in_dim : 2 * prob->N;
    const size_t bytes = sizeof(float) * (size_t)R * (P.I + (nn ? 2 * T.units : 0) + prob->N + PLAN_ZS(prob->N)) + (sc ? PLAN_SCN_BYTES : 0);
    static bool ceiling_set[2][64];
    const void *f = sc ? (const void *)k_plan_score<true> : (const void *)k_plan_score<false>;
    if (plan_ceiling(f, ceiling_set[sc != nullptr])) return -1;
    const dim3 grid((unsigned)((B + R - 1) / R));
    if (sc) hipLaunchKernelGGL(k_plan_score<true>, grid, dim3(NT), bytes, s, T, P, B);
    else hipLaunchKernelGGL(k_plan_score<false>, grid, dim3(NT), bytes, s, T, P, B);
    return (int64_t)bytes;
}

// The sampling planner's launches.  k_plan_sample_score's tile is k_plan_score's, so the assert above
// covers it; the update's dynamic LDS is the K weights:
static_assert(sizeof(float) * LG_MPPI_MAX_K <= 16 * 1024, "k_plan_mppi_update: K weights take at most 16 KiB of LDS");
static_assert(sizeof(float) * (LG_MPPI_MAX_K + 3 * NT) <= LG_TUBE_ROLLOUT_LDS, "k_plan_mppi_update: weights and reduction rows fit the LDS ceiling");
static_assert(LG_MPPI_MAX_K % R == 0 && NT % MPPI_CH == 0, "a tile of candidates belongs to one instance; whole nodes per pass");
static MppiDev mppi_dev(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it) {
    MppiDev M;
    memset(&M, 0, sizeof(M));
    M.seed = cfg->seed; M.inst0 = (uint32_t)cfg->instance_offset; M.it = (uint32_t)it;
    M.K = cfg->K; M.N = prob->N;
    float s = cfg->sigma;               // sigma_it = sigma * sigma_decay^it as `it` float32 products
    for (int i = 0; i < it; ++i) s = s * cfg->sigma_decay;
    M.sigma_it = s; M.lambda = cfg->lambda; M.rho_g = cfg->rho_g; M.rho_w = cfg->rho_w; M.rho_z = cfg->rho_z;
    for (int d = 0; d < 2; ++d) { M.v_min[d] = prob->rom_v_min[d]; M.v_max[d] = prob->rom_v_max[d]; }
    return M;
}
void tubek_plan_mppi_candidates(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const float *vbar, int64_t P_, float *out,
                                hipStream_t s) {
    MppiDev M = mppi_dev(prob, cfg, it);
    M.vbar_in = vbar;
    const int64_t count = P_ * cfg->K * prob->N;
    hipLaunchKernelGGL(k_plan_mppi_candidates, dim3((unsigned)((count + NT - 1) / NT)), dim3(NT), 0, s, M, count, out);
}
// returns the dynamic LDS of the launch in bytes, or -1 where the kernel's ceiling cannot be set
int64_t tubek_plan_sample_score(const TubeDev *D, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const float *z0,
                                const float *e, const float *v_prev, const float *w0, const float *offset, float level, int64_t P_,
                                const float *vbar, float *J, float *cost, float *min_clear, float *pen, const lg_plan_scenes *sc,
                                hipStream_t s) {
    PlanDev P;
    memset(&P, 0, sizeof(P));
    plan_scenes_dev(&P, sc);
    TubeDev T;
    memset(&T, 0, sizeof(T));
    if (D) T = *D;
    const bool nn = prob->tube_kind == LG_PLAN_TUBE_NN;
    P.p = *prob;
    P.z0 = z0; P.e = nn ? e : nullptr; P.v_prev = nn ? v_prev : nullptr; P.w0 = w0; P.offset = offset;
    P.cost = cost; P.min_clear = min_clear;
    P.level = level;
    P.Hr = nn ? prob->H_rev : 0;
    P.I = nn ? T.in_dim : 2 * prob->N;
    MppiDev M = mppi_dev(prob, cfg, it);
    M.vbar_in = vbar; M.J = J; M.pen = pen;
    const size_t bytes = sizeof(float) * ((size_t)R * (P.I + (nn ? 2 * T.units : 0) + prob->N + PLAN_ZS(prob->N)) + (sc ? PLAN_SCN : 0));
    static bool ceiling_set[2][64];
    const void *f = sc ? (const void *)k_plan_sample_score<true> : (const void *)k_plan_sample_score<false>;
    if (plan_ceiling(f, ceiling_set[sc != nullptr])) return -1;
    const dim3 grid((unsigned)(P_ * cfg->K / R));
    if (sc) hipLaunchKernelGGL(k_plan_sample_score<true>, grid, dim3(NT), bytes, s, T, P, M);
    else hipLaunchKernelGGL(k_plan_sample_score<false>, grid, dim3(NT), bytes, s, T, P, M);
    return (int64_t)bytes;
}
// The one-step kind.  Every shape of the envelope fits the ceiling without the weights -- the reference
// configurations (T <= 10, units <= 128, N <= 64) with room to spare --; lg_plan_check asks tubek_plan_step_bytes all the same.
static_assert(sizeof(float) * plan_step_floats(LG_TUBE_MAX_IN, LG_TUBE_MAX_UNITS, LG_PLAN_STEP_MAX_HREV, LG_PLAN_MAX_N, true) <= LG_TUBE_ROLLOUT_LDS,
              "k_plan_score_step: the envelope's largest tile set must fit the dynamic LDS ceiling");
static_assert(sizeof(float) * plan_step_floats(31, 128, LG_PLAN_STEP_MAX_HREV, 64, true) <= LG_TUBE_ROLLOUT_LDS, "the reference one-step shapes fit");
// dynamic LDS of the one-step tile in bytes, without the weights and without the scene rows
int64_t tubek_plan_step_bytes(const TubeDev *D, const lg_plan_problem *prob) {
    return (int64_t)(sizeof(float) * plan_step_floats(D->in_dim, D->units, prob->H_rev, prob->N, false));
}
static PlanDev plan_step_dev(const TubeDev *D, const lg_plan_problem *prob, const float *z0, const float *e, const float *v_prev,
                             const float *w0, const float *offset, float level, const lg_plan_scenes *sc) {
    PlanDev P;
    memset(&P, 0, sizeof(P));
    plan_scenes_dev(&P, sc);
    P.p = *prob;
    P.z0 = z0; P.e = e; P.v_prev = v_prev; P.w0 = w0; P.offset = offset;
    P.level = level;
    P.Hr = prob->H_rev;
    P.I = D->in_dim;
    return P;
}
// weights go to LDS where weights + tile fit the ceiling; *bytes: the launch's dynamic LDS
static bool plan_step_wlds(const TubeDev *D, const lg_plan_problem *prob, bool scenes, size_t *bytes) {
    const size_t tile = (size_t)tubek_plan_step_bytes(D, prob) + (scenes ? PLAN_SCN_BYTES : 0);
    const size_t all = tile + sizeof(float) * (size_t)D->num_params;
    const bool wl = all <= LG_TUBE_ROLLOUT_LDS;
    *bytes = wl ? all : tile;
    return wl;
}
// the four instantiations of a one-step kernel, by (weights in LDS, scenes)
#define PLAN_STEP_PICK(K, wl, sc) \
    ((wl) ? ((sc) ? (const void *)K<true, true> : (const void *)K<true, false>) : ((sc) ? (const void *)K<false, true> : (const void *)K<false, false>))
#define PLAN_STEP_LAUNCH(K, wl, sc, grid, bytes, s, ...)                                         \
    do {                                                                                         \
        if ((wl) && (sc)) hipLaunchKernelGGL((K<true, true>), grid, dim3(NT), bytes, s, __VA_ARGS__);       \
        else if (wl) hipLaunchKernelGGL((K<true, false>), grid, dim3(NT), bytes, s, __VA_ARGS__);           \
        else if (sc) hipLaunchKernelGGL((K<false, true>), grid, dim3(NT), bytes, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((K<false, false>), grid, dim3(NT), bytes, s, __VA_ARGS__);                  \
    } while (0)
// returns the dynamic LDS of the launch in bytes, or -1 where the kernel's ceiling cannot be set
int64_t tubek_plan_score_step(const TubeDev *D, const lg_plan_problem *prob, const float *z0, const float *v, const float *e,
                              const float *v_prev, const float *w0, const float *offset, float level, int64_t B, float *cost,
                              float *min_clear, int32_t *worst_node, int32_t *n_viol, float *fw, float *z, float *w,
                              const lg_plan_scenes *sc, hipStream_t s) {
    PlanDev P = plan_step_dev(D, prob, z0, e, v_prev, w0, offset, level, sc);
    P.v = v; P.cost = cost; P.min_clear = min_clear; P.worst_node = worst_node; P.n_viol = n_viol; P.fw = fw; P.z = z; P.w = w;
    size_t bytes;
    const bool wl = plan_step_wlds(D, prob, sc != nullptr, &bytes);
    static bool ceiling_set[4][64];
    if (plan_ceiling(PLAN_STEP_PICK(k_plan_score_step, wl, sc), ceiling_set[2 * wl + (sc != nullptr)])) return -1;
    const dim3 grid((unsigned)((B + R - 1) / R));
    PLAN_STEP_LAUNCH(k_plan_score_step, wl, sc, grid, bytes, s, *D, P, B);
    return (int64_t)bytes;
}
int64_t tubek_plan_sample_score_step(const TubeDev *D, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const float *z0,
                                     const float *e, const float *v_prev, const float *w0, const float *offset, float level, int64_t P_,
                                     const float *vbar, float *J, float *cost, float *min_clear, float *pen, const lg_plan_scenes *sc,
                                     hipStream_t s) {
    PlanDev P = plan_step_dev(D, prob, z0, e, v_prev, w0, offset, level, sc);
    P.cost = cost; P.min_clear = min_clear;
    MppiDev M = mppi_dev(prob, cfg, it);
    M.vbar_in = vbar; M.J = J; M.pen = pen;
    size_t bytes;
    const bool wl = plan_step_wlds(D, prob, sc != nullptr, &bytes);   // one scene row is read; the tile's budget is k_plan_score_step's
    static bool ceiling_set[4][64];
    if (plan_ceiling(PLAN_STEP_PICK(k_plan_sample_score_step, wl, sc), ceiling_set[2 * wl + (sc != nullptr)])) return -1;
    const dim3 grid((unsigned)(P_ * cfg->K / R));
    PLAN_STEP_LAUNCH(k_plan_sample_score_step, wl, sc, grid, bytes, s, *D, P, M);
    return (int64_t)bytes;
}
void tubek_plan_mppi_update(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, int reset, int64_t P_, float *vbar,
                            const float *J, float *best_J, float *best_v, float *hist, int32_t *n_bad, hipStream_t s) {
    MppiDev M = mppi_dev(prob, cfg, it);
    M.vbar_in = vbar; M.vbar = vbar; M.J = const_cast<float *>(J); M.best_J = best_J; M.best_v = best_v; M.hist = hist; M.n_bad = n_bad;
    M.reset = reset;
    hipLaunchKernelGGL(k_plan_mppi_update, dim3((unsigned)P_), dim3(NT), sizeof(float) * (size_t)cfg->K, s, M);
}

// k_plan_grad.  Its tile keeps every hidden layer's output, so the largest shape of the envelope -- 256
// inputs, 4 x 128 units, N = 64 -- takes 128.4 KiB at R = 32 rows and stays below the ceiling; no smaller tile is needed:
static_assert(sizeof(float) * R * (LG_TUBE_MAX_IN + (LG_TUBE_MAX_LIN - 1) * LG_TUBE_MAX_UNITS + LG_PLAN_MAX_N + PLAN_ZS(LG_PLAN_MAX_N) + PLAN_SCN) <=
                  LG_TUBE_ROLLOUT_LDS,
              "k_plan_grad: the envelope's largest tile set must fit the dynamic LDS ceiling");
static_assert(PLAN_ZS(1) >= 6, "k_plan_grad keeps J, two flags and dJ/dv of step 0 in a row of nodes at N = 1 too");
// returns the dynamic LDS of the launch in bytes, or -1 where the kernel's ceiling cannot be set
int64_t tubek_plan_grad(const TubeDev *D, const lg_plan_problem *prob, const PlanGradArgs *A, int64_t B, const lg_plan_scenes *sc,
                        hipStream_t s) {
    PlanDev P;
    memset(&P, 0, sizeof(P));
    plan_scenes_dev(&P, sc);
    TubeDev T;
    memset(&T, 0, sizeof(T));
    if (D) T = *D;
    const bool nn = prob->tube_kind == LG_PLAN_TUBE_NN;
    P.p = *prob;
    P.z0 = A->z0; P.v = A->v; P.e = nn ? A->e : nullptr; P.v_prev = nn ? A->v_prev : nullptr; P.w0 = A->w0; P.offset = A->offset;
    P.cost = A->cost; P.min_clear = A->min_clear;
    P.level = A->level;
    P.Hr = nn ? prob->H_rev : 0;
    P.I = nn ? T.in_dim : 2 * prob->N;
    GradDev G;
    memset(&G, 0, sizeof(G));
    G.v = A->v; G.J = A->J; G.grad = A->grad; G.pen = A->pen; G.m = A->m; G.s = A->s; G.best_J = A->best_J; G.best_v = A->best_v;
    G.hist = A->hist; G.n_bad = A->n_bad;
    G.step = A->step; G.reset = A->reset;
    G.lr = A->lr; G.beta1 = A->beta1; G.beta2 = A->beta2; G.eps = A->eps; G.bc1 = A->bc1; G.bc2 = A->bc2;
    G.rho_g = A->rho_g; G.rho_w = A->rho_w; G.rho_z = A->rho_z;
    for (int d = 0; d < 2; ++d) { G.v_min[d] = prob->rom_v_min[d]; G.v_max[d] = prob->rom_v_max[d]; }
    const size_t bytes = sizeof(float) * (size_t)R * (P.I + (nn ? T.layers * T.units : 0) + prob->N + PLAN_ZS(prob->N)) + (sc ? PLAN_SCN_BYTES : 0);
    static bool ceiling_set[2][64];
    const void *f = sc ? (const void *)k_plan_grad<true> : (const void *)k_plan_grad<false>;
    if (plan_ceiling(f, ceiling_set[sc != nullptr])) return -1;
    const dim3 grid((unsigned)((B + R - 1) / R));
    if (sc) hipLaunchKernelGGL(k_plan_grad<true>, grid, dim3(NT), bytes, s, T, P, G, B);
    else hipLaunchKernelGGL(k_plan_grad<false>, grid, dim3(NT), bytes, s, T, P, G, B);
    return (int64_t)bytes;
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
