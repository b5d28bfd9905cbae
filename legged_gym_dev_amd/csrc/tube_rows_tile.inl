// Body of k_tube_rows and k_tube_rows_sweep (tube_kernels.hip), included inside each kernel so that both compile the same
// statements in kernel context.  Names it takes from the including kernel: TRAIN, LEVEL (template bools), D (the kernel's TubeDev argument, or a
// sweep kernel's TubeDevView of its member: the same field names), S (TubeSplit), rows (const int32_t *), count (int64_t), key (uint64_t), norm (float),
// level (float; read only when LEVEL).  The tile is blockIdx.x.
// LEVEL (lg_tube_cfg.level_input): the last input column is the row's coverage level -- `level` where it is >= 0 (lg_tube_eval_level),
// else drawn per row position by tube_level -- and the row's pinball loss takes it in place of D.alpha.  The split then holds I - 1
// columns; on a horizon handle the window item holds I - 1 columns, the gather's window branch runs for
// c < I - 1 only, and the row's H_fwd outputs share the level.  Every LEVEL statement sits behind the compile-time flag: with
// LEVEL = false the fragment compiles what it compiled before.
// It declares its own shared arrays and may return early, so it must be the last thing in the kernel.
//
// Why a fragment and not a function: as `template <bool TRAIN> __device__ __forceinline__ void tube_rows_tile(const TubeDev &D,
// const TubeSplit &S, rows, count, key, norm)` the body inlined into k_tube_rows<true> / <false> with a different schedule
// (3749 -> 3745 and 2485 -> 2481 instructions and directives of gfx950 assembly; registers reallocated from the first gather
// loop on), and the single kernels were to come out of this refactor unchanged.  The comparison, to repeat after an edit here
// that is meant to leave k_tube_rows alone:
//     hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 --cuda-device-only -S tube_kernels.hip -o new.s   (and old.s at the old commit)
// then, per kernel symbol, the lines between `<symbol>:` and `.Lfunc_end`, comments stripped and the function number taken out
// of the `.LBB<n>_<m>` labels, must be equal.  With the fragment all 20 kernels of the parent commit were.  With the LEVEL flag they
// were not all: TubeDev grew, which moved kernel-argument offsets (DESIGN.md section 10.4 lists every symbol); results are bit-identical.
    extern __shared__ float lds[];
    const int tid = threadIdx.x, I = D.in_dim, O = D.out_dim, U = D.units, L = D.layers;
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds;                     // (R, I) input
    float *H = X + R * I;               // (L, R, U) hidden activations
    float *F = H + L * R * U;           // (R, O) fw, then dLoss/dfw
    float *Y = F + R * O;               // (R, O) target
    float *D0 = Y + R * O, *D1 = D0 + R * U;   // (R, U) deltas, ping-pong
    __shared__ float rowloss[R], rowpos[R], rowerr[R];
    __shared__ int64_t src[R];
    __shared__ int ind[R];

    if (tid < R) {
        const int64_t s = tid < nr ? (int64_t)rows[base + tid] : -1;
        src[tid] = s >= 0 && s < S.rows ? s : -1;     // a row id outside the split reads nothing (zero input and target)
        if (D.horizon && tid < nr) {
            ind[tid] = tube_window(D, key, base + tid);
            D.starts[base + tid] = ind[tid];
        }
        if (LEVEL) {                    // column I - 1 of the row, written here; the gather below leaves it alone
            float lv = 0.f;
            if (tid < nr) {
                lv = level >= 0.f ? level : tube_level(D, key, base + tid);
                D.levels[base + tid] = lv;
            }
            X[tid * I + I - 1] = lv;
        }
    }
    __syncthreads();
    // ---- gather
    for (int e = tid; e < R * I; e += NT) {
        const int r = e / I, c = e - r * I;
        const int64_t s = src[r];
        float x = 0.f;
        if (LEVEL && c == I - 1) continue;
        if (s >= 0) {
            if (!D.horizon) x = S.x[s * (LEVEL ? I - 1 : I) + c];
            else {
                const int t0 = ind[r];
                if (c < D.H_rev) x = S.x[s * D.T + t0 - D.H_rev + c];
                else if (c < D.H_rev + D.nz) x = S.y[(s * D.T + t0) * D.nz + (c - D.H_rev)];
                else {
                    const int q = c - D.H_rev - D.nz, tt = q / D.m;
                    x = S.v[(s * D.T + t0 - D.H_rev + tt) * D.m + (q - tt * D.m)];
                }
            }
        }
        X[e] = x;
    }
    for (int e = tid; e < R * O; e += NT) {
        const int r = e / O, j = e - r * O;
        const int64_t s = src[r];
        Y[e] = s < 0 ? 0.f : D.horizon ? S.x[s * D.T + ind[r] + 1 + j] : S.y[s * O + j];
    }
    __syncthreads();
    // ---- forward: out[r][j] = b[j] + sum_k W[j][k] in[r][k]; lanes over j (coalesced reads of the transposed weights), RB rows each
    for (int li = 0; li <= L; ++li) {
        const int K = D.din[li], N = D.dout[li];
        const float *in = li == 0 ? X : H + (li - 1) * R * U;
        float *out = li == L ? F : H + li * R * U;
        const float *wt = D.wt + D.off_w[li], *b = D.params + D.off_b[li];
        for (int e = tid; e < N * (R / RB); e += NT) {
            const int j = e % N, r0 = (e / N) * RB;
            float acc[RB];
#pragma unroll
            for (int q = 0; q < RB; ++q) acc[q] = 0.f;
            for (int k = 0; k < K; ++k) {
                const float w = wt[(int64_t)k * N + j];
#pragma unroll
                for (int q = 0; q < RB; ++q) acc[q] = fmaf(in[(r0 + q) * K + k], w, acc[q]);
            }
            const float bj = b[j];
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const float z = acc[q] + bj;
                out[(r0 + q) * N + j] = li == L ? z : tube_act(D.act, z, D.sp_beta);
            }
        }
        __syncthreads();
    }
    // ---- loss per row (fixed order inside the row), dLoss/dfw into F
    if (tid < R) {
        float ls = 0.f, pos = 0.f, err = 0.f;
        if (tid < nr) {
            float *f = F + tid * O;
            const float *y = Y + tid * O;
            const float alpha = LEVEL ? X[tid * I + I - 1] : D.alpha;
            if (D.loss == LG_TUBE_LOSS_MSE) {
                for (int j = 0; j < O; ++j) {
                    const float d = f[j] - y[j];
                    ls += d * d;
                    if (TRAIN) f[j] = 2.f * d / norm;
                }
            } else if (D.loss == LG_TUBE_LOSS_SCALAR) {
                for (int j = 0; j < O; ++j) {
                    float dl, dh;
                    const float fw = f[j];
                    if (fw > y[j]) { pos += 1.f; err += fabsf(y[j] - fw); }
                    ls += tube_huber(D.delta, tube_pinball(alpha, y[j], fw, &dl), &dh);
                    if (TRAIN) f[j] = dh * dl / norm;
                }
            } else {                    // VectorTubeLoss: the pinball residuals summed over the row, then Huber
                float lsum = 0.f, dh;
                for (int j = 0; j < O; ++j) {
                    float dl;
                    const float fw = f[j];
                    if (fw > y[j]) { pos += 1.f; err += fabsf(y[j] - fw); }
                    lsum += tube_pinball(alpha, y[j], fw, &dl);
                }
                ls = tube_huber(D.delta, lsum, &dh);
                if (TRAIN)
                    for (int j = 0; j < O; ++j) {
                        float dl;
                        tube_pinball(alpha, y[j], f[j], &dl);
                        f[j] = dh * dl / norm;
                    }
            }
        } else if (TRAIN) {
            for (int j = 0; j < O; ++j) F[tid * O + j] = 0.f;   // rows past the batch contribute nothing
        }
        rowloss[tid] = ls; rowpos[tid] = pos; rowerr[tid] = err;
    }
    __syncthreads();
    if (!TRAIN) {
        if (tid == 0) {
            float a = 0.f, b = 0.f, c = 0.f;
            for (int r = 0; r < R; ++r) { a += rowloss[r]; b += rowpos[r]; c += rowerr[r]; }
            float *p = D.evpart + (size_t)blockIdx.x * 4;
            p[0] = a; p[1] = b; p[2] = c; p[3] = (float)nr;
        }
        return;
    }
    float *g = D.slab + (size_t)blockIdx.x * D.slab_ld;
    if (tid == 0) {
        float a = 0.f;
        for (int r = 0; r < R; ++r) a += rowloss[r];
        g[D.num_params] = a;
    }
    // ---- backward, output layer first
    float *dcur = F, *dnext = D0;
    for (int li = L; li >= 0; --li) {
        const int K = D.din[li], N = D.dout[li];
        const float *a = li == 0 ? X : H + (li - 1) * R * U;
        // weight gradient dW[j][k] = sum_r d[r][j] a[r][k] (lanes over k), bias gradient db[j] = sum_r d[r][j]
        for (int e = tid; e < N * K; e += NT) {
            const int j = e / K, k = e - j * K;
            float acc = 0.f;
#pragma unroll 8
            for (int r = 0; r < R; ++r) acc = fmaf(dcur[r * N + j], a[r * K + k], acc);
            g[D.off_w[li] + e] = acc;
        }
        for (int j = tid; j < N; j += NT) {
            float acc = 0.f;
            for (int r = 0; r < R; ++r) acc += dcur[r * N + j];
            g[D.off_b[li] + j] = acc;
        }
        if (li == 0) break;
        // input gradient through the activation: dprev[r][k] = act'(a[r][k]) sum_j W[j][k] d[r][j] (lanes over k)
        const float *W = D.params + D.off_w[li];
        for (int e = tid; e < K * (R / RB); e += NT) {
            const int k = e % K, r0 = (e / K) * RB;
            float acc[RB];
#pragma unroll
            for (int q = 0; q < RB; ++q) acc[q] = 0.f;
            for (int j = 0; j < N; ++j) {
                const float w = W[(int64_t)j * K + k];
#pragma unroll
                for (int q = 0; q < RB; ++q) acc[q] = fmaf(dcur[(r0 + q) * N + j], w, acc[q]);
            }
#pragma unroll
            for (int q = 0; q < RB; ++q) dnext[(r0 + q) * K + k] = acc[q] * tube_act_grad(D.act, a[(r0 + q) * K + k], D.sp_beta);
        }
        __syncthreads();
        dcur = dnext;
        dnext = dnext == D0 ? D1 : D0;
    }
