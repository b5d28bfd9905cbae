// The tube MLP's device pieces shared by the trainer and inference kernels (tube_kernels.hip) and the planner kernels
// (plan_kernels.hip): the activation, one Linear layer of a row tile forwards and backwards, and the tile constants.
#pragma once
#include "tube_device.h"

#define LG_TUBE_RB 4                    // rows per thread in the forward / input-gradient loops (one weight load, LG_TUBE_RB FMAs)

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

// One Linear layer of a tile of RT rows, shared by k_tube_predict, every k_tube_rollout shape and the planner kernels.  Each output
// is the same chain as in k_tube_rows -- acc = 0, fmaf over k = 0..K-1 in order, + bias, activation -- whatever RT, RB or the
// weights' address space, so a row's result does not depend on the tile it sits in.  w: the layer's transposed weights [k][j];
// b: its bias.  Hidden layers write the activated output to `out` (LDS, (RT, N)); the LAST one writes the raw output to `out`
// (LDS, may be null) and to g[r * gld + j] for the rows r < nr.
template <int RT, int RB, int NT, bool LAST>
__device__ __forceinline__ void tube_layer(int tid, int K, int N, const float *in, const float *w, const float *b, int act, float beta,
                                           float *out, float *g, int64_t gld, int nr) {
    for (int e = tid; e < N * (RT / RB); e += NT) {
        const int j = e % N, r0 = (e / N) * RB;
        float acc[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) acc[q] = 0.f;
#pragma unroll 8                        // eight operand loads in flight per wait: a lone wave per SIMD has nothing else to hide LDS latency behind
        for (int k = 0; k < K; ++k) {
            const float wv = w[k * N + j];
#pragma unroll
            for (int q = 0; q < RB; ++q) acc[q] = fmaf(in[(r0 + q) * K + k], wv, acc[q]);
        }
        const float bj = b[j];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
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

// The hidden layers of a tile, barriers included: layer 0 reads `in`, every later layer its predecessor's output; returns the last
// output (`in` where the model has no hidden layer).  The outputs alternate between H0 and H1, or with KEEP every layer's stays,
// layer li's at H0 + li * RT * units (H1 is not read then).  wsrc / bsrc: the transposed weights and the biases under params' offsets.
template <int RT, int RB, int NT, bool KEEP = false>
__device__ __forceinline__ const float *tube_hidden(int tid, const TubeDev &D, const float *in, const float *wsrc, const float *bsrc,
                                                    float *H0, float *H1) {
    for (int li = 0; li < D.layers; ++li) {
        float *out = KEEP ? H0 + li * RT * D.units : (li & 1 ? H1 : H0);
        tube_layer<RT, RB, NT, false>(tid, D.din[li], D.units, in, wsrc + D.off_w[li], bsrc + D.off_b[li], D.act, D.sp_beta, out, nullptr, 0, 0);
        __syncthreads();
        in = out;
    }
    return in;
}

// One Linear layer backwards for a tile of LG_TUBE_ROWS rows, in place: h (R, K) holds the layer's activated input and takes
// dIn[r][k] = act'(h[r][k]) * sum_j delta[r][j] W[j][k], W = the layer's weights as the parameters keep them ([j][k], lanes across k),
// each sum one fmaf chain from 0 with j ascending.  No thread reads another's h, so in place needs no second buffer.
__device__ __forceinline__ void tube_layer_back(int tid, int K, int No, const float *delta, const float *w, float *h, int act, float beta) {
    for (int e = tid; e < K * (LG_TUBE_ROWS / LG_TUBE_RB); e += LG_TUBE_THREADS) {
        const int k = e % K, r0 = (e / K) * LG_TUBE_RB;
        float acc[LG_TUBE_RB];
#pragma unroll
        for (int q = 0; q < LG_TUBE_RB; ++q) acc[q] = 0.f;
#pragma unroll 8
        for (int j = 0; j < No; ++j) {
            const float wv = w[j * K + k];
#pragma unroll
            for (int q = 0; q < LG_TUBE_RB; ++q) acc[q] = fmaf(delta[(r0 + q) * No + j], wv, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < LG_TUBE_RB; ++q) h[(r0 + q) * K + k] = tube_act_grad(act, h[(r0 + q) * K + k], beta) * acc[q];
    }
}
