// LSTM front end of rsl_rl's ActorCriticRecurrent (memory_a over the observations, memory_c over the critic observations; one
// nn.LSTM layer each, PyTorch gate order i, f, g, o, biases b_ih and b_hh): the rollout step, the update's forward steps and the
// update's backward-through-time steps.  Both nets run in one launch (blockIdx.z).  The GEMMs here are plain fp32 FMA over LDS
// tiles -- exact fp32 products, the same standard as the MLP's split-bf16 / fp32-MFMA GEMMs.  Each workgroup owns hidden units j
// and all four gate columns of them, so the LSTM cell (forward) and its derivative (backward) are the GEMM's epilogue.
// Host side: ppo_api.hip (lg_ppo_create_recurrent).  DESIGN.md "Recurrent policy" has the schedule.
#include "ppo_launch.h"

#define RB_M 64                  // rows per workgroup
#define RB_K 32                  // reduction chunk staged in LDS
#define RF_J 16                  // forward: hidden units per workgroup (x 4 gates = 64 GEMM columns)
#define RB_J 16                  // backward: hidden units per workgroup.  64 left a 1024-env minibatch at LSTM 256 with 16 x 4 x 2 = 128
                                 // workgroups on 256 CUs (237 us per step launch, profiles/rnn_kernel_stats.txt); 16 gives 512
#define RB_Q (RB_J / 16)         // hidden units per thread

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// gates = [x | h_in] . [W_ih | W_hh]^T + b_ih + b_hh  (or P + h_in . W_hh^T + b_hh), then the cell.  256 threads: thread (tr, tc)
// computes rows 4 tr .. 4 tr + 3 of the four gates of hidden unit j0 + tc.
__global__ void __launch_bounds__(256) k_lstm_fwd(RnnStepArgs a) {
    const RnnNetArgs &n = a.n[blockIdx.z];
    const int H = a.H, M = a.M;
    const int r0 = blockIdx.x * RB_M, j0 = blockIdx.y * RF_J;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    __shared__ float As[RB_K][RB_M + 4];
    __shared__ float Bs[RB_K][4 * RF_J + 1];
    __shared__ int src_sv[RB_M];                     // 1: the row starts from its saved state
    if (tid < RB_M) {
        const int r = r0 + tid;
        src_sv[tid] = !n.h_prev || a.reload_all || (a.reload && r < M && a.reload[r]);
    }
    float acc[4][4];                                 // [gate][row]
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[g][i] = 0.f;
    __syncthreads();
    // phase 0: x . W_ih^T over K columns; phase 1: h_in . W_hh^T over H columns
    for (int ph = n.K > 0 ? 0 : 1; ph < 2; ++ph) {
        const int K = ph == 0 ? n.K : H;
        const float *W = ph == 0 ? n.Wih : n.Whh;
        for (int k0 = 0; k0 < K; k0 += RB_K) {
            for (int e = tid; e < RB_M * RB_K; e += 256) {          // A tile: rows r0.., columns k0.. (coalesced along k)
                const int rr = e / RB_K, kk = e % RB_K, r = r0 + rr, k = k0 + kk;
                float v = 0.f;
                if (r < M && k < K) {
                    if (ph == 0) v = n.X[(size_t)r * n.ldx + k];
                    else {
                        v = src_sv[rr] ? n.h_sv[(size_t)r * H + k] : n.h_prev[(size_t)r * H + k];
                        if (n.h_used && blockIdx.y == 0) n.h_used[(size_t)r * H + k] = v;
                    }
                }
                As[kk][rr] = v;
            }
            for (int e = tid; e < 4 * RF_J * RB_K; e += 256) {      // B tile: gate rows g H + j0 + jj of W, columns k0..
                const int c = e / RB_K, kk = e % RB_K, k = k0 + kk;
                const int g = c / RF_J, jj = c % RF_J;
                Bs[kk][c] = k < K ? W[(size_t)(g * H + j0 + jj) * K + k] : 0.f;
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < RB_K; ++kk) {
                const float4 x = *reinterpret_cast<const float4 *>(&As[kk][4 * tr]);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float w = Bs[kk][g * RF_J + tc];
                    acc[g][0] = fmaf(x.x, w, acc[g][0]);
                    acc[g][1] = fmaf(x.y, w, acc[g][1]);
                    acc[g][2] = fmaf(x.z, w, acc[g][2]);
                    acc[g][3] = fmaf(x.w, w, acc[g][3]);
                }
            }
            __syncthreads();
        }
    }
    const int j = j0 + tc;
    float bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = n.bhh[g * H + j] + (n.P ? 0.f : n.bih[g * H + j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rr = 4 * tr + i, r = r0 + rr;
        if (r >= M) continue;
        float z[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) z[g] = acc[g][i] + bias[g] + (n.P ? n.P[(size_t)r * n.ldp + g * H + j] : 0.f);
        const float c_in = src_sv[rr] ? n.c_sv[(size_t)r * H + j] : n.c_prev[(size_t)r * H + j];
        const float ig = sigm(z[0]), fg = sigm(z[1]), gg = tanhf(z[2]), og = sigm(z[3]);
        const float c = fg * c_in + ig * gg;
        const float h = og * tanhf(c);
        n.h_out[(size_t)r * H + j] = h;
        n.c_out[(size_t)r * H + j] = c;
        if (n.c_used) n.c_used[(size_t)r * H + j] = c_in;
        if (n.gates) {
            float *gp = n.gates + (size_t)r * 4 * H + j;
            gp[0] = ig; gp[H] = fg; gp[2 * H] = gg; gp[3 * H] = og;
        }
    }
}

// dh_t = dh_mlp_t + [step t+1 continues from step t] dG_{t+1} . W_hh, then the cell derivative of step t:
// dG_t (pre-activation gate gradients) and the cell-state carry dc_{t-1} = f_t dc_t, zero where step t reloaded its state.
// 256 threads: thread (tr, tc) owns rows 4 tr .. 4 tr + 3 and hidden units j0 + tc + 16 q, q < RB_Q.
__global__ void __launch_bounds__(256) k_lstm_bwd(RnnBwdArgs a) {
    const RnnBwdNet &n = a.n[blockIdx.z];
    const int H = a.H, M = a.M, H4 = 4 * H;
    const int r0 = blockIdx.x * RB_M, j0 = blockIdx.y * RB_J;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    float acc[RB_Q][4];                              // [q][row]
#pragma unroll
    for (int q = 0; q < RB_Q; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[q][i] = 0.f;
    if (n.dG_next) {
        __shared__ float As[RB_K][RB_M + 4];
        __shared__ float Bs[RB_K][RB_J + 1];
        for (int k0 = 0; k0 < H4; k0 += RB_K) {
            for (int e = tid; e < RB_M * RB_K; e += 256) {
                const int rr = e / RB_K, kk = e % RB_K, r = r0 + rr;
                As[kk][rr] = r < M ? n.dG_next[(size_t)r * H4 + k0 + kk] : 0.f;
            }
            for (int e = tid; e < RB_J * RB_K; e += 256) {          // W_hh rows k0.. (gate rows), columns j0.. (coalesced along j)
                const int kk = e / RB_J, jj = e % RB_J;
                Bs[kk][jj] = j0 + jj < H ? n.Whh[(size_t)(k0 + kk) * H + j0 + jj] : 0.f;
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < RB_K; ++kk) {
                const float4 x = *reinterpret_cast<const float4 *>(&As[kk][4 * tr]);
#pragma unroll
                for (int q = 0; q < RB_Q; ++q) {
                    const float w = Bs[kk][tc + 16 * q];
                    acc[q][0] = fmaf(x.x, w, acc[q][0]);
                    acc[q][1] = fmaf(x.y, w, acc[q][1]);
                    acc[q][2] = fmaf(x.z, w, acc[q][2]);
                    acc[q][3] = fmaf(x.w, w, acc[q][3]);
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + 4 * tr + i;
        if (r >= M) continue;
        const bool carry_in = n.dG_next && !(a.cut_next && a.cut_next[r]);
        const bool cut_here = a.cut_all || (a.cut && a.cut[r]);
#pragma unroll
        for (int q = 0; q < RB_Q; ++q) {
            const int j = j0 + tc + 16 * q;
            if (j >= H) continue;
            const size_t o = (size_t)r * H + j;
            const float dh = n.dh_mlp[o] + (carry_in ? acc[q][i] : 0.f);
            const float *gp = n.gates + (size_t)r * H4 + j;
            const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
            const float tcn = tanhf(n.c_t[o]);
            const float dc = n.dc[o] + dh * og * (1.0f - tcn * tcn);
            float *dg = n.dG + (size_t)r * H4 + j;
            dg[0] = dc * gg * ig * (1.0f - ig);
            dg[H] = dc * n.c_used[o] * fg * (1.0f - fg);
            dg[2 * H] = dc * ig * (1.0f - gg * gg);
            dg[3 * H] = dh * tcn * og * (1.0f - og);
            n.dc[o] = cut_here ? 0.f : dc * fg;
        }
    }
}

// db_ih = db_hh = colsum(dG) over M rows, both nets; rows split over blockIdx.y
__global__ void __launch_bounds__(256) k_lstm_bias_grad(PpoDev P, RnnBiasArgs a) {
    const int col = blockIdx.x * 256 + threadIdx.x, H4 = 4 * a.H;
    if (col >= H4) return;
    const int z = blockIdx.z;
    const int per = (a.M + gridDim.y - 1) / gridDim.y, rb = blockIdx.y * per, re = min(a.M, rb + per);
    float s = 0.f;
    for (int r = rb; r < re; ++r) s += a.dG[z][(size_t)r * H4 + col];
    acc_add(P, a.db_ih[z] + col, s);
    acc_add(P, a.db_hh[z] + col, s);
}

// h = c = 0 for the envs where done is set (all envs: done = nullptr), both nets
__global__ void __launch_bounds__(256) k_lstm_reset(float *h0, float *c0, float *h1, float *c1, const uint8_t *done, int N, int H) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * H) return;
    if (done && !done[e / H]) return;
    h0[e] = 0.f; c0[e] = 0.f; h1[e] = 0.f; c1[e] = 0.f;
}

extern "C" {
void ppok_lstm_fwd(const RnnStepArgs *a, int nz, hipStream_t s) {
    hipLaunchKernelGGL(k_lstm_fwd, dim3((a->M + RB_M - 1) / RB_M, a->H / RF_J, nz), dim3(256), 0, s, *a);
}
void ppok_lstm_bwd(const RnnBwdArgs *a, int nz, hipStream_t s) {
    hipLaunchKernelGGL(k_lstm_bwd, dim3((a->M + RB_M - 1) / RB_M, (a->H + RB_J - 1) / RB_J, nz), dim3(256), 0, s, *a);
}
void ppok_lstm_bias_grad(const PpoDev *P, const RnnBiasArgs *a, hipStream_t s) {
    const int splits = a->M >= 64 * 256 ? 64 : (a->M + 255) / 256;
    hipLaunchKernelGGL(k_lstm_bias_grad, dim3((4 * a->H + 255) / 256, splits > 0 ? splits : 1, 2), dim3(256), 0, s, *P, *a);
}
void ppok_lstm_reset(float *h0, float *c0, float *h1, float *c1, const uint8_t *done, int N, int H, hipStream_t s) {
    const size_t n = (size_t)N * H;
    hipLaunchKernelGGL(k_lstm_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h0, c0, h1, c1, done, N, H);
}
}
