// Empirical observation normalisation (legged_hip.h lg_obs_norm_*): running per-column mean and variance
// of the rows handed to a policy, and y = (x - mean) / (std + eps).
//
// Both kernels are launch- and latency-bound and share one shape: a workgroup owns LG_OBS_NORM_ROWS rows x LG_OBS_NORM_COLS columns,
// the lane is the column (a wave reads 256 contiguous bytes of a row), wave w takes rows w, w + 4, ...; the grid is (row block,
// column block, problem): blockIdx.z picks the actor's or the critic's problem, so a pair costs the launches of one.  Workgroups of
// the narrower problem that lie past its width leave before any barrier.  A thread's 16 rows are loaded before the first is used.
//
// k_obs_norm_stats: per (row block, column) the sums S1 = sum(x - k_j), S2 = sum((x - k_j)^2) in double, shifted by k_j = x[0, j]
// (the same shift in every row block, so the partials add; a constant column gives exactly 0 and 0).  The four waves' sums are
// added in wave order through LDS and STORED, one (S1, S2) per (row block, column): no atomics, so the fold below sees the same
// numbers in the same order on every run.
//
// k_obs_norm_apply: in a training compute the 64 lanes of wave 0 first fold the slab over the row blocks in ascending order and
// evaluate the update rule in double from the f32 state; every workgroup of a column block does this on the same numbers in the same
// order and gets the same new state, which it rounds once to f32.  The state is kept twice and the host flips the copies per update:
// this launch reads one copy and its row-block-0 workgroups write the other, so no workgroup reads what another is writing.  Then
// (and in a frozen compute, at once) the workgroup normalises its rows in f32: one subtraction, one addition std + eps, one
// correctly rounded division.
#include "obsnorm_device.h"

#define R LG_OBS_NORM_ROWS
#define C LG_OBS_NORM_COLS
#define RPT (R / LG_ON_WAVES)           // rows per thread: all their loads are issued before the first use, one round trip to memory
#define FOLD 16                         // slab entries the fold keeps in flight; the sums are still added one by one in ascending order

__global__ __launch_bounds__(LG_ON_THREADS) void k_obs_norm_stats(ObsNormDev D) {
    const ObsNormProb P = blockIdx.z ? D.p[1] : D.p[0];
    if (!P.update || (int)blockIdx.y * C >= P.W) return;
    const int lane = threadIdx.x & (C - 1), w = threadIdx.x / C;
    const int j = (int)blockIdx.y * C + lane, W = P.W;
    const long long r0 = (long long)blockIdx.x * R, r1 = min(D.n, r0 + R);
    double s1 = 0.0, s2 = 0.0;
    if (j < W) {
        const float k = P.x[j];
        float xv[RPT];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {                                 // a row past the end reads as k and adds exact zeros
            const long long r = r0 + w + i * LG_ON_WAVES;
            xv[i] = r < r1 ? P.x[r * W + j] : k;
        }
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const double d = (double)xv[i] - (double)k;
            s1 += d;
            s2 += d * d;
        }
    }
    __shared__ double2 part[LG_ON_WAVES][C];
    part[w][lane] = make_double2(s1, s2);
    __syncthreads();
    if (w == 0 && j < W) {
        double2 s = part[0][lane];
        for (int v = 1; v < LG_ON_WAVES; ++v) { s.x += part[v][lane].x; s.y += part[v][lane].y; }
        P.slab[(long long)blockIdx.x * W + j] = s;
    }
}

__global__ __launch_bounds__(LG_ON_THREADS) void k_obs_norm_apply(ObsNormDev D) {
    const ObsNormProb P = blockIdx.z ? D.p[1] : D.p[0];
    if ((int)blockIdx.y * C >= P.W) return;
    const int lane = threadIdx.x & (C - 1), w = threadIdx.x / C;
    const int j = (int)blockIdx.y * C + lane, W = P.W;
    __shared__ float s_mean[C], s_den[C];
    const long long r0 = (long long)blockIdx.x * R, r1 = min(D.n, r0 + R);
    float xv[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {                                     // in flight while wave 0 folds the slab
        const long long r = r0 + w + i * LG_ON_WAVES;
        xv[i] = (j < W && r < r1) ? P.x[r * W + j] : 0.0f;
    }
    if (w == 0) {
        float m = 0.0f, s = 1.0f;
        if (j < W) {
            m = P.st_in[j];
            s = P.st_in[2 * W + j];
            if (P.update) {
                double S1 = 0.0, S2 = 0.0;
                int rb = 0;
                for (; rb + FOLD <= D.nrb; rb += FOLD) {
                    double2 t[FOLD];
#pragma unroll
                    for (int i = 0; i < FOLD; ++i) t[i] = P.slab[(long long)(rb + i) * W + j];
#pragma unroll
                    for (int i = 0; i < FOLD; ++i) { S1 += t[i].x; S2 += t[i].y; }
                }
                for (; rb < D.nrb; ++rb) {
                    const double2 t = P.slab[(long long)rb * W + j];
                    S1 += t.x;
                    S2 += t.y;
                }
                const double n = (double)D.n, a = S1 / n;
                const double mean_x = (double)P.x[j] + a, var_x = fmax(S2 / n - a * a, 0.0);
                const double mean = (double)m, var = (double)P.st_in[W + j];
                const double delta = mean_x - mean, mean_new = mean + P.rate * delta;
                const double var_new = fmax(var + P.rate * (var_x - var + delta * (mean_x - mean_new)), 0.0);
                const float v = (float)var_new;
                m = (float)mean_new;
                s = (float)sqrt((double)v);             // sqrtf(v), correctly rounded (__fsqrt_rn is the bare v_sqrt_f32, 1 ulp)
                if (blockIdx.x == 0) {
                    P.st_out[j] = m;
                    P.st_out[W + j] = v;
                    P.st_out[2 * W + j] = s;
                }
            }
        }
        s_mean[lane] = m;
        s_den[lane] = s + P.eps;
    }
    __syncthreads();
    if (j >= W) return;
    const float mean = s_mean[lane], den = s_den[lane];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const long long r = r0 + w + i * LG_ON_WAVES;
        if (r < r1) P.y[r * W + j] = (xv[i] - mean) / den;
    }
}

static dim3 on_grid(const ObsNormDev *D, int num) {
    int W = D->p[0].W;
    if (num == 2 && D->p[1].W > W) W = D->p[1].W;
    return dim3((unsigned)D->nrb, (unsigned)((W + C - 1) / C), (unsigned)num);
}

extern "C" void obsnormk_stats(const ObsNormDev *D, int num, hipStream_t st) {
    hipLaunchKernelGGL(k_obs_norm_stats, on_grid(D, num), dim3(LG_ON_THREADS), 0, st, *D);
}

extern "C" void obsnormk_apply(const ObsNormDev *D, int num, hipStream_t st) {
    hipLaunchKernelGGL(k_obs_norm_apply, on_grid(D, num), dim3(LG_ON_THREADS), 0, st, *D);
}
