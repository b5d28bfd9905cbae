// PPO kernels for gfx950: action sampling, GAE scan, PPO loss and heads, grad-norm clip + Adam with the KL-adaptive learning
// rate kept on the device (the GEMMs of the ActorCritic forward/backward are ppo_gemm.hip).  Semantics: rsl_rl v1.0.2
// (SURVEY.md Appendix B -- third-party, not in the reference tree; call sites legged_gym/utils/task_registry.py:148-155).
#include <type_traits>

#include "ppo_launch.h"
#include "ppo_loss.h"
#include "ppo_split_bf16.h"

// ------------------------------------------------------------------------------------------------
// PPO.act epilogue: a ~ N(mu, sigma), log-prob, transition store (rsl_rl PPO.act / storage.add)
__global__ void k_act_sample(PpoDev P, const float *__restrict__ obs, const float *__restrict__ critic_obs,
                             const float *__restrict__ mu, const float *__restrict__ val, int t, int64_t act_count, int inject) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P.N, A = P.A, O = P.O;
    if (t >= 0) {
        // storage.add of the observations: rows of step t are one contiguous block, so the copy is flat and coalesced
        // (grid-stride over the whole launch), not one strided row per lane
        const size_t tot = (size_t)N * O, step = (size_t)gridDim.x * blockDim.x;
        for (size_t k = i; k < tot; k += step) P.st_obs[(size_t)t * tot + k] = obs[k];
        if (P.st_critic_obs != P.st_obs) {
            const size_t totc = (size_t)N * P.OC;
            for (size_t k = i; k < totc; k += step) P.st_critic_obs[(size_t)t * totc + k] = critic_obs[k];
        }
    }
    const float *std = P.params + P.off_std;
    // sigma the rollout was sampled with (PPO.update's old_sigma_batch); before the row guard: with fewer envs than
    // action dimensions the lanes i in [N, A) would otherwise leave it at zero and the KL term at inf
    if (i < A && t == 0) P.st_sigma[i] = std[i];
    if (i >= N) return;
    float lp = 0.f;
    for (int a = 0; a < A; ++a) {
        float m = mu[(size_t)i * A + a], s = std[a];
        float z = inject ? P.noise[(size_t)i * A + a] : philox_normal(P.seed, (uint32_t)(P.env_offset + i), (uint64_t)act_count, a);
        float act = m + s * z;
        lp += -((act - m) * (act - m)) / (2.0f * s * s) - logf(s) - 0.9189385332046727f;
        P.act_actions[(size_t)i * A + a] = act;
        P.act_mu[(size_t)i * A + a] = m;
        if (t >= 0) {
            P.st_actions[((size_t)t * N + i) * A + a] = act;
            P.st_mu[((size_t)t * N + i) * A + a] = m;
        }
    }
    const float v = val[i];
    P.act_values[i] = v;
    P.act_log_prob[i] = lp;
    if (t >= 0) {
        P.st_values[(size_t)t * N + i] = v;
        P.st_log_prob[(size_t)t * N + i] = lp;
    }
}

// PPO.process_env_step: rewards += gamma * V * time_outs ; store
__global__ void k_process_step(PpoDev P, const float *__restrict__ rew, const uint8_t *__restrict__ dones,
                               const uint8_t *__restrict__ time_outs, int t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    process_step_body(P, rew[i], dones[i] != 0, time_outs && time_outs[i], t, i);
}

// RolloutStorage.compute_returns: GAE reverse scan, one lane per env; block sums of adv, adv^2
__global__ void __launch_bounds__(256) k_gae(PpoDev P, const float *__restrict__ last_values) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = P.N, T = P.T;
    float s1 = 0.f, s2 = 0.f;
    if (i < N) {
        float adv = 0.f, next_v = last_values[i];
        for (int t = T - 1; t >= 0; --t) {
            const size_t k = (size_t)t * N + i;
            const float nnt = 1.0f - (P.st_dones[k] ? 1.0f : 0.0f);
            const float v = P.st_values[k];
            const float delta = P.st_rewards[k] + nnt * P.gamma * next_v - v;
            adv = delta + nnt * P.gamma * P.lam * adv;
            const float ret = adv + v;
            P.st_returns[k] = ret;
            const float a = ret - v;
            P.st_adv[k] = a;
            s1 += a; s2 += a * a;
            next_v = v;
        }
    }
    __shared__ float r1[256], r2[256];
    r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { r1[threadIdx.x] += r1[threadIdx.x + w]; r2[threadIdx.x] += r2[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        acc_add(P, &P.adv_partial[0], r1[0]);
        acc_add(P, &P.adv_partial[1], r2[0]);
        if (blockIdx.x == 0) P.adv_partial[2] = (float)((size_t)N * T);
    }
}
// advantages = (adv - mean) / (std_unbiased + 1e-8) over all samples (of all ranks after all-reduce)
__global__ void k_adv_normalize(PpoDev P) {
    const size_t n = (size_t)P.N * P.T;
    const float cnt = P.adv_partial[2], mean = P.adv_partial[0] / cnt;
    const float var = fmaxf((P.adv_partial[1] - cnt * mean * mean) / fmaxf(cnt - 1.0f, 1.0f), 0.f);
    const float inv = 1.0f / (sqrtf(var) + 1e-8f);
    for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x)
        P.st_adv[k] = (P.st_adv[k] - mean) * inv;
    if (blockIdx.x == 0 && threadIdx.x == 0) { P.stats[6] = mean; P.stats[7] = sqrtf(var); }
}

// mini_batch_generator's randperm(T*N), drawn on the device once per update and reused by every epoch:
// feistel_perm (lg_device.h) keyed by the update index.  Not torch.randperm's stream (parity with rsl_rl's sample order is unpinned).
__global__ void __launch_bounds__(256) k_randperm(PpoDev P, int n, int half_bits, uint64_t update_idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    P.perm[i] = (int32_t)feistel_perm(P.seed, update_idx, n, half_bits, (uint32_t)i);
}

// mini_batch_generator: rows perm[mb*R .. (mb+1)*R) of the (T*N)-flattened storage
__global__ void k_gather(PpoDev P, int mb) {
    const int R = P.mb_rows, A = P.A, O = P.O;
    const int r = blockIdx.x;
    if (r >= R) return;
    const int src = P.perm[(size_t)mb * R + r];
    for (int k = threadIdx.x; k < O; k += blockDim.x) P.mb_obs[(size_t)r * P.Op + k] = P.st_obs[(size_t)src * O + k];
    if (P.st_critic_obs != P.st_obs)
        for (int k = threadIdx.x; k < P.OC; k += blockDim.x) P.mb_critic_obs[(size_t)r * P.OCp + k] = P.st_critic_obs[(size_t)src * P.OC + k];
    if ((int)threadIdx.x < A) {
        P.mb_actions[(size_t)r * A + threadIdx.x] = P.st_actions[(size_t)src * A + threadIdx.x];
        P.mb_mu[(size_t)r * A + threadIdx.x] = P.st_mu[(size_t)src * A + threadIdx.x];
    }
    if (threadIdx.x == 0) {
        P.mb_scalars[(size_t)r * 4 + 0] = P.st_values[src];
        P.mb_scalars[(size_t)r * 4 + 1] = P.st_returns[src];
        P.mb_scalars[(size_t)r * 4 + 2] = P.st_adv[src];
        P.mb_scalars[(size_t)r * 4 + 3] = P.st_log_prob[src];
    }
}

// same gather, 32 lanes per row moving 16 bytes each (obs, actions, mu as float4s; the four scalars as one float4):
// used when A is a multiple of 4.  An observation width that is not (235 rough terrain, 169 Cassie, 65 trajectory task: the
// storage rows are then not 16-byte aligned) is read a float per lane; the destination rows are Op / OCp long either way.
__device__ __forceinline__ void gather4_block(const PpoDev &P, int mb, int vblock) {
    const int R = P.mb_rows, A4 = P.A / 4;
    const int gid = vblock * 256 + threadIdx.x;
    const int r = gid >> 5, j = gid & 31;
    if (r >= R) return;
    const int src = P.perm[(size_t)mb * R + r];
    const bool own_critic = P.st_critic_obs != P.st_obs;
    const int O4 = (P.O & 3) ? 0 : P.O / 4, OC4 = (own_critic && !(P.OC & 3)) ? P.OC / 4 : 0;
    // eight loads in flight per lane, then the stores (a load / store pair per trip is one L2 round trip per trip: the stores may
    // alias the loads as far as the compiler knows)
    auto row_copy = [&](const float *__restrict__ from, float *__restrict__ to, int n) {
        for (int k0 = j; k0 < n; k0 += 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = from[min(k0 + 32 * u, n - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + 32 * u < n) to[k0 + 32 * u] = v[u];
        }
    };
    if (P.O & 3) row_copy(P.st_obs + (size_t)src * P.O, P.mb_obs + (size_t)r * P.Op, P.O);
    if (own_critic && (P.OC & 3)) row_copy(P.st_critic_obs + (size_t)src * P.OC, P.mb_critic_obs + (size_t)r * P.OCp, P.OC);
    for (int k = j; k < O4 + OC4 + 2 * A4 + 1; k += 32) {
        if (k < O4) reinterpret_cast<float4 *>(P.mb_obs)[(size_t)r * (P.Op / 4) + k] = reinterpret_cast<const float4 *>(P.st_obs)[(size_t)src * O4 + k];
        else if (k < O4 + OC4) reinterpret_cast<float4 *>(P.mb_critic_obs)[(size_t)r * (P.OCp / 4) + (k - O4)] = reinterpret_cast<const float4 *>(P.st_critic_obs)[(size_t)src * OC4 + (k - O4)];
        else if (k < O4 + OC4 + A4) reinterpret_cast<float4 *>(P.mb_actions)[(size_t)r * A4 + (k - O4 - OC4)] = reinterpret_cast<const float4 *>(P.st_actions)[(size_t)src * A4 + (k - O4 - OC4)];
        else if (k < O4 + OC4 + 2 * A4) reinterpret_cast<float4 *>(P.mb_mu)[(size_t)r * A4 + (k - O4 - OC4 - A4)] = reinterpret_cast<const float4 *>(P.st_mu)[(size_t)src * A4 + (k - O4 - OC4 - A4)];
        else reinterpret_cast<float4 *>(P.mb_scalars)[r] = make_float4(P.st_values[src], P.st_returns[src], P.st_adv[src], P.st_log_prob[src]);
    }
}
__global__ void __launch_bounds__(256) k_gather4(PpoDev P, int mb) { gather4_block(P, mb, blockIdx.x); }

// PPO.update loss for one minibatch: surrogate, clipped value loss, entropy bonus, KL(old || new);
// emits d loss / d mu (R x A), d loss / d value (R), and block-reduced d loss / d std, bias grads
// of both heads and the loss statistics.
__global__ void __launch_bounds__(256) k_loss(PpoDev P, const float *__restrict__ mu_new, const float *__restrict__ v_new,
                                              float *__restrict__ dmu, float *__restrict__ dval) {
    const int R = P.mb_rows, A = P.A;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const float *std = P.params + P.off_std;
    const float invR = 1.0f / (float)R;
    // per-thread partials at the fixed slots of ppo_loss.h
    constexpr int MA = LG_PPO_MAX_A;
    float part[PPO_NSUMS];
#pragma unroll
    for (int k = 0; k < PPO_NSUMS; ++k) part[k] = 0.f;
    // the two logarithms of every action dimension depend on sigma only: once per block instead of once per row
    __shared__ float s_logs[MA], s_logr[MA];
    if ((int)threadIdx.x < A) {
        const float s = std[threadIdx.x], so = P.st_sigma[threadIdx.x];
        s_logs[threadIdx.x] = logf(s);
        s_logr[threadIdx.x] = logf(s / so + 1.e-5f);
    }
    __syncthreads();
    if (r < R) {
        const float4 sc = reinterpret_cast<const float4 *>(P.mb_scalars)[r];
        const float v_old = sc.x, ret = sc.y, adv = sc.z, lp_old = sc.w;
        float lp = 0.f, kl = 0.f, dd[MA];
        // The Gaussian terms stay here, in division form: the fused heads (ppo_loss.h) multiply by staged reciprocals, which
        // rounds differently, and this path keeps its last bits.
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            dd[a] = 0.f;
            if (a < A) {
                const float s = std[a], so = P.st_sigma[a];
                const float m = mu_new[(size_t)r * A + a], mo = P.mb_mu[(size_t)r * A + a];
                const float d = P.mb_actions[(size_t)r * A + a] - m;
                dd[a] = d;
                lp += -(d * d) / (2.0f * s * s) - s_logs[a] - 0.9189385332046727f;
                kl += s_logr[a] + (so * so + (mo - m) * (mo - m)) / (2.0f * s * s) - 0.5f;
            }
        }
        const PpoSurrogate sg = ppo_surrogate(P.clip, lp, lp_old, adv, invR);
#pragma unroll
        for (int a = 0; a < MA; ++a)
            if (a < A) {
                const float s = std[a], d = dd[a];
                const float g = sg.dl_dlp * d / (s * s);
                dmu[(size_t)r * A + a] = g;
                part[PPO_SUM_DBIAS_ACTOR + a] = g;
                part[PPO_SUM_DSTD + a] = sg.dl_dlp * (d * d / (s * s * s) - 1.0f / s) - P.entropy_coef * invR / s;
            }
        const PpoValue vl = ppo_value(P.clipped_value, P.clip, v_new[r], v_old, ret);
        const float dv = vl.dv * (P.value_coef * invR);
        dval[r] = dv;
        part[PPO_SUM_DBIAS_CRITIC] = dv;
        part[PPO_SUM_KL] = kl;
        part[PPO_SUM_VLOSS] = vl.lv;
        part[PPO_SUM_SLOSS] = fmaxf(sg.s1, sg.s2);
    }
    // wave64 butterfly per partial, one LDS slot per wave (summed in wave order below), one global atomic per block and partial
    __shared__ float red[4][PPO_NSUMS];
#pragma unroll
    for (int k = 0; k < PPO_NSUMS; ++k) {
        if (ppo_sum_live(k, A)) {
            float v = part[k];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
        }
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < PPO_NSUMS && ppo_sum_live(k, A)) {
        const float v = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        acc_add(P, ppo_sum_dest(P, k, P.off_bias_actor_head, P.off_bias_critic_head), v);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused head: [actor head 128->A | critic head 128->1] forward + PPO loss + head backward, one
// workgroup per 64 minibatch rows.  Replaces four launches (head GEMM, k_loss, head weight-gradient
// GEMM, head input-gradient GEMM) whose matrices are too thin for the MFMA tiles: the last hidden
// activations of both nets are staged once in LDS and reused for mu/V, for d(loss)/d(act3) and for
// the outer-product weight gradients.  H3 = last hidden width: 64 or 32 (128 wide: k_head_net + k_head_finish below).
#define HEAD_ROWS 64
#define HEAD_GRID 192
#define HEAD_NET_GRID 384                                  // workgroups per network of k_head_net (= scratch rows per network)
#define HEAD_PART_STRIDE(H3) ((LG_PPO_MAX_A + 1) * (H3) + PPO_NSUMS)
template <int H3>
__global__ void __launch_bounds__(256) k_head_fused(PpoDev P, const float *__restrict__ xa_g, const float *__restrict__ xc_g,
                                                    float *__restrict__ dza_g, float *__restrict__ dzc_g, int64_t w_a, int64_t b_a,
                                                    int64_t w_c, int64_t b_c, int64_t b_prev_a, int64_t b_prev_c) {
    constexpr int MA = LG_PPO_MAX_A, LDX = H3 + 1, NH = 256 / H3;   // NH row groups run concurrently in the backward part
    const int R = P.mb_rows, A = P.A, tid = threadIdx.x;
    __shared__ float xa[HEAD_ROWS * LDX], xc[HEAD_ROWS * LDX];
    __shared__ float wa[MA * H3], wc[H3];
    __shared__ float mus[HEAD_ROWS][MA + 1], dmus[HEAD_ROWS][MA + 1];    // [..][MA]: value / d value
    // per-action constants of the Gaussian terms (ppo_gauss)
    __shared__ float red[PPO_NSUMS], s_so2[MA], s_i2s2[MA], s_is2[MA], s_is[MA], s_lgs[MA], s_klc[MA];
    if (tid < MA) {
        const PpoGauss gs = ppo_gauss(tid < A ? P.params[P.off_std + tid] : 1.f, tid < A ? P.st_sigma[tid] : 1.f);
        s_so2[tid] = gs.so2; s_i2s2[tid] = gs.i2s2; s_is2[tid] = gs.is2; s_is[tid] = gs.is;
        s_lgs[tid] = gs.lgs; s_klc[tid] = gs.klc;
    }
    for (int i = tid; i < A * H3; i += 256) wa[i] = P.params[w_a + i];
    for (int i = tid; i < H3; i += 256) wc[i] = P.params[w_c + i];
    if (tid < PPO_NSUMS) red[tid] = 0.f;
    // backward accumulators of this thread's column, kept in registers across all row tiles of the block
    const int c = tid % H3, half = tid / H3;
    float dwa[MA], dwc = 0.f, dba = 0.f, dbc = 0.f, part[PPO_NSUMS];
#pragma unroll
    for (int a = 0; a < MA; ++a) dwa[a] = 0.f;
#pragma unroll
    for (int k = 0; k < PPO_NSUMS; ++k) part[k] = 0.f;
    const int ntiles = (R + HEAD_ROWS - 1) / HEAD_ROWS;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int r0 = tile * HEAD_ROWS;
        __syncthreads();                                   // previous tile fully consumed (also covers the weight staging)
        {   // stage both activation tiles: unconditional 16-byte loads from clamped rows (rows past R are
            // never used: every consumer below checks r < R), issued as one batch
            constexpr int NV = HEAD_ROWS * H3 / 4 / 256;
            float4 va[NV], vc[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int i = tid + v * 256, r = i / (H3 / 4), c4 = i % (H3 / 4);
                const size_t row = (size_t)min(r0 + r, R - 1);
                va[v] = *reinterpret_cast<const float4 *>(xa_g + row * H3 + 4 * c4);
                vc[v] = *reinterpret_cast<const float4 *>(xc_g + row * H3 + 4 * c4);
            }
            __builtin_amdgcn_sched_barrier(0);       // keep the 2*NV loads in flight together (hipcc otherwise pairs each with its LDS store)
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int i = tid + v * 256, r = i / (H3 / 4), c4 = i % (H3 / 4);
                float *da = xa + r * LDX + 4 * c4, *dc = xc + r * LDX + 4 * c4;
                da[0] = va[v].x; da[1] = va[v].y; da[2] = va[v].z; da[3] = va[v].w;
                dc[0] = vc[v].x; dc[1] = vc[v].y; dc[2] = vc[v].z; dc[3] = vc[v].w;
            }
        }
        __syncthreads();
        {   // head forward: lane = row (conflict-free x reads, broadcast weight reads); wave w -> outputs w, w+4, w+8, w+12
            const int r = tid & 63, w = tid >> 6;
            const float *x = xa + r * LDX;
            float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
            const float *w0 = wa + (w < A ? w : 0) * H3, *w1 = wa + (w + 4 < A ? w + 4 : 0) * H3;
            const float *w2 = wa + (w + 8 < A ? w + 8 : 0) * H3, *w3 = wa + (w + 12 < A ? w + 12 : 0) * H3;
#pragma unroll 8
            for (int k = 0; k < H3; ++k) {
                const float xv = x[k];
                o0 += xv * w0[k]; o1 += xv * w1[k]; o2 += xv * w2[k]; o3 += xv * w3[k];
            }
            if (w < A) mus[r][w] = o0 + P.params[b_a + w];
            if (w + 4 < A) mus[r][w + 4] = o1 + P.params[b_a + w + 4];
            if (w + 8 < A) mus[r][w + 8] = o2 + P.params[b_a + w + 8];
            if (w + 12 < A) mus[r][w + 12] = o3 + P.params[b_a + w + 12];
            if (w == 3) {                                  // wave 3 carries the fewest actor outputs: it also does the value
                float sacc = P.params[b_c];
                const float *y = xc + r * LDX;
#pragma unroll 8
                for (int k = 0; k < H3; ++k) sacc += y[k] * wc[k];
                mus[r][MA] = sacc;
            }
        }
        __syncthreads();
        // loss of one row (ppo_loss.h; the Gaussian terms multiply by the staged reciprocals where k_loss divides, so the two
        // paths differ in the last bits), wave 0 only; partials stay in registers
        if (tid < HEAD_ROWS) {
            const int r = r0 + tid;
            const float invR = 1.0f / (float)R;
            float dvl = 0.f;
#pragma unroll
            for (int a = 0; a < MA; ++a) dmus[tid][a] = 0.f;
            // operands of this row: unconditional loads from a clamped row / action index, issued up front
            const size_t rr = (size_t)min(r, R - 1);
            const float4 sc = reinterpret_cast<const float4 *>(P.mb_scalars)[rr];
            float act_r[MA], mo_r[MA];
#pragma unroll
            for (int a = 0; a < MA; ++a) {
                const int ac = min(a, A - 1);
                act_r[a] = P.mb_actions[rr * A + ac];
                mo_r[a] = P.mb_mu[rr * A + ac];
            }
            if (r < R) {
                const float v_old = sc.x, ret = sc.y, adv = sc.z, lp_old = sc.w;
                float lp = 0.f, kl = 0.f, dd[MA];
#pragma unroll
                for (int a = 0; a < MA; ++a) {
                    dd[a] = 0.f;
                    if (a < A) {
                        const float m = mus[tid][a], mo = mo_r[a];
                        const float d = act_r[a] - m;
                        dd[a] = d;
                        lp += ppo_lp_term(d, s_i2s2[a], s_lgs[a]);
                        kl += ppo_kl_term(mo, m, s_so2[a], s_i2s2[a], s_klc[a]);
                    }
                }
                const PpoSurrogate sg = ppo_surrogate(P.clip, lp, lp_old, adv, invR);
#pragma unroll
                for (int a = 0; a < MA; ++a)
                    if (a < A) {
                        const float g = ppo_dmu(sg.dl_dlp, dd[a], s_is2[a]);
                        dmus[tid][a] = g;
                        part[PPO_SUM_DBIAS_ACTOR + a] += g;
                        part[PPO_SUM_DSTD + a] += ppo_dstd(sg.dl_dlp, dd[a], s_is2[a], s_is[a], P.entropy_coef * invR);
                    }
                const PpoValue vl = ppo_value(P.clipped_value, P.clip, mus[tid][MA], v_old, ret);
                dvl = vl.dv * P.value_coef * invR;
                part[PPO_SUM_DBIAS_CRITIC] += dvl;
                part[PPO_SUM_KL] += kl;
                part[PPO_SUM_VLOSS] += vl.lv;
                part[PPO_SUM_SLOSS] += fmaxf(sg.s1, sg.s2);
            }
            dmus[tid][MA] = dvl;
        }
        __syncthreads();
        // head backward for column c: dz3 = (dmu . W) * ELU'(act3) ; dW += dmu^T act3 ; colsum(dz3) -> previous bias grad
        if (half < NH) {
            float wcol[MA];
#pragma unroll
            for (int a = 0; a < MA; ++a) wcol[a] = a < A ? wa[a * H3 + c] : 0.f;
            const float wcc = wc[c];
            for (int r = half; r < HEAD_ROWS && r0 + r < R; r += NH) {
                float g = 0.f;
                const float x = xa[r * LDX + c], y = xc[r * LDX + c];
#pragma unroll
                for (int a = 0; a < MA; ++a) {
                    const float dm = dmus[r][a];
                    g += dm * wcol[a];
                    dwa[a] += dm * x;
                }
                const float dz = g * (x > 0.f ? 1.0f : x + 1.0f);
                const float dv = dmus[r][MA];
                const float dzc = dv * wcc * (y > 0.f ? 1.0f : y + 1.0f);
                dza_g[(size_t)(r0 + r) * H3 + c] = dz;
                dzc_g[(size_t)(r0 + r) * H3 + c] = dzc;
                dwc += dv * y;
                dba += dz;
                dbc += dzc;
            }
        }
    }
    // ---- flush: loss partials of the row lanes (wave 0) transposed through LDS (lane r writes column r, thread k adds row k:
    // a 36 x 6 shuffle butterfly on one wave is several times slower), then column accumulators reduced over the NH row groups
    __shared__ float ptmp[PPO_NSUMS * HEAD_ROWS];
    if (tid < HEAD_ROWS) {
#pragma unroll
        for (int k = 0; k < PPO_NSUMS; ++k) ptmp[k * HEAD_ROWS + tid] = part[k];
    }
    __syncthreads();
    if (tid < PPO_NSUMS && ppo_sum_live(tid, A)) {
        const int k = tid;
        float v = 0.f;
        for (int r = 0; r < HEAD_ROWS; ++r) v += ptmp[k * HEAD_ROWS + r];
        acc_add(P, ppo_sum_dest(P, k, b_a, b_c), v);
    }
    float *acc = xa;                                      // reuse the tile buffer: [MA + 3][NH][H3]
    __syncthreads();
    if (half < NH) {
#pragma unroll
        for (int a = 0; a < MA; ++a) acc[(a * NH + half) * H3 + c] = dwa[a];
        acc[((MA + 0) * NH + half) * H3 + c] = dwc;
        acc[((MA + 1) * NH + half) * H3 + c] = dba;
        acc[((MA + 2) * NH + half) * H3 + c] = dbc;
    }
    __syncthreads();
    for (int i = tid; i < (MA + 3) * H3; i += 256) {
        const int q = i / H3, cc = i % H3;
        float v = 0.f;
        for (int h = 0; h < NH; ++h) v += acc[(q * NH + h) * H3 + cc];
        if (q < MA) { if (q < A) acc_add(P, &P.grads[w_a + (int64_t)q * H3 + cc], v); }
        else if (q == MA) acc_add(P, &P.grads[w_c + cc], v);
        else if (q == MA + 1) acc_add(P, &P.grads[b_prev_a + cc], v);
        else acc_add(P, &P.grads[b_prev_c + cc], v);
    }
}

// The same fused head with one network per workgroup (blockIdx.y: 0 actor, 1 critic).  The two heads share nothing but the
// row index -- surrogate / entropy / KL need mu only, the value loss needs V only -- so each workgroup stages ONE activation
// tile: 50 KB of LDS instead of 84, three workgroups per CU (all 768 of a 24576-row minibatch resident).  Used for H3 = 128, where
// k_head_fused is one wave per SIMD.
//
// Round 4: the arithmetic is the old kernel's, the operand paths are not.  With a row per lane and the head weights and the rows'
// output gradients read from LDS for every multiply-add, the kernel moved 1.25 LDS dwords per FMA and the twelve waves of a CU queued
// on the LDS port for 13 us of its 29.  Now every operand that is uniform over a wave comes through the SCALAR path:
//   forward   lane = row, wave = a quarter of k; the weights are wave-uniform and arrive by s_load from global memory (K$), 32 x reads
//             per lane instead of 640; the four partial sums per (row, output) meet in LDS, added in a fixed order
//   loss      every wave evaluates the 64 rows (lane = row), so each wave holds d loss / d out of all rows in its own registers; wave 0
//             alone accumulates the row sums
//   backward  wave = every fourth row, lane = columns (lane, lane + 64): a row's output gradients are v_readlane'd into SGPRs and feed
//             the multiply-adds as scalar operands; one LDS read per column and row
template <int H3, int NA>
__global__ void __launch_bounds__(256, 3) k_head_net(PpoDev P, const float *__restrict__ xa_g, const float *__restrict__ xc_g,
                                                     float *__restrict__ dza_g, float *__restrict__ dzc_g, const float *__restrict__ wa_g,
                                                     const float *__restrict__ wc_g, int64_t b_a, int64_t b_c) {
    static_assert(H3 == 128, "lane = columns (lane, lane + 64); wave = a quarter of k");
    static_assert(NA <= LG_PPO_MAX_A, "NA = the action count the register arrays are sized for (>= P.A); the scratch row keeps LG_PPO_MAX_A slots");
    constexpr int MA = LG_PPO_MAX_A, LDX = H3 + 1, NWV = 4, KQ = H3 / NWV;
    const int R = P.mb_rows, A = P.A, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool actor = blockIdx.y == 0;
    const float *__restrict__ x_g = actor ? xa_g : xc_g;
    const float *__restrict__ w_g = actor ? wa_g : wc_g;
    float *__restrict__ dz_g = actor ? dza_g : dzc_g;
    const int nout = actor ? A : 1;
    // x tile, then the partial outputs [NWV][HEAD_ROWS][NA + 1]; after the tile loop the same floats hold the column sums and the row sums.
    // s_am: the tile's rows of the minibatch's actions and old means, staged with the tile (the loss lanes' own loads of them sank to
    // their use under the 168-register cap and cost the actor's loss phase 6 us of exposed latency: stamps, round 4)
    // (52.9 KB in all: three workgroups per CU is 158.8 of the 160 KB -- one more KB and a third of the workgroups start a round late)
    constexpr int OP = NA + 1, NBUF = HEAD_ROWS * LDX + NWV * HEAD_ROWS * OP;
    __shared__ float buf[NBUF];
    __shared__ float s_am[2 * HEAD_ROWS * NA];
    __shared__ float s_so2[MA], s_i2s2[MA], s_is2[MA], s_is[MA], s_lgs[MA], s_klc[MA], s_bias[MA];
    float *x = buf, *outs_p = buf + HEAD_ROWS * LDX;
    if (tid < MA) {
        const PpoGauss gs = ppo_gauss(tid < A ? P.params[P.off_std + tid] : 1.f, tid < A ? P.st_sigma[tid] : 1.f);
        s_so2[tid] = gs.so2; s_i2s2[tid] = gs.i2s2; s_is2[tid] = gs.is2; s_is[tid] = gs.is;
        s_lgs[tid] = gs.lgs; s_klc[tid] = gs.klc;
        s_bias[tid] = tid < nout ? P.params[(actor ? b_a : b_c) + tid] : 0.f;
    }
    float wcol0[NA], wcol1[NA];                             // the head weights of this lane's two columns (backward)
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        wcol0[a] = a < nout ? w_g[a * H3 + lane] : 0.f;
        wcol1[a] = a < nout ? w_g[a * H3 + lane + 64] : 0.f;
    }
    float dw0[NA], dw1[NA], db0 = 0.f, db1 = 0.f, part[PPO_NSUMS];
#pragma unroll
    for (int a = 0; a < NA; ++a) { dw0[a] = 0.f; dw1[a] = 0.f; }
#pragma unroll
    for (int k = 0; k < PPO_NSUMS; ++k) part[k] = 0.f;
    const int ntiles = (R + HEAD_ROWS - 1) / HEAD_ROWS;
    const float invR = 1.0f / (float)R;
#ifdef LG_HEAD_STAMPS
    unsigned long long ts[8]; ts[0] = __builtin_amdgcn_s_memrealtime();
#define HSTAMP(k) ts[k] = __builtin_amdgcn_s_memrealtime()
#else
#define HSTAMP(k) do { } while (0)
#endif
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int r0 = tile * HEAD_ROWS;
        // what the loss needs of this lane's row, requested before anything waits
        const int r = r0 + lane;
        const size_t rr = (size_t)min(r, R - 1);
        const float4 sc = reinterpret_cast<const float4 *>(P.mb_scalars)[rr];
        __syncthreads();
        if (actor) {                                        // rows r0 .. r0 + 63 of [R][A]: one contiguous run
            const size_t base = (size_t)r0 * A, lim = (size_t)R * A;
            for (int i = tid; i < HEAD_ROWS * A; i += 256) {
                const size_t g = base + i < lim ? base + i : lim - 1;
                s_am[i] = P.mb_actions[g];
                s_am[HEAD_ROWS * NA + i] = P.mb_mu[g];
            }
        }
        {
            constexpr int NV = HEAD_ROWS * H3 / 4 / 256;
            float4 vx[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int i = tid + v * 256, rw = i / (H3 / 4), c4 = i % (H3 / 4);
                vx[v] = *reinterpret_cast<const float4 *>(x_g + (size_t)min(r0 + rw, R - 1) * H3 + 4 * c4);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int i = tid + v * 256, rw = i / (H3 / 4), c4 = i % (H3 / 4);
                float *d = x + rw * LDX + 4 * c4;
                d[0] = vx[v].x; d[1] = vx[v].y; d[2] = vx[v].z; d[3] = vx[v].w;
            }
        }
        __syncthreads();
        HSTAMP(1);
        {   // forward: lane = row, wave = k quarter; weights through the scalar cache.  One guard per output (not per multiply-add group):
            // the scheduler works inside basic blocks, and a row's 32 activations stay in registers across the outputs
            const float *xr = x + lane * LDX + KQ * wv;
            const float *__restrict__ wq = w_g + KQ * wv;
            float xv[KQ];
#pragma unroll
            for (int j = 0; j < KQ; ++j) xv[j] = xr[j];
#pragma unroll
            for (int a = 0; a < NA; ++a)
                if (a < nout) {
                    float o = 0.f;
#pragma unroll
                    for (int j = 0; j < KQ; ++j) o = __builtin_fmaf(xv[j], wq[a * H3 + j], o);
                    outs_p[(wv * HEAD_ROWS + lane) * OP + a] = o;
                }
        }
        __syncthreads();
        HSTAMP(2);
        float dout[NA];                                     // d loss / d out of row `lane`, in every wave
#pragma unroll
        for (int a = 0; a < NA; ++a) dout[a] = 0.f;
        {
            float outv[NA];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                outv[a] = 0.f;
                if (a < nout) {
                    const float *op = outs_p + lane * OP + a;
                    constexpr int QS = HEAD_ROWS * OP;
                    outv[a] = (op[0] + op[QS]) + (op[2 * QS] + op[3 * QS]);
                }
            }
            const bool sums = wv == 0;                      // the row sums are wave 0's
            if (actor) {
                if (r < R) {
                    const float adv = sc.z, lp_old = sc.w;
                    float lp = 0.f, kl = 0.f, dd[NA];
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        dd[a] = 0.f;
                        if (a < A) {
                            const float m = outv[a] + s_bias[a], mo = s_am[HEAD_ROWS * NA + lane * A + a];
                            const float d = s_am[lane * A + a] - m;
                            dd[a] = d;
                            lp += ppo_lp_term(d, s_i2s2[a], s_lgs[a]);
                            kl += ppo_kl_term(mo, m, s_so2[a], s_i2s2[a], s_klc[a]);
                        }
                    }
                    const PpoSurrogate sg = ppo_surrogate(P.clip, lp, lp_old, adv, invR);
#pragma unroll
                    for (int a = 0; a < NA; ++a)
                        if (a < A) {
                            const float g = ppo_dmu(sg.dl_dlp, dd[a], s_is2[a]);
                            dout[a] = g;
                            if (sums) {
                                part[PPO_SUM_DBIAS_ACTOR + a] += g;
                                part[PPO_SUM_DSTD + a] += ppo_dstd(sg.dl_dlp, dd[a], s_is2[a], s_is[a], P.entropy_coef * invR);
                            }
                        }
                    if (sums) { part[PPO_SUM_KL] += kl; part[PPO_SUM_SLOSS] += fmaxf(sg.s1, sg.s2); }
                }
            } else if (r < R) {
                const PpoValue vl = ppo_value(P.clipped_value, P.clip, s_bias[0] + outv[0], sc.x, sc.y);
                const float dvl = vl.dv * P.value_coef * invR;
                dout[0] = dvl;
                if (sums) { part[PPO_SUM_DBIAS_CRITIC] += dvl; part[PPO_SUM_VLOSS] += vl.lv; }
            }
        }
        // backward for rows wv, wv + 4, ...: dz = (dout . W) act'(x); dW += dout^T x; the row's dout as scalars.  Written twice: without
        // the per-output guard when the register arrays are exactly as long as the head is wide (the actor of every registered task)
        HSTAMP(3);
        auto backward = [&](auto full) {
            for (int rw = wv; rw < HEAD_ROWS && r0 + rw < R; rw += NWV) {
                const float xv0 = x[rw * LDX + lane], xv1 = x[rw * LDX + lane + 64];
                float g0 = 0.f, g1 = 0.f;
#pragma unroll
                for (int a = 0; a < NA; ++a)
                    if (decltype(full)::value || a < nout) {
                        const float sa = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dout[a]), rw));
                        g0 = __builtin_fmaf(sa, wcol0[a], g0); g1 = __builtin_fmaf(sa, wcol1[a], g1);
                        dw0[a] = __builtin_fmaf(sa, xv0, dw0[a]); dw1[a] = __builtin_fmaf(sa, xv1, dw1[a]);
                    }
                const float dz0 = g0 * (xv0 > 0.f ? 1.0f : xv0 + 1.0f), dz1 = g1 * (xv1 > 0.f ? 1.0f : xv1 + 1.0f);
                float *dzr = dz_g + (size_t)(r0 + rw) * H3;
                dzr[lane] = dz0; dzr[lane + 64] = dz1;
                db0 += dz0; db1 += dz1;
            }
        };
        if (nout == NA) backward(std::true_type{}); else backward(std::false_type{});
        HSTAMP(4);
    }
    // Sums over the rows of this workgroup leave through a scratch row, not through atomics: 768 workgroups adding into the
    // same few dozen addresses serialise in L2 (24 us of the first version's 46 were that queue).  k_head_finish folds the rows.
    // Column sums: the four waves' partials [MA + 1][NWV][H3] meet in LDS; the loss lanes' row sums (wave 0) are transposed through
    // LDS (lane r writes its partials as column r, thread k adds the 64 entries of row k).
    float *acc = buf, *ptmp = buf + (MA + 1) * NWV * H3;
    static_assert((MA + 1) * NWV * H3 + PPO_NSUMS * HEAD_ROWS <= NBUF, "sums fit in the tile buffer");
    __syncthreads();                                        // every wave is done with the tile
#pragma unroll
    for (int a = 0; a < MA; ++a) {
        acc[(a * NWV + wv) * H3 + lane] = a < NA ? dw0[a < NA ? a : 0] : 0.f;
        acc[(a * NWV + wv) * H3 + lane + 64] = a < NA ? dw1[a < NA ? a : 0] : 0.f;
    }
    acc[(MA * NWV + wv) * H3 + lane] = db0;
    acc[(MA * NWV + wv) * H3 + lane + 64] = db1;
    if (tid < HEAD_ROWS) {
#pragma unroll
        for (int k = 0; k < PPO_NSUMS; ++k) ptmp[k * HEAD_ROWS + tid] = part[k];
    }
    float *__restrict__ prow = P.head_part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * HEAD_PART_STRIDE(H3);
    __syncthreads();
    if (tid < PPO_NSUMS) {
        float v = 0.f;
        for (int rw = 0; rw < HEAD_ROWS; ++rw) v += ptmp[tid * HEAD_ROWS + rw];
        prow[(MA + 1) * H3 + tid] = v;
    }
    for (int i = tid; i < (MA + 1) * H3; i += 256) {
        const int q = i / H3, cc = i % H3;
        const float *ap = acc + q * NWV * H3 + cc;
        prow[i] = (ap[0] + ap[H3]) + (ap[2 * H3] + ap[3 * H3]);
    }
#ifdef LG_HEAD_STAMPS
    HSTAMP(5);
    if (tid == 0 && (blockIdx.x % 97) == 0)
        printf("head wg %d net %d: stage %llu fwd %llu loss %llu bwd %llu sums %llu (x10 ns) start %llu\n", blockIdx.x, blockIdx.y, ts[1] - ts[0], ts[2] - ts[1],
               ts[3] - ts[2], ts[4] - ts[3], ts[5] - ts[4], ts[0] % 100000ull);
#endif
}

// Folds the scratch rows of k_head_net into the gradient buffer: thread = one sum, blockIdx.y = a chunk of the rows,
// blockIdx.z = the network; HEAD_FIN_CHUNKS-way atomics instead of 768-way.
#define HEAD_FIN_CHUNKS 16
template <int H3>
__global__ void __launch_bounds__(256) k_head_finish(PpoDev P, int nrows, int64_t w_a, int64_t b_a, int64_t w_c, int64_t b_c, int64_t b_prev_a,
                                                     int64_t b_prev_c) {
    constexpr int MA = LG_PPO_MAX_A, NW = (MA + 1) * H3, NTOT = NW + PPO_NSUMS;
    const int i = blockIdx.x * 256 + threadIdx.x, A = P.A;
    if (i >= NTOT) return;
    const bool actor = blockIdx.z == 0;
    const int nout = actor ? A : 1;
    // drop the sums nobody consumes before reading anything
    if (i < NW) { if (i / H3 < MA && i / H3 >= nout) return; }
    else {
        const int k = i - NW;
        if (ppo_sum_of_actor(k) != actor || !ppo_sum_live(k, A)) return;
    }
    const int r0 = (int)((long)nrows * blockIdx.y / HEAD_FIN_CHUNKS), r1 = (int)((long)nrows * (blockIdx.y + 1) / HEAD_FIN_CHUNKS);
    const float *__restrict__ src = P.head_part + ((size_t)blockIdx.z * nrows + r0) * HEAD_PART_STRIDE(H3) + i;
    float v = 0.f;
#pragma unroll 8
    for (int r = r0; r < r1; ++r, src += HEAD_PART_STRIDE(H3)) v += *src;
    if (i < NW) {
        const int q = i / H3, cc = i % H3;
        if (q < MA) acc_add(P, &P.grads[(actor ? w_a : w_c) + (int64_t)q * H3 + cc], v);
        else acc_add(P, &P.grads[(actor ? b_prev_a : b_prev_c) + cc], v);
    } else acc_add(P, ppo_sum_dest(P, i - NW, b_a, b_c), v);
}

// KL-adaptive learning rate (rsl_rl PPO.update) + reset of the norm accumulator
// Optimiser step in two launches.  k_opt_prepare: squared gradient norm (one partial per block into loss_acc[4 + block],
// added in a fixed order by k_opt_adam; deterministic mode: fixed point into loss_acc[2 + par]) and, on one lane, the
// KL-adaptive learning rate, the loss statistics and the Adam step
// count.  k_opt_adam: clip_grad_norm_(max_norm) + torch.optim.Adam step (betas 0.9/0.999, eps 1e-8), then
// zeroes what it consumed -- the gradient buffer (+ KL tail) for the next minibatch and the OTHER norm slot
// (par alternates per step, so no block can still be reading the slot that is cleared).
// Workgroups past `prep_blocks` gather the NEXT minibatch into the other buffer set (G = P with that set's pointers): the
// gather depends on the rollout storage and the permutation only, and this launch leaves most of the chip idle.
__global__ void __launch_bounds__(256) k_opt_prepare(PpoDev P, int par, int prep_blocks, PpoDev G, int gather_mb) {
    if ((int)blockIdx.x >= prep_blocks) { gather4_block(G, gather_mb, (int)blockIdx.x - prep_blocks); return; }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const float kl = P.grads[P.num_params] / ((float)P.mb_rows * (float)P.world);
        float lr = P.stats[0];
        if (P.adaptive) {
            if (kl > P.desired_kl * 2.0f) lr = fmaxf(1e-5f, lr / 1.5f);
            else if (kl < P.desired_kl / 2.0f && kl > 0.0f) lr = fminf(1e-2f, lr * 1.5f);
        }
        P.stats[0] = lr;
        P.stats[1] = kl;
        P.stats[2] += P.loss_acc[0] / (float)P.mb_rows;
        P.stats[3] += P.loss_acc[1] / (float)P.mb_rows;
        P.stats[4] += 1.0f;                                  // Adam step count t (k_opt_adam reads the new value)
        P.stats[5] += 1.0f;
        P.loss_acc[0] = 0.f; P.loss_acc[1] = 0.f;
    }
    float s = 0.f;
    const float inv_world = 1.0f / (float)P.world;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < P.num_params; k += (int64_t)prep_blocks * blockDim.x) {
        float g = P.grads[k] * inv_world;
        s += g * g;
    }
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (P.det64) det_add_norm(P, par, red[0]);           // two-word fixed point: a squared norm leaves the range of acc_add's format
        else P.loss_acc[4 + blockIdx.x] = red[0];            // blockIdx.x < prep_blocks = LG_NORM_BLOCKS; summed in order by k_opt_adam
    }
}
// Deterministic mode: add the fixed-point shadow (PpoDev::det64) into the float buffers it stands for and clear it.  One adder per
// element and launch, so the float result does not depend on the order the contributions arrived in.
__global__ void __launch_bounds__(256) k_det_fold(PpoDev P) {
    const int64_t n = P.num_params + 10;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const long long q = P.det64[i];
        float *t = i < P.num_params + 2 ? P.grads + i : i < P.num_params + 6 ? P.loss_acc + (i - P.num_params - 2) : P.adv_partial + (i - P.num_params - 6);
        if (i == P.num_params + 4 || i == P.num_params + 5) {          // a squared gradient norm: two words (det_add_norm)
            const long long ql = P.det64[i + 6];
            if (q == 0 && ql == 0) continue;
            *t += (float)((double)q * (LG_DET_NORM_SPLIT / LG_DET_SCALE) + (double)ql * (1.0 / LG_DET_SCALE));
            P.det64[i] = 0; P.det64[i + 6] = 0;
            continue;
        }
        if (q == 0) continue;
        *t += (float)((double)q * (1.0 / LG_DET_SCALE));
        P.det64[i] = 0;
    }
}
// split-bf16 image of parameter k: pl_dest[k] = its element index inside a plane (weights) or -1 (biases, std)
__device__ __forceinline__ void write_planes(const PpoDev &P, int64_t k, float x) {
    const int d = P.pl_dest[k];
    if (d < 0) return;
    uint32_t h, m, l;
    split2(x, 0.f, h, m, l);
    P.wpl[d] = (uint16_t)h; P.wpl[P.pl_stride + d] = (uint16_t)m; P.wpl[2 * P.pl_stride + d] = (uint16_t)l;
}
// rebuild every plane from the fp32 parameters (begin of an update: parameters may have been written through
// the zero-copy views -- checkpoint load, initial broadcast)
__global__ void __launch_bounds__(256) k_sync_planes(PpoDev P) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < P.num_params; k += (int64_t)gridDim.x * blockDim.x)
        write_planes(P, k, P.params[k]);
}
__global__ void __launch_bounds__(256) k_opt_adam(PpoDev P, int par) {
    float norm_sq;
    if (P.det64) norm_sq = P.loss_acc[2 + par];
    else {                                                   // the block partials in one fixed order, the same in every wave and on every rank
        static_assert(LG_NORM_BLOCKS == 128, "two partials per lane of a wave");
        const int lane = threadIdx.x & 63;
        norm_sq = P.loss_acc[4 + lane] + P.loss_acc[4 + 64 + lane];
        for (int w = 32; w > 0; w >>= 1) norm_sq += __shfl_xor(norm_sq, w);
    }
    const float total = sqrtf(norm_sq);
    const float coef = fminf(P.max_grad_norm / (total + 1e-6f), 1.0f);
    const float lr = P.stats[0], t = P.stats[4];
    // fp32 corrections: 0.999f is 1.3e-8 above 0.999 and 1 - 0.999^t cancels while t << 1000, so the step is up to 6.6e-6 + 3e-5 / t short
    // or long of torch's (whose corrections are formed in double) -- inside the 1e-4 of a step this learner is held to; measured and
    // bounded in tests/ppo_opt_ref.py (bc_allowance)
    const float bc1 = 1.0f - powf(0.9f, t), bc2 = 1.0f - powf(0.999f, t);
    const float inv_world = 1.0f / (float)P.world;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < P.num_params; k += (int64_t)gridDim.x * blockDim.x) {
        const float g = P.grads[k] * inv_world * coef;
        const float m = 0.9f * P.adam_m[k] + 0.1f * g;
        const float v = 0.999f * P.adam_v[k] + 0.001f * g * g;
        P.adam_m[k] = m;
        P.adam_v[k] = v;
        const float pn = P.params[k] - (lr / bc1) * m / (sqrtf(v) / sqrtf(bc2) + 1e-8f);
        P.params[k] = pn;
        P.grads[k] = 0.f;
        write_planes(P, k, pn);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        P.grads[P.num_params] = 0.f; P.grads[P.num_params + 1] = 0.f;
        P.loss_acc[2 + (par ^ 1)] = 0.f;
    }
}

extern "C" {
void ppok_act_sample(const PpoDev *P, const float *obs, const float *cobs, const float *mu, const float *val, int t,
                     int64_t cnt, int inject, hipStream_t s) {
    // one lane per env for the sampling; at least 256 blocks so the observation copy is spread over the chip
    const int blocks = (P->N + 63) / 64;
    hipLaunchKernelGGL(k_act_sample, dim3(blocks > 256 ? blocks : 256), dim3(64), 0, s, *P, obs, cobs, mu, val, t, cnt, inject);
}
void ppok_process_step(const PpoDev *P, const float *rew, const uint8_t *dones, const uint8_t *tos, int t, hipStream_t s) {
    hipLaunchKernelGGL(k_process_step, dim3((P->N + 255) / 256), dim3(256), 0, s, *P, rew, dones, tos, t);
}
void ppok_det_fold(const PpoDev *P, hipStream_t s) { hipLaunchKernelGGL(k_det_fold, dim3(512), dim3(256), 0, s, *P); }
void ppok_gae(const PpoDev *P, const float *last_values, hipStream_t s) {
    (void)hipMemsetAsync(P->adv_partial, 0, 3 * sizeof(float), s);
    hipLaunchKernelGGL(k_gae, dim3((P->N + 255) / 256), dim3(256), 0, s, *P, last_values);
    if (P->det64) ppok_det_fold(P, s);
}
void ppok_adv_normalize(const PpoDev *P, hipStream_t s) {
    hipLaunchKernelGGL(k_adv_normalize, dim3(256), dim3(256), 0, s, *P);
}
void ppok_randperm(const PpoDev *P, int n, uint64_t update_idx, hipStream_t s) {
    int bits = 2;
    while ((1ll << bits) < n) ++bits;
    bits += bits & 1;                                          // balanced halves
    hipLaunchKernelGGL(k_randperm, dim3((n + 255) / 256), dim3(256), 0, s, *P, n, bits / 2, update_idx);
}
void ppok_gather(const PpoDev *P, int mb, hipStream_t s) {
    if ((P->A & 3) == 0)
        hipLaunchKernelGGL(k_gather4, dim3((P->mb_rows * 32 + 255) / 256), dim3(256), 0, s, *P, mb);
    else
        hipLaunchKernelGGL(k_gather, dim3(P->mb_rows), dim3(64), 0, s, *P, mb);
}
size_t ppok_head_part_floats() { return (size_t)2 * HEAD_NET_GRID * HEAD_PART_STRIDE(128); }
// returns 0 when the fused head kernel supports this width, -1 otherwise (caller falls back to GEMMs + k_loss)
int ppok_head_fused(const PpoDev *P, int H3, const float *xa, const float *xc, float *dza, float *dzc, int64_t w_a, int64_t b_a,
                    int64_t w_c, int64_t b_c, int64_t b_prev_a, int64_t b_prev_c, hipStream_t s) {
    const int ntiles = (P->mb_rows + HEAD_ROWS - 1) / HEAD_ROWS;
    dim3 grid(ntiles < HEAD_GRID ? ntiles : HEAD_GRID), block(256);
    if (H3 == 128) {                                       // one network per workgroup: 3 per CU, a 24576-row minibatch resident at once
        const int nrows = ntiles < HEAD_NET_GRID ? ntiles : HEAD_NET_GRID;
        if (P->A <= 12)
            hipLaunchKernelGGL((k_head_net<128, 12>), dim3(nrows, 2), block, 0, s, *P, xa, xc, dza, dzc, P->params + w_a, P->params + w_c, b_a, b_c);
        else
            hipLaunchKernelGGL((k_head_net<128, LG_PPO_MAX_A>), dim3(nrows, 2), block, 0, s, *P, xa, xc, dza, dzc, P->params + w_a, P->params + w_c, b_a, b_c);
        constexpr int NTOT = HEAD_PART_STRIDE(128);
        hipLaunchKernelGGL((k_head_finish<128>), dim3((NTOT + 255) / 256, HEAD_FIN_CHUNKS, 2), block, 0, s, *P, nrows, w_a, b_a, w_c, b_c,
                           b_prev_a, b_prev_c);
    } else if (H3 == 64) hipLaunchKernelGGL((k_head_fused<64>), grid, block, 0, s, *P, xa, xc, dza, dzc, w_a, b_a, w_c, b_c, b_prev_a, b_prev_c);
    else if (H3 == 32) hipLaunchKernelGGL((k_head_fused<32>), grid, block, 0, s, *P, xa, xc, dza, dzc, w_a, b_a, w_c, b_c, b_prev_a, b_prev_c);
    else return -1;
    return 0;
}
void ppok_loss(const PpoDev *P, const float *mu, const float *v, float *dmu, float *dval, hipStream_t s) {
    hipLaunchKernelGGL(k_loss, dim3((P->mb_rows + 255) / 256), dim3(256), 0, s, *P, mu, v, dmu, dval);
}
void ppok_sync_planes(const PpoDev *P, hipStream_t s) { hipLaunchKernelGGL(k_sync_planes, dim3(256), dim3(256), 0, s, *P); }
// G / gather_mb: buffer set and index of a minibatch to gather beside the norm reduction (gather_mb < 0: none); returns
// whether the gather was taken (the 16-byte row layout of k_gather4)
int ppok_step(const PpoDev *P, int par, const PpoDev *G, int gather_mb, hipStream_t s) {
    const bool g4 = gather_mb >= 0 && (P->A & 3) == 0;
    const int gblocks = g4 ? (P->mb_rows * 32 + 255) / 256 : 0;
    hipLaunchKernelGGL(k_opt_prepare, dim3(LG_NORM_BLOCKS + gblocks), dim3(256), 0, s, *P, par, LG_NORM_BLOCKS, g4 ? *G : *P, gather_mb);
    if (P->det64) ppok_det_fold(P, s);                   // the squared gradient norm
    // one parameter per thread: the per-parameter chain (4 loads, Adam, 4 stores + the three plane stores through pl_dest) is a
    // memory round trip that a grid-stride loop repeats serially (6 x for [512,256,128] on 256 workgroups: 12.2 us; 8.9 us on 1024, 10.2 on 2048)
    constexpr int adam_max = 1024;
    const long want = (P->num_params + 255) / 256;
    hipLaunchKernelGGL(k_opt_adam, dim3((unsigned)(want < adam_max ? (want > 0 ? want : 1) : adam_max)), dim3(256), 0, s, *P, par);
    return g4 ? 1 : 0;
}
}
