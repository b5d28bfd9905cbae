// Planner kernels on a learned or analytic tube (DESIGN.md sections 10.9 to 10.14, 10.18) and their launchers: scoring (k_plan_score), the
// sampling planner (k_plan_sample_score, k_plan_mppi_*), the one-step kind (k_plan_score_step, k_plan_sample_score_step) and the
// gradient planner (k_plan_grad).  The MLP forward and backward are the trainer's and inference's own (tube_mlp.h).
#include <cstring>

#include "plan_device.h"
#include "tube_mlp.h"

constexpr int R = LG_TUBE_ROWS, NT = LG_TUBE_THREADS, RB = LG_TUBE_RB;   // the tile, under the names the kernels use

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
    const float *sc_goal, *sc_obs;      // lg_plan_scenes (section 10.14): read by the kernels with SC != PLAN_SC_PROB alone
    const int32_t *sc_n;
    const float *sc_vel;                // its velocities (section 10.18): read by the <SC = PLAN_SC_MOVING> kernels alone
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
// PlanSceneRowMoving (section 10.18): a row of PLAN_SCNM floats, the static row and then (ux, uy) x LG_PLAN_MAX_OBS; obstacle i has its
// centre at node k at c_i + u_i t_k, t_k = (float)k dt, every operation rounded on its own.  The static accessors ignore k.
#define PLAN_SCN (3 + 3 * LG_PLAN_MAX_OBS)
#define PLAN_SCNM (PLAN_SCN + 2 * LG_PLAN_MAX_OBS)
static_assert(PLAN_SCN == 27 && (PLAN_SCN & 1), "a scene row: 2 + 24 + 1 floats, an odd stride");
static_assert(PLAN_SCNM == 43 && (PLAN_SCNM & 1), "a moving scene row: 27 + 16 floats, an odd stride");
enum { PLAN_SC_PROB = 0, PLAN_SC_ROW = 1, PLAN_SC_MOVING = 2 };    // a kernel's SC flag: the scene its walks read
constexpr int plan_scn(int sc) { return sc == PLAN_SC_MOVING ? PLAN_SCNM : (sc == PLAN_SC_ROW ? PLAN_SCN : 0); }   // floats of a row
struct PlanSceneProb {
    const lg_plan_problem &p;
    __device__ __forceinline__ int n() const { return p.n_obs; }
    __device__ __forceinline__ float cx(int i, int) const { return p.obs_c[i][0]; }
    __device__ __forceinline__ float cy(int i, int) const { return p.obs_c[i][1]; }
    __device__ __forceinline__ float r(int i) const { return p.obs_r[i]; }
    __device__ __forceinline__ float gx() const { return p.goal[0]; }
    __device__ __forceinline__ float gy() const { return p.goal[1]; }
};
struct PlanSceneRow {
    const float *s;
    __device__ __forceinline__ int n() const { return (int)s[PLAN_SCN - 1]; }
    __device__ __forceinline__ float cx(int i, int) const { return s[2 + 3 * i]; }
    __device__ __forceinline__ float cy(int i, int) const { return s[3 + 3 * i]; }
    __device__ __forceinline__ float r(int i) const { return s[4 + 3 * i]; }
    __device__ __forceinline__ float gx() const { return s[0]; }
    __device__ __forceinline__ float gy() const { return s[1]; }
};
struct PlanSceneRowMoving {
    const float *s;
    float dt;
    __device__ __forceinline__ int n() const { return (int)s[PLAN_SCN - 1]; }
    __device__ __forceinline__ float cx(int i, int k) const {
#pragma clang fp contract(off)
        const float t = (float)k * dt, d = s[PLAN_SCN + 2 * i] * t;
        return s[2 + 3 * i] + d;
    }
    __device__ __forceinline__ float cy(int i, int k) const {
#pragma clang fp contract(off)
        const float t = (float)k * dt, d = s[PLAN_SCN + 2 * i + 1] * t;
        return s[3 + 3 * i] + d;
    }
    __device__ __forceinline__ float r(int i) const { return s[4 + 3 * i]; }
    __device__ __forceinline__ float gx() const { return s[0]; }
    __device__ __forceinline__ float gy() const { return s[1]; }
};
// Rows 0 .. rows - 1 of SCN take scenes s0, s0 + 1, ..; rows at and past nr are zeros with a zero count.  A part the scenes leave
// out (goal, or obs and n_obs) comes from the problem; n_obs[s] is clamped into 0 .. LG_PLAN_MAX_OBS and slots past it are not read.
// SC = PLAN_SC_MOVING: rows of PLAN_SCNM floats, whose last 16 take the scene's velocities (zeros past the count).
template <int SC>
__device__ __forceinline__ void plan_scene_stage(const PlanDev &P, float *SCN, int64_t s0, int rows, int nr, int tid) {
    constexpr int W = plan_scn(SC);
    for (int e = tid; e < rows * W; e += NT) {
        const int r = e / W, c = e - r * W;
        float x = 0.f;
        if (r < nr) {
            const int64_t s = s0 + r;
            if (c < 2) x = P.sc_goal ? P.sc_goal[s * 2 + c] : P.p.goal[c];
            else {
                int n = P.sc_n ? P.sc_n[s] : P.p.n_obs;
                n = n < 0 ? 0 : (n > LG_PLAN_MAX_OBS ? LG_PLAN_MAX_OBS : n);
                const int q = c - 2, i = q / 3, k = q - 3 * i;
                if (c == PLAN_SCN - 1) x = (float)n;
                else if (SC == PLAN_SC_MOVING && c >= PLAN_SCN) {
                    const int qv = c - PLAN_SCN;
                    if ((qv >> 1) < n) x = P.sc_vel[s * (2 * LG_PLAN_MAX_OBS) + qv];
                } else if (i < n) x = P.sc_obs ? P.sc_obs[s * (3 * LG_PLAN_MAX_OBS) + q] : (k < 2 ? P.p.obs_c[i][k] : P.p.obs_r[i]);
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
            const float dx = zx - sn.cx(i, k), dy = zy - sn.cy(i, k), rr = sn.r(i) + wk;
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
            W.cost = W.cost + plan_quad(p.R, vx, vy);
        }
        W.cost = W.cost + (wk * p.Qw) * wk;
        if (k < N) {
            zx = zx + p.dt * vx; zy = zy + p.dt * vy;          // SingleInt2D.f
            wk = offset ? fw[k] + offset[k] : fw[k];
        }
    }
    return W;
}

// The one place a kernel's SC flag turns into a scene: the row `scn` of the tile's SCN, or the problem's own.
template <int SC>
__device__ __forceinline__ auto plan_scene(const PlanDev &P, const float *scn) {
    if constexpr (SC == PLAN_SC_MOVING) return PlanSceneRowMoving{scn, P.p.dt};
    else if constexpr (SC == PLAN_SC_ROW) return PlanSceneRow{scn};
    else return PlanSceneProb{P.p};
}
// plan_walk of a lane of a tile of kernel flag SC
template <bool PEN, int SC>
__device__ __forceinline__ PlanWalk plan_walk_tile(const PlanDev &P, const float *scn, bool nn, const float *vr, float *fw, float *zw, float zx,
                                                   float zy, float wk) {
    return plan_walk<PEN>(P.p, plan_scene<SC>(P, scn), nn, vr, fw, zw, zx, zy, wk, P.offset);
}

// The outputs of a scoring tile: plan_store_score in the lane that walked plan b, its four results; plan_store_nodes in every
// thread once all walks are done, behind a barrier of its own, the (z, w) nodes the walks left in ZW.
__device__ __forceinline__ void plan_store_score(const PlanDev &P, const PlanWalk &W, int64_t b) {
    P.cost[b] = W.cost; P.min_clear[b] = W.minc; P.worst_node[b] = W.worst;
    P.n_viol[b * 4] = W.nv_g; P.n_viol[b * 4 + 1] = W.nv_v; P.n_viol[b * 4 + 2] = W.nv_z; P.n_viol[b * 4 + 3] = W.nv_w;
}
__device__ __forceinline__ void plan_store_nodes(const PlanDev &P, const float *ZW, int64_t base, int nr, int tid) {
    const int N = P.p.N, ZS = PLAN_ZS(N);
    __syncthreads();
    for (int e = tid; e < nr * (N + 1); e += NT) {
        const int r = e / (N + 1), k = e - r * (N + 1);
        const float *zw = ZW + r * ZS + 3 * k;
        const int64_t o = (base + r) * (N + 1) + k;
        if (P.z) { P.z[o * 2] = zw[0]; P.z[o * 2 + 1] = zw[1]; }
        if (P.w) P.w[o] = zw[2];
    }
}
// J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z of plan b's walk, every operation rounded on its own, stored to J[b] with
// the optional cost, min_clear and pen (.., 3); returns J
__device__ __forceinline__ float plan_store_J(const PlanDev &P, const PlanWalk &W, float rho_g, float rho_w, float rho_z, float *J, float *pen,
                                              int64_t b) {
#pragma clang fp contract(off)
    const float j = ((W.cost + rho_g * W.pen_g) + rho_w * W.pen_w) + rho_z * W.pen_z;
    J[b] = j;
    if (P.cost) P.cost[b] = W.cost;
    if (P.min_clear) P.min_clear[b] = W.minc;
    if (pen) { pen[b * 3] = W.pen_g; pen[b * 3 + 1] = W.pen_w; pen[b * 3 + 2] = W.pen_z; }
    return j;
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
// and with SC the scenes SCN (R, plan_scn(SC)): row r walks against scene base + r.
template <int SC>
__global__ void __launch_bounds__(NT) k_plan_score(TubeDev D, PlanDev P, int64_t count) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, I = P.I, Hr = P.Hr;
    const bool nn = P.p.tube_kind == LG_PLAN_TUBE_NN;
    const int U = nn ? D.units : 0, L = D.layers, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds, *H0 = X + R * I, *H1 = H0 + R * U, *FW = H1 + R * U, *ZW = FW + R * N, *SCN = ZW + R * ZS;
    plan_gather(P, X, base, nr, tid);
    if constexpr (SC != PLAN_SC_PROB) plan_scene_stage<SC>(P, SCN, base, R, nr, tid);
    __syncthreads();
    if (nn) {
        const float *in = tube_hidden<R, RB, NT>(tid, D, X, D.wt, D.params, H0, H1);
        tube_layer<R, RB, NT, true>(tid, D.din[L], N, in, D.wt + D.off_w[L], D.params + D.off_b[L], D.act, D.sp_beta, FW,
                                    P.fw ? P.fw + base * N : nullptr, N, P.fw ? nr : 0);
        __syncthreads();
    }
    if (tid < nr) {
        const int64_t b = base + tid;
        plan_store_score(P, plan_walk_tile<false, SC>(P, SCN + tid * plan_scn(SC), nn, X + tid * I + 3 * Hr, FW + tid * N, ZW + tid * ZS,
                                                      P.z0[b * 2], P.z0[b * 2 + 1], P.w0 ? P.w0[b] : 0.f), b);
    }
    if (!P.z && !P.w && (nn || !P.fw)) return;
    plan_store_nodes(P, ZW, base, nr, tid);
    if (!nn && P.fw)                    // an analytic kind's tube values: the walk wrote them to FW
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
template <int SC>
__global__ void __launch_bounds__(NT) k_plan_sample_score(TubeDev D, PlanDev P, MppiDev M) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, I = P.I, Hr = P.Hr;
    const bool nn = P.p.tube_kind == LG_PLAN_TUBE_NN;
    const int U = nn ? D.units : 0, L = D.layers, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int pi = (int)(base / M.K), j0 = (int)(base - (int64_t)pi * M.K);
    float *X = lds, *H0 = X + R * I, *H1 = H0 + R * U, *FW = H1 + R * U, *ZW = FW + R * N, *SCN = ZW + R * ZS;
    if constexpr (SC != PLAN_SC_PROB) plan_scene_stage<SC>(P, SCN, pi, 1, 1, tid);
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
        // the chain and the scene fork below are written out, not tube_hidden / plan_walk_tile: with either inlined here one MPPI
        // iteration at the reference shape measured 0.2 .. 0.8 % slower than before them (profiles/plan_refactor_bench.txt)
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
        const PlanWalk W = SC == PLAN_SC_MOVING
                               ? plan_walk<true>(P.p, PlanSceneRowMoving{SCN, P.p.dt}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[pi * 2],
                                                 P.z0[pi * 2 + 1], w0, P.offset)
                           : SC ? plan_walk<true>(P.p, PlanSceneRow{SCN}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[pi * 2], P.z0[pi * 2 + 1],
                                                w0, P.offset)
                              : plan_walk<true>(P.p, PlanSceneProb{P.p}, nn, vr, FW + tid * N, ZW + tid * ZS, P.z0[pi * 2],
                                                P.z0[pi * 2 + 1], w0, P.offset);
        plan_store_J(P, W, M.rho_g, M.rho_w, M.rho_z, M.J, M.pen, b);
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
constexpr size_t plan_step_floats(int I, int U, int Hr, int N, int sc) {   // the tile without the weights; sc: the kernels' SC flag
    return (size_t)R * (PLAN_STEP_VS(Hr, N) + PLAN_STEP_WS(Hr, N) + I + 2 * U + PLAN_ZS(N) + plan_scn(sc));
}
struct PlanStepTile {
    float *W, *V, *WL, *X, *H0, *H1, *ZW, *SCN;         // SCN (R, plan_scn(SC)): the tile's scenes, kernels with SC alone
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
    const int N = P.p.N, I = P.I, Hr = P.Hr, L = D.layers, Ix = I - (D.level_input ? 1 : 0);
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
        const float *in = tube_hidden<R, RB, NT>(tid, D, S.X, wsrc, bsrc, S.H0, S.H1);
        tube_layer<R, RB, NT, true>(tid, D.din[L], 1, in, wsrc + D.off_w[L], bsrc + D.off_b[L], D.act, D.sp_beta, nullptr,
                                    S.WL + Hr + 1 + k, S.WS, R);
        __syncthreads();
    }
}

// k_plan_score for the one-step kind.  Dynamic LDS: (W the parameters), V (R, VS), WL (R, WS), X (R, I), H0, H1 (R, U), ZW (R, PLAN_ZS),
// (SCN (R, plan_scn(SC)) the scenes).
template <bool WLDS, int SC>
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
    if constexpr (SC != PLAN_SC_PROB) plan_scene_stage<SC>(P, S.SCN, base, R, nr, tid);
    plan_step_roll<WLDS>(D, P, S, tid);
    if (tid < nr) {
        const int64_t b = base + tid;
        plan_store_score(P, plan_walk_tile<false, SC>(P, S.SCN + tid * plan_scn(SC), true, S.V + tid * S.VS + 2 * Hr, S.WL + tid * S.WS + Hr + 1,
                                                      S.ZW + tid * ZS, P.z0[b * 2], P.z0[b * 2 + 1], S.WL[tid * S.WS + Hr]), b);
    }
    if (P.fw)
        for (int e = tid; e < nr * N; e += NT) {
            const int r = e / N, k = e - r * N;
            P.fw[base * N + e] = S.WL[r * S.WS + Hr + 1 + k];
        }
    if (!P.z && !P.w) return;
    plan_store_nodes(P, S.ZW, base, nr, tid);
}

// k_plan_sample_score for the one-step kind: the same tile with the plan columns drawn in place; tile t holds candidates of one
// instance, whose v_prev, e and w0 every row shares.  J is formed by k_plan_sample_score's expression.
template <bool WLDS, int SC>
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
    if constexpr (SC != PLAN_SC_PROB) plan_scene_stage<SC>(P, S.SCN, pi, 1, 1, tid);
    plan_step_roll<WLDS>(D, P, S, tid);
    if (tid < R) {
        const PlanWalk W = plan_walk_tile<true, SC>(P, S.SCN, true, S.V + tid * S.VS + 2 * Hr, S.WL + tid * S.WS + Hr + 1, S.ZW + tid * ZS,
                                                    P.z0[pi * 2], P.z0[pi * 2 + 1], P.w0 ? P.w0[pi] : 0.f);
        plan_store_J(P, W, M.rho_g, M.rho_w, M.rho_z, M.J, M.pen, base + tid);
    }
}

// ------------------------------------------------------------------ gradient planner on a tube
// J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z of R plans per workgroup and dJ/dv of every plan by a reverse sweep in the
// same workgroup, with projected Adam and the elite fused behind it.  No atomics; a plan's outputs depend on its own row alone.
//
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
    const float *Ri = p.R;
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
            const float dx = zx - sn.cx(i, k), dy = zy - sn.cy(i, k), rr = sn.r(i) + wk;
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

template <int SC>                       // SC: the scenes SCN (R, plan_scn(SC)) follow ZW; both walks of row r read scene base + r
__global__ void __launch_bounds__(NT) k_plan_grad(TubeDev D, PlanDev P, GradDev G, int64_t count) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, N = P.p.N, I = P.I, Hr = P.Hr;
    const bool nn = P.p.tube_kind == LG_PLAN_TUBE_NN;
    const int U = nn ? D.units : 0, L = nn ? D.layers : 0, ZS = PLAN_ZS(N);
    const int64_t base = (int64_t)blockIdx.x * R;
    const int nr = (int)(count - base < R ? count - base : R);
    float *X = lds, *H = X + R * I, *FW = H + R * U * L, *ZW = FW + R * N, *SCN = ZW + R * ZS;
    plan_gather(P, X, base, nr, tid);
    if constexpr (SC != PLAN_SC_PROB) plan_scene_stage<SC>(P, SCN, base, R, nr, tid);
    __syncthreads();
    if (nn) {
        const float *in = tube_hidden<R, RB, NT, true>(tid, D, X, D.wt, D.params, H, nullptr);
        tube_layer<R, RB, NT, true>(tid, D.din[L], N, in, D.wt + D.off_w[L], D.params + D.off_b[L], D.act, D.sp_beta, FW, nullptr, N, 0);
        __syncthreads();
    }
    if (tid < nr) {
        const int64_t b = base + tid;
        float *zw = ZW + tid * ZS;
        const float *vr = X + tid * I + 3 * Hr, *scn = SCN + tid * plan_scn(SC);
        const PlanWalk W = plan_walk_tile<true, SC>(P, scn, nn, vr, FW + tid * N, zw, P.z0[b * 2], P.z0[b * 2 + 1], P.w0 ? P.w0[b] : 0.f);
        const float J = plan_store_J(P, W, G.rho_g, G.rho_w, G.rho_z, G.J, G.pen, b);
        plan_walk_back(P.p, plan_scene<SC>(P, scn), nn, vr, FW + tid * N, zw, G.rho_g, G.rho_w, G.rho_z);
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

// ------------------------------------------------------------------ launchers
// Per-plan scenes: without them (A->scenes null) a launch takes the instantiation without, the code of
// the entries before scenes; otherwise the <SC = PLAN_SC_ROW> one, whose tile carries R scene rows (one row in the sampling kernels,
// within the same budget), or with scenes->vel (section 10.18) the <SC = PLAN_SC_MOVING> one, whose rows are 16 floats longer.
static int plan_sc(const lg_plan_scenes *scenes) { return !scenes ? PLAN_SC_PROB : (scenes->vel ? PLAN_SC_MOVING : PLAN_SC_ROW); }
static size_t plan_scn_bytes(int sc) { return sizeof(float) * (size_t)R * plan_scn(sc); }     // the R scene rows of a tile

// The PlanDev of a launch.  D: the handle's TubeDev, or null for an analytic kind, whose item is the plan's inputs alone.
static PlanDev plan_dev(const TubeDev *D, const lg_plan_problem *prob, const PlanArgs *A) {
    PlanDev P;
    memset(&P, 0, sizeof(P));
    P.p = *prob;
    P.z0 = A->z0; P.v = A->v; P.e = D ? A->e : nullptr; P.v_prev = D ? A->v_prev : nullptr; P.w0 = A->w0; P.offset = A->offset;
    P.cost = A->cost; P.min_clear = A->min_clear; P.worst_node = A->worst_node; P.n_viol = A->n_viol; P.fw = A->fw; P.z = A->z; P.w = A->w;
    P.level = A->level;
    P.Hr = D ? prob->H_rev : 0;
    P.I = D ? D->in_dim : 2 * prob->N;
    if (A->scenes) { P.sc_goal = A->scenes->goal; P.sc_obs = A->scenes->obs; P.sc_n = A->scenes->n_obs; P.sc_vel = A->scenes->vel; }
    return P;
}
// the TubeDev a kernel takes: the handle's, or zeros for an analytic kind
static TubeDev plan_tube(const TubeDev *D) {
    TubeDev T;
    memset(&T, 0, sizeof(T));
    if (D) T = *D;
    return T;
}
// floats of a one-shot tile: the items, `hidden` floats of activations per row, FW and ZW
static size_t plan_tile_floats(const PlanDev &P, int hidden) { return (size_t)R * (P.I + hidden + P.p.N + PLAN_ZS(P.p.N)); }

// Kernel K on nwg workgroups with `bytes` of dynamic LDS.  K's dynamic LDS ceiling is set once per device, not per launch.
// Returns bytes, or -1 where the ceiling cannot be set.
template <auto K, class... Args>
static int64_t plan_launch_kernel(unsigned nwg, size_t bytes, hipStream_t s, const Args &...args) {
    static bool ceiling_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev < 0 || dev >= 64 || !ceiling_set[dev]) {
        if (hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, LG_TUBE_ROLLOUT_LDS) != hipSuccess) return -1;
        if (dev >= 0 && dev < 64) ceiling_set[dev] = true;
    }
    hipLaunchKernelGGL(K, dim3(nwg), dim3(NT), bytes, s, args...);
    return (int64_t)bytes;
}
// One planner launch: instantiation `pick` of K... -- pick = the SC flag, or for a one-step kernel 3 (weights in LDS) + SC.
template <auto... K, class... Args>
static int64_t plan_launch(int pick, unsigned nwg, size_t bytes, hipStream_t s, const Args &...args) {
    using Launch = int64_t (*)(unsigned, size_t, hipStream_t, const Args &...);
    static constexpr Launch launch[] = {plan_launch_kernel<K, Args...>...};
    return launch[pick](nwg, bytes, s, args...);
}

extern "C" {
// k_plan_score.  D: the horizon handle's TubeDev, or null for an analytic kind.  Returns the dynamic LDS of the launch in bytes, or
// -1 where the kernel's ceiling cannot be set.  The reference shape (130 inputs, 128 units, N = 50) takes 74 KiB, past k_tube_predict's
// own 64 KiB, so the ceiling is the roll-out kernels'; the largest shape of the envelope stays below it:
static_assert(sizeof(float) * R * (LG_TUBE_MAX_IN + 2 * LG_TUBE_MAX_UNITS + LG_PLAN_MAX_N + PLAN_ZS(LG_PLAN_MAX_N) + PLAN_SCNM) <= LG_TUBE_ROLLOUT_LDS,
              "k_plan_score: the envelope's largest tile set must fit the dynamic LDS ceiling");
int64_t tubek_plan_score(const TubeDev *D, const lg_plan_problem *prob, const PlanArgs *A, int64_t B, hipStream_t s) {
    const PlanDev P = plan_dev(D, prob, A);
    const TubeDev T = plan_tube(D);
    const int sc = plan_sc(A->scenes);
    const size_t bytes = sizeof(float) * plan_tile_floats(P, 2 * T.units) + plan_scn_bytes(sc);
    return plan_launch<k_plan_score<0>, k_plan_score<1>, k_plan_score<2>>(sc, (unsigned)((B + R - 1) / R), bytes, s, T, P, B);
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
int64_t tubek_plan_sample_score(const TubeDev *D, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const PlanArgs *A, int64_t P_,
                                const float *vbar, float *J, float *pen, hipStream_t s) {
    const PlanDev P = plan_dev(D, prob, A);
    const TubeDev T = plan_tube(D);
    MppiDev M = mppi_dev(prob, cfg, it);
    M.vbar_in = vbar; M.J = J; M.pen = pen;
    const int sc = plan_sc(A->scenes);
    const size_t bytes = sizeof(float) * (plan_tile_floats(P, 2 * T.units) + plan_scn(sc));
    return plan_launch<k_plan_sample_score<0>, k_plan_sample_score<1>, k_plan_sample_score<2>>(sc, (unsigned)(P_ * cfg->K / R), bytes, s, T, P, M);
}
// The one-step kind.  Every shape of the envelope fits the ceiling without the weights -- the reference
// configurations (T <= 10, units <= 128, N <= 64) with room to spare --; lg_plan_check asks tubek_plan_step_bytes all the same.
static_assert(sizeof(float) * plan_step_floats(LG_TUBE_MAX_IN, LG_TUBE_MAX_UNITS, LG_PLAN_STEP_MAX_HREV, LG_PLAN_MAX_N, PLAN_SC_MOVING) <=
                  LG_TUBE_ROLLOUT_LDS,
              "k_plan_score_step: the envelope's largest tile set must fit the dynamic LDS ceiling");
static_assert(sizeof(float) * plan_step_floats(31, 128, LG_PLAN_STEP_MAX_HREV, 64, PLAN_SC_MOVING) <= LG_TUBE_ROLLOUT_LDS,
              "the reference one-step shapes fit");
// dynamic LDS of the one-step tile in bytes, without the weights and without the scene rows
int64_t tubek_plan_step_bytes(const TubeDev *D, const lg_plan_problem *prob) {
    return (int64_t)(sizeof(float) * plan_step_floats(D->in_dim, D->units, prob->H_rev, prob->N, PLAN_SC_PROB));
}
// weights go to LDS where weights + tile fit the ceiling; *bytes: the launch's dynamic LDS
static bool plan_step_wlds(const TubeDev *D, const lg_plan_problem *prob, int sc, size_t *bytes) {
    const size_t tile = (size_t)tubek_plan_step_bytes(D, prob) + plan_scn_bytes(sc);
    const size_t all = tile + sizeof(float) * (size_t)D->num_params;
    const bool wl = all <= LG_TUBE_ROLLOUT_LDS;
    *bytes = wl ? all : tile;
    return wl;
}
// returns the dynamic LDS of the launch in bytes, or -1 where the kernel's ceiling cannot be set
int64_t tubek_plan_score_step(const TubeDev *D, const lg_plan_problem *prob, const PlanArgs *A, int64_t B, hipStream_t s) {
    const PlanDev P = plan_dev(D, prob, A);
    const int sc = plan_sc(A->scenes);
    size_t bytes;
    const bool wl = plan_step_wlds(D, prob, sc, &bytes);
    return plan_launch<k_plan_score_step<false, 0>, k_plan_score_step<false, 1>, k_plan_score_step<false, 2>, k_plan_score_step<true, 0>,
                       k_plan_score_step<true, 1>, k_plan_score_step<true, 2>>(3 * wl + sc, (unsigned)((B + R - 1) / R), bytes, s, *D, P, B);
}
int64_t tubek_plan_sample_score_step(const TubeDev *D, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int it, const PlanArgs *A,
                                     int64_t P_, const float *vbar, float *J, float *pen, hipStream_t s) {
    const PlanDev P = plan_dev(D, prob, A);
    MppiDev M = mppi_dev(prob, cfg, it);
    M.vbar_in = vbar; M.J = J; M.pen = pen;
    const int sc = plan_sc(A->scenes);
    size_t bytes;
    const bool wl = plan_step_wlds(D, prob, sc, &bytes);   // one scene row is read; the tile's budget is k_plan_score_step's
    return plan_launch<k_plan_sample_score_step<false, 0>, k_plan_sample_score_step<false, 1>, k_plan_sample_score_step<false, 2>,
                       k_plan_sample_score_step<true, 0>, k_plan_sample_score_step<true, 1>, k_plan_sample_score_step<true, 2>>(
        3 * wl + sc, (unsigned)(P_ * cfg->K / R), bytes, s, *D, P, M);
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
static_assert(sizeof(float) * R * (LG_TUBE_MAX_IN + (LG_TUBE_MAX_LIN - 1) * LG_TUBE_MAX_UNITS + LG_PLAN_MAX_N + PLAN_ZS(LG_PLAN_MAX_N) + PLAN_SCNM) <=
                  LG_TUBE_ROLLOUT_LDS,
              "k_plan_grad: the envelope's largest tile set must fit the dynamic LDS ceiling");
static_assert(PLAN_ZS(1) >= 6, "k_plan_grad keeps J, two flags and dJ/dv of step 0 in a row of nodes at N = 1 too");
// returns the dynamic LDS of the launch in bytes, or -1 where the kernel's ceiling cannot be set
int64_t tubek_plan_grad(const TubeDev *D, const lg_plan_problem *prob, const PlanGradArgs *A, int64_t B, hipStream_t s) {
    const PlanDev P = plan_dev(D, prob, &A->plan);
    const TubeDev T = plan_tube(D);
    GradDev G;
    memset(&G, 0, sizeof(G));
    G.v = A->v; G.J = A->J; G.grad = A->grad; G.pen = A->pen; G.m = A->m; G.s = A->s; G.best_J = A->best_J; G.best_v = A->best_v;
    G.hist = A->hist; G.n_bad = A->n_bad;
    G.step = A->step; G.reset = A->reset;
    G.lr = A->lr; G.beta1 = A->beta1; G.beta2 = A->beta2; G.eps = A->eps; G.bc1 = A->bc1; G.bc2 = A->bc2;
    G.rho_g = A->rho_g; G.rho_w = A->rho_w; G.rho_z = A->rho_z;
    for (int d = 0; d < 2; ++d) { G.v_min[d] = prob->rom_v_min[d]; G.v_max[d] = prob->rom_v_max[d]; }
    const int sc = plan_sc(A->plan.scenes);
    const size_t bytes = sizeof(float) * plan_tile_floats(P, T.layers * T.units) + plan_scn_bytes(sc);
    return plan_launch<k_plan_grad<0>, k_plan_grad<1>, k_plan_grad<2>>(sc, (unsigned)((B + R - 1) / R), bytes, s, T, P, G, B);
}
}
