// The actor's observation history: a stacked row [obs_t | sel(obs_t-1) | ... | sel(obs_t-H+1)] per env, newest first, kept in a
// buffer the handle owns and advanced by ONE launch after the env step (legged_hip.h lg_obs_hist_*).
//
// Pure copying, launch- and memory-bound.  A workgroup owns LG_OH_TILE envs and its lanes run along (env, obs column); the lane of
// column c of env i does all of that column's work and touches no other lane's entries: it moves past frame k-1 to past frame k
// for k = H-1 .. 1 (past frame 0 being the row's own old current block), or on a reinitialisation fills the past frames, and then
// writes the new obs[i, c] into the current block.  One owner per entry: no LDS, no barrier, no atomics.  The selected-or-not
// test walks the range table of the kernel arguments, so it is the same for every env of a column.  The marks are not cleared
// here (that would need the env's lanes to agree that all have read them): a mark is the NUMBER of the compute it is meant
// for, so it lapses by itself when that compute has run.
#include "obshist_device.h"

// entry s of past frame k (k >= 1), or column c of the current block (k == 0)
__device__ __forceinline__ float *oh_slot(const ObsHistDev &D, float *row, int k, int s, int c) {
    return k == 0 ? row + c : row + D.O + (k - 1) * D.S + s;
}

__global__ __launch_bounds__(LG_OH_THREADS) void k_obs_history(ObsHistDev D) {
    const int env0 = (int)blockIdx.x * LG_OH_TILE;
    const int nE = min(LG_OH_TILE, D.n - env0);
    const int O = D.O;
    for (int idx = threadIdx.x; idx < nE * O; idx += LG_OH_THREADS) {
        const int e = idx / O, c = idx - e * O;
        const int i = env0 + e;
        float *row = D.row + (size_t)i * D.W;
        const float x = D.obs[(size_t)i * O + c];
        int s = -1;
        if (D.num_ranges == 0) s = c;                              // columns = None: every column is kept
        for (int r = 0; r < D.num_ranges; ++r)
            if (c >= D.lo[r] && c < D.hi[r]) s = D.pos[r] + (c - D.lo[r]);
        if (s >= 0) {
            if (D.reset[i] != 0 || D.marks[i] == D.epoch) {        // no frame of the previous episode survives
                const float fill = D.reset_mode == LG_OBS_HIST_ZERO ? 0.0f : x;
                for (int k = 1; k < D.H; ++k) *oh_slot(D, row, k, s, c) = fill;
            } else {
                int k = D.H - 1;
                for (; k >= 4; k -= 4) {                           // four loads in flight, then their four stores
                    const float v0 = *oh_slot(D, row, k - 1, s, c), v1 = *oh_slot(D, row, k - 2, s, c);
                    const float v2 = *oh_slot(D, row, k - 3, s, c), v3 = *oh_slot(D, row, k - 4, s, c);
                    *oh_slot(D, row, k, s, c) = v0; *oh_slot(D, row, k - 1, s, c) = v1;
                    *oh_slot(D, row, k - 2, s, c) = v2; *oh_slot(D, row, k - 3, s, c) = v3;
                }
                for (; k >= 1; --k) *oh_slot(D, row, k, s, c) = *oh_slot(D, row, k - 1, s, c);
            }
        }
        row[c] = x;
    }
}

// marks[id] = epoch for the n ids given, or for envs 0..n-1 when ids is NULL
__global__ __launch_bounds__(256) void k_obs_hist_mark(int64_t *__restrict__ marks, const int32_t *__restrict__ ids, int n, int num_envs,
                                                       int64_t epoch) {
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= n) return;
    const int i = ids ? ids[j] : j;
    if (i >= 0 && i < num_envs) marks[i] = epoch;
}

extern "C" void obshistk_launch(const ObsHistDev *D, hipStream_t st) {
    hipLaunchKernelGGL(k_obs_history, dim3((D->n + LG_OH_TILE - 1) / LG_OH_TILE), dim3(LG_OH_THREADS), 0, st, *D);
}

extern "C" void obshistk_mark(int64_t *marks, const int32_t *ids, int n, int num_envs, int64_t epoch, hipStream_t st) {
    hipLaunchKernelGGL(k_obs_hist_mark, dim3((n + 255) / 256), dim3(256), 0, st, marks, ids, n, num_envs, epoch);
}
