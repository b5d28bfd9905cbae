// Host side of the PPO learner, private to ppo_api.hip (the lg_ppo_* entries, allocation) and ppo_sched.hip (which launch goes to
// which stream in which order): the handle, its allocation helpers and the scheduling functions.
#pragma once
#include <string>
#include <vector>

#include "lg_internal.h"
#include "ppo_launch.h"

// LSTM front ends of a recurrent learner (lg_ppo_create_recurrent); H = 0 on a feed-forward one
struct Rnn {
    int H, mbs;                              // hidden size; envs per minibatch
    int in_dim[2];                           // LSTM input width: num_obs, num_critic_obs
    int64_t w_ih[2], w_hh[2], b_ih[2], b_hh[2];   // flat parameter offsets
    float *h[2], *c[2];                      // live state (N, H)
    float *sv_h[2], *sv_c[2];                // state before each rollout step (T, N, H)
    float *tmp_h[2], *tmp_c[2];              // input copy of the live state for the steps outside the rollout (N, H)
    // update workspace, rows t-major over the minibatch's envs (T x mbs)
    float *pg[2];                            // x . W_ih^T + b_ih (forward), then dG (backward)   [R][4H]
    float *hout[2], *cout[2], *hused[2], *cused[2], *dh[2];   // [R][H]
    float *gates[2];                         // [R][4H]
    float *dc[2];                            // [mbs][H]
};

struct Net {
    int nl;                                  // linear layers (hidden + head)
    int dims[LG_PPO_MAX_LAYERS + 1];         // dims[0] = input, dims[nl] = output
    int64_t w_off[LG_PPO_MAX_LAYERS], b_off[LG_PPO_MAX_LAYERS];
    int64_t pl_off[LG_PPO_MAX_LAYERS];       // offset of this layer's weight matrix inside a bf16 plane (multiple of 8)
    int pl_ld0;                              // row length of W_0's plane image: dims[0] rounded up to 32 = one k-tile (pad columns zero)
    float *act[LG_PPO_MAX_LAYERS + 1];       // act[l], l >= 1: output of layer l-1 (workspace, Mmax rows)
    float *dz[LG_PPO_MAX_LAYERS + 1];        // gradient wrt act[l] pre-activation
};

struct lg_ppo {
    lg_comm *comm = nullptr;                 // when set: gradients are reduced per layer inside the backward pass
    hipEvent_t ev_bucket = nullptr;          // a layer's weight gradients are complete on the side stream
    int comm_rc = 0;
    int comm_timing = 0;                     // lg_ppo_comm_timing: event pairs around the wait for the last bucket
    std::vector<hipEvent_t> comm_ev;         // [2 k], [2 k + 1]: before / after the wait of recorded minibatch k
    size_t comm_ev_used = 0;
    lg_ppo_cfg cfg = {};
    PpoDev dev = {};
    Net net[2] = {};                         // 0 actor, 1 critic
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;              // weight-gradient GEMMs run here, overlapping the input-gradient chain
    hipEvent_t ev_dz = nullptr, ev_side = nullptr;
    int overlap = 0;                         // weight gradients on the side stream (LG_PPO_OVERLAP, lg_ppo_debug_set_overlap)
    long long *det_buf = nullptr;            // fixed-point shadow of the accumulators (lg_ppo_set_deterministic); dev.det64 = it when on
    int act_code = 0;                        // kernels' activation code = cfg.activation + 1 (0 is 'none')
    int grads_dirty = 0;                     // gradients hold a backward pass that no optimiser step has consumed (and zeroed)
    // fused rollout epilogue (lg_ppo_attach_env): a process_env_step recorded for the next act launch
    lg_ctx *env = nullptr;
    int pp_pending = 0, pp_t = 0, pp_use_tos = 0;
    int params_dirty = 1;                    // the fp32 parameters changed since the rollout images (fragment-order weights / bf16 planes)
                                             // were derived from them: optimiser step, broadcast, lg_ppo_params_changed()
    int fused_act = 0;                       // rollout forward through k_mlp_fwd when the network shape allows (else per-layer GEMMs)
    MlpArgs mlp = {};                        // its arguments (fragment-order weight image allocated at create)
    int step = 0, inject = 0;
    int64_t act_count = 0, update_count = 0;
    int Mmax = 0;
    std::vector<void *> allocs;
    int64_t perm_count = 0;                  // updates begun: keys the device-side minibatch permutation
    // minibatch gathers are double-buffered: the optimiser step of minibatch mb gathers mb + 1 into the other set in the spare
    // workgroups of its norm-reduction launch (the gather depends on the rollout storage and the permutation only).  A gather launch
    // of its own before each minibatch: 0.474 / 0.485 ms per minibatch against 0.465 / 0.469, within that bench's noise (profiles/r02_ab.txt)
    struct MbSet { float *obs, *critic_obs, *actions, *mu, *scalars; } mbset[2] = {};
    int mb_cur = 0, mb_ready = -1, mb_last = -1;   // set the kernels read now; minibatch held by the other set (-1: none); last backward
    lg_ppo_buffers pub = {};
    Rnn rnn = {};
};

// the minibatch gathers the kernels given `dev` read and write: those of set m
inline void use_mb_set(PpoDev &dev, const lg_ppo::MbSet &m) {
    dev.mb_obs = m.obs; dev.mb_critic_obs = m.critic_obs; dev.mb_actions = m.actions; dev.mb_mu = m.mu; dev.mb_scalars = m.scalars;
}

template <typename T>
static bool palloc(lg_ppo *p, T **out, size_t n) {
    void *q = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    if (hipMalloc(&q, bytes) != hipSuccess || hipMemset(q, 0, bytes) != hipSuccess) return false;
    p->allocs.push_back(q);
    *out = (T *)q;
    return true;
}
#define PA(ptr, n) do { if (!palloc(p, &(ptr), (n))) { lg_set_error("hipMalloc failed in lg_ppo_create"); lg_ppo_destroy(p); return -100; } } while (0)

inline int launch_ok() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { lg_set_error(std::string("ppo kernel launch: ") + hipGetErrorString(e)); return -100; }
    return 0;
}

// ppo_sched.hip
namespace sched {
struct FwdOpts {
    bool skip_head;                          // stop before the head layer (the fused head kernel runs it)
    bool planes;                             // weights from the bf16 planes: valid inside an update (lg_ppo_begin_update syncs them) and
                                             // after a ppok_sync_planes
    bool in_pad;                             // the inputs are the minibatch gathers, rows padded to a multiple of 32 floats (PpoDev::Op / OCp);
                                             // otherwise rows of dims[0]
};
// forward of the selected nets on M rows.  in[z] = input of net z.  mask bit z selects the net.
void forward(lg_ppo *p, int M, const float *in0, const float *in1, int mask, FwdOpts o = {});
// backward of both nets on M rows given dz[nl] (head output gradients) already filled
void backward(lg_ppo *p, int M, const float *in0, const float *in1, bool skip_head);
int bucket_extents(lg_ppo *p, int l, float **bufs, int64_t *counts);
void reduce_layer_bucket(lg_ppo *p, int l, hipStream_t ready_on);
void flush_rollout_epilogue(lg_ppo *p);
void rnn_live_step(lg_ppo *p, int mask, const float *x0, const float *x1, int t);
void rnn_stash_live(lg_ppo *p, int mask, int t);
void rnn_forward_seq(lg_ppo *p, int mb);
void rnn_backward_seq(lg_ppo *p, int mb);
}  // namespace sched
