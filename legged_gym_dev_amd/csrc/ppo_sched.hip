// Scheduling of the PPO learner (ppo_learner.h): which launch goes to which stream in which order -- the layer-by-layer GEMMs of the
// ActorCritic forward and backward, the per-layer gradient buckets, the LSTM sequences, and what a deferred rollout epilogue still
// owes.  The lg_ppo_* entries and the allocation are ppo_api.hip's.
#include <cstring>

#include "ppo_learner.h"

// problem z of a GEMM launch: C (M x N, rows of ldc) from A (rows of lda) and B (rows of ldb) over a reduction of length K
static void gemm_problem(GemmArgs &g, int z, const float *A, int lda, const float *B, int ldb, float *C, int ldc, int M, int N, int K) {
    g.A[z] = A; g.lda[z] = lda;
    g.B[z] = B; g.ldb[z] = ldb;
    g.C[z] = C; g.ldc[z] = ldc;
    g.M[z] = M; g.N[z] = N; g.K[z] = K;
}
// deterministic mode: gradient atomics go to the fixed-point shadow
static void gemm_det(GemmArgs &g, const PpoDev &d) { g.det_base = d.grads; g.det64 = d.det64; g.det_n = d.num_params + 2; }

namespace sched {

void forward(lg_ppo *p, int M, const float *in0, const float *in1, int mask, FwdOpts o) {
    const float *in[2] = {in0, in1};
    const int in_ld[2] = {o.in_pad ? p->dev.Op : p->net[0].dims[0], o.in_pad ? p->dev.OCp : p->net[1].dims[0]};
    int sel[2], nz = 0;
    for (int z = 0; z < 2; ++z) if (mask & (1 << z)) sel[nz++] = z;
    const int nl = p->net[sel[0]].nl;
    for (int l = 0; l < nl - (o.skip_head ? 1 : 0); ++l) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        for (int k = 0; k < nz; ++k) {
            Net &n = p->net[sel[k]];
            gemm_problem(g, k, l == 0 ? in[sel[k]] : n.act[l], l == 0 ? in_ld[sel[k]] : n.dims[l], p->dev.params + n.w_off[l], n.dims[l],
                         n.act[l + 1], n.dims[l + 1], M, n.dims[l + 1], n.dims[l]);
            g.bias[k] = p->dev.params + n.b_off[l];
            g.Bpl[k] = o.planes ? p->dev.wpl + n.pl_off[l] : nullptr;
            // W_0's plane image has rows as long as the padded gather rows: with both padded the plane path reduces over whole chunks
            if (l == 0 && o.in_pad && o.planes && n.pl_ld0 != n.dims[0]) { g.Kpl[k] = n.pl_ld0; g.ldbpl[k] = n.pl_ld0; }
            else if (l == 0 && n.pl_ld0 != n.dims[0]) g.Bpl[k] = nullptr;   // unpadded input against padded plane rows: fp32 operand
        }
        g.elu = l < nl - 1 ? p->act_code : 0;
        g.pl_stride = p->dev.pl_stride;
        ppok_gemm_fwd(&g, nz, p->stream);
    }
}

// Gradient bucket of layer l (both nets: W_l and b_l are adjacent in the flat buffer), all-reduced on the communicator's stream
// as soon as the layer's weight-gradient GEMM is done.  b_l was summed by the input-gradient GEMM of layer l+1 (or by the loss
// kernel for the head), which the weight-gradient GEMM of layer l already waited for.  The head's bucket also carries std and
// the [KL sum | pad] tail.  The collectives of one bucket are one RCCL group.
int bucket_extents(lg_ppo *p, int l, float **bufs, int64_t *counts) {
    int n = 0;
    for (int z = 0; z < 2; ++z) {
        Net &net = p->net[z];
        bufs[n] = p->dev.grads + net.w_off[l];
        counts[n++] = (int64_t)net.dims[l + 1] * net.dims[l] + net.dims[l + 1];
    }
    if (l == p->net[0].nl - 1) {
        bufs[n] = p->dev.grads + p->dev.off_std; counts[n++] = p->cfg.num_actions;
        bufs[n] = p->dev.grads + p->dev.num_params; counts[n++] = 2;
    }
    return n;
}
void reduce_layer_bucket(lg_ppo *p, int l, hipStream_t ready_on) {
    float *bufs[4];
    int64_t counts[4];
    const int n = bucket_extents(p, l, bufs, counts);
    hipStream_t cs = lg_comm_stream_(p->comm);
    (void)hipEventRecord(p->ev_bucket, ready_on);
    (void)hipStreamWaitEvent(cs, p->ev_bucket, 0);
    const int rc = lg_comm_group_allreduce_(p->comm, bufs, counts, n, cs);
    if (rc && !p->comm_rc) p->comm_rc = rc;
}

void backward(lg_ppo *p, int M, const float *in0, const float *in1, bool skip_head) {
    const float *in[2] = {in0, in1};
    const int nl = p->net[0].nl;
    for (int l = nl - 1 - (skip_head ? 1 : 0); l >= 0; --l) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        gemm_det(g, p->dev);
        for (int z = 0; z < 2; ++z) {                // dW_l += dz[l+1]^T . act[l]
            Net &n = p->net[z];
            gemm_problem(g, z, n.dz[l + 1], n.dims[l + 1], l == 0 ? in[z] : n.act[l], n.dims[l], p->dev.grads + n.w_off[l], n.dims[l],
                         n.dims[l + 1], n.dims[l], M);
            if (l == 0 && !p->rnn.H) {               // the minibatch gathers: padded rows, the pad columns computed but not stored
                const int ldp = z == 0 ? p->dev.Op : p->dev.OCp;
                g.ldb[z] = ldp;
                if (ldp != n.dims[0]) { g.N[z] = ldp; g.nstore[z] = n.dims[0]; }
            }
        }
        // the weight gradient of layer l runs beside the input-gradient chain on the side stream -- except the last one
        // (l = 0), which has nothing left to overlap with: on the main stream it starts without the cross-stream event wait
        // (on the side stream: 0.479 / 0.490 ms per minibatch against 0.465 / 0.469, within that bench's noise: profiles/r02_ab.txt)
        const bool on_side = p->overlap && l > 0;
        hipStream_t dw_stream = on_side ? p->side : p->stream;
        if (on_side) {                               // dz[l+1] is complete on the main stream at this point
            (void)hipEventRecord(p->ev_dz, p->stream);
            (void)hipStreamWaitEvent(p->side, p->ev_dz, 0);
        }
        ppok_gemm_dw(&g, 2, dw_stream);
        if (p->comm) reduce_layer_bucket(p, l, dw_stream);
        if (l > 0) {                                 // dz[l] = (dz[l+1] . W_l) * act'(act[l]); db_{l-1} = colsum(dz[l])
            memset(&g, 0, sizeof(g));
            gemm_det(g, p->dev);
            for (int z = 0; z < 2; ++z) {
                Net &n = p->net[z];
                gemm_problem(g, z, n.dz[l + 1], n.dims[l + 1], p->dev.params + n.w_off[l], n.dims[l], n.dz[l], n.dims[l],
                             M, n.dims[l], n.dims[l + 1]);
                g.Bpl[z] = p->dev.wpl + n.pl_off[l];         // current inside an update (begin_update / k_opt_adam keep them)
                g.aux[z] = n.act[l]; g.ldaux[z] = n.dims[l];
                g.colsum[z] = p->dev.grads + n.b_off[l - 1];
            }
            g.elu = p->act_code;                         // derivative of the hidden activation, through its output act[l]
            g.pl_stride = p->dev.pl_stride;
            ppok_gemm_dx(&g, 2, p->stream);
        }
    }
    if (p->rnn.H) {                                  // recurrent: dL/dh = dz[1] . W_0 (no activation derivative: h feeds W_0 directly)
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        for (int z = 0; z < 2; ++z) {
            Net &n = p->net[z];
            gemm_problem(g, z, n.dz[1], n.dims[1], p->dev.params + n.w_off[0], n.dims[0], p->rnn.dh[z], n.dims[0], M, n.dims[0], n.dims[1]);
            g.Bpl[z] = p->dev.wpl + n.pl_off[0];
            g.aux[z] = p->rnn.dh[z]; g.ldaux[z] = n.dims[0];   // read before written by the same lane; activation code 0 ignores it
        }
        g.elu = 0;
        g.pl_stride = p->dev.pl_stride;
        ppok_gemm_dx(&g, 2, p->stream);
    }
    if (p->overlap) {                                // join: the optimiser step (main stream) needs every dW
        (void)hipEventRecord(p->ev_side, p->side);
        (void)hipStreamWaitEvent(p->stream, p->ev_side, 0);
    }
    if (p->comm) {                                   // ... and every reduced bucket
        const bool rec = p->comm_timing && p->comm_ev_used + 2 <= 2 * 4096;
        if (rec) {
            while (p->comm_ev.size() < p->comm_ev_used + 2) { hipEvent_t e; (void)hipEventCreate(&e); p->comm_ev.push_back(e); }
            (void)hipEventRecord(p->comm_ev[p->comm_ev_used], p->stream);
        }
        (void)hipEventRecord(lg_comm_event_(p->comm), lg_comm_stream_(p->comm));
        (void)hipStreamWaitEvent(p->stream, lg_comm_event_(p->comm), 0);
        if (rec) { (void)hipEventRecord(p->comm_ev[p->comm_ev_used + 1], p->stream); p->comm_ev_used += 2; }
    }
}

// What a deferred process_env_step (and the env's epilogue before it) still owes, the ordinary way: env epilogue first, then the
// process kernel on the refreshed extras["time_outs"] -- the order of the unfused loop.
void flush_rollout_epilogue(lg_ppo *p) {
    if (!p->env) return;
    (void)lg_finalize(p->env);
    if (p->pp_pending) {
        const lg_buffers &b = lg_internal_host_params(p->env)->buf;
        ppok_process_step(&p->dev, b.rew, b.reset, p->pp_use_tos ? b.extras_time_outs : nullptr, p->pp_t, p->stream);
        p->pp_pending = 0;
    }
}

// ------------------------------------------------------------------ recurrent learner (ActorCriticRecurrent)
static void rnn_net_params(lg_ppo *p, int z, RnnNetArgs &n) {
    const Rnn &q = p->rnn;
    n.Wih = p->dev.params + q.w_ih[z]; n.Whh = p->dev.params + q.w_hh[z];
    n.bih = p->dev.params + q.b_ih[z]; n.bhh = p->dev.params + q.b_hh[z];
}

// one step of the selected memories (mask bit z) on all N envs from (tmp_h, tmp_c) or, at rollout step t >= 0, from the saved state
// of step t; the new state goes to the live buffers
void rnn_live_step(lg_ppo *p, int mask, const float *x0, const float *x1, int t) {
    Rnn &q = p->rnn;
    const int N = p->cfg.num_envs, H = q.H;
    RnnStepArgs a;
    memset(&a, 0, sizeof(a));
    a.M = N; a.H = H; a.reload_all = 1;
    const float *x[2] = {x0, x1};
    int nz = 0;
    for (int z = 0; z < 2; ++z) {
        if (!(mask & (1 << z))) continue;
        RnnNetArgs &n = a.n[nz++];
        rnn_net_params(p, z, n);
        n.X = x[z]; n.ldx = q.in_dim[z]; n.K = q.in_dim[z];
        n.h_sv = t >= 0 ? q.sv_h[z] + (size_t)t * N * H : q.tmp_h[z];
        n.c_sv = t >= 0 ? q.sv_c[z] + (size_t)t * N * H : q.tmp_c[z];
        n.h_out = q.h[z]; n.c_out = q.c[z];
    }
    ppok_lstm_fwd(&a, nz, p->stream);
}

// copy the live state of the selected memories to the saved state of rollout step t (t < 0: to tmp)
void rnn_stash_live(lg_ppo *p, int mask, int t) {
    Rnn &q = p->rnn;
    const size_t nh = (size_t)p->cfg.num_envs * q.H;
    for (int z = 0; z < 2; ++z) {
        if (!(mask & (1 << z))) continue;
        float *dh = t >= 0 ? q.sv_h[z] + (size_t)t * nh : q.tmp_h[z];
        float *dc = t >= 0 ? q.sv_c[z] + (size_t)t * nh : q.tmp_c[z];
        (void)hipMemcpyAsync(dh, q.h[z], nh * sizeof(float), hipMemcpyDeviceToDevice, p->stream);
        (void)hipMemcpyAsync(dc, q.c[z], nh * sizeof(float), hipMemcpyDeviceToDevice, p->stream);
    }
}

// update forward of minibatch mb: the input projection of all T x mbs rows in one GEMM, then T step launches
void rnn_forward_seq(lg_ppo *p, int mb) {
    Rnn &q = p->rnn;
    PpoDev &d = p->dev;
    const int T = d.T, N = d.N, mbs = q.mbs, H = q.H, R = d.mb_rows, e0 = mb * mbs;
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    for (int z = 0; z < 2; ++z) {
        gemm_problem(g, z, z ? d.mb_critic_obs : d.mb_obs, z ? d.OCp : d.Op, d.params + q.w_ih[z], q.in_dim[z], q.pg[z], 4 * H,
                     R, 4 * H, q.in_dim[z]);
        g.bias[z] = d.params + q.b_ih[z];
    }
    g.elu = 0;
    ppok_gemm_fwd(&g, 2, p->stream);
    for (int t = 0; t < T; ++t) {
        RnnStepArgs a;
        memset(&a, 0, sizeof(a));
        a.M = mbs; a.H = H;
        a.reload_all = t == 0;
        a.reload = t ? d.st_dones + (size_t)(t - 1) * N + e0 : nullptr;
        for (int z = 0; z < 2; ++z) {
            RnnNetArgs &n = a.n[z];
            rnn_net_params(p, z, n);
            const size_t r0 = (size_t)t * mbs, rp = (size_t)(t ? t - 1 : 0) * mbs;
            n.P = q.pg[z] + r0 * 4 * H; n.ldp = 4 * H;
            n.h_prev = t ? q.hout[z] + rp * H : nullptr; n.c_prev = t ? q.cout[z] + rp * H : nullptr;
            n.h_sv = q.sv_h[z] + ((size_t)t * N + e0) * H; n.c_sv = q.sv_c[z] + ((size_t)t * N + e0) * H;
            n.h_out = q.hout[z] + r0 * H; n.c_out = q.cout[z] + r0 * H;
            n.gates = q.gates[z] + r0 * 4 * H;
            n.h_used = q.hused[z] + r0 * H; n.c_used = q.cused[z] + r0 * H;
        }
        ppok_lstm_fwd(&a, 2, p->stream);
    }
}

// update backward of minibatch mb, after the MLP backward left dL/dh in rnn.dh: T step launches back through time, then the
// weight gradients over all T x mbs rows (dW_ih = dG^T X, dW_hh = dG^T h_used, db_ih = db_hh = colsum dG)
void rnn_backward_seq(lg_ppo *p, int mb) {
    Rnn &q = p->rnn;
    PpoDev &d = p->dev;
    const int T = d.T, N = d.N, mbs = q.mbs, H = q.H, R = d.mb_rows, e0 = mb * mbs;
    for (int z = 0; z < 2; ++z) (void)hipMemsetAsync(q.dc[z], 0, (size_t)mbs * H * sizeof(float), p->stream);
    for (int t = T - 1; t >= 0; --t) {
        RnnBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.M = mbs; a.H = H;
        a.cut_next = t < T - 1 ? d.st_dones + (size_t)t * N + e0 : nullptr;
        a.cut = t ? d.st_dones + (size_t)(t - 1) * N + e0 : nullptr;
        a.cut_all = t == 0;
        for (int z = 0; z < 2; ++z) {
            RnnBwdNet &n = a.n[z];
            const size_t r0 = (size_t)t * mbs;
            n.dG_next = t < T - 1 ? q.pg[z] + (r0 + mbs) * 4 * H : nullptr;
            n.Whh = d.params + q.w_hh[z];
            n.dh_mlp = q.dh[z] + r0 * H;
            n.dc = q.dc[z];
            n.gates = q.gates[z] + r0 * 4 * H; n.c_t = q.cout[z] + r0 * H; n.c_used = q.cused[z] + r0 * H;
            n.dG = q.pg[z] + r0 * 4 * H;
        }
        ppok_lstm_bwd(&a, 2, p->stream);
    }
    for (int w = 0; w < 2; ++w) {                   // 0: W_ih against the gathered inputs, 1: W_hh against the states used
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        gemm_det(g, d);
        for (int z = 0; z < 2; ++z) {
            if (w == 0) {
                const int ldp = z ? d.OCp : d.Op;
                gemm_problem(g, z, q.pg[z], 4 * H, z ? d.mb_critic_obs : d.mb_obs, ldp, d.grads + q.w_ih[z], q.in_dim[z], 4 * H, ldp, R);
                if (ldp != q.in_dim[z]) g.nstore[z] = q.in_dim[z];
            } else
                gemm_problem(g, z, q.pg[z], 4 * H, q.hused[z], H, d.grads + q.w_hh[z], H, 4 * H, H, R);
        }
        ppok_gemm_dw(&g, 2, p->stream);
    }
    RnnBiasArgs b;
    memset(&b, 0, sizeof(b));
    b.M = R; b.H = H;
    for (int z = 0; z < 2; ++z) { b.dG[z] = q.pg[z]; b.db_ih[z] = d.grads + q.b_ih[z]; b.db_hh[z] = d.grads + q.b_hh[z]; }
    ppok_lstm_bias_grad(&d, &b, p->stream);
}

}  // namespace sched
