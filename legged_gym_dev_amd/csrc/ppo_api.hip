// C-ABI (include/legged_hip.h, lg_ppo_*) for the PPO learner: parameter/storage allocation in HBM and the entries.  What an entry
// launches, on which stream and in which order, is ppo_sched.hip's; the handle is ppo_learner.h's.
#include <cstdlib>
#include <cstring>

#include "ppo_learner.h"

extern "C" {

int lg_ppo_destroy(lg_ppo *p) {
    if (!p) return 0;
    if (p->env) { sched::flush_rollout_epilogue(p); lg_internal_defer_finalize(p->env, 0); p->env = nullptr; }
    if (p->side) { (void)hipStreamSynchronize(p->side); (void)hipStreamDestroy(p->side); }
    if (p->ev_dz) (void)hipEventDestroy(p->ev_dz);
    if (p->ev_side) (void)hipEventDestroy(p->ev_side);
    if (p->ev_bucket) (void)hipEventDestroy(p->ev_bucket);
    for (hipEvent_t e : p->comm_ev) (void)hipEventDestroy(e);
    for (void *q : p->allocs) (void)hipFree(q);
    delete p;
    return 0;
}

static int ppo_create(const lg_ppo_cfg *cfg, const lg_ppo_rnn_cfg *rc, lg_ppo **out) {
    if (!cfg || !out) { lg_set_error("null argument"); return -1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { lg_set_error("no HIP device: no CPU fallback"); return -2; }
    if (cfg->activation < 0 || cfg->activation > 5) { lg_set_error("activation must be one of 0 elu, 1 selu, 2 relu (also rsl_rl's crelu), 3 lrelu, 4 tanh, 5 sigmoid"); return -3; }
    if (cfg->num_hidden < 1 || cfg->num_hidden > LG_MAX_HIDDEN || cfg->num_actions > LG_PPO_MAX_A) {
        lg_set_error("unsupported network size"); return -4;
    }
    const int N = cfg->num_envs, T = cfg->num_steps, A = cfg->num_actions, O = cfg->num_obs;
    const int OC = cfg->num_critic_obs > 0 ? cfg->num_critic_obs : O;
    if ((long)N * T % cfg->num_mini_batches != 0 && (long)N * T / cfg->num_mini_batches == 0) { lg_set_error("bad minibatch count"); return -5; }
    const int H = rc ? rc->hidden : 0;
    if (rc) {
        if (rc->type != 0) { lg_set_error("recurrent policy: only rnn_type 'lstm' (0) is implemented"); return -6; }
        if (rc->layers != 1) { lg_set_error("recurrent policy: only rnn_num_layers = 1 is implemented"); return -6; }
        if (H < 32 || H > 512 || H % 32) { lg_set_error("recurrent policy: rnn_hidden_size must be a multiple of 32 in [32, 512]"); return -6; }
    }
    lg_ppo *p = new lg_ppo();
    p->cfg = *cfg;
    p->act_code = cfg->activation + 1;
    p->fused_act = getenv("LG_FUSED_ACT") ? atoi(getenv("LG_FUSED_ACT")) : 1;   // one-launch rollout forward (ppo_mlp_fused.hip) when the shape allows
    p->overlap = getenv("LG_PPO_OVERLAP") ? atoi(getenv("LG_PPO_OVERLAP")) : 1;
    if (hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_dz, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_side, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_bucket, hipEventDisableTiming) != hipSuccess) {
        lg_set_error("stream/event creation failed"); delete p; return -100;
    }
    const int R = (int)((long)N * T / cfg->num_mini_batches);
    p->Mmax = R > N ? R : N;

    // parameter layout: std, actor (W,b)*, critic (W,b)*  -- the order of ActorCritic.parameters()
    int64_t off = 0;
    PpoDev &d = p->dev;
    d.off_std = (int)off; off += A;
    for (int z = 0; z < 2; ++z) {
        Net &n = p->net[z];
        n.nl = cfg->num_hidden + 1;
        n.dims[0] = H ? H : z == 0 ? O : OC;              // a recurrent learner's MLPs read the LSTM's hidden state
        for (int l = 0; l < cfg->num_hidden; ++l) n.dims[l + 1] = z == 0 ? cfg->actor_hidden[l] : cfg->critic_hidden[l];
        n.dims[n.nl] = z == 0 ? A : 1;
        for (int l = 0; l < n.nl; ++l) {
            n.w_off[l] = off; off += (int64_t)n.dims[l + 1] * n.dims[l];
            n.b_off[l] = off; off += n.dims[l + 1];
        }
    }
    if (H) {                                 // then memory_a.rnn.*, memory_c.rnn.*: weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0
        Rnn &q = p->rnn;
        q.H = H; q.mbs = N / cfg->num_mini_batches;
        for (int z = 0; z < 2; ++z) {
            q.in_dim[z] = z == 0 ? O : OC;
            q.w_ih[z] = off; off += (int64_t)4 * H * q.in_dim[z];
            q.w_hh[z] = off; off += (int64_t)4 * H * H;
            q.b_ih[z] = off; off += 4 * H;
            q.b_hh[z] = off; off += 4 * H;
        }
        p->fused_act = 0;                    // the one-launch rollout forward has no LSTM stage
    }
    d.num_params = off;
    int seg_ld[LG_PPO_MAX_SEG];
    {   // bf16 plane layout: one segment per weight matrix, 16-byte aligned
        int64_t po = 0;
        d.nseg = 0;
        for (int z = 0; z < 2; ++z)
            for (int l = 0; l < p->net[z].nl; ++l) {
                Net &n = p->net[z];
                n.pl_off[l] = po;
                d.seg_off[d.nseg] = n.w_off[l]; d.seg_pl[d.nseg] = po;
                d.seg_rows[d.nseg] = n.dims[l + 1]; d.seg_cols[d.nseg] = n.dims[l];
                // rows of the first layer's image padded to whole k-tiles of 32 (the observation width need not be one: 48, 235, 169, 65):
                // the LDS-DMA forward (ppo_gemm_glds.h) moves whole k-tiles, the plane path of k_gemm whole 16-byte chunks
                const int ld = l == 0 ? (n.dims[0] + 31) / 32 * 32 : n.dims[l];
                if (l == 0) n.pl_ld0 = ld;
                seg_ld[d.nseg] = ld;
                ++d.nseg;
                po += ((int64_t)n.dims[l + 1] * ld + 7) / 8 * 8;
            }
        d.pl_stride = po;
    }
    d.off_bias_actor_head = (int)p->net[0].b_off[p->net[0].nl - 1];
    d.off_bias_critic_head = (int)p->net[1].b_off[p->net[1].nl - 1];
    d.N = N; d.T = T; d.A = A; d.O = O; d.OC = OC; d.mb_rows = R;
    d.Op = (O + 31) / 32 * 32; d.OCp = (OC + 31) / 32 * 32;
    d.world = cfg->world_size > 0 ? cfg->world_size : 1;
    d.env_offset = 0;
    d.adaptive = cfg->adaptive_schedule; d.clipped_value = cfg->use_clipped_value_loss;
    d.seed = cfg->seed;
    d.gamma = cfg->gamma; d.lam = cfg->lam; d.clip = cfg->clip_param; d.value_coef = cfg->value_loss_coef;
    d.entropy_coef = cfg->entropy_coef; d.desired_kl = cfg->desired_kl; d.max_grad_norm = cfg->max_grad_norm;

    PA(d.params, off + 2); PA(d.grads, off + 2); PA(d.adam_m, off + 2); PA(d.adam_v, off + 2);
    {
        const int64_t pls = d.pl_stride;            // PA memsets through d.*: keep the stride across the allocation macros
        PA(d.wpl, (size_t)3 * pls + 8);
        PA(d.pl_dest, (size_t)off + 2);
        std::vector<int32_t> dest((size_t)off + 2, -1);
        for (int sg = 0; sg < d.nseg; ++sg)
            for (int64_t e = 0; e < (int64_t)d.seg_rows[sg] * d.seg_cols[sg]; ++e)
                dest[d.seg_off[sg] + e] = (int32_t)(d.seg_pl[sg] + (e / d.seg_cols[sg]) * seg_ld[sg] + e % d.seg_cols[sg]);
        (void)hipMemcpy(d.pl_dest, dest.data(), dest.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    const size_t TN = (size_t)T * N;
    PA(d.st_obs, TN * O);
    if (cfg->num_critic_obs > 0) PA(d.st_critic_obs, TN * OC); else d.st_critic_obs = d.st_obs;
    PA(d.st_actions, TN * A); PA(d.st_rewards, TN); PA(d.st_values, TN); PA(d.st_returns, TN); PA(d.st_adv, TN);
    PA(d.st_log_prob, TN); PA(d.st_mu, TN * A); PA(d.st_sigma, A); PA(d.st_dones, TN);
    PA(d.act_actions, (size_t)N * A); PA(d.act_values, N); PA(d.act_log_prob, N); PA(d.act_mu, (size_t)N * A);
    PA(d.stats, 8); PA(d.loss_acc, 4 + LG_NORM_BLOCKS); PA(d.noise, (size_t)N * A); PA(d.perm, TN); PA(d.adv_partial, 4);
    for (int k = 0; k < 2; ++k) {
        lg_ppo::MbSet &m = p->mbset[k];
        PA(m.obs, (size_t)R * d.Op);                // pad columns: zeroed here, never written
        if (cfg->num_critic_obs > 0) PA(m.critic_obs, (size_t)R * d.OCp); else m.critic_obs = m.obs;
        PA(m.actions, (size_t)R * A); PA(m.mu, (size_t)R * A); PA(m.scalars, (size_t)R * 4);
    }
    use_mb_set(d, p->mbset[p->mb_cur]);
    PA(d.head_part, ppok_head_part_floats());
    PA(d.cur_reward_sum, N); PA(d.cur_episode_len, N); PA(d.ep_stats, 4); PA(d.ep_ring, 200); PA(d.ep_ring_count, 1);
    for (int z = 0; z < 2; ++z) {
        Net &n = p->net[z];
        n.act[0] = nullptr; n.dz[0] = nullptr;
        for (int l = 1; l <= n.nl; ++l) { PA(n.act[l], (size_t)p->Mmax * n.dims[l]); PA(n.dz[l], (size_t)p->Mmax * n.dims[l]); }
    }
    if (H) {
        Rnn &q = p->rnn;
        const size_t NH = (size_t)N * H, Rr = (size_t)R;
        for (int z = 0; z < 2; ++z) {
            PA(q.h[z], NH); PA(q.c[z], NH); PA(q.sv_h[z], TN * H); PA(q.sv_c[z], TN * H); PA(q.tmp_h[z], NH); PA(q.tmp_c[z], NH);
            PA(q.pg[z], Rr * 4 * H); PA(q.gates[z], Rr * 4 * H);
            PA(q.hout[z], Rr * H); PA(q.cout[z], Rr * H); PA(q.hused[z], Rr * H); PA(q.cused[z], Rr * H); PA(q.dh[z], Rr * H);
            PA(q.dc[z], (size_t)q.mbs * H);
        }
        // rsl_rl's reccurent_mini_batch_generator: no permutation, minibatch mb = envs [mb mbs, (mb + 1) mbs) over all T steps, rows
        // t-major -- as a fixed gather table, so the MLP's gathers (and the gather-ahead of the optimiser step) serve it unchanged.
        // A learner whose envs do not split into whole minibatches (play / inference on one env) is created but refuses to update.
        std::vector<int32_t> perm(TN);
        for (int mb = 0; N % cfg->num_mini_batches == 0 && mb < cfg->num_mini_batches; ++mb)
            for (int t = 0; t < T; ++t)
                for (int e = 0; e < q.mbs; ++e) perm[(size_t)mb * R + (size_t)t * q.mbs + e] = (int32_t)((size_t)t * N + (size_t)mb * q.mbs + e);
        (void)hipMemcpy(d.perm, perm.data(), TN * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (p->fused_act) {                                         // arguments + weight image of the one-launch rollout forward
        MlpArgs &g = p->mlp;
        g.params = d.params; g.M = N; g.nl = p->net[0].nl; g.act = p->act_code;
        int64_t tot = 0;
        if (p->net[0].nl != p->net[1].nl) p->fused_act = 0;
        for (int z = 0; z < 2 && p->fused_act; ++z) {
            Net &n = p->net[z];
            for (int l = 0; l <= n.nl; ++l) g.dims[z][l] = n.dims[l];
            for (int l = 0; l < n.nl; ++l) {
                g.w_off[z][l] = n.w_off[l]; g.b_off[z][l] = n.b_off[l]; g.frag_off[z][l] = tot;
                tot += ppok_mlp_frag_elems(n.dims[l], n.dims[l + 1]);
            }
        }
        if (p->fused_act && ppok_mlp_supported(&g) != 0) p->fused_act = 0;
        if (p->fused_act) { uint16_t *wf = nullptr; PA(wf, (size_t)tot); g.wfrag = wf; }
    }
    {   // std = init_noise_std, lr = learning_rate
        std::vector<float> h(A, cfg->init_noise_std);
        (void)hipMemcpy(d.params + d.off_std, h.data(), sizeof(float) * A, hipMemcpyHostToDevice);
        float lr = cfg->learning_rate;
        (void)hipMemcpy(d.stats, &lr, sizeof(float), hipMemcpyHostToDevice);
    }
    lg_ppo_buffers &b = p->pub;
    b.params = d.params; b.grads = d.grads; b.adam_m = d.adam_m; b.adam_v = d.adam_v;
    b.obs = d.st_obs; b.critic_obs = d.st_critic_obs; b.actions = d.st_actions; b.rewards = d.st_rewards;
    b.values = d.st_values; b.returns = d.st_returns; b.advantages = d.st_adv; b.log_prob = d.st_log_prob;
    b.mu = d.st_mu; b.sigma = d.st_sigma; b.dones = d.st_dones;
    b.act_actions = d.act_actions; b.act_values = d.act_values; b.act_log_prob = d.act_log_prob; b.act_mu = d.act_mu;
    b.stats = d.stats; b.noise = d.noise; b.perm = d.perm; b.adv_partial = d.adv_partial;
    b.cur_reward_sum = d.cur_reward_sum; b.cur_episode_len = d.cur_episode_len; b.ep_stats = d.ep_stats;
    b.ep_ring = d.ep_ring; b.ep_ring_count = d.ep_ring_count;
    b.num_params = off; b.num_reduce = off + 2;
    if (hipDeviceSynchronize() != hipSuccess) { lg_set_error("device sync failed in lg_ppo_create"); lg_ppo_destroy(p); return -100; }
    *out = p;
    return 0;
}

int lg_ppo_create(const lg_ppo_cfg *cfg, lg_ppo **out) { return ppo_create(cfg, nullptr, out); }
int lg_ppo_create_recurrent(const lg_ppo_cfg *cfg, const lg_ppo_rnn_cfg *rnn, lg_ppo **out) {
    if (!rnn) { lg_set_error("null argument"); return -1; }
    return ppo_create(cfg, rnn, out);
}
int lg_ppo_get_rnn_buffers(lg_ppo *p, lg_ppo_rnn_buffers *out) {
    if (!p->rnn.H) { lg_set_error("lg_ppo_get_rnn_buffers: not a recurrent learner"); return -15; }
    for (int z = 0; z < 2; ++z) {
        out->h[z] = p->rnn.h[z]; out->c[z] = p->rnn.c[z]; out->saved_h[z] = p->rnn.sv_h[z]; out->saved_c[z] = p->rnn.sv_c[z];
    }
    out->hidden = p->rnn.H;
    return 0;
}
int lg_ppo_reset_hidden(lg_ppo *p, const uint8_t *dones) {
    if (!p->rnn.H) { lg_set_error("lg_ppo_reset_hidden: not a recurrent learner"); return -15; }
    sched::flush_rollout_epilogue(p);
    const Rnn &q = p->rnn;
    ppok_lstm_reset(q.h[0], q.c[0], q.h[1], q.c[1], dones, p->cfg.num_envs, q.H, p->stream);
    return launch_ok();
}
int lg_ppo_get_buffers(lg_ppo *p, lg_ppo_buffers *out) { *out = p->pub; return 0; }
int lg_ppo_set_stream(lg_ppo *p, void *s) { p->stream = (hipStream_t)s; return 0; }
int lg_ppo_inject_noise(lg_ppo *p, int enable) { p->inject = enable; return 0; }
int lg_ppo_debug_set_overlap(lg_ppo *p, int v) { p->overlap = v; return 0; }
int lg_ppo_debug_set_fused_act(lg_ppo *p, int v) { p->fused_act = v && p->mlp.wfrag; return 0; }
int lg_ppo_debug_get_fused_act(lg_ppo *p) { return p->fused_act; }          // 1: lg_ppo_act runs the one-launch forward for this shape
int lg_ppo_debug_set_act_count(lg_ppo *p, long long v) { p->act_count = v; return 0; }   // replay the same Philox draws (tests)

// entries: std, then per net per layer (W, b).  offsets[i]; shapes[2i] = rows, shapes[2i+1] = cols (0 for vectors)
int lg_ppo_param_layout(lg_ppo *p, int64_t *offsets, int64_t *shapes, int max_entries) {
    int k = 0;
    auto put = [&](int64_t o, int64_t r, int64_t c) {
        if (k < max_entries) { offsets[k] = o; shapes[2 * k] = r; shapes[2 * k + 1] = c; }
        ++k;
    };
    put(p->dev.off_std, p->cfg.num_actions, 0);
    for (int z = 0; z < 2; ++z)
        for (int l = 0; l < p->net[z].nl; ++l) {
            put(p->net[z].w_off[l], p->net[z].dims[l + 1], p->net[z].dims[l]);
            put(p->net[z].b_off[l], p->net[z].dims[l + 1], 0);
        }
    const Rnn &q = p->rnn;
    for (int z = 0; q.H && z < 2; ++z) {
        put(q.w_ih[z], 4 * q.H, q.in_dim[z]);
        put(q.w_hh[z], 4 * q.H, q.H);
        put(q.b_ih[z], 4 * q.H, 0);
        put(q.b_hh[z], 4 * q.H, 0);
    }
    return k;
}

int lg_ppo_attach_env(lg_ppo *p, lg_ctx *env) {
    sched::flush_rollout_epilogue(p);
    if (p->env) lg_internal_defer_finalize(p->env, 0);
    p->env = nullptr;
    if (env) {
        if (lg_internal_host_params(env)->cfg.num_envs != p->cfg.num_envs) { lg_set_error("lg_ppo_attach_env: env and learner differ in num_envs"); return -12; }
        // the fused epilogue reads the env's rew / reset / time_out inside the learner's next act launch: only stream order makes that safe
        if (lg_internal_stream(env) != p->stream) { lg_set_error("lg_ppo_attach_env: env and learner must run on the same stream (lg_set_stream / lg_ppo_set_stream)"); return -12; }
        p->env = env;
        lg_internal_defer_finalize(env, 1);
    }
    return launch_ok();
}

int lg_ppo_act(lg_ppo *p, const float *obs, const float *critic_obs) {
    if (p->step >= p->cfg.num_steps) { lg_set_error("Rollout buffer overflow"); return -10; }
    const float *cobs = critic_obs ? critic_obs : obs;
    int fused = -1;
    // rollout images of the weights (fragment-order image / bf16 planes) are rebuilt when the parameters changed since they were built AND
    // at the first act of every rollout: a write through the zero-copy parameter views without lg_ppo_params_changed() is then stale for
    // at most the rollout in progress.  The flag is cleared once the launch that consumed it has gone out.
    const bool dirty = p->params_dirty != 0 || p->step == 0;
    if (p->fused_act) {
        // the image is rebuilt from the fp32 parameters whenever they changed since it was built (optimiser step, broadcast, or a
        // host write announced through lg_ppo_params_changed: checkpoint load, load_state_dict) -- also in the middle of a rollout
        MlpArgs &g = p->mlp;
        g.in[0] = obs; g.in[1] = cobs;
        g.out[0] = p->net[0].act[p->net[0].nl]; g.out[1] = p->net[1].act[p->net[1].nl];
        if (dirty) ppok_mlp_frag_build(&g, p->stream);
        // sampled and stored by the same launch (a separate k_act_sample: rollout 4.40 / 4.41 ms against 4.15 / 4.19, profiles/r02_ab.txt)
        g.t = p->step; g.inject = p->inject; g.act_count = p->act_count;
        g.pp = 0;
        const int N = p->cfg.num_envs;
        const bool fits = (N + 255) / 256 + 1 <= (N + 31) / 32;  // epilogue workgroups within the launch's grid.x
        if (p->env && p->pp_pending && fits) {        // the previous step's epilogue rides on this launch
            g.pp = lg_internal_finalize_pending(p->env) ? 2 : 1;
            g.pp_t = p->pp_t; g.pp_use_tos = p->pp_use_tos;
            g.pp_env = lg_internal_take_finalize(p->env, &g.pp_counter);
            p->pp_pending = 0;
        } else sched::flush_rollout_epilogue(p);
        fused = ppok_mlp_fwd(&g, &p->dev, p->stream);
        if (fused != 0 && g.pp) { lg_set_error("fused act launch refused with a rollout epilogue attached"); return -13; }
        if (fused == 0) {                                                         // sampled and stored by the same launch
            p->act_count++;
            const int rc = launch_ok();
            if (rc == 0) p->params_dirty = 0;
            return rc;
        }
    }
    if (!p->fused_act) sched::flush_rollout_epilogue(p);
    if (fused != 0) {
        // per-layer GEMMs on the optimiser's weight planes (no re-split of W per tile); same freshness rule as above
        if (dirty) ppok_sync_planes(&p->dev, p->stream);
        const float *in0 = obs, *in1 = cobs;
        if (p->rnn.H) {                          // the transition keeps the state before the step; both memories advance
            sched::rnn_stash_live(p, 3, p->step);
            sched::rnn_live_step(p, 3, obs, cobs, p->step);
            in0 = p->rnn.h[0]; in1 = p->rnn.h[1];
        }
        sched::FwdOpts fo{};
        fo.planes = true;
        sched::forward(p, p->cfg.num_envs, in0, in1, 3, fo);
    }
    ppok_act_sample(&p->dev, obs, cobs, p->net[0].act[p->net[0].nl], p->net[1].act[p->net[1].nl], p->step, p->act_count,
                    p->inject, p->stream);
    p->act_count++;
    const int rc = launch_ok();
    if (rc == 0) p->params_dirty = 0;
    return rc;
}

int lg_ppo_process_env_step(lg_ppo *p, const float *rew, const uint8_t *dones, const uint8_t *time_outs) {
    if (p->step >= p->cfg.num_steps) { lg_set_error("Rollout buffer overflow"); return -10; }
    if (p->env) {
        // attached env: when the arguments are that env's own step outputs, record the call for the next act launch
        const lg_buffers &b = lg_internal_host_params(p->env)->buf;
        if (p->fused_act && !p->pp_pending && rew == b.rew && dones == b.reset && (!time_outs || time_outs == b.extras_time_outs)) {
            p->pp_pending = 1; p->pp_t = p->step; p->pp_use_tos = time_outs != nullptr;
            p->step++;
            return 0;
        }
        sched::flush_rollout_epilogue(p);
    }
    ppok_process_step(&p->dev, rew, dones, time_outs, p->step, p->stream);
    if (p->rnn.H) ppok_lstm_reset(p->rnn.h[0], p->rnn.c[0], p->rnn.h[1], p->rnn.c[1], dones, p->cfg.num_envs, p->rnn.H, p->stream);
    p->step++;
    return launch_ok();
}

int lg_ppo_compute_returns(lg_ppo *p, const float *last_critic_obs) {
    sched::flush_rollout_epilogue(p);
    if (p->rnn.H) {                              // rsl_rl's evaluate() advances memory_c once more on the last observations
        sched::rnn_stash_live(p, 2, -1);
        sched::rnn_live_step(p, 2, nullptr, last_critic_obs, -1);
        sched::forward(p, p->cfg.num_envs, nullptr, p->rnn.h[1], 2);
    } else
        sched::forward(p, p->cfg.num_envs, nullptr, last_critic_obs, 2);
    ppok_gae(&p->dev, p->net[1].act[p->net[1].nl], p->stream);
    return launch_ok();
}

int lg_ppo_normalize_advantages(lg_ppo *p) {
    ppok_adv_normalize(&p->dev, p->stream);
    return launch_ok();
}

static int rnn_update_refused(const lg_ppo *p) {
    if (!p->rnn.H || p->cfg.num_envs % p->cfg.num_mini_batches == 0) return 0;
    lg_set_error("recurrent policy: the update needs num_envs to be a multiple of num_mini_batches (its minibatches are whole envs)");
    return 1;
}

int lg_ppo_begin_update(lg_ppo *p) {
    if (rnn_update_refused(p)) return -6;
    sched::flush_rollout_epilogue(p);
    // randperm(num_mini_batches * mini_batch_size), drawn once per update and reused by every epoch (Appendix B): on the device
    const size_t n = (size_t)p->dev.mb_rows * p->cfg.num_mini_batches;
    if (!p->rnn.H) ppok_randperm(&p->dev, (int)n, (uint64_t)p->perm_count++, p->stream);   // recurrent: the fixed table of create
    p->mb_ready = -1;                           // a set gathered ahead belongs to the previous permutation
    (void)hipMemsetAsync(p->dev.stats + 2, 0, 2 * sizeof(float), p->stream);
    (void)hipMemsetAsync(p->dev.stats + 5, 0, sizeof(float), p->stream);
    (void)hipMemsetAsync(p->dev.loss_acc, 0, 4 * sizeof(float), p->stream);
    p->grads_dirty = 1;                      // first backward of this update clears the gradient buffer
    ppok_sync_planes(&p->dev, p->stream);    // weight planes follow whatever the fp32 parameters hold now
    return launch_ok();
}

int lg_ppo_minibatch_backward(lg_ppo *p, int epoch, int mb) {
    (void)epoch;
    if (rnn_update_refused(p)) return -6;
    PpoDev &d = p->dev;
    const int R = d.mb_rows;
    // k_opt_adam leaves the gradient buffer zeroed; only a backward pass that was never stepped needs a clear
    if (p->grads_dirty) (void)hipMemsetAsync(d.grads, 0, (size_t)(d.num_params + 2) * sizeof(float), p->stream);
    p->grads_dirty = 1;
    if (p->mb_ready == mb) {                                    // gathered ahead by the previous optimiser step
        p->mb_cur ^= 1;
        use_mb_set(d, p->mbset[p->mb_cur]);
    } else {
        ppok_gather(&d, mb, p->stream);
    }
    p->mb_ready = -1;
    p->mb_last = mb;
    Net &na = p->net[0], &nc = p->net[1];
    const int nl = na.nl, H3 = na.dims[nl - 1];
    // fused head (forward + loss + backward of the two thin head layers) when both nets end in the same
    // supported width; otherwise head GEMMs + k_loss
    // at 128 wide the fused head was 18 us slower per minibatch while the weight-gradient stream had slack; with that stream the
    // long pole (profiles/r02_timelines.txt) it is 9 us faster than head GEMM + k_loss + two head-gradient GEMMs (A/B on one box)
    const bool fuse = p->act_code == 1 && nl >= 2 && nc.dims[nl - 1] == H3 && (H3 == 128 || H3 == 64 || H3 == 32);
    sched::FwdOpts fo{};
    fo.skip_head = fuse; fo.planes = true; fo.in_pad = !p->rnn.H;       // the LSTM's output rows are not padded, the gathers are
    if (p->rnn.H) {
        sched::rnn_forward_seq(p, mb);
        sched::forward(p, R, p->rnn.hout[0], p->rnn.hout[1], 3, fo);
    } else
        sched::forward(p, R, d.mb_obs, d.mb_critic_obs, 3, fo);
    if (fuse) {
        ppok_head_fused(&d, H3, na.act[nl - 1], nc.act[nl - 1], na.dz[nl - 1], nc.dz[nl - 1], na.w_off[nl - 1], na.b_off[nl - 1],
                        nc.w_off[nl - 1], nc.b_off[nl - 1], na.b_off[nl - 2], nc.b_off[nl - 2], p->stream);
    } else {
        ppok_loss(&d, na.act[na.nl], nc.act[nc.nl], na.dz[na.nl], nc.dz[nc.nl], p->stream);
    }
    if (fuse && p->comm) sched::reduce_layer_bucket(p, nl - 1, p->stream);   // the fused head produced the head layer's gradients itself
    if (p->rnn.H) {
        sched::backward(p, R, p->rnn.hout[0], p->rnn.hout[1], fuse);
        sched::rnn_backward_seq(p, mb);
    } else
        sched::backward(p, R, d.mb_obs, d.mb_critic_obs, fuse);
    if (d.det64) ppok_det_fold(&d, p->stream);       // gradients, KL sum and loss sums of this minibatch, order-independent
    if (p->comm_rc) { const int rc = p->comm_rc; p->comm_rc = 0; return rc; }
    return launch_ok();
}

int lg_ppo_minibatch_step(lg_ppo *p) {
    int next = -1;
    PpoDev other = p->dev;
    if (p->cfg.num_mini_batches > 1 && p->mb_last >= 0) {
        // the next minibatch of the generator's order (the permutation is fixed for the whole update)
        next = (p->mb_last + 1) % p->cfg.num_mini_batches;
        use_mb_set(other, p->mbset[p->mb_cur ^ 1]);
    }
    if (ppok_step(&p->dev, (int)(p->update_count & 1), &other, next, p->stream)) p->mb_ready = next;
    p->mb_last = -1;
    p->grads_dirty = 0;
    p->params_dirty = 1;
    p->update_count++;
    return launch_ok();
}

int lg_ppo_end_update(lg_ppo *p) { p->step = 0; return 0; }

int lg_ppo_set_comm(lg_ppo *p, lg_comm *c) {
    if (c && p->rnn.H) { lg_set_error("lg_ppo_set_comm: the per-layer gradient buckets do not cover the LSTM of a recurrent learner; reduce the whole gradient buffer between lg_ppo_minibatch_backward and lg_ppo_minibatch_step instead"); return -14; }
    if (c && p->dev.det64) { lg_set_error("gradient buckets inside the backward pass cannot be combined with deterministic mode"); return -14; }
    p->comm = c;
    return 0;
}
int lg_ppo_comm_timing(lg_ppo *p, int enable) { p->comm_timing = enable ? 1 : 0; return 0; }
int lg_ppo_comm_wait_ms(lg_ppo *p, double *ms_total, int64_t *minibatches) {
    if (!ms_total || !minibatches) { lg_set_error("null argument"); return -1; }
    (void)hipStreamSynchronize(p->stream);
    double sum = 0.0;
    for (size_t k = 0; k + 1 < p->comm_ev_used; k += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p->comm_ev[k], p->comm_ev[k + 1]) == hipSuccess) sum += ms;
    }
    *ms_total = sum; *minibatches = (int64_t)(p->comm_ev_used / 2);
    p->comm_ev_used = 0;
    return 0;
}
int lg_ppo_allreduce_adv_moments(lg_ppo *p, lg_comm *c) { return lg_comm_allreduce_sum(c, p->dev.adv_partial, 4, p->stream); }
int lg_ppo_broadcast_params(lg_ppo *p, lg_comm *c, int root) {
    p->params_dirty = 1;
    return lg_comm_broadcast(c, p->dev.params, p->dev.num_params + 2, root, p->stream);
}
int lg_ppo_params_changed(lg_ppo *p) { p->params_dirty = 1; return 0; }

int lg_ppo_set_deterministic(lg_ppo *p, int on) {
    if (on && p->comm) { lg_set_error("deterministic mode cannot be combined with gradient buckets reduced inside the backward pass (lg_ppo_set_comm)"); return -14; }
    if (on && !p->det_buf) {
        const size_t n = LG_DET_WORDS(p->dev.num_params);
        void *q = nullptr;
        if (hipMalloc(&q, n * sizeof(long long)) != hipSuccess || hipMemset(q, 0, n * sizeof(long long)) != hipSuccess) {
            lg_set_error("hipMalloc failed in lg_ppo_set_deterministic"); return -100;
        }
        p->allocs.push_back(q);
        p->det_buf = (long long *)q;
    }
    if (!on && p->dev.det64) ppok_det_fold(&p->dev, p->stream);    // nothing stays behind in the shadow
    p->dev.det64 = on ? p->det_buf : nullptr;
    return launch_ok();
}

// The extents sched::reduce_layer_bucket() hands to RCCL for layer l, as offsets into the flat gradient buffer (host-side, for tests:
// the buckets of all layers must tile [0, num_reduce) exactly once).  Returns the number of extents (<= 4).
int lg_ppo_debug_bucket_extents(lg_ppo *p, int l, int64_t *offsets, int64_t *counts) {
    if (l < 0 || l >= p->net[0].nl) return -1;
    float *bufs[4];
    const int n = sched::bucket_extents(p, l, bufs, counts);
    for (int k = 0; k < n; ++k) offsets[k] = bufs[k] - p->dev.grads;
    return n;
}

// The two minibatch buffer sets (host-side, for tests of the gathers): cur[5] = obs, critic_obs, actions, mu, scalars of the set the
// next forward reads (after lg_ppo_minibatch_backward: the one it read), other[5] = those of the set lg_ppo_minibatch_step gathers the
// following minibatch into; dims = {Op, OCp, mb_rows}.
int lg_ppo_debug_mb_sets(lg_ppo *p, void **cur, void **other, int *dims) {
    const PpoDev &d = p->dev;
    const lg_ppo::MbSet &m = p->mbset[p->mb_cur ^ 1];
    void *c[5] = {d.mb_obs, d.mb_critic_obs, d.mb_actions, d.mb_mu, d.mb_scalars};
    void *o[5] = {m.obs, m.critic_obs, m.actions, m.mu, m.scalars};
    for (int k = 0; k < 5; ++k) { cur[k] = c[k]; other[k] = o[k]; }
    dims[0] = d.Op; dims[1] = d.OCp; dims[2] = d.mb_rows;
    return 0;
}

// The split-bf16 weight planes the optimiser step keeps current (host-side, for tests; device pointers only, nothing is launched):
// *wpl = plane h, planes m and l follow *pl_stride and 2 * *pl_stride uint16 elements later (3 * pl_stride + 8 elements in all);
// *pl_dest = int32 [num_params]: element index of each parameter inside a plane, -1 for parameters without an image.
int lg_ppo_debug_weight_planes(lg_ppo *p, void **wpl, int64_t *pl_stride, void **pl_dest) {
    if (!p || !wpl || !pl_stride || !pl_dest) { lg_set_error("null argument"); return -1; }
    *wpl = p->dev.wpl; *pl_stride = p->dev.pl_stride; *pl_dest = p->dev.pl_dest;
    return 0;
}

int lg_ppo_act_inference(lg_ppo *p, const float *obs, float *actions_out, int64_t rows) {
    if (rows > p->Mmax) { lg_set_error("too many rows for act_inference"); return -11; }
    if (p->rnn.H) {                              // rsl_rl's act_inference advances memory_a
        if (rows != p->cfg.num_envs) { lg_set_error("act_inference of a recurrent learner takes exactly num_envs rows"); return -11; }
        sched::rnn_stash_live(p, 1, -1);
        sched::rnn_live_step(p, 1, obs, nullptr, -1);
        obs = p->rnn.h[0];
    }
    sched::forward(p, (int)rows, obs, nullptr, 1);
    Net &na = p->net[0];
    if (hipMemcpyAsync(actions_out, na.act[na.nl], (size_t)rows * p->cfg.num_actions * sizeof(float), hipMemcpyDeviceToDevice,
                       p->stream) != hipSuccess) { lg_set_error("copy failed"); return -100; }
    return launch_ok();
}

}  // extern "C"
