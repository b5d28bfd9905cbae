/* legged_hip.h -- C-ABI of liblegged_hip.so (MI355X / gfx950).
 *
 * The reference has no FFI boundary on this path: the hot loop sits behind two Python
 * duck-typed interfaces:
 *   B1  VecEnv            legged_gym/envs/base/base_task.py:60-81,101-122,
 *                         legged_gym/envs/base/legged_robot.py:80-104
 *   B3  gym tensor API    the ~45 gym.* calls of legged_robot.py (acquire_*_tensor :537-539,
 *                         set_dof_actuation_force_tensor :92, simulate :93, refresh_* :96,111-112,
 *                         set_*_tensor_indexed :428,452,461 ...)
 * and, for the learner, rsl_rl's PPO/RolloutStorage/OnPolicyRunner (call sites
 * legged_gym/utils/task_registry.py:148-155).  This header is the C-ABI introduced UNDERNEATH
 * them; each entry cites the reference interface it replaces.  Plain pointers and PODs only,
 * int return codes (0 = ok, negative = error, text via lg_last_error()), no exceptions cross the
 * boundary.  One context = one HIP device + one stream; a context is not thread-safe.
 *
 * All device pointers handed in or out are HBM addresses on the context's device.
 * The same structs (with host pointers) are used by the CPU oracle in oracle/ (lgo_* symbols),
 * which is test infrastructure and never linked into this library.
 */
#ifndef LEGGED_HIP_H
#define LEGGED_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_MAX_DOF      16
#define LG_MAX_BODIES   24
#define LG_MAX_SPHERES  48
#define LG_MAX_FEET      8
#define LG_MAX_PEN      16
#define LG_MAX_TERM      8
#define LG_LSTM_NW     972   /* actuator net: see lg_cfg.lstm_w */
#define LG_MAX_HIDDEN    4

/* Reward terms in the order the reference sums them: alphabetical by name (class_to_dict walks
 * dir(), legged_gym/utils/helpers.py:111-126); "termination" is applied last, after the optional
 * positive clip (legged_robot.py:189-206). */
enum lg_reward {
    LG_REW_ACTION_RATE = 0, LG_REW_ANG_VEL_XY, LG_REW_BASE_HEIGHT, LG_REW_COLLISION, LG_REW_DOF_ACC,
    LG_REW_DOF_POS_LIMITS, LG_REW_DOF_VEL, LG_REW_DOF_VEL_LIMITS, LG_REW_FEET_AIR_TIME,
    LG_REW_FEET_CONTACT_FORCES, LG_REW_LIN_VEL_Z, LG_REW_NO_FLY, LG_REW_ORIENTATION, LG_REW_STAND_STILL,
    LG_REW_STUMBLE, LG_REW_TERMINATION, LG_REW_TORQUE_LIMITS, LG_REW_TORQUES, LG_REW_TRACKING_ANG_VEL,
    LG_REW_TRACKING_LIN_VEL, LG_NUM_REWARDS
};

/* Per-env random-draw slots.  In normal operation slot s of env e at step k is
 * Philox4x32-10(key = seed, counter = (global env id, k, s / 4, 0))[s % 4] >> 8 scaled to [0,1);
 * with lg_inject_uniforms() the value is read from the injected (N, K) buffer instead (parity
 * tests replay the reference's torch.rand draws this way).  K = LG_SLOT_NOISE(A) + num_obs
 * (LG_TSLOT_NOISE(A) + num_obs for the trajectory env). */
#define LG_SLOT_CMD        0   /* 3: callback command resample x, y, yaw|heading (legged_robot.py:365-387) */
#define LG_SLOT_PUSH       3   /* 2: push velocity xy (:456-461) */
#define LG_SLOT_LEVEL      5   /* 1: terrain level when the curriculum wraps (:479-483) */
#define LG_SLOT_DOF        6   /* A: reset joint position factors (:415-430) */
#define LG_SLOT_XY(A)     (6 + (A))        /* 2: reset xy offset on terrain (:443-446) */
#define LG_SLOT_VEL(A)    (8 + (A))        /* 6: reset base twist (:451) */
#define LG_SLOT_RCMD(A)   (14 + (A))       /* 3: command resample of reset envs */
#define LG_SLOT_NOISE(A)  (17 + (A))       /* num_obs: observation noise (:224-226) */

/* Collapsed articulated model: what gym.load_asset + get_asset_* give the reference
 * (legged_robot.py:693-724).  Produced by legged_gym_dev_amd/model/robot_model.py.
 * Dynamics links: index 0 = floating base, 1+d = link moved by DOF d.  Topology: L serial
 * chains of J revolute joints, DOF index = leg * J + joint. */
typedef struct lg_model {
    int32_t num_bodies, num_dofs, num_legs, joints_per_leg, num_spheres, _pad0[3];
    float mass[LG_MAX_DOF + 1];
    float com[LG_MAX_DOF + 1][3];         /* link frame */
    float inertia[LG_MAX_DOF + 1][9];     /* about com, link axes, row major */
    float R_pj[LG_MAX_DOF][9];            /* joint frame axes in the parent link frame (columns) */
    float p_pj[LG_MAX_DOF][3];
    float axis[LG_MAX_DOF][3];            /* unit, joint frame */
    float q_lower[LG_MAX_DOF], q_upper[LG_MAX_DOF];   /* equal -> no position limit */
    float effort[LG_MAX_DOF], vel_limit[LG_MAX_DOF], joint_damping[LG_MAX_DOF];
    int32_t body_dyn[LG_MAX_BODIES];      /* body -> dynamics link (-1 base, else DOF) */
    int32_t sph_link[LG_MAX_SPHERES];     /* -1 base, else DOF */
    int32_t sph_body[LG_MAX_SPHERES];     /* row of the net-contact-force tensor it reports to */
    float sph_center[LG_MAX_SPHERES][3];  /* dynamics-link frame */
    float sph_radius[LG_MAX_SPHERES];
} lg_model;

/* ---- Extra reward terms.  The reference binds ANY method named _reward_<name> of the env class to a non-zero
 * rewards.scales.<name> (legged_robot.py:605-629; cassie.py:43-46 and legged_robot_trajectory.py:1060-1110 add terms that way).
 * Python code cannot run inside the step kernel, so a subclass declares such a term as data: one of a few generic kinds over
 * named per-env signals.  The term takes part in the reward sum at its alphabetical position (lg_cfg.term_order) and gets its
 * own episode_sums / extras_episode row (LG_NUM_REWARDS + index). */
#define LG_MAX_XTERMS 4
#define LG_NUM_TERMS (LG_NUM_REWARDS + LG_MAX_XTERMS)
enum lg_xterm_kind {
    LG_XT_NONE = 0,
    LG_XT_EXP_NEG_WSQ_ERR,     /* exp(-sum_k w[k] (a[k] - b[k])^2 / p[0])          e.g. tracking_lin_vel, tracking_rom           */
    LG_XT_WSQ,                 /* sum_k w[k] a[k]^2                                 e.g. orientation, ang_vel_xy                  */
    LG_XT_SLOPED_ERR_CHANGE    /* d = |(a-b)^2|_2 - |c|_2 ; (d < 0 ? p[0] : p[1]) d e.g. differential_error (c = error at reset)  */
};
enum lg_signal {               /* per-env vectors a term may read (length): */
    LG_SIG_ZERO = 0, LG_SIG_BASE_LIN_VEL /*3*/, LG_SIG_BASE_ANG_VEL /*3*/, LG_SIG_PROJ_GRAVITY /*3*/, LG_SIG_COMMANDS /*4*/,
    LG_SIG_ROOT_POS /*3*/, LG_SIG_TRAJ0 /*2: first point of the reference trajectory*/, LG_SIG_PREV_ERROR /*2*/,
    LG_SIG_DOF_POS_REL /*A: q - default*/, LG_SIG_DOF_VEL /*A*/, LG_SIG_TORQUES /*A*/, LG_SIG_ACTIONS /*A*/, LG_SIG_LAST_ACTIONS /*A*/,
    LG_NUM_SIGNALS
};
typedef struct lg_xterm {
    int32_t kind, n;                      /* kind; vector length used (<= 8) */
    int32_t sig_a, off_a, sig_b, off_b, sig_c, off_c;   /* signals and first component */
    float scale;                          /* rewards.scales.<name> * dt */
    float p[3];
    float w[8];
} lg_xterm;

/* ---- Trajectory-tracking env variant (legged_robot_trajectory.py): the velocity commands are replaced by
 * a reference trajectory from a reduced-order model (trajopt/rom_dynamics.py: SingleInt2D, state = xy position, input = xy
 * velocity) driven by the random input generator TrajectoryGenerator (:441-616).  Per env the generator keeps four input
 * laws -- sample-and-hold, ramp, extreme (v_min | 0 | v_max), sinusoid -- mixed with random weights, all redrawn when the
 * env's hold time t_final runs out; the ROM integrates the mixed input every rom_dt, the env observes the N last points
 * interpolated at its own time.  Pushes come from per-env timers (:150-160). */
#define LG_TRAJ_MAX_PTS 17                /* N * dN + 1 points kept per env */
#define LG_TG_NDRAW 20                    /* uniforms of one generator resample: const 2, ramp 2, extreme 2, sin mag/mean/freq/off
                                             4 x 2, hold time 1, weights 4, stationary 1 */
/* layout of one row of lg_buffers.tg_state (LG_TG_STRIDE floats per env): */
#define LG_TG_W 0          /* 4 mixing weights */
#define LG_TG_T_FINAL 4
#define LG_TG_T 5
#define LG_TG_K 6
#define LG_TG_CONST 7      /* 2 */
#define LG_TG_EXTREME 9    /* 2 */
#define LG_TG_RAMP_T0 11
#define LG_TG_RAMP_V0 12   /* 2 */
#define LG_TG_RAMP_V1 14   /* 2 */
#define LG_TG_SIN_MAG 16   /* 2 */
#define LG_TG_SIN_FREQ 18  /* 2 */
#define LG_TG_SIN_OFF 20   /* 2 */
#define LG_TG_SIN_MEAN 22  /* 2 */
#define LG_TG_STATIONARY 24 /* 0 | 1 */
#define LG_TG_V 25         /* 2: the mixed input of the last evaluation (TrajectoryGenerator.v, what dataset rollouts log) */
#define LG_TG_CENTER 28    /* 2: CircleTrajectoryGenerator.center (rom_dynamics.py:677-681); untouched by the other generators */
#define LG_TG_STRIDE 30
/* generator classes (trajectory_generator.cls; rom_dynamics.py:441-699) and weight samplers (weight_samp_cls; deep_tube_learning/
 * utils.py:27-79), chosen per context by lg_set_traj_generator.  RANDOM is TrajectoryGenerator, the training generator; ZERO,
 * SQUARE and CIRCLE are the fixed evaluation paths (no draws: their resample never samples).  The weight sampler only matters for
 * RANDOM: NO_RAMP zeroes the ramp weight before normalising.
 * PLAN (trajectory_generator.cls = 'PlanTrajectoryGenerator') is THIS PROJECT'S OWN class, not one of rom_dynamics.py: every env
 * follows a plan of its own -- n_nodes ROM inputs handed in by lg_traj_set_plans, piecewise constant per ROM step and indexed by the
 * env's ROM step counter LG_TG_K: the ROM step that takes k to k + 1 advances the window with v_plan[env][k] for 0 <= k < n_nodes and
 * with 0 otherwise (the reset's pre-roll at k < 0, past the plan's end, before any plan was set).  It draws nothing, is never
 * stationary, uses the inputs as given (bounds are the host's business) and leaves LG_TG_V = the input last applied to the window
 * (the ROM interval in force).  A reset env replays its plan from node 0 at its new root position.  lg_traj_replan moves a per-env
 * base b (0 otherwise), and the node read is k - b: replanning on the robot.  It is what lets the env track
 * the plans of tube/plan.py the way deep_tube_learning/evaluation/evaluate_tube_simple_oneshot_on_mpc_traj.py:75-132 lets its ROM
 * stand-in track them (legged_gym_dev_amd/tube/plan_env.py). */
#define LG_TG_KIND_RANDOM 0
#define LG_TG_KIND_ZERO 1
#define LG_TG_KIND_SQUARE 2
#define LG_TG_KIND_CIRCLE 3
#define LG_TG_KIND_PLAN 4
#define LG_TG_WSAMP_UNIFORM 0
#define LG_TG_WSAMP_NO_RAMP 1
typedef struct lg_traj_cfg {
    int32_t enabled, N, dN, randomize_rom_distance;
    float rom_dt, t_low, t_high, freq_low, freq_high, prob_stationary, zero_rom_dist_llh, max_push_vel_xy;
    float v_min[2], v_max[2], obs_scale[2], max_rom_dist[2];
    float push_t_lo, push_t_hi;           /* domain_rand.time_between_pushes */
} lg_traj_cfg;
/* uniform slots of the trajectory env (replace LG_SLOT_* when lg_cfg.traj.enabled): */
#define LG_TSLOT_TG        0                        /* LG_TG_NDRAW: generator resample in the step callback */
#define LG_TSLOT_PUSH      LG_TG_NDRAW              /* 2: push velocity xy */
#define LG_TSLOT_TIMER     (LG_TG_NDRAW + 2)        /* 1: next push time */
#define LG_TSLOT_LEVEL     (LG_TG_NDRAW + 3)
#define LG_TSLOT_DOF       (LG_TG_NDRAW + 4)        /* A */
#define LG_TSLOT_XY(A)     (LG_TG_NDRAW + 4 + (A))  /* 2 */
#define LG_TSLOT_VEL(A)    (LG_TG_NDRAW + 6 + (A))  /* 6 */
#define LG_TSLOT_ROMD(A)   (LG_TG_NDRAW + 12 + (A)) /* 3: start-offset mask draw + xy offset (:224-229) */
#define LG_TSLOT_RTG(A)    (LG_TG_NDRAW + 15 + (A)) /* LG_TG_NDRAW: generator resample of a reset env -- or of a NON-reset env
                                                       whose hold time ran out on a step where some env resets: the reference's
                                                       reset loop re-checks every env (rom_dynamics.py:571-574,598-608) */
#define LG_TSLOT_NOISE(A)  (2 * LG_TG_NDRAW + 15 + (A))

/* Flattened LeggedRobotCfg (+ what _parse_cfg/_init_buffers derive from it,
 * legged_robot.py:533-603,819-837). */
typedef struct lg_cfg {
    int32_t num_envs, num_obs, num_actions, num_bodies;
    int32_t num_feet, num_pen, num_term, num_height_points;
    int32_t feet_idx[LG_MAX_FEET], pen_idx[LG_MAX_PEN], term_idx[LG_MAX_TERM];
    int32_t decimation, control_type /*0 P,1 V,2 T*/, use_actuator_net, heading_command;
    int32_t max_episode_length, resample_steps, push_interval, push_robots;
    int32_t add_noise, measure_heights, only_positive_rewards, send_timeouts;
    int32_t terrain_type /*0 plane, 1 height samples*/, curriculum, custom_origins, max_terrain_level;
    int32_t hf_rows, hf_cols, terrain_num_cols, phys_substeps;
    int32_t env_offset, total_envs;       /* this shard's first global env id / envs over all ranks */
    int32_t solver_iterations;
    int32_t material_rand;                /* lg_buffers.material holds per-env restitution / compliance / thickness draws (else unread) */
    uint64_t seed;
    float sim_dt, dt, action_scale, clip_actions, clip_obs, max_push_vel, episode_length_s;
    float ground_restitution;             /* terrain.restitution; combined with the env's by averaging, like friction */
    float cmd_lo[4], cmd_hi[4];           /* lin_vel_x, lin_vel_y, ang_vel_yaw, heading */
    float obs_scale_lin_vel, obs_scale_ang_vel, obs_scale_dof_pos, obs_scale_dof_vel, obs_scale_height;
    float tracking_sigma, soft_dof_vel_limit, soft_torque_limit, base_height_target, max_contact_force;
    float hf_hscale, hf_vscale, border_size, terrain_env_length;
    float rew_scale[LG_NUM_REWARDS];      /* already multiplied by dt; 0 = term inactive */
    float base_init_state[13];
    float default_dof_pos[LG_MAX_DOF], p_gains[LG_MAX_DOF], d_gains[LG_MAX_DOF];
    float dof_pos_limits[LG_MAX_DOF][2];  /* soft limits (legged_robot.py:313-327) */
    float dof_vel_limits[LG_MAX_DOF], torque_limits[LG_MAX_DOF];
    float gravity[3], ground_friction;    /* ground mu; combined with the env's mu by averaging */
    float contact_offset, max_depenetration_velocity, contact_erp;
    float bounce_threshold;               /* sim.physx.bounce_threshold_velocity: approach speeds below it do not bounce */
    /* asset options the simulator is given (legged_robot.py:692-705): */
    float max_linear_velocity, max_angular_velocity;   /* :701-702: the base's velocities are clamped at these magnitudes after every
                                                          solve, as PhysX clamps a body's (0 = no clamp); each clamp is counted */
    float armature;                       /* :703: added to the inertia every joint sees about its own axis */
    float rest_offset;                    /* :704 thickness: the robot's shapes come to rest this far off a surface; replaced per env by
                                             lg_buffers.material[.][2] when that property is randomised (material_rand) */
    int32_t num_xterms, feet_air_time_ungated /* trajectory env: no command gate (legged_robot_trajectory.py:1071-1080) */;
    int32_t num_terms, _pad4;
    int32_t term_order[LG_NUM_TERMS];   /* active terms (builtin id, or LG_NUM_REWARDS + xterm index) in the order the
                                                             reference sums them (alphabetical); termination is not listed (applied last) */
    lg_xterm xterms[LG_MAX_XTERMS];
    lg_traj_cfg traj;
    float lstm_w[LG_LSTM_NW];             /* in_scale2 out_scale1 | w_ih0 64 w_hh0 256 b_ih0 32 b_hh0 32 |
                                             w_ih1 256 w_hh1 256 b_ih1 32 b_hh1 32 | lin_w 8 lin_b 1 */
    const float *noise_vec;               /* host, num_obs   (legged_robot.py:507-530) */
    const float *height_points;           /* host, num_height_points x 2, x-major grid (:861-875) */
    const float *terrain_origins;         /* host, rows(levels) x terrain_num_cols x 3, or NULL */
} lg_cfg;

/* State tensors.  Layouts are the reference's: root (N,13) =
 * [pos3, quat xyzw, lin vel3, ang vel3] world frame; dof_state (N,A,2) = [q, qdot] interleaved;
 * contact (N,B,3) world N; episode_sums is (LG_NUM_REWARDS + LG_MAX_XTERMS, N) so each term is a contiguous (N,). */
typedef struct lg_buffers {
    float *root_states, *dof_state, *contact_forces, *torques, *actions;
    float *obs, *rew;
    uint8_t *reset, *time_out;
    int64_t *episode_length;
    float *commands, *last_actions, *last_dof_vel, *last_root_vel, *feet_air_time;
    uint8_t *last_contacts;
    float *episode_sums, *base_lin_vel, *base_ang_vel, *projected_gravity, *measured_heights;
    float *env_origins;
    int64_t *terrain_levels, *terrain_types;
    float *lstm_h, *lstm_c;               /* (2, N*A, 8) each, anymal.py:62-69 */
    float *friction, *base_mass_delta;    /* per-env randomised constants (legged_robot.py:259-341) */
    /* extras: filled by the step's finalize pass; episode means only change on steps where at
     * least one env resets, time_outs likewise (the reference's stale-mask quirk, :156-157,186-187) */
    float *extras_episode;                /* LG_NUM_REWARDS + LG_MAX_XTERMS */
    float *extras_terrain_level;          /* 1 */
    uint8_t *extras_time_outs;            /* N */
    float *extras_episode_acc;            /* LG_NUM_REWARDS + LG_MAX_XTERMS + 2: running sums over steps of extras_episode, of extras_terrain_level
                                             and the number of steps summed -- rsl_rl's log() averages infos["episode"] over every
                                             step of an iteration; the reader divides and clears */
    int32_t *n_reset;                     /* 1: envs reset by the last step */
    int32_t *n_fault;                     /* 1: envs whose solve came back non-finite during the last step: brought to rest and reset (they are among n_reset) */
    int64_t *fault_total;                 /* 1: the same, summed since lg_create */
    int32_t *n_vel_clamp;                 /* 1: physics substeps of the last step in which an env's base velocity was clamped at
                                             max_linear_velocity / max_angular_velocity (the env carries on, as under PhysX) */
    int64_t *vel_clamp_total;             /* 1: the same, summed since lg_create */
    /* trajectory env (all unused otherwise): */
    float *tg_state;                      /* (N, LG_TG_STRIDE) generator state, LG_TG_* */
    float *tg_traj;                       /* (N, traj.N * traj.dN + 1, 2) ROM states, oldest first */
    float *trajectory;                    /* (N, traj.N, 2) what the env observes: interpolated at the env's time (:410-411) */
    float *prev_error;                    /* (N, 2) squared tracking error at the last reset (:199) */
    float *push_timer;                    /* (N) time_until_next_push (:150-160) */
    float *inject_uniforms;               /* (N, K) or unused */
    int64_t *inject_levels;               /* N */
    float *material;                      /* (N, 4) per-env randomised shape / body properties beside friction and base mass:
                                             [restitution, compliance, thickness, inverse base mass] (legged_robot.py:284-299,337-339);
                                             zeros = the asset's defaults */
} lg_buffers;

/* ---- Staged curriculum (legged_robot.py:360-363,488-505 base env: command ranges, push magnitude / period;
 * legged_robot_trajectory.py:414-417,519-553 trajectory env: reward scales, tracking sigma, ROM input bounds, hold-time sampler,
 * start-offset range).  The stage machine itself (curriculum_state, `common_step_counter % curriculum_steps[state] == 0`) is host
 * logic, as in the reference; a stage change rewrites these device constants.  In the reference the change happens at the END of
 * _post_physics_step_callback of the step that triggers it: the callback's own command resample / push / generator resample still
 * see the old values, everything after it (rewards, resets, observations of the same step) the new ones.
 * lg_set_curriculum_stage(.., in_callback = 1) reproduces exactly that for the next lg_step / lg_post_physics_step;
 * in_callback = 0 applies at once (the update at construction, legged_robot.py:828-829 / legged_robot_trajectory.py:78-79). */
typedef struct lg_stage {
    float cmd_lo[4], cmd_hi[4];           /* lin_vel_x, lin_vel_y, ang_vel_yaw, heading */
    float max_push_vel, _pad;
    double push_time;                     /* policy steps between pushes; may be fractional (nominal x multiplier): a push fires when
                                             step_counter % push_time == 0 in Python float arithmetic */
    float rew_scale[LG_NUM_REWARDS];      /* x dt, as lg_cfg.rew_scale */
    float xterm_scale[LG_MAX_XTERMS];     /* x dt, as lg_xterm.scale */
    float xterm_p0[LG_MAX_XTERMS];        /* lg_xterm.p[0] (tracking_rom: its sigma) */
    float traj_v_min[2], traj_v_max[2], traj_t_low, traj_t_high, traj_max_rom_dist[2];
} lg_stage;

typedef struct lg_ctx lg_ctx;

const char *lg_last_error(void);
int lg_version(void);

/* Replaces create_sim/_create_envs/prepare_sim/acquire_*_tensor (base_task.py:84-85,
 * legged_robot.py:228-245,537-539).  height_samples: host int16 (hf_rows x hf_cols) or NULL. */
int lg_create(const lg_cfg *cfg, const lg_model *model, const int16_t *height_samples, lg_ctx **out);
int lg_destroy(lg_ctx *ctx);
int lg_get_buffers(lg_ctx *ctx, lg_buffers *out);
/* stream = hipStream_t; all later calls enqueue on it (the caller's torch stream). */
int lg_set_stream(lg_ctx *ctx, void *stream);
/* counterpart of env.common_step_counter (legged_robot.py:115); set by tests/resume. */
int lg_set_step_counter(lg_ctx *ctx, int64_t counter);
int64_t lg_get_step_counter(lg_ctx *ctx);
int lg_set_init_done(lg_ctx *ctx, int init_done);     /* legged_robot.py:472-474 */
/* enable (1) / disable (0) replay of buffers.inject_uniforms / inject_levels. */
int lg_inject_uniforms(lg_ctx *ctx, int enable);

/* LeggedRobot.step (legged_robot.py:80-104): clip actions, decimation x {torque law, physics
 * substep}, post_physics_step, clip observations.  actions: device (N, A) f32.
 * The clip + decimation loop is one kernel launch (state resident on chip).  lg_compute_torques and lg_simulate run
 * the same kernel with one stage switched off, so the result equals the sequence lg_set_actions, decimation x
 * {lg_compute_torques, lg_simulate}, lg_post_physics_step bit for bit. */
int lg_step(lg_ctx *ctx, const float *actions);
/* Finer-grained entry points (tests, teacher forcing): */
int lg_set_actions(lg_ctx *ctx, const float *actions);         /* :86-87 */
int lg_compute_torques(lg_ctx *ctx);                           /* :91 (PD :389-413 / LSTM anymal.py:71-81) */
int lg_simulate(lg_ctx *ctx);                                  /* :92-96, one sim_dt of physics */
int lg_post_physics_step(lg_ctx *ctx);                         /* :106-137 + obs clip :100-103 */
int lg_reset_all(lg_ctx *ctx);                                 /* reset_idx(arange(N)), base_task.py:113 */
/* reset_idx(env_ids) for an arbitrary subset (legged_robot.py:147-187): terrain curriculum, _reset_dofs + _reset_root_states
 * (what the reference pushes through set_dof_state_tensor_indexed :428 / set_actor_root_state_tensor_indexed :452, with the
 * same int32 id tensor), command resample, buffer clears, actuator-net state (anymal.py:56-60), extras["episode"] means
 * over the ids and extras["time_outs"].  ids: DEVICE int32[n], local env indices, no duplicates.  n == 0 returns at once
 * (legged_robot.py:156-157).  Draws come from the env's reset slots at the current step counter. */
int lg_reset_ids(lg_ctx *ctx, const int32_t *ids, int n);
/* Trajectory env: the generator class and weight sampler (LG_TG_KIND_*, LG_TG_WSAMP_*) of this context; call before the first
 * reset.  At creation: LG_TG_KIND_RANDOM / LG_TG_WSAMP_UNIFORM.  Refused for the velocity-command env. */
int lg_set_traj_generator(lg_ctx *ctx, int kind, int weight_sampler);
/* Trajectory env: TrajectoryGenerator.reset(z) (rom_dynamics.py:592-593) for every env -- the window restarts at z, the clocks at
 * -N rom_dt, and N ROM steps fill the window -- without touching the rest of the env (the observed trajectory follows at the next
 * step callback).  z: DEVICE f32 (N, 2).  RANDOM draws its resample from the reset slots at the current step counter. */
int lg_traj_reset(lg_ctx *ctx, const float *z);
/* Trajectory env of kind LG_TG_KIND_PLAN: the plans of every env, v DEVICE f32 (num_envs, n_nodes, 2), 0 <= n_nodes <= LG_PLAN_MAX_N
 * (v may be NULL when n_nodes is 0).  A stream-ordered copy into the context's own (num_envs, LG_PLAN_MAX_N, 2) buffer: the
 * caller's array need not outlive the call.  The ROM step counters are not touched: lg_traj_reset / a reset restart the plans.
 * Refused (lg_last_error) for a non-trajectory env, a kind other than PLAN, n_nodes out of range, a null v with n_nodes > 0. */
int lg_traj_set_plans(lg_ctx *ctx, const float *v, int32_t n_nodes);
/* Trajectory env of kind LG_TG_KIND_PLAN: replanning on the robot, the "plan from z_k[k+1]" of the re-solve at every control step of
 * trajopt/tube_planning_closed_loop.py:82-168 ("TPCL" :159-163), by rewriting the window instead of appending behind its head.
 * v: DEVICE f32 (num_envs, n_nodes, 2), 1 <= n_nodes <= LG_PLAN_MAX_N, new plans that START AT WINDOW POINT 1, the node the robot
 * is heading for (it tracks between window points 0 and 1).  skip: DEVICE u8 (num_envs) or NULL; env i with skip[i] != 0 keeps its
 * window, plan and base untouched (pass the recorder's `dead`; the node count is the context's, so a skipped env's old plan is read
 * with the new count).  One launch on the env's stream; the caller's arrays need not outlive the call.
 * The law, as an "as if": with k = LG_TG_K at the call, the generator state of env i, and all that evolves from it, is afterwards
 * that of an env whose inputs had always been the old ones for the ROM steps that produced window points 0 and 1, then v[i][0],
 * v[i][1], ... from window point 1 on, and 0 past the plan.  With Nw = lg_traj_cfg.N window intervals (points w[0..Nw]):
 *   w[0], w[1] are kept;  w[p] = w[p-1] + rom_dt v[i][p-2] for p = 2..Nw (input 0 where p - 2 >= n_nodes), one rounding per
 *   operation, so the points are the nodes a plan scored from w[1] has, on the bits;
 *   the plan is copied into the context's buffer and the env's plan base becomes k - (Nw - 1): the ROM step k' -> k' + 1 then takes
 *   node j = k' - base, so the next head advance takes v[i][Nw - 1]; inputs are 0 for j < 0 and j >= n_nodes;
 *   LG_TG_V = v[i][Nw - 2] (0 past the plan), the input last applied to the window; unchanged at Nw = 1;
 *   lg_buffers.trajectory is re-interpolated from the new window at the env's stored LG_TG_T / LG_TG_K.
 * LG_TG_K, LG_TG_T and the stationary flag are not touched.  The observation buffer's trajectory columns follow at the next step
 * callback, as after lg_traj_reset.  lg_traj_set_plans, lg_traj_reset and every env reset put the base back to 0: a reset env
 * replays the plan in its buffer from node 0.
 * Refused (lg_last_error) for a non-trajectory env, a kind other than PLAN, n_nodes outside 1..LG_PLAN_MAX_N, a null v. */
int lg_traj_replan(lg_ctx *ctx, const float *v, int32_t n_nodes, const uint8_t *skip);
/* ROM-rate recorder of the trajectory env (any generator kind), per env and on the device: one small launch per env step, one
 * lane per env, no host read.  The caller owns the (device) buffers.  lg_traj_rec_begin writes row 0 -- z = trajectory[:, 0] (the
 * point the robot tracks), pz_x = root xy, x = the state vector in get_state()'s layout (base pose 7, joint positions, base twist
 * 6, joint velocities) -- and sets rows = 1, dead = 0, k_mark = LG_TG_K.  lg_traj_rec_step, called after an env step, does for
 * each env: (1) nothing if it is dead; (2) if its reset flag (lg_buffers.reset, the step's dones) is set: dead = 1, rows kept;
 * (3) otherwise, if LG_TG_K != k_mark and rows < rows_max: row `rows` of z, pz_x (and x), v[rows - 1] = LG_TG_V, rows += 1,
 * k_mark = LG_TG_K.  So row r of an env is what it was right after its own r-th ROM step since begin. */
typedef struct lg_traj_rec {
    int32_t rows_max, x_n;                /* rows per env (>= 2); floats per row of x: 13 + 2 num_actions, or 0 without x */
    float *z, *pz_x;                      /* (N, rows_max, 2) */
    float *v;                             /* (N, rows_max - 1, 2) */
    int32_t *rows;                        /* (N) rows written */
    uint8_t *dead;                        /* (N) the env reset (termination or time-out) while recording */
    float *k_mark;                        /* (N) LG_TG_K at the last row */
    float *x;                             /* (N, rows_max, x_n) or NULL */
} lg_traj_rec;
/* host: refuses, the field named in lg_last_error, rows_max < 2, a null required buffer, an x_n that is not env_x_n */
int lg_traj_rec_check(const lg_traj_rec *rec, int64_t N, int32_t env_x_n);
int lg_traj_rec_begin(lg_ctx *ctx, const lg_traj_rec *rec);
int lg_traj_rec_step(lg_ctx *ctx, const lg_traj_rec *rec);
/* Runs the step's single-workgroup epilogue (extras["episode"], extras["time_outs"], counters) if a learner attached with
 * lg_ppo_attach_env left it pending; a no-op otherwise.  Every env entry point does this itself before it touches the env. */
int lg_finalize(lg_ctx *ctx);
int lg_get_stage(lg_ctx *ctx, lg_stage *out);          /* the values in force (at creation: what lg_cfg holds) */
int lg_set_curriculum_stage(lg_ctx *ctx, const lg_stage *stage, int in_callback);

/* ------------------------------------------------------------------ PPO (rsl_rl v1.0.2 semantics,
 * SURVEY.md Appendix B; call sites task_registry.py:148-155, scripts/train.py:44) */
typedef struct lg_ppo_cfg {
    int32_t num_envs, num_obs, num_critic_obs, num_actions;
    int32_t num_hidden, actor_hidden[LG_MAX_HIDDEN], critic_hidden[LG_MAX_HIDDEN];
    int32_t activation /*0 elu, 1 selu, 2 relu, 3 lrelu, 4 tanh, 5 sigmoid (rsl_rl get_activation; its "crelu" is nn.ReLU: 2)*/, num_steps, num_epochs, num_mini_batches;
    int32_t adaptive_schedule, use_clipped_value_loss, world_size, _pad;
    uint64_t seed;
    float init_noise_std, value_loss_coef, clip_param, entropy_coef, learning_rate;
    float gamma, lam, desired_kl, max_grad_norm, _padf;
} lg_ppo_cfg;

typedef struct lg_ppo_buffers {
    float *params, *grads, *adam_m, *adam_v;      /* flat, num_params (+ tail, see num_reduce) */
    float *obs, *critic_obs, *actions, *rewards, *values, *returns, *advantages, *log_prob, *mu, *sigma;
    uint8_t *dones;                                /* storage, time major (T, N, .) */
    float *act_actions, *act_values, *act_log_prob, *act_mu;   /* outputs of the last act() */
    float *stats;                                  /* [lr, kl, value_loss_sum, surrogate_loss_sum, adam_t, n_updates, adv_mean, adv_std] */
    float *noise;                                  /* (N, A) injected N(0,1) for act(), or unused */
    int32_t *perm;                                 /* minibatch permutation (T*N) */
    float *adv_partial;                            /* [sum, sumsq, count] for cross-rank normalisation */
    float *cur_reward_sum, *cur_episode_len;       /* (N) running episode return / length (runner logging) */
    float *ep_stats;                               /* [sum return, sum length, count] of episodes finished since cleared */
    float *ep_ring;                                /* (2, 100): returns / lengths of the last 100 finished episodes (rsl_rl's rewbuffer and
                                                      lenbuffer deques); slot = finish order % 100, unordered within one step */
    int32_t *ep_ring_count;                        /* 1: episodes finished since creation */
    int64_t num_params, num_reduce;                /* floats to all-reduce per optimiser step */
} lg_ppo_buffers;

typedef struct lg_ppo lg_ppo;

/* rsl_rl's ActorCriticRecurrent: memory_a / memory_c = one nn.LSTM layer each (type 0 = LSTM; the only one), hidden a multiple of 32,
 * <= 512; the actor / critic MLPs of lg_ppo_cfg take the hidden state as input.  lg_ppo_begin_update and lg_ppo_minibatch_backward
 * refuse a learner whose num_envs is not a multiple of num_mini_batches (rollout and inference work for any num_envs). */
typedef struct lg_ppo_rnn_cfg {
    int32_t type, hidden, layers, _pad;
} lg_ppo_rnn_cfg;

typedef struct lg_ppo_rnn_buffers {
    float *h[2], *c[2];                            /* live state (N, H) of memory_a [0] and memory_c [1] */
    float *saved_h[2], *saved_c[2];                /* state before each rollout step (T, N, H): RolloutStorage.saved_hidden_states_{a,c} */
    int64_t hidden;
} lg_ppo_rnn_buffers;

int lg_ppo_create(const lg_ppo_cfg *cfg, lg_ppo **out);
/* A recurrent learner.  Parameters: std, actor.*, critic.*, then memory_a.rnn.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}
 * and the same four of memory_c (lg_ppo_param_layout).  lg_ppo_act stores the state before the step and advances both memories;
 * lg_ppo_process_env_step zeroes the state of the envs that are done; lg_ppo_compute_returns advances memory_c once more on the
 * last observations (rsl_rl's evaluate); lg_ppo_act_inference advances memory_a and needs rows == num_envs.  The update runs
 * rsl_rl's recurrent minibatch generator: minibatch i = envs [i N / nmb, (i + 1) N / nmb) over all T steps, same order every epoch,
 * each trajectory starting from its saved state.  lg_ppo_set_comm is refused (its per-layer buckets do not cover the LSTM). */
int lg_ppo_create_recurrent(const lg_ppo_cfg *cfg, const lg_ppo_rnn_cfg *rnn, lg_ppo **out);
int lg_ppo_get_rnn_buffers(lg_ppo *p, lg_ppo_rnn_buffers *out);     /* error on a feed-forward learner */
int lg_ppo_reset_hidden(lg_ppo *p, const uint8_t *dones);           /* zero the state of the envs with dones[i] set; NULL = all */
int lg_ppo_destroy(lg_ppo *p);
int lg_ppo_get_buffers(lg_ppo *p, lg_ppo_buffers *out);
int lg_ppo_set_stream(lg_ppo *p, void *stream);
int lg_ppo_param_layout(lg_ppo *p, int64_t *offsets, int64_t *shapes, int max_entries); /* returns #tensors */
int lg_ppo_inject_noise(lg_ppo *p, int enable);
/* PPO.act: actor+critic forward, sample, log-prob; stores the transition at the current step. */
int lg_ppo_act(lg_ppo *p, const float *obs, const float *critic_obs);
/* PPO.process_env_step: reward += gamma * V * time_outs; store reward/done; advance step. */
int lg_ppo_process_env_step(lg_ppo *p, const float *rew, const uint8_t *dones, const uint8_t *time_outs);
/* PPO.compute_returns: bootstrap value, GAE reverse scan, local advantage sums. */
int lg_ppo_compute_returns(lg_ppo *p, const float *last_critic_obs);
int lg_ppo_normalize_advantages(lg_ppo *p);        /* after adv_partial was (all-)reduced */
/* PPO.update split so the caller can all-reduce grads between the two halves: */
int lg_ppo_begin_update(lg_ppo *p);                /* new permutation, zero loss stats; re-derives the bf16 weight planes
                                                      from params (so params may be written through lg_ppo_buffers
                                                      between updates: checkpoint load, broadcast) */
int lg_ppo_minibatch_backward(lg_ppo *p, int epoch, int mb);   /* fwd, loss, bwd -> grads (+KL tail) */
int lg_ppo_minibatch_step(lg_ppo *p);              /* KL-adaptive lr, clip_grad_norm, Adam; clears grads */
int lg_ppo_end_update(lg_ppo *p);                  /* finalise mean losses, clear storage */
/* Rollout fusion (optional; OnPolicyRunner.rollout switches it on for the duration of a rollout).  With an env attached, lg_step
 * leaves its single-workgroup epilogue pending and lg_ppo_process_env_step only records its arguments; both run inside the launch
 * of the NEXT lg_ppo_act (extra workgroups beside the two MLPs: 5 launches per policy step become 3).  Any other entry point of
 * either object, and lg_ppo_attach_env(p, NULL), first runs what is pending the ordinary way, so results are identical.
 * While attached, extras / n_reset / the logging sums of a step become visible with the next lg_ppo_act (or flush).
 * Contract: env and learner run on the SAME stream (checked: the fused epilogue reads the env's step outputs in stream order), and
 * the env outlives the attachment -- lg_destroy refuses an env that is still attached; detach with lg_ppo_attach_env(p, NULL) or
 * destroy the learner first. */
int lg_ppo_attach_env(lg_ppo *p, lg_ctx *env);
/* The caller wrote lg_ppo_buffers.params itself (checkpoint load, a broadcast of its own): the weight images the rollout forward
 * reads are re-derived by the next lg_ppo_act.  (lg_ppo_minibatch_step and lg_ppo_broadcast_params mark them stale themselves.) */
int lg_ppo_params_changed(lg_ppo *p);
/* Reproducible runs (debugging aid; off by default).  The learner's sums over the minibatch rows -- weight-gradient slices, bias
 * column sums, the head's row sums, loss statistics, the gradient norm, the advantage moments -- are float atomics, whose order
 * differs from run to run (last-bit differences in every gradient; the gradient norm itself, taken from the reduced gradients,
 * is added in a fixed order in either mode, so that ranks holding the same gradients clip alike).  on != 0: the same contributions are accumulated as 2^-40
 * fixed-point 64-bit integers (order-independent) and folded into the float buffers before they are read: two runs from the
 * same seed then agree bit for bit, on one rank and across a fixed set of ranks.  Costs three small launches per optimiser step.
 * Range: |sum| < 2^23 per accumulator; the squared gradient norm is kept in two such words (a norm below 1.9e8).
 * Not combinable with gradient buckets reduced inside the backward pass (lg_ppo_set_comm): returns an error then. */
int lg_ppo_set_deterministic(lg_ppo *p, int on);
/* Tests of the optimiser step: device pointers of the split-bf16 weight planes (uint16; plane h at *wpl, m and l *pl_stride and
 * 2 * *pl_stride elements later, 3 * pl_stride + 8 elements in all) and of the int32 [num_params] map from a parameter to its element
 * inside a plane (-1: biases, std, LSTM weights).  Read-only: nothing is launched or changed. */
int lg_ppo_debug_weight_planes(lg_ppo *p, void **wpl, int64_t *pl_stride, void **pl_dest);
/* actor mean only (act_inference) for play/eval */
int lg_ppo_act_inference(lg_ppo *p, const float *obs, float *actions_out, int64_t rows);

/* ------------------------------------------------------------------ collectives (nothing in the reference to
 * replace -- it has no multi-GPU code; this is the exchange step the env-sharded learner needs).  One process per GPU; rank r
 * owns envs [r N/G, (r+1) N/G).  RCCL over xGMI, resolved from the librccl.so already in the process (no link dependency).
 * The Python runner may use torch.distributed instead (same RCCL underneath); these entries are for hosts without it, and for
 * the reduction overlapped with the backward pass, which needs the learner's own streams.
 * LG_RCCL_LIB (environment, read at the first lg_comm_* call of the process): the path of the library to resolve RCCL's entry
 * points from instead -- a deployment hook for an RCCL at a non-default path.  It is opened as given (RTLD_NOW | RTLD_LOCAL) and
 * there is no fallback: if it cannot be loaded the call fails with an error that names the path.  The tests use it to put a
 * stand-in transport (tests/comm_standin) under these entries. */
#define LG_COMM_ID_BYTES 128
typedef struct lg_comm lg_comm;
int lg_comm_get_unique_id(void *id_out /* LG_COMM_ID_BYTES, host */);   /* rank 0; the host carries the bytes to the other ranks */
int lg_comm_init(int rank, int nranks, const void *id, lg_comm **out);  /* collective over all ranks; device = hipGetDevice() */
int lg_comm_destroy(lg_comm *c);
int lg_comm_rank(lg_comm *c);
int lg_comm_size(lg_comm *c);
int lg_comm_allreduce_sum(lg_comm *c, float *buf /* device, in place */, int64_t n, void *stream);
int lg_comm_broadcast(lg_comm *c, float *buf, int64_t n, int root, void *stream);
/* The learner's three exchanges.  lg_ppo_set_comm(p, c) makes lg_ppo_minibatch_backward reduce the gradients itself, layer by
 * layer as their weight-gradient GEMMs finish (the head's bucket carries std and the KL sum), on the communicator's stream
 * beside the remaining backward GEMMs; lg_ppo_minibatch_step then waits for the last bucket.  c = NULL switches it off. */
int lg_ppo_set_comm(lg_ppo *p, lg_comm *c);
int lg_ppo_allreduce_adv_moments(lg_ppo *p, lg_comm *c);   /* between lg_ppo_compute_returns and lg_ppo_normalize_advantages */
int lg_ppo_broadcast_params(lg_ppo *p, lg_comm *c, int root);   /* identical initial policy on every rank */
/* How long the learner's stream stood waiting for the gradient buckets (what the overlap did NOT hide), measured with HIP events
 * around the wait of every minibatch while timing is enabled (at most 4096 minibatches are recorded, then recording stops).
 * lg_ppo_comm_wait_ms synchronises the learner's stream, returns the sum in ms and the number of minibatches summed, and clears. */
int lg_ppo_comm_timing(lg_ppo *p, int enable);
int lg_ppo_comm_wait_ms(lg_ppo *p, double *ms_total, int64_t *minibatches);

/* ------------------------------------------------------------------ tube-model trainer (deep_tube_learning/train_tube.py: the
 * reference MLP, ScalarTube / VectorTube / ScalarHorizonTube / Error losses, Adam + StepLR).
 * One training step = one fused forward / loss / backward launch + one launch that reduces the per-workgroup gradients in a
 * fixed order and runs Adam: bit-reproducible from run to run.  Nothing in a step synchronises the host. */
#define LG_TUBE_MAX_IN 256
#define LG_TUBE_MAX_OUT 64
#define LG_TUBE_MAX_UNITS 128                      /* num_units: 16..128, multiple of 16; num_layers 1..4 */
#define LG_TUBE_ACT_RELU 0
#define LG_TUBE_ACT_SOFTPLUS 1                     /* torch.nn.Softplus(beta, threshold=20) */
#define LG_TUBE_ACT_TANH 2
#define LG_TUBE_ACT_ELU 3                          /* alpha 1 */
#define LG_TUBE_LOSS_SCALAR 0                      /* ScalarTubeLoss / ScalarHorizonTubeLoss: Huber mean over rows x outputs */
#define LG_TUBE_LOSS_VECTOR 1                      /* VectorTubeLoss: pinball residuals summed per row, Huber mean over rows */
#define LG_TUBE_LOSS_MSE 2                         /* ErrorLoss */
#define LG_TUBE_MAX_LEVELS 64                       /* levels of one lg_tube_predict_levels / lg_tube_predict_windows_levels call */
typedef struct lg_tube_cfg {
    int32_t input_dim, output_dim, num_units, num_layers;
    int32_t activation, loss, horizon /*0: flat (data, target) rows; 1: ScalarHorizonTubeDataset windows*/, batch_size;
    int32_t H_fwd, H_rev, step_size /*StepLR*/, _pad;
    uint64_t seed;                                 /* epoch permutations and horizon window draws */
    float alpha, delta, softplus_beta, _padf;
    double lr, gamma;                              /* Adam lr0; StepLR: lr = lr0 * gamma^floor(step / step_size) */
    /* Level-conditioned tube; 0 = off.  With level_input = 1 the LAST input column is the coverage level
     * of the row: input_dim counts it, the data of lg_tube_set_data has input_dim - 1 columns, every step / eval draws one level
     * per row, uniform over [level_lo, level_hi), and the row's pinball loss takes that level where it takes alpha otherwise
     * (alpha is not read).  Needs a tube loss (not mse), input_dim >= 2 and 0 <= level_lo < level_hi <= 1.
     * With horizon = 1 the window item gains the level as its last column: [w[t0-H_rev : t0], z[t0],
     * v[t0-H_rev : t0+H_fwd], level], input_dim = H_rev + nz + (H_rev + H_fwd) m + 1; one level per row, shared by the row's H_fwd
     * outputs in the loss; starts and levels both record the draw.  Chosen edge of the envelope: a conditioned horizon handle needs
     * H_rev >= 1 -- an item without a past error carries no error history; the conditioned flat kinds serve that case. */
    int32_t level_input, _pad2;
    float level_lo, level_hi;
} lg_tube_cfg;

typedef struct lg_tube_buffers {
    float *params, *grads, *adam_m, *adam_v;      /* flat, num_params, lg_tube_param_layout order; grads = the last step's */
    float *log;                                    /* (log_cap, 4) per step, slot (step - 1) % log_cap: loss, lr after the step
                                                      (StepLR's get_last_lr), gradient norm, rows */
    float *eval;                                   /* 4: test loss, fraction of outputs with fw > w, mean |w - fw| where fw > w, rows */
    int32_t *starts;                               /* horizon dataset: window start drawn per row of the last step / eval */
    int32_t *perm;                                 /* the epoch's permutation of the training rows */
    int64_t num_params, log_cap, starts_cap, perm_cap, step;
    float *levels;                                 /* level_input: the level of every row of the last step / eval (as starts) */
    int64_t levels_cap;
} lg_tube_buffers;

typedef struct lg_tube lg_tube;
int lg_tube_check_cfg(const lg_tube_cfg *cfg);    /* 0 inside the supported envelope, else -1 and lg_last_error says why */
int lg_tube_create(const lg_tube_cfg *cfg, lg_tube **out);
int lg_tube_destroy(lg_tube *t);
int lg_tube_set_stream(lg_tube *t, void *stream);
int lg_tube_get_buffers(lg_tube *t, lg_tube_buffers *out);
/* per Linear layer: weight (offset, [out, in]) then bias (offset, [out, 0]); returns #tensors = 2 * (num_layers + 1) */
int lg_tube_param_layout(lg_tube *t, int64_t *offsets, int64_t *shapes, int max_entries);
int lg_tube_params_changed(lg_tube *t);            /* after the caller wrote params (initialisation, checkpoint load) */
int lg_tube_set_step(lg_tube *t, int64_t step);    /* Adam / StepLR step count (resume) */
/* which: 0 train, 1 test.  Device pointers the caller keeps alive.  Flat: x = data (rows, input_dim), y = target
 * (rows, output_dim), v unused.  Horizon: x = w (rows, T), y = z (rows, T, nz), v = v (rows, T, m), padded in front by H_rev;
 * -1 unless input_dim == H_rev + nz + (H_rev + H_fwd) m (+ 1 on a level_input handle). */
int lg_tube_set_data(lg_tube *t, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T, int32_t nz,
                     int32_t m);
int lg_tube_begin_epoch(lg_tube *t, int64_t epoch);   /* a new permutation of the training rows, keyed by (seed, epoch) */
/* One Adam step on `count` rows (1..batch_size): rows (device, count) or NULL = the next count rows of the epoch's permutation.
 * The ids are not checked on the host.  An id outside [0, rows of the training split) reads nothing: the kernel takes it as a row of
 * zeros -- zero input, zero target; on a level_input handle its level column is still drawn -- that runs through the model and the
 * loss like any other and COUNTS in the loss's divisor and in log[3].  With zero biases such a row contributes exactly nothing; in
 * general it contributes the gradient of the loss at x = 0, w = 0.  Callers that mean to skip rows pass a shorter list. */
int lg_tube_step(lg_tube *t, const int32_t *rows, int64_t count);
int lg_tube_eval(lg_tube *t);                      /* metrics of the test split into lg_tube_buffers.eval (one window per row;
                                                      level_input: one drawn level per row) */
/* level_input handles: lg_tube_eval with every test row at `level` (0..1) instead of a drawn one; eval[1] is then the coverage
 * at that level.  -1 on an unconditioned handle. */
int lg_tube_eval_level(lg_tube *t, float level);

/* Inference.  The three entries read params / the transposed copy and change neither; all pointers are device pointers, everything
 * runs on the handle's stream and nothing waits for the device.  A row's result does not depend on the batch it is in.
 * Each returns -1 (reason in lg_last_error) for the wrong handle kind, fb out of range, non-positive counts, or nz / m that
 * disagree with input_dim. */
/* out[i] = MLP(x[rows ? rows[i] : i]);  x (n, input_dim), out (count, output_dim).  Flat (non-horizon) handles.  The caller
 * guarantees 0 <= rows[i] < n. */
int lg_tube_predict(lg_tube *t, const float *x, const int32_t *rows, int64_t count, float *out);
/* level_input handles: out[i, l] = MLP([x[rows ? rows[i] : i], levels[l]]), one launch; x (n, input_dim - 1), levels (device,
 * n_levels, 1 <= n_levels <= 64), out (count, n_levels, output_dim).  The part of the first layer that does not depend on the
 * level is computed once per row.  Each out[i, l] equals, bit for bit, lg_tube_predict on that row with levels[l] appended.
 * lg_tube_predict, lg_tube_rollout and lg_tube_rollout_window take rows of full input_dim on such a handle: the caller fills the
 * level column, a teacher column like any other.  -1 on an unconditioned handle. */
int lg_tube_predict_levels(lg_tube *t, const float *x, const int32_t *rows, int64_t count, const float *levels, int32_t n_levels,
                           float *out);
/* Horizon handles: item (env[i], start[i]) built as ScalarHorizonTubeDataset._get_item_helper does, out (count, H_fwd).
 * w (n, T), z (n, T, nz), v (n, T, m) padded in front by H_rev as for lg_tube_set_data.
 * Caller guarantees 0 <= env[i] < n, H_rev <= start[i] and start[i] + H_fwd <= T.  -1 on a level_input handle: a window holds no
 * level, lg_tube_predict_windows_levels takes them. */
int lg_tube_predict_windows(lg_tube *t, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz,
                            int32_t m, const int32_t *env, const int32_t *start, int64_t count, float *out);
/* level_input horizon handles: out[i, l] = MLP([item (env[i], start[i]), levels[l]]), one launch; the arrays and the caller's
 * guarantees are lg_tube_predict_windows', input_dim = H_rev + nz + (H_rev + H_fwd) m + 1, levels (device, n_levels,
 * 1 <= n_levels <= 64), out (count, n_levels, H_fwd).  The first layer's chain over the shared columns is computed once per window.
 * Each out[i, l] equals, bit for bit, lg_tube_predict of a flat level_input handle with the same parameters on the item with
 * levels[l] appended.  -1 on an unconditioned handle and on a flat handle. */
int lg_tube_predict_windows_levels(lg_tube *t, const float *w, const float *z, const float *v, int64_t n, int32_t T, int32_t nz,
                                   int32_t m, const int32_t *env, const int32_t *start, int64_t count, const float *levels,
                                   int32_t n_levels, float *out);
/* Closed loop over time, one launch.  x (n_seq, T, input_dim): the teacher rows in time order.  out (n_seq, T, output_dim).
 * out[s, t] = MLP(xt) where xt = x[s, t] with its leading fb columns replaced by out[s, t-1, 0:fb],
 * except at t == 0 and where reseed[s, t] != 0 (reseed (n_seq, T) may be NULL): there xt = x[s, t] unchanged.
 * 0 <= fb <= min(input_dim, output_dim).  Flat handles. */
int lg_tube_rollout(lg_tube *t, const float *x, int64_t n_seq, int32_t T, int32_t fb, const uint8_t *reseed, float *out);
/* The closed loop of a windowed model, one launch.  An input row is `taps` blocks of `stride` columns, block i the dataset row
 * delayed by i * dN steps; the leading fb columns of every block hold the fed-back quantity.  With s0(t) the last step t' <= t
 * that is 0 or has reseed[s, t'] != 0:  out[s, t] = MLP(xt), xt = x[s, t] except that for every tap i with t - i*dN > s0(t)
 * columns [i*stride, i*stride + fb) are out[s, t-1-i*dN, 0:fb].  Every other column is the teacher's, taps that reach back to
 * or before the seed included.  taps == 1 is lg_tube_rollout (stride is then not read).  The history stays on chip.
 * Returns -1 unless fb, taps, dN >= 1, fb <= output_dim, stride >= fb (taps > 1), (taps-1)*stride + fb <= input_dim and
 * ((taps-1)*dN + 1) * fb <= 1024 (the ring of past outputs a sequence keeps).  Flat handles. */
int lg_tube_rollout_window(lg_tube *t, const float *x, int64_t n_seq, int32_t T, int32_t fb, int32_t taps, int32_t dN,
                           int32_t stride, const uint8_t *reseed, float *out);

/* ------------------------------------------------------------------ sweep of tube models (DESIGN.md sections 10.3, 10.21): K
 * models of one shape train on one dataset in the same two launches per step, the members along the grid's y axis.  It is the
 * trainer behind lg_tube with K members instead of one, on one host path; member k is, bit for bit, the lg_tube built from
 * cfgs[k] and given the same calls.  With K > 1, create and set_data copy the member array to the device and wait for the
 * handle's stream; step, eval and begin_epoch wait for nothing.  Members share input_dim, output_dim, num_units, num_layers, loss,
 * horizon, H_fwd, H_rev, batch_size and level_input; they may differ in alpha, delta, activation, softplus_beta, lr, gamma, step_size,
 * seed, level_lo and level_hi.
 * Every member owns a full set of a single trainer's buffers (parameters, moments, gradient slab, log, eval, starts, perm), so a
 * sweep takes K times a single trainer's memory; the dataset is held once.  The members step together: one step count, one
 * position in the epoch (each member in its own permutation).  Every entry returns 0, or -1 / a negative code with the reason in
 * lg_last_error. */
#define LG_TUBE_SWEEP_MAX 64
typedef struct lg_tube_sweep lg_tube_sweep;
/* -1: K outside 1..LG_TUBE_SWEEP_MAX; a member outside lg_tube_check_cfg's envelope (the message names the member and the reason);
 * a shared field that differs (the message names the field and both members).  -100: a failed allocation. */
int lg_tube_sweep_create(const lg_tube_cfg *cfgs, int32_t K, lg_tube_sweep **out);
int lg_tube_sweep_destroy(lg_tube_sweep *s);
int lg_tube_sweep_set_stream(lg_tube_sweep *s, void *stream);
int lg_tube_sweep_get_buffers(lg_tube_sweep *s, int32_t k, lg_tube_buffers *out);   /* member k's buffers */
int lg_tube_sweep_param_layout(lg_tube_sweep *s, int64_t *offsets, int64_t *shapes, int max_entries);   /* as lg_tube_param_layout */
int lg_tube_sweep_params_changed(lg_tube_sweep *s, int32_t k);   /* after the caller wrote member k's params; k = -1: all members
                                                                    (one launch per member) */
int lg_tube_sweep_set_step(lg_tube_sweep *s, int64_t step);
/* The arguments of lg_tube_set_data; the split is shared by all members. */
int lg_tube_sweep_set_data(lg_tube_sweep *s, int which, const float *x, const float *y, const float *v, int64_t rows, int32_t T,
                           int32_t nz, int32_t m);
int lg_tube_sweep_begin_epoch(lg_tube_sweep *s, int64_t epoch);   /* every member's permutation, keyed by (its seed, epoch); one launch */
/* One Adam step of every member on `count` rows: rows (device, count) shared by all members, or NULL = the next count rows of
 * each member's own permutation.  Two launches for all members. */
int lg_tube_sweep_step(lg_tube_sweep *s, const int32_t *rows, int64_t count);
int lg_tube_sweep_eval(lg_tube_sweep *s);          /* every member's test metrics into its lg_tube_buffers.eval; two launches */
int lg_tube_sweep_eval_level(lg_tube_sweep *s, float level);   /* lg_tube_eval_level of every member; two launches */

/* ------------------------------------------------------------------ ROM-on-ROM simulator (deep_tube_learning/custom_sim.py
 * CustomSim with the `custom` branch of data_collection_trajectory.py:87-90 and configs/data_generation/double_single_int.yaml;
 * DESIGN.md section 10.2): a DoubleInt2D "robot" (state x, y, vx, vy; input = acceleration) tracks the random trajectory of the
 * SingleInt2D reduced-order model under the DoubleSingleTracking law (controllers.py:80-92).  Tube data without a policy.
 * One lane per env; lg_romsim_collect runs a whole epoch -- reset, every env step, every record -- in one launch.
 * The generator state is the LG_TG_* row and its laws are those of the trajectory env (csrc/lg_traj.h).
 * Draws: Philox keyed (seed, env_offset + env, counter, slot) with counter = epoch << 32 | event; event 0 = the reset of that
 * epoch (LG_RS_SLOT_*), event r + 1 = the env's r-th generator resample since that reset (LG_TG_NDRAW slots; r = 0 is the
 * reset's own).  The epoch counts resets, from 1.  With lg_romsim_inject the draws are read from lg_romsim_buffers.inject
 * instead: per env LG_RS_NRESET floats in LG_RS_SLOT_* order, then R blocks of LG_TG_NDRAW (torch.randint's value as itself). */
#define LG_RS_SLOT_ROOT 0      /* 4: root_states in [noise_lo, noise_hi] (custom_sim.py:88-91) */
#define LG_RS_SLOT_MASK 4      /* 1: start offset applied when u > zero_rom_dist_llh (:83) */
#define LG_RS_SLOT_DIST 5      /* 2: start offset in +-max_rom_dist (:84) */
#define LG_RS_SLOT_RAMP 7      /* 2: ramp_v_end drawn at construction (rom_dynamics.py:495); read by the first reset only */
#define LG_RS_NRESET 9
#define LG_RS_NOBS 8           /* root_states 4, interpolated trajectory point 0 (2), v_trajectory[:, 1] (2)  (custom_sim.py:95-100) */
typedef struct lg_romsim_cfg {
    int32_t num_envs, env_offset, N, dN;
    /* class selectors: 0 is the supported class, anything else is refused (lg_romsim_check_cfg) */
    int32_t model_cls /*0 DoubleInt2D*/, rom_cls /*0 SingleInt2D*/, controller_cls /*0 DoubleSingleTracking*/;
    int32_t generator_cls /*LG_TG_KIND_*: RANDOM only*/, t_samp_cls /*0 UniformSampleHoldDT*/, weight_sampler /*LG_TG_WSAMP_**/;
    int32_t randomize_rom_distance, _pad;
    uint64_t seed;
    float model_dt, rom_dt, Kp, Kd;
    float model_z_min[4], model_z_max[4];         /* only the velocity bounds [2..3] act (DoubleInt2D.clip_v_z) */
    float model_v_min[2], model_v_max[2];         /* acceleration bounds */
    float rom_v_min[2], rom_v_max[2];
    float t_low, t_high, freq_low, freq_high, prob_stationary, zero_rom_dist_llh;
    float max_rom_dist[2];
    float noise_lo[4], noise_hi[4];               /* init_state.default_noise_lower / upper */
} lg_romsim_cfg;

typedef struct lg_romsim_buffers {
    float *root_states;                   /* (N, 4) */
    float *tg_state;                      /* (N, LG_TG_STRIDE), LG_TG_* */
    float *tg_traj;                       /* (N, N dN + 1, 2) ROM states, oldest first (TrajectoryGenerator.trajectory) */
    float *v_traj;                        /* (N, N dN, 2) ROM inputs (TrajectoryGenerator.v_trajectory, rom_dynamics.py:505,586-587) */
    float *trajectory;                    /* (N, N, 2) the window interpolated at the env's time (get_trajectory) */
    float *obs;                           /* (N, LG_RS_NOBS) */
    float *actions;                       /* (N, 2) the action the last env step applied */
    uint8_t *done;                        /* (N) zeros: CustomSim.step returns done all False */
    float *inject;                        /* (N, inject_K) or NULL before lg_romsim_inject */
    int32_t *n_resample;                  /* (N) generator resamples of the env since its last reset */
    int32_t *inject_overrun;              /* 1: resamples that found the injected blocks used up (lg_romsim_inject_status) */
    int64_t inject_K;                     /* LG_RS_NRESET + R LG_TG_NDRAW */
} lg_romsim_buffers;

typedef struct lg_romsim lg_romsim;
int lg_romsim_check_cfg(const lg_romsim_cfg *cfg);   /* 0 inside the supported envelope, else -1 and lg_last_error names the field */
/* CustomSim.__init__ (custom_sim.py:7-35): buffers only; the construction draw of ramp_v_end is made by the first reset. */
int lg_romsim_create(const lg_romsim_cfg *cfg, lg_romsim **out);
int lg_romsim_destroy(lg_romsim *s);
int lg_romsim_set_stream(lg_romsim *s, void *stream);
int lg_romsim_get_buffers(lg_romsim *s, lg_romsim_buffers *out);
/* resets made so far (the Philox epoch of the last reset); set by tests / resume.  epoch >= 0. */
int lg_romsim_set_epoch(lg_romsim *s, int64_t epoch);
int64_t lg_romsim_get_epoch(lg_romsim *s);
/* enable != 0: replay recorded draws with room for R >= 1 resamples per env (allocates inject, zero-filled, when R changes).
 * The state installed through the buffers is taken as constructed (no construction draw) when constructed != 0. */
int lg_romsim_inject(lg_romsim *s, int enable, int32_t R, int constructed);
/* Waits for the stream.  -1 if a resample since the last call needed more injected blocks than R (those resamples re-read the
 * last block: nothing is read out of bounds); clears the count. */
int lg_romsim_inject_status(lg_romsim *s);
/* CustomSim.reset_idx (custom_sim.py:77-93) for all envs: ids = NULL or DEVICE int32[num_envs] holding 0..num_envs-1 in order;
 * n != num_envs (a partial reset) is refused. */
int lg_romsim_reset(lg_romsim *s, const int32_t *ids, int n);
/* CustomSim.step (custom_sim.py:71-75) + get_observations (:95-100).  actions: DEVICE (N, 2) f32, or NULL = DoubleSingleTracking
 * with DoubleInt2D.clip_v_z (controllers.py:87-92, rom_dynamics.py:244-250) on the current observation. */
int lg_romsim_step(lg_romsim *s, const float *actions);
/* The controller alone: out (rows, 2) from obs (rows, LG_RS_NOBS), both DEVICE. */
int lg_romsim_policy(lg_romsim *s, const float *obs, float *out, int64_t rows);
/* One epoch of data_collection_trajectory.py:111-149 in one launch: reset, then T records, each after as many env steps (built-in
 * controller) as the ROM step counter k needs to advance.  DEVICE outputs z (N, T+1, 2), v (N, T, 2), pz_x (N, T+1, 2),
 * done (N, T) u8, x (N, T+1, 4) or NULL.  An env's records equal, bit for bit, lg_romsim_reset + repeated lg_romsim_step(NULL). */
int lg_romsim_collect(lg_romsim *s, int32_t T, float *z, float *v, float *pz_x, uint8_t *done, float *x);

/* ------------------------------------------------------------------ tube datasets built on the device:
 * the rows of deep_tube_learning/datasets.py (tube/data.py) from records laid out as lg_romsim_collect or an epoch pickle has them:
 * z, pz_x (n_env, T+1, n) f32, v (n_env, T, m) f32, done (n_env, T) u8.  Per (env e, step t < T) a base row b[e, t]:
 *     scalar, recursive      (w, z[2:], v)      w = |pz_x - z|, sqrtf of the squares summed in column order, one rounding per op
 *     scalar, not recursive  (z[2:], v)         and the single column w[e, t] in front of the whole window
 *     vector                 (|pz_x - z|, z, v)
 *     error dynamics         (pz_x - z, z, v)
 * Block i < N of row (e, t) is b[e, src], src = (T-1 - i dN) - (T-1 - t) dN, when src >= 0, else b[e, 0] with its m v columns zeroed.
 * The target is the leading quantity at t + 1 (1 column for scalar, n otherwise).
 * compact = 1 drops the rows with done[e, t] != 0 -- and, with mark_last_env = 1, every row of the envs e with
 * e % epoch_envs == epoch_envs - 1 (construct_dataset's done[-1, :] = True per epoch) -- keeping (env, time) order; the order and
 * the bytes do not depend on the run (no atomics).  compact = 0 writes all n_env T rows in order.
 * Envelope: n 2..6, m 1..4, N >= 1, dN >= 1, T >= 1, input_dim <= LG_TUBE_MAX_IN, epoch_envs divides n_env.
 * Every entry returns 0, or -1 with the reason (the field named) in lg_last_error.  Every array is a DEVICE pointer; the builds
 * queue their launches on `stream` and wait for nothing. */
#define LG_TUBE_ROWS_SCALAR 0
#define LG_TUBE_ROWS_VECTOR 1
#define LG_TUBE_ROWS_ERROR 2
typedef struct lg_tube_rows_spec {
    int32_t kind /*LG_TUBE_ROWS_**/, N, dN, recursive;
    int32_t n, m, T, n_env;
    int32_t compact, mark_last_env, epoch_envs, _pad;
} lg_tube_rows_spec;
int lg_tube_rows_check(const lg_tube_rows_spec *spec);                  /* host code: needs no GPU */
int lg_tube_rows_dims(const lg_tube_rows_spec *spec, int32_t *input_dim, int32_t *output_dim);   /* host code */
int64_t lg_tube_rows_workspace(const lg_tube_rows_spec *spec);          /* bytes (0 for compact = 0); -1 outside the envelope */
/* data (rows, input_dim), target (rows, output_dim) with room for n_env T rows; n_rows: one int64, the rows written.  workspace:
 * lg_tube_rows_workspace bytes, 8-byte aligned; done and workspace may be NULL for compact = 0.  Rows past n_rows are not touched. */
int lg_tube_rows_build(const lg_tube_rows_spec *spec, const float *z, const float *pz_x, const float *v, const uint8_t *done,
                       float *data, float *target, int64_t *n_rows, void *workspace, void *stream);
/* ScalarHorizonTubeDataset's arrays, padded in front by H_rev steps (w and z with their first sample, v with zeros):
 * w (n_env, T + H_rev), z_no_pos (n_env, T + H_rev, n - 2) (no columns, and may be NULL, for n = 2), v_pad (n_env, T + H_rev, m).
 * Uses steps 0..T-1 of z and pz_x.  No compaction. */
int lg_tube_horizon_build(const float *z, const float *pz_x, const float *v, int64_t n_env, int32_t T, int32_t n, int32_t m,
                          int32_t H_rev, float *w, float *z_no_pos, float *v_pad, void *stream);

/* ------------------------------------------------------------------ batched exact k-th smallest: the order
 * statistic of conformal calibration.  values (B, ld) f32, batch row b = values[b ld .. b ld + n), ld >= n, no alignment or padding
 * asked of the rows; keep NULL or (n) u8 shared by every batch row, element i takes part iff keep[i] != 0; ranks (B, R) int64,
 * 1-based; out (B, R) f32; n_kept one int64, the number of kept elements.  out[b, r] is the ranks[b, r]-th smallest kept element
 * of row b in IEEE order: -0.0 counts and comes back as +0.0; every NaN sorts above +inf (torch.sort's place for it) and comes back
 * as the canonical quiet NaN; a rank below 1 or above n_kept gives +inf.  Exact, and the same bits on every run: four passes of a
 * most-significant-digit radix select over the order-preserving key, integer counting only.
 * Envelope: 1 <= B <= 4096, 1 <= R <= 8, 1 <= n < 2^31.  Every array is a DEVICE pointer; workspace: lg_select_workspace(B, R)
 * bytes, 8-byte aligned, contents arbitrary (the call clears it).  The call queues its work on `stream` and waits for nothing.
 * 0, or -1 with the reason (the field named) in lg_last_error. */
int64_t lg_select_workspace(int32_t B, int32_t R);     /* host code; bytes, -1 outside the envelope */
int32_t lg_select_chunk(void);                         /* host code; elements per step of a workgroup's walk over its row */
int lg_select_kth(const float *values, int64_t ld, int32_t B, int64_t n, const uint8_t *keep, const int64_t *ranks, int32_t R,
                  float *out, int64_t *n_kept, void *workspace, void *stream);

/* ------------------------------------------------------------------ grouped exact k-th smallest: one
 * conformal offset per group -- per age of a roll-out, say -- from one call.  values (B, ld) f32 as for lg_select_kth; group (n)
 * int32 shared by every batch row, 4-byte aligned: element i belongs to group group[i] when 0 <= group[i] < G and takes no part
 * otherwise; cov_num, cov_den: R coverages as fractions, HOST arrays read by the call, 1 <= num < den <= 2^31 - 1.
 * Written by the call: counts (G) int64, the members of each group (the same for every batch row); ranks (G, R) int64,
 * ranks[g, r] = ceil((counts[g] + 1) cov_num[r] / cov_den[r]), computed on the device in 64-bit integers, no host round trip
 * between the count and the selection; out (B, G, R) f32, out[b, g, r] = the ranks[g, r]-th smallest member of group g in row b,
 * in lg_select_kth's order and with its special values (-0.0 counts and returns +0.0, NaNs above +inf returning the canonical
 * quiet NaN); a rank above counts[g] -- an empty group included -- gives +inf, and ranks[g, r] is still written.
 * Envelope: 1 <= B <= 4096, 1 <= G <= LG_SELECT_MAX_GROUPS, 1 <= R <= 8, B G R <= 65536 (1 KiB of bins per (row, group, rank)),
 * 1 <= n < 2^31.  values, group, out, counts and ranks are DEVICE pointers; workspace: lg_select_grouped_workspace(B, G, R) bytes,
 * 8-byte aligned, contents arbitrary (the call clears it).  The call queues its work on `stream` and waits for nothing; the same
 * bits on every run.  0, or -1 with the reason (the field named) in lg_last_error. */
#define LG_SELECT_MAX_GROUPS 1024
int64_t lg_select_grouped_workspace(int32_t B, int32_t G, int32_t R);   /* host code; bytes, -1 outside the envelope */
int32_t lg_select_group_tile(int32_t R);                                /* host code; groups one workgroup counts at a time */
int lg_select_kth_grouped(const float *values, int64_t ld, int32_t B, int64_t n, const int32_t *group, int32_t G,
                          const int64_t *cov_num, const int64_t *cov_den, int32_t R, float *out, int64_t *counts, int64_t *ranks,
                          void *workspace, void *stream);

/* ------------------------------------------------------------------ plans against a tube: score B plans
 * -- a start z0 and N inputs of the SingleInt2D ROM -- against a one-shot horizon tube, and track B plans on the ROM-on-ROM model, one
 * launch each.  The evaluation step of a planner; no optimiser is part of it.  Reference lines: trajopt/tube_trajopt.py ("TT"),
 * deep_tube_learning/evaluation/evaluate_tube_simple_oneshot_on_mpc_traj.py ("MT"), trajopt/rom_dynamics.py ("RD"). */
#define LG_PLAN_MAX_N 64
#define LG_PLAN_MAX_OBS 8
#define LG_PLAN_STEP_MAX_HREV 64                   /* LG_PLAN_TUBE_NN_STEP: the caller's history, 0..64 steps */
#define LG_PLAN_TUBE_NN 0                          /* the one-shot MLP of a horizon lg_tube handle (TT:561-568, tube_dyn "NN_oneshot") */
#define LG_PLAN_TUBE_L1 1                          /* scaling (|vx| + |vy|)                                      (TT:489-499) */
#define LG_PLAN_TUBE_L2 2                          /* scaling (vx^2 + vy^2)                                      (TT:502-512) */
#define LG_PLAN_TUBE_L1_ROLLING 3                  /* mean of the last min(window_size, k + 1) l1 values         (TT:515-526) */
#define LG_PLAN_TUBE_L2_ROLLING 4                  /* the same of the l2 values                                  (TT:529-540) */
#define LG_PLAN_TUBE_NN_STEP 5                     /* the one-step MLP of a flat scalar lg_tube handle, fed back node by node (section 10.13) */
typedef struct lg_plan_problem {                   /* one problem for every plan of a call (TT:11-21 problem_dict, TT:460 solve_tube);
                                                    * a goal and obstacles per plan: lg_plan_scenes below (section 10.14) */
    int32_t N /*nodes after the start: 1..LG_PLAN_MAX_N*/, H_rev /*past steps of the tube item*/, n_obs /*0..LG_PLAN_MAX_OBS*/;
    int32_t tube_kind /*LG_PLAN_TUBE_**/, window_size /*rolling kinds: >= 1*/, recursive /*nn_step: 0 / 1, the row layout*/;
    float dt /*ROM step, > 0*/, scaling /*analytic kinds*/, w_max, Qw;
    float obs_c[LG_PLAN_MAX_OBS][2], obs_r[LG_PLAN_MAX_OBS], goal[2];
    float Q[4], Qf[4], R[4];                       /* 2 x 2, row-major; each quadratic is sum((d @ M) * d) (TT:41-56) */
    float rom_z_min[2], rom_z_max[2], rom_v_min[2], rom_v_max[2];
} lg_plan_problem;
/* Host code, needs no GPU.  0, or -1 with the field named in lg_last_error: N outside 1..64, n_obs outside 0..8, dt <= 0, a negative
 * radius, an unknown tube_kind, window_size < 1 on a rolling kind, the NN kind without a handle, a handle that is not a horizon
 * handle or whose H_fwd != N, nz != 0 (input_dim != H_rev + 2 (H_rev + N) [+ 1]) or H_rev differs from the problem's, has_level
 * given on an unconditioned handle or missing on a conditioned one.  tube may be NULL for the analytic kinds (it is then not read).
 * LG_PLAN_TUBE_NN_STEP (the recursion of trajopt/old/rom_tube_planning.py:106-107): the handle is a FLAT one
 * (a horizon handle is refused) with output_dim 1.  The taps T come from the handle: with I' = input_dim minus the level column,
 * I' = 1 + 2 T (recursive = 0) or I' = 3 T (recursive = 1); any other I' is refused, and so are recursive outside 0 / 1, H_rev
 * outside 0..64 or below T - 1 (the delayed taps of node 0 come from e and v_prev) and the level rules above.
 * Row of node k: [ww(k), vv(k), vv(k-1), .., vv(k-T+1), (level)] or, recursive, [ww(k), vv(k), ww(k-1), vv(k-1), .., (level)] with
 * vv(j) = v[j] (j >= 0) or v_prev[H_rev + j], ww(j) = fw[j-1] (j >= 1), w0 (j = 0) or e[H_rev + j]; fw[k] = MLP(row_k), the raw value
 * fed back, never the calibrated one.  fw equals lg_tube_rollout_window on such rows (fb = 1, taps 1 or T with stride 3, no reseed)
 * bit for bit.  lg_plan_score, lg_plan_mppi_step and lg_plan_mppi take the kind (k_plan_score_step, k_plan_sample_score_step);
 * lg_plan_grad* and lg_plan_descend* refuse it: reverse mode through N chained MLP passes is not built. */
int lg_plan_check(const lg_plan_problem *prob, const lg_tube *tube, int32_t has_level);
/* Per-plan scenes: a goal and an
 * obstacle list of its own for every plan of a scoring or gradient launch, or for every instance of an MPPI launch, in place of the
 * one goal and list of lg_plan_problem.  Everything else of the problem -- N, dt, the tube, the weights, the bounds -- stays shared.
 * Row r of a tile reads scene base + r from a row of 27 floats in LDS (2 goal, 24 obstacles, the count), staged once per tile; a
 * tile of candidates reads its instance's one row.  The walk and the reverse walk are the arithmetic of a call without scenes, operation
 * for operation, so plan b of a call with scenes equals, bit for bit, a call of B = 1 without scenes on a problem that carries
 * scene b (an MPPI instance p: a P = 1 call with instance_offset + p). */
typedef struct lg_plan_scenes {                    /* DEVICE pointers; one scene per plan (scoring, gradient) or per instance (MPPI) */
    int64_t S;                                     /* must equal the call's B (or P) */
    const float *goal;                             /* (S, 2), or NULL = prob->goal for every scene */
    const float *obs;                              /* (S, LG_PLAN_MAX_OBS, 3): cx, cy, r; slots past n_obs[s] are not read */
    const int32_t *n_obs;                          /* (S); obs and n_obs are both given or both NULL (= the problem's obstacles) */
    const float *vel;                              /* (S, LG_PLAN_MAX_OBS, 2): ux, uy in m/s of every obstacle slot, or NULL = every
                                                    * obstacle stands still (section 10.18).  obs holds the centres at node 0, "now";
                                                    * at node k of the plan obstacle i is at c_i + u_i * t_k, t_k = (float)k * prob->dt,
                                                    * three roundings (k dt, u t_k, c + ..).  Needs obs; slots past n_obs[s] are not read */
} lg_plan_scenes;
/* Host code, needs no GPU.  0, or -1 with the field named in lg_last_error: S < 1, S != count, one of obs / n_obs without the other,
 * all three of goal, obs, n_obs NULL (the struct then says nothing: pass NULL scenes), or vel without obs.  The arrays are not read: n_obs[s] is clamped into
 * 0..LG_PLAN_MAX_OBS on the device, and a scene without obstacles gives min_clear = +inf and worst_node = -1 as n_obs = 0 does.
 * Radii, centres and goals are the caller's to validate before upload (tube/plan.py Scenes does). */
int lg_plan_scenes_check(const lg_plan_scenes *scenes, int64_t count);
/* What every planner launch reads, said once: the six entries below take it after the problem (and their cfg), then only their own
 * arguments.  e, v_prev and w0 are per plan or per instance; level is read on a level_input handle only (has_level must say so).
 * With scenes, prob->goal, obs_c, obs_r and n_obs are still checked by lg_plan_check but not read by the kernel for the parts the
 * scenes supply; NULL scenes launch the kernels' instantiations without a scene row.  All six tube kinds are taken by the scoring
 * and MPPI entries; the gradient entries refuse nn_step.  A NULL call is refused ("null argument"). */
typedef struct lg_plan_call {                      /* DEVICE pointers */
    const float *z0;                               /* (count, 2) */
    const float *e, *v_prev, *w0;                  /* (count, H_rev) past error norms, (count, H_rev, 2), (count) the tube at node 0;
                                                    * each may be NULL = zeros */
    const float *offset;                           /* (N) a calibration offset per step ahead, or NULL */
    const lg_plan_scenes *scenes;                  /* NULL: the problem's own goal and obstacles */
    int64_t count;                                 /* B plans or P instances */
    int32_t has_level; float level;
    void *stream;
} lg_plan_call;
/* Score B = call->count plans in one launch (k_plan_score, 32 plans per 256-thread workgroup).  DEVICE pointers: v (B, N, 2).
 * Tube: fw (N) = MLP([e, v_prev.flatten(), v.flatten(), (level)]) -- the ScalarHorizonTubeDataset item at start = H_rev of w = e,
 * v = cat(v_prev, v), gathered on chip; it equals lg_tube_predict_windows (lg_tube_predict_windows_levels) on those arrays bit for
 * bit -- or the analytic kind.  The reference flattens v column-major (TT:563), not the order its dataset trained on; the dataset's
 * order is used here.  Nodes: w[0] = w0, w[k+1] = fw[k] + offset[k]; z[0] = z0, z[k+1] = z[k] + dt v[k] (RD:192, one rounding per
 * op).  g[i, k] = |z_k - c_i|^2 - (r_i + w_k)^2 (TT:59-62,73).  cost = sum_k<N (z_k - goal) Q (z_k - goal)' + the same with Qf at
 * node N + sum v_k R v_k' + Qw sum w_k^2 (TT:206-212), one chain: nodes ascending, state, input, tube term per node.
 * Outputs (DEVICE): cost (B); min_clear (B) = min g, +inf without obstacles; worst_node (B) int32, the first node that attains it
 * (-1 without obstacles); n_viol (B, 4) int32: nodes with some g < 0, steps with v outside rom_v_min/max, nodes with z outside
 * rom_z_min/max, nodes with w > w_max; fw (B, N), z (B, N+1, 2), w (B, N+1) optional (NULL = not written).
 * A plan's outputs do not depend on B or on its place in the batch; no atomics.  -1 as lg_plan_check, for B < 1 or a missing array.
 * Every shape of the envelope fits the kernel's dynamic LDS (checked where the kernel is compiled). */
int lg_plan_score(lg_tube *tube, const lg_plan_problem *prob, const lg_plan_call *call, const float *v, float *cost, float *min_clear,
                  int32_t *worst_node, int32_t *n_viol, float *fw, float *z, float *w);
/* Track B prescribed plans on the simulator's DoubleInt2D model under its DoubleSingleTracking law in one launch (k_plan_track, one
 * lane per plan; the loop of MT:75-88 at S = 1).  Kp, Kd, the velocity / acceleration bounds and the model dt are the handle's; its
 * generator state and buffers are neither read nor written.  DEVICE: z (B, N+1, 2), v (B, N, 2), x0 (B, 4) or NULL = (z[0], 0, 0).
 * S model steps per node, 1..8, refused unless |S model_dt - rom_dt| <= 1e-6 rom_dt.  Per node t and substep s the reference point
 * is z[t] + (z[t+1] - z[t]) ((s model_dt) / rom_dt) (get_trajectory's interpolation, RD:607-612; z[t] at S = 1), the feed-forward
 * v[min(t+1, N-1)] (MT:80), the action the controller's on (x, ref, ff) (MT:81, controllers.py:87-92), then x = f(x, a) (RD:224-225).
 * Outputs (DEVICE): pz_x (B, N+1, 2); w_true (B, N+1) = |pz_x - z| as lg_tube_rows_build takes it; x (B, N+1, 4) and
 * u (B, N S, 2) optional.  A plan's outputs equal, bit for bit, the same steps made one at a time with lg_romsim_policy. */
int lg_plan_track(lg_romsim *sim, const float *z, const float *v, const float *x0, int64_t B, int32_t N, int32_t S, float rom_dt,
                  float *pz_x, float *w_true, float *x, float *u);

/* ------------------------------------------------------------------ sampling planner on a tube: MPPI for P
 * problem instances at once, in place of the reference's NLP solve -- trajopt/tube_trajopt.py:460 solve_tube ("TT") -- and of the
 * re-solve at every control step of trajopt/tube_planning_closed_loop.py:82-168 ("TPCL").  The instances share one lg_plan_problem
 * (its goal and obstacles can be each instance's own: lg_plan_call.scenes, section 10.14);
 * each has its own z0 (P, 2), e (P, H_rev), v_prev (P, H_rev, 2), w0 (P) and mean plan vbar (P, N, 2).  One iteration is two
 * launches: k_plan_sample_score (K candidates per instance drawn around vbar and scored by k_plan_score's own code, no candidate
 * stored) and k_plan_mppi_update (softmin-weighted mean, elite, history). */
#define LG_MPPI_MAX_K 4096
typedef struct lg_mppi_cfg {                       /* the sampler that stands in for TT:460's solver options */
    int32_t K /*candidates per instance: a multiple of 32 in 32..LG_MPPI_MAX_K*/, iters /*>= 1*/;
    uint64_t seed;                                 /* Philox key of the call */
    int32_t instance_offset /*instance p draws as instance id instance_offset + p*/, _pad;
    float sigma /*> 0*/, sigma_decay /*(0, 1]: sigma_it = sigma * sigma_decay^it, `it` float32 products*/, lambda /*> 0*/;
    float rho_g, rho_w, rho_z;                     /* >= 0: weights of the obstacle, tube and state hinge sums */
} lg_mppi_cfg;
/* Host code, needs no GPU.  0, or -1 with the field named in lg_last_error: whatever lg_plan_check refuses, K outside 32..4096 or no
 * multiple of 32, iters < 1, sigma <= 0, sigma_decay outside (0, 1], lambda <= 0, a negative rho, P < 1, P * K past int32. */
int lg_mppi_check(const lg_mppi_cfg *cfg, const lg_plan_problem *prob, const lg_tube *tube, int32_t has_level, int64_t P);
/* For tests and tools: out (P, K, N, 2) (DEVICE), the candidates of iteration `it` around vbar (P, N, 2), through the device function
 * both kernels draw with.  Candidate j of instance p: clip(vbar[p] + sigma_it eps, rom_v_min, rom_v_max) with eps from one
 * Philox4x32-10 block per (instance_offset + p, it, j, node), keyed by seed: Box-Muller, cosine branch x, sine branch y.  Candidate 0
 * is the mean plan (eps = 0).  The tube handle is not read. */
int lg_plan_mppi_candidates(const lg_plan_problem *prob, const lg_mppi_cfg *cfg, int32_t it, const float *vbar, int64_t P, float *out,
                            void *stream);
/* One iteration `it` (cfg->iters is not read): what & 1 launches k_plan_sample_score, what & 2 k_plan_mppi_update.  DEVICE pointers;
 * P = call->count instances.
 * Score: J (P, K) = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z, one rounding per operation, where cost and the nodes are
 * lg_plan_score's of the candidate and pen_g = sum_k sum_i max(0, -g[i, k]), pen_w = sum_k max(0, w_k - w_max), pen_z = sum_k sum_d
 * max(0, z_d - z_max_d) + max(0, z_min_d - z_d), nodes 0..N ascending.  Optional (NULL = not written): cost (P, K), min_clear (P, K),
 * pen (P, K, 3).  A candidate's outputs do not depend on P, K or its place in a tile.
 * Update (reads J, so J may be given): weights expf(-(J_j - Jmin) / lambda), 0 for a non-finite J; vbar[p] becomes the weighted mean
 * of the candidates, drawn again; sums in an order fixed by K alone, no float atomics.  With no finite J vbar[p] stays and n_bad[p]
 * (int32) counts the iteration.  best_J (P), best_v (P, N, 2): the first arg-min candidate wherever Jmin < best_J; reset_best != 0
 * starts them (and n_bad) afresh, so they need no initial value.  hist_row (P, 2) optional: (J of candidate 0, Jmin). */
int lg_plan_mppi_step(lg_tube *tube, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, const lg_plan_call *call, int32_t it, int32_t what,
                      int32_t reset_best, float *vbar, float *J, float *cost, float *min_clear, float *pen, float *best_J, float *best_v,
                      float *hist_row, int32_t *n_bad);
/* The plan of TT:460 by cfg->iters iterations of lg_plan_mppi_step from the mean plans in vbar (in-out): 2 iters launches on the
 * stream, no host synchronisation.  J_scratch (P, K); best_J (P), best_v (P, N, 2), n_bad (P) int32 are started by the call;
 * hist (iters, P, 2) optional. */
int lg_plan_mppi(lg_tube *tube, const lg_plan_problem *prob, const lg_mppi_cfg *cfg, const lg_plan_call *call, float *vbar,
                 float *J_scratch, float *best_J, float *best_v, float *hist, int32_t *n_bad);

/* ------------------------------------------------------------------ gradient planner on a tube: the
 * objective of lg_plan_mppi_step, J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z, of B plans and its gradient dJ/dv by a
 * reverse sweep in the scoring tile (k_plan_grad, 32 plans per 256-thread workgroup, one launch), with projected Adam and an elite
 * fused behind it: a first-order stand-in for the NLP solve of trajopt/tube_trajopt.py:460.  Plain fp32 FMA arithmetic; the forward
 * half is lg_plan_mppi_step's code, so J, cost, min_clear and pen carry its bits.  A hinge max(0, a) has derivative 1 where a > 0
 * strictly, else 0; |v| has derivative 0 at 0; ReLU'(0) = 0.  w0, z0, e, v_prev and the level get no gradient. */
typedef struct lg_grad_cfg {
    int32_t iters;                                 /* >= 1: stepping launches of lg_plan_descend */
    float lr /*> 0*/, beta1, beta2 /*[0, 1)*/, eps /*> 0*/;   /* Adam, bias-corrected */
    float rho_g, rho_w, rho_z;                     /* >= 0: weights of the obstacle, tube and state hinge sums */
} lg_grad_cfg;
/* Host code, needs no GPU.  0, or -1 with the field named in lg_last_error: whatever lg_plan_check refuses, iters < 1, lr <= 0, a
 * beta outside [0, 1), eps <= 0, a negative rho, B < 1 or past int32. */
int lg_plan_grad_check(const lg_grad_cfg *cfg, const lg_plan_problem *prob, const lg_tube *tube, int32_t has_level, int64_t B);
/* One evaluation of B = call->count plans.  DEVICE pointers; call->z0 and v (B, N, 2) required.
 * Outputs: J (B), grad (B, N, 2) = dJ/dv; cost (B), min_clear (B), pen (B, 3) optional (NULL = not written).  Of cfg only the
 * rho are read (the rest is still checked).  A plan's outputs do not depend on B or on its place in a tile; no atomics. */
int lg_plan_grad(lg_tube *tube, const lg_plan_problem *prob, const lg_grad_cfg *cfg, const lg_plan_call *call, const float *v, float *J,
                 float *grad, float *cost, float *min_clear, float *pen);
/* One iteration `it` (cfg->iters is not read) in one launch: what = 1 evaluates the plans in v (B, N, 2); what = 3 also steps them
 * in place (the step is fused into the launch that makes the gradient, so 2 alone is refused).  Evaluation: J (B) required; grad,
 * cost, min_clear, pen optional as above; the elite best_J (B), best_v (B, N, 2) takes the plan evaluated wherever J is finite and
 * J < best_J; hist_row (B, 2) optional = (J, max |dJ/dv|).  Step, per element, every operation rounded on its own, with t = it + 1:
 * m = beta1 m + (1 - beta1) g; s = beta2 s + ((1 - beta2) g) g; v = clip(v - lr (m / (1 - beta1^t)) / (sqrt(s / (1 - beta2^t)) + eps),
 * rom_v_min, rom_v_max), the two bias corrections rounded once from double.  A plan whose J or gradient is not finite keeps v, m
 * and s, and n_bad[b] (int32) counts the step.  reset != 0 starts m, s (B, N, 2), the elite and n_bad afresh, so they need no
 * initial value; a reset without a finite J leaves best_J = inf and best_v = the plan. */
int lg_plan_descend_step(lg_tube *tube, const lg_plan_problem *prob, const lg_grad_cfg *cfg, const lg_plan_call *call, int32_t it,
                         int32_t what, int32_t reset, float *v, float *J, float *grad, float *cost, float *min_clear, float *pen, float *m,
                         float *s, float *best_J, float *best_v, float *hist_row, int32_t *n_bad);
/* cfg->iters stepping launches from the plans in v (in-out), then one evaluation-only launch, so that the elite also covers the
 * last iterate: iters + 1 launches on the stream, no host synchronisation.  J_scratch (B); m, s (B, N, 2), best_J, best_v and n_bad
 * are started by the call; hist (iters + 1, B, 2) optional. */
int lg_plan_descend(lg_tube *tube, const lg_plan_problem *prob, const lg_grad_cfg *cfg, const lg_plan_call *call, float *v,
                    float *J_scratch, float *m, float *s, float *best_J, float *best_v, float *hist, int32_t *n_bad);

/* ------------------------------------------------------------------ a fleet's scenes: the robots of a fleet
 * are each other's moving obstacles.  One launch writes, for every robot p of P, the obs / vel / n_obs arrays of an lg_plan_scenes of
 * S = P from the fleet's own positions and velocities, with nothing read back:
 *   1. its n_s = clamp(n_static[p], 0, 8) static obstacles first, each centre advanced to time t: c + u * t, two roundings, its
 *      velocity static_vel (zeros where static_vel is NULL; n_s = 0 where static_obs is NULL);
 *   2. then at most min(max_neighbours, 8 - n_s) other robots q != p with d2 = dx*dx + dy*dy <= sense_radius*sense_radius, d2 in
 *      float32 with every operation rounded on its own; a d2 that is not finite never passes;
 *   3. neighbours ordered by (d2, q) ascending -- the walk sums and takes minima over obstacles in slot order;
 *   4. a neighbour's slot is (pos_q, separation) with velocity vel_q;
 *   5. slots past n_obs[p] are zeros.
 * Every array is a DEVICE pointer.  0, or -1 with the field named in lg_last_error before a device is touched: a null cfg or required
 * array, separation or sense_radius negative or not finite, max_neighbours outside 0..8, P outside 1..2^31-1, static_obs without
 * n_static or the reverse, static_vel without static_obs, t not finite. */
typedef struct lg_fleet_cfg {
    float separation;                              /* the radius of a neighbour's disc: the distance two robots keep, centre to centre */
    float sense_radius;                            /* robots farther than this are not seen */
    int32_t max_neighbours;                        /* 0..LG_PLAN_MAX_OBS */
} lg_fleet_cfg;
int lg_plan_fleet_scenes(const lg_fleet_cfg *cfg, const float *pos /*(P,2)*/, const float *vel /*(P,2)*/, int64_t P,
                         const float *static_obs /*(P,8,3) or NULL*/, const float *static_vel /*(P,8,2) or NULL*/,
                         const int32_t *n_static /*(P) or NULL*/, float t, float *obs /*(P,8,3)*/, float *obs_vel /*(P,8,2)*/,
                         int32_t *n_obs /*(P)*/, void *stream);

/* ------------------------------------------------------------------ command tracker: ROM trajectories
 * tracked by a VELOCITY-COMMAND policy, the loop of deep_tube_learning/data_collection_velocity.py:84-156 ("DV").  A SingleInt2D ROM
 * at rom_dt = the env's dt runs beside the velocity-command env; a proportional law turns its desired pose and velocity into a
 * body-frame velocity command, written over the three command columns of the observation; the velocity policy does the rest.
 * One launch per env step, one lane per env, nothing read back.  Per env and step t, fp32 with one rounding per operation:
 *   v = input(t rom_dt): RANDOM = TrajectoryGenerator.get_input_t with the stationary mask (the LG_TG_* row and the laws of
 *       csrc/lg_traj.h, the hold time checked on every evaluation); PLAN = plan[env][t], 0 for t >= n_nodes, used as given;
 *   des = (z_x, z_y, atan2(v_y, v_x)), des_vel = (v_x, v_y, 0)                                  (SingleInt2D.des_pose_vel)
 *   yaw = atan2(2 (q_x q_y + q_w q_z), q_w^2 + q_x^2 - q_y^2 - q_z^2)   (quat2yaw: the xyz-Euler yaw, for a quaternion of any norm)
 *   err = des - (x, y, yaw); err[2] = track_yaw ? ((err[2] + pi) mod 2 pi) - pi : 0, mod in the floor sense       (DV:129-130)
 *   err_local[:2] = [[c, s], [-s, c]] err[:2], des_vel_local[:2] likewise, c = cos yaw, s = sin yaw                (DV:133,138)
 *   u = min(max(des_vel_local + Kp err_local, u_min), u_max)                                                      (DV:140-141)
 *   obs[env, cmd_col + j] = u[j] cmd_scale[j]  (DV:144 writes u raw: cmd_scale = 1; the env's own observation holds
 *                                               command x commands_scale, which is what cmd_scale defaults to on the host)
 * and, after the env step that consumed command t (DV:149-156): done[t] = the env's reset flag, v[t] = v, u[t] = u,
 * z[t+1] = done ? root xy : z + rom_dt v, pz_x[t+1] = root xy, x[t+1] = get_state().  The next step's ROM state is z[t+1].  The
 * generator is not reset on a done.  The env's commands buffer, rewards and heading logic are not touched.
 * Records are ENV-MAJOR -- z, pz_x (N, T+1, 2), v (N, T, 2), done (N, T), u (N, T, 3), x (N, T+1, x_n) -- the layout of
 * lg_romsim_collect and the epoch pickles; DV's own arrays are time-major.
 * Draws (RANDOM): lg_romsim's keys, Philox (seed, env_offset + env, epoch << 32 | event, slot) with event 0 = the begin
 * (LG_RS_SLOT_RAMP only, at the tracker's first begin) and event r + 1 = the env's r-th resample since the begin; with
 * lg_cmdtrack_inject they are read from lg_cmdtrack_buffers.inject in lg_romsim_inject's block layout.
 * Lifetime: the tracker holds no pointer into the env -- every entry that touches the device takes the env and borrows its
 * buffers and stream for that call alone -- so either may be destroyed first; an entry refuses an env of other dimensions than
 * the one the tracker was created for. */
typedef struct lg_cmdtrack_cfg {
    int32_t kind /*LG_TG_KIND_RANDOM | LG_TG_KIND_PLAN*/, track_yaw, cmd_col /*9 for every LeggedRobot observation*/;
    int32_t weight_sampler /*LG_TG_WSAMP_**/, tg_N /*ROM steps of TrajectoryGenerator.reset's pre-roll, 1..LG_TRAJ_MAX_PTS-1*/;
    int32_t x_n;                          /* floats per row of the optional x record: 0, or the env's 13 + 2 num_actions */
    uint64_t seed;
    float Kp[9];                          /* row-major 3 x 3 */
    float u_min[3], u_max[3], cmd_scale[3];
    float rom_v_min[2], rom_v_max[2];
    float t_low, t_high, freq_low, freq_high, prob_stationary, _padf;
} lg_cmdtrack_cfg;
typedef struct lg_cmdtrack_rec {          /* caller-owned DEVICE buffers of one epoch */
    int32_t T, _pad;
    float *z, *v, *pz_x;                  /* (N, T+1, 2), (N, T, 2), (N, T+1, 2) */
    uint8_t *done;                        /* (N, T) */
    float *u;                             /* (N, T, 3) or NULL */
    float *x;                             /* (N, T+1, x_n) or NULL */
} lg_cmdtrack_rec;
typedef struct lg_cmdtrack_buffers {
    float *state;                         /* (N, 8): z 2, v 2, u 3 of the command in force, 1 unused */
    float *tg_state;                      /* (N, LG_TG_STRIDE) */
    float *plan;                          /* (N, LG_PLAN_MAX_N, 2) */
    float *inject;                        /* (N, inject_K) or NULL before lg_cmdtrack_inject */
    int32_t *n_resample, *inject_overrun; /* (N) each: resamples since the begin; resamples that found the injected blocks used up */
    int64_t inject_K;                     /* LG_RS_NRESET + R LG_TG_NDRAW */
} lg_cmdtrack_buffers;
typedef struct lg_cmdtrack lg_cmdtrack;
/* Host code, needs no GPU.  0, or -1 with the field named in lg_last_error ("lg_cmdtrack: ...").  rec may be NULL (the
 * configuration alone).  env_traj: the env is a trajectory env (refused); num_obs, env_x_n: the env's. */
int lg_cmdtrack_check(const lg_cmdtrack_cfg *cfg, const lg_cmdtrack_rec *rec, int32_t env_traj, int32_t num_obs, int32_t env_x_n);
int lg_cmdtrack_create(lg_ctx *env, const lg_cmdtrack_cfg *cfg, lg_cmdtrack **out);
int lg_cmdtrack_destroy(lg_cmdtrack *tr);
int lg_cmdtrack_get_buffers(lg_cmdtrack *tr, lg_cmdtrack_buffers *out);
/* PLAN: v DEVICE f32 (N, n_nodes, 2), 0 <= n_nodes <= LG_PLAN_MAX_N (v may be NULL at 0); a copy ordered on the env's stream. */
int lg_cmdtrack_set_plans(lg_cmdtrack *tr, lg_ctx *env, const float *v, int32_t n_nodes);
int lg_cmdtrack_inject(lg_cmdtrack *tr, int enable, int32_t R);
/* 0, or -1 if a resample found its block missing since the last call (waits for the device; clears the counts) */
int lg_cmdtrack_inject_status(lg_cmdtrack *tr);
/* One launch: the generator restarts as TrajectoryGenerator.reset(root xy) leaves it, z = root xy, row 0 of z, pz_x (x), then
 * command 0 into obs.  epoch: 0..2^31-1, the key of this epoch's draws. */
int lg_cmdtrack_begin(lg_cmdtrack *tr, lg_ctx *env, const lg_cmdtrack_rec *rec, int64_t epoch);
/* One launch, after env step t (0 <= t < T; a host integer): the record of step t, then, if t + 1 < T, command t + 1 into obs. */
int lg_cmdtrack_step(lg_cmdtrack *tr, lg_ctx *env, const lg_cmdtrack_rec *rec, int32_t t);

/* ------------------------------------------------------------------ privileged observations: the
 * critic's own observation row, the buffer the reference allocates, clips and returns but never fills
 * (legged_robot_config.py:38 num_privileged_obs; base_task.py:62-79 the buffer, :104-105 get_privileged_observations;
 * legged_robot.py:100-104 the clip and step()'s second return value).  A row is a list of terms; entry j of a term is
 *   out[env, off_term + j] = min(max(raw * scale_term, -clip_observations), +clip_observations)
 * in fp32 with one rounding per operation, off_term = the widths of the terms before it.  raw per kind:
 *   OBS                  num_obs      the policy observation entry BEFORE noise, by the expressions of legged_robot.py:208-226
 *                                     (trajectory env: legged_robot_trajectory.py:280-288): with noise off and scale 1 it is obs
 *   FRICTION             1            lg_buffers.friction          (legged_robot.py:259-282)
 *   BASE_MASS            1            lg_buffers.base_mass_delta   (legged_robot.py:330-341)
 *   MATERIAL             4            lg_buffers.material          (legged_robot.py:284-299,337-339)
 *   FEET_CONTACT_FORCES  3 num_feet   contact_forces[env, feet_idx[f], :]
 *   FEET_CONTACT         num_feet     contact_forces[env, feet_idx[f], 2] > 1 ? 1 : 0        (_reward_feet_air_time's contact test)
 *   FEET_AIR_TIME        num_feet     lg_buffers.feet_air_time
 *   BODY_CONTACT         num_pen      |contact_forces[env, pen_idx[b], :]|^2 > 0.01 ? 1 : 0  (_reward_collision's norm > 0.1)
 *   TORQUES              num_actions  lg_buffers.torques
 *   HEIGHTS              H            the height block of OBS; refused unless measure_heights
 *   EPISODE_PROGRESS     1            (float)episode_length * float(1 / max_episode_length)
 * One launch on the env's stream AFTER the step (lg_step / lg_post_physics_step), so an env the step reset shows its post-reset
 * state, as obs does.  It reads the env's buffers, writes only its own, and leaves a deferred step epilogue (lg_ppo_attach_env)
 * deferred.  Lifetime as lg_cmdtrack: the handle keeps no pointer into the env; lg_priv_obs_compute takes the env, borrows its
 * buffers and stream for that call and refuses an env of other dimensions than the one the handle was created for. */
#define LG_PRIV_MAX_TERMS 16
#define LG_PRIV_MAX_WIDTH 1024
enum { LG_PRIV_OBS = 0, LG_PRIV_FRICTION, LG_PRIV_BASE_MASS, LG_PRIV_MATERIAL, LG_PRIV_FEET_CONTACT_FORCES, LG_PRIV_FEET_CONTACT,
       LG_PRIV_FEET_AIR_TIME, LG_PRIV_BODY_CONTACT, LG_PRIV_TORQUES, LG_PRIV_HEIGHTS, LG_PRIV_EPISODE_PROGRESS, LG_PRIV_NUM_KINDS };
typedef struct lg_priv_term { int32_t kind /*LG_PRIV_**/; float scale; } lg_priv_term;
typedef struct lg_priv_cfg {
    int32_t num_terms /*1..LG_PRIV_MAX_TERMS, each kind at most once*/, _pad;
    lg_priv_term terms[LG_PRIV_MAX_TERMS];
} lg_priv_cfg;
typedef struct lg_priv_obs lg_priv_obs;
/* Host code, needs no GPU.  0 and *width (may be NULL) = the row's width, or -1 with the field named in lg_last_error
 * ("lg_priv_obs: ...").  The dimensions are the env's lg_cfg fields of the same names. */
int lg_priv_obs_check(const lg_priv_cfg *cfg, int32_t num_obs, int32_t num_actions, int32_t num_feet, int32_t num_pen,
                      int32_t num_height_points, int32_t measure_heights, int32_t *width);
int lg_priv_obs_create(lg_ctx *env, const lg_priv_cfg *cfg, lg_priv_obs **out);
/* *out: DEVICE f32 (num_envs, *width), zeros until the first lg_priv_obs_compute */
int lg_priv_obs_buffer(lg_priv_obs *po, float **out, int32_t *width);
int lg_priv_obs_compute(lg_priv_obs *po, lg_ctx *env);
int lg_priv_obs_destroy(lg_priv_obs *po);

/* ------------------------------------------------------------------ actor observation history: a
 * stacked row for a feed-forward actor, W = num_obs + (length - 1) S wide, S = the number of selected obs columns.  Env i after
 * step t holds, newest first,
 *   [ obs_t (all num_obs columns) | sel(obs_t-1) | sel(obs_t-2) | ... | sel(obs_t-length+1) ]
 * where a frame is lg_buffers.obs as the actor saw it (after noise and the clip) and sel() keeps the columns of the ranges in
 * order.  An env is REINITIALISED by a compute when lg_buffers.reset (the step's dones) is set for it or when it was marked
 * (lg_obs_hist_mark) since the previous compute: every past frame becomes sel(obs_t) (REPEAT) or zeros (ZERO), so no frame of
 * the previous episode survives a reset.  Pure copying: the row can be restated bit for bit.
 * One launch on the env's stream AFTER the step.  It reads only lg_buffers.obs and lg_buffers.reset, writes only the handle's
 * row, and leaves a deferred step epilogue (lg_ppo_attach_env) deferred.  Lifetime as lg_priv_obs: the handle keeps no pointer into
 * the env; every call takes the env, borrows its buffers and stream for that call and refuses an env whose num_envs or num_obs
 * differ from those of the env the handle was created for.  Env and handle may be destroyed in either order. */
#define LG_OBS_HIST_MAX_RANGES 8
#define LG_OBS_HIST_MAX_LENGTH 64
#define LG_OBS_HIST_MAX_WIDTH 1024
enum { LG_OBS_HIST_REPEAT = 0, LG_OBS_HIST_ZERO = 1 };
typedef struct lg_obs_hist_cfg {
    int32_t length /*frames including the current one, 2..LG_OBS_HIST_MAX_LENGTH*/,
            num_ranges /*0: every obs column is kept; else 1..LG_OBS_HIST_MAX_RANGES*/, reset_mode /*LG_OBS_HIST_**/, _pad;
    int32_t lo[LG_OBS_HIST_MAX_RANGES], hi[LG_OBS_HIST_MAX_RANGES];      /* half-open [lo, hi) of obs columns, ascending, non-overlapping */
} lg_obs_hist_cfg;
typedef struct lg_obs_hist lg_obs_hist;
/* Host code, needs no GPU.  0 and *width_out (may be NULL) = W, or -1 with the refused field named in lg_last_error
 * ("lg_obs_hist: ...": length, num_ranges, reset_mode, lo[r], hi[r] or width). */
int lg_obs_hist_check(const lg_obs_hist_cfg *cfg, int32_t num_obs, int32_t *width_out);
/* Allocates the row (zeros) and marks every env, so that the first compute initialises every row.  Waits for the device. */
int lg_obs_hist_create(lg_ctx *env, const lg_obs_hist_cfg *cfg, lg_obs_hist **out);
/* *ptr: DEVICE f32 (num_envs, *W), zeros until the first lg_obs_hist_compute */
int lg_obs_hist_buffer(lg_obs_hist *h, void **ptr, int32_t *W);
/* Marks n envs (ids_device: DEVICE int32, kept alive by the caller until the stream has passed; NULL: all envs) for
 * reinitialisation by the next compute; for a reset made outside the step (lg_reset_ids).  One small launch on the env's stream;
 * the row itself is not touched. */
int lg_obs_hist_mark(lg_obs_hist *h, lg_ctx *env, const int32_t *ids_device, int32_t n);
/* Advances every env's row by one frame (or reinitialises it) in one launch on the env's stream; the marks lapse with it.
 * A mark holds until the next successful compute: one that is refused (-1: null argument, an env of other dimensions) or whose
 * launch fails (-3) touches neither row nor marks, and the marks stay meant for the next one. */
int lg_obs_hist_compute(lg_obs_hist *h, lg_ctx *env);
/* Waits for the device, frees the row and the marks.  NULL is accepted. */
int lg_obs_hist_destroy(lg_obs_hist *h);

/* ------------------------------------------------------------------ empirical observation normalisation (DESIGN.md section
 * 10.20): running per-column moments of the rows handed to a policy, and y = (x - mean) / (std + eps).  State per column: mean
 * (0), var (1), std (1), all f32 on the device, and a row counter `count` (0) kept on the host.  update(x), x of (n, W):
 *   nothing when until >= 0 and count >= until; else count += n, rate = n / count,
 *   mean_x, var_x = column mean and BIASED column variance of the batch, delta = mean_x - mean,
 *   mean += rate * delta;  var += rate * (var_x - var + delta * (mean_x - mean)) with the new mean;  std = sqrt(var)
 * (Chan's merge: until `until` is reached the state is the pooled moments of every row seen).  The batch sums are taken in
 * double and summed in a fixed order, the rule is evaluated in double from the f32 state and rounded once, so the state and y
 * are bitwise reproducible.  A training compute (update = 1) updates and then normalises with the NEW state, in two launches
 * (k_obs_norm_stats, k_obs_norm_apply) for one handle or for a pair; a frozen compute (update = 0, or `until` reached) only
 * normalises, in one.  All launches go on the stream given; nothing in a compute waits for the device.  The handle holds no
 * pointer into an env or a learner: x and y are the caller's (or y the handle's own (max_rows, W) buffer). */
#define LG_OBS_NORM_MAX_WIDTH 1024          /* = LG_OBS_HIST_MAX_WIDTH */
#define LG_OBS_NORM_ROWS 64                 /* rows per workgroup of either kernel: a training compute keeps one (S1, S2) per 64 rows */
#define LG_OBS_NORM_COLS 64                 /* columns per workgroup: one lane per column */
typedef struct lg_obs_norm_cfg {
    int32_t width /*1..LG_OBS_NORM_MAX_WIDTH*/;
    float eps /*finite, > 0; rsl_rl's default 1e-2*/;
    int64_t until /*rows after which updates stop; -1: never; rsl_rl's default 10^8*/;
} lg_obs_norm_cfg;
typedef struct lg_obs_norm lg_obs_norm;
/* Host code, needs no GPU.  0, or -1 with the refused field named in lg_last_error ("lg_obs_norm: ...": width, eps or until). */
int lg_obs_norm_check(const lg_obs_norm_cfg *cfg);
/* Allocates the state (two copies, flipped by the host per update), the slab of batch partials for max_rows rows and a
 * (max_rows, width) output.  Waits for the device. */
int lg_obs_norm_create(const lg_obs_norm_cfg *cfg, int64_t max_rows, lg_obs_norm **out);
/* *y: DEVICE f32 (max_rows, *width), the handle's own output; zeros until the first compute into it */
int lg_obs_norm_buffer(lg_obs_norm *h, void **y, int32_t *width);
/* num = 1 or 2 handles (two different ones), x[i] DEVICE f32 (n, width_i), the same n for both.  y[i] NULL: the handle's own
 * buffer (needs n <= max_rows); else DEVICE f32 (n, width_i), not x[i].  update = 1 needs n <= max_rows (the slab); a handle
 * whose `until` is reached takes the frozen path by itself.  update = 0 takes any n >= 1 when y[i] is given.  A refused call
 * (-1) or a failed launch (-3) leaves state and count as they were. */
int lg_obs_norm_compute(lg_obs_norm *const *h, const float *const *x, float *const *y, int32_t num, int64_t n, int32_t update,
                        void *stream);
/* HOST pointers (each may be NULL), `width` floats each.  Waits for the device. */
int lg_obs_norm_get_state(lg_obs_norm *h, float *mean, float *var, float *std, int64_t *count);
/* HOST pointers; std = sqrtf(var) on the host.  Refuses a negative or non-finite var, a non-finite mean and a negative count.
 * Waits for the device. */
int lg_obs_norm_set_state(lg_obs_norm *h, const float *mean, const float *var, int64_t count);
/* Waits for the device and frees everything.  NULL is accepted. */
int lg_obs_norm_destroy(lg_obs_norm *h);

#ifdef __cplusplus
}
#endif
#endif /* LEGGED_HIP_H */
