"""ctypes mirror of include/legged_hip.h (struct layouts, constants, prototypes).

Only declarations live here; ``lib.py`` loads the HIP library.  The CPU oracle under oracle/
(test infrastructure) reuses these struct definitions for its own ``lgo_*`` symbols.
"""
import ctypes as C

MAX_DOF, MAX_BODIES, MAX_SPHERES = 16, 24, 48
MAX_FEET, MAX_PEN, MAX_TERM = 8, 16, 8
LSTM_NW = 972
MAX_HIDDEN = 4

REWARD_NAMES = [
    "action_rate", "ang_vel_xy", "base_height", "collision", "dof_acc", "dof_pos_limits", "dof_vel",
    "dof_vel_limits", "feet_air_time", "feet_contact_forces", "lin_vel_z", "no_fly", "orientation",
    "stand_still", "stumble", "termination", "torque_limits", "torques", "tracking_ang_vel",
    "tracking_lin_vel"]
NUM_REWARDS = len(REWARD_NAMES)
assert REWARD_NAMES == sorted(REWARD_NAMES)

SLOT_CMD, SLOT_PUSH, SLOT_LEVEL, SLOT_DOF = 0, 3, 5, 6
MAX_XTERMS = 4
NUM_TERMS = NUM_REWARDS + MAX_XTERMS
XT_EXP_NEG_WSQ_ERR, XT_WSQ, XT_SLOPED_ERR_CHANGE = 1, 2, 3
SIGNALS = {"zero": (0, 8), "base_lin_vel": (1, 3), "base_ang_vel": (2, 3), "projected_gravity": (3, 3), "commands": (4, 4),
           "root_pos": (5, 3), "traj0": (6, 2), "prev_error": (7, 2), "dof_pos_rel": (8, MAX_DOF), "dof_vel": (9, MAX_DOF),
           "torques": (10, MAX_DOF), "actions": (11, MAX_DOF), "last_actions": (12, MAX_DOF)}      # name -> (lg_signal, length)
TRAJ_MAX_PTS, TG_NDRAW, TG_STRIDE = 17, 20, 30
TG_CENTER = 28                                                   # LG_TG_CENTER: 2 floats, CircleTrajectoryGenerator.center
TG_KINDS = {"TrajectoryGenerator": 0, "ZeroTrajectoryGenerator": 1, "SquareTrajectoryGenerator": 2,
            "CircleTrajectoryGenerator": 3,
            "PlanTrajectoryGenerator": 4}                        # LG_TG_KIND_*; the last is this project's own class (tube/plan_env.py)
TG_WEIGHT_SAMPLERS = {"UniformWeightSampler": 0, "UniformWeightSamplerNoRamp": 1}    # LG_TG_WSAMP_*
TG_FIELDS = {"weights": (0, 4), "t_final": (4, 1), "t": (5, 1), "k": (6, 1), "const": (7, 2), "extreme": (9, 2),
             "ramp_t_start": (11, 1), "ramp_v_start": (12, 2), "ramp_v_end": (14, 2), "sin_mag": (16, 2), "sin_freq": (18, 2),
             "sin_off": (20, 2), "sin_mean": (22, 2), "stationary": (24, 1), "v": (25, 2)}                        # LG_TG_* offsets


def tslots(A):
    """LG_TSLOT_* of the trajectory env."""
    n = TG_NDRAW
    return {"tg": 0, "push": n, "timer": n + 2, "level": n + 3, "dof": n + 4, "xy": n + 4 + A, "vel": n + 6 + A,
            "romd": n + 12 + A, "rtg": n + 15 + A, "noise": 2 * n + 15 + A}


def slot_xy(A): return 6 + A
def slot_vel(A): return 8 + A
def slot_rcmd(A): return 14 + A
def slot_noise(A): return 17 + A


f32, i32, i64, u8, u64 = C.c_float, C.c_int32, C.c_int64, C.c_uint8, C.c_uint64
PF, PU8, PI64, PI32 = C.POINTER(f32), C.POINTER(u8), C.POINTER(i64), C.POINTER(i32)


class lg_model(C.Structure):
    _fields_ = [
        ("num_bodies", i32), ("num_dofs", i32), ("num_legs", i32), ("joints_per_leg", i32),
        ("num_spheres", i32), ("_pad0", i32 * 3),
        ("mass", f32 * (MAX_DOF + 1)), ("com", f32 * 3 * (MAX_DOF + 1)), ("inertia", f32 * 9 * (MAX_DOF + 1)),
        ("R_pj", f32 * 9 * MAX_DOF), ("p_pj", f32 * 3 * MAX_DOF), ("axis", f32 * 3 * MAX_DOF),
        ("q_lower", f32 * MAX_DOF), ("q_upper", f32 * MAX_DOF), ("effort", f32 * MAX_DOF),
        ("vel_limit", f32 * MAX_DOF), ("joint_damping", f32 * MAX_DOF),
        ("body_dyn", i32 * MAX_BODIES), ("sph_link", i32 * MAX_SPHERES), ("sph_body", i32 * MAX_SPHERES),
        ("sph_center", f32 * 3 * MAX_SPHERES), ("sph_radius", f32 * MAX_SPHERES)]


class lg_xterm(C.Structure):
    _fields_ = [("kind", i32), ("n", i32), ("sig_a", i32), ("off_a", i32), ("sig_b", i32), ("off_b", i32), ("sig_c", i32),
                ("off_c", i32), ("scale", f32), ("p", f32 * 3), ("w", f32 * 8)]


class lg_traj_cfg(C.Structure):
    _fields_ = [("enabled", i32), ("N", i32), ("dN", i32), ("randomize_rom_distance", i32),
                ("rom_dt", f32), ("t_low", f32), ("t_high", f32), ("freq_low", f32), ("freq_high", f32), ("prob_stationary", f32),
                ("zero_rom_dist_llh", f32), ("max_push_vel_xy", f32),
                ("v_min", f32 * 2), ("v_max", f32 * 2), ("obs_scale", f32 * 2), ("max_rom_dist", f32 * 2),
                ("push_t_lo", f32), ("push_t_hi", f32)]


class lg_cfg(C.Structure):
    _fields_ = [
        ("num_envs", i32), ("num_obs", i32), ("num_actions", i32), ("num_bodies", i32),
        ("num_feet", i32), ("num_pen", i32), ("num_term", i32), ("num_height_points", i32),
        ("feet_idx", i32 * MAX_FEET), ("pen_idx", i32 * MAX_PEN), ("term_idx", i32 * MAX_TERM),
        ("decimation", i32), ("control_type", i32), ("use_actuator_net", i32), ("heading_command", i32),
        ("max_episode_length", i32), ("resample_steps", i32), ("push_interval", i32), ("push_robots", i32),
        ("add_noise", i32), ("measure_heights", i32), ("only_positive_rewards", i32), ("send_timeouts", i32),
        ("terrain_type", i32), ("curriculum", i32), ("custom_origins", i32), ("max_terrain_level", i32),
        ("hf_rows", i32), ("hf_cols", i32), ("terrain_num_cols", i32), ("phys_substeps", i32),
        ("env_offset", i32), ("total_envs", i32), ("solver_iterations", i32), ("material_rand", i32),
        ("seed", u64),
        ("sim_dt", f32), ("dt", f32), ("action_scale", f32), ("clip_actions", f32), ("clip_obs", f32),
        ("max_push_vel", f32), ("episode_length_s", f32), ("ground_restitution", f32),
        ("cmd_lo", f32 * 4), ("cmd_hi", f32 * 4),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32),
        ("obs_scale_dof_vel", f32), ("obs_scale_height", f32),
        ("tracking_sigma", f32), ("soft_dof_vel_limit", f32), ("soft_torque_limit", f32),
        ("base_height_target", f32), ("max_contact_force", f32),
        ("hf_hscale", f32), ("hf_vscale", f32), ("border_size", f32), ("terrain_env_length", f32),
        ("rew_scale", f32 * NUM_REWARDS), ("base_init_state", f32 * 13),
        ("default_dof_pos", f32 * MAX_DOF), ("p_gains", f32 * MAX_DOF), ("d_gains", f32 * MAX_DOF),
        ("dof_pos_limits", f32 * 2 * MAX_DOF), ("dof_vel_limits", f32 * MAX_DOF), ("torque_limits", f32 * MAX_DOF),
        ("gravity", f32 * 3), ("ground_friction", f32),
        ("contact_offset", f32), ("max_depenetration_velocity", f32), ("contact_erp", f32), ("bounce_threshold", f32),
        ("max_linear_velocity", f32), ("max_angular_velocity", f32), ("armature", f32), ("rest_offset", f32),
        ("num_xterms", i32), ("feet_air_time_ungated", i32), ("num_terms", i32), ("_pad4", i32),
        ("term_order", i32 * NUM_TERMS), ("xterms", lg_xterm * MAX_XTERMS), ("traj", lg_traj_cfg),
        ("lstm_w", f32 * LSTM_NW),
        ("noise_vec", PF), ("height_points", PF), ("terrain_origins", PF)]


_BUF_FIELDS = [
    ("root_states", PF), ("dof_state", PF), ("contact_forces", PF), ("torques", PF), ("actions", PF),
    ("obs", PF), ("rew", PF), ("reset", PU8), ("time_out", PU8), ("episode_length", PI64),
    ("commands", PF), ("last_actions", PF), ("last_dof_vel", PF), ("last_root_vel", PF), ("feet_air_time", PF),
    ("last_contacts", PU8), ("episode_sums", PF), ("base_lin_vel", PF), ("base_ang_vel", PF),
    ("projected_gravity", PF), ("measured_heights", PF), ("env_origins", PF),
    ("terrain_levels", PI64), ("terrain_types", PI64), ("lstm_h", PF), ("lstm_c", PF),
    ("friction", PF), ("base_mass_delta", PF), ("extras_episode", PF), ("extras_terrain_level", PF),
    ("extras_time_outs", PU8), ("extras_episode_acc", PF), ("n_reset", PI32), ("n_fault", PI32), ("fault_total", PI64),
    ("n_vel_clamp", PI32), ("vel_clamp_total", PI64),
    ("tg_state", PF), ("tg_traj", PF), ("trajectory", PF), ("prev_error", PF), ("push_timer", PF),
    ("inject_uniforms", PF), ("inject_levels", PI64), ("material", PF)]


class lg_buffers(C.Structure):
    _fields_ = _BUF_FIELDS


class lg_stage(C.Structure):
    """Constants a curriculum stage rewrites (include/legged_hip.h lg_stage)."""
    _fields_ = [("cmd_lo", f32 * 4), ("cmd_hi", f32 * 4), ("max_push_vel", f32), ("_pad", f32), ("push_time", C.c_double),
                ("rew_scale", f32 * NUM_REWARDS), ("xterm_scale", f32 * MAX_XTERMS), ("xterm_p0", f32 * MAX_XTERMS),
                ("traj_v_min", f32 * 2), ("traj_v_max", f32 * 2), ("traj_t_low", f32), ("traj_t_high", f32),
                ("traj_max_rom_dist", f32 * 2)]


def buffer_shapes(N, A, B, O, F, H, traj_N=0, traj_dN=1):
    """name -> (shape, numpy dtype string) of every lg_buffers entry."""
    K = (tslots(A)["noise"] if traj_N else slot_noise(A)) + O
    return {
        "tg_state": ((N, TG_STRIDE), "f4"), "tg_traj": ((N, traj_N * traj_dN + 1, 2), "f4"),
        "trajectory": ((N, max(traj_N, 1), 2), "f4"), "prev_error": ((N, 2), "f4"), "push_timer": ((N,), "f4"),
        "root_states": ((N, 13), "f4"), "dof_state": ((N, A, 2), "f4"), "contact_forces": ((N, B, 3), "f4"),
        "torques": ((N, A), "f4"), "actions": ((N, A), "f4"), "obs": ((N, O), "f4"), "rew": ((N,), "f4"),
        "reset": ((N,), "u1"), "time_out": ((N,), "u1"), "episode_length": ((N,), "i8"),
        "commands": ((N, 4), "f4"), "last_actions": ((N, A), "f4"), "last_dof_vel": ((N, A), "f4"),
        "last_root_vel": ((N, 6), "f4"), "feet_air_time": ((N, F), "f4"), "last_contacts": ((N, F), "u1"),
        "episode_sums": ((NUM_TERMS, N), "f4"), "base_lin_vel": ((N, 3), "f4"), "base_ang_vel": ((N, 3), "f4"),
        "projected_gravity": ((N, 3), "f4"), "measured_heights": ((N, max(H, 1)), "f4"),
        "env_origins": ((N, 3), "f4"), "terrain_levels": ((N,), "i8"), "terrain_types": ((N,), "i8"),
        "lstm_h": ((2, N * A, 8), "f4"), "lstm_c": ((2, N * A, 8), "f4"), "friction": ((N,), "f4"),
        "base_mass_delta": ((N,), "f4"), "extras_episode": ((NUM_TERMS,), "f4"),
        "extras_terrain_level": ((1,), "f4"), "extras_time_outs": ((N,), "u1"),
        "extras_episode_acc": ((NUM_TERMS + 2,), "f4"), "n_reset": ((1,), "i4"),
        "n_fault": ((1,), "i4"), "fault_total": ((1,), "i8"), "n_vel_clamp": ((1,), "i4"), "vel_clamp_total": ((1,), "i8"),
        "inject_uniforms": ((N, K), "f4"), "inject_levels": ((N,), "i8"), "material": ((N, 4), "f4")}


class lg_ppo_cfg(C.Structure):
    _fields_ = [
        ("num_envs", i32), ("num_obs", i32), ("num_critic_obs", i32), ("num_actions", i32),
        ("num_hidden", i32), ("actor_hidden", i32 * MAX_HIDDEN), ("critic_hidden", i32 * MAX_HIDDEN),
        ("activation", i32), ("num_steps", i32), ("num_epochs", i32), ("num_mini_batches", i32),
        ("adaptive_schedule", i32), ("use_clipped_value_loss", i32), ("world_size", i32), ("_pad", i32),
        ("seed", u64),
        ("init_noise_std", f32), ("value_loss_coef", f32), ("clip_param", f32), ("entropy_coef", f32),
        ("learning_rate", f32), ("gamma", f32), ("lam", f32), ("desired_kl", f32), ("max_grad_norm", f32),
        ("_padf", f32)]


class lg_ppo_buffers(C.Structure):
    _fields_ = [
        ("params", PF), ("grads", PF), ("adam_m", PF), ("adam_v", PF),
        ("obs", PF), ("critic_obs", PF), ("actions", PF), ("rewards", PF), ("values", PF), ("returns", PF),
        ("advantages", PF), ("log_prob", PF), ("mu", PF), ("sigma", PF), ("dones", PU8),
        ("act_actions", PF), ("act_values", PF), ("act_log_prob", PF), ("act_mu", PF),
        ("stats", PF), ("noise", PF), ("perm", PI32), ("adv_partial", PF),
        ("cur_reward_sum", PF), ("cur_episode_len", PF), ("ep_stats", PF), ("ep_ring", PF), ("ep_ring_count", PI32),
        ("num_params", i64), ("num_reduce", i64)]


class lg_ppo_rnn_cfg(C.Structure):
    _fields_ = [("type", i32), ("hidden", i32), ("layers", i32), ("_pad", i32)]


class lg_ppo_rnn_buffers(C.Structure):
    _fields_ = [("h", PF * 2), ("c", PF * 2), ("saved_h", PF * 2), ("saved_c", PF * 2), ("hidden", i64)]


TUBE_MAX_IN, TUBE_MAX_OUT, TUBE_MAX_UNITS = 256, 64, 128     # LG_TUBE_MAX_*; num_units a multiple of 16, num_layers 1..4
TUBE_SWEEP_MAX = 64                                             # LG_TUBE_SWEEP_MAX: members of one lg_tube_sweep
TUBE_RING_MAX = 1024                                            # LG_TUBE_RING_MAX: floats of output history per sequence (rollout_window)
TUBE_ACT = {"relu": 0, "softplus": 1, "tanh": 2, "elu": 3}      # LG_TUBE_ACT_*
TUBE_MAX_LEVELS = 64                                            # levels of one lg_tube_predict_levels call
TUBE_LOSS = {"scalar": 0, "vector": 1, "mse": 2}                # LG_TUBE_LOSS_*


class lg_tube_cfg(C.Structure):
    _fields_ = [
        ("input_dim", i32), ("output_dim", i32), ("num_units", i32), ("num_layers", i32),
        ("activation", i32), ("loss", i32), ("horizon", i32), ("batch_size", i32),
        ("H_fwd", i32), ("H_rev", i32), ("step_size", i32), ("_pad", i32),
        ("seed", u64),
        ("alpha", f32), ("delta", f32), ("softplus_beta", f32), ("_padf", f32),
        ("lr", C.c_double), ("gamma", C.c_double),
        ("level_input", i32), ("_pad2", i32), ("level_lo", f32), ("level_hi", f32)]


class lg_tube_buffers(C.Structure):
    _fields_ = [
        ("params", PF), ("grads", PF), ("adam_m", PF), ("adam_v", PF), ("log", PF), ("eval", PF),
        ("starts", PI32), ("perm", PI32),
        ("num_params", i64), ("log_cap", i64), ("starts_cap", i64), ("perm_cap", i64), ("step", i64),
        ("levels", PF), ("levels_cap", i64)]


def declare_tube_api(lib):
    vp = C.c_void_p
    lib.lg_tube_check_cfg.argtypes = [C.POINTER(lg_tube_cfg)]
    lib.lg_tube_create.argtypes = [C.POINTER(lg_tube_cfg), C.POINTER(vp)]
    lib.lg_tube_destroy.argtypes = [vp]
    lib.lg_tube_set_stream.argtypes = [vp, vp]
    lib.lg_tube_get_buffers.argtypes = [vp, C.POINTER(lg_tube_buffers)]
    lib.lg_tube_param_layout.argtypes = [vp, PI64, PI64, C.c_int]
    lib.lg_tube_params_changed.argtypes = [vp]
    lib.lg_tube_set_step.argtypes = [vp, i64]
    lib.lg_tube_set_data.argtypes = [vp, C.c_int, vp, vp, vp, i64, i32, i32, i32]
    lib.lg_tube_begin_epoch.argtypes = [vp, i64]
    lib.lg_tube_step.argtypes = [vp, vp, i64]
    lib.lg_tube_eval.argtypes = [vp]
    lib.lg_tube_predict.argtypes = [vp, vp, vp, i64, vp]
    lib.lg_tube_predict_windows.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, i64, vp]
    lib.lg_tube_rollout.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    lib.lg_tube_rollout_window.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp]
    lib.lg_tube_sweep_create.argtypes = [C.POINTER(lg_tube_cfg), i32, C.POINTER(vp)]
    lib.lg_tube_sweep_destroy.argtypes = [vp]
    lib.lg_tube_sweep_set_stream.argtypes = [vp, vp]
    lib.lg_tube_sweep_get_buffers.argtypes = [vp, i32, C.POINTER(lg_tube_buffers)]
    lib.lg_tube_sweep_param_layout.argtypes = [vp, PI64, PI64, C.c_int]
    lib.lg_tube_sweep_params_changed.argtypes = [vp, i32]
    lib.lg_tube_sweep_set_step.argtypes = [vp, i64]
    lib.lg_tube_sweep_set_data.argtypes = [vp, C.c_int, vp, vp, vp, i64, i32, i32, i32]
    lib.lg_tube_sweep_begin_epoch.argtypes = [vp, i64]
    lib.lg_tube_sweep_step.argtypes = [vp, vp, i64]
    lib.lg_tube_sweep_eval.argtypes = [vp]
    lib.lg_tube_eval_level.argtypes = [vp, f32]
    lib.lg_tube_predict_levels.argtypes = [vp, vp, vp, i64, vp, i32, vp]
    lib.lg_tube_predict_windows_levels.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, i64, vp, i32, vp]
    lib.lg_tube_sweep_eval_level.argtypes = [vp, f32]


RS_SLOT_ROOT, RS_SLOT_MASK, RS_SLOT_DIST, RS_SLOT_RAMP, RS_NRESET, RS_NOBS = 0, 4, 5, 7, 9, 8     # LG_RS_*


class lg_romsim_cfg(C.Structure):
    _fields_ = [
        ("num_envs", i32), ("env_offset", i32), ("N", i32), ("dN", i32),
        ("model_cls", i32), ("rom_cls", i32), ("controller_cls", i32), ("generator_cls", i32), ("t_samp_cls", i32),
        ("weight_sampler", i32), ("randomize_rom_distance", i32), ("_pad", i32),
        ("seed", u64),
        ("model_dt", f32), ("rom_dt", f32), ("Kp", f32), ("Kd", f32),
        ("model_z_min", f32 * 4), ("model_z_max", f32 * 4), ("model_v_min", f32 * 2), ("model_v_max", f32 * 2),
        ("rom_v_min", f32 * 2), ("rom_v_max", f32 * 2),
        ("t_low", f32), ("t_high", f32), ("freq_low", f32), ("freq_high", f32), ("prob_stationary", f32),
        ("zero_rom_dist_llh", f32), ("max_rom_dist", f32 * 2), ("noise_lo", f32 * 4), ("noise_hi", f32 * 4)]


class lg_romsim_buffers(C.Structure):
    _fields_ = [
        ("root_states", PF), ("tg_state", PF), ("tg_traj", PF), ("v_traj", PF), ("trajectory", PF), ("obs", PF),
        ("actions", PF), ("done", PU8), ("inject", PF), ("n_resample", PI32), ("inject_overrun", PI32), ("inject_K", i64)]


def declare_romsim_api(lib):
    vp = C.c_void_p
    if not hasattr(lib, "lg_romsim_create"):       # an A/B library (LG_HIP_LIB) built before the simulator: its entries stay undeclared
        return
    lib.lg_romsim_check_cfg.argtypes = [C.POINTER(lg_romsim_cfg)]
    lib.lg_romsim_create.argtypes = [C.POINTER(lg_romsim_cfg), C.POINTER(vp)]
    lib.lg_romsim_destroy.argtypes = [vp]
    lib.lg_romsim_set_stream.argtypes = [vp, vp]
    lib.lg_romsim_get_buffers.argtypes = [vp, C.POINTER(lg_romsim_buffers)]
    lib.lg_romsim_set_epoch.argtypes = [vp, i64]
    lib.lg_romsim_get_epoch.argtypes = [vp]
    lib.lg_romsim_get_epoch.restype = i64
    lib.lg_romsim_inject.argtypes = [vp, C.c_int, i32, C.c_int]
    lib.lg_romsim_inject_status.argtypes = [vp]
    lib.lg_romsim_reset.argtypes = [vp, vp, C.c_int]
    lib.lg_romsim_step.argtypes = [vp, vp]
    lib.lg_romsim_policy.argtypes = [vp, vp, vp, i64]
    lib.lg_romsim_collect.argtypes = [vp, i32, vp, vp, vp, vp, vp]


TUBE_ROWS_KIND = {"scalar": 0, "vector": 1, "error_dynamics": 2}     # LG_TUBE_ROWS_*


class lg_tube_rows_spec(C.Structure):
    _fields_ = [
        ("kind", i32), ("N", i32), ("dN", i32), ("recursive", i32),
        ("n", i32), ("m", i32), ("T", i32), ("n_env", i32),
        ("compact", i32), ("mark_last_env", i32), ("epoch_envs", i32), ("_pad", i32)]


def declare_tube_data_api(lib):
    vp, ps = C.c_void_p, C.POINTER(lg_tube_rows_spec)
    if not hasattr(lib, "lg_tube_rows_build"):     # an A/B library (LG_HIP_LIB) built before the device builder
        return
    lib.lg_tube_rows_check.argtypes = [ps]
    lib.lg_tube_rows_dims.argtypes = [ps, PI32, PI32]
    lib.lg_tube_rows_workspace.argtypes = [ps]
    lib.lg_tube_rows_workspace.restype = i64
    lib.lg_tube_rows_build.argtypes = [ps, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lg_tube_horizon_build.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp]


def declare_select_api(lib):
    vp = C.c_void_p
    if not hasattr(lib, "lg_select_kth"):          # an A/B library (LG_HIP_LIB) built before the selection
        return
    lib.lg_select_workspace.argtypes = [i32, i32]
    lib.lg_select_workspace.restype = i64
    lib.lg_select_chunk.argtypes = []
    lib.lg_select_chunk.restype = i32
    lib.lg_select_kth.argtypes = [vp, i64, i32, i64, vp, vp, i32, vp, vp, vp, vp]
    if not hasattr(lib, "lg_select_kth_grouped"):  # an A/B library built before the grouped selection
        return
    lib.lg_select_grouped_workspace.argtypes = [i32, i32, i32]
    lib.lg_select_grouped_workspace.restype = i64
    lib.lg_select_group_tile.argtypes = [i32]
    lib.lg_select_group_tile.restype = i32
    lib.lg_select_kth_grouped.argtypes = [vp, i64, i32, i64, vp, i32, C.POINTER(i64), C.POINTER(i64), i32, vp, vp, vp, vp, vp]


PLAN_MAX_N, PLAN_MAX_OBS = 64, 8                                # LG_PLAN_MAX_*
PLAN_STEP_MAX_HREV = 64                                         # LG_PLAN_STEP_MAX_HREV
PLAN_TUBE = {"nn": 0, "l1": 1, "l2": 2, "l1_rolling": 3, "l2_rolling": 4, "nn_step": 5}     # LG_PLAN_TUBE_*


class lg_plan_problem(C.Structure):
    _fields_ = [
        ("N", i32), ("H_rev", i32), ("n_obs", i32), ("tube_kind", i32), ("window_size", i32), ("recursive", i32),
        ("dt", f32), ("scaling", f32), ("w_max", f32), ("Qw", f32),
        ("obs_c", (f32 * 2) * 8), ("obs_r", f32 * 8), ("goal", f32 * 2),
        ("Q", f32 * 4), ("Qf", f32 * 4), ("R", f32 * 4),
        ("rom_z_min", f32 * 2), ("rom_z_max", f32 * 2), ("rom_v_min", f32 * 2), ("rom_v_max", f32 * 2)]


MPPI_MAX_K = 4096                                               # LG_MPPI_MAX_K


class lg_mppi_cfg(C.Structure):
    _fields_ = [
        ("K", i32), ("iters", i32), ("seed", u64), ("instance_offset", i32), ("_pad", i32),
        ("sigma", f32), ("sigma_decay", f32), ("lambda_", f32), ("rho_g", f32), ("rho_w", f32), ("rho_z", f32)]


class lg_grad_cfg(C.Structure):
    _fields_ = [
        ("iters", i32), ("lr", f32), ("beta1", f32), ("beta2", f32), ("eps", f32), ("rho_g", f32), ("rho_w", f32), ("rho_z", f32)]


class lg_plan_scenes(C.Structure):
    """One goal and obstacle list per plan or MPPI instance (include/legged_hip.h lg_plan_scenes); device pointers."""
    _fields_ = [("S", i64), ("goal", C.c_void_p), ("obs", C.c_void_p), ("n_obs", C.c_void_p), ("vel", C.c_void_p)]


class lg_fleet_cfg(C.Structure):
    """How a fleet's robots see each other (include/legged_hip.h lg_fleet_cfg)."""
    _fields_ = [("separation", f32), ("sense_radius", f32), ("max_neighbours", i32)]


class lg_plan_call(C.Structure):
    """What every planner launch reads (include/legged_hip.h lg_plan_call); device pointers."""
    _fields_ = [("z0", C.c_void_p), ("e", C.c_void_p), ("v_prev", C.c_void_p), ("w0", C.c_void_p), ("offset", C.c_void_p),
                ("scenes", C.POINTER(lg_plan_scenes)), ("count", i64), ("has_level", i32), ("level", f32), ("stream", C.c_void_p)]


def declare_plan_api(lib):
    """An entry that an A/B library (LG_HIP_LIB) was built before stays undeclared.  lib.plan_api_old: the library still has the
    *_scenes twins, so it was built before lg_plan_call and its six planning entries take the older positional lists; they stay
    undeclared too, and HipPlanScorer refuses the library (calling them with today's lists would corrupt memory)."""
    vp = C.c_void_p
    pp, pc, pg = C.POINTER(lg_plan_problem), C.POINTER(lg_mppi_cfg), C.POINTER(lg_grad_cfg)
    ps, pk = C.POINTER(lg_plan_scenes), C.POINTER(lg_plan_call)
    lib.plan_api_old = hasattr(lib, "lg_plan_score_scenes")
    sigs = {"lg_plan_check": [pp, vp, i32], "lg_plan_track": [vp, vp, vp, vp, i64, i32, i32, f32, vp, vp, vp, vp],
            "lg_mppi_check": [pc, pp, vp, i32, i64], "lg_plan_mppi_candidates": [pp, pc, i32, vp, i64, vp, vp],
            "lg_plan_grad_check": [pg, pp, vp, i32, i64], "lg_plan_scenes_check": [ps, i64],
            "lg_plan_fleet_scenes": [C.POINTER(lg_fleet_cfg), vp, vp, i64, vp, vp, vp, f32, vp, vp, vp, vp]}
    if not lib.plan_api_old:                       # (tube, prob, [cfg,] call, the entry's own arguments)
        sigs.update({"lg_plan_score": [vp, pp, pk] + [vp] * 8,
                     "lg_plan_mppi_step": [vp, pp, pc, pk, i32, i32, i32] + [vp] * 9, "lg_plan_mppi": [vp, pp, pc, pk] + [vp] * 6,
                     "lg_plan_grad": [vp, pp, pg, pk] + [vp] * 6,
                     "lg_plan_descend_step": [vp, pp, pg, pk, i32, i32, i32] + [vp] * 12, "lg_plan_descend": [vp, pp, pg, pk] + [vp] * 8})
    for name, argtypes in sigs.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes


class lg_traj_rec(C.Structure):
    """The ROM-rate recorder's caller-owned device buffers (include/legged_hip.h lg_traj_rec)."""
    _fields_ = [("rows_max", i32), ("x_n", i32), ("z", C.c_void_p), ("pz_x", C.c_void_p), ("v", C.c_void_p), ("rows", C.c_void_p),
                ("dead", C.c_void_p), ("k_mark", C.c_void_p), ("x", C.c_void_p)]


class lg_cmdtrack_cfg(C.Structure):
    """The command tracker's law and generator (include/legged_hip.h lg_cmdtrack_cfg)."""
    _fields_ = [("kind", i32), ("track_yaw", i32), ("cmd_col", i32), ("weight_sampler", i32), ("tg_N", i32), ("x_n", i32),
                ("seed", u64),
                ("Kp", f32 * 9), ("u_min", f32 * 3), ("u_max", f32 * 3), ("cmd_scale", f32 * 3),
                ("rom_v_min", f32 * 2), ("rom_v_max", f32 * 2),
                ("t_low", f32), ("t_high", f32), ("freq_low", f32), ("freq_high", f32), ("prob_stationary", f32), ("_padf", f32)]


class lg_cmdtrack_rec(C.Structure):
    """One epoch's caller-owned device records, env-major (include/legged_hip.h lg_cmdtrack_rec)."""
    _fields_ = [("T", i32), ("_pad", i32), ("z", C.c_void_p), ("v", C.c_void_p), ("pz_x", C.c_void_p), ("done", C.c_void_p),
                ("u", C.c_void_p), ("x", C.c_void_p)]


class lg_cmdtrack_buffers(C.Structure):
    _fields_ = [("state", PF), ("tg_state", PF), ("plan", PF), ("inject", PF), ("n_resample", PI32), ("inject_overrun", PI32),
                ("inject_K", i64)]


CT_STATE = 8                                                    # LG_CT_STATE: z 2, v 2, u 3, 1 unused


def declare_cmdtrack_api(lib):
    """The lg_cmdtrack_* entries; raises if the library was built without them (there is no fallback)."""
    vp, pc, pr = C.c_void_p, C.POINTER(lg_cmdtrack_cfg), C.POINTER(lg_cmdtrack_rec)
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_cmdtrack_check.argtypes = [pc, pr, i32, i32, i32]
    lib.lg_cmdtrack_create.argtypes = [vp, pc, C.POINTER(vp)]
    lib.lg_cmdtrack_destroy.argtypes = [vp]
    lib.lg_cmdtrack_get_buffers.argtypes = [vp, C.POINTER(lg_cmdtrack_buffers)]
    lib.lg_cmdtrack_set_plans.argtypes = [vp, vp, vp, i32]
    lib.lg_cmdtrack_inject.argtypes = [vp, C.c_int, i32]
    lib.lg_cmdtrack_inject_status.argtypes = [vp]
    lib.lg_cmdtrack_begin.argtypes = [vp, vp, pr, i64]
    lib.lg_cmdtrack_step.argtypes = [vp, vp, pr, i32]
    return lib


PRIV_MAX_TERMS, PRIV_MAX_WIDTH = 16, 1024                       # LG_PRIV_MAX_*
PRIV_TERMS = ["obs", "friction", "base_mass", "material", "feet_contact_forces", "feet_contact", "feet_air_time", "body_contact",
              "torques", "heights", "episode_progress"]          # LG_PRIV_*: a term's kind is its index


class lg_priv_term(C.Structure):
    _fields_ = [("kind", i32), ("scale", f32)]


class lg_priv_cfg(C.Structure):
    """The privileged observation row, term by term (include/legged_hip.h lg_priv_cfg)."""
    _fields_ = [("num_terms", i32), ("_pad", i32), ("terms", lg_priv_term * PRIV_MAX_TERMS)]


def declare_priv_obs_api(lib):
    """The lg_priv_obs_* entries; raises if the library was built without them (there is no fallback)."""
    vp, pc = C.c_void_p, C.POINTER(lg_priv_cfg)
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_priv_obs_check.argtypes = [pc, i32, i32, i32, i32, i32, i32, PI32]
    lib.lg_priv_obs_create.argtypes = [vp, pc, C.POINTER(vp)]
    lib.lg_priv_obs_buffer.argtypes = [vp, C.POINTER(vp), PI32]
    lib.lg_priv_obs_compute.argtypes = [vp, vp]
    lib.lg_priv_obs_destroy.argtypes = [vp]
    return lib


OBS_HIST_MAX_RANGES, OBS_HIST_MAX_LENGTH, OBS_HIST_MAX_WIDTH = 8, 64, 1024     # LG_OBS_HIST_MAX_*
OBS_HIST_RESET = ["repeat", "zero"]                              # LG_OBS_HIST_REPEAT / _ZERO: a mode's value is its index


class lg_obs_hist_cfg(C.Structure):
    """The actor's observation history (include/legged_hip.h lg_obs_hist_cfg)."""
    _fields_ = [("length", i32), ("num_ranges", i32), ("reset_mode", i32), ("_pad", i32),
                ("lo", i32 * OBS_HIST_MAX_RANGES), ("hi", i32 * OBS_HIST_MAX_RANGES)]


def declare_obs_hist_api(lib):
    """The lg_obs_hist_* entries; raises if the library was built without them (there is no fallback)."""
    vp, pc = C.c_void_p, C.POINTER(lg_obs_hist_cfg)
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_obs_hist_check.argtypes = [pc, i32, PI32]
    lib.lg_obs_hist_create.argtypes = [vp, pc, C.POINTER(vp)]
    lib.lg_obs_hist_buffer.argtypes = [vp, C.POINTER(vp), PI32]
    lib.lg_obs_hist_mark.argtypes = [vp, vp, vp, i32]
    lib.lg_obs_hist_compute.argtypes = [vp, vp]
    lib.lg_obs_hist_destroy.argtypes = [vp]
    return lib


OBS_NORM_MAX_WIDTH, OBS_NORM_ROWS, OBS_NORM_COLS = 1024, 64, 64       # LG_OBS_NORM_MAX_WIDTH / _ROWS / _COLS


class lg_obs_norm_cfg(C.Structure):
    """Empirical observation normalisation (include/legged_hip.h lg_obs_norm_cfg)."""
    _fields_ = [("width", i32), ("eps", f32), ("until", i64)]


def declare_obs_norm_api(lib):
    """The lg_obs_norm_* entries; raises if the library was built without them (there is no fallback)."""
    vp, pc, pf = C.c_void_p, C.POINTER(lg_obs_norm_cfg), C.POINTER(f32)
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_obs_norm_check.argtypes = [pc]
    lib.lg_obs_norm_create.argtypes = [pc, i64, C.POINTER(vp)]
    lib.lg_obs_norm_buffer.argtypes = [vp, C.POINTER(vp), PI32]
    lib.lg_obs_norm_compute.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, i64, i32, vp]
    lib.lg_obs_norm_get_state.argtypes = [vp, pf, pf, pf, C.POINTER(i64)]
    lib.lg_obs_norm_set_state.argtypes = [vp, pf, pf, i64]
    lib.lg_obs_norm_destroy.argtypes = [vp]
    return lib


def declare_env_api(lib, prefix="lg_"):
    """Attach argtypes/restypes for the env entry points on a loaded library."""
    vp = C.c_void_p
    g = lambda n: getattr(lib, prefix + n)
    g("last_error").restype = C.c_char_p
    g("last_error").argtypes = []
    g("create").argtypes = [C.POINTER(lg_cfg), C.POINTER(lg_model), C.c_void_p, C.POINTER(vp)]
    g("destroy").argtypes = [vp]
    g("get_buffers").argtypes = [vp, C.POINTER(lg_buffers)]
    g("set_step_counter").argtypes = [vp, i64]
    g("get_step_counter").argtypes = [vp]
    g("get_step_counter").restype = i64
    g("set_init_done").argtypes = [vp, C.c_int]
    g("inject_uniforms").argtypes = [vp, C.c_int]
    g("step").argtypes = [vp, vp]
    g("set_actions").argtypes = [vp, vp]
    for n in ("compute_torques", "simulate", "post_physics_step", "reset_all"):
        g(n).argtypes = [vp]
    g("reset_ids").argtypes = [vp, vp, C.c_int]
    if prefix == "lg_":
        g("finalize").argtypes = [vp]
    g("get_stage").argtypes = [vp, C.POINTER(lg_stage)]
    g("set_curriculum_stage").argtypes = [vp, C.POINTER(lg_stage), C.c_int]
    if prefix == "lg_":
        g("set_traj_generator").argtypes = [vp, C.c_int, C.c_int]
        g("traj_reset").argtypes = [vp, vp]
        if hasattr(lib, "lg_traj_set_plans"):          # an A/B library (LG_HIP_LIB) built before the plan-following generator
            g("traj_set_plans").argtypes = [vp, vp, i32]
            g("traj_rec_check").argtypes = [C.POINTER(lg_traj_rec), i64, i32]
            g("traj_rec_begin").argtypes = [vp, C.POINTER(lg_traj_rec)]
            g("traj_rec_step").argtypes = [vp, C.POINTER(lg_traj_rec)]
        if hasattr(lib, "lg_traj_replan"):             # ... or before replanning on the robot
            g("traj_replan").argtypes = [vp, vp, i32, vp]
        g("set_stream").argtypes = [vp, vp]
        lib.lg_version.restype = C.c_int
        lib.lg_version.argtypes = []


def declare_ppo_api(lib):
    """The lg_ppo_* entries of the learner itself; a library built without the PPO sources keeps them undeclared."""
    vp = C.c_void_p
    if not hasattr(lib, "lg_ppo_create"):
        return
    lib.lg_ppo_create.argtypes = [C.POINTER(lg_ppo_cfg), C.POINTER(vp)]
    lib.lg_ppo_destroy.argtypes = [vp]
    lib.lg_ppo_get_buffers.argtypes = [vp, C.POINTER(lg_ppo_buffers)]
    lib.lg_ppo_set_stream.argtypes = [vp, vp]
    lib.lg_ppo_param_layout.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    lib.lg_ppo_inject_noise.argtypes = [vp, C.c_int]
    lib.lg_ppo_act.argtypes = [vp, vp, vp]
    lib.lg_ppo_process_env_step.argtypes = [vp, vp, vp, vp]
    lib.lg_ppo_compute_returns.argtypes = [vp, vp]
    lib.lg_ppo_normalize_advantages.argtypes = [vp]
    lib.lg_ppo_begin_update.argtypes = [vp]
    lib.lg_ppo_minibatch_backward.argtypes = [vp, C.c_int, C.c_int]
    lib.lg_ppo_minibatch_step.argtypes = [vp]
    lib.lg_ppo_end_update.argtypes = [vp]
    lib.lg_ppo_act_inference.argtypes = [vp, vp, vp, C.c_int64]
    lib.lg_ppo_params_changed.argtypes = [vp]
    lib.lg_ppo_set_deterministic.argtypes = [vp, C.c_int]
    lib.lg_ppo_attach_env.argtypes = [vp, vp]
    lib.lg_ppo_create_recurrent.argtypes = [C.POINTER(lg_ppo_cfg), C.POINTER(lg_ppo_rnn_cfg), C.POINTER(vp)]
    lib.lg_ppo_get_rnn_buffers.argtypes = [vp, C.POINTER(lg_ppo_rnn_buffers)]
    lib.lg_ppo_reset_hidden.argtypes = [vp, vp]
    lib.lg_ppo_debug_bucket_extents.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.lg_ppo_debug_mb_sets.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
    lib.lg_ppo_debug_weight_planes.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(vp)]
    # the learner's entries that take a communicator (declare_comm_api)
    lib.lg_ppo_set_comm.argtypes = [vp, vp]
    lib.lg_ppo_comm_timing.argtypes = [vp, C.c_int]
    lib.lg_ppo_comm_wait_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.lg_ppo_allreduce_adv_moments.argtypes = [vp, vp]
    lib.lg_ppo_broadcast_params.argtypes = [vp, vp, C.c_int]


def declare_comm_api(lib):
    """The lg_comm_* collectives."""
    vp = C.c_void_p
    lib.lg_comm_get_unique_id.argtypes = [vp]
    lib.lg_comm_init.argtypes = [C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.lg_comm_destroy.argtypes = [vp]
    lib.lg_comm_rank.argtypes = [vp]
    lib.lg_comm_size.argtypes = [vp]
    lib.lg_comm_allreduce_sum.argtypes = [vp, vp, C.c_int64, vp]
    lib.lg_comm_broadcast.argtypes = [vp, vp, C.c_int64, C.c_int, vp]


ENV_SYMBOLS = ["last_error", "create", "destroy", "get_buffers", "set_step_counter", "get_step_counter",
               "set_init_done", "inject_uniforms", "step", "set_actions", "compute_torques", "simulate",
               "post_physics_step", "reset_all", "reset_ids", "get_stage", "set_curriculum_stage"]
PPO_SYMBOLS = ["ppo_create", "ppo_destroy", "ppo_get_buffers", "ppo_set_stream", "ppo_param_layout",
               "ppo_inject_noise", "ppo_act", "ppo_process_env_step", "ppo_compute_returns",
               "ppo_normalize_advantages", "ppo_begin_update", "ppo_minibatch_backward", "ppo_minibatch_step",
               "ppo_end_update", "ppo_act_inference", "ppo_create_recurrent", "ppo_get_rnn_buffers", "ppo_reset_hidden"]
HIP_ONLY_SYMBOLS = ["version", "set_stream"]
COMM_SYMBOLS = ["comm_get_unique_id", "comm_init", "comm_destroy", "comm_rank", "comm_size", "comm_allreduce_sum", "comm_broadcast",
                "ppo_set_comm", "ppo_allreduce_adv_moments", "ppo_broadcast_params"]
