"""What this build does with every leaf of an env configuration (``class_to_dict(LeggedRobotCfg)`` and the task / trajectory
configs derived from it): no field is silently ignored.

The reference hands most of these to Isaac Gym (asset options legged_robot.py:692-705, sim params helpers.py:parse_sim_params,
terrain params :631-677); here each leaf is exactly one of

  consumed    read and acted on; the note says where
  inert       has no effect on the results of the hot path IN THE REFERENCE either (viewer, renderer, PhysX resource knobs, fields of
              other tasks); never read here
  fixed       only the listed value(s) are accepted: anything else raises at construction (``enforce``), in the message style of
              env_setup.py's refusals -- the behaviour the other values select in the reference is not implemented
  unmodelled  accepted, with a one-time warning: the reference's behaviour for this value is NOT reproduced and the note says what is
              lost (parity with PhysX is unpinned for all of A4 anyway)

``tests/test_cfg_contract.py`` walks the cfg tree of every registered task against this table and fails on an unlisted leaf, and
checks with a recording proxy that what the table calls consumed by the setup is in fact read.
"""
from __future__ import annotations

import fnmatch
import warnings

# where a consumed leaf is read: "setup" = EnvSetup (+ to_structs / stage_values), "env" = the LeggedRobot constructor (model, terrain,
# per-env constants), "sim" = helpers.parse_sim_params / task_registry, "base" = BaseTask, "reward" = the env class's declared terms
CONSUMED, INERT, FIXED, UNMODELLED = "consumed", "inert", "fixed", "unmodelled"

# (pattern, kind, note[, accepted values for FIXED | predicate for UNMODELLED])
CONTRACT = [
    # ---- asset (legged_robot.py:692-705,745)
    ("asset.file", CONSUMED, "env: URDF path -> model/robot_model.resolve_model"),
    ("asset.name", CONSUMED, "env: asset name -> model/robot_model.resolve_model"),
    ("asset.foot_name", CONSUMED, "setup: feet_indices"),
    ("asset.penalize_contacts_on", CONSUMED, "setup: penalised_contact_indices"),
    ("asset.terminate_after_contacts_on", CONSUMED, "setup: termination_contact_indices"),
    ("asset.collapse_fixed_joints", CONSUMED, "env: model/urdf.load_urdf"),
    ("asset.replace_cylinder_with_capsule", CONSUMED, "env: model/urdf.load_urdf (collision sphere sets)"),
    ("asset.disable_gravity", CONSUMED, "setup: lg_cfg.gravity = 0 for the robot"),
    ("asset.max_angular_velocity", CONSUMED, "setup: lg_cfg.max_angular_velocity, base twist clamped after every solve (lg_physics*.h)"),
    ("asset.max_linear_velocity", CONSUMED, "setup: lg_cfg.max_linear_velocity"),
    ("asset.armature", CONSUMED, "setup: lg_cfg.armature, added to every joint's inertia about its axis (ABA inward pass)"),
    ("asset.thickness", CONSUMED, "setup: lg_cfg.rest_offset (+ sim.physx.rest_offset): the robot's shapes rest that far off the ground"),
    ("asset.fix_base_link", FIXED, "a fixed base is not implemented (floating-base ABA only)", (False,)),
    ("asset.default_dof_drive_mode", FIXED, "joints are driven by torques only (set_dof_actuation_force_tensor, legged_robot.py:92, needs "
     "effort mode); PhysX position / velocity drives are not implemented", (3,)),
    ("asset.angular_damping", FIXED, "PhysX's per-link angular velocity damping is not implemented", (0, 0.0)),
    ("asset.linear_damping", FIXED, "PhysX's per-link linear velocity damping is not implemented", (0, 0.0)),
    ("asset.density", INERT, "Isaac Gym uses it only for links without <inertial>; model/urdf.load_urdf refuses such a link when it has "
     "collision geometry, every link of the registered assets carries its own mass"),
    ("asset.flip_visual_attachments", INERT, "visual meshes only; there is no renderer"),
    ("asset.self_collisions", UNMODELLED, "0 enables self-collision in the reference (anymal_c_flat, anymal_c_flat_trajectory): contacts "
     "between the robot's own links are NOT modelled, the sphere sets collide with the terrain only -- legs pass through each other and "
     "through the base", lambda v: v == 0),
    # ---- commands
    ("commands.num_commands", FIXED, "the command vector is (lin_vel_x, lin_vel_y, ang_vel_yaw, heading)", (4,)),
    ("commands.resampling_time", CONSUMED, "setup: lg_cfg.resample_steps"),
    ("commands.heading_command", CONSUMED, "setup"),
    ("commands.ranges.*", CONSUMED, "setup: lg_cfg.cmd_lo / cmd_hi"),
    # ---- control
    ("control.control_type", CONSUMED, "setup"),
    ("control.stiffness", CONSUMED, "setup: p_gains"),
    ("control.damping", CONSUMED, "setup: d_gains"),
    ("control.action_scale", CONSUMED, "setup"),
    ("control.decimation", CONSUMED, "setup"),
    ("control.use_actuator_network", CONSUMED, "setup"),
    ("control.actuator_net_file", CONSUMED, "setup: load_actuator_weights (compiled weights, the archive is never executed)"),
    # ---- staged curriculum (read only when use_curriculum)
    ("curriculum.*", CONSUMED, "setup: CurriculumClock / stage_values (trajectory env: freq_low / freq_high / weight_sampler / rom.z rows are "
     "ignored by the reference's update as well, legged_robot_trajectory.py:519-553)"),
    # ---- domain randomisation
    ("domain_rand.randomize_friction", CONSUMED, "env: draw_env_constants"),
    ("domain_rand.friction_range", CONSUMED, "env: draw_env_constants"),
    ("domain_rand.randomize_base_mass", CONSUMED, "env: draw_env_constants"),
    ("domain_rand.added_mass_range", CONSUMED, "env: draw_env_constants"),
    ("domain_rand.randomize_inv_base_mass", UNMODELLED, "the draw is consumed in the reference's order and exposed (env.base_inv_mass) but has "
     "no effect on the dynamics", lambda v: bool(v)),
    ("domain_rand.inv_mass_range", CONSUMED, "env: draw_env_constants"),
    ("domain_rand.rigid_shape_properties.randomize_*", UNMODELLED, "restitution / compliance / thickness act through this build's own "
     "contact model (one material per robot = mean over its shapes), not PhysX's", lambda v: bool(v)),
    ("domain_rand.rigid_shape_properties.*_range", CONSUMED, "env: draw_env_constants"),
    ("domain_rand.dof_properties.*", INERT, "read by the hopper env only; LeggedRobot._process_dof_props (legged_robot.py:301-328) never looks"),
    ("domain_rand.push_robots", CONSUMED, "setup"),
    ("domain_rand.push_interval_s", CONSUMED, "setup"),
    ("domain_rand.max_push_vel_xy", CONSUMED, "setup"),
    ("domain_rand.max_push_vel", CONSUMED, "setup"),
    ("domain_rand.time_between_pushes", CONSUMED, "setup (trajectory env)"),
    ("domain_rand.randomize_rom_distance", CONSUMED, "setup (trajectory env)"),
    ("domain_rand.max_rom_dist", CONSUMED, "setup (trajectory env)"),
    ("domain_rand.zero_rom_distance_likelihood", CONSUMED, "setup (trajectory env)"),
    # ---- env
    ("env.num_envs", CONSUMED, "setup"),
    ("env.num_observations", CONSUMED, "setup (checked against the observation layout)"),
    ("env.num_privileged_obs", CONSUMED, "base: BaseTask; env: None or the width of privileged_obs.terms (privileged_obs.py); a number "
     "without terms is refused: LeggedRobot then produces none, as in the reference"),
    ("env.num_actions", CONSUMED, "setup (checked against the asset)"),
    ("env.env_spacing", CONSUMED, "env: grid origins"),
    ("env.send_timeouts", CONSUMED, "setup"),
    ("env.episode_length_s", CONSUMED, "setup"),
    # ---- init state, noise, normalisation, rewards
    ("init_state.*", CONSUMED, "setup"),
    ("noise.*", CONSUMED, "setup: noise_scale_vec"),
    ("normalization.*", CONSUMED, "setup"),
    # ---- actor observation history (this build's own section; the reference's actor sees one frame)
    ("obs_history.length", CONSUMED, "env: obs_history.ObsHistorySpec, frames in the actor's row including the current one; 1 is off"),
    ("obs_history.columns", CONSUMED, "env: obs_history.ObsHistorySpec, None or the [lo, hi) ranges of obs columns past frames keep"),
    ("obs_history.reset", CONSUMED, "env: obs_history.ObsHistorySpec, what a reset leaves in the past frames: repeat | zero"),
    # ---- privileged observations (this build's own section; the reference has the buffer, legged_robot_config.py:38, and no terms)
    ("privileged_obs.terms", CONSUMED, "env: privileged_obs.PrivilegedObsSpec, the terms of the critic's row in order (lg_priv_cfg)"),
    ("privileged_obs.scales.*", CONSUMED, "env: privileged_obs.PrivilegedObsSpec, lg_priv_term.scale of the term of that name"),
    ("rewards.scales.*", CONSUMED, "setup: reward terms"),
    ("rewards.differential_error.*", CONSUMED, "reward: declared term (trajectory env)"),
    ("rewards.reward_weighting.position", CONSUMED, "reward: tracking_rom weights (trajectory env, SingleInt2D.get_weighting_vector)"),
    ("rewards.reward_weighting.*", INERT, "weights of reduced-order models other than SingleInt2D (rom_dynamics.py:209-211 reads position only)"),
    ("rewards.*", CONSUMED, "setup"),
    # ---- trajectory generator / reduced-order model (trajectory env)
    ("rom.cls", FIXED, "SingleInt2D is the implemented reduced-order model; the reference env cannot run the others either "
     "(legged_robot_trajectory.py:279 subtracts an (N, 1, 2) offset from an (N, N_traj, n) window)", ("SingleInt2D",)),
    ("rom.dt", CONSUMED, "setup"),
    ("rom.v_min", CONSUMED, "setup"),
    ("rom.v_max", CONSUMED, "setup"),
    ("rom.*", INERT, "state bounds / curricula of other reduced-order models: SingleInt2D.clip_v_z returns v unchanged (rom_dynamics.py:201-202) "
     "and legged_robot_trajectory.py:89-103 passes nothing else"),
    ("trajectory_generator.cls", CONSUMED, "setup: lg_set_traj_generator (TrajectoryGenerator, the Zero / Square / Circle "
     "evaluation generators, and PlanTrajectoryGenerator -- this project's own class, not one of rom_dynamics.py: every env follows the "
     "plan traj_gen.set_plans gave it (tube/plan_env.py); env_setup._parse_trajectory refuses any other name)"),
    ("trajectory_generator.t_samp_cls", FIXED, "UniformSampleHoldDT is the implemented hold-time sampler", ("UniformSampleHoldDT",)),
    ("trajectory_generator.weight_samp_cls", CONSUMED, "setup: lg_set_traj_generator (UniformWeightSampler, UniformWeightSamplerNoRamp; "
     "env_setup._parse_trajectory refuses UniformWeightSamplerNoExtreme, which raises in the reference, and unknown names)"),
    ("trajectory_generator.dN", FIXED, "one ROM step per trajectory point", (1,)),
    ("trajectory_generator.DN", INERT, "the fork's misspelling of dN; nothing reads it"),
    ("trajectory_generator.seed", INERT, "seeds the numpy generator of the casadi backend; the torch backend the env uses draws from torch's "
     "global generator (rom_dynamics.py:441-470)"),
    ("trajectory_generator.*", CONSUMED, "setup"),
    # ---- sim (helpers.parse_sim_params -> gymapi.SimParams in the reference)
    ("sim.dt", CONSUMED, "sim / setup: sim_dt as a C float"),
    ("sim.substeps", CONSUMED, "setup: lg_cfg.phys_substeps"),
    ("sim.gravity", CONSUMED, "setup"),
    ("sim.up_axis", FIXED, "z is up (legged_robot.py:231 hard-codes it too)", (1,)),
    ("sim.physx.num_position_iterations", CONSUMED, "setup: lg_cfg.solver_iterations"),
    ("sim.physx.contact_offset", CONSUMED, "setup"),
    ("sim.physx.rest_offset", CONSUMED, "setup: added to asset.thickness in lg_cfg.rest_offset"),
    ("sim.physx.bounce_threshold_velocity", CONSUMED, "setup"),
    ("sim.physx.max_depenetration_velocity", CONSUMED, "setup"),
    ("sim.physx.solver_type", FIXED, "one solver (projected sweeps over positions, the role of PhysX's TGS); PGS is not implemented", (1,)),
    ("sim.physx.num_velocity_iterations", FIXED, "no separate velocity iterations", (0,)),
    ("sim.physx.contact_collection", FIXED, "net contact forces are gathered over all substeps", (2,)),
    ("sim.physx.num_threads", INERT, "PhysX CPU worker threads"),
    ("sim.physx.max_gpu_contact_pairs", INERT, "PhysX buffer capacity"),
    ("sim.physx.default_buffer_size_multiplier", INERT, "PhysX buffer capacity"),
    # ---- terrain
    ("terrain.dynamic_friction", CONSUMED, "enforce(): must equal static_friction (single-coefficient Coulomb friction); refused otherwise"),
    ("terrain.*", CONSUMED, "env / setup: utils/terrain.Terrain, lg_cfg"),
    # ---- viewer
    ("viewer.*", INERT, "camera placement; the reference reads it only when a viewer exists (legged_robot.py:238-240 under `not headless`)"),
    # ---- top-level scalars task_registry writes
    ("seed", CONSUMED, "sim: task_registry.make_env -> set_seed / Philox key"),
]


def lookup(path: str):
    """First matching row (rows are ordered from specific to general)."""
    for row in CONTRACT:
        if fnmatch.fnmatchcase(path, row[0]):
            return row
    return None


def leaves(d: dict, prefix: str = ""):
    """Leaf paths of a class_to_dict tree; dict-valued settings (joint-name maps) are leaves."""
    out = []
    for k, v in d.items():
        if isinstance(v, dict) and k not in ("default_joint_angles", "stiffness", "damping", "terrain_kwargs"):
            out += leaves(v, prefix + k + ".")
        else:
            out.append((prefix + k, v))
    return out


_warned = set()


def enforce(cfg) -> None:
    """Raise for a value the table fixes elsewhere, warn (once per process and leaf) for an accepted-but-unmodelled one, raise for a
    leaf the table does not know."""
    from legged_gym_dev_amd.utils.helpers import class_to_dict
    for path, val in leaves(class_to_dict(cfg)):
        row = lookup(path)
        if row is None:
            raise AttributeError(f"cfg.{path}: not in the configuration contract (envs/base/cfg_contract.py): decide whether it is "
                                 "consumed, inert, fixed or unmodelled before using it")
        kind = row[1]
        if kind == FIXED and val not in row[3]:
            raise NotImplementedError(f"cfg.{path} = {val!r}: {row[2]} (accepted: {', '.join(repr(v) for v in row[3])})")
        if kind == UNMODELLED and row[3](val) and path not in _warned:
            _warned.add(path)
            warnings.warn(f"cfg.{path} = {val!r}: {row[2]}", stacklevel=3)
    t = cfg.terrain
    if float(t.dynamic_friction) != float(t.static_friction):
        raise NotImplementedError(f"cfg.terrain.dynamic_friction = {t.dynamic_friction!r} != static_friction = {t.static_friction!r}: "
                                  "the contact law has one Coulomb coefficient per pair")
