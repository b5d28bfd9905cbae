"""Inputs and drivers of the HIP-versus-oracle comparisons of tests/test_hip_env.py, shared with tests/test_env_ragged_host.py.

Every recipe is written once, for any env count: the GPU tests run it on [hip, oracle], the host tests on [oracle] alone, so both
see exactly the same seeds, clocks, actions and id lists.  The LAST handle of `envs` is the oracle: the others are glued to it
after every step.  A recipe takes a `check` callback that is called where the GPU test compares, and returns a log of what the
oracle did, from which the assert_*_events functions decide whether the case still covers what it is there for.

Env counts.  The counts the file compared at before (64 ... 256) are whole numbers of every tile; COUNTS are not:
post-step tile 16 envs; k_substeps block 16 / 8 envs (quadrupeds, 4-wave / 2-wave shape) and 32 / 16 envs (Cassie); k_reset_all and
k_traj_reset 64 envs per block; finalize_body copies byte masks as N >> 4 uint4 plus a scalar tail.  1 and 7 sit below every block
and have no uint4 part, 17 is one tile plus one env, 47 is two quadruped blocks (one Cassie block) plus 15, 65 is one reset block
plus one.  At a count of COUNTS the clocks are seeded so that env N - 1 times out; at any other count the recipes are the ones the
file has always run, value for value."""
import numpy as np

from tests import harness

COUNTS = (1, 7, 17, 47, 65)
TILE = 16                                                  # post-step tile and uint4 of byte masks

FULL_STEP_ROBOTS = ("anymal_c_flat", "anymal_c_rough", "cassie")
FULL_STEP_CASES = [(name, n) for name in FULL_STEP_ROBOTS for n in COUNTS]
SUBSTEP_CASES = [(name, z0, n) for name, z0 in (("anymal_c_flat", 0.50), ("cassie", 0.85), ("anymal_c_randomised", 0.50))
                 for n in (1, 17, 47)]
# The block shape of k_substeps that a robot does NOT take by default, against the oracle: quadrupeds run 4-wave blocks of 16 envs
# compiled for one wave per SIMD, so theirs are the 2-wave block of 8 envs and the two-per-CU build; Cassie runs 2-wave blocks of 16
# envs, so its other shape is the 4-wave block of 32 (47 = 32 + 15; there is no two-per-CU build for L = 2).
SHAPE_CASES = ([("anymal_c_flat", shape, n) for shape in ("two_waves", "two_per_cu") for n in (7, 47)]
               + [("cassie", "four_waves", n) for n in (7, 47)])
SHAPE_SWITCH = {"two_waves": ("nw", 2), "four_waves": ("nw", 4), "two_per_cu": ("occ", 2)}
RESET_IDS_CASES = [(name, n) for name in FULL_STEP_ROBOTS for n in (17, 47, 65)]
TRAJ = "anymal_c_flat_trajectory"
TRAJ_COUNTS = (1, 17, 65)

# Cassie spawns with its feet 0.1 m above the ground and random actions keep it airborne for most of four policy steps.  The ragged
# full-step cases lower every base by this much after reset_all (envs that reset afterwards respawn at the nominal height), so
# that the contact-force write-back and the contact terms of the post-step run on the ragged tile of the L = 2 kernel as well.
CASSIE_DROP = 0.10
SUBSTEP_LAST_ENV_BELOW = 0.15                              # physics-substep cases: env N - 1 starts this far below the nominal height


def ragged(n):
    return n in COUNTS


def pair_inputs(name, n=None):
    """(mk, height_samples, z, meta): mk() builds one EnvSetup of `n` envs of the fixture's task (seed 7)."""
    z, meta = harness.load_fixture(name)
    cfg = harness.make_cfg(name)
    if n:
        cfg.env.num_envs = n
        meta = dict(meta, num_envs=n)
    from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
    from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model
    cm = compile_model(resolve_model("", meta["robot"]))
    terrain = harness.FixtureTerrain(z, meta, cfg) if "const_height_samples" in z.files else None
    hs = z["const_height_samples"] if terrain else None

    def mk():
        return EnvSetup(cfg, cm, sim_dt_float(cfg.sim.dt), terrain=terrain, seed=7)
    return mk, hs, z, meta


def traj_inputs(n):
    cfg = harness.make_cfg(TRAJ)
    cfg.env.num_envs = n
    from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
    from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model
    cm = compile_model(resolve_model("", "anymal_c"))

    def mk():
        return EnvSetup(cfg, cm, sim_dt_float(cfg.sim.dt), seed=17, extra_terms=harness.extra_terms_for(cfg))
    return mk


def seed_state(envs, rng, n, A, z0, origins=None, spread=0.02):
    root = np.zeros((n, 13), np.float32)
    root[:, 2] = z0 + rng.uniform(-spread, 0.15, n)
    if origins is not None:
        root[:, :3] += origins
        root[:, :2] += rng.uniform(-2, 2, (n, 2))
    ang = rng.uniform(-0.3, 0.3, (n, 3))
    qw = np.sqrt(np.maximum(1 - (ang ** 2).sum(1) / 4, 0))
    root[:, 3:6], root[:, 6] = ang / 2, qw
    root[:, 3:7] /= np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    root[:, 7:13] = rng.uniform(-0.5, 0.5, (n, 6))
    dof = np.zeros((n, A, 2), np.float32)
    dof[..., 0] = envs[0].setup.default_dof_pos + rng.uniform(-0.2, 0.2, (n, A))
    dof[..., 1] = rng.uniform(-1, 1, (n, A))
    fr = rng.uniform(0.2, 1.2, n).astype(np.float32)
    dm = rng.uniform(-5, 5, n).astype(np.float32)
    for e in envs:
        e.set("root_states", root)
        e.set("dof_state", dof)
        e.set("friction", fr)
        e.set("base_mass_delta", dm)


def set_tiled_terrain(envs, z, meta, n):
    if meta["custom_origins"]:
        for e in envs:
            e.set("env_origins", z["const_env_origins_init"][np.arange(n) % len(z["const_env_origins_init"])])
            e.set("terrain_levels", z["const_terrain_levels_init"][np.arange(n) % len(z["const_terrain_levels_init"])])
            e.set("terrain_types", z["const_terrain_types"][np.arange(n) % len(z["const_terrain_types"])])


def _nop(*a, **k):
    pass


def events_first(make_oracle, drive, assert_events, n):
    """Before a ragged case compares anything: the recipe on a fresh oracle alone, and the events it is there for asserted."""
    if not ragged(n):
        return
    ora = make_oracle()
    try:
        assert_events(drive([ora]), n)
    finally:
        ora.close()


def episode_clocks(rng, n, head, limit):
    """Scattered episode clocks with `head` (clocks around the time-out and the command resample) in front.  At a ragged count the
    head is cut to fit and env N - 1 gets the clock `limit` - 1, which times out on the second step (a time-out is clock > limit)."""
    ep = rng.integers(0, 1000, n)
    if not ragged(n):
        ep[:len(head)] = head
        return ep
    ep[:min(n, len(head))] = head[:n]
    ep[n - 1] = limit - 1
    return ep


# ------------------------------------------------------------------------------------------------ full step, built-in Philox streams
FULL_STEP_GLUE = ("root_states", "dof_state", "lstm_h", "lstm_c", "last_dof_vel", "last_root_vel", "feet_air_time", "episode_sums")


# Policy steps of the full-step comparison, at every count.  With the clocks of episode_clocks the resets fall on steps 0, 1 and 2,
# so step 3 is the step without a reset after one with.  The strict per-entry tolerances of this comparison hold for the steps in
# which the robots come down from their spawn; from the step on in which second feet land, a contact that opens one substep apart
# moves a joint rate past them at any env count, which the comparisons made for landed robots allow for.
FULL_STEP_STEPS = 4


def drive_full_step(envs, name, n, z, meta, after_reset_all=_nop, check=_nop):
    """reset_all, scattered clocks, a push inside the window, then policy steps with random actions, glued after every step."""
    ora = envs[-1]
    rng = np.random.default_rng(5)
    A = meta["num_dofs"]
    set_tiled_terrain(envs, z, meta, n)
    for e in envs:
        if ragged(n) and meta["use_lstm"]:                  # reset_all has something to clear in every actuator-net row
            e.set("lstm_h", np.full((2, n * A, 8), 0.25, np.float32))
            e.set("lstm_c", np.full((2, n * A, 8), -0.5, np.float32))
        e.set_step_counter(0)
        e.inject(0)
        e.call("reset_all")
    after_reset_all()
    ep = episode_clocks(rng, n, [199, 499, 999, 1000, 1001, 399, 0, 1], int(ora.setup.max_episode_length))
    if ragged(n) and name == "cassie":
        root = ora.get("root_states")
        root[:, 2] -= CASSIE_DROP
        for e in envs:
            e.set("root_states", root)
    for e in envs:
        e.set("episode_length", ep)
        e.set_step_counter(748)                             # a push (751) falls inside the window
    log = {"reset": [], "time_out": [], "contacts": []}
    for t in range(FULL_STEP_STEPS):
        act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
        for e in envs:
            e.step(act)
        log["reset"].append(ora.get("reset").astype(bool))
        log["time_out"].append(ora.get("time_out").astype(bool))
        log["contacts"].append(int((np.abs(ora.get("contact_forces")).sum(-1) > 0).sum()))
        check(t)
        for e in envs[:-1]:                                 # keep the trajectories glued together (contacts amplify fp32 noise)
            for key in FULL_STEP_GLUE:
                e.set(key, ora.get(key))
    return log


def assert_reset_events(log, n):
    """What a ragged case is there for: a time-out reset, env N - 1 among the resets, and a step without any reset after a step
    with one (extras_time_outs then keeps the stale mask of the earlier step)."""
    rst, to = np.array(log["reset"]), np.array(log["time_out"])
    assert (rst & to).any(), "no time-out reset"
    assert rst[:, n - 1].any(), "env N - 1 never resets"
    per_step = rst.any(1)
    assert any(per_step[t] and not per_step[t + 1] for t in range(len(per_step) - 1)), f"no step without a reset after one with: {per_step}"
    assert to[per_step].any() and not per_step[-1], "the stale mask the last step must keep is empty, or the last step resets"


def assert_full_step_events(log, n):
    assert_reset_events(log, n)
    assert sum(log["contacts"]) > 0, "no body touched the ground"


# ------------------------------------------------------------------------------------------------ one physics substep
def drive_substeps(envs, name, z0, n, z, meta, check=_nop):
    """Six sim_dt of ABA + contact from a seeded state near the ground under constant random torques, re-synchronised every substep."""
    ora = envs[-1]
    rng = np.random.default_rng(3)
    A = meta["num_dofs"]
    if name == "anymal_c_randomised":
        mat = np.zeros((n, 4), np.float32)
        mat[:, 0], mat[:, 1], mat[:, 2] = rng.uniform(0, 1, n), rng.uniform(0, 2e-6, n), rng.uniform(0, 0.03, n)
        last = mat[n - 1].copy()
        mat[::7] = 0.0
        if ragged(n):                                       # the material row the lanes past the end read is not a row of zeros
            mat[n - 1] = last
        for e in envs:
            e.set("material", mat)
    origins = z["const_env_origins_init"][rng.integers(0, len(z["const_env_origins_init"]), n)] if meta["custom_origins"] else None
    seed_state(envs, rng, n, A, z0, origins)
    if ragged(n):                                           # env N - 1 starts below the band of the draw: the last lane pair touches
        root = ora.get("root_states")
        root[n - 1, 2] = z0 - SUBSTEP_LAST_ENV_BELOW + (origins[n - 1, 2] if origins is not None else 0.0)
        for e in envs:
            e.set("root_states", root)
    tau = rng.uniform(-20, 20, (n, A)).astype(np.float32)
    log = {"in_contact": [], "n_contact": 0}
    for step in range(6):
        for e in envs:
            e.set("torques", tau)
            e.call("simulate")
        cf_o = ora.get("contact_forces")
        log["n_contact"] += int((np.abs(cf_o).sum(-1) > 0).sum())
        log["in_contact"].append(np.abs(cf_o).reshape(n, -1).sum(1) > 0.0)
        check(step)
        for e in envs[:-1]:                                 # re-synchronise so fp32 drift does not accumulate (chaotic contacts)
            e.set("root_states", ora.get("root_states"))
            e.set("dof_state", ora.get("dof_state"))
    return log


def assert_substep_events(log, n):
    if ragged(n):
        assert np.array(log["in_contact"])[:, n - 1].any(), "env N - 1 is never in ground contact"
    else:
        assert log["n_contact"] > 100, "test state never touched the ground"


# ------------------------------------------------------------------------------------------------ reset_ids
def reset_id_list(rng, n):
    """17 random ids at the size the test always ran (96).  At a ragged count: env 0, env N - 1, one id of the last full tile,
    one of the partial tile (which at 17 and 65 envs is env N - 1 itself), and a few random ones; fewer ids than envs."""
    if not ragged(n):
        return np.array(sorted(rng.choice(n, 17, replace=False)), np.int32)
    full = n // TILE
    want = {0, n - 1, (full - 1) * TILE + 5, full * TILE + (n - full * TILE) // 2}
    want |= set(int(i) for i in rng.choice(n, 4, replace=False))
    ids = np.array(sorted(want), np.int32)
    assert len(ids) < n and ids.min() >= 0 and ids.max() == n - 1
    return ids


def drive_reset_ids_prologue(envs, name, n, z, meta):
    """reset_all, three glued policy steps, some robots walked far enough for the terrain curriculum to move them.  Returns the rng
    (the id list is drawn from it next)."""
    ora = envs[-1]
    rng = np.random.default_rng(12)
    A = meta["num_dofs"]
    set_tiled_terrain(envs, z, meta, n)
    for e in envs:
        e.set_step_counter(0)
        e.inject(0)
        e.call("reset_all")
    for t in range(3):
        act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
        for e in envs:
            e.step(act)
        for e in envs[:-1]:
            for key in FULL_STEP_GLUE + ("commands", "last_actions"):
                e.set(key, ora.get(key))
    if meta["custom_origins"]:                              # walk some robots far enough for the curriculum to move them
        root = ora.get("root_states")
        root[::5, 0] += 5.0
        for e in envs:
            e.set("root_states", root)
    return rng


# ------------------------------------------------------------------------------------------------ trajectory task
TRAJ_GLUE = ("root_states", "dof_state", "lstm_h", "lstm_c", "last_dof_vel", "last_root_vel", "feet_air_time",
             "episode_sums", "tg_state", "tg_traj", "trajectory", "prev_error", "push_timer")


def drive_trajectory(envs, n, after_reset_all=_nop, check=_nop):
    """30 policy steps of the trajectory env on its own Philox streams, clocks scattered so that generator resamples, ROM steps,
    pushes, time-outs and resets occur; glued after every step."""
    from legged_gym_dev_amd import capi
    ora = envs[-1]
    o = capi.TG_FIELDS
    rng = np.random.default_rng(6)
    tg = np.zeros((n, capi.TG_STRIDE), np.float32)
    tg[:, o["ramp_v_end"][0]:o["ramp_v_end"][0] + 2] = rng.uniform(-0.35, 0.35, (n, 2))
    pt = rng.uniform(0.0, 0.5, n).astype(np.float32)
    for e in envs:
        e.set("tg_state", tg)
        e.set("push_timer", pt)
        e.set_step_counter(0)
        e.inject(0)
        e.call("reset_all")
    after_reset_all()
    ep = episode_clocks(rng, n, [1000, 1001, 999, 3], int(ora.setup.max_episode_length))
    for e in envs:
        e.set("episode_length", ep)
    log = {"reset": [], "time_out": [], "seen": {"reset": 0, "pushed": 0, "resampled": 0, "rom": 0, "late": 0}}
    seen = log["seen"]
    for t in range(30):
        act = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        before = ora.get("tg_state").copy()
        pt_before = ora.get("push_timer").copy()
        for e in envs:
            e.step(act)
        check(t)
        go = ora.get("tg_state")
        rst = ora.get("reset").astype(bool)
        log["reset"].append(rst)
        log["time_out"].append(ora.get("time_out").astype(bool))
        seen["reset"] += int(rst.sum())
        seen["pushed"] += int((ora.get("push_timer") > pt_before).sum())
        seen["resampled"] += int(((go[:, o["t_final"][0]] != before[:, o["t_final"][0]]) & ~rst).sum())
        seen["rom"] += int(((go[:, o["k"][0]] != before[:, o["k"][0]]) & ~rst).sum())
        seen["late"] += int(rst.any()) * int((~rst).sum())  # envs the reset loop's late resample pass visits
        for e in envs[:-1]:
            for key in TRAJ_GLUE:
                e.set(key, ora.get(key))
    return log


def assert_trajectory_events(log, n):
    seen = log["seen"]
    if not ragged(n):
        assert seen["reset"] > 5 and seen["pushed"] > 20 and seen["resampled"] > 10 and seen["rom"] > 500, seen
        return
    rst, to = np.array(log["reset"]), np.array(log["time_out"])
    assert (rst & to).any() and rst[:, n - 1].any(), "env N - 1 never times out"
    per_step = rst.any(1)
    assert any(per_step[t] and not per_step[t + 1] for t in range(len(per_step) - 1)), per_step
    # the ROM steps every env every few policy steps, whatever the count; the late pass needs a second env
    assert seen["rom"] >= n and (n == 1 or seen["late"] > 0), seen
