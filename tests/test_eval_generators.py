"""The evaluation trajectory generators of the trajectory-tracking env (trajopt/rom_dynamics.py:618-699: Zero, Square, Circle)
and UniformWeightSamplerNoRamp (deep_tube_learning/utils.py:69-79): construction and refusals on the host, replays of the
reference's own generators (tests/golden/anymal_c_flat_traj_*.npz, tools/gen_fixtures_eval_traj.py) through the HIP env, the
input laws at full size against a float64 restatement, and the evaluation script."""
import os
import subprocess
import sys

import numpy as np
import pytest

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model
from tests import harness

TRAJ = "anymal_c_flat_trajectory"
GENS = {"zero": "ZeroTrajectoryGenerator", "square": "SquareTrajectoryGenerator", "circle": "CircleTrajectoryGenerator"}
TOL = dict(rtol=2e-5, atol=2e-5)


def _setup(cfg, seed=1):
    cm = compile_model(resolve_model("", "anymal_c"))
    return EnvSetup(cfg, cm, sim_dt_float(cfg.sim.dt), seed=seed, extra_terms=harness.extra_terms_for(cfg))


def _cfg(gen=None, sampler=None, n=None):
    cfg = harness.make_cfg(TRAJ)
    if gen is not None:
        cfg.trajectory_generator.cls = gen
    if sampler is not None:
        cfg.trajectory_generator.weight_samp_cls = sampler
    if n is not None:
        cfg.env.num_envs = n
    return cfg


# ------------------------------------------------------------------------------------------------ host: configuration
@pytest.mark.parametrize("gen", sorted(GENS.values()))
def test_evaluation_generators_construct(gen):
    s = _setup(_cfg(gen))
    assert s.traj["kind"] == capi.TG_KINDS[gen] and s.traj["weight_sampler"] == 0


def test_no_ramp_weight_sampler_constructs():
    s = _setup(_cfg(sampler="UniformWeightSamplerNoRamp"))
    assert s.traj["kind"] == 0 and s.traj["weight_sampler"] == capi.TG_WEIGHT_SAMPLERS["UniformWeightSamplerNoRamp"]


def test_default_generator_is_unchanged():
    s = _setup(_cfg())
    assert (s.traj["kind"], s.traj["weight_sampler"]) == (0, 0)


@pytest.mark.parametrize("path,value,match", [
    ("trajectory_generator.weight_samp_cls", "UniformWeightSamplerNoExtreme", "TypeError"),
    ("trajectory_generator.weight_samp_cls", "SomeSampler", "not a sampler"),
    ("trajectory_generator.cls", "HelixTrajectoryGenerator", "not a generator class"),
    ("rom.cls", "DoubleInt2D", "SingleInt2D"),
    ("trajectory_generator.dN", 2, "dN"),
])
def test_what_stays_refused_says_why(path, value, match):
    cfg = _cfg()
    obj = cfg
    *parents, leaf = path.split(".")
    for p in parents:
        obj = getattr(obj, p)
    setattr(obj, leaf, value)
    with pytest.raises(NotImplementedError, match=match):
        _setup(cfg)


# ------------------------------------------------------------------------------------------------ float64 restatements
def square_v(t, v_min, v_max):
    """SquareTrajectoryGenerator.get_input_t for SingleInt2D (rom_dynamics.py:632-641), float64."""
    c1 = 2 / v_max[1]
    c2 = c1 + 1 / v_max[0]
    c3 = c2 + 2 / abs(v_min[1])
    c4 = c3 + 1 / abs(v_min[0])
    v = np.zeros(2)
    if 0 <= t < c1:
        v[1] = v_max[1] / 2
    if c1 <= t < c2:
        v[0] = v_max[0]
    if c2 <= t < c3:
        v[1] = v_min[1] / 2
    if c3 <= t < c4:
        v[0] = v_min[1]                                    # index 1, as the reference writes it
    return v


def test_square_restatement_closes_with_corners_between_rom_steps():
    """With +-1.6 m/s the corners (1.25 / 1.875 / 3.125 / 3.75 s) fall between ROM steps and the path is a closed rectangle."""
    vmin, vmax = [-1.6, -1.6], [1.6, 1.6]
    z = np.zeros(2)
    for k in range(60):
        z += 0.1 * square_v(0.1 * k, vmin, vmax)
    np.testing.assert_allclose(z, 0.0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ GPU: fixture replays
def _fixture_cfg(z, gen):
    cfg = _cfg(gen)
    cfg.rom.v_min = [float(v) for v in z["const_rom_v_min"]]
    cfg.rom.v_max = [float(v) for v in z["const_rom_v_max"]]
    return cfg


def _tg_rows(z, prefix, n):
    """harness._tg_rows + the Circle centre."""
    rows = harness._tg_rows(z, prefix, n)
    if prefix + "tg_center" in z.files:
        rows[:, capi.TG_CENTER:capi.TG_CENTER + 2] = z[prefix + "tg_center"]
    return rows


def replay_eval_fixture(env, z, meta):
    """harness.replay_trajectory_fixture for the evaluation generators: the same teacher forcing and tolerances, the generator
    state compared with its Circle centre; the event census of the random generator (resamples) does not apply."""
    N = meta["num_envs"]
    names = meta["reward_names"]
    ridx = [env.setup.term_row[n] for n in names]
    for key in ("root_states", "dof_state", "last_actions", "last_dof_vel", "last_root_vel", "feet_air_time", "env_origins",
                "prev_error", "trajectory", "lstm_h", "lstm_c"):
        env.set(key, z["init_" + key])
    env.set("last_contacts", z["init_last_contacts"].astype(np.uint8))
    env.set("episode_length", z["init_episode_length_buf"])
    env.set("push_timer", z["init_time_until_next_push"])
    env.set("tg_state", _tg_rows(z, "init_", N))
    env.set("tg_traj", z["init_tg_traj"])
    es = np.zeros((capi.NUM_TERMS, N), np.float32)
    for k, n in enumerate(names):
        es[env.setup.term_row[n]] = z["init_episode_sums"][:, k]
    env.set("episode_sums", es)
    counter = int(z["init_common_step_counter"])
    env.set_step_counter(counter)
    env.set_init_done(1)
    env.inject(1)
    dec = z["s0_sub_dof"].shape[0]
    seen = {"reset": 0, "rom_steps": 0, "partial_reset_steps": 0}
    for t in range(meta["n_steps"]):
        p = f"s{t}_"
        env.set("episode_length", z[p + "pre_episode_length_buf"])
        env.set_actions(z[p + "actions"])
        for k in range(dec):
            env.call("compute_torques")
            env.set("dof_state", z[p + "sub_dof"][k])
        env.set("root_states", z[p + "new_root"])
        env.set("contact_forces", z[p + "contact_forces"])
        env.set("inject_uniforms", np.nan_to_num(z[p + "uniforms"], nan=0.5))
        k_before = env.get("tg_state")[:, capi.TG_FIELDS["k"][0]].copy()
        env.call("post_physics_step")
        env.sync()
        rst = z[p + "reset"].astype(bool)
        np.testing.assert_array_equal(env.get("reset").astype(bool), rst, err_msg=p + "reset")
        np.testing.assert_array_equal(env.get("time_out").astype(bool), z[p + "time_out"], err_msg=p + "time_out")
        np.testing.assert_array_equal(env.get("episode_length"), z[p + "post_episode_length_buf"], err_msg=p + "ep_len")
        assert int(env.get("n_reset")[0]) == int(z[p + "n_reset"]), p + "n_reset"
        want, got = _tg_rows(z, p + "post_", N), env.get("tg_state")
        for name in ("k", "stationary"):
            o = capi.TG_FIELDS[name][0]
            np.testing.assert_array_equal(got[:, o], want[:, o], err_msg=p + "generator " + name)
        np.testing.assert_allclose(got, want, err_msg=p + "generator state", **TOL)
        for key, ref, tol in (("tg_traj", z[p + "post_tg_traj"], TOL), ("trajectory", z[p + "post_trajectory"], TOL),
                              ("prev_error", z[p + "post_prev_error"], dict(rtol=2e-4, atol=2e-4)),
                              ("obs", z[p + "obs"], TOL), ("rew", z[p + "rew"], TOL),
                              ("push_timer", z[p + "post_time_until_next_push"], TOL)):
            np.testing.assert_allclose(env.get(key), np.asarray(ref).reshape(env.get(key).shape), err_msg=p + key, **tol)
        es = env.get("episode_sums")[ridx].T
        np.testing.assert_allclose(es, z[p + "post_episode_sums"], err_msg=p + "episode_sums (tracking_rom, differential_error ...)",
                                   **TOL)
        if rst.any():
            np.testing.assert_allclose(env.get("extras_episode")[ridx], z[p + "extras_episode"], rtol=1e-4, atol=1e-5,
                                       err_msg=p + "extras episode means")
        seen["reset"] += int(rst.sum())
        seen["rom_steps"] += int(((want[:, capi.TG_FIELDS["k"][0]] != k_before) & ~rst).sum())
        seen["partial_reset_steps"] += int(0 < rst.sum() < N)
    assert seen["reset"] > 20 and seen["rom_steps"] > 40 and seen["partial_reset_steps"] >= 3, seen
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(GENS))
def test_hip_replays_reference_evaluation_generator(which):
    """The reference's Zero / Square / Circle generator in its own env (tests/golden/anymal_c_flat_traj_<which>.npz): ROM window,
    interpolated trajectory, v, stationary flag, Circle centre (re-centred for EVERY env on a step where some env resets),
    observations, tracking_rom / differential_error, resets."""
    z, meta = harness.load_fixture(f"anymal_c_flat_traj_{which}")
    setup = _setup(_fixture_cfg(z, GENS[which]))
    env = harness.HipHandle(setup)
    try:
        replay_eval_fixture(env, z, meta)
        if which == "square":                               # corners turned inside the recorded steps
            vs = set()
            for t in range(meta["n_steps"]):
                vs |= {tuple(r) for r in z[f"s{t}_post_tg_v"][~z[f"s{t}_reset"].astype(bool)].tolist()}
            assert len(vs - {(0.0, 0.0)}) >= 3, vs
        if which == "circle":                               # the fixture pins the re-centring of non-reset envs
            moved = 0
            for t in range(meta["n_steps"]):
                pre = z["init_tg_center"] if t == 0 else z[f"s{t - 1}_post_tg_center"]
                moved += int(((z[f"s{t}_post_tg_center"] != pre).any(1) & ~z[f"s{t}_reset"].astype(bool)).sum())
            assert moved > 50
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ GPU: full size
def _run_no_reset(env, n_steps, record=None):
    """post_physics_step with zero contact forces and short episodes: the generator and ROM run, no env resets."""
    n = env.setup.num_envs
    nb = env.get("contact_forces").shape
    for s in range(n_steps):
        env.set("contact_forces", np.zeros(nb, np.float32))
        env.set("episode_length", np.zeros(n, np.int64))
        env.call("post_physics_step")
        if record is not None:
            record(s)
    env.sync()
    assert int(env.get("n_reset")[0]) == 0


@pytest.mark.gpu
def test_square_path_at_full_size_against_float64():
    """4096 envs: the ROM path of Square is the discrete sum of rom_dt v(t_k) over the ROM steps, and it closes (the corners
    sit between ROM steps with +-1.6 m/s)."""
    n, vmin, vmax = 4096, [-1.6, -1.6], [1.6, 1.6]
    cfg = _cfg(GENS["square"], n=n)
    cfg.rom.v_min, cfg.rom.v_max = vmin, vmax
    env = harness.HipHandle(_setup(cfg, seed=3))
    try:
        env.set_step_counter(0)
        env.call("reset_all")
        env.sync()
        z0 = env.get("tg_traj")[:, -1, :].astype(np.float64)
        np.testing.assert_array_equal(env.get("tg_traj"), np.repeat(env.get("tg_traj")[:, -1:, :], 11, 1))  # t < 0: v = 0
        ot, ok = capi.TG_FIELDS["t"][0], capi.TG_FIELDS["k"][0]
        tk = []
        state = {"t": float(env.get("tg_state")[0, ot]), "k": float(env.get("tg_state")[0, ok])}

        def rec(s):
            g = env.get("tg_state")
            assert np.all(g[:, ot] == g[0, ot]) and np.all(g[:, ok] == g[0, ok])
            if g[0, ok] != state["k"]:
                tk.append(state["t"])                       # the ROM step of this env step used the time before the advance
            state["t"], state["k"] = float(g[0, ot]), float(g[0, ok])
        _run_no_reset(env, 200, rec)
        assert len(tk) == 40
        v = np.stack([square_v(t, vmin, vmax) for t in tk])
        path = z0[:, None, :] + np.cumsum(0.1 * v, 0)[None]               # (n, 40, 2)
        # 1e-4, plus the rounding of 40 fp32 additions at the magnitude of the env origins (a 64 x 64 grid of 3 m)
        tol = 1e-4 + 40 * float(np.spacing(np.float32(np.abs(z0).max())))
        np.testing.assert_allclose(env.get("tg_traj")[:, 1:, :], path[:, -10:, :], rtol=0, atol=tol)
        np.testing.assert_allclose(env.get("tg_traj")[:, -1, :], z0, rtol=0, atol=tol)      # back at the start
        assert np.abs(v).sum(0).min() > 0 and len({tuple(r) for r in v}) == 5               # all four legs + the stop
    finally:
        env.close()


@pytest.mark.gpu
def test_circle_and_zero_at_full_size():
    """4096 envs: every Circle ROM step has length rom_dt * min(min(v_max, |v_min|)) and the centre is the start point - (0.5, 0);
    Zero keeps the window on the start point; reset(z) (lg_traj_reset) restarts both at z."""
    n = 4096
    for which in ("circle", "zero"):
        env = harness.HipHandle(_setup(_cfg(GENS[which], n=n), seed=5))
        try:
            env.set_step_counter(0)
            env.call("reset_all")
            env.sync()
            z0 = env.get("tg_traj")[:, 0, :].copy()                # the start point: the oldest point after the reset loop
            _run_no_reset(env, 60)
            w = env.get("tg_traj").astype(np.float64)
            g = env.get("tg_state")
            if which == "circle":
                np.testing.assert_allclose(g[:, capi.TG_CENTER:capi.TG_CENTER + 2], z0 - np.float32([0.5, 0.0]), rtol=0, atol=1e-6)
                step = np.linalg.norm(np.diff(w, axis=1), axis=-1)        # fp32: one rounding of each point's coordinates
                np.testing.assert_allclose(step, 0.1 * 0.35, rtol=1e-5, atol=2 * float(np.spacing(np.float32(np.abs(w).max()))))
            else:
                np.testing.assert_array_equal(w, np.repeat(z0[:, None, :], 11, 1))
                assert np.all(g[:, capi.TG_FIELDS["stationary"][0]] == 1.0) and np.all(g[:, capi.TG_FIELDS["v"][0]:][:, :2] == 0)
            import torch
            zr = torch.tensor(np.random.default_rng(1).uniform(-3, 3, (n, 2)), dtype=torch.float32, device="cuda")
            import ctypes as C
            env.call("traj_reset", C.c_void_p(zr.data_ptr()))
            env.sync()
            w, g, zz = env.get("tg_traj"), env.get("tg_state"), zr.cpu().numpy()
            np.testing.assert_array_equal(w[:, 0, :], zz)                               # the oldest point is z
            np.testing.assert_array_equal(g[:, capi.TG_FIELDS["k"][0]], 0.0)
            if which == "circle":
                np.testing.assert_array_equal(g[:, capi.TG_CENTER:capi.TG_CENTER + 2], zz - np.float32([0.5, 0.0]))
            else:
                np.testing.assert_array_equal(w, np.repeat(zz[:, None, :], 11, 1))
        finally:
            env.close()


@pytest.mark.gpu
def test_no_ramp_sampler_zeroes_the_ramp_weight():
    """TrajectoryGenerator with UniformWeightSamplerNoRamp, 4096 envs: after the reset's resample the ramp weight is 0 and the
    weights still sum to 1; the default sampler keeps it."""
    n = 4096
    ow = capi.TG_FIELDS["weights"][0]
    for sampler, zero in (("UniformWeightSamplerNoRamp", True), ("UniformWeightSampler", False)):
        env = harness.HipHandle(_setup(_cfg(sampler=sampler, n=n), seed=7))
        try:
            env.set_step_counter(0)
            env.call("reset_all")
            env.sync()
            w = env.get("tg_state")[:, ow:ow + 4]
            np.testing.assert_allclose(w.sum(1), 1.0, rtol=0, atol=1e-6)
            assert np.all(w[:, 1] == 0.0) == zero and np.all(w >= 0)
        finally:
            env.close()


# ------------------------------------------------------------------------------------------------ GPU: evaluation script
@pytest.mark.gpu
def test_evaluation_script_square(tmp_path):
    """scripts/evaluate_tracking.py --traj_cls square on a fresh policy, 2 envs x 300 steps, in a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "eval.npz"
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(root, "legged_gym_dev_amd", "scripts", "evaluate_tracking.py"),
                        "--traj_cls", "square", "--num_envs", "2", "--steps", "300", "--headless", "--out", str(out),
                        "--experiment_name", "eval_test_no_such_run"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rms" in r.stdout
    d = np.load(out)
    x, z, pz = d["x"], d["z"], d["pz_x"]
    assert x.shape == (301, 2, 13 + 24) and z.shape == (301, 2, 2) and pz.shape == (301, 2, 2)
    np.testing.assert_array_equal(z[0], pz[0])
    # the oldest window point moves by 0 or by rom_dt v of a Square leg (rom bounds +-0.35), except where an env restarts
    legs = np.array([[0, 0], [0, 0.0175], [0.035, 0], [0, -0.0175], [-0.035, 0]])
    dz = np.diff(z[:300], axis=0)                                          # rows 0..299 are recorded
    jump = np.linalg.norm(dz, axis=-1) > 0.05
    d_leg = np.min(np.linalg.norm(dz[..., None, :] - legs[None, None], axis=-1), axis=-1)
    ok = d_leg < 1e-5
    assert np.mean(ok | jump) > 0.97, (np.mean(ok | jump), d_leg.max())
    assert np.sum(np.abs(dz[..., 1] - 0.0175) < 1e-5) >= 20                # it walks the first leg (+y)
