"""Moving obstacles and fleets, host side: lg_plan_scenes.vel against the header and its refusal, Scenes with
velocities (validation, packing, round trips, time), random speeds, the three audits against an obstacle where it is at each node's
time, lg_plan_fleet_scenes' refusals before a device is touched, the fleet rule's restatement on a hand-made case, the separation
audit and the scripts' refusals.  No GPU."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
from legged_gym_dev_amd import capi  # noqa: E402
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402
from tests import plan_moving_ref as mr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


def test_vel_is_the_last_field_and_null_by_default():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(lg_plan_scenes),' \
          'offsetof(lg_plan_scenes,n_obs),offsetof(lg_plan_scenes,vel),sizeof(lg_fleet_cfg));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    T = capi.lg_plan_scenes
    assert out == [C.sizeof(T), T.n_obs.offset, T.vel.offset, C.sizeof(capi.lg_fleet_cfg)]
    assert T.vel.offset > T.n_obs.offset and T._fields_[-1][0] == "vel" and T().vel is None


def test_check_refuses_vel_without_obs_in_a_sentence_of_its_own(lib):
    st = capi.lg_plan_scenes()
    st.S, st.goal, st.vel = 4, 64, 64
    assert lib.lg_plan_scenes_check(C.byref(st), 4) == -1
    assert lib.lg_last_error().decode().startswith("lg_plan_scenes: vel is given without obs")
    st.obs, st.n_obs = 64, 64
    assert lib.lg_plan_scenes_check(C.byref(st), 4) == 0
    st.goal = None                                                      # the earlier sentences come first and keep their words
    st.obs = None
    assert lib.lg_plan_scenes_check(C.byref(st), 4) == -1 and "n_obs is given without obs" in lib.lg_last_error().decode()


OC, OR = np.zeros((3, 2, 2)), np.full((3, 2), 0.1)
BAD = [(dict(goal=np.zeros((3, 2)), obs_v=np.zeros((3, 2, 2))), "obs_v is given without obs_c"),
       (dict(obs_c=OC, obs_r=OR, obs_v=np.zeros((3, 2))), "obs_v must be"), (dict(obs_c=OC, obs_r=OR, obs_v=np.zeros((3, 3, 2))), "obs_v must be"),
       (dict(obs_c=OC, obs_r=OR, obs_v=np.where(np.arange(12).reshape(3, 2, 2) == 7, np.inf, 0.0)), "velocity is finite")]


@pytest.mark.parametrize("kw,word", BAD, ids=[w[:12] for _, w in BAD])
def test_velocities_are_validated(kw, word):
    with pytest.raises(ValueError, match=word):
        pl.Scenes(**kw)


def _two():
    """Two scenes of up to 3 slots: scene 0 has one live obstacle, scene 1 two; dead slots hold NaN."""
    c, r, u = np.full((2, 3, 2), np.nan), np.full((2, 3), -1.0), np.full((2, 3, 2), np.nan)
    c[0, 0], r[0, 0], u[0, 0] = [1.0, 2.0], 0.5, [0.25, -0.5]
    c[1, :2], r[1, :2], u[1, :2] = [[3.0, 4.0], [5.0, 6.0]], [0.25, 0.75], [[0.0, 0.0], [-1.0, 0.125]]
    return pl.Scenes(goal=[[0.0, 0.0], [1.0, 1.0]], obs_c=c, obs_r=r, n_obs=[1, 2], obs_v=u)


def test_packing_take_save_load_and_time(tmp_path):
    sc = _two()
    vel = sc.packed_vel()
    assert vel.shape == (2, 8, 2) and vel.dtype == np.float32 and sc.moving and not pl.Scenes(goal=sc.goal).moving
    assert vel[0, 0].tolist() == [0.25, -0.5] and vel[1, 1].tolist() == [-1.0, 0.125] and not vel[0, 1:].any() and not vel[1, 2:].any()
    assert pl.Scenes(obs_c=sc.obs_c, obs_r=sc.obs_r, n_obs=sc.n_obs).packed_vel() is None
    one = sc.take([1])
    assert one.S == 1 and one.obs_v[0, 1].tolist() == [-1.0, 0.125] and sc.take(slice(None)).obs_v.shape == (2, 3, 2)
    f = str(tmp_path / "s.npz")
    sc.save(f)
    back = pl.Scenes.load(f)
    for k in ("goal", "obs_c", "obs_r", "n_obs", "obs_v"):
        np.testing.assert_array_equal(getattr(back, k), getattr(sc, k))
    pl.Scenes(goal=sc.goal).save(f)
    assert pl.Scenes.load(f).obs_v is None and "obs_v" not in np.load(f).files
    # at(t): c + u * t in float32, the multiply and the add rounded one by one
    t = 0.3
    at = sc.at(t)
    want = (sc.obs_c[1, 1] + sc.obs_v[1, 1] * np.float32(t)).astype(np.float32)
    assert at.obs_c.dtype == np.float32 and at.obs_c[1, 1].tolist() == want.tolist() and at.obs_c[1, 0].tolist() == [3.0, 4.0]
    np.testing.assert_array_equal(at.obs_v, sc.obs_v), np.testing.assert_array_equal(at.goal, sc.goal)
    np.testing.assert_array_equal(sc.at(0.0).packed(), sc.packed())
    still = pl.Scenes(goal=sc.goal, obs_c=sc.obs_c, obs_r=sc.obs_r, n_obs=sc.n_obs)
    np.testing.assert_array_equal(still.at(5.0).packed(), still.packed())
    # obstacles(problem, t): float64 centres at one time or per node
    base = pl.PlanProblem.named("gap", tube_kind="l1", N=4)
    c0, r0, live0 = sc.obstacles(base)
    c1, r1, live1 = sc.obstacles(base, t=2.0)
    assert c1.dtype == np.float64 and c1[1, 1].tolist() == [3.0, 6.25] and c1[0, 0].tolist() == [1.5, 1.0] and (live0 == live1).all()
    cn, _, _ = sc.obstacles(base, t=np.array([0.0, 1.0, 2.0]))
    assert cn.shape == (2, 3, 3, 2) and cn[1, 2, 1].tolist() == [3.0, 6.25] and cn[1, 0, 1].tolist() == [5.0, 6.0]
    ps, _, _ = pl.Scenes(goal=sc.goal).obstacles(base, t=np.array([0.0, 1.0]))      # the problem's own obstacles stand still
    assert ps.shape == (2, 2, base.n_obs, 2) and (ps[:, 0] == ps[:, 1]).all()
    assert pl.Scenes.repeat(base, 3).obs_v is None


def test_problem_refuses_a_moving_scene():
    sc, base = _two(), pl.PlanProblem.named("gap", tube_kind="l1", N=4)
    with pytest.raises(ValueError, match=r"scene 0 has a moving obstacle.*take\(\[0\]\)"):
        sc.problem(0, base)
    zero = pl.Scenes(goal=sc.goal, obs_c=sc.obs_c, obs_r=sc.obs_r, n_obs=sc.n_obs, obs_v=np.where(np.isnan(sc.obs_v), np.nan, 0.0))
    assert zero.problem(1, base).obs_c == [[3.0, 4.0], [5.0, 6.0]]    # zero live velocities: a PlanProblem says it all


def test_random_scenes_with_and_without_speeds():
    start, kw = [0.0, 0.0], dict(n_obs=(0, 8))
    a = pl.random_scenes(64, 11, start, **kw)
    assert a.obs_v is None
    # what random_scenes(64, 11, [0, 0], n_obs=(0, 8)) drew before speeds existed (sha256 of goal, obs_c, obs_r, n_obs)
    h = hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in (a.goal, a.obs_c, a.obs_r, a.n_obs))).hexdigest()
    assert h == "79be6d855164b1f04e93cddc2285a8e853d7b9ebad234fb7c3103a0f5a6d2c7c"
    b, c = pl.random_scenes(64, 11, start, speed=(0.02, 0.08), **kw), pl.random_scenes(64, 11, start, speed=(0.02, 0.08), **kw)
    np.testing.assert_array_equal(b.obs_v, c.obs_v), np.testing.assert_array_equal(b.obs_c, c.obs_c)
    np.testing.assert_array_equal(b.obs_c[0], a.obs_c[0])             # the speeds are drawn after the scene is accepted
    live = b._live()
    sp = np.linalg.norm(b.obs_v.astype(np.float64), axis=2)
    assert live.sum() > 100 and sp[live].min() >= 0.02 - 1e-7 and sp[live].max() <= 0.08 + 1e-7 and not b.obs_v[~live].any()
    ang = np.arctan2(b.obs_v[..., 1], b.obs_v[..., 0])[live]
    assert (np.histogram(ang, bins=4, range=(-np.pi, np.pi))[0] > 0.15 * live.sum()).all(), "directions in every quadrant"
    for bad in ((-0.1, 0.2), (0.3, 0.2)):
        with pytest.raises(ValueError, match="speed"):
            pl.random_scenes(2, 0, start, speed=bad)


def _hand_made():
    """Two robots walk from (0, 0) to (1, 0) in 10 steps of dt = 0.1.  Scene 0's disc stands at (0.5, 0.3), r = 0.1, and comes down at
    0.6 m/s: it meets the walker at t = 0.5.  Scene 1's disc stands on the path at (1.0, 0.0) and leaves upwards at 2 m/s before the
    walker arrives.  Static, scene 0 is safe and scene 1 is hit; moving, the reverse."""
    base = pl.PlanProblem.named("gap", tube_kind="l1", N=10, dt=0.1, obs_c=[], obs_r=[])
    c, r = np.array([[[0.5, 0.3]], [[1.0, 0.0]]]), np.full((2, 1), 0.1)
    u = np.array([[[0.0, -0.6]], [[0.0, 2.0]]])
    pz = torch.stack([torch.linspace(0, 1, 11), torch.zeros(11)], dim=1)[None].repeat(2, 1, 1)
    return base, pl.Scenes(obs_c=c, obs_r=r), pl.Scenes(obs_c=c, obs_r=r, obs_v=u), pz


def test_the_three_audits_test_an_obstacle_where_it_is_at_each_nodes_time():
    from legged_gym_dev_amd.tube.plan_env import audit_env
    base, still, moving, pz = _hand_made()
    B, T = pz.shape[:2]
    score = {"w": torch.full((B, T), 0.2), "min_clear": torch.ones(B)}
    track = {"w_true": torch.full((B, T), 0.1), "pz_x": pz}
    a, b = pl.audit(score, track, base, scenes=still), pl.audit(score, track, base, scenes=moving)
    assert a["by_plan"]["actually_safe"] == [True, False] and b["by_plan"]["actually_safe"] == [False, True]
    res = {"z": pz, "w": torch.full((B, T), 0.2), "pz_x": pz, "min_clear": torch.ones(B, T - 1)}
    a, b = pl.audit_closed_loop(res, base, scenes=still), pl.audit_closed_loop(res, base, scenes=moving)
    assert a["by_robot"]["actually_safe"] == [True, False] and b["by_robot"]["actually_safe"] == [False, True]
    trk = {**track, "completed": torch.ones(B, dtype=torch.bool), "dead": torch.zeros(B, dtype=torch.bool)}
    a, b = audit_env(score, trk, base, scenes=still), audit_env(score, trk, base, scenes=moving)
    assert a["by_plan"]["actually_safe"] == [True, False] and b["by_plan"]["actually_safe"] == [False, True]
    # zero velocities: what the audits returned before
    zero = pl.Scenes(obs_c=still.obs_c, obs_r=still.obs_r, obs_v=np.zeros((2, 1, 2)))
    assert pl.audit(score, track, base, scenes=zero) == pl.audit(score, track, base, scenes=still)
    assert pl.audit_closed_loop(res, base, scenes=zero) == pl.audit_closed_loop(res, base, scenes=still)


def test_fleet_entry_refuses_before_a_device_is_touched(lib):
    """Junk pointers everywhere: a launch, or any read of an array, would fault; the refusal comes first.  No GPU is present here."""
    j = C.c_void_p(64)
    ok = dict(separation=0.2, sense_radius=1.0, max_neighbours=3)
    call = lambda cfg, *a: lib.lg_plan_fleet_scenes(C.byref(capi.lg_fleet_cfg(**cfg)) if cfg else None, *a)
    full = (j, j, 4, None, None, None, 0.0, j, j, j, None)
    cases = [(None, full, "cfg is null"), ({**ok, "separation": -0.1}, full, "separation"), ({**ok, "separation": float("nan")}, full, "separation"),
             ({**ok, "sense_radius": float("inf")}, full, "sense_radius"), ({**ok, "max_neighbours": 9}, full, "max_neighbours = 9"),
             ({**ok, "max_neighbours": -1}, full, "max_neighbours = -1"), (ok, (j, j, 0) + full[3:], "P = 0"),
             (ok, (None,) + full[1:], "missing array"), (ok, full[:8] + (None, j, None), "missing array"),
             (ok, (j, j, 4, j, None, None, 0.0, j, j, j, None), "static_obs and n_static"), (ok, (j, j, 4, None, None, j, 0.0, j, j, j, None), "static_obs and n_static"),
             (ok, (j, j, 4, None, j, None, 0.0, j, j, j, None), "static_vel is given without static_obs"),
             (ok, (j, j, 4, None, None, None, float("nan"), j, j, j, None), "t must be finite")]
    for cfg, args, word in cases:
        assert call(cfg, *args) == -1, word
        msg = lib.lg_last_error().decode()
        assert msg.startswith("lg_plan_fleet_scenes: ") and word in msg, (word, msg)
    for kw, word in ((dict(separation=-1.0), "separation"), (dict(sense_radius=float("nan")), "sense_radius"), (dict(max_neighbours=9), "max_neighbours = 9")):
        with pytest.raises(ValueError, match=word):
            pl.FleetCfg(**kw).check()


def test_the_fleet_rule_on_a_hand_made_fleet():
    """Five robots on a line at x = 0, 0.25, 0.25, 0.5, 1.0; sense radius 0.5, so d2 = 0.25 is seen and 0.5625 is not."""
    pos = np.array([[0.0, 0.0], [0.25, 0.0], [0.25, 0.0], [0.5, 0.0], [1.0, 0.0]], np.float32)
    vel = np.arange(10, dtype=np.float32).reshape(5, 2)
    obs, ov, n = mr.fleet_rule(0.2, 0.5, 8, pos, vel)
    assert n.tolist() == [3, 3, 3, 4, 1]
    assert obs[0, :3].tolist() == [[0.25, 0.0, np.float32(0.2)]] * 2 + [[0.5, 0.0, np.float32(0.2)]]      # ties in d2: the smaller index first
    assert ov[0, :3].tolist() == [[2.0, 3.0], [4.0, 5.0], [6.0, 7.0]] and not obs[0, 3:].any() and not ov[0, 3:].any()
    assert ov[1, :3].tolist() == [[4.0, 5.0], [0.0, 1.0], [6.0, 7.0]]    # the coincident robot (d2 = 0), then 0 before 3 at d2 = 0.0625
    assert ov[3, :4].tolist() == [[2.0, 3.0], [4.0, 5.0], [0.0, 1.0], [8.0, 9.0]] and ov[4, 0].tolist() == [6.0, 7.0]
    # the cap, the static part in front, and a robot at NaN
    assert mr.fleet_rule(0.2, 0.5, 2, pos, vel)[2].tolist() == [2, 2, 2, 2, 1] and not mr.fleet_rule(0.2, 0.5, 0, pos, vel)[2].any()
    s_obs = np.tile(np.array([1.0, 2.0, 0.3], np.float32), (5, 8, 1))
    s_vel = np.tile(np.array([0.5, -1.0], np.float32), (5, 8, 1))
    obs, ov, n = mr.fleet_rule(0.2, 0.5, 8, pos, vel, s_obs, s_vel, np.array([0, 5, 8, 7, -2]), t=0.5)
    assert n.tolist() == [3, 8, 8, 8, 1] and obs[1, 4].tolist() == [1.25, 1.5, np.float32(0.3)] and ov[1, 4].tolist() == [0.5, -1.0]
    assert ov[1, 5:].tolist() == [[4.0, 5.0], [0.0, 1.0], [6.0, 7.0]] and obs[2, 7].tolist() == [1.25, 1.5, np.float32(0.3)]
    assert ov[3, 7].tolist() == [2.0, 3.0] and obs[3, 7, 2] == np.float32(0.2)
    pos[1] = np.nan
    obs, ov, n = mr.fleet_rule(0.2, 0.5, 8, pos, vel)
    assert n.tolist() == [2, 0, 2, 3, 1] and not obs[1].any() and not np.isnan(obs).any()


def test_fleet_scenes_on_the_host_and_the_separation_audit():
    cfg = pl.FleetCfg(separation=0.2, sense_radius=1.0, max_neighbours=3)
    f = pl.FleetScenes(4, cfg)
    assert f.S == 4 and len(f) == 4 and f.moving and f.goal is None
    c, r, live = f.obstacles(None)
    assert c.shape == (4, 0, 2) and r.shape == (4, 0) and f.obstacles(None, t=np.arange(3.0))[0].shape == (4, 3, 0, 2)
    static = pl.Scenes(obs_c=np.zeros((4, 2, 2)), obs_r=np.full((4, 2), 0.1), obs_v=np.ones((4, 2, 2)))
    g = pl.FleetScenes(4, cfg, goal=np.ones((4, 2)), static=static)
    assert g.obs_v.shape == (4, 2, 2) and g.goals(None).tolist() == [[1.0, 1.0]] * 4 and g.obstacles(None, t=2.0)[0][0, 0].tolist() == [2.0, 2.0]
    for kw, word in ((dict(static=pl.Scenes(goal=np.zeros((4, 2)))), "with obstacles"), (dict(goal=np.zeros((3, 2))), "3 scenes"),
                     (dict(static=pl.Scenes(goal=np.zeros((4, 2)), obs_c=static.obs_c, obs_r=static.obs_r)), "goals")):
        with pytest.raises(ValueError, match=word):
            pl.FleetScenes(4, cfg, **kw)
    with pytest.raises(ValueError, match="take"):
        f.take([0])
    # three robots: 0 and 1 pass at 0.1 of each other at step 1, robot 2 stays 1.0 away
    pz = torch.tensor([[[0.0, 0.0], [0.5, 0.0], [1.0, 0.0]], [[1.0, 0.0], [0.5, 0.1], [0.0, 0.0]], [[0.5, 1.1], [0.5, 1.1], [0.5, 1.1]]])
    np.testing.assert_allclose(pl.fleet_separation(pz.double()).numpy(), [0.1, 0.1, 1.0], rtol=0, atol=1e-7)
    old, pl.FLEET_AUDIT_CHUNK = pl.FLEET_AUDIT_CHUNK, 2
    try:
        np.testing.assert_allclose(pl.fleet_separation(pz.double()).numpy(), [0.1, 0.1, 1.0], rtol=0, atol=1e-7)      # chunked over pairs
    finally:
        pl.FLEET_AUDIT_CHUNK = old
    base = pl.PlanProblem.named("gap", tube_kind="l1", N=4, obs_c=[], obs_r=[])
    res = {"z": pz, "w": torch.ones(3, 3), "pz_x": pz, "min_clear": torch.ones(3, 2)}
    plain = pl.audit_closed_loop(res, base)
    got = pl.audit_closed_loop(res, base, fleet=cfg)
    assert abs(got["min_separation"] - 0.1) < 1e-7 and got["collision_free"] == 1 / 3 and got["by_robot"] == {"collision_free": [False, False, True]}
    assert {k: v for k, v in got.items() if k not in ("min_separation", "collision_free", "by_robot")} == plain
    assert pl.audit_closed_loop(res, base, fleet=pl.FleetCfg(separation=0.05))["collision_free"] == 1.0
    one = pl.audit_closed_loop({k: t[:1] for k, t in res.items()}, base, fleet=cfg)
    assert one["min_separation"] is None and one["collision_free"] == 1.0


def test_script_refusals(capsys):
    import plan_tube
    base = ["--tube", "l1", "--problem", "gap"]
    for extra, word in ((["--scene_speed", "0.1,0.2"], "--scene_speed belongs to --scenes random"),
                        (["--scenes", "some.npz", "--scene_speed", "0.1,0.2"], "--scene_speed belongs to --scenes random"),
                        (["--scenes", "random", "--scene_speed", "0.3,0.2"], "--scene_speed 0.3,0.2: 0 <= LO <= HI"),
                        (["--scenes", "random", "--scene_speed", "fast"], "--scene_speed fast: LO,HI"),
                        (["--fleet", "0.2"], "--fleet belongs to --closed_loop"), (["--fleet_sense", "1.0"], "--fleet_sense belongs to --fleet"),
                        (["--closed_loop", "3", "--fleet_neighbours", "2"], "--fleet_neighbours belongs to --fleet"),
                        (["--closed_loop", "3", "--fleet", "0.2", "--fleet_neighbours", "9"], "max_neighbours = 9"),
                        (["--closed_loop", "3", "--fleet", "-0.2"], "separation"),
                        (["--closed_loop", "3", "--fleet", "0.2", "--robot"], "per-env frames")):
        with pytest.raises(SystemExit):
            plan_tube.parse_args(base + extra)
        assert word in capsys.readouterr().err, word
    a = plan_tube.parse_args(base + ["--scenes", "random", "--scene_speed", "0.02,0.08", "--closed_loop", "3", "--starts", "4", "--fleet", "0.2"])
    assert a.scene_speed == (0.02, 0.08) and (a.fleet, a.fleet_sense, a.fleet_neighbours) == (0.2, 1.0, 8)
    p = plan_tube.build_problem(a, None)
    sc, src = plan_tube.build_scenes(a, p)
    assert src["random"]["speed"] == [0.02, 0.08] and sc.obs_v is not None
    fl = plan_tube.build_fleet(a, p, sc)
    np.testing.assert_array_equal(fl.obs_v, sc.obs_v), np.testing.assert_array_equal(fl.goal, sc.goal)
    b = plan_tube.parse_args(base + ["--scenes", "random", "--starts", "4"])
    assert b.scene_speed is None and b.fleet is None and "speed" not in plan_tube.build_scenes(b, p)[1]["random"]
    lone = plan_tube.build_fleet(plan_tube.parse_args(base + ["--closed_loop", "3", "--starts", "4", "--fleet", "0.2"]), p, None)
    assert lone.goal is None and lone.obs_c.shape == (4, p.n_obs, 2) and lone.obs_v is None
