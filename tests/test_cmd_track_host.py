"""The command tracker, the part that needs no GPU (legged_gym_dev_amd/tube/cmd_track.py, lg_cmdtrack_check; DESIGN.md section
10.16): every refusal in the same words on both sides, lg_cmdtrack_cfg / lg_cmdtrack_rec against the header, the restatement
(tests/cmd_track_ref.py) against the reference's own functions (tests/golden/cmd_track.npz, tools/gen_fixtures_cmd_track.py), the
stated ties of the law, the script's refusals, and collect / track_cmd on a stub tracker."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import cmd_track as ct
from tests import cmd_track_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    return capi.declare_cmdtrack_api(C.CDLL(L.SO_PATH))


def _rec(**kw):
    r = capi.lg_cmdtrack_rec()
    r.T, r.z, r.v, r.pz_x, r.done = 4, 64, 128, 192, 256            # never dereferenced by the check
    for k, v in kw.items():
        setattr(r, k, v)
    return r


NAN, INF = float("nan"), float("inf")
REFUSALS = [   # (cfg changes, rec changes or None for no rec, env_traj, num_obs, a word of the sentence)
    (dict(), None, True, 48, "trajectory env"),
    (dict(kind=1), None, False, 48, "kind = 1"),
    (dict(kind=5), None, False, 48, "kind = 5"),
    (dict(cmd_col=46), None, False, 48, "cmd_col = 46"),
    (dict(cmd_col=-1), None, False, 48, "cmd_col = -1"),
    (dict(cmd_col=9), None, False, 11, "num_obs = 11"),
    (dict(x_n=36), None, False, 48, "x_n = 36 must be 0 or the env's 37"),
    (dict(Kp=(1, 0, 0, 0, NAN, 0, 0, 0, 1)), None, False, 48, "Kp[4] is not finite"),
    (dict(Kp=(1, 0, 0, 0, 1, 0, 0, 0, INF)), None, False, 48, "Kp[8] is not finite"),
    (dict(u_min=(-1, 0.5, -1), u_max=(1, 0.25, 1)), None, False, 48, "u_min[1] exceeds u_max[1]"),
    (dict(u_max=(1, 1, NAN)), None, False, 48, "u_min[2] exceeds u_max[2]"),
    (dict(cmd_scale=(2, INF, 0.25)), None, False, 48, "cmd_scale[1] is not finite"),
    (dict(weight_sampler=2), None, False, 48, "weight_sampler = 2"),
    (dict(tg_N=0), None, False, 48, "tg_N = 0 must lie in 1..16"),
    (dict(tg_N=17), None, False, 48, "tg_N = 17"),
    (dict(t_low=0.0), None, False, 48, "0 < t_low <= t_high"),
    (dict(t_low=2.0, t_high=1.0), None, False, 48, "0 < t_low <= t_high"),
    (dict(rom_v_min=(-1, 0.5), rom_v_max=(1, 0.25)), None, False, 48, "rom_v_min[1] exceeds rom_v_max[1]"),
    (dict(), dict(T=0), False, 48, "T = 0 must be at least 1"),
    (dict(), dict(z=None), False, 48, "z is null"),
    (dict(), dict(v=None), False, 48, "v is null"),
    (dict(), dict(pz_x=None), False, 48, "pz_x is null"),
    (dict(), dict(done=None), False, 48, "done is null"),
    (dict(), dict(x=512), False, 48, "x is given but x_n = 0"),
]


@pytest.mark.parametrize("cfg_kw, rec_kw, env_traj, num_obs, word", REFUSALS)
def test_every_refusal_in_the_same_words_on_both_sides(lib, cfg_kw, rec_kw, env_traj, num_obs, word):
    cfg = ct.CmdTrackCfg(**cfg_kw)
    rec = None if rec_kw is None else _rec(**rec_kw)
    with pytest.raises(ValueError) as ei:
        cfg.check(env_traj, num_obs, 37, rec)
    why = str(ei.value)
    assert word in why
    st = cfg.to_struct()
    assert lib.lg_cmdtrack_check(C.byref(st), None if rec is None else C.byref(rec), int(env_traj), num_obs, 37) == -1
    assert lib.lg_last_error().decode() == "lg_cmdtrack: " + why                  # the same words


def test_the_check_passes_what_is_inside_the_envelope_and_entries_refuse_before_a_device(lib):
    for cfg, rec in ((ct.CmdTrackCfg(), None), (ct.CmdTrackCfg(kind=ct.PLAN, tg_N=0, t_low=0.0, weight_sampler=7), _rec()),
                     (ct.CmdTrackCfg(x_n=37, track_yaw=True), _rec(x=512, u=1024)), (ct.CmdTrackCfg(cmd_col=45), _rec(T=1))):
        cfg.check(False, 48, 37, rec)
        st = cfg.to_struct()
        assert lib.lg_cmdtrack_check(C.byref(st), None if rec is None else C.byref(rec), 0, 48, 37) == 0
    assert lib.lg_cmdtrack_check(None, None, 0, 48, 37) == -1 and lib.lg_last_error().decode() == "lg_cmdtrack: cfg is null"
    assert ct.refusal(None, None, False, 48, 37) == "cfg is null"
    st, out = ct.CmdTrackCfg().to_struct(), C.c_void_p()
    assert lib.lg_cmdtrack_create(None, C.byref(st), C.byref(out)) == -1 and "null argument" in lib.lg_last_error().decode()
    r = _rec()
    for fn, args in (("begin", (None, C.byref(r), 0)), ("step", (None, C.byref(r), 0)), ("set_plans", (None, None, 0))):
        assert getattr(lib, "lg_cmdtrack_" + fn)(None, *args) == -1 and "null argument" in lib.lg_last_error().decode()
    assert lib.lg_cmdtrack_destroy(None) == 0
    with pytest.raises(ValueError, match="Kp must have 9 entries"):
        ct.CmdTrackCfg(Kp=(1, 1, 1)).to_struct()


def test_structs_match_the_header():
    cf = ["kind", "track_yaw", "cmd_col", "weight_sampler", "tg_N", "x_n", "seed", "Kp", "u_min", "u_max", "cmd_scale", "rom_v_min",
          "rom_v_max", "t_low", "t_high", "freq_low", "freq_high", "prob_stationary"]
    rf = ["T", "z", "v", "pz_x", "done", "u", "x"]
    bf = ["state", "tg_state", "plan", "inject", "n_resample", "inject_overrun", "inject_K"]
    items = ["sizeof(lg_cmdtrack_cfg)", "sizeof(lg_cmdtrack_rec)", "sizeof(lg_cmdtrack_buffers)"] + \
        [f"offsetof(lg_cmdtrack_cfg,{f})" for f in cf] + [f"offsetof(lg_cmdtrack_rec,{f})" for f in rf] + \
        [f"offsetof(lg_cmdtrack_buffers,{f})" for f in bf] + ["(size_t)LG_TG_KIND_RANDOM", "(size_t)LG_TG_KIND_PLAN", "(size_t)LG_PLAN_MAX_N",
                                                             "(size_t)LG_RS_NRESET", "(size_t)LG_TG_NDRAW"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){' + \
        "".join(f'printf("%zu\\n",{it});' for it in items) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    c, r, b = capi.lg_cmdtrack_cfg, capi.lg_cmdtrack_rec, capi.lg_cmdtrack_buffers
    want = [C.sizeof(c), C.sizeof(r), C.sizeof(b)] + [getattr(c, f).offset for f in cf] + [getattr(r, f).offset for f in rf] + \
        [getattr(b, f).offset for f in bf] + [ct.RANDOM, ct.PLAN, capi.PLAN_MAX_N, capi.RS_NRESET, capi.TG_NDRAW]
    assert out == want


# ------------------------------------------------------------------------------------------------ the law
def _fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "cmd_track.npz"))
    cfg = {"kind": ref.PLAN, "Kp": z["Kp"], "u_min": z["u_min"], "u_max": z["u_max"], "cmd_scale": [1, 1, 1], "rom_dt": 0.02}
    return z, cfg


@pytest.mark.parametrize("track_yaw", [False, True])
def test_the_restatement_is_the_references_law(track_yaw):
    """64 poses through the reference's own des_pose_vel, quat2yaw (scipy's xyz Euler angles), yaw2rot, wrap_angles and its
    command lines, in float64: the float64 restatement agrees to rounding (another order of the same sums), the float32 one to
    float32 rounding of quantities of order 1..4."""
    z, cfg = _fixture()
    cfg["track_yaw"] = track_yaw
    k = f"yaw{int(track_yaw)}_"
    parts = {}
    u = ref.command(cfg, z["z"], z["v"], z["base"], np.float64, parts)
    np.testing.assert_allclose(parts["raw"], z[k + "raw"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(u, z[k + "u"], rtol=0, atol=1e-13)
    u32 = ref.command(cfg, z["z"], z["v"], z["base"], np.float32)
    assert u32.dtype == np.float32
    np.testing.assert_allclose(u32, z[k + "u"], rtol=0, atol=4e-6)
    np.testing.assert_allclose(ref.quat2yaw(z["base"][:, 3:7], np.float64), z["yaw"], rtol=0, atol=1e-13)
    # what the fixture exercises: both clips on every axis, a wrap from each side, quaternions off the unit sphere
    raw = z[k + "raw"]
    for j in range(3):
        assert (raw[:, j] < z["u_min"][j]).any() and (raw[:, j] > z["u_max"][j]).any()
        # ... and rows inside the bounds (the yaw axis under track_yaw saturates on all 64: its law is held by `raw` above)
        assert (z[k + "u"][:, j] == raw[:, j]).any() or (j == 2 and track_yaw)
    assert (z["yaw_err"] > np.pi).any() and (z["yaw_err"] < -np.pi).any()
    assert (np.abs(np.linalg.norm(z["base"][:, 3:7], axis=1) - 1) > 0.05).any()
    if track_yaw:
        assert np.abs(z[k + "err_local"][:, 2]).max() <= np.pi
    else:
        assert not z[k + "err_local"][:, 2].any()


def test_the_stated_ties():
    """wrap at +-pi is -pi from both sides, in both precisions; atan2(0, 0) = 0, so a ROM at rest asks for yaw 0."""
    for D in (np.float64, np.float32):
        pi = D(np.pi)
        assert ref.wrap(np.array([pi, -pi], D), D).tolist() == [-pi, -pi]
        assert ref.wrap(np.array([0, 1, -1], D), D).dtype == D
        np.testing.assert_allclose(ref.wrap(np.array([0, 1, -1, 4, -4], D), D), [0, 1, -1, 4 - 2 * math.pi, 2 * math.pi - 4], atol=1e-6)
    assert ((math.pi + math.pi) % (2 * math.pi)) - math.pi == -math.pi            # Python's floor mod, the stated sense
    assert np.arctan2(np.float32(0), np.float32(0)) == 0 and math.atan2(0.0, 0.0) == 0.0
    z, cfg = _fixture()
    cfg["track_yaw"] = True
    base = z["base"][:4]
    parts = {}
    ref.command(cfg, z["z"][:4], np.zeros((4, 2), np.float32), base, np.float64, parts)
    np.testing.assert_array_equal(parts["wrap_arg"], -ref.quat2yaw(base[:, 3:7], np.float64))


def test_the_restatement_records_as_the_reference_loop_does():
    """PLAN kind on hand-made roots: v is the plan and 0 past it, z integrates it, a done row restarts at the robot, pz_x is
    the robot, u[t] is the command the step consumed."""
    n, T = 3, 5
    rng = np.random.default_rng(0)
    plan = rng.uniform(-1, 1, (n, 3, 2)).astype(np.float32)
    roots = rng.uniform(-1, 1, (T + 1, n, 13)).astype(np.float32)
    roots[..., 6] += 2
    done = np.zeros((T, n), bool)
    done[2, 1] = True
    cfg = {"kind": ref.PLAN, "track_yaw": True, "Kp": np.eye(3).reshape(9), "u_min": [-9] * 3, "u_max": [9] * 3, "cmd_scale": [2, 2, 0.25],
           "rom_dt": 0.02}
    r = ref.CmdTrackRef(cfg, n, T, np.float64, plan=plan)
    r.begin(roots[0])
    for t in range(T):
        r.step(t, roots[t + 1], done[t])
    rec = r.rec
    np.testing.assert_array_equal(rec["v"][:, :3], plan)
    assert not rec["v"][:, 3:].any() and len(r.cmd) == T
    np.testing.assert_array_equal(rec["pz_x"], roots[:, :, :2].transpose(1, 0, 2))
    np.testing.assert_array_equal(rec["done"], done.T)
    for t in range(T):
        want = rec["z"][:, t] + np.float64(np.float32(0.02)) * rec["v"][:, t]
        want[done[t]] = roots[t + 1][done[t], :2]
        np.testing.assert_array_equal(rec["z"][:, t + 1], want)
        np.testing.assert_array_equal(r.cmd[t], rec["u"][:, t] * np.array([2, 2, 0.25]))


# ------------------------------------------------------------------------------------------------ the script
def test_the_script_refuses_by_name_and_by_flag():
    from legged_gym_dev_amd.scripts import collect_velocity_data as cvd
    for task in ("anymal_c_flat_trajectory", "anymal_c_rough_trajectory"):
        with pytest.raises(SystemExit, match="is a trajectory-tracking task"):
            cvd.refuse_trajectory_task(task)
        with pytest.raises(SystemExit, match="is a trajectory-tracking task"):        # before any env is made
            cvd.main(["--task", task, "--untrained"])
    with pytest.raises(SystemExit, match="not a registered task"):
        cvd.refuse_trajectory_task("no_such_task")
    env_cfg, _ = cvd.refuse_trajectory_task("anymal_c_flat")
    assert not hasattr(env_cfg, "trajectory_generator")
    assert cvd.kp_matrix([2]) == [2, 0, 0, 0, 2, 0, 0, 0, 2] and cvd.kp_matrix([1, 2, 3]) == [1, 0, 0, 0, 2, 0, 0, 0, 3]
    assert cvd.kp_matrix(range(9)) == list(range(9))
    with pytest.raises(SystemExit, match="1, 3 or 9"):
        cvd.kp_matrix([1, 2])
    own, rest = cvd.parse(["--task", "a1", "--num_envs", "8", "--steps", "5", "--Kp", "1", "2", "3", "--track_yaw", "--raw_commands",
                           "--u_min", "-1", "-2", "-3", "--rom_v_max", "0.5", "0.25"])
    assert (own.steps, own.Kp, own.track_yaw, own.raw_commands, own.u_min, own.rom_v_max) == (5, [1, 2, 3], True, True, [-1, -2, -3], [0.5, 0.25])
    assert rest == ["--task", "a1", "--num_envs", "8"]


# ------------------------------------------------------------------------------------------------ collect / track_cmd on a stub
class StubEnv:
    device = "cpu"

    def __init__(self, n, dones):
        self.num_envs, self.num_actions, self.dones, self.log, self.t = n, 2, dones, [], 0
        self.obs = torch.zeros(n, 12)
        self.root = torch.zeros(n, 2)

    def reset(self):
        self.log.append("reset")
        self.t = 0
        self.root = torch.arange(self.num_envs, dtype=torch.float32)[:, None].repeat(1, 2)

    def get_observations(self):
        return self.obs

    def step(self, a):
        self.log.append(("env", self.t))
        assert tuple(a.shape) == (self.num_envs, 2)
        self.root = self.root + 0.5
        self.done = self.dones[:, self.t]
        self.t += 1
        return self.obs, None, None, self.done, {}


class StubTracker:
    """begin / step / records of HipCommandTracker on CPU tensors: the ROM stands still at the robot's start."""

    def __init__(self, env, kind=ct.PLAN):
        self.env, self.cfg, self.plans = env, ct.CmdTrackCfg(kind=kind), None

    def set_plans(self, v):
        self.plans = v
        self.env.log.append("plans")

    def begin(self, T, epoch=0, want_u=False):
        n = self.env.num_envs
        self.env.log.append(("begin", T, epoch))
        self.rec = {"z": torch.zeros(n, T + 1, 2), "v": torch.zeros(n, T, 2), "pz_x": torch.zeros(n, T + 1, 2),
                    "done": torch.zeros(n, T, dtype=torch.bool)}
        if want_u:
            self.rec["u"] = torch.zeros(n, T, 3)
        self.rec["z"][:, 0] = self.rec["pz_x"][:, 0] = self.env.root
        self.env.obs[:, 9:12] = 1.0

    def step(self, t):
        self.env.log.append(("trk", t))
        r = self.rec
        r["done"][:, t], r["pz_x"][:, t + 1] = self.env.done, self.env.root
        r["z"][:, t + 1] = torch.where(self.env.done[:, None], self.env.root, r["z"][:, t])

    def records(self):
        return self.rec

    def close(self):
        self.env.log.append("close")


def test_collect_on_a_stub_tracker_keeps_the_order_and_the_layout():
    n, T = 3, 4
    dones = torch.zeros(n, T, dtype=torch.bool)
    dones[1, 2] = True
    env = StubEnv(n, dones)
    trk = StubTracker(env, ct.RANDOM)
    seen = []
    recs = ct.collect(env, lambda o: (seen.append(float(o[0, 9])), torch.zeros(n, 2))[1], trk, epochs=2, T=T, first_epoch=5, want_u=True)
    one = ["reset", ("begin", T, 5)] + [x for t in range(T) for x in (("env", t), ("trk", t))]
    assert env.log == one + ["reset", ("begin", T, 6)] + one[2:]
    assert seen == [1.0] * (2 * T)                                  # the policy reads the observation the tracker wrote
    assert len(recs) == 2 and sorted(recs[0]) == ["done", "pz_x", "u", "v", "z"]
    r = recs[1]
    assert all(isinstance(a, np.ndarray) for a in r.values())
    assert r["z"].shape == (n, T + 1, 2) and r["v"].shape == (n, T, 2) and r["done"].shape == (n, T) and r["done"].dtype == bool
    np.testing.assert_array_equal(r["done"], dones.numpy())
    np.testing.assert_array_equal(r["pz_x"][:, :, 0], np.arange(n)[:, None] + 0.5 * np.arange(T + 1)[None])
    dev = ct.collect(env, lambda o: torch.zeros(n, 2), trk, 1, T, to_host=False)[0]
    assert isinstance(dev["z"], torch.Tensor)


def test_track_cmd_on_a_stub_tracker_returns_tracks_keys_and_marks_resets():
    from legged_gym_dev_amd.tube import plan as P
    n, Np = 3, 4
    dones = torch.zeros(n, Np, dtype=torch.bool)
    dones[1, 2] = True
    env = StubEnv(n, dones)
    trk = StubTracker(env)
    z0 = torch.tensor([[10.0, 20.0]] * n)
    v = torch.zeros(n, Np, 2)
    out = ct.track_cmd(env, lambda o: torch.zeros(n, 2), z0, v, tracker=trk)
    assert env.log[:3] == ["reset", "plans", ("begin", Np, 0)] and "close" not in env.log      # a tracker handed in stays open
    assert {"pz_x", "w_true"} <= set(out) and tuple(out["pz_x"].shape) == (n, Np + 1, 2) and tuple(out["w_true"].shape) == (n, Np + 1)
    assert out["dead"].tolist() == [False, True, False] and out["completed"].tolist() == [True, False, True]
    assert out["rows"].tolist() == [Np + 1, 3, Np + 1]
    # the plan's frame: (world - start) + z0; the error in world coordinates
    np.testing.assert_allclose(out["pz_x"][0, :, 0], 10.0 + 0.5 * np.arange(Np + 1))
    np.testing.assert_allclose(out["z_ref"][0], z0[0].expand(Np + 1, 2))
    np.testing.assert_allclose(out["w_true"][0], 0.5 * np.arange(Np + 1) * math.sqrt(2), rtol=1e-6)
    assert float(out["w_true"][1, 3]) == 0.0                        # the reset row restarts at the robot
    prob = type("Prob", (), {"obs_c": [(100.0, 100.0)], "obs_r": [1.0]})()
    res = P.audit({"w": torch.full((n, Np + 1), 5.0), "min_clear": torch.ones(n)}, out, prob)
    assert res["plans"] == n and res["nodes"] == Np + 1 and res["coverage"] == 1.0 and res["actually_safe"] == 1.0
    for bad, msg in (((torch.zeros(n, 0, 2), z0), "Np >= 1"), ((torch.zeros(n, capi.PLAN_MAX_N + 1, 2), z0), "LG_PLAN_MAX_N"),
                     ((v, torch.zeros(n, 3)), "z0 must be")):
        with pytest.raises(ValueError, match=msg):
            ct.track_cmd(env, None, bad[1], bad[0], tracker=trk)
    with pytest.raises(ValueError, match="kind PLAN"):
        ct.track_cmd(env, None, z0, v, tracker=StubTracker(env, ct.RANDOM))
    with pytest.raises(ValueError, match="want"):
        ct.track_cmd(env, None, z0, v, tracker=trk, want=("y",))
