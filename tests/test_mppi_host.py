"""The sampling planner, the part that needs no GPU (legged_gym_dev_amd/tube/plan.py, lg_mppi_check): every
refusal with the field named, on both sides and in the same words; lg_mppi_cfg against the header; the restatement's update
(tests/mppi_ref.py) by hand; the bookkeeping of closed_loop on a stub planner and a stub tracker; the NumPy MPPI on the fixed
small problem; the script's argument refusals."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

from tests import mppi_ref, plan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
from legged_gym_dev_amd import capi  # noqa: E402
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


# (changes to a valid configuration, P, the words the message must hold)
BAD = [(dict(K=0), 1, "K = 0"), (dict(K=31), 1, "K = 31"), (dict(K=48), 1, "K = 48"), (dict(K=4128), 1, "K = 4128"),
       (dict(iters=0), 1, "iters = 0"), (dict(sigma=0.0), 1, "sigma must be positive"), (dict(sigma=-1.0), 1, "sigma must be positive"),
       (dict(sigma_decay=0.0), 1, "sigma_decay"), (dict(sigma_decay=1.5), 1, "sigma_decay"), (dict(lambda_=0.0), 1, "lambda"),
       (dict(lambda_=float("nan")), 1, "lambda"), (dict(rho_g=-1.0), 1, "rho_g"), (dict(rho_w=-1.0), 1, "rho_w"),
       (dict(rho_z=-1e-3), 1, "rho_z"), (dict(), 0, "P = 0"), (dict(K=4096), 2 ** 19, "P * K = 2147483648")]


@pytest.mark.parametrize("change,P,word", BAD, ids=[f"{(list(c) or ['P'])[0]}-{i}" for i, (c, _, _) in enumerate(BAD)])
def test_refusals_name_the_field_on_both_sides(lib, change, P, word):
    cfg = pl.MppiCfg(**{"K": 64, **change})
    with pytest.raises(ValueError) as ei:
        cfg.check(P)
    assert word in str(ei.value)
    prob = pl.PlanProblem.named("gap", tube_kind="l1", N=5).to_struct()
    assert lib.lg_mppi_check(C.byref(cfg.to_struct()), C.byref(prob), None, 0, P) == -1
    assert lib.lg_last_error().decode() == "lg_mppi: " + str(ei.value)            # the same words


def test_valid_configurations_pass_and_the_problem_is_checked_first(lib):
    prob = pl.PlanProblem.named("gap", tube_kind="l1", N=5)
    for K in (32, 96, 4096):
        cfg = pl.MppiCfg(K=K, iters=1, sigma_decay=1.0, rho_g=0.0)
        cfg.check(3)
        assert lib.lg_mppi_check(C.byref(cfg.to_struct()), C.byref(prob.to_struct()), None, 0, 3) == 0
    cfg = pl.MppiCfg(K=64)
    for change, word in ((dict(N=0), "N"), (dict(dt=0.0), "dt"), (dict(tube_kind="nn"), "handle")):
        st = pl.PlanProblem.named("gap", **{"tube_kind": "l1", "N": 5, **change}).to_struct()
        assert lib.lg_mppi_check(C.byref(cfg.to_struct()), C.byref(st), None, 0, 1) == -1
        assert lib.lg_last_error().decode().startswith("lg_plan: ") and word in lib.lg_last_error().decode()
    assert lib.lg_mppi_check(C.byref(cfg.to_struct()), C.byref(prob.to_struct()), None, 1, 1) == -1 and "level" in lib.lg_last_error().decode()
    # the entries refuse before they touch a device
    one = C.byref(capi.lg_plan_call(count=1))
    assert lib.lg_plan_mppi(None, C.byref(prob.to_struct()), C.byref(pl.MppiCfg(K=33).to_struct()), one, *([None] * 6)) == -1
    assert "K = 33" in lib.lg_last_error().decode()
    assert lib.lg_plan_mppi_step(None, C.byref(prob.to_struct()), C.byref(cfg.to_struct()), one, 0, 0, 0, *([None] * 9)) == -1
    assert "what" in lib.lg_last_error().decode()
    assert lib.lg_plan_mppi_step(None, C.byref(prob.to_struct()), C.byref(cfg.to_struct()), one, 0, 3, 0, *([None] * 9)) == -1
    assert "missing array" in lib.lg_last_error().decode()
    assert lib.lg_plan_mppi_candidates(C.byref(prob.to_struct()), C.byref(cfg.to_struct()), 0, None, 1, None, None) == -1
    assert "missing array" in lib.lg_last_error().decode()


def test_struct_matches_the_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %d\\n",sizeof(lg_mppi_cfg),' \
          'offsetof(lg_mppi_cfg,seed),offsetof(lg_mppi_cfg,instance_offset),offsetof(lg_mppi_cfg,sigma),offsetof(lg_mppi_cfg,rho_z),' \
          'LG_MPPI_MAX_K);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    c = capi.lg_mppi_cfg
    assert out == [C.sizeof(c), c.seed.offset, c.instance_offset.offset, c.sigma.offset, c.rho_z.offset, capi.MPPI_MAX_K]
    st = pl.MppiCfg(K=96, iters=7, seed=2 ** 40 + 5, instance_offset=9, sigma=0.25, sigma_decay=0.5, lambda_=2.0, rho_g=3.0, rho_w=4.0,
                    rho_z=5.0).to_struct()
    assert (st.K, st.iters, st.seed, st.instance_offset) == (96, 7, 2 ** 40 + 5, 9)
    assert (st.sigma, st.sigma_decay, st.lambda_, st.rho_g, st.rho_w, st.rho_z) == (0.25, 0.5, 2.0, 3.0, 4.0, 5.0)
    assert pl.MppiCfg(sigma=0.3, sigma_decay=0.9).sigma_it(2) == np.float32(np.float32(np.float32(0.3) * np.float32(0.9)) * np.float32(0.9))
    assert mppi_ref.sigma_it(0.3, 0.9, 2) == pl.MppiCfg(sigma=0.3, sigma_decay=0.9).sigma_it(2)


def test_restatement_update_by_hand():
    # three candidates of one node; J = (1, 1 + ln 2, inf): weights 1, 1/2, 0
    cand = np.array([[[1.0, 0.0]], [[4.0, 3.0]], [[100.0, 100.0]]])
    J = np.array([1.0, 1.0 + np.log(2.0), np.inf])
    w, Jmin, idx = mppi_ref.weights(J, 1.0, np.float64)
    np.testing.assert_allclose(w, [1.0, 0.5, 0.0], rtol=1e-15)
    assert Jmin == 1.0 and idx == 0
    np.testing.assert_allclose(mppi_ref.update(cand, J, 1.0, np.float64), [[(1 + 2) / 1.5, 1.5 / 1.5]], rtol=1e-15)
    np.testing.assert_allclose(mppi_ref.update(cand, J, 1.0, np.float32), [[2.0, 1.0]], rtol=1e-6)
    # lambda scales the exponent; nan counts as inf; the first of two equal minima is the arg-min
    w, Jmin, idx = mppi_ref.weights(np.array([np.nan, 3.0, 3.0, 5.0]), 2.0, np.float64)
    np.testing.assert_allclose(w, [0.0, 1.0, 1.0, np.exp(-1.0)], rtol=1e-15)
    assert Jmin == 3.0 and idx == 1
    assert mppi_ref.update(cand, np.array([np.inf, np.nan, -np.inf]), 1.0) is None
    assert mppi_ref.weights(np.array([np.inf, np.nan]), 1.0)[2] == -1
    # the summation order: chunks of 64, then a tree -- in float64 any order gives the sum of small integers exactly
    x = np.arange(200, dtype=np.float64)
    assert mppi_ref.chunk_sum(x, np.float64) == x.sum() and mppi_ref.chunk_sum(x[:32], np.float32) == x[:32].sum()
    # float32: chunk 0 holds 2^24 + 1 -> 2^24, the others 1 each; the tree's first level adds chunk 32's 1 to it and loses that too
    big = np.array([2.0 ** 24] + [1.0] * 64, np.float32)
    assert mppi_ref.chunk_sum(big, np.float32) == np.float32(2.0 ** 24 + 62) and mppi_ref.chunk_sum(big, np.float64) == 2.0 ** 24 + 64
    # J and the elite
    assert mppi_ref.total(np.array([1.0]), np.array([[2.0, 3.0, 4.0]]), [10.0, 100.0, 1000.0], np.float64)[0] == 4321.0
    bJ, bv = mppi_ref.elite(np.float32(9.0), np.zeros((1, 2)), np.array([5.0, 4.0, 4.0], np.float32), cand, cand[0], False)
    assert bJ == 4.0 and (bv == cand[1]).all()
    bJ, bv = mppi_ref.elite(np.float32(3.0), np.zeros((1, 2)), np.array([5.0, 4.0, 4.0], np.float32), cand, cand[0], False)
    assert bJ == 3.0 and (bv == 0).all()
    bJ, bv = mppi_ref.elite(np.float32(3.0), np.zeros((1, 2)), np.array([5.0, 4.0, 4.0], np.float32), cand, cand[0], True)
    assert bJ == 4.0 and (bv == cand[1]).all()


def test_restatement_penalties_by_hand():
    p = {"w_max": 0.5, "rom_z_min": [0.0, -1.0], "rom_z_max": [1.0, 1.0]}
    res = {"z": np.array([[[0.5, 0.0], [1.25, -1.5], [-0.25, 2.0]]]), "w": np.array([[0.0, 0.75, 1.0]]),
           "g": np.array([[[1.0, -0.5], [-0.25, 2.0], [0.0, -1.0]]])}
    np.testing.assert_array_equal(mppi_ref.penalties(p, res, np.float64), [[0.5 + 0.25 + 1.0, 0.25 + 0.5, 0.25 + 0.5 + 0.25 + 1.0]])
    np.testing.assert_array_equal(mppi_ref.penalties(p, res, np.float32), [[1.75, 0.75, 2.0]])


SMALL = dict(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l2", scaling=0.02, Q=[10.0, 0, 0, 10.0],
             R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])


def _small_ref():
    p = pl.PlanProblem(**SMALL)
    d = p.to_json()
    d["Qf"] = d["Q"]
    v0 = np.clip(pl.warm_start("interpolate", p.start, p.goal, p.N, p.dt)[1], -2.0, 2.0)
    return p, d, v0


def test_the_small_problem_is_solved_by_a_numpy_mppi():
    """The fixed problem of the GPU test: the clipped warm start cuts the obstacle (min_clear -0.0310, J 661.2); MPPI on
    plan_ref.score with NumPy's generator clears it and brings J below a tenth, in float32 and float64."""
    p, d, v0 = _small_ref()
    rho = [1e4, 0.0, 0.0]
    res, _, J0 = mppi_ref.score_J(d, p.start, v0[None], rho, np.float64)
    assert res["min_clear"][0] == pytest.approx(-0.0310, abs=5e-5) and J0[0] == pytest.approx(661.2, abs=0.05)
    for D, seed in ((np.float64, 0), (np.float32, 1)):
        v = mppi_ref.mppi(d, p.start, v0, 256, 20, 0.3, 1.0, 1.0, rho, seed, D)
        res, _, J = mppi_ref.score_J(d, p.start, v[None].astype(np.float32), rho, np.float64)
        print(f"{D.__name__} seed {seed}: min_clear {res['min_clear'][0]:.4f}, J {J[0]:.2f}")
        assert res["min_clear"][0] >= 0 and J[0] <= 0.1 * J0[0] and res["n_viol"][0, 0] == 0


class _StubPlanner:
    """plan() returns a plan that is a known function of its arguments, and records them."""

    def __init__(self, N, Hr):
        self.problem = types.SimpleNamespace(N=N, H_rev=Hr, dt=0.5)
        self.device = torch.device("cpu")
        self.calls = []

    def plan(self, z0, v_init=None, e=None, v_prev=None, w0=None, iters=None):
        P, N = z0.shape[0], self.problem.N
        n = len(self.calls)
        self.calls.append({"z0": z0.clone(), "v_init": None if v_init is None else v_init.clone(), "e": e.clone(), "v_prev": v_prev.clone(),
                           "w0": w0, "iters": iters})
        v = (torch.zeros(P, N, 2) if v_init is None else v_init) + (n + 1) * torch.arange(1, N + 1, dtype=torch.float32)[None, :, None]
        z = torch.cat([z0[:, None], z0[:, None] + 0.5 * torch.cumsum(v, dim=1)], dim=1)
        w = 0.01 * (n + 1) * torch.arange(N + 1, dtype=torch.float32)[None].repeat(P, 1)
        return {"v": v, "best_J": torch.full((P,), float(n)), "n_bad": torch.zeros(P, dtype=torch.int32),
                "score": {"z": z, "w": w, "cost": torch.full((P,), 10.0 * n), "min_clear": torch.full((P,), 1.0 - n)}}


def _stub_track(sim, z, v, x0, rom_dt=None, want=("x", "u")):
    """x[:, 1] = (x0 position + 0.1, the feed-forward); two actions per node."""
    assert tuple(z.shape[1:]) == (2, 2) and tuple(v.shape[1:]) == (1, 2) and rom_dt == 0.5
    _stub_track.seen.append((z.clone(), v.clone(), x0.clone()))
    x1 = torch.cat([x0[:, :2] + 0.1, v[:, 0]], dim=1)
    return {"x": torch.stack([x0, x1], dim=1), "u": torch.stack([v[:, 0], -v[:, 0]], dim=1)}


@pytest.mark.parametrize("Hr", [0, 2])
def test_closed_loop_bookkeeping_on_stubs(Hr):
    N, H, P = 3, 3, 2
    pln = _StubPlanner(N, Hr)
    _stub_track.seen = []
    start = torch.tensor([[0.0, 0.0], [1.0, -1.0]])
    out = pl.closed_loop(pln, None, H, start, iters_first=7, keep_plans=True, track_fn=_stub_track)
    assert [c["iters"] for c in pln.calls] == [7, None, None] and pln.calls[0]["v_init"] is None       # H plans, none after the last step
    assert {k: tuple(t.shape) for k, t in out.items()} == {
        "z": (P, H + 1, 2), "v": (P, H, 2), "w": (P, H + 1), "pz_x": (P, H + 1, 2), "x": (P, H + 1, 4), "u": (P, 2 * H, 2), "cost": (P, H),
        "min_clear": (P, H), "best_J": (P, H), "n_bad": (P, H), "plans_v": (H, P, N, 2), "plans_z": (H, P, N + 1, 2), "plans_w": (H, P, N + 1)}
    assert torch.equal(out["z"][:, 0], start) and torch.equal(out["x"][:, 0], torch.cat([start, torch.zeros(P, 2)], 1))
    assert torch.equal(out["w"][:, 0], torch.zeros(P)) and torch.equal(out["pz_x"][:, 0], start)
    e, vp = torch.zeros(P, Hr), torch.zeros(P, Hr, 2)
    for k in range(H):
        vs, zs, ws = out["plans_v"][k], out["plans_z"][k], out["plans_w"][k]
        zt, ff, x0 = _stub_track.seen[k]
        assert torch.equal(zt, zs[:, :2]) and torch.equal(ff[:, 0], vs[:, 1]) and torch.equal(x0, out["x"][:, k])   # z_sol[0..1], v_sol[1]
        assert torch.equal(out["v"][:, k], vs[:, 0]) and torch.equal(out["z"][:, k + 1], zs[:, 1]) and torch.equal(out["w"][:, k + 1], ws[:, 1])
        assert torch.equal(out["pz_x"][:, k + 1], out["x"][:, k + 1, :2]) and torch.equal(out["x"][:, k + 1, 2:], vs[:, 1])
        assert torch.equal(out["u"][:, 2 * k], vs[:, 1]) and torch.equal(out["cost"][:, k], torch.full((P,), 10.0 * k))
        c = pln.calls[k]
        assert torch.equal(c["z0"], out["z"][:, k]) and torch.equal(c["e"], e) and torch.equal(c["v_prev"], vp) and c["w0"] is None
        if k:
            prev = out["plans_v"][k - 1]
            assert torch.equal(c["v_init"], torch.cat([prev[:, 1:], prev[:, -1:]], 1))                 # shifted, the last row repeated
        err = torch.linalg.vector_norm(out["z"][:, k] - out["pz_x"][:, k], dim=1)
        if Hr:                                                                                         # a true shift of both
            e, vp = torch.cat([e[:, 1:], err[:, None]], 1), torch.cat([vp[:, 1:], out["v"][:, k][:, None]], 1)
    if Hr:
        ne, nv = mppi_ref.shift_past(np.zeros((P, Hr)), np.zeros((P, Hr, 2)), np.ones(P), np.full((P, 2), 2.0))
        assert ne.tolist() == [[0.0, 1.0]] * P and nv[:, -1].tolist() == [[2.0, 2.0]] * P and (nv[:, 0] == 0).all()
    assert mppi_ref.shift_plan(np.arange(6.0).reshape(1, 3, 2)).tolist() == [[[2.0, 3.0], [4.0, 5.0], [4.0, 5.0]]]
    assert torch.equal(pl.shift_plan(torch.arange(6.0).reshape(1, 3, 2)), torch.tensor([[[2.0, 3.0], [4.0, 5.0], [4.0, 5.0]]]))
    with pytest.raises(ValueError, match="H = 0"):
        pl.closed_loop(pln, None, 0, start, track_fn=_stub_track)
    with pytest.raises(ValueError, match="x0 must be"):
        pl.closed_loop(pln, None, 1, start, x0=torch.zeros(3, 4), track_fn=_stub_track)


def test_audit_closed_loop_by_hand():
    p = pl.PlanProblem(N=3, goal=[1.0, 0.0], obs_c=[[0.5, 0.5]], obs_r=[0.1])
    res = {"z": torch.tensor([[[0.0, 0.0], [0.5, 0.0], [1.0, 0.0]], [[0.0, 0.0], [0.5, 0.3], [0.5, 0.5]]]),
           "pz_x": torch.tensor([[[0.0, 0.0], [0.5, 0.1], [1.0, 0.0]], [[0.0, 0.0], [0.5, 0.45], [0.5, 0.5]]]),
           "w": torch.tensor([[0.0, 0.2, 0.0], [0.0, 0.1, 0.0]]), "min_clear": torch.tensor([[0.1, 0.2], [0.1, -0.2]])}
    a = pl.audit_closed_loop(res, p, goal_tol=0.05)
    assert a["robots"] == 2 and a["steps"] == 2 and a["coverage_by_step"] == [1.0, 0.5, 1.0] and a["coverage"] == pytest.approx(5 / 6)
    assert a["covered_robots"] == 0.5 and a["actually_safe"] == 0.5 and a["predicted_safe"] == 0.5 and a["reached_goal"] == 0.5
    assert json.loads(json.dumps(a, allow_nan=False)) == a


def test_warm_start_of_the_planner_is_the_clipped_interpolation():
    p = pl.PlanProblem.named("gap", tube_kind="l1", N=7)
    z0 = np.array([[0.3, 0.3], [0.1, -0.2], [5.0, 5.0]])
    got = pl.HipMppiPlanner.warm_start(types.SimpleNamespace(problem=p), z0)
    for i, s in enumerate(z0):
        want = np.clip(pl.warm_start("interpolate", s, p.goal, p.N, p.dt)[1], -0.2, 0.2).astype(np.float32)
        np.testing.assert_array_equal(got[i], want)
    assert got.dtype == np.float32 and (np.abs(got[2]) == np.float32(0.2)).all()


def test_script_refuses_bad_arguments(tmp_path):
    import plan_tube
    ok = ["--tube", "l1", "--problem", "gap"]
    for argv in (["--problem", "gap"], ["--tube", "l1"], ["--tube", "l1", "--problem", "left"], ok + ["--K", "33"], ok + ["--iters", "0"],
                 ok + ["--sigma", "0"], ok + ["--lambda", "-1"], ok + ["--starts", "0"], ok + ["--start_noise", "-1"], ok + ["--closed_loop", "0"],
                 ok + ["--calibration"], ok + ["--level", "0.9"], ["--tube", "l1", "--run", "r", "--problem", "gap"], ok + ["--rho_g", "-1"]):
        with pytest.raises(SystemExit):
            plan_tube.parse_args(argv)
    a = plan_tube.parse_args(ok + ["--N", "7", "--K", "64", "--lambda", "2", "--starts", "3", "--start_noise", "0.1", "--closed_loop", "4"])
    c = plan_tube.mppi_cfg(a)
    assert (c.K, c.lambda_, a.closed_loop) == (64, 2.0, 4)
    p = plan_tube.build_problem(a, None)
    assert p.N == 7 and p.tube_kind == "l1" and p.rom_v_max == [0.2, 0.2]
    s = plan_tube.starts(a, p)
    assert tuple(s.shape) == (3, 2) and s[0].tolist() == [np.float32(0.3), np.float32(0.3)] and not torch.equal(s[1], s[0])
    assert torch.equal(s, plan_tube.starts(a, p))
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.json").write_text(json.dumps({"dataset": "scalar", "H_fwd": 5, "H_rev": 3}))
    with pytest.raises(ValueError, match="scalar_horizon"):                 # what audit_plans.py refuses
        plan_tube.main(["--run", str(run), "--problem", "gap"])
    with pytest.raises(FileNotFoundError, match="config.json"):
        plan_tube.main(["--run", str(tmp_path / "none"), "--problem", "gap"])
    bad = tmp_path / "p.json"
    bad.write_text(json.dumps({"N": 5, "speed": 1.0}))
    with pytest.raises(ValueError, match="speed"):
        plan_tube.main(["--tube", "l1", "--problem", str(bad)])
