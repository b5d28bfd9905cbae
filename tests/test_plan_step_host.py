"""tube_kind 'nn_step', the part that needs no GPU (legged_gym_dev_amd/tube/plan.py, lg_plan_check): every
refusal of the envelope on both sides of the C boundary with the field in the message (the handle rules on a stand-in for the model;
the library's own are asked on the GPU, where a handle exists), the struct against the header, the taps, the row builder of
tests/plan_step_ref.py by hand and against the dataset's own rows (tests/golden/tube_rows.npz), the calibration-to-offset mapping,
the scripts' argument refusals and closed_loop's w0."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import plan_step_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
from legged_gym_dev_amd import capi  # noqa: E402
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402
from legged_gym_dev_amd.tube.calibrate import AgeCalibration, Calibration  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


def _model(input_dim=9, output_dim=1, horizon=None, level_input=False, num_units=32):
    return types.SimpleNamespace(horizon=horizon, input_dim=input_dim, output_dim=output_dim, level_input=level_input, num_units=num_units)


def _problem(**kw):
    return pl.PlanProblem.named("gap", **{"tube_kind": "nn_step", "N": 5, "H_rev": 2, "recursive": True, **kw})


# ---------------------------------------------------------------- the envelope
def test_the_kind_and_the_struct(lib):
    assert capi.PLAN_TUBE["nn_step"] == 5 and pl.TUBE_KINDS[-1] == "nn_step" and capi.PLAN_STEP_MAX_HREV == 64
    st = _problem().to_struct()
    assert st.tube_kind == 5 and st.recursive == 1 and _problem(recursive=False).to_struct().recursive == 0
    assert pl.PlanProblem().recursive is False and pl.PlanProblem.named("gap").to_struct().recursive == 0
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %d %d\\n",' \
          'sizeof(lg_plan_problem),offsetof(lg_plan_problem,window_size),offsetof(lg_plan_problem,recursive),offsetof(lg_plan_problem,dt),' \
          'offsetof(lg_plan_problem,rom_v_max),LG_PLAN_TUBE_NN_STEP,LG_PLAN_STEP_MAX_HREV);return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    S = capi.lg_plan_problem
    assert out == [C.sizeof(S), S.window_size.offset, S.recursive.offset, S.dt.offset, S.rom_v_max.offset, 5, 64]
    assert S.recursive.offset == 20 and S.dt.offset == 24              # the former pad: every other field where it was


def test_refusals_on_the_c_side_without_a_handle(lib):
    err = lambda: lib.lg_last_error().decode()
    st = _problem().to_struct()
    assert lib.lg_plan_check(C.byref(st), None, 0) == -1 and "nn_step" in err() and "handle" in err()
    for N in (0, 65):
        assert lib.lg_plan_check(C.byref(_problem(N=N).to_struct()), None, 0) == -1 and "N = " in err()
    for kind in (6, 7, -1):
        st.tube_kind = kind
        assert lib.lg_plan_check(C.byref(st), None, 0) == -1 and "tube_kind" in err() and "nn_step (5)" in err()
    st = _problem().to_struct()
    assert lib.lg_mppi_check(C.byref(pl.MppiCfg().to_struct()), C.byref(st), None, 0, 1) == -1 and "handle" in err()
    assert lib.lg_plan_grad_check(C.byref(pl.GradCfg().to_struct()), C.byref(st), None, 0, 1) == -1
    assert "nn_step" in err() and "chained MLP passes" in err()
    z = torch.zeros(4)
    p = C.c_void_p(z.data_ptr())
    call = capi.lg_plan_call(z0=p, count=1)
    assert lib.lg_plan_descend(None, C.byref(st), C.byref(pl.GradCfg().to_struct()), C.byref(call), p, p, p, p, p, p, None,
                               p) == -1 and "chained MLP passes" in err()


STAND_IN = [(dict(), _model(), None, None),
            (dict(recursive=False, H_rev=3), _model(), None, None),                                 # 9 = 1 + 2 * 4
            (dict(), _model(input_dim=10, level_input=True), 0.9, None),
            (dict(H_rev=0, recursive=False), _model(input_dim=3), None, None),
            (dict(H_rev=64, N=64), _model(input_dim=30, num_units=128), None, None),                # the largest reference shape
            (dict(), None, None, "handle"),
            (dict(), _model(horizon=(5, 2)), None, "is a horizon model"),
            (dict(), _model(output_dim=2), None, "output_dim=2"),
            (dict(), _model(input_dim=8), None, r"input_dim=8.*recursive=True"),
            (dict(recursive=False), _model(input_dim=8), None, r"input_dim=8.*recursive=False"),
            (dict(), _model(input_dim=2), None, "input_dim=2"),
            (dict(), _model(input_dim=9, level_input=True), 0.9, r"input_dim=9.*level"),
            (dict(H_rev=1), _model(), None, r"H_rev=1.*T - 1 = 2"),
            (dict(H_rev=2, recursive=False), _model(), None, r"H_rev=2.*T - 1 = 3"),
            (dict(H_rev=65), _model(), None, "H_rev=65"),
            (dict(H_rev=-1), _model(input_dim=3), None, "H_rev=-1"),
            (dict(N=0), _model(), None, "N=0"), (dict(N=65), _model(), None, "N=65"),
            (dict(), _model(), 0.9, "not level-conditioned"),
            (dict(), _model(input_dim=10, level_input=True), None, "level is missing")]


@pytest.mark.parametrize("i", range(len(STAND_IN)))
def test_envelope_on_a_stand_in(i):
    change, model, level, word = STAND_IN[i]
    if word is None:
        pl.check_envelope(_problem(**change), model, level)
    else:
        with pytest.raises(ValueError, match=word):
            pl.check_envelope(_problem(**change), model, level)


def test_the_other_kinds_keep_their_words():
    with pytest.raises(ValueError, match="not a horizon model"):
        pl.check_envelope(pl.PlanProblem.named("gap", N=5, H_rev=3), _model())
    with pytest.raises(ValueError, match="handle"):
        pl.check_envelope(pl.PlanProblem.named("gap", N=5))
    with pytest.raises(ValueError, match="tube_kind"):
        pl.check_envelope(pl.PlanProblem.named("gap", tube_kind="nn_roll"))
    pl.check_envelope(pl.PlanProblem.named("gap", tube_kind="l1", recursive=True))


def test_tile_bytes_and_the_ceiling():
    # R (VS + WS + I + 2 U + ZS) floats: the default model at N = 50 and the envelope's largest shape, by hand
    assert pl.step_tile_bytes(3, 32, 0, 50) == 4 * 32 * (101 + 51 + 3 + 64 + 153)
    assert pl.step_tile_bytes(256, 128, 64, 64) == 4 * 32 * (257 + 129 + 256 + 256 + 195) <= 144 * 1024
    big = _model(input_dim=129, num_units=128)                     # not recursive: T = 64, so H_rev = 64 will do
    pl.check_envelope(_problem(H_rev=64, N=64, recursive=False), big)
    old = pl._STEP_LDS
    try:
        pl._STEP_LDS = 64 * 1024                                       # a smaller ceiling shows the refusal and the field it names
        with pytest.raises(ValueError, match="input_dim=129.*does not fit"):
            pl.check_envelope(_problem(H_rev=64, N=64, recursive=False), big)
    finally:
        pl._STEP_LDS = old


def test_gradient_planners_refuse_the_kind():
    p = _problem()
    with pytest.raises(ValueError, match="chained MLP passes"):
        pl.HipGradPlanner(_model(), p, pl.GradCfg())
    mp = types.SimpleNamespace(problem=p, device="cpu")
    with pytest.raises(ValueError, match="chained MLP passes"):
        pl.ChainedPlanner(mp, types.SimpleNamespace(problem=p, device="cpu", needs_gradient=True))
    pl.ChainedPlanner(mp, mp)
    assert pl.HipGradPlanner.needs_gradient and not getattr(pl.HipMppiPlanner, "needs_gradient", False)


# ---------------------------------------------------------------- taps and rows
def test_taps():
    for I, level, rec, T in ((3, False, False, 1), (3, False, True, 1), (7, False, False, 3), (9, False, False, 4), (9, False, True, 3),
                             (30, False, True, 10), (31, True, True, 10), (8, True, False, 3), (21, False, False, 10)):
        assert sr.taps(I, level, rec) == T == pl.step_taps(I, level, rec), (I, level, rec)
    for I, level, rec in ((8, False, False), (8, False, True), (7, False, True), (30, False, False), (2, False, False), (1, False, True),
                          (3, True, False), (9, True, False)):
        assert sr.taps(I, level, rec) is None
        with pytest.raises(ValueError, match=f"input_dim={I}.*recursive={rec}"):
            pl.step_taps(I, level, rec)


def test_rows_by_hand():
    # T = 3, H_rev = 2, N = 4, one plan: e = w_-2, w_-1; inputs named by their step
    e, w0 = torch.tensor([[-2.0, -1.0]]), torch.tensor([0.5])
    vp = torch.tensor([[[-20.0, -21.0], [-10.0, -11.0]]])
    v = torch.tensor([[[0.0, 1.0], [10.0, 11.0], [20.0, 21.0], [30.0, 31.0]]])
    fw = torch.tensor([[100.0, 200.0, 300.0, 400.0]])                  # fw[k] = w_{k+1}
    plain = sr.rows(e, vp, w0, v, 3, False, fw=fw)
    assert plain[0].tolist() == [[0.5, 0, 1, -10, -11, -20, -21], [100, 10, 11, 0, 1, -10, -11], [200, 20, 21, 10, 11, 0, 1],
                                 [300, 30, 31, 20, 21, 10, 11]]
    rec = sr.rows(e, vp, w0, v, 3, True, fw=fw)
    assert rec[0].tolist() == [[0.5, 0, 1, -1, -10, -11, -2, -20, -21], [100, 10, 11, 0.5, 0, 1, -1, -10, -11],
                               [200, 20, 21, 100, 10, 11, 0.5, 0, 1], [300, 30, 31, 200, 20, 21, 100, 10, 11]]
    lv = sr.rows(e, vp, w0, v, 3, True, level=0.75, fw=fw)
    assert torch.equal(lv[..., :-1], rec) and lv[0, :, -1].tolist() == [0.75] * 4
    assert torch.equal(sr.rows(e, vp, w0, v, 3, False, level=0.75, fw=fw)[..., :-1], plain)
    # the teacher rows of a closed-loop roll-out: 0 where the model's own output goes, the caller's history everywhere else
    t = sr.rows(e, vp, w0, v, 3, True)
    assert t[0, :, 0].tolist() == [0.5, 0, 0, 0] and t[0, :, 3].tolist() == [-1, 0.5, 0, 0] and t[0, :, 6].tolist() == [-2, -1, 0.5, 0]
    assert torch.equal(t[..., [1, 2, 4, 5, 7, 8]], rec[..., [1, 2, 4, 5, 7, 8]])
    # a longer history than the taps need is read from its end
    more = sr.rows(torch.tensor([[9.0, -2.0, -1.0]]), torch.cat([torch.full((1, 1, 2), 9.0), vp], 1), w0, v, 3, True, fw=fw)
    assert torch.equal(more, rec)
    # the literal loop feeds its own output back
    f = lambda x: x.sum(dim=1, keepdim=True)
    got = sr.roll(f, e, vp, w0, v[:, :2], 3, True)
    r0 = 0.5 + 0 + 1 - 1 - 10 - 11 - 2 - 20 - 21
    assert got[0].tolist() == [r0, r0 + 10 + 11 + 0.5 + 0 + 1 - 1 - 10 - 11]


def test_rows_equal_the_dataset_rows():
    """The reference-made rows of ScalarTubeDataset (N = 3, recursive and not): from an interior step t0 on, N rows of the dataset
    equal the builder fed that env's w, v history -- e and v_prev the steps before t0, w0 = w[t0], the true w as the values fed back."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "tube_rows.npz"))
    one = torch.from_numpy(z["scalar_n1_data"])
    w, v = one[:, 0], one[:, 1:3]
    T, N = 3, 6
    for name, rec in (("scalar_n3", False), ("scalar_n3_rec", True)):
        data = torch.from_numpy(z[name + "_data"])
        assert torch.equal(data[:, :3], one)
        for t0, Hr in ((2, 2), (5, 2), (7, 4)):
            got = sr.rows(w[None, t0 - Hr:t0], v[None, t0 - Hr:t0], w[None, t0], v[None, t0:t0 + N], T, rec, fw=w[None, t0 + 1:t0 + N + 1])
            assert torch.equal(got[0], data[t0:t0 + N]), (name, t0, Hr)


# ---------------------------------------------------------------- calibration to offsets
def test_offsets_from_a_calibration():
    age = AgeCalibration([0.9, 0.95], torch.tensor([[[0.1], [0.2], [0.3]], [[1.0], [2.0], [3.0]]]), [10, 10, 10], [[9, 10]] * 3,
                         margin=torch.tensor([[0.5], [0.25]]), margin_n=4, margin_ranks=[4, 4])
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    assert torch.equal(pl.step_offsets(age, 5, coverage=0.9), f([0.1, 0.2, 0.3, 0.3, 0.3]))             # clamped at max_age - 1
    assert torch.equal(pl.step_offsets(age, 2, coverage=0.95), f([1.0, 2.0]))
    assert torch.equal(pl.step_offsets(age, 4, coverage=0.95, trajectory=True), f([1.25, 2.25, 3.25, 3.25]))
    for N, kw in ((5, dict(coverage=0.9)), (4, dict(coverage=0.95, trajectory=True)), (1, dict(coverage=0.9))):
        assert torch.equal(pl.step_offsets(age, N, **kw), sr.offsets(age, N, **kw))
    with pytest.raises(ValueError, match="coverage"):
        pl.step_offsets(age, 3)
    with pytest.raises(KeyError, match="0.8"):
        pl.step_offsets(age, 3, coverage=0.8)
    plain = AgeCalibration([0.9], torch.tensor([[[0.1], [0.2]]]), [10, 10], [[9]] * 2)
    assert torch.equal(pl.step_offsets(plain, 3), f([0.1, 0.2, 0.2]))                                    # a single coverage needs no name
    with pytest.raises(ValueError, match="margin"):
        pl.step_offsets(plain, 3, trajectory=True)
    flat = Calibration("flat", [0.9, 0.95], torch.tensor([[[0.05], [0.06]], [[0.2], [0.3]]]), 10, [9, 10])
    assert torch.equal(pl.step_offsets(flat, 4, coverage=0.95), f([0.06, 0.3, 0.3, 0.3])) and torch.equal(pl.step_offsets(flat, 1, coverage=0.9), f([0.05]))
    assert torch.equal(pl.step_offsets(flat, 4, coverage=0.95), sr.offsets(flat, 4, coverage=0.95))
    lev = Calibration("levels", [0.5, 0.9], torch.tensor([[[0.0], [0.01]], [[0.1], [0.4]]]), 10, [5, 9])
    assert torch.equal(pl.step_offsets(lev, 3, level=0.9), f([0.01, 0.4, 0.4])) and torch.equal(pl.step_offsets(lev, 3, level=0.9), sr.offsets(lev, 3, level=0.9))
    with pytest.raises(ValueError, match="margin"):
        pl.step_offsets(flat, 3, coverage=0.9, trajectory=True)
    for kind, off in (("horizon", torch.zeros(1, 5)), ("horizon_levels", torch.zeros(1, 5))):
        with pytest.raises(ValueError, match=f"'{kind}' calibration"):
            pl.step_offsets(Calibration(kind, [0.9], off, 10, [9]), 5, coverage=0.9, level=0.9)
    wide = AgeCalibration([0.9], torch.zeros(1, 2, 2), [10, 10], [[9]] * 2)
    with pytest.raises(ValueError, match="scalar"):
        pl.step_offsets(wide, 3)


# ---------------------------------------------------------------- the scripts
def _run(tmp_path, name, **cfg):
    run = tmp_path / name
    run.mkdir()
    (run / "config.json").write_text(json.dumps(cfg))
    return str(run)


def test_scripts_refuse_bad_arguments(tmp_path):
    import audit_plans
    import plan_tube
    ok_a = ["--problem", "gap", "--warm_start", "interpolate"]
    ok_p = ["--problem", "gap"]
    for mod, ok in ((audit_plans, ok_a), (plan_tube, ok_p)):
        for argv in (["--tube", "nn_step"] + ok, ["--tube", "nn"] + ok, ["--tube", "l1", "--age_calibration"] + ok,
                     ["--run", "r", "--age_calibration", "--calibration"] + ok, ["--run", "r", "--trajectory_margin"] + ok,
                     ["--tube", "l1", "--H_rev", "2"] + ok, ["--run", "r", "--H_rev", "-1"] + ok):
            with pytest.raises(SystemExit):
                mod.parse_args(argv)
        assert mod.parse_args(["--tube", "l2_rolling"] + ok).tube == "l2_rolling"
    for argv in (["--tube", "l1", "--w0", "error"] + ok_p, ["--run", "r", "--closed_loop", "3", "--w0", "last"] + ok_p):
        with pytest.raises(SystemExit):
            plan_tube.parse_args(argv)
    a = plan_tube.parse_args(["--run", "r", "--closed_loop", "3", "--w0", "error", "--age_calibration", "--trajectory_margin", "--coverage", "0.9"] + ok_p)
    assert a.w0 == "error" and a.age_calibration == "" and a.trajectory_margin and plan_tube.parse_args(["--run", "r"] + ok_p).w0 == "zero"
    # the runs: scalar / scalar_level with dN = 1 are step runs; vector, error-dynamics and Alpha runs stay refused by name
    base = dict(N=10, dN=1, recursive=True, H_fwd=50, H_rev=10)
    step = _run(tmp_path, "step", dataset="scalar", **base)
    cfg = audit_plans.run_config(step)
    assert audit_plans.is_step(cfg) and not audit_plans.is_step({"dataset": "scalar_horizon"}) and not audit_plans.is_step(None)
    p = audit_plans.build_problem(audit_plans.parse_args(["--run", step, "--N", "20"] + ok_a), cfg)
    assert (p.tube_kind, p.recursive, p.N, p.H_rev, p.rom_v_max) == ("nn_step", True, 20, 9, [0.2, 0.2])
    p = plan_tube.build_problem(plan_tube.parse_args(["--run", step, "--H_rev", "12"] + ok_p), cfg)
    assert (p.tube_kind, p.N, p.H_rev) == ("nn_step", 50, 12)
    p = audit_plans.build_problem(audit_plans.parse_args(["--run", step] + ok_a), {**cfg, "N": 1, "recursive": False})
    assert (p.recursive, p.H_rev) == (False, 0)
    for kind in ("vector", "error_dynamics", "alpha", "vector_level"):
        with pytest.raises(ValueError, match=f"'{kind}' model"):
            audit_plans.main(["--run", _run(tmp_path, kind, dataset=kind, **base)] + ok_a)
    with pytest.raises(ValueError, match="dN = 2"):
        plan_tube.main(["--run", _run(tmp_path, "dn2", dataset="scalar", **{**base, "dN": 2})] + ok_p)
    with pytest.raises(ValueError, match="holds no N, dN, recursive"):
        audit_plans.main(["--run", _run(tmp_path, "old", dataset="scalar_level", H_fwd=5, H_rev=3)] + ok_a)
    with pytest.raises(ValueError, match="--level is required"):
        audit_plans.main(["--run", _run(tmp_path, "lvl", dataset="scalar_level", **base)] + ok_a)
    with pytest.raises(FileNotFoundError, match="calibration_age.json"):
        plan_tube.main(["--run", step, "--age_calibration"] + ok_p)
    with pytest.raises(FileNotFoundError, match="calibration.json"):
        audit_plans.main(["--run", step, "--calibration"] + ok_a)
    one_shot = _run(tmp_path, "oneshot", dataset="scalar_horizon", **base)
    with pytest.raises(ValueError, match="--age_calibration belongs to a step run"):
        audit_plans.main(["--run", one_shot, "--age_calibration"] + ok_a)
    step_p = types.SimpleNamespace(tube_kind="nn_step")
    for planner in ("grad", "mppi+grad"):
        with pytest.raises(ValueError, match="chained MLP passes"):
            plan_tube.make_planner(plan_tube.parse_args(["--run", step, "--planner", planner] + ok_p), None, step_p, None)


# ---------------------------------------------------------------- closed_loop's w0
class _StubPlanner:
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
    x1 = torch.cat([x0[:, :2] + 0.1, v[:, 0]], dim=1)
    return {"x": torch.stack([x0, x1], dim=1), "u": torch.stack([v[:, 0], -v[:, 0]], dim=1)}


def test_closed_loop_w0():
    N, H, Hr = 3, 3, 2
    start = torch.tensor([[0.0, 0.0], [1.0, -1.0]])
    x0 = torch.tensor([[0.3, 0.4, 0.0, 0.0], [1.0, -1.0, 0.0, 0.0]])
    runs = {}
    for name, kw in (("before", {}), ("zero", {"w0": "zero"}), ("error", {"w0": "error"})):
        pln = _StubPlanner(N, Hr)
        runs[name] = (pln.calls, pl.closed_loop(pln, None, H, start, x0=x0, iters_first=7, keep_plans=True, track_fn=_stub_track, **kw))
    for (ca, oa), (cb, ob) in ((runs["before"], runs["zero"]), (runs["zero"], runs["error"])):
        assert len(ca) == len(cb) == H
        for a, b in zip(ca, cb):                                       # everything but w0 is the same in all three
            assert a["iters"] == b["iters"] and all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in ("z0", "v_init", "e", "v_prev"))
        assert all(torch.equal(oa[k], ob[k]) for k in oa)
    assert all(c["w0"] is None for c in runs["before"][0]) and all(c["w0"] is None for c in runs["zero"][0])
    calls, out = runs["error"]
    for k, c in enumerate(calls):                                      # |z_k - pz_x_k| at every replanning, the first included
        assert torch.equal(c["w0"], torch.linalg.vector_norm(out["z"][:, k] - out["pz_x"][:, k], dim=1))
    assert calls[0]["w0"].tolist() == [0.5, 0.0]
    with pytest.raises(ValueError, match="w0 = 'last'"):
        pl.closed_loop(_StubPlanner(N, Hr), None, H, start, track_fn=_stub_track, w0="last")
