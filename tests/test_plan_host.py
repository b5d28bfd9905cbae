"""Plans against a tube, the part that needs no GPU (legged_gym_dev_amd/tube/plan.py, lg_plan_check): every
refusal of the envelope with the field in the message, PROBLEMS against the numbers the fixture recorded from the reference,
warm_start and audit by hand, the NumPy restatement (tests/plan_ref.py) against the reference's own tracking loop
(tests/golden/plan_track.npz, written by tools/gen_fixtures_plan.py), and the script's argument refusals."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import plan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(ROOT, "tests", "golden", "plan_track.npz"))
    return {**{k: z[k] for k in ("z", "v", "x", "u", "w")}, "problems": json.loads(str(z["meta_problems"])),
            "cfg": json.loads(str(z["meta_cfg"])), "names": json.loads(str(z["meta_names"]))}


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


def _model(horizon=(5, 3), input_dim=3 + 2 * 8, level_input=False):
    return types.SimpleNamespace(horizon=horizon, input_dim=input_dim, level_input=level_input)


# (changes to a valid analytic problem, the words the message must hold); the same list is asked of lg_plan_check
BAD = [(dict(N=0), "N"), (dict(N=65), "N"), (dict(obs_c=[[0.0, 0.0]] * 9, obs_r=[0.1] * 9), "n_obs"), (dict(dt=0.0), "dt"),
       (dict(dt=-0.1), "dt"), (dict(obs_c=[[0.0, 0.0], [1.0, 1.0]], obs_r=[0.5, -0.1]), "obs_r[1]"),
       (dict(tube_kind="l1_rolling", window_size=0), "window_size"), (dict(tube_kind="l2_rolling", window_size=-3), "window_size"),
       (dict(tube_kind="nn"), "handle")]


@pytest.mark.parametrize("change,word", BAD, ids=[f"{list(c)[0]}-{i}" for i, (c, _) in enumerate(BAD)])
def test_refusals_name_the_field(lib, change, word):
    p = pl.PlanProblem.named("gap", **{"tube_kind": "l1", "N": 5, **change})
    with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
        pl.check_envelope(p)
    st = p.to_struct()
    if "obs_c" in change and len(change["obs_c"]) > 8:
        st.n_obs = 9
    assert lib.lg_plan_check(C.byref(st), None, 0) == -1
    assert word in lib.lg_last_error().decode()


def test_valid_problems_pass_and_level_rules(lib):
    for kind in ("l1", "l2", "l1_rolling", "l2_rolling"):
        p = pl.PlanProblem.named("right", tube_kind=kind, N=64, window_size=1)
        pl.check_envelope(p)
        assert lib.lg_plan_check(C.byref(p.to_struct()), None, 0) == 0
    p = pl.PlanProblem.named("right", tube_kind="l1", N=5)
    with pytest.raises(ValueError, match="level"):
        pl.check_envelope(p, None, 0.9)
    assert lib.lg_plan_check(C.byref(p.to_struct()), None, 1) == -1 and "level" in lib.lg_last_error().decode()
    st = p.to_struct()
    st.tube_kind = 7
    assert lib.lg_plan_check(C.byref(st), None, 0) == -1 and "tube_kind" in lib.lg_last_error().decode()
    with pytest.raises(ValueError, match="tube_kind"):
        pl.check_envelope(pl.PlanProblem.named("right", tube_kind="l3"))
    # the handle rules, on a stand-in for the model (the library's own are asked on the GPU, where a handle exists)
    nn = pl.PlanProblem.named("gap", N=5, H_rev=3)
    pl.check_envelope(nn, _model())
    pl.check_envelope(nn, _model(input_dim=20, level_input=True), 0.9)
    for model, level, word in ((_model(horizon=None), None, "horizon"), (_model(horizon=(4, 3)), None, "H_fwd"),
                               (_model(horizon=(5, 2)), None, "H_rev"), (_model(input_dim=21), None, "nz"),
                               (_model(), 0.9, "level"), (_model(input_dim=20, level_input=True), None, "level")):
        with pytest.raises(ValueError, match=word):
            pl.check_envelope(nn, model, level)


def test_problems_are_the_reference_numbers(fx):
    assert sorted(pl.PROBLEMS) == sorted(fx["problems"])
    for name, rec in fx["problems"].items():
        assert pl.PROBLEMS[name] == rec, name
        p = pl.PlanProblem.named(name)
        assert p.start == rec["start"] and p.goal == rec["goal"] and p.obs_c == rec["obs_c"] and p.obs_r == rec["obs_r"] and p.dt == rec["dt"]
        assert p.rom_v_max == [rec["vel_max"]] * 2 and p.rom_v_min == [-rec["vel_max"]] * 2 and p.rom_z_max == [rec["pos_max"]] * 2
        st = p.to_struct()
        assert st.n_obs == 2 and st.obs_r[1] == np.float32(rec["obs_r"][1]) and st.obs_c[1][0] == np.float32(rec["obs_c"][1][0])
        assert list(st.Q) == [10.0, 0.0, 0.0, 10.0] == list(st.Qf) == list(st.R) and st.N == 50 and st.w_max == 1.0 and st.Qw == 0.0
    with pytest.raises(KeyError, match="gap"):
        pl.PlanProblem.named("left")


def test_struct_matches_the_header(lib):
    import subprocess
    import tempfile
    from legged_gym_dev_amd import capi
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(lg_plan_problem),' \
          'offsetof(lg_plan_problem,goal),offsetof(lg_plan_problem,rom_v_max));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [C.sizeof(capi.lg_plan_problem), capi.lg_plan_problem.goal.offset, capi.lg_plan_problem.rom_v_max.offset]


def test_call_struct_matches_the_header():
    import subprocess
    import tempfile
    from legged_gym_dev_amd import capi
    T = capi.lg_plan_call
    names = [n for n, _ in T._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu' + ' %zu' * len(names) + \
          '\\n",sizeof(lg_plan_call)' + "".join(f",offsetof(lg_plan_call,{n})" for n in names) + ');return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert names == ["z0", "e", "v_prev", "w0", "offset", "scenes", "count", "has_level", "level", "stream"]
    assert out == [C.sizeof(T)] + [getattr(T, n).offset for n in names]


def test_argtypes_match_the_prototypes(lib):
    """Every lg_plan_* / lg_mppi_* prototype of the header against the ctypes declaration: as many arguments, and per position the
    same class -- pointer, 32-bit integer, 64-bit integer or float.  ctypes checks none of this at a call."""
    import re
    import subprocess
    from legged_gym_dev_amd.lib import SO_PATH
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "legged_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(lg_(?:plan|mppi)_\w+)\s*\(([^)]*)\)\s*;", text))
    assert len(protos) == 13 and {"lg_plan_score", "lg_plan_descend_step", "lg_mppi_check", "lg_plan_track", "lg_plan_fleet_scenes"} <= set(protos)

    def of_c(param):
        if "*" in param:
            return "pointer"
        return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "float"}[param.split()[-2]]

    def of_ctypes(t):
        if t is C.c_void_p or t is C.c_char_p or issubclass(t, C._Pointer):
            return "pointer"
        return {C.c_int32: "i32", C.c_int64: "i64", C.c_float: "float"}[t]

    for name, params in protos.items():
        want = [of_c(q.strip()) for q in params.split(",")]
        got = [of_ctypes(t) for t in getattr(lib, name).argtypes]
        assert got == want, name
    # the twins are gone, from the header and from the library, and the library exports what the header declares
    keep = {"lg_plan_scenes", "lg_plan_scenes_check", "lg_plan_fleet_scenes"}
    assert set(re.findall(r"\blg_plan_\w*scenes\w*", text)) == keep
    syms = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", SO_PATH]).decode().splitlines() if ln.strip()}
    assert {n for n in syms if re.match(r"lg_(plan|mppi)_", n)} == set(protos)


def test_warm_start_by_hand():
    z, v = pl.warm_start("interpolate", [0.0, 1.0], [2.0, 0.0], 4, 0.5)
    np.testing.assert_allclose(z, [[0, 1], [0.5, 0.75], [1.0, 0.5], [1.5, 0.25], [2.0, 0.0]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(v, [[1.0, -0.5]] * 4, rtol=0, atol=1e-15)
    z, v = pl.warm_start("start", [0.0, 1.0], [2.0, 0.0], 3, 0.5)
    assert z.tolist() == [[0.0, 1.0]] * 4 and v.tolist() == [[0.0, 0.0]] * 3
    z, v = pl.warm_start("goal", [0.0, 1.0], [2.0, 0.0], 3, 0.5)
    assert z.tolist() == [[2.0, 0.0]] * 4 and v.tolist() == [[0.0, 0.0]] * 3
    with pytest.raises(NotImplementedError, match="CasADi"):
        pl.warm_start("nominal", [0, 0], [1, 1], 3, 0.1)
    with pytest.raises(ValueError, match="ic"):
        pl.warm_start("ic", [0, 0], [1, 1], 3, 0.1)


def test_perturb_is_clipped_and_repeatable():
    v = np.full((6, 2), 0.19, np.float32)
    a, b = pl.perturb(v, 0.05, 8, 3, [-0.2, -0.2], [0.2, 0.2]), pl.perturb(v, 0.05, 8, 3, [-0.2, -0.2], [0.2, 0.2])
    assert tuple(a.shape) == (8, 6, 2) and a.dtype == torch.float32 and torch.equal(a, b)
    assert float(a.max()) == np.float32(0.2) and float(a.min()) < 0.19 and not torch.equal(a, pl.perturb(v, 0.05, 8, 4, [-0.2, -0.2], [0.2, 0.2]))
    assert torch.equal(pl.perturb(v, 0.0, 2, 1, [-1, -1], [1, 1]), torch.as_tensor(v).repeat(2, 1, 1))


def test_audit_by_hand():
    # three plans of two nodes; one obstacle of radius 0.5 at (1, 0)
    p = pl.PlanProblem(N=1, obs_c=[[1.0, 0.0]], obs_r=[0.5])
    score = {"w": torch.tensor([[0.0, 0.2], [0.0, 0.1], [0.1, 0.3]]), "min_clear": torch.tensor([0.5, -0.1, 0.0])}
    track = {"w_true": torch.tensor([[0.0, 0.1], [0.0, 0.2], [0.2, 0.3]]),
             "pz_x": torch.tensor([[[0.0, 0.0], [0.4, 0.0]], [[0.0, 0.0], [0.6, 0.0]], [[0.0, 0.0], [0.5, 0.0]]])}
    a = pl.audit(score, track, p)
    assert a["plans"] == 3 and a["nodes"] == 2
    assert a["coverage_by_node"] == [2 / 3, 2 / 3] and a["coverage"] == 4 / 6 and a["covered_plans"] == 1 / 3
    assert a["predicted_safe"] == 2 / 3 and a["actually_safe"] == 2 / 3        # |(0.5, 0) - (1, 0)| = r is outside: strict <
    assert a["table"] == {"safe_safe": 2 / 3, "safe_unsafe": 0.0, "unsafe_safe": 0.0, "unsafe_unsafe": 1 / 3}
    np.testing.assert_allclose([a["w_true_mean"], a["w_true_max"]], [0.8 / 6, 0.3], rtol=1e-6)
    assert json.loads(json.dumps(a, allow_nan=False)) == a
    ref = plan_ref.audit(score["w"].numpy(), track["w_true"].numpy(), track["pz_x"].numpy(), score["min_clear"].numpy(), p.obs_c, p.obs_r)
    assert ref == a
    free = pl.audit({"w": score["w"], "min_clear": torch.full((3,), float("inf"))}, track, pl.PlanProblem(N=1))
    assert free["predicted_safe"] == 1.0 == free["actually_safe"] and json.loads(json.dumps(free, allow_nan=False)) == free


def test_restatement_against_the_reference_loop(fx):
    """Two links, each at rtol = atol = 1e-6.  The float64 restatement against the reference's run over the whole chain of 50
    steps (x, u, pz_x = x[:, :, :2], w).  Then, per step, the float32 restatement against the float64 one, both restarted from the
    reference's state at that step rounded to float32: the same inputs on both sides, so the figure is the rounding of one step's
    arithmetic alone, for the state and for the action."""
    c, z, v, x, u = fx["cfg"], fx["z"], fx["v"], fx["x"], fx["u"]
    P, N = v.shape[:2]
    assert P == 16 and N == 50 and fx["names"][-1] == "saturating" and not x[:, 0].any() and v.dtype == np.float32
    r64 = plan_ref.track(c, z, v, x0=x[:, 0], S=1, rom_dt=c["model_dt"], dtype=np.float64)
    # the constants enter at their float32 values (dt = float32(0.1), as the device holds it): still within the bound of the run
    for k, want in (("x", x), ("u", u), ("pz_x", x[:, :, :2]), ("w_true", fx["w"])):
        np.testing.assert_allclose(r64[k], want, rtol=1e-6, atol=1e-6, err_msg=k)
    worst = {"u": 0.0, "x": 0.0}
    for t in range(N):                                               # a one-node plan restarted from the reference's state at t
        z32, ff, x32 = z[:, t:t + 2].astype(np.float32), v[:, min(t + 1, N - 1)][:, None], x[:, t].astype(np.float32)
        one = {D: plan_ref.track(c, z32, ff, x0=x32, S=1, rom_dt=c["model_dt"], dtype=D) for D in (np.float32, np.float64)}
        assert one[np.float32]["u"].dtype == np.float32 and one[np.float64]["u"].dtype == np.float64
        for k, i in (("u", 0), ("x", 1)):
            got, want = one[np.float32][k][:, i], one[np.float64][k][:, i]
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6, err_msg=f"{k} of step {t}")
            worst[k] = max(worst[k], float((np.abs(got - want) / (1e-6 + 1e-6 * np.abs(want))).max()))
        np.testing.assert_array_equal(one[np.float32]["pz_x"][:, 1], one[np.float32]["x"][:, 1, :2])
    print(f"largest one-step difference of the float32 restatement, in units of the bound: u {worst['u']:.3f}, x {worst['x']:.3f}")
    # the saturating plan: first the acceleration bound, then the velocity bound, on the steps the restatement names
    bind = r64["bind"][-1]
    assert (np.abs(bind) == 1).any() and (np.abs(bind) == 2).any()
    first_vel = int(np.argmax((np.abs(bind) == 2).any(axis=1)))
    # 2 / (2 * 0.1) = 10 steps at full acceleration; after 9 of them (2 - 1.8) / 0.1 is 2 to within an ulp, on either side of it
    assert (np.abs(bind[:first_vel]) == 1).all() and first_vel in (9, 10)
    assert (np.abs(fx["u"][-1][:first_vel]) == 2.0).all() and np.abs(fx["x"][-1][first_vel:, 2:]).max() <= 2.0 + 1e-12


def test_restatement_score_by_hand():
    p = dict(N=2, H_rev=0, dt=0.5, goal=[1.0, 0.0], obs_c=[[0.5, 0.0]], obs_r=[0.25], Q=[1, 0, 0, 1], Qf=[2, 0, 0, 2], R=[1, 0, 0, 1], Qw=3.0,
             w_max=0.2, scaling=0.5, window_size=2, tube_kind="l1", rom_z_min=[-10, -10], rom_z_max=[0.9, 10], rom_v_min=[-1, -1], rom_v_max=[0.5, 1])
    v = np.array([[[1.0, 0.0], [1.0, 0.0]]])
    fw = plan_ref.analytic("l1", v, 0.5, 2, np.float64)
    assert fw.tolist() == [[0.5, 0.5]]
    assert plan_ref.analytic("l2_rolling", np.array([[[1.0, 1.0], [2.0, 0.0], [0.0, 0.0]]]), 0.5, 2, np.float64).tolist() == [[1.0, 1.5, 1.0]]
    s = plan_ref.score(p, np.zeros((1, 2)), v, fw, dtype=np.float64)
    assert s["z"].tolist() == [[[0, 0], [0.5, 0], [1.0, 0]]] and s["w"].tolist() == [[0, 0.5, 0.5]]
    # g: node 0 0.25 - 0.0625, node 1 0 - 0.5625, node 2 0.25 - 0.5625
    assert s["g"][0, :, 0].tolist() == [0.1875, -0.5625, -0.3125] and s["min_clear"][0] == -0.5625 and s["worst_node"][0] == 1
    assert s["cost"][0] == (1.0 + 0.25) + 2 * 0.0 + (1.0 + 1.0) + 3 * (0.25 + 0.25)
    assert s["n_viol"].tolist() == [[2, 2, 1, 2]]                     # v_x = 1 > 0.5 twice; z_x = 1 > 0.9 once; w = 0.5 > 0.2 twice
    x = plan_ref.item(np.array([[7.0]]), np.array([[[1.0, 2.0]]]), np.array([[[3.0, 4.0], [5.0, 6.0]]]), 0.9)
    assert x.tolist() == [[7.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.9]]


def test_script_refuses_bad_arguments(tmp_path):
    import audit_plans
    for argv in (["--tube", "l1", "--problem", "gap"], ["--tube", "l1", "--problem", "gap", "--plans", "x.npz", "--perturb", "3"],
                 ["--tube", "l1", "--problem", "gap", "--warm_start", "interpolate", "--calibration"],
                 ["--tube", "l1", "--problem", "gap", "--warm_start", "interpolate", "--level", "0.9"],
                 ["--tube", "l3", "--problem", "gap", "--warm_start", "interpolate"],
                 ["--tube", "l1", "--run", "r", "--problem", "gap", "--warm_start", "interpolate"]):
        with pytest.raises(SystemExit):
            audit_plans.parse_args(argv)
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.json").write_text(json.dumps({"dataset": "scalar", "H_fwd": 5, "H_rev": 3}))
    with pytest.raises(ValueError, match="scalar_horizon"):
        audit_plans.main(["--run", str(run), "--problem", "gap", "--warm_start", "interpolate"])
    with pytest.raises(FileNotFoundError, match="config.json"):
        audit_plans.main(["--run", str(tmp_path / "none"), "--problem", "gap", "--warm_start", "interpolate"])
    with pytest.raises(NotImplementedError, match="CasADi"):
        audit_plans.main(["--tube", "l1", "--problem", "gap", "--warm_start", "nominal"])
    bad = tmp_path / "p.json"
    bad.write_text(json.dumps({"N": 5, "speed": 1.0}))
    with pytest.raises(ValueError, match="speed"):
        audit_plans.main(["--tube", "l1", "--problem_json", str(bad), "--warm_start", "interpolate"])
    a = audit_plans.parse_args(["--tube", "l2_rolling", "--problem", "right", "--warm_start", "interpolate", "--perturb", "3", "--N", "7",
                                "--sim_cfg", "env.model.dt=0.1", "controller.Kp=5"])
    p = audit_plans.build_problem(a, None)
    assert p.N == 7 and p.tube_kind == "l2_rolling" and p.rom_v_max == [1.0, 1.0]
    z0, v, src = audit_plans.build_plans(a, p)
    assert tuple(z0.shape) == (4, 2) and tuple(v.shape) == (4, 7, 2) and src["perturb"] == 3
    rc = audit_plans.sim_config(a, p)
    assert rc.env.model.dt == 0.1 and rc.controller.Kp == 5 and rc.rom.dt == 0.1 and rc.env.num_envs == 1
    f = tmp_path / "plans.npz"
    np.savez(f, z0=np.zeros((3, 2), np.float32), v=np.zeros((3, 7, 2), np.float32))
    a.plans, a.perturb = str(f), 0
    z0, v, src = audit_plans.build_plans(a, p)
    assert tuple(z0.shape) == (3, 2) and tuple(v.shape) == (3, 7, 2) and src == {"plans_file": str(f)}
    a.sim_cfg = ["env.model.speed=1"]
    with pytest.raises(ValueError, match="env.model.speed"):
        audit_plans.sim_config(a, p)
