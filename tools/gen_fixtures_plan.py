#!/usr/bin/env python3
"""Golden fixture of plan tracking: tests/golden/plan_track.npz

TEST INFRASTRUCTURE -- needs the reference tree (REF of oracle/gen_fixtures.py); the .npz it writes is committed and holds data
only.  Drives the reference's own SingleInt2D and DoubleInt2D (trajopt/rom_dynamics.py, backend='numpy'), imported the way
tools/gen_fixtures_rom_sim.py imports them, through the loop of deep_tube_learning/evaluation/
evaluate_tube_simple_oneshot_on_mpc_traj.py:75-90 -- driven from here, batched over the plans and in this tool's own terms, since
that script solves an NLP (CasADi, IPOPT, wandb) before it reaches its loop; clip_v_z, f and proj_z are the reference's.  problem_dict and get_warm_start are taken from trajopt/tube_trajopt.py's own text (the module
itself imports CasADi and l4casadi): the assignment and the function are cut out with ast and evaluated with numpy alone.

Plans, N = 50: per problem (gap, right, right_wide) the 'interpolate' warm start and 4 clipped Gaussian perturbations of it
(legged_gym_dev_amd.tube.plan.perturb, sigma 0.05, seeds 1..3), then one plan of |v| = 5 on which first the acceleration bound and
then the velocity bound of the tracking model binds.  Every v is a float32 value; z is SingleInt2D.f rolled out from the start in
float64; the model is the script's DoubleInt2D(dt, +-[inf, inf, 2, 2], +-[2, 2]) with Kp = Kd = 10, started at x = 0 as the script does.
Recorded: z, x, u, w in float64 (the yardstick: 16 plans x 51 nodes x 9 numbers) and v in float32; pz_x is x[:, :, :2] and is not
stored.  About 50 KiB: the perturbed plans and their float64 responses do not compress.

    python tools/gen_fixtures_plan.py
"""
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import gen_fixtures as gf  # noqa: E402
import gen_fixtures_trajectory as gft  # noqa: E402
from legged_gym_dev_amd.tube.plan import perturb  # noqa: E402

N, KP, KD, SIGMA, K_PERTURB = 50, 10.0, 10.0, 0.05, 4


def from_reference_text(names):
    """{name: object} of top-level assignments / functions of trajopt/tube_trajopt.py, evaluated with numpy only."""
    src = open(os.path.join(gf.REF, "trajopt", "tube_trajopt.py")).read()
    ns = {"np": np}
    for node in ast.parse(src).body:
        name = node.targets[0].id if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) else getattr(node, "name", None)
        if name in names:
            exec(compile(ast.Module([node], []), "tube_trajopt.py", "exec"), ns)
    return {k: ns[k] for k in names}


def drive(model, z, v):
    """Every plan at once through the reference's DoubleInt2D: from rest at the origin, per node k the tracking law
    Kp (z[k] - position) + Kd (v[min(k + 1, N - 1)] - velocity), clipped by the model's clip_v_z, then the model's f.
    The law is that of evaluate_tube_simple_oneshot_on_mpc_traj.py:75-88; the arithmetic is the reference classes' own."""
    P, N = v.shape[:2]
    state, act = np.zeros((P, N + 1, model.n)), np.zeros((P, N, model.m))
    for k in range(N):
        here, ahead = state[:, k], v[:, min(k + 1, N - 1)]
        act[:, k] = model.clip_v_z(here, KP * (z[:, k] - here[:, :2]) + KD * (ahead - here[:, 2:]))
        state[:, k + 1] = model.f(here, act[:, k])
    return state, act


def main():
    gf._build_isaacgym_stub(gf._STATE)
    gf._load_reference_modules()
    gft.load_trajectory_modules()
    rd = sys.modules["trajopt.rom_dynamics"]
    ref = from_reference_text(("problem_dict", "get_warm_start"))
    problems = ref["problem_dict"]
    assert list(problems) == ["gap", "right", "right_wide"]
    dt = problems["gap"]["dt"]
    zmax, vmax = np.array([np.inf, np.inf, 2.0, 2.0]), np.array([2.0, 2.0])
    double_int = rd.DoubleInt2D(dt, -zmax, zmax, -vmax, vmax, n_robots=1, backend="numpy")
    plans, names = [], []
    for pi, (name, p) in enumerate(problems.items()):
        assert p["dt"] == dt
        pm = rd.SingleInt2D(p["dt"], -np.ones(2) * p["pos_max"], np.ones(2) * p["pos_max"], -np.ones(2) * p["vel_max"],
                            np.ones(2) * p["vel_max"], backend="numpy")
        z_init, v_init = ref["get_warm_start"]("interpolate", p["start"], p["goal"], N, pm)
        v0 = v_init.astype(np.float32)
        vs = [v0] + list(perturb(v0, SIGMA, K_PERTURB, pi + 1, pm.v_min, pm.v_max).numpy())
        for j, v in enumerate(vs):
            plans.append((pm, p["start"].astype(np.float64), v.astype(np.float64)))
            names.append(f"{name}/{'interpolate' if j == 0 else f'perturbed{j}'}")
    pm = rd.SingleInt2D(dt, -np.ones(2) * 10, np.ones(2) * 10, -np.ones(2) * 5, np.ones(2) * 5, backend="numpy")
    plans.append((pm, np.zeros(2), np.tile(np.array([5.0, -5.0]), (N, 1))))
    names.append("saturating")
    zs = []
    for pm, start, v in plans:                                     # the ROM nodes: SingleInt2D.f from the start
        z = np.zeros((N + 1, 2))
        z[0] = start
        for k in range(N):
            z[k + 1] = pm.f(z[k][None, :], v[k][None, :])[0]
        zs.append(z)
    z, v = np.stack(zs), np.stack([v for _, _, v in plans])
    x, u = drive(double_int, z, v)
    w = np.linalg.norm(z - double_int.proj_z(x.reshape(-1, 4)).reshape(z.shape), axis=-1)
    out = {"z": z, "v": v.astype(np.float32), "x": x, "u": u, "w": w}
    assert (out["v"].astype(np.float64) == v).all()
    u = out["u"][-1]
    assert (np.abs(u) == 2.0).any() and ((np.abs(u) < 2.0) & (np.abs(out["x"][-1][:-1, 2:]) >= 2.0 - 1e-9)).any(), \
        "the saturating plan must meet the acceleration bound and then the velocity bound"
    recorded = {k: {"start": p["start"].tolist(), "goal": p["goal"].tolist(), "obs_c": p["obs"]["c"].tolist(), "obs_r": p["obs"]["r"].tolist(),
                    "vel_max": float(p["vel_max"]), "pos_max": float(p["pos_max"]), "dt": float(p["dt"])} for k, p in problems.items()}
    cfg = {"Kp": KP, "Kd": KD, "model_dt": dt, "model_z_min": [-1e9, -1e9, -2.0, -2.0], "model_z_max": [1e9, 1e9, 2.0, 2.0],
           "model_v_min": [-2.0, -2.0], "model_v_max": [2.0, 2.0], "N": N, "sigma": SIGMA}
    dst = os.path.join(ROOT, "tests", "golden", "plan_track.npz")
    np.savez_compressed(dst, meta_problems=np.array(json.dumps(recorded)), meta_cfg=np.array(json.dumps(cfg)),
                        meta_names=np.array(json.dumps(names)), **out)
    print(f"{dst}: {len(plans)} plans of N = {N}, {os.path.getsize(dst) / 1024:.0f} KiB; w max {out['w'].max():.3f}")


if __name__ == "__main__":
    main()
