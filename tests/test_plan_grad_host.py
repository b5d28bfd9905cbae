"""The gradient planner, the part that needs no GPU (legged_gym_dev_amd/tube/plan.py, lg_plan_grad_check):
every refusal with the field named, on both sides and in the same words; lg_grad_cfg against the header; the restatement's float64
gradient (tests/plan_grad_ref.py) against central differences of its own J; its projected Adam on the fixed small problem, in
float64 and float32; ChainedPlanner on stubs; the script's --planner refusals."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

from tests import mppi_ref, plan_grad_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
from legged_gym_dev_amd import capi  # noqa: E402
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402
from legged_gym_dev_amd.tube.trainer import initial_params  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


# (changes to a valid configuration, B, the words the message must hold)
BAD = [(dict(iters=0), 1, "iters = 0"), (dict(iters=-3), 1, "iters = -3"), (dict(lr=0.0), 1, "lr must be positive"),
       (dict(lr=-0.1), 1, "lr must be positive"), (dict(lr=float("nan")), 1, "lr"), (dict(beta1=1.0), 1, "beta1"), (dict(beta1=-0.1), 1, "beta1"),
       (dict(beta2=1.0), 1, "beta2"), (dict(beta2=float("nan")), 1, "beta2"), (dict(eps=0.0), 1, "eps must be positive"),
       (dict(rho_g=-1.0), 1, "rho_g"), (dict(rho_w=-1.0), 1, "rho_w"), (dict(rho_z=-1e-3), 1, "rho_z"), (dict(), 0, "B = 0"),
       (dict(), 2 ** 31, "B = 2147483648")]


@pytest.mark.parametrize("change,B,word", BAD, ids=[f"{(list(c) or ['B'])[0]}-{i}" for i, (c, _, _) in enumerate(BAD)])
def test_refusals_name_the_field_on_both_sides(lib, change, B, word):
    cfg = pl.GradCfg(**change)
    with pytest.raises(ValueError) as ei:
        cfg.check(B)
    assert word in str(ei.value)
    prob = pl.PlanProblem.named("gap", tube_kind="l1", N=5).to_struct()
    assert lib.lg_plan_grad_check(C.byref(cfg.to_struct()), C.byref(prob), None, 0, B) == -1
    assert lib.lg_last_error().decode() == "lg_plan_grad: " + str(ei.value)       # the same words


def test_valid_configurations_pass_and_the_problem_is_checked_first(lib):
    prob = pl.PlanProblem.named("gap", tube_kind="l1", N=5)
    for kw in (dict(), dict(iters=1, beta1=0.0, beta2=0.0, rho_g=0.0), dict(lr=1e-6, eps=1e-12, rho_w=3.0, rho_z=2.0)):
        cfg = pl.GradCfg(**kw)
        cfg.check(3)
        assert lib.lg_plan_grad_check(C.byref(cfg.to_struct()), C.byref(prob.to_struct()), None, 0, 3) == 0
    cfg = pl.GradCfg()
    for change, word in ((dict(N=0), "N"), (dict(dt=0.0), "dt"), (dict(tube_kind="nn"), "handle")):
        st = pl.PlanProblem.named("gap", **{"tube_kind": "l1", "N": 5, **change}).to_struct()
        assert lib.lg_plan_grad_check(C.byref(cfg.to_struct()), C.byref(st), None, 0, 1) == -1
        assert lib.lg_last_error().decode().startswith("lg_plan: ") and word in lib.lg_last_error().decode()
    assert lib.lg_plan_grad_check(C.byref(cfg.to_struct()), C.byref(prob.to_struct()), None, 1, 1) == -1 and "level" in lib.lg_last_error().decode()
    # the entries refuse before they touch a device
    ps, cs, one = C.byref(prob.to_struct()), C.byref(cfg.to_struct()), C.byref(capi.lg_plan_call(count=1))
    assert lib.lg_plan_grad(None, ps, C.byref(pl.GradCfg(lr=0.0).to_struct()), one, *([None] * 6)) == -1
    assert "lr must be positive" in lib.lg_last_error().decode()
    assert lib.lg_plan_grad(None, ps, cs, one, *([None] * 6)) == -1 and "missing array" in lib.lg_last_error().decode()
    for what in (0, 2, 4):
        assert lib.lg_plan_descend_step(None, ps, cs, one, 0, what, 0, *([None] * 12)) == -1
        assert "what" in lib.lg_last_error().decode()
    assert lib.lg_plan_descend_step(None, ps, cs, one, -1, 3, 0, *([None] * 12)) == -1 and "it must" in lib.lg_last_error().decode()
    assert lib.lg_plan_descend_step(None, ps, cs, one, 0, 3, 0, *([None] * 12)) == -1
    assert "missing array" in lib.lg_last_error().decode()
    assert lib.lg_plan_descend(None, ps, C.byref(pl.GradCfg(iters=0).to_struct()), one, *([None] * 8)) == -1
    assert "iters = 0" in lib.lg_last_error().decode()


def test_struct_matches_the_header():
    fields = ("iters", "lr", "beta1", "beta2", "eps", "rho_g", "rho_w", "rho_z")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) + '\\n",sizeof(lg_grad_cfg),' + \
          ",".join(f"offsetof(lg_grad_cfg,{f})" for f in fields) + ');return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    c = capi.lg_grad_cfg
    assert out == [C.sizeof(c)] + [getattr(c, f).offset for f in fields]
    st = pl.GradCfg(iters=7, lr=0.25, beta1=0.5, beta2=0.75, eps=0.125, rho_g=3.0, rho_w=4.0, rho_z=5.0).to_struct()
    assert [getattr(st, f) for f in fields] == [7, 0.25, 0.5, 0.75, 0.125, 3.0, 4.0, 5.0]
    assert pl.GradCfg(iters=7).to_struct(iters=3).iters == 3


def _problem(N, kind, **kw):
    """tests/test_hip_mppi.py's problem: two obstacles, a tube bound and state bounds that bind."""
    return {**dict(N=N, H_rev=0, dt=0.1, goal=[1.0, 0.5], obs_c=[[0.2, 0.0], [0.5, 0.4]], obs_r=[0.1, 0.15], tube_kind=kind, scaling=0.5,
                   window_size=3, w_max=0.02, Qw=2.0, Q=[10.0, 1.0, 2.0, 10.0], Qf=[20.0, 0.0, 3.0, 15.0], R=[10.0, 0.5, 0.0, 8.0],
                   rom_z_min=[0.01, -0.05], rom_z_max=[0.35, 0.3], rom_v_min=[-1.0, -1.0], rom_v_max=[1.0, 1.0]), **kw}


@pytest.mark.parametrize("kind", ["l1", "l2", "l1_rolling", "l2_rolling", "nn-tanh", "nn-softplus", "nn-elu"])
def test_float64_gradient_against_central_differences(kind):
    B, N, Hr = 6, 5, 2
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    z0, v = (torch.tensor([0.3, 0.25]) + 0.1 * (r(B, 2) - 0.5)).float(), (0.8 * (2 * r(B, N, 2) - 1)).float()
    kw, p = {}, _problem(N, kind)
    if kind.startswith("nn"):
        p = _problem(N, "nn", H_rev=Hr)
        sd = initial_params(3 * Hr + 2 * N + 1, N, 16, 2, seed=3)
        kw = dict(model={"sd": sd, "act": kind[3:], "beta": 5.0}, e=0.1 * r(B, Hr), v_prev=0.2 * (2 * r(B, Hr, 2) - 1), level=0.85,
                  offset=np.linspace(-0.01, 0.05, N))
    rho = [50.0, 30.0, 7.0]
    w0 = (0.03 + 0.02 * r(B)).float()
    J, grad, parts = gr.value_and_grad(p, rho, z0, v, torch.float64, w0=w0, **kw)
    ok = parts["margin"] >= 1e-3
    assert ok.sum() >= 4 and (parts["pen"][ok] > 0).any(axis=0).all(), "the plans compared exercise all three hinge sums"
    h, vn = 1e-6, v.double().numpy()
    for b in np.nonzero(ok)[0]:
        for k in range(N):
            for d in range(2):
                up, dn = vn.copy(), vn.copy()
                up[b, k, d] += h
                dn[b, k, d] -= h
                fd = (gr.value_and_grad(p, rho, z0, up, torch.float64, w0=w0, **kw)[0][b] -
                      gr.value_and_grad(p, rho, z0, dn, torch.float64, w0=w0, **kw)[0][b]) / (2 * h)
                assert abs(fd - grad[b, k, d]) <= 1e-6 * max(1.0, np.abs(grad[b]).max()), (kind, b, k, d, fd, grad[b, k, d])


def test_restatement_adam_and_elite_by_hand():
    # first step of Adam from zero moments: m / bc1 = g, s / bc2 = g^2, so the step is lr g / (|g| + eps)
    v, g0 = np.array([[[0.5, -0.25]]]), np.array([[[2.0, -4.0]]])
    nv, m, s, x = gr.adam_step(v, g0, np.zeros_like(v), np.zeros_like(v), 1, 0.1, 0.9, 0.999, 1e-8, [-1.0, -1.0], [1.0, 1.0], np.float64)
    np.testing.assert_allclose(x, [[[0.4, -0.15]]], rtol=1e-6)
    np.testing.assert_allclose(m, 0.1 * g0, rtol=1e-6), np.testing.assert_allclose(s, 0.001 * g0 * g0, rtol=1e-4)
    nv, _, _, x = gr.adam_step(np.array([[[0.95, -0.95]]]), np.array([[[-1.0, 1.0]]]), m * 0, s * 0, 1, 0.1, 0.9, 0.999, 1e-8, [-1.0, -1.0], [1.0, 1.0])
    assert nv.dtype == np.float32 and nv.tolist() == [[[1.0, -1.0]]] and x[0, 0, 0] > 1.0                   # the projection
    J, plans = np.array([5.0, np.nan, 3.0], np.float32), np.arange(6, dtype=np.float32).reshape(3, 1, 2)
    bJ, bv = gr.elite(None, None, J, plans, True)
    assert bJ.tolist() == [5.0, np.inf, 3.0] and (bv == plans).all()
    bJ2, bv2 = gr.elite(bJ, bv, np.array([6.0, 2.0, np.inf], np.float32), plans + 10, False)
    assert bJ2.tolist() == [5.0, 2.0, 3.0] and (bv2[0] == plans[0]).all() and (bv2[1] == plans[1] + 10).all() and (bv2[2] == plans[2]).all()


SMALL = dict(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l2", scaling=0.02, Q=[10.0, 0, 0, 10.0],
             R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_the_small_problem_is_solved_by_projected_adam(dtype):
    """The fixed problem of tests/test_mppi_host.py from the clipped warm start (min_clear -0.0310, J 661.2): lr 0.05, 100
    iterations, rho_g = 1e4.  The elite clears the obstacle and brings J below a tenth -- 101 evaluations against MPPI's 5120."""
    p = pl.PlanProblem(**SMALL)
    d = p.to_json()
    d["Qf"] = d["Q"]
    v0 = np.clip(pl.warm_start("interpolate", p.start, p.goal, p.N, p.dt)[1], -2.0, 2.0).astype(np.float32)
    rho = [1e4, 0.0, 0.0]
    res, _, J0 = mppi_ref.score_J(d, p.start, v0[None], rho, np.float64)
    assert res["min_clear"][0] == pytest.approx(-0.0310, abs=5e-5) and J0[0] == pytest.approx(661.2, abs=0.05)
    z0 = np.asarray([p.start], np.float32)
    v, best_J, best_v, hist = gr.descend(d, rho, z0, v0[None], 100, 0.05, dtype=dtype)
    assert hist.shape == (101, 1, 2) and hist[0, 0, 0] == pytest.approx(J0[0], rel=1e-5)
    np.testing.assert_array_equal(best_J, hist[:, :, 0].min(axis=0))                # the elite is the running minimum
    res, _, J = mppi_ref.score_J(d, p.start, best_v.astype(np.float32), rho, np.float64)
    print(f"{np.dtype(dtype).name}: elite min_clear {res['min_clear'][0]:.4f}, J {J[0]:.2f} (from {J0[0]:.2f}); last iterate J {hist[-1, 0, 0]:.2f}")
    assert res["min_clear"][0] >= 0 and res["n_viol"][0, 0] == 0 and J[0] <= 0.1 * 661.2


class _Stub:
    def __init__(self, problem, tag):
        self.problem, self.device, self.tag, self.calls = problem, torch.device("cpu"), tag, []

    def plan(self, z0, v_init=None, e=None, v_prev=None, w0=None, iters=None):
        self.calls.append(dict(z0=z0, v_init=v_init, e=e, v_prev=v_prev, w0=w0, iters=iters))
        P = z0.shape[0]
        return {"v": torch.full((P, 3, 2), float(self.tag)), "best_v": torch.full((P, 3, 2), self.tag + 0.5), "best_J": torch.full((P,), float(self.tag)),
                "hist": torch.zeros(1, P, 2), "n_bad": torch.zeros(P, dtype=torch.int32), "score": {"tag": self.tag}, "best_score": {"tag": self.tag}}


def test_chained_planner_on_stubs():
    prob = types.SimpleNamespace(N=3, H_rev=0, dt=0.5)
    a, b = _Stub(prob, 1), _Stub(prob, 2)
    ch = pl.ChainedPlanner(a, b)
    assert ch.problem is prob and ch.device == torch.device("cpu")
    z0, e, vp, w0, vi = torch.zeros(2, 2), torch.zeros(2, 0), torch.zeros(2, 0, 2), torch.ones(2), torch.ones(2, 3, 2)
    sol = ch.plan(z0, vi, e, vp, w0, iters=7)
    assert a.calls == [dict(z0=z0, v_init=vi, e=e, v_prev=vp, w0=w0, iters=7)]
    c = b.calls[0]
    assert torch.equal(c["v_init"], torch.full((2, 3, 2), 1.5)) and c["iters"] is None            # first's best plan; second's own iterations
    assert c["z0"] is z0 and c["e"] is e and c["v_prev"] is vp and c["w0"] is w0
    assert set(sol) == {"v", "best_v", "best_J", "hist", "n_bad", "score", "best_score", "first"}
    assert sol["score"] == {"tag": 2} and sol["first"]["score"] == {"tag": 1} and float(sol["v"][0, 0, 0]) == 2.0
    with pytest.raises(ValueError, match="share one problem"):
        pl.ChainedPlanner(a, _Stub(types.SimpleNamespace(N=4, H_rev=0, dt=0.5), 3))


def test_script_planner_arguments():
    import plan_tube
    ok = ["--tube", "l1", "--problem", "gap"]
    for argv in (ok + ["--planner", "newton"], ok + ["--planner", "grad", "--lr", "0"], ok + ["--planner", "grad", "--grad_iters", "0"],
                 ok + ["--planner", "mppi+grad", "--lr", "-1"], ok + ["--planner", "mppi+grad", "--K", "33"],
                 ok + ["--planner", "grad", "--rho_g", "-1"]):
        with pytest.raises(SystemExit):
            plan_tube.parse_args(argv)
    a = plan_tube.parse_args(ok)
    assert a.planner == "mppi" and (a.lr, a.grad_iters) == (pl.GradCfg().lr, pl.GradCfg().iters)
    a = plan_tube.parse_args(ok + ["--planner", "mppi+grad", "--lr", "0.02", "--grad_iters", "30", "--rho_w", "2"])
    g = plan_tube.grad_cfg(a)
    assert (a.planner, g.lr, g.iters, g.rho_g, g.rho_w) == ("mppi+grad", 0.02, 30, plan_tube.mppi_cfg(a).rho_g, 2.0)
    assert plan_tube.parse_args(ok + ["--planner", "grad", "--K", "33"]).K == 33                  # MPPI's settings are not read
