"""tube_kind 'nn_step' on the GPU (k_plan_score_step, k_plan_sample_score_step): the tube values against
the closed-loop roll-out on host-built rows on the bits, tile independence, the nodes on the bits, fw / cost / clearance / tube nodes
against the float64 restatement (tests/plan_step_ref.py, tests/plan_ref.py) under the chain yardstick of sections 10.1 and 10.9, the
counts, the fused sampler against lg_plan_score on its candidates, the refusals that need a handle, the older kinds' bits, and
train_tube.py -> calibrate_tube.py --by_age -> plan_tube.py --closed_loop --w0 error -> audit_plans.py end to end, and
audit_plans.py --robot on a step run."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import plan_ref, plan_step_ref as sr, tube_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))


def _trainer(I, U, L, act, beta=1.0, level=False, seed=4, O=1, horizon=None):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    loss = ("scalar_level" if level else "scalar") if horizon is None else "scalar_horizon"
    return HipTubeTrainer(I, O, num_units=U, num_layers=L, activation=act, softplus_beta=beta, loss=loss, alpha=0.9, batch_size=32, seed=seed,
                          horizon=horizon, device=DEV)


def _problem(N, Hr, recursive, **kw):
    from legged_gym_dev_amd.tube.plan import PlanProblem
    return PlanProblem.named("gap", **{"N": N, "H_rev": Hr, "tube_kind": "nn_step", "recursive": recursive, **kw})


def _plans(B, N, Hr, seed, scale=0.2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    return {"z0": 0.3 + 0.2 * (r(B, 2) - 0.5), "v": scale * (2 * r(B, N, 2) - 1), "e": 0.1 * r(B, Hr), "v_prev": scale * (2 * r(B, Hr, 2) - 1),
            "w0": 0.05 * r(B)}


def _same(a, b, what=""):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), what


def _rollout(tr, x, T, recursive):
    """The contract's right-hand side: the existing closed loop on host-built rows, no reseed."""
    out = tr.rollout_window(x, 1, T, 1, 3) if recursive else tr.rollout(x, 1)
    return out[:, :, 0]


def _mlp(tr, dtype):
    I, O, U, L = tr.dims
    r = tube_ref.MLP(I, O, U, L, tr.activation, tr.softplus_beta).to(dtype)
    r.load_state_dict({k: v.to(dtype).cpu() for k, v in tr.state_dict().items()})
    return r


# ---------------------------------------------------------------- 1. fw against the roll-out, z against a float32 loop
# (input_dim, units, layers, activation, beta, recursive, conditioned) -> T.  The last row is wider than 32 columns: the row build
# leaves the sources kept in registers for the per-element path.
MODELS = [(3, 16, 1, "relu", 1.0, False, False), (7, 32, 2, "tanh", 1.0, False, False), (9, 32, 2, "relu", 1.0, True, False),
          (31, 128, 2, "softplus", 5.0, True, True), (35, 16, 1, "relu", 1.0, False, False)]


@pytest.mark.parametrize("case", MODELS, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-{'recursive' if c[5] else 'plain'}" for c in MODELS])
def test_fw_equals_the_rollout_on_host_built_rows(case):
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    I, U, L, act, beta, rec, level = case
    T = sr.taps(I, level, rec)
    lv = 0.85 if level else None
    tr = _trainer(I, U, L, act, beta, level)
    try:
        for N in (1, 5, 64):
            for Hr in (T - 1, T + 1):
                p = _problem(N, Hr, rec)
                sc = HipPlanScorer(tr, p, level=lv)
                for B in (1, 31, 33, 65):
                    d = _plans(B, N, Hr, seed=B + N)
                    for given in (True, False):
                        e, vp, w0 = (d["e"], d["v_prev"], d["w0"]) if given else (None, None, None)
                        got = sc.score(d["z0"], d["v"], e, vp, w0)
                        ze, zv, zw = (d["e"], d["v_prev"], d["w0"]) if given else (torch.zeros(B, Hr), torch.zeros(B, Hr, 2), torch.zeros(B))
                        want = _rollout(tr, sr.rows(ze, zv, zw, d["v"], T, rec, lv), T, rec)
                        what = f"N {N}, H_rev {Hr}, B {B}, given {given}"
                        assert bool(torch.isfinite(got["fw"]).all()), what
                        _same(got["fw"], want, "fw: " + what)
                        z, dt = [d["z0"]], torch.tensor(p.dt, dtype=torch.float32)
                        for k in range(N):
                            z.append(z[-1] + dt * d["v"][:, k])
                        _same(got["z"], torch.stack(z, dim=1), "z: " + what)
                        _same(got["w"], torch.cat([zw[:, None], want.cpu()], dim=1), "w: " + what)
        if T > 1:                                                            # the delayed taps are really read
            d = _plans(5, 5, T - 1, seed=1)
            a = HipPlanScorer(tr, _problem(5, T - 1, rec), level=lv).score(d["z0"], d["v"], d["e"], d["v_prev"], d["w0"])["fw"]
            b = HipPlanScorer(tr, _problem(5, T - 1, rec), level=lv).score(d["z0"], d["v"], d["e"], d["v_prev"] + 0.1, d["w0"])["fw"]
            assert not torch.equal(a[:, 0], b[:, 0])
    finally:
        tr.close()


def test_a_plan_does_not_depend_on_its_place_in_the_batch():
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    for I, rec in ((7, False), (9, True)):
        T = sr.taps(I, False, rec)
        Hr, N = T + 1, 5
        tr = _trainer(I, 32, 2, "tanh")
        try:
            sc = HipPlanScorer(tr, _problem(N, Hr, rec, Qw=2.0), device=DEV)
            d = _plans(65, N, Hr, seed=9)
            for k in d:                                                  # the same plan at positions 0, 31 (tile 0) and 32 (tile 1)
                d[k][31], d[k][32] = d[k][0], d[k][0]
            args = (d["z0"], d["v"], d["e"], d["v_prev"], d["w0"])
            big, one = sc.score(*args), sc.score(*[a[:1] for a in args])
            for name, t in big.items():
                _same(t[0], t[31], f"{name}: position 31"), _same(t[0], t[32], f"{name}: position 32")
                _same(t[:1], one[name], f"{name}: a batch of one")
        finally:
            tr.close()


def _age_calibration(offsets):
    from legged_gym_dev_amd.tube.calibrate import AgeCalibration
    A = len(offsets)
    return AgeCalibration([0.9], torch.tensor(offsets, dtype=torch.float32).reshape(1, A, 1), [100] * A, [[91]] * A)


def test_tube_nodes_add_the_offset_in_float32():
    from legged_gym_dev_amd.tube.calibrate import Calibration
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    N, Hr = 6, 2
    tr = _trainer(9, 32, 2, "relu")
    try:
        d = _plans(33, N, Hr, seed=2)
        args = (d["z0"], d["v"], d["e"], d["v_prev"], d["w0"])
        raw = HipPlanScorer(tr, _problem(N, Hr, True)).score(*args)
        age = _age_calibration([0.25, -0.01, 0.03, 0.125])               # max_age 4: nodes 3, 4, 5 share the last group
        flat = Calibration("flat", [0.9], torch.tensor([[[0.05]], [[0.2]]]), 10, [9])
        for calib, want in ((age, [0.25, -0.01, 0.03, 0.125, 0.125, 0.125]), (flat, [0.05, 0.2, 0.2, 0.2, 0.2, 0.2])):
            sc = HipPlanScorer(tr, _problem(N, Hr, True), calibration=calib, coverage=0.9)
            _same(sc.offset, torch.tensor(want).to(DEV), "offsets")
            got = sc.score(*args)
            _same(got["fw"], raw["fw"], "the raw value is fed back, never the calibrated one")
            _same(got["w"][:, 1:], raw["fw"] + torch.tensor(want).to(DEV), "w = fw + offset")
            _same(got["w"][:, 0], d["w0"].to(DEV), "w[0] = w0")
    finally:
        tr.close()


# ---------------------------------------------------------------- 2. fw, cost, clearance and the tube nodes against float64
def _ref_problem(p):
    d = p.to_json()
    d["Qf"] = d["Qf"] if d["Qf"] is not None else d["Q"]
    return d


def _yardstick(name, got, r32, r64):
    """The chain yardstick of DESIGN.md sections 10.1 / 10.9: e32 = max |float32 restatement - float64|, the device within 4 e32."""
    fin = np.isfinite(r64)
    assert (np.asarray(got)[~fin] == r64[~fin]).all(), name
    e32 = float(np.abs(r32.astype(np.float64) - r64)[fin].max()) if fin.any() else 0.0
    ours = float(np.abs(np.asarray(got, np.float64) - r64)[fin].max()) if fin.any() else 0.0
    print(f"{name}: e32 = {e32:.3e}, device / e32 = {ours / e32 if e32 else 0:.2f}")
    if e32 == 0:
        assert ours == 0, name
    else:
        assert ours <= 4 * e32, (name, ours, e32)


YARD = [(7, 32, 2, "tanh", 1.0, False), (30, 32, 2, "softplus", 5.0, True)]


@pytest.mark.parametrize("case", YARD, ids=["plain-T3", "recursive-T10"])
def test_fw_cost_clearance_and_tube_against_float64(case):
    """Both restatements run the whole chain at their own precision: the literal loop of tests/plan_step_ref.py through the torch
    MLP, then the walk of tests/plan_ref.py on that loop's fw."""
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    I, U, L, act, beta, rec = case
    T, N, B = sr.taps(I, False, rec), 16, 257
    Hr = T + 1
    tr = _trainer(I, U, L, act, beta)
    try:
        p = _problem(N, Hr, rec, Qw=3.0, Qf=[20.0, 1.0, 1.0, 30.0], Q=[10.0, 0.5, 0.5, 8.0], R=[4.0, 0.0, 0.25, 6.0])
        offs = [-0.01 + 0.004 * k for k in range(N)]
        sc = HipPlanScorer(tr, p, calibration=_age_calibration(offs), coverage=0.9, device=DEV)
        d = _plans(B, N, Hr, seed=17)
        got = {k: t.cpu().numpy() for k, t in sc.score(d["z0"], d["v"], d["e"], d["v_prev"], d["w0"]).items()}
        rp, res = _ref_problem(p), {}
        with torch.no_grad():
            for D, TD in ((np.float32, torch.float32), (np.float64, torch.float64)):
                fw = sr.roll(_mlp(tr, TD), *(d[k].to(TD) for k in ("e", "v_prev", "w0", "v")), T, rec).numpy()
                res[D] = {"fw": fw, **plan_ref.score(rp, d["z0"].numpy(), d["v"].numpy(), fw, d["w0"].numpy(), np.asarray(offs, np.float32), D)}
        for name in ("fw", "cost", "min_clear", "w"):
            _yardstick(f"{case[0]}-{'rec' if rec else 'plain'} {name}", got[name], res[np.float32][name], res[np.float64][name])
    finally:
        tr.close()


def _count_case():
    """512 random plans of 16 nodes near three obstacles, with input, state and tube bounds that a part of them crosses."""
    from legged_gym_dev_amd.tube.plan import PlanProblem
    N, B, Hr = 16, 512, 2
    p = PlanProblem(N=N, H_rev=Hr, dt=0.1, goal=[1.0, 1.0], obs_c=[[0.45, 0.3], [0.3, 0.55], [0.1, 0.1]], obs_r=[0.08, 0.1, 0.05],
                    tube_kind="nn_step", recursive=True, w_max=COUNT_W_MAX, rom_z_min=[0.22, 0.22], rom_z_max=[0.4, 0.4], rom_v_min=[-0.2, -0.2],
                    rom_v_max=[0.2, 0.2])
    return p, _plans(B, N, Hr, seed=24, scale=0.25)


COUNT_W_MAX = 0.13                  # between the quantiles of the untrained model's fw; the float32 restatement leaves out 0.59 % of these plans


def test_counts_and_worst_node_equal_the_float64_walk_on_the_device_fw():
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    p, d = _count_case()
    tr = _trainer(9, 32, 2, "relu")
    try:
        got = HipPlanScorer(tr, p, device=DEV).score(d["z0"], d["v"], d["e"], d["v_prev"], d["w0"], want=("fw",))
        fw = got["fw"].cpu().numpy()
        r64 = plan_ref.score(_ref_problem(p), d["z0"].numpy(), d["v"].numpy(), fw, d["w0"].numpy(), None, np.float64)
        gmargin, bmargin = r64["margin"]
        keep = (gmargin >= 1e-5) & (bmargin >= 1e-6)
        print(f"left out: {1 - keep.mean():.4f} of the plans")
        assert keep.mean() >= 0.99, f"{1 - keep.mean():.4f} of the plans lie within the margins"
        nv = r64["n_viol"][keep]
        assert all(len(np.unique(nv[:, j])) >= 4 for j in range(4)), "every count takes several values over the plans"
        per_node = np.sort(r64["g"].min(axis=2), axis=1)
        assert (per_node[keep, 1] - per_node[keep, 0]).min() >= 1e-5, "two nodes tie for the smallest clearance: choose other plans"
        np.testing.assert_array_equal(got["n_viol"].cpu().numpy()[keep], nv)
        np.testing.assert_array_equal(got["worst_node"].cpu().numpy()[keep], r64["worst_node"][keep])
        assert len(np.unique(r64["worst_node"][keep])) > 4
    finally:
        tr.close()


# ---------------------------------------------------------------- 3. the fused sampler
@pytest.mark.parametrize("rec", [False, True], ids=["plain", "recursive"])
@pytest.mark.parametrize("P,K", [(1, 32), (3, 96)])
def test_fused_scores_equal_lg_plan_score_on_the_candidates(P, K, rec):
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    I, N = (9, 8) if rec else (7, 8)
    T = sr.taps(I, False, rec)
    Hr = T
    tr = _trainer(I, 32, 2, "relu")
    try:
        p = _problem(N, Hr, rec, goal=[1.0, 0.5], obs_c=[[0.2, 0.0], [0.5, 0.4]], obs_r=[0.1, 0.15], w_max=-1.0, rom_z_min=[-0.05, -0.3],
                     rom_z_max=[0.2, 0.35], rom_v_min=[-1.0, -1.0], rom_v_max=[1.0, 1.0])
        cfg = MppiCfg(K=K, sigma=0.2, sigma_decay=0.5, seed=5, rho_g=1e4, rho_w=30.0, rho_z=7.0, instance_offset=3)
        pln = HipMppiPlanner(tr, p, cfg, calibration=_age_calibration([0.01, 0.02, 0.03]), coverage=0.9, device=DEV)
        g = torch.Generator().manual_seed(K)
        d = _plans(P, N, Hr, seed=K)
        z0 = torch.zeros(P, 2)
        vbar = torch.tensor([0.5, 0.0]).repeat(P, N, 1) + 0.05 * torch.randn(P, N, 2, generator=g)
        it = 1
        st = pln.step(pln.state(z0, vbar, d["e"], d["v_prev"], d["w0"], want=("cost", "min_clear", "pen")), it, what=1)
        _same(st["vbar"], vbar, "the score leaves the mean plans alone")
        cand = pln.candidates(vbar, it)
        rep = lambda t: t.repeat_interleave(K, dim=0)
        sc = pln.scorer.score(rep(z0), cand.reshape(P * K, N, 2), rep(d["e"]), rep(d["v_prev"]), rep(d["w0"]))
        _same(st["cost"].reshape(-1), sc["cost"], "cost")
        _same(st["min_clear"].reshape(-1), sc["min_clear"], "min_clear")
        cost, pen = st["cost"].cpu(), st["pen"].cpu()
        rho = [torch.tensor(x, dtype=torch.float32) for x in (cfg.rho_g, cfg.rho_w, cfg.rho_z)]
        _same(st["J"], ((cost + rho[0] * pen[..., 0]) + rho[1] * pen[..., 1]) + rho[2] * pen[..., 2], "J")
        # pen: the three hinge sums formed in float32 from lg_plan_score's own nodes, nodes ascending, obstacles ascending per node
        z, w = sc["z"].cpu(), sc["w"].cpu()
        f = lambda x: torch.tensor(x, dtype=torch.float32)
        pg, pw, pz = torch.zeros(P * K), torch.zeros(P * K), torch.zeros(P * K)
        for k in range(N + 1):
            for c, r in zip(p.obs_c, p.obs_r):
                dx, dy, rr = z[:, k, 0] - f(c[0]), z[:, k, 1] - f(c[1]), f(r) + w[:, k]
                pg = pg + torch.clamp(-((dx * dx + dy * dy) - rr * rr), min=0)
            pw = pw + torch.clamp(w[:, k] - f(p.w_max), min=0)
            for a in range(2):
                pz = pz + (torch.clamp(z[:, k, a] - f(p.rom_z_max[a]), min=0) + torch.clamp(f(p.rom_z_min[a]) - z[:, k, a], min=0))
        _same(st["pen"].reshape(P * K, 3), torch.stack([pg, pw, pz], dim=1), "pen")
        assert all(bool((st["pen"][..., c] > 0).any()) for c in range(3)), "every penalty binds somewhere"
    finally:
        tr.close()


def test_plan_is_bit_identical_over_two_runs():
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    tr = _trainer(9, 32, 2, "relu")
    try:
        p = _problem(8, 2, True, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], rom_v_min=[-1.5, -1.5], rom_v_max=[1.5, 1.5])
        pln = HipMppiPlanner(tr, p, MppiCfg(K=64, iters=5, sigma=0.3, seed=2, lambda_=10.0), device=DEV)
        z0 = torch.tensor([[0.0, 0.0], [0.0, 0.05]])
        a, b = pln.plan(z0), pln.plan(z0)
        for k in ("v", "best_v", "best_J", "hist", "n_bad"):
            _same(a[k], b[k], k)
        for k in ("cost", "min_clear", "z", "w"):
            _same(a["score"][k], b["score"][k], k)
        assert not torch.equal(a["v"], torch.as_tensor(pln.warm_start(z0.numpy())).to(DEV))
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. refusals that need a handle; the older kinds' bits
def test_refusals():
    from legged_gym_dev_amd import capi
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.calibrate import Calibration
    flat, cond = _trainer(9, 16, 1, "relu"), _trainer(10, 16, 1, "relu", level=True)
    hor = _trainer(3 + 2 * 8, 16, 1, "relu", O=5, horizon=(5, 3))
    two = _trainer(9, 16, 1, "relu", O=2)
    odd = _trainer(8, 16, 1, "relu")
    lib = flat.lib
    err = lambda: lib.lg_last_error().decode()
    check = lambda h, p, has: lib.lg_plan_check(C.byref(p.to_struct()), h, has)
    try:
        assert check(flat.h, _problem(5, 2, True), 0) == 0 and check(flat.h, _problem(5, 3, False), 0) == 0     # 9 = 3 * 3 = 1 + 2 * 4
        assert check(cond.h, _problem(5, 2, True), 1) == 0
        assert check(None, _problem(5, 2, True), 0) == -1 and "handle" in err()
        assert check(hor.h, _problem(5, 3, True), 0) == -1 and "is a horizon handle" in err()
        nn = pl.PlanProblem.named("gap", N=5, H_rev=3)
        assert check(flat.h, nn, 0) == -1 and "not a horizon handle" in err()
        assert check(two.h, _problem(5, 2, True), 0) == -1 and "output_dim" in err()
        assert check(odd.h, _problem(5, 2, True), 0) == -1 and "input_dim" in err() and "recursive" in err()
        assert check(odd.h, _problem(5, 2, False), 0) == -1 and "input_dim" in err() and "recursive" in err()
        assert check(flat.h, _problem(5, 1, True), 0) == -1 and "H_rev" in err()
        assert check(flat.h, _problem(5, 2, False), 0) == -1 and "H_rev" in err()                                # T = 4 needs 3
        assert check(flat.h, _problem(5, 65, True), 0) == -1 and "H_rev" in err()
        assert check(flat.h, _problem(65, 2, True), 0) == -1 and "N" in err()
        assert check(flat.h, _problem(5, 2, True), 1) == -1 and "not level-conditioned" in err()
        assert check(cond.h, _problem(5, 2, True), 0) == -1 and "level is missing" in err()
        st = _problem(5, 2, True).to_struct()
        st.recursive = 2
        assert lib.lg_plan_check(C.byref(st), flat.h, 0) == -1 and "recursive" in err()
        st.recursive, st.tube_kind = 1, 6
        assert lib.lg_plan_check(C.byref(st), flat.h, 0) == -1 and "tube_kind" in err()
        for model, p, level, word in ((hor, _problem(5, 3, True), None, "is a horizon model"), (flat, nn, None, "not a horizon model"),
                                      (two, _problem(5, 2, True), None, "output_dim"), (odd, _problem(5, 2, True), None, "input_dim"),
                                      (flat, _problem(5, 1, True), None, "H_rev"), (flat, _problem(5, 2, True), 0.9, "level"),
                                      (cond, _problem(5, 2, True), None, "level")):
            with pytest.raises(ValueError, match=word):
                pl.HipPlanScorer(model, p, level=level)
        with pytest.raises(ValueError, match="'horizon' calibration"):
            pl.HipPlanScorer(flat, _problem(5, 2, True), calibration=Calibration("horizon", [0.9], torch.zeros(1, 5), 10, [9]))
        # the gradient planner
        gcfg = pl.GradCfg(iters=2)
        p = _problem(5, 2, True)
        d = {k: t.to(DEV) for k, t in _plans(2, 5, 2, seed=1).items()}
        J, grad = torch.empty(2, device=DEV), torch.empty(2, 5, 2, device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert lib.lg_plan_grad_check(C.byref(gcfg.to_struct()), C.byref(p.to_struct()), flat.h, 0, 2) == -1
        assert "nn_step" in err() and "chained MLP passes" in err()
        call = capi.lg_plan_call(z0=d["z0"].data_ptr(), count=2)
        assert lib.lg_plan_grad(flat.h, C.byref(p.to_struct()), C.byref(gcfg.to_struct()), C.byref(call), ptr(d["v"]),
                                ptr(J), ptr(grad), None, None, None) == -1 and "chained MLP passes" in err()
        with pytest.raises(ValueError, match="chained MLP passes"):
            pl.HipGradPlanner(flat, p, gcfg)
        mp = pl.HipMppiPlanner(flat, p, pl.MppiCfg(K=32, iters=1), device=DEV)
        import types
        with pytest.raises(ValueError, match="chained MLP passes"):
            pl.ChainedPlanner(mp, types.SimpleNamespace(problem=p, device=mp.device, needs_gradient=True))
        pl.ChainedPlanner(mp, mp)
        assert capi.PLAN_TUBE["nn_step"] == 5
    finally:
        for t in (flat, cond, hor, two, odd):
            t.close()


def test_the_older_kinds_keep_their_bits_with_the_former_pad_at_zero():
    """One nn and one l1 case of lg_plan_score and lg_plan_mppi_step: `recursive`, the struct's former pad, is not read by them."""
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg, PlanProblem
    Hr, N = 3, 5
    tr = _trainer(Hr + 2 * (Hr + N), 16, 1, "relu", O=N, horizon=(N, Hr))
    try:
        for kind, model, hr in (("nn", tr, Hr), ("l1", None, 0)):
            d = _plans(33, N, hr, seed=3)
            out = []
            for rec in (False, True):
                p = PlanProblem.named("gap", N=N, H_rev=hr, tube_kind=kind, recursive=rec)
                assert p.to_struct().recursive == int(rec)
                pln = HipMppiPlanner(model, p, MppiCfg(K=32, seed=1), device=DEV)
                hist = (d["e"], d["v_prev"]) if model else (None, None)
                s = pln.scorer.score(d["z0"], d["v"], *hist, d["w0"])
                st = pln.step(pln.state(d["z0"][:2], d["v"][:2], *[h[:2] if h is not None else None for h in hist], d["w0"][:2],
                                        want=("cost", "min_clear", "pen")), 1, what=1)
                out.append({**s, **{"mppi_" + k: st[k] for k in ("J", "cost", "min_clear", "pen")}})
            for k in out[0]:
                _same(out[0][k], out[1][k], f"{kind} {k}")
    finally:
        tr.close()


# ---------------------------------------------------------------- 5. end to end, structure only
def test_scripts_on_a_trained_default_tube(tmp_path):
    """The default scalar tube (3 -> 32 x 2 ReLU -> 1) trained from the simulator at the smallest shape of the other end-to-end tests,
    calibrated per age, planned with in closed loop from the tracking error, its plans audited.  No coverage is promised."""
    import audit_plans
    import calibrate_tube
    import plan_tube
    import train_tube
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.calibrate import AgeCalibration, default_age_path
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    run, out = str(tmp_path / "run"), str(tmp_path / "plan")
    sim_flags = ["--sim_envs", "64", "--sim_T", "50"]
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--dataset", "scalar", "--out", run, "--num_epochs", "2", "--batch_size", "128",
                     "--lr", "3e-3", "--seed", "3", "--steps_per_model_checkpoint", "10", "--steps_per_model_evaluation", "10", "--device", DEV]
                    + sim_flags)
    calibrate_tube.main(["--run", run, "--sim", "--checkpoint", "latest", "--coverage", "0.9", "--by_age", "--max_age", "6", "--device", DEV] + sim_flags)
    prob = pl.PlanProblem.named("gap", N=6, goal=[0.35, 0.36], obs_c=[[0.36, 0.28], [0.28, 0.37]], obs_r=[0.02, 0.03])
    pj = str(tmp_path / "problem.json")
    json.dump(prob.to_json(), open(pj, "w"))
    argv = ["--run", run, "--checkpoint", "latest", "--problem", pj, "--N", "6", "--age_calibration", "--coverage", "0.9", "--K", "64", "--iters", "4",
            "--sigma", "0.05", "--rho_g", "1e4", "--starts", "3", "--start_noise", "0.01", "--seed", "4", "--closed_loop", "5", "--w0", "error",
            "--device", DEV]
    got = plan_tube.main(argv + ["--out", out])
    saved = json.load(open(os.path.join(out, "plan.json")))
    assert saved == json.loads(json.dumps(got, allow_nan=False)) == got
    assert got["closed_loop"] == 5 and got["audit"]["robots"] == 3 and got["audit"]["steps"] == 5 and got["calibrated"] is True
    assert got["tube"] == "nn_step" and got["w0"] == "error" and got["problem"]["recursive"] is False and got["problem"]["H_rev"] == 0
    a = plan_tube.parse_args(argv)
    p = plan_tube.build_problem(a, audit_plans.run_config(run))
    assert p.tube_kind == "nn_step" and p.N == 6
    calib = AgeCalibration.load(default_age_path(run))
    model, sim = HipTubeModel.load(run, checkpoint="latest", device=DEV), HipRomSim(audit_plans.sim_config(a, p), device=DEV)
    try:
        pln = pl.HipMppiPlanner(model, p, plan_tube.mppi_cfg(a), calibration=calib, coverage=0.9, device=DEV)
        res = pl.closed_loop(pln, sim, 5, plan_tube.starts(a, p), keep_plans=True, w0="error")
        assert pl.audit_closed_loop(res, p) == got["audit"]
        zero = pl.closed_loop(pln, sim, 5, plan_tube.starts(a, p), keep_plans=True)
        assert not torch.equal(zero["plans_w"][1:, :, 0], res["plans_w"][1:, :, 0])         # the replannings start at the error
        _same(res["plans_w"][1:, :, 0], torch.linalg.vector_norm(res["z"][:, 1:5] - res["pz_x"][:, 1:5], dim=-1).t(), "w0 = |z_k - pz_x_k|")
        assert not bool(zero["plans_w"][:, :, 0].any())
        for k in (0, 4):                                                 # calibrated w >= raw w wherever the offset is >= 0
            raw = pl.HipPlanScorer(model, p, device=DEV).score(res["plans_z"][k, :, 0], res["plans_v"][k], w0=res["plans_w"][k, :, 0])
            off = pln.scorer.offset
            _same(res["plans_w"][k][:, 1:], raw["fw"] + off, "the plan's tube is the raw roll plus the per-age offset")
            assert bool((res["plans_w"][k][:, 1:][:, off >= 0] >= raw["fw"][:, off >= 0]).all())
    finally:
        model.close()
        sim.close()
    f = os.path.join(out, "plans.npz")
    z = np.load(f)
    assert z["z0"].shape == (15, 2) and z["v"].shape == (15, 6, 2)
    np.testing.assert_array_equal(z["v"], res["plans_v"].reshape(15, 6, 2).cpu().numpy())
    aargv = ["--run", run, "--checkpoint", "latest", "--problem_json", pj, "--N", "6", "--age_calibration", "--coverage", "0.9", "--plans", f, "--device", DEV]
    aud = audit_plans.main(aargv + ["--out", str(tmp_path / "audit")])
    assert json.load(open(os.path.join(str(tmp_path / "audit"), "audit.json"))) == json.loads(json.dumps(aud, allow_nan=False)) == aud
    assert aud["plans"] == 15 and aud["nodes"] == 7 and aud["source"] == {"plans_file": f} and aud["tube"] == "nn_step" and aud["calibrated"] is True
    # the same through the library
    model, sim = HipTubeModel.load(run, checkpoint="latest", device=DEV), HipRomSim(audit_plans.sim_config(audit_plans.parse_args(aargv), p), device=DEV)
    try:
        s = pl.HipPlanScorer(model, p, calibration=calib, coverage=0.9, device=DEV).score(torch.as_tensor(z["z0"]), torch.as_tensor(z["v"]))
        lib_aud = pl.audit(s, pl.track(sim, s["z"], torch.as_tensor(z["v"])), p)
        assert all(aud[k] == v for k, v in lib_aud.items())
    finally:
        model.close()
        sim.close()
    shares = [got["audit"][k] for k in ("coverage", "covered_robots", "actually_safe", "predicted_safe", "reached_goal")] + \
             [aud[k] for k in ("coverage", "covered_plans", "predicted_safe", "actually_safe")] + list(aud["table"].values()) + aud["coverage_by_node"]
    assert all(0.0 <= x <= 1.0 for x in shares)
    print(f"closed loop on the trained one-step tube: coverage {got['audit']['coverage']:.3f}, actually safe {got['audit']['actually_safe']:.2f}; "
          f"its plans audited open loop: coverage {aud['coverage']:.3f}")


def test_audit_script_on_the_robot_with_a_step_run(tmp_path):
    """audit_plans.py --robot on a step run (an untrained recursive T = 3 tube: no training is needed to see the plumbing): the robot's
    own e_past, v_prev and w0 reach the roll, and audit.json is track_env + score + audit_env."""
    import audit_plans
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import initial_params
    run, out = tmp_path / "run", str(tmp_path / "audit")
    run.mkdir()
    torch.save(initial_params(9, 1, 32, 2, 3), str(run / "model.pth"))
    (run / "config.json").write_text(json.dumps({"dataset": "scalar", "N": 3, "dN": 1, "recursive": True, "H_fwd": 50, "H_rev": 10,
                                                 "activation": "relu", "softplus_beta": 1.0}))
    prob = pl.PlanProblem.named("gap", N=5, goal=[0.35, 0.36], obs_c=[[0.36, 0.28], [0.28, 0.37]], obs_r=[0.02, 0.03])
    pj = str(tmp_path / "problem.json")
    json.dump(prob.to_json(), open(pj, "w"))
    argv = ["--run", str(run), "--checkpoint", "latest", "--problem_json", pj, "--N", "5", "--H_rev", "3", "--warm_start", "interpolate",
            "--perturb", "32", "--sigma", "0.05", "--seed", "4", "--device", DEV, "--robot"]
    res = audit_plans.main(argv + ["--out", out])
    assert json.load(open(os.path.join(out, "audit.json"))) == json.loads(json.dumps(res, allow_nan=False)) == res
    assert res["tracker"] == "robot" and res["plans"] == 33 and res["nodes"] == 6 and res["tube"] == "nn_step"
    assert res["problem"]["H_rev"] == 3 and res["problem"]["recursive"] is True
    a = audit_plans.parse_args(argv)
    p = audit_plans.build_problem(a, audit_plans.run_config(str(run)))
    z0, v, _ = audit_plans.build_plans(a, p)
    model = HipTubeModel.load(str(run), checkpoint="latest", device=DEV)
    try:
        s, lib, extra = audit_plans.main_robot(a, p, pl.HipPlanScorer(model, p, device=DEV), z0, v)
    finally:
        model.close()
    assert extra["tracker"] == "robot"
    for k, val in lib.items():
        assert res[k] == val, k
