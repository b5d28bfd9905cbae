"""lg_plan_score on the GPU (k_plan_score): the tube values against the window queries on the bits, the ROM
nodes against a float32 loop on the bits, tile independence, cost / clearance / tube nodes against the float64 restatement
(tests/plan_ref.py) under the chain yardstick of sections 10.1 and 10.2, the counts against the float64 restatement's, the analytic
tubes, the obstacle cases and the refusals that need a handle."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _trainer(Hr, N, U, L, act, beta=1.0, level=False, seed=4):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    return HipTubeTrainer(Hr + 2 * (Hr + N) + int(level), N, num_units=U, num_layers=L, activation=act, softplus_beta=beta,
                          loss="scalar_level" if level else "scalar_horizon", alpha=0.9, batch_size=32, seed=seed, horizon=(N, Hr), device=DEV)


def _problem(N, Hr, **kw):
    from legged_gym_dev_amd.tube.plan import PlanProblem
    return PlanProblem.named("gap", **{"N": N, "H_rev": Hr, **kw})


def _plans(B, N, Hr, seed, scale=0.2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    return {"z0": 0.3 + 0.2 * (r(B, 2) - 0.5), "v": scale * (2 * r(B, N, 2) - 1), "e": 0.1 * r(B, Hr), "v_prev": scale * (2 * r(B, Hr, 2) - 1),
            "w0": 0.05 * r(B)}


def _window_ds(e, v_prev, v, N, Hr):
    w, vv = plan_ref.window_arrays(e.numpy(), v_prev.numpy(), v.numpy())
    B = v.shape[0]
    return types.SimpleNamespace(H_fwd=N, H_rev=Hr, w=torch.from_numpy(w), z=torch.zeros(B, Hr + N, 0), v=torch.from_numpy(vv))


def _same(a, b, what=""):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), what


# ---------------------------------------------------------------- 1. fw against the window queries, z against a float32 loop
# (H_rev, N, units, layers, activation, beta, batch sizes); the last is the reference one-shot shape, once
BITS = [(3, 5, 16, 1, "relu", 1.0, (1, 31, 33, 65)), (1, 64, 32, 2, "tanh", 1.0, (1, 31, 33, 65)), (10, 50, 128, 2, "softplus", 5.0, (33,))]


BITS_CASES = [(c, lv) for c in BITS for lv in (False, True) if not (lv and c[2] == 128)]


@pytest.mark.parametrize("case,level", BITS_CASES, ids=[f"Hrev{c[0]}-N{c[1]}-{c[2]}x{c[3]}-{'conditioned' if lv else 'plain'}" for c, lv in BITS_CASES])
def test_fw_equals_the_window_query_and_z_the_float32_loop(case, level):
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    Hr, N, U, L, act, beta, counts = case
    tr = _trainer(Hr, N, U, L, act, beta, level)
    lv = 0.85 if level else None
    try:
        p = _problem(N, Hr)
        sc = HipPlanScorer(tr, p, level=lv)
        for B in counts:
            d = _plans(B, N, Hr, seed=B)
            for given in (True, False):
                e, vp, w0 = (d["e"], d["v_prev"], d["w0"]) if given else (None, None, None)
                got = sc.score(d["z0"], d["v"], e, vp, w0)
                ze, zv = (d["e"], d["v_prev"]) if given else (torch.zeros(B, Hr), torch.zeros(B, Hr, 2))
                ds = _window_ds(ze, zv, d["v"], N, Hr)
                env, start = torch.arange(B, dtype=torch.int32), torch.full((B,), Hr, dtype=torch.int32)
                want = tr.predict_windows_levels(ds, env, start, [lv])[:, 0, :] if level else tr.predict_windows(ds, env, start)
                _same(got["fw"], want, f"fw: B {B}, given {given}")
                # nodes: z[k+1] = z[k] + dt * v[k], a multiply and an add; w[0] = w0, w[k+1] = fw[k]
                z, dt = [d["z0"]], torch.tensor(p.dt, dtype=torch.float32)
                for k in range(N):
                    z.append(z[-1] + dt * d["v"][:, k])
                _same(got["z"], torch.stack(z, dim=1), f"z: B {B}")
                _same(got["w"], torch.cat([(d["w0"] if given else torch.zeros(B))[:, None], want.cpu()], dim=1), f"w: B {B}")
    finally:
        tr.close()


def test_a_plan_does_not_depend_on_its_place_in_the_batch():
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    Hr, N = 3, 5
    tr = _trainer(Hr, N, 32, 2, "tanh")
    try:
        for kind, model in (("nn", tr), ("l2_rolling", None)):
            sc = HipPlanScorer(model, _problem(N, Hr if model else 0, tube_kind=kind, window_size=3, Qw=2.0), device=DEV)
            d = _plans(65, N, Hr if model else 0, seed=9)
            for k in d:                                                  # the same plan at positions 0, 31 (tile 0) and 32 (tile 1)
                d[k][31], d[k][32] = d[k][0], d[k][0]
            args = (d["z0"], d["v"], d["e"], d["v_prev"], d["w0"]) if model else (d["z0"], d["v"], None, None, d["w0"])
            big, one = sc.score(*args), sc.score(*[a[:1] if a is not None else None for a in args])
            for name, t in big.items():
                _same(t[0], t[31], f"{kind} {name}: position 31"), _same(t[0], t[32], f"{kind} {name}: position 32")
                _same(t[:1], one[name], f"{kind} {name}: a batch of one")
    finally:
        tr.close()


# ---------------------------------------------------------------- 2. cost, clearance and the tube nodes against float64
def _ref_problem(p):
    d = p.to_json()
    d["Qf"] = d["Qf"] if d["Qf"] is not None else d["Q"]
    return d


def _yardstick(name, got, r32, r64):
    """The chain yardstick of DESIGN.md sections 10.1 / 10.2: e32 = max |float32 restatement - float64|, the device within 4 e32."""
    fin = np.isfinite(r64)
    assert (np.asarray(got)[~fin] == r64[~fin]).all(), name
    e32 = float(np.abs(r32.astype(np.float64) - r64)[fin].max()) if fin.any() else 0.0
    ours = float(np.abs(np.asarray(got, np.float64) - r64)[fin].max()) if fin.any() else 0.0
    print(f"{name}: e32 = {e32:.3e}, device / e32 = {ours / e32 if e32 else 0:.2f}")
    if e32 == 0:
        assert ours == 0, name
    else:
        assert ours <= 4 * e32, (name, ours, e32)


@pytest.mark.parametrize("kind", ["nn", "l1"])
def test_cost_clearance_and_tube_against_float64(kind):
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    Hr, N, B = (3, 16, 257) if kind == "nn" else (0, 16, 257)
    tr = _trainer(Hr, N, 32, 2, "softplus", 5.0) if kind == "nn" else None
    try:
        p = _problem(N, Hr, tube_kind=kind, Qw=3.0, Qf=[20.0, 1.0, 1.0, 30.0], Q=[10.0, 0.5, 0.5, 8.0], R=[4.0, 0.0, 0.25, 6.0])
        offset = torch.linspace(-0.01, 0.05, N)
        from legged_gym_dev_amd.tube.calibrate import Calibration
        sc = HipPlanScorer(tr, p, calibration=Calibration("horizon", [0.9], offset[None], 100, [91]), device=DEV)
        d = _plans(B, N, Hr, seed=17)
        got = {k: t.cpu().numpy() for k, t in sc.score(d["z0"], d["v"], d["e"] if tr else None, d["v_prev"] if tr else None, d["w0"]).items()}
        fw = got["fw"] if kind == "nn" else None
        rp, res = _ref_problem(p), {}
        for D in (np.float32, np.float64):
            f = fw if fw is not None else plan_ref.analytic(kind, d["v"].numpy(), p.scaling, p.window_size, D)
            res[D] = plan_ref.score(rp, d["z0"].numpy(), d["v"].numpy(), f, d["w0"].numpy(), offset.numpy(), D)
        for name in ("cost", "min_clear", "w"):
            _yardstick(f"{kind} {name}", got[name], res[np.float32][name], res[np.float64][name])
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 3. the counts and the worst node
def _count_case():
    """512 random plans of 16 nodes near three obstacles, with input, state and tube bounds that a part of them crosses."""
    from legged_gym_dev_amd.tube.plan import PlanProblem
    N, B = 16, 512
    p = PlanProblem(N=N, dt=0.1, goal=[1.0, 1.0], obs_c=[[0.45, 0.3], [0.3, 0.55], [0.1, 0.1]], obs_r=[0.08, 0.1, 0.05], tube_kind="l1",
                    scaling=0.5, w_max=0.2, rom_z_min=[0.22, 0.22], rom_z_max=[0.4, 0.4], rom_v_min=[-0.2, -0.2], rom_v_max=[0.2, 0.2])
    d = _plans(B, N, 0, seed=23, scale=0.25)
    return p, d


def test_counts_and_worst_node_equal_the_float64_restatement():
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    p, d = _count_case()
    fw64 = plan_ref.analytic("l1", d["v"].numpy(), p.scaling, 1, np.float64)
    r64 = plan_ref.score(_ref_problem(p), d["z0"].numpy(), d["v"].numpy(), fw64, d["w0"].numpy(), None, np.float64)
    gmargin, bmargin = r64["margin"]
    keep = (gmargin >= 1e-5) & (bmargin >= 1e-6)
    assert keep.mean() >= 0.99, f"the restatement leaves out {1 - keep.mean():.4f} of the plans"
    nv = r64["n_viol"][keep]
    assert all(len(np.unique(nv[:, j])) >= 4 for j in range(4)), "every count takes several values over the plans"
    # worst_node is a first arg-min: the inputs must not leave it to rounding.  No plan is left out for this; the plans themselves
    # are checked to hold no two nodes whose smallest g lie within 1e-5 of each other at the minimum.
    per_node = np.sort(r64["g"].min(axis=2), axis=1)
    assert (per_node[keep, 1] - per_node[keep, 0]).min() >= 1e-5, "two nodes tie for the smallest clearance: choose other plans"
    got = HipPlanScorer(None, p, device=DEV).score(d["z0"], d["v"], None, None, d["w0"], want=())
    np.testing.assert_array_equal(got["n_viol"].cpu().numpy()[keep], nv)
    np.testing.assert_array_equal(got["worst_node"].cpu().numpy()[keep], r64["worst_node"][keep])
    assert len(np.unique(r64["worst_node"][keep])) > 4


# ---------------------------------------------------------------- 4. analytic tubes and obstacle cases
@pytest.mark.parametrize("window", [1, 3, 20])
@pytest.mark.parametrize("kind", ["l1", "l2", "l1_rolling", "l2_rolling"])
def test_analytic_tubes(kind, window):
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    N, B = 7, 33
    p = _problem(N, 0, tube_kind=kind, scaling=0.7, window_size=window)
    d = _plans(B, N, 0, seed=window)
    got = HipPlanScorer(None, p, device=DEV).score(d["z0"], d["v"], None, None, None)
    f32, f64 = (plan_ref.analytic(kind, d["v"].numpy(), 0.7, window, D) for D in (np.float32, np.float64))
    _yardstick(f"{kind} window {window} fw", got["fw"].cpu().numpy(), f32, f64)
    _same(got["w"][:, 1:], got["fw"]), _same(got["w"][:, 0], torch.zeros(B, device=DEV))
    if not kind.endswith("rolling") or window == 1:
        plain = plan_ref.analytic(kind[:2], d["v"].numpy(), 0.7, 1, np.float64)
        np.testing.assert_allclose(f64, plain, rtol=1e-15)                   # a window of one is the plain tube
    else:
        assert np.abs(f64[:, 1:] - plan_ref.analytic(kind[:2], d["v"].numpy(), 0.7, 1, np.float64)[:, 1:]).max() > 1e-3


@pytest.mark.parametrize("n_obs", [0, 1, 8])
def test_obstacle_counts(n_obs):
    from legged_gym_dev_amd.tube.plan import HipPlanScorer, PlanProblem
    N, B = 6, 40
    g = torch.Generator().manual_seed(n_obs)
    oc = (torch.rand(n_obs, 2, generator=g) * 0.6).tolist()
    p = PlanProblem(N=N, dt=0.1, goal=[1.0, 1.0], obs_c=oc, obs_r=[0.05 + 0.01 * i for i in range(n_obs)], tube_kind="l2", scaling=0.5)
    d = _plans(B, N, 0, seed=5)
    got = {k: t.cpu().numpy() for k, t in HipPlanScorer(None, p, device=DEV).score(d["z0"], d["v"], None, None, None).items()}
    if n_obs == 0:
        assert np.isposinf(got["min_clear"]).all() and (got["worst_node"] == -1).all() and not got["n_viol"][:, 0].any()
        return
    res = {D: plan_ref.score(_ref_problem(p), d["z0"].numpy(), d["v"].numpy(), plan_ref.analytic("l2", d["v"].numpy(), 0.5, 1, D), None, None, D)
           for D in (np.float32, np.float64)}
    _yardstick(f"{n_obs} obstacles min_clear", got["min_clear"], res[np.float32]["min_clear"], res[np.float64]["min_clear"])
    assert (got["worst_node"] >= 0).all() and (got["worst_node"] <= N).all()


def test_a_plan_through_an_obstacle_is_flagged_and_the_shifted_one_is_not():
    from legged_gym_dev_amd.tube.plan import HipPlanScorer, PlanProblem, warm_start
    N, r = 10, 0.2
    p = PlanProblem(N=N, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.0]], obs_r=[r], tube_kind="l1", scaling=0.1)
    _, v = warm_start("interpolate", p.start, p.goal, N, p.dt)
    v = torch.as_tensor(v, dtype=torch.float32)[None].repeat(2, 1, 1)
    z0 = torch.tensor([[0.0, 0.0], [0.0, 10 * r]])                          # the second plan runs 10 radii beside the first
    got = HipPlanScorer(None, p, device=DEV).score(z0, v)
    mc, nv, wn = got["min_clear"].cpu(), got["n_viol"].cpu(), got["worst_node"].cpu()
    w = 0.1 * 1.0                                                            # scaling * (|1.0| + |0|)
    assert float(mc[0]) == pytest.approx(-(r + w) ** 2, rel=1e-5) and int(wn[0]) == 5 and int(nv[0, 0]) >= 3
    assert float(mc[1]) == pytest.approx((10 * r) ** 2 - (r + w) ** 2, rel=1e-5) and int(nv[1, 0]) == 0
    assert float(got["cost"][0]) < float(got["cost"][1])                    # the shifted plan ends farther from the goal


# ---------------------------------------------------------------- 5. refusals that need a handle
def test_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    from legged_gym_dev_amd.tube.plan import HipPlanScorer
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    from legged_gym_dev_amd.tube.calibrate import Calibration
    Hr, N = 3, 5
    plain, cond = _trainer(Hr, N, 16, 1, "relu"), _trainer(Hr, N, 16, 1, "relu", level=True)
    flat = HipTubeTrainer(19, 5, num_units=16, num_layers=1, batch_size=32, device=DEV)
    wide = HipTubeTrainer(Hr + 2 + 2 * (Hr + N), N, num_units=16, num_layers=1, loss="scalar_horizon", batch_size=32, horizon=(N, Hr), device=DEV)
    lib = plain.lib
    err = lambda: lib.lg_last_error().decode()
    check = lambda h, p, has: lib.lg_plan_check(C.byref(p.to_struct()), h, has)
    try:
        assert check(plain.h, _problem(N, Hr), 0) == 0 and check(cond.h, _problem(N, Hr), 1) == 0
        assert check(flat.h, _problem(N, Hr), 0) == -1 and "horizon" in err()
        assert check(plain.h, _problem(4, Hr), 0) == -1 and "H_fwd" in err()
        assert check(plain.h, _problem(N, 2), 0) == -1 and "H_rev" in err()
        assert check(wide.h, _problem(N, Hr), 0) == -1 and "nz" in err() and "input_dim" in err()
        assert check(plain.h, _problem(N, Hr), 1) == -1 and "level" in err() and "not level-conditioned" in err()
        assert check(cond.h, _problem(N, Hr), 0) == -1 and "level is missing" in err()
        assert check(None, _problem(N, Hr), 0) == -1 and "handle" in err()
        for model, level, word in ((flat, None, "horizon"), (plain, 0.9, "level"), (cond, None, "level"), (wide, None, "nz")):
            with pytest.raises(ValueError, match=word):
                HipPlanScorer(model, _problem(N, Hr), level=level)
        c = Calibration("flat", [0.9], torch.zeros(2, 1, 1), 10, [9])
        with pytest.raises(ValueError, match="'flat' calibration"):
            HipPlanScorer(plain, _problem(N, Hr), calibration=c)
        with pytest.raises(ValueError, match="steps ahead"):
            HipPlanScorer(plain, _problem(N, Hr), calibration=Calibration("horizon", [0.9], torch.zeros(1, 4), 10, [9]))
        sc = HipPlanScorer(plain, _problem(N, Hr), calibration=Calibration("horizon", [0.9], torch.full((1, N), 0.25), 10, [9]))
        d = _plans(3, N, Hr, seed=1)
        raw = HipPlanScorer(plain, _problem(N, Hr)).score(d["z0"], d["v"])
        _same(sc.score(d["z0"], d["v"])["w"][:, 1:], raw["fw"] + 0.25, "the offset is added per step ahead")
        with pytest.raises(ValueError, match="v must be"):
            sc.score(d["z0"], d["v"][:, :4])
        z0, v = d["z0"].to(DEV), d["v"].to(DEV)
        st = _problem(N, Hr).to_struct()
        from legged_gym_dev_amd import capi
        call = lambda B: C.byref(capi.lg_plan_call(z0=z0.data_ptr(), count=B))
        assert lib.lg_plan_score(plain.h, C.byref(st), call(3), C.c_void_p(v.data_ptr()),
                                 None, None, None, None, None, None, None) == -1 and "missing array" in err()
        assert lib.lg_plan_score(plain.h, C.byref(st), call(0), C.c_void_p(v.data_ptr()),
                                 None, None, None, None, None, None, None) == -1 and "B must be" in err()
        assert LeggedHipError is not None
    finally:
        for t in (plain, cond, flat, wide):
            t.close()
