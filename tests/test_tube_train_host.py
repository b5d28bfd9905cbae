"""CPU-only checks of tests/tube_train_ref.py: every condition that tests/test_hip_tube_train.py's cases rest on is asserted here on the
reference alone, so a case can never quietly stop testing what it claims to -- the coverage of the case list, the kink filter, the
sentinel rows (a row lost at a tile edge is a failure), the saturation shares, the exact family's representability and ties, the Adam
regimes, the StepLR boundary and the trajectories' kink condition.  Each sensitivity assertion fails when the reference is mutated the
way its name says: drop a sentinel row, flip one tie rule, use the logged lr for the update."""
import math

import numpy as np
import pytest
import torch

from tests import tube_train_ref as tt


# ---------------------------------------------------------------- 1. step cases
def test_case_list_covers_what_it_must():
    cs = tt.STEP_CASES
    flat_ = {(c[2], c[3]) for c in cs if c[1] == "rand" and c[9] is None}
    assert {(l, a) for l in ("scalar", "vector", "error") for a in ("relu", "softplus", "tanh", "elu")} <= flat_
    assert {"scalar_level", "vector_level"} <= {c[2] for c in cs if c[9] is None}
    assert {c[2] for c in cs if c[9] is not None} == {"scalar_horizon", "scalar_level"} and tt.HORIZON_ENVS >= 70
    assert {1, 31, 32, 33, 63, 65, 2047, 2048} <= {c[4] for c in cs} and max(c[4] for c in cs) == 2048
    assert (256, 64, 128, 4) in {c[5:9] for c in cs} and (3, 1, 16, 1) in {c[5:9] for c in cs}
    assert {c[3] for c in cs if c[1] == "saturated"} == {"softplus", "tanh", "elu"}


@pytest.mark.parametrize("name", tt.STEP_IDS)
def test_step_case_conditions(name):
    """Kink filter: 7/8 of the pool survives and every batch row clears KINK.  Sentinels: removing the term of a row at a tile edge
    from the float64 gradient, at the unchanged norm, moves it by at least 16 x the bound the device is held to."""
    c = tt.case(name)
    assert int(c.pool_survives.sum()) * 8 >= c.pool * 7, (int(c.pool_survives.sum()), c.pool)
    rows = tt.select_rows(c)
    assert rows.numel() == c.B and rows.unique().numel() == c.B
    ref = tt.step_reference(c, rows)
    assert bool((ref.margins >= c.kink).all()) and ref.margins.numel() == c.B
    assert ref.mean64 == pytest.approx(ref.l64, rel=1e-13)                          # terms.sum() / norm is tube_ref's mean
    whole, blocks = ref.e32
    gmax = float(np.abs(ref.g64).max())
    assert 0 < whole < 2e-5 * gmax and bool((blocks > 0).all()), (whole, gmax)
    # the two fp32 restatements (fmaf chains in the kernel's order: the yardstick; autograd per tile) are evaluations of one arithmetic
    both = max(whole, ref.e32_auto[0])
    assert float(np.abs(ref.yard.astype(np.float64) - ref.auto).max()) <= 2 * tt.MARGIN * both
    assert whole < 8 * ref.e32_auto[0] and ref.e32_auto[0] < 8 * whole, (whole, ref.e32_auto[0])
    print(f"{name}: kink {c.kink:.2e}, survivors {int(c.pool_survives.sum())}/{c.pool}, e32/max|g| {whole / gmax:.2e} (autograd per tile {ref.e32_auto[0] / gmax:.2e}), "
          f"loss e32 {ref.loss_e32 / abs(ref.l64):.2e}")
    for p, move in ref.sentinels.items():
        print(f"  sentinel {p}: moves the gradient by {move / (tt.MARGIN * whole):.0f} x the bound")
        assert move >= tt.SENTINEL_FACTOR * tt.MARGIN * whole, (p, move, whole)
    if c.B > 1:                      # the mutation: a reference that drops a sentinel row lies outside the bound by that factor
        p = tt.sentinel_positions(c.B)[-1]
        keep = [i for i in range(c.B) if i != p]
        a = ref.a64[keep] if torch.is_tensor(ref.a64) else ref.a64
        g, _ = tt.grad_whole(c.m64, c.loss, ref.x64[keep], ref.y64[keep], a, c.delta, ref.norm)
        assert tt.grad_ratios(g.numpy(), ref.g64, ref.e32, c.dims)[0] >= tt.SENTINEL_FACTOR


def _first_layer(c, ref, n=0):
    with torch.no_grad():
        return c.m64.layers[n](ref.x64)


def test_saturated_family_reaches_the_output_formed_derivatives():
    """softplus: at least 5 % of first-layer pre-activations beyond the threshold (beta z > 20); tanh outputs beyond 0.999; ELU
    pre-activations below -5."""
    c = tt.case("sat-softplus")
    ref = tt.step_reference(c, tt.select_rows(c))
    share = float((c.beta * _first_layer(c, ref) > 20).double().mean())
    assert c.beta == 5.0 and share >= 0.05, share
    c = tt.case("sat-tanh")
    ref = tt.step_reference(c, tt.select_rows(c))
    h = torch.tanh(_first_layer(c, ref))
    with torch.no_grad():
        h2 = torch.tanh(c.m64.layers[2](h))
    t_share = float(((h.abs() > 0.999).double().mean() + (h2.abs() > 0.999).double().mean()) / 2)
    assert t_share >= 0.05, t_share
    c = tt.case("sat-elu")
    ref = tt.step_reference(c, tt.select_rows(c))
    e_share = float((_first_layer(c, ref) < -5).double().mean())
    assert e_share >= 0.05, e_share
    print(f"saturated shares: softplus {share:.3f}, tanh {t_share:.3f}, elu {e_share:.3f}")


# ---------------------------------------------------------------- 2. the exact family
def _representable(v):
    v = np.asarray(v, dtype=np.float64)
    return bool((v.astype(np.float32).astype(np.float64) == v).all())


@pytest.mark.parametrize("name", tt.EXACT_IDS)
def test_exact_case_conditions(name):
    c = tt.exact_case(name)
    O = c.dims[1]
    assert c.norm & (c.norm - 1) == 0 and O in (1, 2, 4)
    g64, l64 = tt.exact_reference(c)
    assert _representable(g64) and _representable(l64) and np.abs(g64).max() > 0
    # float32 autograd lands on it exactly, in another row order too
    g32, l32 = tt.grad_whole(c.m32, c.loss, c.x, c.y, c.alpha, c.delta, c.norm)
    assert np.array_equal(g32.double().numpy(), g64) and float(l32) == l64
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(1))
    g32p, l32p = tt.grad_whole(c.m32, c.loss, c.x[perm], c.y[perm], c.alpha, c.delta, c.norm)
    assert np.array_equal(g32p.double().numpy(), g64) and float(l32p) == l64
    g32t, l32t = tt.grad_tiles(c.m32, c.loss, c.x, c.y, c.alpha, c.delta, c.norm)
    assert np.array_equal(g32t.double().numpy(), g64) and float(l32t) == l64
    gc, lc = tt.grad_chains(c, c.x.numpy(), c.y.numpy(), c.alpha, c.norm)          # the kernel's order, with its tie rules
    assert np.array_equal(gc.astype(np.float64), g64) and float(lc) == l64
    # the hand-written backward with torch's tie rules is autograd, exactly
    rows, t, z, r, l = tt.manual_grad(c, c.x, c.y, per_row=True)
    assert np.array_equal(rows.sum(axis=0), g64) and float(t.sum()) == l64
    # any fp32 summation order is exact: on the grid of the terms every partial sum stays below 2^24 grid steps
    q = tt.pow2_divisor(rows)
    assert float(np.abs(rows).sum(axis=0).max()) / q < 2.0 ** 24, (q, float(np.abs(rows).sum(axis=0).max()))
    assert float(np.abs(t).sum()) / tt.pow2_divisor(t) < 2.0 ** 24
    # ties present, and each one the case pins decides the gradient
    zeros = sum(int((zi == 0).sum()) for zi in z)
    assert zeros > 0
    flips = [("elu0", 0.0)] if c.act == "elu" else [("relu0", 1.0)]
    if r is not None:
        assert int((r == 0).sum()) > 0 and int((np.abs(l) == c.delta).sum()) > 0, (int((r == 0).sum()), int((np.abs(l) == c.delta).sum()))
        if tt.kernel_loss(c.loss) == "vector":          # scalar: l = 0 there, and Huber's derivative clamp(l) is 0 whatever dl/dfw is
            flips.append(("pin0", 1.0 - c.alpha))
    if c.act == "elu":
        assert min(float(zi.min()) for zi in z) >= 0
    for key, val in flips:
        g, _, _, _, _ = tt.manual_grad(c, c.x, c.y, ties={**tt.TIES, key: val})
        assert not np.array_equal(g, g64), f"{name}: flipping {key} leaves the gradient unchanged"


def test_exact_family_covers_its_ties():
    assert {(c[1], c[2]) for c in tt.EXACT_CASES} >= {("scalar", "relu"), ("vector", "relu"), ("error", "relu"), ("scalar", "elu")}
    assert {c[3] for c in tt.EXACT_CASES} == {32, 64, 2048}
    elu = [c for c in tt.EXACT_CASES if c[2] == "elu"]
    assert all(c[7] == 1 for c in elu)


# ---------------------------------------------------------------- 4. Adam
def test_adam_restatements_agree():
    """adam64 is torch.optim.Adam in float64; adam32 (the yardstick) sits at fp32 distance from it."""
    g = np.random.default_rng(0)
    p, m, v, gr = g.standard_normal(50), 1e-3 * g.standard_normal(50), 1e-6 * g.random(50), 1e-2 * g.standard_normal(50)
    for t in (1, 2, 1000, 10 ** 6):
        a = tt.adam64(p, m, v, gr, t, 1e-3)
        q = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = torch.optim.Adam([q], lr=1e-3, foreach=False)
        opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
        q.grad = torch.from_numpy(gr.copy())
        opt.step()
        np.testing.assert_allclose(a["params"], q.detach().numpy(), rtol=0, atol=1e-15)
        np.testing.assert_allclose(a["v"], opt.state[q]["exp_avg_sq"].numpy(), rtol=1e-14)
        b = tt.adam32(p.astype(np.float32), m.astype(np.float32), v.astype(np.float32), gr.astype(np.float32), t, 1e-3)
        np.testing.assert_allclose(b["params"], a["params"], rtol=0, atol=1e-6)


def test_adam_case_regimes():
    assert {c[1] for c in tt.ADAM_CASES} >= {1, 2, 1000, 10 ** 6}
    assert {c[2] for c in tt.ADAM_CASES} == {False, True} and any(c[3] for c in tt.ADAM_CASES)
    for name in tt.ADAM_IDS:
        c = tt.adam_case(name)
        dead = c.dead
        assert dead.sum() > 0 and bool((c.g64[dead] == 0).all()) and bool((c.m0[dead] == 0).all()) and bool((c.v0[dead] == 0).all())
        assert bool((c.g64[~dead] != 0).mean() > 0.5)
        before = dict(params=c.p0, m=c.m0, v=c.v0)
        ref, yard, e32 = tt.adam_one_step(before, c.g64.astype(np.float32), c.t, c.lr, c.dims)
        assert np.array_equal(ref["params"][dead], c.p0[dead].astype(np.float64)) and bool(np.isfinite(ref["params"]).all())
        assert np.array_equal(yard["params"][dead], c.p0[dead])
        if c.tiny:                       # eps decides: sqrt(v-hat) below eps for most live elements
            vhat = ref["v"] / (1.0 - 0.999 ** c.t)
            share = float((np.sqrt(vhat[~dead]) < 1e-8).mean())
            assert share > 0.5, share
        else:
            assert float(np.abs(ref["params"] - c.p0).max()) > 0.5 * c.lr * (0.01 if c.warm else 1.0)
        r = tt.adam_ratios(yard, ref, e32, c.dims)
        assert max(r.values()) <= 1.0 / tt.MARGIN + 1e-12, r


def test_steplr_boundary_is_visible():
    """The rate that sizes step t is lr0 gamma^((t - 1) // 3); the log holds lr0 gamma^(t // 3).  At t = 3, 6, 9 the two differ, and a
    reference stepping with the logged rate lies far outside the bound."""
    s = tt.STEPLR
    c = tt.adam_case("t1-fresh")
    state = dict(params=c.p0, m=c.m0, v=c.v0)
    g = c.g64.astype(np.float32)
    seen = 0
    for t in range(1, s["steps"] + 1):
        sized, logged = tt.lr_of_step(s["lr0"], s["gamma"], s["step_size"], t), tt.lr_logged(s["lr0"], s["gamma"], s["step_size"], t)
        ref, yard, e32 = tt.adam_one_step(state, g, t, sized, c.dims)
        assert (sized != logged) == (t % 3 == 0)
        if sized != logged:
            wrong = tt.adam64(state["params"], state["m"], state["v"], g, t, logged)
            assert tt.adam_ratios(dict(wrong, m=ref["m"], v=ref["v"]), ref, e32, c.dims)["params"] >= 16.0
            seen += 1
        state = {a: yard[a] for a in ("params", "m", "v")}
    assert seen == 3
    assert tt.lr_logged(s["lr0"], s["gamma"], s["step_size"], 10) == s["lr0"] / 8 and tt.lr_of_step(s["lr0"], s["gamma"], s["step_size"], 10) == s["lr0"] / 8
    assert tt.lr_of_step(s["lr0"], s["gamma"], s["step_size"], 3) == s["lr0"]


@pytest.mark.parametrize("name", tt.TRAJ_IDS)
def test_trajectory_conditions(name):
    tr = tt.trajectory(name)
    counts = [int(s["rows"].numel()) for s in tr.steps]
    assert len(counts) == tt.TRAJ_STEPS == 20 and len(set(counts)) == 5
    if tr.loss == "error":
        assert set(counts) == {2048, 33, 1, 64, 2047}
    else:
        assert max(counts) <= 65 and tr.dims[1] == 1 and tr.beta == 5.0
        assert tr.min_r >= tt.KINK_FACTOR * tr.out_diff, (tr.min_r, tr.out_diff)    # no batch row crosses the pinball kink
    last = tr.steps[-1]
    moved = float(np.abs(last["ref"]["params"] - tt.flat(tr.sd).double().numpy()).max())
    assert moved > 5 * tr.lr and last["e32"]["params"][0] < 1e-3 * moved
    print(f"{name}: min |w - fw| {tr.min_r:.2e}, output difference {tr.out_diff:.2e}, params moved {moved:.2e}, "
          f"e32 {last['e32']['params'][0]:.2e}")


# ---------------------------------------------------------------- 5. eval
@pytest.mark.parametrize("name", tt.EVAL_IDS)
def test_eval_case_conditions(name):
    c = tt.eval_case(name)
    assert c.pool_survivors * 8 >= tt.EVAL_POOL * 7 and c.tx.shape[0] == c.n
    assert c.same_side                                  # the kink filter's purpose: fp32 and float64 count the same elements
    assert c.mean64 == pytest.approx(c.l64, rel=1e-13)
    if c.n > 1:
        assert 0 < c.count64 < c.elems
    if name == "n8225":
        assert math.ceil(c.n / tt.R) == 258 and c.dims == (3, 1, 16, 1)
    print(f"{name}: count {c.count64}/{c.elems}, loss e32 {c.loss_e32 / abs(c.l64):.2e}" +
          (f", err e32 {c.err_e32 / abs(c.err64):.2e}" if c.count64 else ""))


def test_eval_sizes():
    assert {c[3] for c in tt.EVAL_CASES} >= {1, 31, 33, 8225} and max(c[3] for c in tt.EVAL_CASES) == 8225
    assert any(c[1] == "scalar_level" for c in tt.EVAL_CASES)
    assert set(tt.PERM_SIZES) == {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097}
