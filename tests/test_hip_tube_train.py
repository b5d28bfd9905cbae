"""The single tube trainer (k_tube_rows, k_tube_adam, k_tube_eval_finish, k_tube_wt, k_tube_perm through HipTubeTrainer) against
float64 under the fp32 yardstick of tests/tube_train_ref.py: one step's gradient, loss and norm on every loss x activation, the level
and horizon kinds, batch counts off and on every tile edge, saturated activations; the tie rules and the row accounting on the bits
(the exact family, rows outside the split); identities that need no tolerance (stale slab rows, the transposed weight copy, the
epoch permutation); one Adam step in isolation, StepLR, two 20-step trajectories; the eval metrics up to a second trip of the
finish kernel's loop.  The conditions every case rests on are asserted on the CPU by tests/test_tube_train_host.py.

Every yardstick comparison prints device error / e32; the bound is 4."""
import math

import numpy as np
import pytest
import torch

from tests import tube_train_ref as tt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _trainer(c, **kw):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    I, O, U, L = c.dims
    hz = getattr(c, "horizon", None)
    kw = {**dict(lr=0.0, batch_size=2048, seed=3, alpha=getattr(c, "alpha", None), delta=getattr(c, "delta", 1.0)), **kw}
    if getattr(c, "level", False):
        kw.update(level_lo=tt.LEVEL_LO, level_hi=tt.LEVEL_HI)
    tr = HipTubeTrainer(I, O, num_units=U, num_layers=L, activation=c.act, softplus_beta=getattr(c, "beta", 1.0), loss=c.loss,
                        horizon=(hz[0], hz[1]) if hz else None, device=DEV, **kw)
    tr.load_state_dict(c.sd)
    return tr


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _norm_check(log, grads64, P):
    n64 = math.sqrt(float((grads64 * grads64).sum()))
    return abs(float(log[2]) - n64) / max(n64, 1e-300) / tt.norm_rtol(P)


# ---------------------------------------------------------------- 1. step gradient and loss under the yardstick
@pytest.mark.parametrize("name", tt.STEP_IDS)
def test_step_gradient_loss_and_norm(name):
    c = tt.case(name)
    B = c.B
    tr = _trainer(c)
    try:
        tr.set_data(c.ds if c.horizon else tt.Flat(c.x, c.y))
        starts = levels = None
        if c.horizon or c.level:          # the draws depend on (seed, step count, position) only: read them, then replay the step
            tr.step(rows=c.order[:B].to(torch.int32).to(DEV))
            torch.cuda.synchronize()
            starts = tr.starts[:B].cpu().clone() if c.horizon else None
            levels = tr.read_levels(B).clone() if c.level else None
            tr.set_step(0)
        rows = tt.select_rows(c, starts, levels)
        tr.step(rows=rows.to(DEV))
        torch.cuda.synchronize()
        if c.horizon:
            assert torch.equal(tr.starts[:B].cpu(), starts)
            assert bool(((starts >= c.horizon[1]) & (starts < tt.HORIZON_T - c.horizon[0] - 1)).all()) and starts.unique().numel() > 4
        if c.level:
            _same(tr.read_levels(B), levels, "levels of the replayed step")
            assert bool(((levels >= tt.LEVEL_LO) & (levels < tt.LEVEL_HI)).all()) and levels.unique().numel() > B // 2
        ref = tt.step_reference(c, rows, starts, levels)
        assert bool((ref.margins >= c.kink).all()) and rows.unique().numel() == B        # every batch row is compared
        for p, move in ref.sentinels.items():
            assert move >= tt.SENTINEL_FACTOR * tt.MARGIN * ref.e32[0], (p, move, ref.e32[0])
        got = tr.grads.cpu().double().numpy()
        log = tr.read_log(1, 1)[0]
        whole, block = tt.grad_ratios(got, ref.g64, ref.e32, c.dims)
        lratio = abs(float(log[0]) - ref.l64) / ref.loss_e32
        nratio = _norm_check(log, got, got.size)
        print(f"\n{name}: grad device/e32 {tt.MARGIN * whole:.2f} (blocks {tt.MARGIN * block:.2f}), e32/max|g| "
              f"{ref.e32[0] / np.abs(ref.g64).max():.2e}, loss device/e32 {lratio:.2f}, norm err/bound {nratio:.2f}")
        assert whole <= 1.0 and block <= 1.0, (whole, block)
        assert lratio <= tt.MARGIN, lratio
        assert nratio <= 1.0, nratio
        assert float(log[3]) == B
    finally:
        tr.close()


# ---------------------------------------------------------------- 2. ties and row accounting on the bits
@pytest.mark.parametrize("name", tt.EXACT_IDS)
def test_exact_family_equals_float64_on_the_bits(name):
    c = tt.exact_case(name)
    g64, l64 = tt.exact_reference(c)
    tr = _trainer(c)
    try:
        tr.set_data(tt.Flat(c.x, c.y), tt.Flat(c.x, c.y))
        tr.step(rows=torch.arange(c.B, dtype=torch.int32).to(DEV))
        ev = tr.evaluate().cpu()
        got, log = tr.grads.cpu().double().numpy(), tr.read_log(1, 1)[0]
        bad = np.nonzero(got != g64)[0]
        assert bad.size == 0, (bad[:8], got[bad[:8]], g64[bad[:8]])
        assert float(log[0]) == l64 and float(log[3]) == c.B
        assert float(ev[0]) == l64 and float(ev[3]) == c.B
    finally:
        tr.close()


def test_row_ids_outside_the_split_are_zero_rows_that_count():
    """31 real rows and 33 ids from {-1, rows, rows + 5} equal, on the bits, the batch whose other 33 rows are a zero row inside the
    split; with zero biases such a row contributes exactly nothing, but it counts in the norm."""
    c = tt.exact_case("scalar-relu-64")
    I, O = c.dims[:2]
    x, y = torch.cat([c.x, torch.zeros(1, I)]), torch.cat([c.y, torch.zeros(1, O)])
    n = x.shape[0]                                          # the zero row is row n - 1
    outside = torch.tensor([-1, n, n + 5], dtype=torch.int32)[torch.arange(33) % 3]
    real = torch.arange(31, dtype=torch.int32)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5))
    a = torch.cat([real, outside])[perm]
    b = torch.cat([real, torch.full((33,), n - 1, dtype=torch.int32)])[perm]
    assert int((a != b).sum()) == 33
    g64, l64 = tt.exact_reference(c, x[b.long()], y[b.long()])
    tr = _trainer(c)
    try:
        tr.set_data(tt.Flat(x, y))
        out = []
        for rows in (a, b):
            tr.set_step(0)
            tr.step(rows=rows.to(DEV))
            out.append((tr.grads.cpu().clone(), tr.read_log(1, 1)[0].clone()))
        _same(out[0][0], out[1][0], "grads")
        _same(out[0][1], out[1][1], "log")
        assert np.array_equal(out[0][0].double().numpy(), g64) and float(out[0][1][0]) == l64 and float(out[0][1][3]) == 64
    finally:
        tr.close()


# ---------------------------------------------------------------- 3. identities that need no tolerance
def test_stale_slab_rows_are_not_read():
    """A 2048-row step fills 64 slab rows; the 33-row step after it must read two."""
    c = tt.case("scalar-softplus")
    big, small = c.order[:2048].to(torch.int32), c.order[100:133].to(torch.int32)
    out = []
    for first in (big, None):
        tr = _trainer(c)
        try:
            tr.set_data(tt.Flat(c.x, c.y))
            if first is not None:
                tr.step(rows=first.to(DEV))
                tr.set_step(0)
            tr.step(rows=small.to(DEV))
            out.append((tr.grads.cpu().clone(), tr.read_log(1, 1)[0].clone()))
        finally:
            tr.close()
    _same(out[0][0], out[1][0], "grads after a larger step")
    _same(out[0][1], out[1][1], "log after a larger step")


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_transposed_copy_after_real_steps(L):
    """k_tube_adam keeps the transposed weights current; a fresh trainer given the state dict builds them with k_tube_wt."""
    from types import SimpleNamespace
    dims = (7, 3, 16 * L, L)
    g = torch.Generator().manual_seed(L)
    x, y = torch.randn(200, 7, generator=g), torch.rand(200, 3, generator=g)
    c = SimpleNamespace(dims=dims, act="tanh", loss="vector", alpha=0.8, delta=1.0, sd=tt.default_params(dims, L))
    tr, fresh = _trainer(c, lr=1e-2), _trainer(c, lr=1e-2)
    try:
        tr.set_data(tt.Flat(x, y))
        for count in (33, 1, 65):
            tr.step(rows=torch.randint(0, 200, (count,), generator=g, dtype=torch.int32).to(DEV))
        assert float((tr.params.cpu() - tt.flat(c.sd)).abs().max()) > 1e-2
        fresh.load_state_dict(tr.state_dict())
        q = torch.randn(50, 7, generator=g).to(DEV)
        _same(tr.predict(q), fresh.predict(q), f"{L} layers")
    finally:
        tr.close()
        fresh.close()


def test_epoch_permutation():
    from types import SimpleNamespace
    dims = (3, 1, 16, 1)
    c = SimpleNamespace(dims=dims, act="relu", loss="scalar", alpha=0.8, delta=1.0, sd=tt.default_params(dims, 1))
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(max(tt.PERM_SIZES), 3, generator=g), torch.rand(max(tt.PERM_SIZES), 1, generator=g)
    tr, other = _trainer(c, seed=3, batch_size=7), _trainer(c, seed=4, batch_size=7)
    try:
        for n in tt.PERM_SIZES:
            perms = []
            for t in (tr, other):
                t.set_data(tt.Flat(x[:n], y[:n]))
                for e in (0, 1):
                    t.begin_epoch(e)
                    perms.append(t.perm[:n].cpu().clone())
            for p in perms:
                assert sorted(p.tolist()) == list(range(n)), n
            if n >= 17:
                assert not torch.equal(perms[0], perms[1]) and not torch.equal(perms[0], perms[2]), n
        # an epoch in chunks of 7 through `count` is the same epoch through perm's slices as `rows`
        n = 65
        tr.set_data(tt.Flat(x[:n], y[:n]))
        tr.begin_epoch(1)
        perm = tr.perm[:n].clone()
        by_count = []
        for b in range(0, n, 7):
            tr.step(min(7, n - b))
            by_count.append(tr.grads.cpu().clone())
        tr.begin_epoch(1)
        for i, b in enumerate(range(0, n, 7)):
            tr.step(rows=perm[b:b + 7])
            _same(tr.grads, by_count[i], f"chunk {i}")
        assert len({tuple(_bits(gq).tolist()) for gq in by_count}) == len(by_count)
    finally:
        tr.close()
        other.close()


# ---------------------------------------------------------------- 4. Adam
def _adam_trainer(c, **kw):
    from types import SimpleNamespace
    cc = SimpleNamespace(dims=c.dims, act="relu", loss="error", alpha=None, delta=1.0, sd=c.sd)
    tr = _trainer(cc, batch_size=64, **kw)
    tr.set_data(tt.Flat(c.x, c.y))
    return tr


def _state(tr):
    return dict(params=tr.params.cpu().numpy().copy(), m=tr.adam_m.cpu().numpy().copy(), v=tr.adam_v.cpu().numpy().copy())


@pytest.mark.parametrize("name", tt.ADAM_IDS)
def test_one_adam_step_against_float64_on_the_device_gradient(name):
    c = tt.adam_case(name)
    tr = _adam_trainer(c, lr=c.lr, gamma=1.0)
    try:
        tr.adam_m.copy_(torch.from_numpy(c.m0))
        tr.adam_v.copy_(torch.from_numpy(c.v0))
        tr.set_step(c.t - 1)
        before = _state(tr)
        tr.step(rows=torch.arange(tt.ADAM_ROWS, dtype=torch.int32).to(DEV))
        got, g = _state(tr), tr.grads.cpu().numpy().copy()
        ref, yard, e32 = tt.adam_one_step(before, g, c.t, c.lr, c.dims)
        r = tt.adam_ratios(got, ref, e32, c.dims)
        print(f"\n{name}: device/e32 " + ", ".join(f"{k} {tt.MARGIN * v:.2f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, r
        dead = c.dead
        assert bool((g[dead] == 0).all()) and bool(np.isfinite(got["params"]).all())
        assert np.array_equal(got["params"][dead].view(np.int32), before["params"][dead].view(np.int32))
        assert bool((got["m"][dead] == 0).all()) and bool((got["v"][dead] == 0).all())
        if c.tiny:
            share = float((np.sqrt(ref["v"][~dead] / (1.0 - 0.999 ** c.t)) < 1e-8).mean())
            assert share > 0.5, share
        log = tr.read_log(c.t, c.t)[0]
        assert float(log[1]) == float(np.float32(c.lr)) and float(log[3]) == tt.ADAM_ROWS
    finally:
        tr.close()


def test_steplr_sizes_the_step_with_the_rate_before_the_scheduler_step():
    s = tt.STEPLR
    c = tt.adam_case("t1-fresh")
    tr = _adam_trainer(c, lr=s["lr0"], gamma=s["gamma"], step_size=s["step_size"])
    rows = torch.arange(tt.ADAM_ROWS, dtype=torch.int32).to(DEV)
    try:
        worst = 0.0
        for t in range(1, s["steps"] + 1):
            before = _state(tr)
            tr.step(rows=rows)
            got, g = _state(tr), tr.grads.cpu().numpy().copy()
            sized, logged = tt.lr_of_step(s["lr0"], s["gamma"], s["step_size"], t), tt.lr_logged(s["lr0"], s["gamma"], s["step_size"], t)
            ref, yard, e32 = tt.adam_one_step(before, g, t, sized, c.dims)
            r = tt.adam_ratios(got, ref, e32, c.dims)
            worst = max(worst, max(r.values()))
            assert max(r.values()) <= 1.0, (t, r)
            assert float(tr.read_log(t, t)[0, 1]) == float(np.float32(logged)), t
            if t % s["step_size"] == 0:       # the logged rate is not the one that sized the step
                wrong = tt.adam64(before["params"], before["m"], before["v"], g, t, logged)
                assert tt.adam_ratios(dict(got, params=wrong["params"]), ref, e32, c.dims)["params"] >= 16.0
        print(f"\nsteplr: worst device/e32 {tt.MARGIN * worst:.2f}")
    finally:
        tr.close()


@pytest.mark.parametrize("name", tt.TRAJ_IDS)
def test_twenty_steps_against_the_float64_trajectory(name):
    from types import SimpleNamespace
    t = tt.trajectory(name)
    c = SimpleNamespace(dims=t.dims, act=t.act, beta=t.beta, loss=t.loss, alpha=tt.ALPHA, delta=tt.DELTA, sd=t.sd)
    tr = _trainer(c, lr=t.lr, gamma=1.0)
    try:
        tr.set_data(tt.Flat(t.x, t.y))
        worst = {}
        for k, st in enumerate(t.steps):
            tr.step(rows=st["rows"].to(DEV))
            r = tt.adam_ratios(_state(tr), st["ref"], st["e32"], t.dims)
            for key, v in r.items():
                worst[key] = max(worst.get(key, 0.0), v)
            assert max(r.values()) <= 1.0, (k + 1, r)
        print(f"\n{name}: worst device/e32 over 20 steps " + ", ".join(f"{k} {tt.MARGIN * v:.2f}" for k, v in worst.items()))
    finally:
        tr.close()


# ---------------------------------------------------------------- 5. eval metrics
@pytest.mark.parametrize("name", tt.EVAL_IDS)
def test_eval_metrics(name):
    c = tt.eval_case(name)
    tr = _trainer(c, batch_size=64)
    try:
        tr.set_data(tt.Flat(c.tx[:1], c.ty[:1]), tt.Flat(c.tx, c.ty))
        ev = (tr.eval_level(c.fixed_level) if c.level else tr.evaluate()).cpu()
        lratio = abs(float(ev[0]) - c.l64) / c.loss_e32
        assert float(ev[3]) == c.n
        assert float(ev[1]) == float(np.float32(c.count64) / np.float32(c.elems))
        msg = f"\n{name}: loss device/e32 {lratio:.2f}"
        assert lratio <= tt.MARGIN, lratio
        if c.count64:
            eratio = abs(float(ev[2]) - c.err64) / c.err_e32
            msg += f", err device/e32 {eratio:.2f}"
            assert eratio <= tt.MARGIN, eratio
        else:
            assert math.isnan(float(ev[2]))
        print(msg)
    finally:
        tr.close()


def test_eval_of_an_empty_selection():
    """Zero weights and an output bias of -100: no fw > w, the coverage is 0 and the mean over nothing is nan, as torch's."""
    c = tt.eval_case("n33")
    tr = _trainer(c, batch_size=64)
    try:
        sd = {k: torch.zeros_like(v) for k, v in c.sd.items()}
        sd[list(sd)[-1]] = torch.full_like(sd[list(sd)[-1]], -100.0)
        tr.load_state_dict(type(c.sd)(sd))
        tr.set_data(tt.Flat(c.tx[:1], c.ty[:1]), tt.Flat(c.tx, c.ty))
        ev = tr.evaluate().cpu()
        assert float(ev[1]) == 0.0 and math.isnan(float(ev[2])) and float(ev[3]) == c.n and math.isfinite(float(ev[0]))
    finally:
        tr.close()
