"""Host side of the windowed closed-loop roll-out: feedback_layout, the layout claim the kernel relies on (on the reference
fixtures), and the rule of DESIGN.md section 10.1 against literal restatements of the reference's two evaluation loops.

The layout claim is checked with the tap distance feedback_layout returns, which is what the kernel is given.  That distance is
1 row for every dN: get_slice (the reference's, restated in tube/data.py and pinned by tests/golden/tube_rows.npz) keeps every
dN-th sample counted back from the end of the episode in every block, so entry t of block i is the raw sample at
T-1 - (T-1-t + i) * dN and block i at row t is block 0 at row t - i.  A distance of i * dN rows would not hold on these rows: on
the fixtures (12 envs, T = 40, N = 3, dN = 2) 444 of 888 (recursive scalar), 888 of 1776 (vector) and 888 of 1776 (error
dynamics) delayed fed-back elements differ from tap 0 at t - i * dN; test_layout_claim_on_fixtures asserts that as well, so
that a layout which handed the kernel dN would be caught.
"""
import os
import pickle

import numpy as np
import pytest
import torch

from legged_gym_dev_amd.tube import data as td
from tests import tube_ref
from tests import tube_window_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("tube_win_fx")
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "tube_dataset.npz")))
    for k in (0, 1):
        with open(d / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump({key: fx[f"e{k}_{key}"] for key in ("z", "pz_x", "v", "done")}, f)
    return str(d)


def test_feedback_layout():
    # n = 4 (z), m = 2 (v)
    assert td.feedback_layout("scalar", 1, 1, False, 4, 2) == (1, 1, 1, 5)
    assert td.feedback_layout("scalar", 10, 2, False, 4, 2) == (1, 1, 1, 41)          # the window holds only z and v
    assert td.feedback_layout("scalar", 1, 1, True, 4, 2) == (1, 1, 1, 5)
    assert td.feedback_layout("scalar", 10, 1, True, 4, 2) == (1, 10, 1, 5)
    assert td.feedback_layout("scalar", 10, 1, True, 2, 2) == (1, 10, 1, 3)            # the simulator's data: z is the position alone
    assert td.feedback_layout("vector", 1, 1, False, 2, 2) == (2, 1, 1, 6)
    assert td.feedback_layout("vector", 10, 3, False, 2, 2) == (2, 10, 1, 6)           # taps are 1 row apart whatever dN is
    assert td.feedback_layout("error_dynamics", 10, 1, False, 4, 3) == (4, 10, 1, 11)
    with pytest.raises(ValueError):
        td.feedback_layout("scalar_horizon", 1, 1, False, 4, 2)
    with pytest.raises(ValueError):
        td.feedback_layout("vector", 2, 1, False, None, 2)
    with pytest.raises(ValueError):
        td.feedback_layout("vector", 2, 1, False, 2, None)
    with pytest.raises(ValueError):
        td.feedback_layout("vector", 0, 1, False, 2, 2)
    with pytest.raises(ValueError):
        td.feedback_layout("vector", 2, 0, False, 2, 2)


KINDS = [("scalar", False), ("scalar", True), ("vector", False), ("error_dynamics", False)]


@pytest.mark.parametrize("dN", [1, 2])
@pytest.mark.parametrize("kind,rec", KINDS, ids=lambda k: str(k))
def test_layout_claim_on_fixtures(folder, kind, rec, dN):
    """The fb columns of tap i at row t are those of tap 0 at row t - i*lag wherever t - i*lag >= 0, lag being the tap distance
    feedback_layout returns for the rows sequences() builds with this N and dN."""
    N = 3
    raw = td.construct_dataset(folder)
    win = {"N": N, "dN": dN, **({"recursive": rec} if kind == "scalar" else {})}
    data, target, _ = td.sequences(kind, raw, **win)
    fb, taps, lag, stride = td.feedback_layout(kind, N, dN, rec, n=raw["z"].shape[-1], m=raw["v"].shape[-1])
    assert lag >= 1 and fb <= target.shape[-1]
    assert (taps - 1) * stride + fb <= data.shape[-1]
    assert data.shape[-1] == (taps * stride if taps > 1 else stride)
    T = data.shape[1]

    def differing(step):
        bad = total = 0
        for i in range(1, taps):
            a, b = data[:, i * step:, i * stride:i * stride + fb], data[:, :T - i * step, :fb]
            bad += int((a != b).sum())
            total += a.numel()
        return bad, total
    bad, total = differing(lag)
    print(f"{kind} recursive={rec} dN={dN}: {bad} of {total} delayed fed-back elements differ from tap 0 at t - i*{lag}")
    assert bad == 0
    assert total == (taps - 1) * data.shape[0] * fb * T - data.shape[0] * fb * lag * sum(range(1, taps))   # every row t >= i*lag
    if dN > 1 and taps > 1:
        bad, total = differing(dN)
        print(f"    at t - i*{dN}: {bad} of {total} differ")
        assert bad > 0                                              # a tap distance of dN rows is not this dataset's


def _mlp(I, O, seed):
    """Row by row, so that a row's bits do not depend on the batch it is evaluated in (BLAS picks its kernel by batch size)."""
    torch.manual_seed(seed)
    net = tube_ref.MLP(I, O, 16, 2, "tanh").double()
    return lambda x: torch.stack([net(r[None])[0].detach() for r in x])


def test_rule_equals_shift_register():
    g = torch.Generator().manual_seed(3)
    E, T, N, nz, m = 3, 30, 4, 2, 2
    rep = 1 + nz + m
    base = torch.rand(E, T, rep, generator=g, dtype=torch.float64)
    x = torch.from_numpy(td.sliding_window(base.numpy(), N, 1, m))
    assert torch.equal(x, torch.stack([wr.delayed_window(base[e], N, 1, m) for e in range(E)]))
    f = _mlp(N * rep, 1, 0)
    rule = wr.rollout_rule(f, x, 1, N, 1, rep)
    lit = torch.stack([wr.shift_register(f, x[e], rep) for e in range(E)])
    assert torch.equal(rule, lit)
    assert not torch.equal(rule, wr.rollout_rule(f, x, 1, 1, 1, rep))             # the delayed taps are fed


@pytest.mark.parametrize("dN", [1, 2])
def test_rule_equals_gather(dN):
    g = torch.Generator().manual_seed(4 + dN)
    E, T, N, n, m = 3, 30, 4, 2, 2
    e, z, v = (torch.rand(E, T, k, generator=g, dtype=torch.float64) - 0.5 for k in (n, n, m))
    base = torch.cat((e, z, v), -1)
    x = torch.stack([wr.delayed_window(base[s], N, dN, m) for s in range(E)])       # the window the script's gather builds from e
    if dN == 1:
        assert torch.equal(x, torch.from_numpy(td.sliding_window(base.numpy(), N, 1, m)))
    f = _mlp(N * (2 * n + m), n, 1)
    rule = wr.rollout_rule(f, x, n, N, dN, 2 * n + m)
    lit = torch.stack([wr.gather(f, e[s], z[s], v[s], N, dN) for s in range(E)])
    assert torch.equal(rule, lit)
    assert not torch.equal(rule, wr.rollout_rule(f, x, n, 1, 1, 2 * n + m))


def test_rule_reseed_restarts_the_history():
    """After a reseed at step r the roll-out of x[:, r:] alone is the roll-out's tail: no tap reaches across the seed."""
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 20, 12, generator=g, dtype=torch.float64)
    f = _mlp(12, 2, 2)
    reseed = torch.zeros(2, 20, dtype=torch.bool)
    reseed[:, 7] = True
    full = wr.rollout_rule(f, x, 2, 3, 2, 4, reseed)
    assert torch.equal(full[:, 7:], wr.rollout_rule(f, x[:, 7:], 2, 3, 2, 4))
    assert torch.equal(full[:, :7], wr.rollout_rule(f, x[:, :7], 2, 3, 2, 4))


def test_feedback_width_is_unchanged():
    assert td.feedback_width("scalar", 3, 2, False, 4) == 1
    assert td.feedback_width("error_dynamics", 1, 1, False, 2) == 2
    for kind, rec in (("vector", False), ("error_dynamics", False), ("scalar", True)):
        with pytest.raises(NotImplementedError):
            td.feedback_width(kind, 2, 1, rec, 4)
