"""Level-conditioned tubes, host side (no GPU): the level dataset kinds against the base kinds' recorded rows, the row layouts for
the closed loop, the envelope on both sides of the C boundary, the struct sizes, and the float64 restatement of the per-row loss
(tests/tube_level_ref.py) against the fixed-alpha losses."""
import ctypes
import os
import pickle
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from legged_gym_dev_amd.tube import data as td
from tests import tube_level_ref, tube_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fx(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    fx = _fx("tube_dataset")
    d = tmp_path_factory.mktemp("rom")
    for k in (0, 1):
        with open(d / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump({key: fx[f"e{k}_{key}"] for key in ("z", "pz_x", "v", "done")}, f)
    return str(d)


CASES = {"scalar_n1": ("scalar_level", dict(N=1, dN=1)), "scalar_n3": ("scalar_level", dict(N=3, dN=1, recursive=False)),
         "scalar_n3_rec": ("scalar_level", dict(N=3, dN=1, recursive=True)), "vector_n2": ("vector_level", dict(N=2, dN=2))}


@pytest.mark.parametrize("case", sorted(CASES))
def test_level_kinds_build_the_base_kinds_rows(folder, case):
    kind, args = CASES[case]
    fx = _fx("tube_rows")
    ds = td.DATASETS[kind].from_folder(folder, **args)
    assert torch.equal(ds.data, torch.from_numpy(fx[case + "_data"]))
    assert torch.equal(ds.target, torch.from_numpy(fx[case + "_target"]))
    assert [ds.input_dim, ds.output_dim] == [int(fx[case + "_dims"][0]) + 1, int(fx[case + "_dims"][1])]
    assert ds.input_dim == ds.data.shape[1] + 1 and ds.conditioned is True
    base = td.DATASETS[td.LEVEL_KINDS[kind]].from_folder(folder, **args)
    assert base.conditioned is False and base.input_dim == ds.input_dim - 1
    np.random.seed(3)
    tr, te = ds.random_split(0.8)
    assert type(tr) is type(ds) and tr.input_dim == ds.input_dim and te.conditioned
    d, t, done = td.sequences(kind, folder, **args)
    d0, t0, done0 = td.sequences(td.LEVEL_KINDS[kind], folder, **args)
    assert torch.equal(d, d0) and torch.equal(t, t0) and torch.equal(done, done0)


def test_feedback_layouts():
    n, m = 4, 2
    for N in (1, 3):
        width = 1 + N * (n - 2 + m)
        assert td.feedback_layout("scalar_level", N, 1, False, n=n, m=m) == (1, 1, 1, width + 1)
        assert td.feedback_layout("scalar", N, 1, False, n=n, m=m) == (1, 1, 1, width)
        assert td.feedback_layout("scalar_level", N, 1, True, n=n, m=m) == (1, N, 1, 1 + (n - 2) + m)
        assert td.feedback_layout("vector_level", N, 1, n=n, m=m) == (n, N, 1, 2 * n + m) == td.feedback_layout("vector", N, 1, n=n, m=m)
        # no block reaches the level column: (taps - 1) * stride + fb <= input_dim for all three layouts
        for kind, rec, input_dim in (("scalar_level", False, width + 1), ("scalar_level", True, N * (1 + n - 2 + m) + 1),
                                     ("vector_level", False, N * (2 * n + m) + 1)):
            fb, taps, lag, stride = td.feedback_layout(kind, N, 1, rec, n=n, m=m)
            assert (taps - 1) * (stride if taps > 1 else 0) + fb <= input_dim - 1
    assert td.feedback_width("scalar_level") == 1 and td.feedback_width("vector_level", n=4) == 4


def test_alpha_classes_still_raise():
    for cls in (td.AlphaScalarTubeDataset, td.AlphaVectorTubeDataset):
        with pytest.raises(NotImplementedError, match="B x B"):
            cls.from_folder("x")
        with pytest.raises(NotImplementedError, match="B x B"):
            cls(None, None, 1, 1)
    assert "AlphaScalarTubeDataset" not in [c.__name__ for c in td.DATASETS.values()]


def _cfg(**over):
    from legged_gym_dev_amd import capi
    base = dict(input_dim=4, output_dim=1, num_units=16, num_layers=1, activation=0, loss=capi.TUBE_LOSS["scalar"], horizon=0,
                batch_size=32, H_fwd=0, H_rev=0, step_size=10, seed=1, alpha=0.0, delta=1.0, softplus_beta=1.0, lr=1e-3, gamma=0.1,
                level_input=1, level_lo=0.0, level_hi=1.0)
    return capi.lg_tube_cfg(**{**base, **over})


REFUSED = [(dict(loss=2), dict(loss="error"), "mse"), (dict(horizon=1, H_fwd=1, H_rev=0), dict(horizon=(1, 0)), "horizon"),
           (dict(input_dim=1), dict(input_dim=1), "input_dim"), (dict(level_lo=0.5, level_hi=0.5), dict(level_lo=0.5, level_hi=0.5), "level"),
           (dict(level_lo=-0.1), dict(level_lo=-0.1), "level"), (dict(level_hi=1.5), dict(level_hi=1.5), "level"),
           (dict(level_lo=0.9, level_hi=0.1), dict(level_lo=0.9, level_hi=0.1), "level")]


@pytest.mark.parametrize("c_over,py_over,word", REFUSED, ids=[r[2] + str(i) for i, r in enumerate(REFUSED)])
def test_both_sides_refuse_the_same(c_over, py_over, word):
    """lg_tube_check_cfg is host code: callable without a GPU."""
    import torch  # noqa: F401
    from legged_gym_dev_amd import lib as L
    from legged_gym_dev_amd.tube.trainer import check_envelope
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = ctypes.CDLL(L.SO_PATH)
    lib.lg_last_error.restype = ctypes.c_char_p
    assert lib.lg_tube_check_cfg(ctypes.byref(_cfg())) == 0, lib.lg_last_error().decode()
    assert lib.lg_tube_check_cfg(ctypes.byref(_cfg(**c_over))) == -1
    assert word in lib.lg_last_error().decode()
    kw = dict(input_dim=4, output_dim=1, num_units=16, num_layers=1, loss="scalar_level", level_input=True)
    check_envelope(**kw)
    with pytest.raises((ValueError, NotImplementedError), match=word):
        check_envelope(**{**kw, **py_over})
    # the same fields are not read on an unconditioned configuration
    assert lib.lg_tube_check_cfg(ctypes.byref(_cfg(level_input=0, level_lo=0.0, level_hi=0.0, loss=2))) == 0


def test_ctypes_structs_match_header_sizes():
    from legged_gym_dev_amd import capi
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",' \
          'sizeof(lg_tube_cfg),sizeof(lg_tube_buffers),offsetof(lg_tube_cfg,level_input),offsetof(lg_tube_cfg,level_hi),' \
          'offsetof(lg_tube_buffers,levels));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [ctypes.sizeof(capi.lg_tube_cfg), ctypes.sizeof(capi.lg_tube_buffers), capi.lg_tube_cfg.level_input.offset,
                   capi.lg_tube_cfg.level_hi.offset, capi.lg_tube_buffers.levels.offset]
    assert capi.lg_tube_cfg.level_input.offset == 88                       # appended: every earlier field keeps its offset
    assert capi.TUBE_MAX_LEVELS == 64


@pytest.mark.parametrize("name", ["scalar", "vector"])
def test_restatement_agrees_with_the_fixed_alpha_losses(name):
    g = torch.Generator().manual_seed(5)
    fw, w = torch.rand(37, 3, generator=g, dtype=torch.float64), torch.rand(37, 3, generator=g, dtype=torch.float64)
    fw[3, 1] = w[3, 1]                                                     # the tie: r = 0 takes the (1 - level) |r| branch
    for alpha, delta in ((0.8, 1.0), (0.3, 0.05)):
        level = torch.full((37, 1), alpha, dtype=torch.float64)
        got = tube_level_ref.loss(name + "_level", fw, w, level, delta)
        assert torch.equal(got, tube_ref.loss(name, fw, w, alpha, delta))
    # one level per row: the loss of a batch is the mean of its rows' losses at their own levels, not a B x B broadcast
    level = torch.rand(37, 1, generator=g, dtype=torch.float64)
    rows = torch.stack([tube_level_ref.loss(name + "_level", fw[i:i + 1], w[i:i + 1], level[i:i + 1], 0.05) for i in range(37)])
    np.testing.assert_allclose(float(tube_level_ref.loss(name + "_level", fw, w, level, 0.05)), float(rows.mean()), rtol=1e-14)


def test_train_tube_flags():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
    import train_tube
    a = train_tube.parse_args(["--data", "d", "--dataset", "vector_level", "--level_lo", "0.2", "--sweep", "seed=1,2"])
    assert (a.loss, a.level_input, a.level_lo, a.level_hi) == ("vector_level", True, 0.2, 1.0)
    cfg = train_tube.run_config(a)
    assert cfg["level_input"] is True and cfg["level_lo"] == 0.2 and cfg["level_hi"] == 1.0 and cfg["dataset"] == "vector_level"
    assert "level_input" not in train_tube.run_config(train_tube.parse_args(["--data", "d"]))
    with pytest.raises(SystemExit):
        train_tube.parse_args(["--data", "d", "--level_lo", "0.2"])
