"""The windowed closed-loop roll-out in HIP (k_tube_rollout_window; lg_tube_rollout_window): its bit-exact identities, float64
over 1000 steps, the refusals, and collect_rom_sim_data.py -> train_tube.py (N = 10) -> evaluate_tube.py end to end.

The float64 yardstick is the one of tests/test_hip_tube_eval.py: e32 = max |fp32 torch on the CPU - float64| on the same model,
inputs and rule (tests/tube_window_ref.py), and the HIP result must lie within 4 * e32 of float64.
"""
import ctypes as C
import json
import math
import os
import sys

import pytest
import torch

from tests import tube_ref
from tests import tube_window_ref as wr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(I, O, U, L, act, beta=1.0, seed=0, horizon=None):
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import initial_params
    return HipTubeModel(initial_params(I, O, U, L, seed), activation=act, softplus_beta=beta, horizon=horizon, device=DEV)


def _ref(m, dtype):
    r = tube_ref.MLP(m.input_dim, m.output_dim, m.num_units, m.num_layers, m.activation, m.softplus_beta).to(dtype)
    r.load_state_dict({k: v.to(dtype).cpu() for k, v in m.state_dict().items()})
    return r


# (inputs, outputs, units, layers, activation, beta, fb, taps, stride).  small: weights in LDS; big: 130 -> 128 x 2 -> 50 does not
# fit and reads the transposed copy.  n_seq covers every tile shape (1, 4 and 16 rows per workgroup) with partial tiles; with
# dN = 2 the big model's ring is 19 deep, below T.
WIN_MODELS = {"small": (15, 2, 32, 2, "relu", 1.0, 2, 3, 5), "big": (130, 50, 128, 2, "softplus", 5.0, 3, 10, 13)}


@pytest.mark.parametrize("dN", [1, 2])
@pytest.mark.parametrize("n_seq", [1, 37, 64, 700, 2100])
@pytest.mark.parametrize("name", ["small", "big"])
def test_window_identities(name, n_seq, dN):
    I, O, U, L, act, beta, fb, taps, stride = WIN_MODELS[name]
    T = 50
    g = torch.Generator().manual_seed(n_seq + dN)
    x = (torch.rand(n_seq, T, I, generator=g) - 0.3).to(DEV)
    reseed = torch.rand(n_seq, T, generator=g).lt(0.1).to(DEV)
    m = _model(I, O, U, L, act, beta, seed=7)
    try:
        single = m.rollout(x, fb)
        assert torch.equal(m.rollout_window(x, fb, 1, dN, stride), single)                   # one tap is the single-tap kernel
        assert torch.equal(m.rollout_window(x, fb, 1, dN, stride, reseed), m.rollout(x, fb, reseed))
        flat = m.predict(x.reshape(n_seq * T, I)).reshape(n_seq, T, O)
        assert torch.equal(m.rollout_window(x, fb, taps, dN, stride, torch.ones(n_seq, T, dtype=torch.bool)), flat)
        closed = m.rollout_window(x, fb, taps, dN, stride)
        assert torch.equal(closed, wr.rollout_rule(m.predict, x, fb, taps, dN, stride))     # T predict calls, history by the host
        assert torch.equal(m.rollout_window(x, fb, taps, dN, stride), closed)                # two runs
        assert not torch.equal(closed, single)                                               # the delayed taps are really fed
        assert torch.equal(m.rollout_window(x, fb, taps, dN, stride, reseed), wr.rollout_rule(m.predict, x, fb, taps, dN, stride, reseed))
    finally:
        m.close()


# (kind, inputs, outputs, units, layers, activation, beta, fb, stride): N = 10 taps, default-initialised models, T = 1000
LONG_CASES = [("scalar_recursive", 30, 1, 32, 2, "relu", 1.0, 1, 3), ("vector", 60, 2, 128, 2, "softplus", 5.0, 2, 6),
              ("error_dynamics", 60, 2, 48, 4, "tanh", 1.0, 2, 6)]


@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c[0])
def test_window_1000_steps_matches_float64(case):
    name, I, O, U, L, act, beta, fb, stride = case
    n, T, taps, dN = 8, 1000, 10, 1
    g = torch.Generator().manual_seed(len(name))
    x = torch.rand(n, T, I, generator=g) * 0.8
    done = torch.rand(n, T, generator=g).lt(0.004)                   # a few episode ends per sequence
    reseed = torch.zeros(n, T, dtype=torch.bool)
    reseed[:, 0] = True
    reseed[:, 1:] = done[:, :-1]
    reseed[3] = False                                                # one sequence runs closed for all 1000 steps
    m = _model(I, O, U, L, act, beta, seed=11)
    try:
        with torch.no_grad():
            f64 = wr.rollout_rule(_ref(m, torch.float64), x.double(), fb, taps, dN, stride, reseed)
            f32 = wr.rollout_rule(_ref(m, torch.float32), x, fb, taps, dN, stride, reseed)
        got = m.rollout_window(x, fb, taps, dN, stride, reseed).cpu()
        e32 = float((f32.double() - f64).abs().max())
        err = float((got.double() - f64).abs().max())
        print(f"rollout_window {name} N={taps} T={T}: e32 {e32:.3e}  hip {err:.3e}  ratio {err / e32 if e32 else float('inf'):.2f}  "
              f"scale {float(f64.abs().max()):.3g}")
        assert err <= 4 * e32
    finally:
        m.close()


def test_window_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    flat = _model(12, 2, 16, 1, "relu")                               # 3 taps x stride 4
    wide = _model(256, 64, 16, 1, "relu")
    hz = _model(3 + 2 + 11 * 2, 8, 16, 1, "relu", horizon=(8, 3))
    x = torch.zeros(4, 5, 12, device=DEV)
    xw = torch.zeros(4, 5, 256, device=DEV)
    # (fb, taps, dN, stride)
    bad = [(0, 3, 1, 4), (2, 0, 1, 4), (2, 3, 0, 4), (-1, 3, 1, 4),   # fb, taps or dN below 1
           (3, 3, 1, 4),                                              # fb > output_dim
           (2, 3, 1, 1),                                              # taps > 1 with stride < fb
           (2, 3, 1, 6), (2, 4, 1, 4)]                                # (taps - 1) * stride + fb > input_dim
    bad_wide = [(4, 4, 86, 64), (64, 2, 16, 64), (1, 2, 1024, 1)]    # rings of 1036, 1088 and 1025 floats: beyond 1024
    try:
        assert flat.rollout_window(x, 2, 3, 1, 4).shape == (4, 5, 2)
        assert flat.rollout_window(x, 2, 3, 1, 5).shape == (4, 5, 2)                          # 2 * 5 + 2 = 12: the last legal stride
        assert wide.rollout_window(xw, 4, 4, 21, 64).shape == (4, 5, 64)                      # depth 64, fb 4
        assert wide.rollout_window(xw, 64, 2, 15, 64).shape == (4, 5, 64)                     # a ring of exactly 1024 floats
        for args in bad:
            with pytest.raises(ValueError):
                flat.rollout_window(x, *args)
        for args in bad_wide:
            with pytest.raises(ValueError):
                wide.rollout_window(xw, *args)
        with pytest.raises(ValueError):
            hz.rollout_window(torch.zeros(4, 5, hz.input_dim), 1, 1, 1, 1)
        with pytest.raises(ValueError):
            flat.rollout_window(x[:, :, :11], 2, 3, 1, 4)
        with pytest.raises(ValueError):
            flat.rollout_window(x, 2, 3, 1, 4, torch.zeros(4, 4, dtype=torch.bool))
        # the C side refuses the same with -1 and a reason
        lib, out = flat._tr.lib, torch.zeros(4 * 5 * 64, device=DEV)
        p = lambda t: C.c_void_p(t.data_ptr())
        calls = [lambda a=a: lib.lg_tube_rollout_window(flat._tr.h, p(x), 4, 5, *a, None, p(out)) for a in bad]
        calls += [lambda a=a: lib.lg_tube_rollout_window(wide._tr.h, p(xw), 4, 5, *a, None, p(out)) for a in bad_wide]
        calls += [lambda: lib.lg_tube_rollout_window(hz._tr.h, p(x), 4, 5, 1, 1, 1, 1, None, p(out)),
                  lambda: lib.lg_tube_rollout_window(flat._tr.h, p(x), 0, 5, 2, 3, 1, 4, None, p(out)),
                  lambda: lib.lg_tube_rollout_window(flat._tr.h, p(x), 4, 0, 2, 3, 1, 4, None, p(out)),
                  lambda: lib.lg_tube_rollout_window(flat._tr.h, None, 4, 5, 2, 3, 1, 4, None, p(out))]
        for call in calls:
            assert call() == -1
            reason = lib.lg_last_error().decode()
            assert reason.startswith("lg_tube_rollout_window: ") and len(reason) > len("lg_tube_rollout_window: ")
        with pytest.raises(LeggedHipError):
            flat._tr._call("rollout_window", p(x), 4, 5, 3, 3, 1, 4, None, p(out))
        torch.cuda.synchronize()
    finally:
        flat.close()
        wide.close()
        hz.close()


def _finite(o):
    if isinstance(o, dict):
        return all(_finite(v) for v in o.values())
    if isinstance(o, list):
        return all(_finite(v) for v in o)
    return not isinstance(o, float) or math.isfinite(o)


def _same(a, b):
    """Integers, names and None equal; floats to 1e-9 relative.  The per-age curves of tube_metrics are float64 sums that
    index_add_ accumulates on the device by atomics, in an order that changes from call to call: for the few thousand terms of
    this test the same roll-out gives sums that differ by up to terms * 2^-53, about 1e-12 relative, and no more."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return abs(a - b) <= 1e-9 * max(abs(a), abs(b))
    return type(a) is type(b) and a == b


def test_collect_train_evaluate_windowed_end_to_end(tmp_path):
    from legged_gym_dev_amd.tube import data as td
    from legged_gym_dev_amd.tube import evaluate as ev
    from legged_gym_dev_amd.tube.model import HipTubeModel
    sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
    import collect_rom_sim_data
    import evaluate_tube
    import train_tube
    data = tmp_path / "data"
    collect_rom_sim_data.main(["--num_envs", "64", "--epochs", "2", "--episode_length_s", "5", "--out", str(data), "--seed", "2"])
    raw = td.construct_dataset(str(data))
    n, mv = raw["z"].shape[-1], raw["v"].shape[-1]
    common = ["--data", str(data), "--num_epochs", "2", "--batch_size", "1024", "--lr", "3e-3", "--steps_per_model_checkpoint", "5", "--N", "10"]
    runs = [("scalar", ["--dataset", "scalar", "--recursive"], {"N": 10, "dN": 1, "recursive": True}, 1, 1 + (n - 2) + mv),
            ("error_dynamics", ["--dataset", "error_dynamics", "--loss", "error"], {"N": 10, "dN": 1}, n, 2 * n + mv)]
    for kind, flags, win, fb, stride in runs:
        run = tmp_path / ("run_" + kind)
        train_tube.main(common + flags + ["--out", str(run)])
        evaluate_tube.main(["--run", str(run), "--data", str(data), "--checkpoint", "latest"])
        saved = json.load(open(run / "eval.json"))
        assert _finite(saved) and saved["dataset"] == kind
        assert saved["feedback_width"] == fb and fb == (1 if kind == "scalar" else 2)
        assert (saved["feedback_taps"], saved["feedback_dN"], saved["feedback_stride"]) == (10, 1, stride)
        for part in ("one_step", "rollout"):
            assert saved[part]["steps"] > 0 and 0.0 <= saved[part]["success_rate"] <= 1.0
        # the roll-out's numbers again, from the model called directly
        xs, ys, done = (t.to(DEV) for t in td.sequences(kind, raw, **win))
        assert xs.shape[2] == 10 * stride
        m = HipTubeModel.load(str(run), checkpoint="latest", device=DEV)
        try:
            reseed = ev.reseed_mask(done, None)
            fw = m.rollout_window(xs, fb, 10, 1, stride, reseed)
            again = ev.tube_metrics(fw, ys, done, reseed, kind == "error_dynamics")
            assert _same(json.loads(json.dumps(evaluate_tube._json_safe(again))), saved["rollout"])
            assert again["steps"] == saved["rollout"]["steps"] and again["success_rate"] == saved["rollout"]["success_rate"]
            assert not torch.equal(fw, m.rollout(xs, fb, reseed))                            # and they are not the single-tap ones
        finally:
            m.close()
