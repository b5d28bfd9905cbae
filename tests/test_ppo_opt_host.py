"""On the CPU: the conditions of tests/ppo_opt_ref.py.  Its float64 step is torch.optim.Adam + clip_grad_norm_ + rsl_rl's lr rule in
float64; every step of every trajectory is in the regime its case names, with the margins that keep fp32 on the same branch; both
clamps are reached and held; the restated plane map is injective and its pads are the complement of its image; the split-bf16 terms
sum back exactly; and a numpy-float32 restatement of the kernels' own order of operations uses a small share of every bound the GPU
test asserts (printed)."""
import numpy as np
import pytest
import torch

from tests import ppo_opt_ref as R

CASES = [(s, t) for s in R.SIZES for t in R.TRAJECTORIES]
HOST_CASES = [c for c in CASES if c[0] != "large"] + [("large", "mixed"), ("large", "spread")]      # (CPU time: the others run on the GPU)


def test_sizes_reach_the_code_paths_they_name():
    n = {s: R.layout(s)["n"] for s in R.SIZES}
    assert n["tiny"] < 256 and n["small"] == 12 + 2 * (48 * 64 + 64 + 64 * 32 + 32) + 32 * 12 + 12 + 32 + 1
    assert n["large"] > 2 * 1024 * 256                                   # a third trip of k_opt_adam's 1024 x 256 threads
    segs = {s: R.layout(s)["segs"] for s in R.SIZES}
    assert [sg[3] for sg in segs["large"] if sg[2] == 235] == [256, 256]
    assert sorted(sg[3] for sg in segs["priv"] if sg[2] in (65, 169)) == [96, 192]
    rnn = R.layout("rnn")
    assert all((rnn["dest"][o:o + r * (c or 1)] < 0).all() for name, o, r, c in rnn["blocks"] if name.startswith("memory_"))
    assert all(len(t["steps"]) >= 12 for t in R.TRAJECTORIES.values()) and R.BEGIN_AFTER % 2 == 1


@pytest.mark.parametrize("size", list(R.SIZES))
def test_plane_map_is_injective_and_pads_are_its_complement(size):
    L = R.layout(size)
    dest, stride = L["dest"], L["pl_stride"]
    img = dest[dest >= 0]
    assert stride % 8 == 0 and img.size == sum(r * c for _, r, c, _ in L["segs"])
    assert np.unique(img).size == img.size and img.min() == 0 and img.max() < stride
    for name, off, r, c in L["blocks"]:                      # exactly the MLP weight matrices have an image
        has = dest[off:off + r * (c or 1)] >= 0
        assert has.all() if (c and not name.startswith("memory_")) else not has.any(), name
    pad = np.ones(stride, dtype=bool)
    pad[img] = False
    want = 0                                                 # pad columns of the first layers + the round-up of every segment
    for _, r, c, ld in L["segs"]:
        want += r * (ld - c) + (-(r * ld) % 8)
    assert int(pad.sum()) == want == stride - img.size
    if size in ("large", "priv"):
        assert want > 0


def test_split_planes_sum_back_exactly():
    g = torch.Generator().manual_seed(5)
    w = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-12, 3, (4096,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -100, 1.0 + 2.0 ** -23, 3.0 - 2.0 ** -22])])
    pl = R.split_planes(w)
    assert pl.dtype == torch.bfloat16 and torch.equal(pl.double().sum(0), w.double())
    assert bool((pl[2][:4096] != 0).any())                   # the third term is needed: two do not hold 24 bits


@pytest.mark.parametrize("size,traj", CASES, ids=lambda v: v)
def test_every_step_is_in_the_regime_its_case_names(size, traj):
    spec = R.TRAJECTORIES[traj]
    rows, lr, held = R.mb_rows(size), float(np.float32(spec["lr0"])), {"@min": 0, "@max": 0}
    n = R.layout(size)["n"]
    for i, (family, norm, kl_nominal, regime) in enumerate(spec["steps"]):
        gs, ks = R.gradient(size, traj, i, family, norm), R.kl_sum(size, kl_nominal)
        kl = float(ks) / rows
        assert float(np.float32(kl * rows)) == kl * rows                  # exactly representable: both precisions divide one number
        got = float(np.sqrt((gs.astype(np.float64) ** 2).sum()))
        assert abs(got - norm) <= 1e-6 * norm and abs(norm - R.MAX_GRAD_NORM) >= 0.01
        assert ("clip" in regime) == (got > R.MAX_GRAD_NORM)
        assert min(abs(kl / (2 * R.DESIRED_KL) - 1), abs(kl / (R.DESIRED_KL / 2) - 1)) >= 0.1
        rule = "zero" if kl == 0 else "down" if kl > 2 * R.DESIRED_KL else "up" if kl < R.DESIRED_KL / 2 else "band"
        assert rule == regime.split()[1].split("@")[0]
        new = R.lr_rule(lr, kl, spec["adaptive"])
        if not spec["adaptive"] or rule in ("zero", "band"):
            assert new == lr
        elif "@" in regime:
            assert new == {"@min": R.LR_MIN, "@max": R.LR_MAX}[regime[-4:]] and new != (lr / 1.5 if rule == "down" else lr * 1.5)
            held[regime[-4:]] += 1
        else:
            assert new == (lr / 1.5 if rule == "down" else lr * 1.5) and R.LR_MIN < new < R.LR_MAX
        lr = new
        if family == "zero":
            assert not gs.any()
        if family == "spread":
            assert not gs[R.zero_mask(n)].any() and (gs[~R.zero_mask(n)] != 0).all()
            if n > 1000:
                a = np.abs(gs[gs != 0])
                assert a.max() / a.min() > 1e10
    if traj == "raise":
        assert held["@max"] >= 3                             # reached once, held for two steps or more
    if traj == "lower":
        assert held["@min"] >= 3
    regimes = {s[3] for t in R.TRAJECTORIES.values() for s in t["steps"]}
    assert {a + " " + b for a in ("clip", "free") for b in ("band", "up", "down", "zero")} <= regimes


@pytest.mark.parametrize("size,traj", [c for c in HOST_CASES if c[0] in ("tiny", "small", "rnn")], ids=lambda v: v)
def test_float64_reference_is_torch_adam_in_float64(size, traj):
    spec = R.TRAJECTORIES[traj]
    cfg = dict(world=1, mb_rows=R.mb_rows(size), adaptive=spec["adaptive"])
    a = b = R.initial_state(size, spec["lr0"])
    for i, (family, norm, kl, _) in enumerate(spec["steps"]):
        gs, ks = R.gradient(size, traj, i, family, norm), R.kl_sum(size, kl)
        a, b = R.step(a, gs, ks, cfg), R.torch_step(b, gs, ks, cfg, torch.float64)
        assert a["lr"] == b["lr"] and a["t"] == b["t"] == i + 1 and abs(a["norm"] - b["norm"]) <= 1e-14 * a["norm"]
        for k in R.ARRAYS:
            assert np.abs(a[k] - b[k]).max() <= 1e-13 * np.abs(a[k]).max(), (i, k)


def test_float64_reference_divides_by_world_in_all_three_places():
    spec = R.TRAJECTORIES["mixed"]
    cfg = dict(world=4, mb_rows=R.mb_rows("small"), adaptive=True)
    a = b = R.initial_state("small", spec["lr0"])
    for i, (family, norm, kl, _) in enumerate(spec["steps"]):
        gs, ks = R.gradient("small", "mixed", i, family, norm, 4), R.kl_sum("small", kl, 4)
        a, b = R.step(a, gs, ks, cfg), R.torch_step(b, gs, ks, cfg, torch.float64)
        assert a["lr"] == b["lr"] and abs(a["norm"] - norm) <= 1e-6 * norm and abs(a["kl"] - kl) <= 1e-6 * kl
        assert np.abs(a["params"] - b["params"]).max() <= 1e-13


@pytest.mark.parametrize("size,traj", HOST_CASES, ids=lambda v: v)
def test_fp32_restatement_of_the_kernels_uses_a_small_share_of_the_bounds(size, traj):
    """The spread family's untouched entries keep their bits in the reference; emulate32 sits inside 4 e32 on every array, block and
    step, inside the lr and KL bounds, and its worst share is printed."""
    steps = R.run(size, traj)
    n = R.layout(size)["n"]
    em = R.initial_state(size, R.TRAJECTORIES[traj]["lr0"])
    p0 = em["params"].copy()
    worst = {}
    for s in steps:
        em = R.emulate32(em, s["grad_sum"], s["kl_sum"], s["cfg"])
        ref = s["ref"]
        for k, v in R.ratios(em, ref, s["e32"], size, s["allow"]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        worst["lr"] = max(worst.get("lr", 0.0), abs(em["lr"] - ref["lr"]) / (R.LR_RTOL * ref["lr"]))
        if ref["kl"]:
            worst["kl"] = max(worst.get("kl", 0.0), abs(em["kl"] - ref["kl"]) / (R.KL_RTOL * ref["kl"]))
        if traj == "spread":
            z = R.zero_mask(n)
            assert np.array_equal(ref["params"][z], p0[z]) and not ref["m"][z].any() and not ref["v"][z].any()
            assert np.array_equal(em["params"][z], p0[z].astype(np.float32))
    print("ppo_opt_errors host", size, traj, {k: round(float(v), 3) for k, v in worst.items()})
    assert max(R.asserted(worst).values()) <= 1.0, worst


@pytest.mark.parametrize("t", (0, 1, 11) + R.LATE_T)
def test_bias_corrections_formed_in_fp32_stay_inside_the_step_share_and_the_allowance(t):
    """k_opt_adam forms 1 - powf(0.999f, t) on every lane.  0.999f is 1.3e-8 above 0.999, so 0.999f^t is off by 1.3e-8 t of itself
    and the correction 1 - 0.999^t (about 1e-3 t while t << 1000) by 1.3e-5 of itself: 6.6e-6 of a step through the square root, on
    every early step and always in the step's own direction, with up to one rounding of 0.999^t over 1e-3 t beside it; about 4e-6 at
    t = 1000, nothing once 0.999^t has died out.  That is inside the project's 1e-4 of a step, so the kernel stays; bc_allowance
    bounds it from the number formats, and is itself inside 1e-4 at every step count the tests reach."""
    state, grad, ks = R.late_case("small", t)
    cfg = dict(world=1, mb_rows=R.mb_rows("small"), adaptive=True)
    ref = R.step(state, grad, ks, cfg)
    worst = {}
    for name, fn in (("kernel order", lambda: R.emulate32(state, grad, ks, cfg)), ("corrections in double", lambda: R.emulate32(state, grad, ks, cfg, pow64=True)),
                     ("yardstick", lambda: R.torch_step(state, grad, ks, cfg, torch.float32))):
        worst[name] = float(np.abs(fn()["params"].astype(np.float64) - ref["params"]).max() / ref["lr"])
    step_size = float(np.abs(ref["params"]).max() / ref["lr"])
    allow = R.bc_allowance(t + 1)
    print("ppo_opt_errors host late", t + 1, {k: f"{v:.2e}" for k, v in worst.items()}, f"of lr; allowance {allow:.2e} of a step of {step_size:.2f} lr; allowed",
          R.STEP_SHARE)
    assert worst["kernel order"] <= R.STEP_SHARE and worst["corrections in double"] <= R.STEP_SHARE / 100
    assert worst["kernel order"] <= allow * step_size + worst["corrections in double"] + worst["yardstick"]
    assert allow <= R.STEP_SHARE
    if t == 0:
        assert 1e-6 < worst["kernel order"] < 2e-5                                # (this step is 0.45 lr at its largest)
    assert step_size > 0.1                                                        # the step is of the size of lr: the share means something


def test_allowance_is_inside_the_step_share_at_every_step_count():
    steps = list(range(1, 20)) + [100, 1000, 10000, 100000]
    a = [R.bc_allowance(t) for t in steps]
    print("ppo_opt_errors host allowance", {t: f"{v:.1e}" for t, v in zip(steps, a)})
    assert max(a) == a[0] <= R.STEP_SHARE and all(x >= y for x, y in zip(a, a[1:])) and a[-1] < 1e-12
