"""On the CPU: the inputs of tests/gemm_ref.py have the properties its bounds rest on, the ctypes mirror of GemmArgs has the
library's size, and the case list covers the launch arithmetic it names (slice counts, k-tiles per slice, empty slices, tile
counts of the two problems)."""
import ctypes
import os

import pytest
import torch

from tests import gemm_ref as gr

F64 = torch.float64
BIG = 5e7                       # M N K above which the float64 product is left to the GPU test (the int family's bound needs none)


def _small(case):
    return all(M * N * K <= BIG for M, N, K in case["probs"])


def test_gemm_args_mirror_has_the_library_size():
    import torch  # noqa: F401  (shares the HIP runtime instance)
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = ctypes.CDLL(L.SO_PATH)
    assert gr.bind(lib) == ctypes.sizeof(gr.GemmArgs) == 232
    assert gr.GemmArgs.Bpl.offset == 160 and gr.GemmArgs.pl_stride.offset == 176 and gr.GemmArgs.det_base.offset == 208


def test_labels_are_unique_and_every_kernel_path_is_named():
    labels = [c["label"] for c in gr.CASES]
    assert len(set(labels)) == len(labels)
    named = {c["kernel"] for c in gr.CASES}
    assert named == {gr.GEMM_SMALL, gr.GEMM_BIG, gr.PL1_SMALL, gr.PL1_BIG, gr.PL2_SMALL, gr.PL2_BIG, gr.GLDS, gr.DW_SMALL, gr.DW_BIG}
    for kind in (0, 1, 2):
        two = [c for c in gr.CASES if c["kind"] == kind and len(c["probs"]) == 2]
        assert any(c["label"].endswith("z0small") for c in two) and any(c["label"].endswith("z1small") for c in two)
    for kind in (0, 1):
        assert {c["act"] for c in gr.CASES if c["kind"] == kind} == set(range(7))


@pytest.mark.parametrize("case", gr.CASES, ids=gr.case_id)
def test_integer_sums_stay_below_2_to_24(case):
    """|entries| <= 15 and |addends| <= 1000: every partial sum of an output element, in any order, is an integer of magnitude at most
    K * 225 + 1000."""
    for M, N, K in case["probs"]:
        assert K * 225 + 1000 < 2 ** 24


@pytest.mark.parametrize("case", [c for c in gr.CASES if c["kind"] == 2], ids=gr.case_id)
def test_weight_gradient_cases_name_the_slices_the_launch_takes(case):
    if case["splits"]:
        assert case["slices"] == case["splits"]
    else:
        assert case["slices"] == gr.dw_splits(case["probs"])
    big = case["kernel"] == gr.DW_BIG
    maxM, maxN = max(p[0] for p in case["probs"]), max(p[1] for p in case["probs"])
    big_tiles = -(-maxM // 128) * -(-maxN // 128)
    assert big == (big_tiles * case["slices"] >= 192 and maxM > 64 and maxN > 64)


def test_weight_gradient_cases_cover_the_launch_arithmetic():
    dw = [c for c in gr.CASES if c["kind"] == 2]
    t = lambda p, big: -(-p[0] // (128 if big else 64)) * -(-p[1] // (128 if big else 64))
    tiles = lambda c: [t(p, c["kernel"] == gr.DW_BIG) for p in c["probs"]]
    pairs = [c for c in dw if len(c["probs"]) == 2]
    for kernel in (gr.DW_SMALL, gr.DW_BIG):               # both xcd_tile branches on unequal tile counts, with either tile
        for mult8 in (True, False):
            assert any(c["kernel"] == kernel and (c["slices"] % 8 == 0) == mult8 and len(set(tiles(c))) == 2 for c in pairs), (kernel, mult8)
    assert any(len(set(tiles(c))) == 1 and c["probs"][0] != c["probs"][1] and c["slices"] % 8 == 0 for c in pairs)
    assert {c["slices"] for c in dw if not c["splits"]} >= {7, 8, 16, 48, 96}
    assert {c["splits"] for c in dw} >= {1, 3, 8, 16}
    per = {gr.k_tiles_per_slice(p[2], c["slices"])[0] for c in dw for p in c["probs"]}
    assert per >= {1, 2, 3}                                # both parities of the two-deep prefetch
    assert any(gr.k_tiles_per_slice(p[2], c["slices"])[1] < c["slices"] for c in dw for p in c["probs"])      # empty trailing slices
    assert any(p[2] % 32 for c in dw for p in c["probs"])
    assert any(c["nstore"][z] and c["nstore"][z] < c["probs"][z][1] for c in dw for z in range(len(c["probs"])))


@pytest.mark.parametrize("run", [r for r in gr.runs() if r[1] == "int" and r[0]["kind"] == 1], ids=gr.run_id)
def test_integer_column_sums_are_exact(run):
    """colsum adds M values per column: the sum of their magnitudes (a bound on every partial sum in any order) stays below 2^24."""
    case, fam = run
    for z in range(len(case["probs"])):
        p = gr.build_problem(case, z, fam)
        ref = gr.reference(case, p)
        assert float((p["colsum0"].double().abs() + ref["out"].abs().sum(0)).max()) < 2 ** 24
        assert torch.equal(ref["out"], ref["out"].round())


@pytest.mark.parametrize("run", [r for r in gr.runs() if r[1] == "int" and _small(r[0])], ids=gr.run_id)
def test_integer_family(run):
    case, fam = run
    for z in range(len(case["probs"])):
        p = gr.build_problem(case, z, fam)
        for k in ("a", "b"):
            assert torch.equal(p[k], p[k].round()) and float(p[k].abs().max()) <= 15
        for k in ("bias", "colsum0", "C0"):
            if p[k] is not None:
                assert torch.equal(p[k], p[k].round()) and float(p[k].abs().max()) <= 1000
        ref = gr.reference(case, p)
        assert float(ref["S"].max()) < 2 ** 24
        assert torch.equal(ref["out"].float().double(), ref["out"])
        assert case["act"] in (0, 3)                      # an activation that keeps integers


@pytest.mark.parametrize("run", [r for r in gr.runs() if r[1].startswith(("planes", "deep"))], ids=gr.run_id)
def test_three_plane_families(run):
    """planes_*: 16 fraction bits, at most 120 nonzero products, sums multiples of 2^-16 below 256.  deep_*: 22 fraction bits, one
    nonzero product, sums multiples of 2^-22 below 4.  Either way 24 bits: exact in fp32 in any order.  The m term is live in both;
    the l term is ZERO throughout planes_* (h and m, rounded to nearest with signed remainders, carry all 17 bits) and live in deep_*."""
    case, fam = run
    bits, cap, top, below = (16, 120, 16, 256) if fam.startswith("planes") else (22, 1, 2, 4)
    assert case["act"] == 0
    for z in range(len(case["probs"])):
        p = gr.build_problem(case, z, fam)
        x, t = (p["a"], p["b"]) if fam.endswith("_a") else (p["b"], p["a"])
        n = (x.double().abs() - 1) * 2 ** bits
        assert torch.equal(n, n.round()) and float(n.min()) >= 0 and float(n.max()) < 2 ** bits
        h, m, l = (q.double() for q in gr.split_planes(x))
        assert torch.equal(h + m + l, x.double())
        if x.numel() >= 512:
            assert float((m != 0).double().mean()) > 0.9
            assert float((l != 0).double().mean()) > 0.9 if bits == 22 else not bool((l != 0).any())
        assert set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
        nonzero = (t != 0).sum(0 if fam.endswith("_a") else 1)       # along k, per output column (_a) / row (_b)
        assert int(nonzero.max()) <= cap
        if p["K"] > cap:
            assert int(nonzero.min()) == cap
        for k in ("bias", "C0"):
            if p[k] is not None:
                q = p[k].double() * 2 ** bits
                assert torch.equal(q, q.round()) and float(p[k].abs().max()) < top
        assert p["colsum0"] is None
        ref = gr.reference(case, p)
        assert float(ref["S"].max()) < below               # bounds every partial sum in any order
        q = ref["out"] * 2 ** bits
        assert torch.equal(q, q.round()) and torch.equal(ref["out"].float().double(), ref["out"])


@pytest.mark.parametrize("run", [r for r in gr.runs() if r[1] == "rand" and _small(r[0])][::7], ids=gr.run_id)
def test_random_family(run):
    """Mixed exponents along k (the scale cancels in the product), a split that loses nothing, aux on both branches, and a
    structural bound the float64-rounded-to-fp32 reference itself sits far inside."""
    case, fam = run
    for z in range(len(case["probs"])):
        p = gr.build_problem(case, z, fam)
        if p["K"] >= 16:
            e = torch.frexp(p["a"].abs().max(0).values)[1]
            assert int(e.max()) - int(e.min()) >= 8
        for x in (p["a"], p["b"]):
            h, m, l = (q.double() for q in gr.split_planes(x))
            assert torch.equal(h + m + l, x.double())
        if p["aux"] is not None:
            assert float(p["aux"].min()) > -1 and float(p["aux"].max()) < 2
            if p["aux"].numel() >= 8:
                assert bool((p["aux"] > 0).any()) and bool((p["aux"] < 0).any())
        ref = gr.reference(case, p)
        bound = gr.structural_bound(case, p, ref, case["slices"])
        assert bool(((ref["out"].float().double() - ref["out"]).abs() <= bound).all())
        if case["act"] in (0, 3, 4) and p["K"] <= 512:     # the yardstick obeys the bound it is the measure for
            Y = gr.yardstick(case, p, "cpu").double()
            assert bool(((Y - ref["out"]).abs() <= bound).all())


def test_activation_restatements_agree_with_torch():
    v = torch.linspace(-4, 4, 801, dtype=F64)
    import torch.nn.functional as Fn
    want = {1: Fn.elu(v), 2: Fn.selu(v), 3: Fn.relu(v), 4: Fn.leaky_relu(v, 0.01), 5: torch.tanh(v), 6: torch.sigmoid(v), 0: v}
    for code, w in want.items():
        torch.testing.assert_close(gr.act_fwd64(code, v), w, rtol=1e-12, atol=1e-12)
        x = v.clone().requires_grad_(True)
        gr.act_fwd64(code, x).sum().backward()
        ok = v != 0
        torch.testing.assert_close(gr.act_slope64(code, v)[ok], x.grad[ok], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(gr.act_bwd64(code, w)[ok], x.grad[ok], rtol=1e-9, atol=1e-12)     # through the OUTPUT
