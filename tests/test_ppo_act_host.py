"""On the CPU: the case list of tests/ppo_act_ref.py reaches every entry of the dispatch matrix of k_mlp_fwd, its input families have the
properties their bounds rest on, the numpy Philox reproduces the published known-answer vectors, and the Box-Muller uniforms stay in
their intervals."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests import ppo_act_ref as ar

F64 = torch.float64


def _nets(c, inp):
    for call in inp["calls"]:
        yield "actor", call["obs"]
        yield "critic", call["cobs"] if c["OC"] else call["obs"]


def test_dispatch_restatement_on_known_layers():
    d = ar.layer_dispatch(235, 512)                            # rough-terrain observations into 512: four tiles per wave, 15 k-steps
    assert (d["kpad"], d["nks"], d["ntiles"]) == (240, 15, 16)
    assert all(w == (4, [(4, 1, 0, 15, False)]) for w in d["waves"])
    d = ar.layer_dispatch(65, 288)                             # 9 tiles: wave 0 has three (<2,2> then <1,4> at t0 = 2), the others two
    assert d["waves"][0] == (3, [(2, 2, 0, 3, True), (1, 4, 2, 2, True)])
    assert d["waves"][1] == d["waves"][3] == (2, [(2, 2, 0, 3, True)])
    d = ar.layer_dispatch(128, 12)                             # a head: one tile on wave 0, none elsewhere
    assert [m for m, _ in d["waves"]] == [1, 0, 0, 0] and d["waves"][0][1] == [(1, 4, 0, 2, False)]
    assert ar.supported(([48, 512, 256, 128, 12], [48, 512, 256, 128, 1]))
    assert not ar.supported(([169, 96, 40, 24, 12], [169, 96, 40, 24, 1]))           # 40: a deeper layer's K off the 16-grid, N off 32
    assert not ar.supported(([520, 64, 32, 12], [520, 64, 32, 1]))                   # wider than the LDS image
    assert ar.supported(([512, 64, 32, 12], [500, 64, 32, 1]))


def test_case_list_reaches_every_entry_of_the_dispatch_matrix():
    labels = [c["label"] for c in ar.CASES]
    assert len(set(labels)) == len(labels)
    reached = {}
    for c in ar.CASES:
        e = ar.entries(c)
        assert bool(e) == c["fused"] == ar.supported(ar.case_dims(c)), c["label"]
        print(f"{c['label']}: {sorted(map(str, e))}")
        for x in e:
            reached.setdefault(x, []).append(c["label"])
    for x in ar.MATRIX:
        assert x in reached, f"no case reaches {x}"
    # <1,4> at t0 = 2 behind <2,2> (mine = 3)
    assert any(calls[-1][:3] == (1, 4, 2) for c in ar.CASES if c["fused"] for d in ar.case_dims(c) for l in range(len(d) - 1)
               for _, calls in ar.layer_dispatch(d[l], d[l + 1])["waves"] if calls)
    fused = [c for c in ar.CASES if c["fused"]]
    widths = {w for c in fused for w in (c["O"], c["OC"]) if w}
    assert widths >= {3, 16, 48, 65, 169, 235, 500, 512}
    assert {c["N"] for c in fused} >= {1, 31, 32, 33, 300} and {c["A"] for c in fused} >= {1, 12, 16}
    assert {c["act"] for c in fused} == {"elu", "selu", "relu", "lrelu", "tanh", "sigmoid", "crelu"}
    for O in (48, 235, 169, 65):
        assert any(c["O"] == O and c["OC"] is None and c["actor"] == c["critic"] == [512, 256, 128] for c in fused)
    assert sum(not c["fused"] for c in ar.CASES) == 2
    assert any(c["actor"] != c["critic"] and c["OC"] for c in fused)


@pytest.mark.parametrize("run", [r for r in ar.runs() if r[1] != "rand"], ids=ar.run_id)
def test_integer_families_are_exact_in_fp32(run):
    """|W| . |x| + |b| < 2^24 at every layer of every call (it bounds each partial sum in any order), first-layer weights and
    observations on their h term alone, deeper weights ternary, and for int_elu no negative pre-activation anywhere."""
    c, fam = run
    assert c["act"] == ("relu" if fam == "int_relu" else "elu")
    inp = ar.build_inputs(c, fam)
    for name, w in inp["params"].items():
        if name == "std":
            continue
        assert torch.equal(w, w.round())
        planes = gr.split_planes(w).double()
        assert torch.equal(planes[0], w.double()) and not bool(planes[1].any()) and not bool(planes[2].any()), name
        if name.endswith("weight") and ".0." not in name:
            assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and int((w != 0).sum(1).max()) <= ar.INT_CAP
        if fam == "int_elu":
            assert float(w.min()) >= 0
    for net, x in _nets(c, inp):
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= ar.INT_X
        assert not bool(gr.split_planes(x)[1:].double().any())
        out, S, trace = ar.forward64(c, inp["params"], x, net)
        for t in trace:
            assert float(t["S"].max()) < 2 ** 24
            assert torch.equal(t["out"], t["out"].round()) and torch.equal(t["out"].float().double(), t["out"])
            if fam == "int_elu":
                assert float(t["pre"].min()) >= 0
        assert float(out.abs().max()) > 0


@pytest.mark.parametrize("run", [r for r in ar.runs() if r[1] == "rand"], ids=ar.run_id)
def test_random_family(run):
    """Mixed exponents along the first layer's k with a lossless split, distinct std in [0.05, 3], no degenerate pre-activation
    interval, and a structural bound that the float64 reference rounded to fp32 and the fp32 yardstick both sit inside."""
    c, fam = run
    inp = ar.build_inputs(c, fam)
    std = inp["std"]
    assert float(std.min()) >= 0.05 and float(std.max()) <= 3.0 and len(set(std.tolist())) == c["A"]
    for name, w in inp["params"].items():
        assert torch.equal(gr.split_planes(w).double().sum(0), w.double()), name
    call = inp["calls"][0]
    if c["O"] >= 16:
        e = torch.frexp(call["obs"].abs().max(0).values)[1]
        assert int(e.max()) - int(e.min()) >= 4
    for net, x in list(_nets(c, inp))[:2]:
        out, S, trace = ar.forward64(c, inp["params"], x, net)
        for t, B in zip(trace, ar.pre_bounds(trace)):
            assert bool(torch.isfinite(B).all()) and float(B.min()) > 0 and float(t["S"].min()) > 0
        bound = ar.structural_bound(trace)
        assert bool(((out.float().double() - out).abs() <= bound).all())
        Y = ar.yardstick(c, inp["params"], x, net).double()
        worst = float(((Y - out).abs() / bound).max())
        print(f"{ar.run_id(run)} {net}: yardstick uses {worst:.4f} of the structural bound")
        assert worst <= 1.0


KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_numpy_philox_reproduces_the_random123_known_answers(ctr, key, want):
    got = ar.philox4x32_10([np.uint32(x) for x in ctr], key)
    assert tuple(int(x) for x in got) == want
    vec = ar.philox4x32_10([np.full(5, x, np.uint32) for x in ctr], key)          # the array form the GPU test uses
    assert all((v == w).all() for v, w in zip(vec, want))


def test_box_muller_uniforms_stay_in_their_intervals():
    seed = ar.learner_seed(3)
    u1, u2 = ar.uniforms(seed, 4096, 16, 0)
    assert float(u1.min()) > 0 and float(u1.max()) <= 1 and float(u2.min()) >= 0 and float(u2.max()) < 1
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    # the ends of the intervals themselves: the largest word gives u1 = 1 (log 0 never taken) and u2 = 1 - 2^-24
    top = np.uint32(0xFFFFFFFF)
    assert ((top >> np.uint32(8)).astype(np.float64) + 1) / 16777216.0 == 1.0 and (top >> np.uint32(8)).astype(np.float64) / 16777216.0 < 1.0
    z = ar.box_muller64(u1, u2)
    assert np.isfinite(z).all() and abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    assert np.abs(ar.box_muller32(u1, u2).astype(np.float64) - z).max() < 1e-5
    # the counter takes the low word of act_count; a learner of another rank draws another stream through its seed
    a, _ = ar.uniforms(seed, 8, 4, 5)
    b, _ = ar.uniforms(seed, 8, 4, (1 << 32) + 5)
    c, _ = ar.uniforms(ar.learner_seed(3, rank=1), 8, 4, 5)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    off, _ = ar.uniforms(seed, 8, 4, 5, env_offset=3)
    assert np.array_equal(off[:5], a[3:])


def test_log_prob_bound_holds_for_an_fp32_emulation():
    """The kernel's arithmetic restated in numpy float32 (act = fl(mu + std z) as one fma-like rounding, the term, the sequential sum)
    sits inside lp_bound against the float64 log-prob."""
    g = torch.Generator().manual_seed(5)
    for A in (1, 12, 16):
        std = (0.05 + 2.95 * torch.rand(A, generator=g)).float()
        mu, z = torch.randn(300, A, generator=g) * 3, torch.randn(300, A, generator=g)
        act = (mu.double() + std.double() * z.double()).float()
        m, s, a = mu.numpy(), std.numpy(), act.numpy()
        lp = np.zeros(300, np.float32)
        for k in range(A):
            d = a[:, k] - m[:, k]
            lp = lp + (-(d * d) / (np.float32(2.0) * s[k] * s[k]) - np.log(s[k]) - np.float32(ar.LOG_SQRT_2PI))
        ref = ar.log_prob64(z.double(), std.double())
        bound = ar.lp_bound(mu.double(), act.double(), z.double(), std.double())
        assert bool(((torch.from_numpy(lp).double() - ref).abs() <= bound).all())
