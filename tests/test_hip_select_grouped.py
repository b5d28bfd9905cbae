"""lg_select_kth_grouped on the GPU (select_kernels.hip) against torch.sort on the CPU: per batch row
and group, the sorted members indexed at conformal_rank(count, c) - 1.  The comparisons are those of test_hip_select.py: torch.equal
after mapping -0 to +0 on both sides, NaN positions by isnan, and on the bits a zero is +0.0 and a NaN the canonical quiet NaN;
counts and ranks by torch.equal."""
import ctypes as C

import pytest
import torch

from tests.select_ref import _assert_same, _bit_patterns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
COVERAGES = ("0.5", "0.9", "0.999")


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


def _reference(values, group, G, coverages):
    """values (B, n), group (n) on the CPU -> out (B, G, R), counts (G), ranks (G, R)."""
    from legged_gym_dev_amd.tube.calibrate import conformal_rank
    B, R = values.shape[0], len(coverages)
    out = torch.full((B, G, R), INF)
    counts = torch.zeros(G, dtype=torch.int64)
    ranks = torch.zeros(G, R, dtype=torch.int64)
    values = torch.where(values == 0, torch.zeros_like(values), values)
    for g in range(G):
        member = group == g
        counts[g] = int(member.sum())
        s = torch.sort(values[:, member], dim=1).values
        for r, c in enumerate(coverages):
            k = conformal_rank(int(counts[g]), c)
            ranks[g, r] = k
            if k <= int(counts[g]):
                out[:, g, r] = s[:, k - 1]
    return out, counts, ranks


def _check(values, group, G, coverages=COVERAGES, what=""):
    """values: a CPU (B, n) tensor, or a device view whose CPU copy is the reference's input; group likewise."""
    from legged_gym_dev_amd.tube.calibrate import select_kth_grouped
    dev = values if values.is_cuda else values.to(DEV)
    gdev = group if group.is_cuda else group.to(DEV)
    got, counts, ranks = select_kth_grouped(dev, gdev, G, coverages)
    want, c_want, r_want = _reference(dev.cpu(), gdev.cpu(), G, coverages)
    _assert_same(got, want, what)
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), c_want), what
    assert ranks.dtype == torch.int64 and torch.equal(ranks.cpu(), r_want), what
    return got, counts, ranks


def _random_groups(n, G, seed):
    """ids in [-2, G + 1]: those below 0 and at or above G take no part."""
    return torch.randint(-2, G + 2, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.int32)


def _sizes(lib):
    chunk = lib.lg_select_chunk()
    return (1, 2, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5)


def _group_counts(lib, R):
    gt = lib.lg_select_group_tile(R)
    return sorted({min(G, 1024) for G in (1, 2, gt - 1, gt, gt + 1, 2 * gt + 1) if G >= 1})


@pytest.mark.parametrize("n_index", range(9))
def test_sizes_around_the_wave_the_workgroup_and_the_chunk(lib, n_index):
    n = _sizes(lib)[n_index]
    v = _bit_patterns(2, n, n)
    gt = lib.lg_select_group_tile(len(COVERAGES))
    assert gt >= 2 and lib.lg_select_chunk() >= 1024
    for G in _group_counts(lib, len(COVERAGES)):
        group = _random_groups(n, G, 100 * G + n_index)
        if n >= 64:
            assert bool((group < 0).any()) and bool((group >= G).any())
        _check(v, group, G, what=f"n = {n}, G = {G}")


def test_other_tiles_one_rank_and_eight(lib):
    """R = 1 (the widest tile) and R = 8 (the narrowest), each one group past two tiles."""
    n = 3001
    v = _bit_patterns(2, n, 21)
    for cov in (("0.9",), ("0.1", "0.2", "0.3", "0.5", "0.5", "0.9", "0.99", "0.999")):
        G = 2 * lib.lg_select_group_tile(len(cov)) + 1
        _check(v, _random_groups(n, G, G), G, cov, what=f"R = {len(cov)}, G = {G}")


def test_one_group_equals_the_ungrouped_kernel_bit_for_bit():
    from legged_gym_dev_amd.tube.calibrate import conformal_rank, select_kth, select_kth_grouped
    n = 9001
    v = _bit_patterns(3, n, 31).to(DEV)
    keep = torch.rand(n, generator=torch.Generator().manual_seed(32)) < 0.6
    n_kept = int(keep.sum())
    ranks = [conformal_rank(n_kept, c) for c in COVERAGES]
    want, nk = select_kth(v, torch.tensor(ranks), keep.to(DEV))
    got, counts, rk = select_kth_grouped(v, keep.to(torch.int32) - 1, 1, COVERAGES)
    assert int(counts[0]) == int(nk) == n_kept and rk.cpu().tolist() == [ranks]
    assert torch.equal(got[:, 0, :].contiguous().view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(want[:, :2]).all())
    _check(v, (keep.to(torch.int32) - 1), 1, what="G = 1 against the sort")


def test_empty_and_short_groups():
    n = 5000
    v = torch.randn(2, n, generator=torch.Generator().manual_seed(41))
    group = torch.full((n,), 3, dtype=torch.int32)            # group 0: nobody; 1: ten members; 2: one member; 3: the rest
    ten = torch.arange(10) * 397 + 5
    group[ten] = 1
    group[4321] = 2
    got, counts, ranks = _check(v, group, 5, ("0.99", "0.9", "0.5"), what="empty and short groups")          # group 4: nobody either
    assert counts.tolist() == [0, 10, 1, n - 11, 0]
    assert ranks[0].tolist() == [1, 1, 1] and bool(torch.isinf(got[:, 0]).all()) and bool((got[:, 0] > 0).all())
    assert ranks[1].tolist() == [11, 10, 6] and got[:, 1, 0].tolist() == [INF, INF]
    assert torch.equal(got[:, 1, 1].cpu(), v[:, ten].max(dim=1).values)
    assert ranks[2].tolist() == [2, 2, 1] and torch.equal(got[:, 2, 2].cpu(), v[:, 4321]) and got[:, 2, 0].tolist() == [INF, INF]
    assert bool(torch.isinf(got[:, 4]).all())
    # num / den = 1 / (count + 1): rank 1, the minimum
    got, counts, ranks = _check(v, group, 4, (f"{1 / 8:.3f}",), what="coverage 1 / 8")
    from legged_gym_dev_amd.lib import load
    lib = load()
    p = lambda t: C.c_void_p(t.data_ptr())
    dv, dg = v.to(DEV), group.to(DEV)
    out = torch.empty(2, 4, 1, device=DEV)
    cnt, rk = torch.empty(4, dtype=torch.int64, device=DEV), torch.empty(4, 1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.lg_select_grouped_workspace(2, 4, 1) // 8, dtype=torch.int64, device=DEV)
    for g, count in ((1, 10), (3, n - 11)):
        num, den = (C.c_int64 * 1)(1), (C.c_int64 * 1)(count + 1)
        assert lib.lg_select_kth_grouped(p(dv), n, 2, n, p(dg), 4, num, den, 1, p(out), p(cnt), p(rk), p(ws), None) == 0
        assert int(rk[g, 0]) == 1 and int(cnt[g]) == count
        assert torch.equal(out[:, g, 0].cpu(), v[:, group == g].min(dim=1).values)


def test_degenerate_values_inside_groups():
    n, G = 5000, 7
    g = torch.Generator().manual_seed(51)
    group = _random_groups(n, G, 52)
    _check(torch.full((2, n), 1.25), group, G, what="all equal")
    got, _, _ = _check(torch.full((1, n), -0.0), group, G, what="all -0.0")
    assert bool((got[..., :2].contiguous().view(torch.int32) == 0).all()) and bool(torch.isinf(got[..., 2]).all())     # rank 0.999 is above ~550
    low = (0x3F800000 + torch.randint(0, 256, (2, n), generator=g)).to(torch.int32).view(torch.float32)
    _check(low, group, G, what="only the lowest key byte differs")
    high = (torch.randint(0, 256, (2, n), generator=g) << 24 | 0x00123456).to(torch.int32).view(torch.float32)
    _check(high, group, G, what="only the highest key byte differs")
    # the eight specials in one group of eight (and random values in another): every rank 1..8 through coverages k / 9
    mixed = torch.cat((torch.tensor([0.0, -0.0, 1.0, -1.0, INF, -INF, float("nan"), -float("nan")]), torch.randn(40, generator=g)))[None, :]
    grp = torch.cat((torch.ones(8, dtype=torch.int32), torch.zeros(40, dtype=torch.int32)))
    perm = torch.randperm(48, generator=g)
    from legged_gym_dev_amd.lib import load
    lib = load()
    p = lambda t: C.c_void_p(t.data_ptr())
    dv, dg = mixed[:, perm].contiguous().to(DEV), grp[perm].contiguous().to(DEV)
    out = torch.empty(1, 2, 8, device=DEV)
    cnt, rk = torch.empty(2, dtype=torch.int64, device=DEV), torch.empty(2, 8, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.lg_select_grouped_workspace(1, 2, 8) // 8, dtype=torch.int64, device=DEV)
    num, den = (C.c_int64 * 8)(*range(1, 9)), (C.c_int64 * 8)(*[9] * 8)
    assert lib.lg_select_kth_grouped(p(dv), 48, 1, 48, p(dg), 2, num, den, 8, p(out), p(cnt), p(rk), p(ws), None) == 0
    assert cnt.tolist() == [40, 8] and rk[1].tolist() == list(range(1, 9))
    want = torch.tensor([-INF, -1.0, 0.0, 0.0, 1.0, INF, float("nan"), float("nan")])
    _assert_same(out[0, 1], want, "the order of the specials")


def test_unaligned_rows_and_group():
    n, G = 1027, 5
    v = _bit_patterns(3, n, 61)
    group = _random_groups(n, G, 62)
    want, _, _ = _check(v, group, G, what="ld = n = 1027")
    same = lambda got, what: torch.equal(got.view(torch.int32), want.view(torch.int32)) or pytest.fail(what)
    wide = torch.zeros(3, 1040, device=DEV)
    wide[:, :n] = v.to(DEV)
    view = wide[:, :n]
    assert view.stride(0) == 1040
    same(_check(view, group, G, what="ld = 1040")[0], "ld = 1040")
    flat = torch.zeros(3 * n + 1, device=DEV)
    off = flat[1:].view(3, n)                                             # row 0 starts 4 bytes past a 16-byte boundary
    off.copy_(v.to(DEV))
    assert off.data_ptr() % 16 == 4
    same(_check(off, group, G, what="base + 4 bytes")[0], "base + 4 bytes")
    gbuf = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    goff = gbuf[1:]                                                       # the group ids start 4 bytes past a 16-byte boundary
    goff.copy_(group.to(DEV))
    assert goff.data_ptr() % 16 == 4
    same(_check(v, goff, G, what="group + 4 bytes")[0], "group + 4 bytes")
    same(_check(off, goff, G, what="both + 4 bytes")[0], "both + 4 bytes")
    same(_check(view, goff, G, what="ld = 1040, group + 4 bytes")[0], "ld = 1040, group + 4 bytes")


def test_the_age_pattern_and_a_random_assignment_at_70001():
    """B = 5, n = 70 001, G = 50, R = 3: group = index mod 50, the age of a step under --horizon 50, and a random assignment."""
    n, G = 70001, 50
    v = _bit_patterns(5, n, 7)
    assert bool(torch.isnan(v).any()) and bool(torch.isinf(v).any())
    _, counts, _ = _check(v, (torch.arange(n) % G).to(torch.int32), G, what="index mod 50")
    assert counts.tolist() == [1401] + [1400] * 49
    _check(v, _random_groups(n, G, 71), G, what="random groups")


def _raw(lib, values, group, G, cov, ws):
    B, n = values.shape
    R = len(cov)
    out = torch.empty(B, G, R, device=DEV)
    counts, ranks = torch.zeros(G, dtype=torch.int64, device=DEV), torch.zeros(G, R, dtype=torch.int64, device=DEV)
    num, den = (C.c_int64 * R)(*[c[0] for c in cov]), (C.c_int64 * R)(*[c[1] for c in cov])
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.lg_select_kth_grouped(p(values), n, B, n, p(group), G, num, den, R, p(out), p(counts), p(ranks), p(ws),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.lg_last_error().decode()
    return out, counts, ranks


def test_one_workspace_twice_and_dirty(lib):
    from legged_gym_dev_amd.tube.calibrate import coverage_fractions
    v, group = _bit_patterns(4, 20011, 81), _random_groups(20011, 40, 82)
    cov = ("0.5", "0.9")
    big = max(lib.lg_select_grouped_workspace(4, 40, 2), lib.lg_select_grouped_workspace(2, 9, 5))
    ws = torch.full((big // 8,), -1, dtype=torch.int64, device=DEV)          # arbitrary contents: the call clears what it uses
    dv, dg = v.to(DEV), group.to(DEV)
    a = _raw(lib, dv, dg, 40, coverage_fractions(cov), ws)
    b = _raw(lib, dv, dg, 40, coverage_fractions(cov), ws)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    want = _reference(v, group, 40, cov)
    _assert_same(a[0], want[0])
    assert torch.equal(a[1].cpu(), want[1]) and torch.equal(a[2].cpu(), want[2])
    v2, g2 = _bit_patterns(2, 9999, 83), _random_groups(9999, 9, 84)
    cov2 = ("0.1", "0.5", "0.9", "0.99", "0.999")
    c = _raw(lib, v2.to(DEV), g2.to(DEV), 9, coverage_fractions(cov2), ws)   # another (B, G, R): another layout of the same bytes
    want2 = _reference(v2, g2, 9, cov2)
    _assert_same(c[0], want2[0], "dirty workspace, other B, G and R")
    assert torch.equal(c[1].cpu(), want2[1]) and torch.equal(c[2].cpu(), want2[2])
    d = _raw(lib, dv, dg, 40, coverage_fractions(cov), ws)
    assert torch.equal(a[0].view(torch.int32), d[0].view(torch.int32))


def test_refusals_name_the_field(lib):
    err = lambda: lib.lg_last_error().decode()
    v = torch.zeros(2, 16, device=DEV)
    group = torch.zeros(17, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 3, 1, device=DEV)
    counts, ranks = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(3, 1, dtype=torch.int64, device=DEV)
    ws = torch.zeros(lib.lg_select_grouped_workspace(2, 3, 1) // 8 + 1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    one = lambda x: (C.c_int64 * 1)(x)
    base = dict(values=p(v), ld=16, B=2, n=16, group=p(group), G=3, num=one(9), den=one(10), R=1, out=p(out), counts=p(counts),
                ranks=p(ranks), ws=p(ws))
    order = ("values", "ld", "B", "n", "group", "G", "num", "den", "R", "out", "counts", "ranks", "ws")

    def call(**kw):
        a = dict(base, **kw)
        return lib.lg_select_kth_grouped(*[a[k] for k in order], None)
    for name in ("values", "group", "num", "den", "out", "counts", "ranks", "ws"):
        assert call(**{name: None}) == -1 and "missing array" in err(), name
    for kw, field in ((dict(ld=15), "ld must be at least n"), (dict(n=0), "n must be 1..2^31-1"), (dict(n=2 ** 31, ld=2 ** 31), "n must be 1..2^31-1"),
                      (dict(B=0), "B must be 1..4096"), (dict(G=0), "G must be 1..1024"), (dict(G=1025), "G must be 1..1024"),
                      (dict(R=9), "R must be 1..8"), (dict(num=one(10)), "cov_num[0] must be below cov_den"),
                      (dict(num=one(11)), "cov_num[0] must be below cov_den"), (dict(num=one(0)), "cov_num[0] must be at least 1"),
                      (dict(num=one(-3)), "cov_num[0] must be at least 1"), (dict(den=one(2 ** 31)), "cov_den[0] must be at most 2^31-1"),
                      (dict(ws=C.c_void_p(ws.data_ptr() + 4)), "the workspace must be 8-byte aligned"),
                      (dict(values=C.c_void_p(v.data_ptr() + 2)), "values must be 4-byte aligned"),
                      (dict(group=C.c_void_p(group.data_ptr() + 2)), "group must be 4-byte aligned")):
        assert call(**kw) == -1 and field in err(), kw
    assert call(den=one(2 ** 31 - 1), num=one(2 ** 31 - 2)) == 0          # the largest fraction the entry takes
    torch.cuda.synchronize()
    assert counts.tolist() == [16, 0, 0] and ranks[:, 0].tolist() == [17, 1, 1] and bool(torch.isinf(out).all())
    from legged_gym_dev_amd.tube.calibrate import select_kth_grouped
    from legged_gym_dev_amd.lib import LeggedHipError
    with pytest.raises(ValueError, match="G must be 1..1024"):
        select_kth_grouped(v, group[:16], 1025, ["0.9"])
    with pytest.raises(ValueError, match="0.12345678901"):
        select_kth_grouped(v, group[:16], 3, ["0.12345678901"])
    with pytest.raises(ValueError, match="inside \\(0, 1\\)"):
        select_kth_grouped(v, group[:16], 3, ["1.0"])
    with pytest.raises(ValueError, match="n = 16 elements"):
        select_kth_grouped(v, group, 3, ["0.9"])
    with pytest.raises(LeggedHipError, match="no CPU fallback"):
        select_kth_grouped(v.cpu(), group[:16], 3, ["0.9"])
    torch.cuda.synchronize()
