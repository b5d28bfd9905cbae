"""lg_select_kth on the GPU (select_kernels.hip): the batched exact k-th smallest against torch.sort on the
CPU.  Every comparison is torch.equal on the values after mapping -0 to +0 on both sides, NaN positions compared by isnan; on top
of that the kernel's own promise is checked on the bits: a zero comes back as +0.0 and a NaN as the canonical quiet NaN."""
import ctypes as C

import pytest
import torch

from tests.select_ref import _assert_same, _bit_patterns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


def _reference(values, ranks, keep=None):
    """values (B, n), ranks (B, R) on the CPU: torch.sort of the kept values, [rank - 1]; +inf outside 1..n_kept."""
    B, R = ranks.shape
    out = torch.empty(B, R)
    for b in range(B):
        kept = values[b] if keep is None else values[b][keep.bool()]
        kept = torch.where(kept == 0, torch.zeros_like(kept), kept)
        s = torch.sort(kept).values
        for r in range(R):
            k = int(ranks[b, r])
            out[b, r] = s[k - 1] if 1 <= k <= s.numel() else INF
    return out, (values.shape[1] if keep is None else int(keep.bool().sum()))


def _check(values, ranks, keep=None, what=""):
    """values: a CPU (B, n) tensor, or a device view whose CPU copy is the reference's input."""
    from legged_gym_dev_amd.tube.calibrate import select_kth
    dev = values if values.is_cuda else values.to(DEV)
    ranks = torch.as_tensor(ranks, dtype=torch.int64)
    if ranks.dim() == 1:
        ranks = ranks[None, :].expand(dev.shape[0], -1)
    got, n_kept = select_kth(dev, ranks, None if keep is None else keep.to(DEV))
    want, n_want = _reference(dev.cpu(), ranks, keep)
    _assert_same(got, want, what)
    assert int(n_kept) == n_want, what
    return got


def _middle_ranks(n_kept, B):
    return torch.tensor([[1, max(1, (n_kept * (b + 2)) // (B + 3)), n_kept] for b in range(B)])


def test_sizes_around_the_wave_the_workgroup_and_the_chunk(lib):
    chunk = lib.lg_select_chunk()
    assert chunk >= 1024
    for n in (1, 2, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5):
        v = _bit_patterns(2, n, n)
        _check(v, _middle_ranks(n, 2), what=f"n = {n}")


def test_more_chunks_than_workgroups_per_row(lib):
    """600 rows leave four workgroups to a row; six chunks and a tail make some of them walk two chunks."""
    chunk = lib.lg_select_chunk()
    n = 5 * chunk + 77
    v = _bit_patterns(600, n, 12)
    g = torch.Generator().manual_seed(13)
    _check(v, torch.randint(1, n + 1, (600, 2), generator=g), what="B = 600")
    keep = torch.rand(n, generator=g) < 0.5
    _check(v[:300], torch.randint(1, int(keep.sum()) + 1, (300, 1), generator=g), keep, what="B = 300, keep")


def test_rows_that_are_not_16_byte_aligned():
    v = _bit_patterns(3, 1027, 5)
    ranks = _middle_ranks(1027, 3)
    want = _check(v, ranks, what="ld = n = 1027")
    wide = torch.zeros(3, 1040, device=DEV)
    wide[:, :1027] = v.to(DEV)
    view = wide[:, :1027]
    assert view.stride(0) == 1040
    assert torch.equal(_check(view, ranks, what="ld = 1040").view(torch.int32), want.view(torch.int32))
    flat = torch.zeros(3 * 1027 + 1, device=DEV)
    off = flat[1:].view(3, 1027)                                           # row 0 starts 4 bytes past a 16-byte boundary
    off.copy_(v.to(DEV))
    assert off.data_ptr() % 16 == 4
    assert torch.equal(_check(off, ranks, what="base + 4 bytes").view(torch.int32), want.view(torch.int32))
    keep = torch.rand(1027, generator=torch.Generator().manual_seed(1)) < 0.5
    _check(off, _middle_ranks(int(keep.sum()), 3), keep, what="base + 4 bytes, keep")


def test_a_strided_view():
    big = _bit_patterns(4, 3000, 6).to(DEV)
    _check(big[:, 7:2000], _middle_ranks(1993, 4), what="columns 7..2000 of (4, 3000)")
    _check(big[::2, :1500], _middle_ranks(1500, 2), what="every other row")
    _check(big.t()[:3000:1000], [1, 2, 4], what="a transposed view (copied)")


def test_random_bit_patterns_at_70001():
    """B = 5, n = 70 001, R = 3: all four digits, denormals, the infinities and NaNs of both signs occur."""
    v = _bit_patterns(5, 70001, 7)
    assert bool(torch.isnan(v).any()) and bool(torch.isinf(v).any()) and bool(((v != 0) & (v.abs() < 1e-38)).any())
    assert bool((torch.isnan(v) & (v.view(torch.int32) < 0)).any()) and bool((torch.isnan(v) & (v.view(torch.int32) > 0)).any())
    got = _check(v, _middle_ranks(70001, 5))
    assert bool(torch.isnan(got[:, 2]).all())                             # rank n of a row with NaNs is a NaN, as torch.sort has it
    keep = torch.rand(70001, generator=torch.Generator().manual_seed(2)) < 0.5
    _check(v, _middle_ranks(int(keep.sum()), 5), keep, what="a random half")


def test_degenerate_value_sets():
    n = 5000
    _check(torch.full((2, n), 1.25), [1, n // 2, n], what="all equal")
    _check(torch.full((1, n), -0.0), [1, n], what="all -0.0")
    g = torch.Generator().manual_seed(3)
    two = torch.where(torch.rand(2, n, generator=g) < 0.3, torch.tensor(-2.5), torch.tensor(7.0))
    k = int((two[0] == -2.5).sum())
    _check(two, torch.tensor([[1, k, k + 1, n], [1, k, k + 1, n]]), what="two distinct values")
    low = (0x3F800000 + torch.randint(0, 256, (2, n), generator=g)).to(torch.int32).view(torch.float32)
    _check(low, [1, 17, n // 2, n], what="only the lowest key byte differs")
    high = (torch.randint(0, 256, (2, n), generator=g) << 24 | 0x00123456).to(torch.int32).view(torch.float32)
    _check(high, [1, 17, n // 2, n], what="only the highest key byte differs")
    mixed = torch.tensor([[0.0, -0.0, 1.0, -1.0, INF, -INF, float("nan"), -float("nan")]])
    _check(mixed, [1, 2, 3, 4, 5, 6, 7, 8], what="the order of the specials")


def test_eight_ranks_with_repeats():
    v = _bit_patterns(3, 9001, 8)
    _check(v, torch.tensor([[5, 5, 9001, 1, 4500, 4500, 1, 5], [1] * 8, [9001, 9000, 8999, 3, 2, 1, 4500, 9001]]))


def test_keep():
    n = 6000
    v = _bit_patterns(2, n, 9)
    one = torch.zeros(n, dtype=torch.bool)
    one[4321] = True
    got = _check(v, [0, 1, 2], one, what="all but one dropped")
    assert got[:, 0].tolist() == [INF, INF] and got[:, 2].tolist() == [INF, INF]
    none = torch.zeros(n, dtype=torch.bool)
    got = _check(v, [1, 2, n], none, what="every element dropped")
    assert bool(torch.isinf(got).all()) and bool((got > 0).all())
    half = torch.rand(n, generator=torch.Generator().manual_seed(4)) < 0.5
    k = int(half.sum())
    _check(v, [1, k // 3, k], half, what="a random half")
    _check(v, [1, k // 3, k], half.to(torch.uint8) * 7, what="any non-zero byte keeps")


def test_ranks_outside_give_inf():
    v = torch.randn(2, 777, generator=torch.Generator().manual_seed(5))
    got = _check(v, [0, 778, -3, 2 ** 40, 777])
    assert bool(torch.isinf(got[:, :4]).all()) and bool(torch.isfinite(got[:, 4]).all())
    keep = torch.arange(777) % 3 == 0
    got = _check(v, [0, 259, 260], keep)
    assert bool(torch.isfinite(got[:, 1]).all()) and bool(torch.isinf(got[:, 2]).all())


def _raw(lib, values, ranks, ws, keep=None):
    B, n = values.shape
    R = ranks.shape[1]
    out = torch.empty(B, R, device=DEV)
    n_kept = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.lg_select_kth(p(values), n, B, n, p(keep) if keep is not None else None, p(ranks), R, p(out), p(n_kept), p(ws),
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.lg_last_error().decode()
    return out, n_kept


def test_one_workspace_twice_and_dirty(lib):
    v = _bit_patterns(4, 20011, 10)
    ranks = _middle_ranks(20011, 4)
    big = max(lib.lg_select_workspace(4, 3), lib.lg_select_workspace(2, 5))
    ws = torch.full((big // 8,), -1, dtype=torch.int64, device=DEV)          # arbitrary contents: the call clears what it uses
    a, _ = _raw(lib, v.to(DEV), ranks.to(DEV), ws)
    b, _ = _raw(lib, v.to(DEV), ranks.to(DEV), ws)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _assert_same(a, _reference(v, ranks)[0])
    v2 = _bit_patterns(2, 9999, 11)
    r2 = torch.tensor([[1, 2, 5000, 9999, 10000], [9999, 9999, 1, 1, 77]])
    c, nk = _raw(lib, v2.to(DEV), r2.to(DEV), ws)                          # another (B, R): another layout of the same bytes
    _assert_same(c, _reference(v2, r2)[0], "dirty workspace, other B and R")
    assert int(nk) == 9999
    d, _ = _raw(lib, v.to(DEV), ranks.to(DEV), ws)
    assert torch.equal(a.view(torch.int32), d.view(torch.int32))


def test_envelope_refusals_name_the_field(lib):
    err = lambda: lib.lg_last_error().decode()
    for B, R, field in ((0, 1, "B must be 1..4096"), (4097, 1, "B must be 1..4096"), (1, 0, "R must be 1..8"), (1, 9, "R must be 1..8")):
        assert lib.lg_select_workspace(B, R) == -1 and field in err()
    assert lib.lg_select_workspace(4096, 8) > 0
    v = torch.zeros(2, 16, device=DEV)
    ranks = torch.ones(2, 1, dtype=torch.int64, device=DEV)
    out, nk = torch.zeros(2, 1, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = torch.zeros(lib.lg_select_workspace(2, 1) // 8, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda ld, B, n, R, o=out: lib.lg_select_kth(p(v), ld, B, n, None, p(ranks), R, p(o) if o is not None else None, p(nk), p(ws), None)
    for args, field in (((16, 2, 0, 1), "n must be 1..2^31-1"), ((16, 2, 2 ** 31, 1), "n must be 1..2^31-1"), ((15, 2, 16, 1), "ld must be at least n"),
                        ((16, 0, 16, 1), "B must be 1..4096"), ((16, 2, 16, 9), "R must be 1..8"), ((16, 2, 16, 1, None), "missing array")):
        assert call(*args) == -1 and field in err(), args
    from legged_gym_dev_amd.tube.calibrate import select_kth
    from legged_gym_dev_amd.lib import LeggedHipError
    with pytest.raises(ValueError, match="R must be 1..8"):
        select_kth(v, torch.ones(2, 9, dtype=torch.int64))
    with pytest.raises(LeggedHipError, match="no CPU fallback"):
        select_kth(v.cpu(), [1])
    torch.cuda.synchronize()
