"""What the tests of lg_select_kth and lg_select_kth_grouped share (test_hip_select.py, test_hip_select_grouped.py,
test_hip_select_alignment.py): the comparison of a selection with its torch.sort reference, and the random bit patterns they select
from."""
import torch


def _assert_same(got, want, what=""):
    """torch.equal after mapping -0 to +0 on both sides, NaN positions by isnan; and on the bits the kernel's own promise: a zero
    comes back as +0.0 and a NaN as the canonical quiet NaN."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    g0 = torch.where(got == 0, torch.zeros_like(got), got)
    assert torch.equal(g0[~nan], want[~nan]), what
    bits = got.view(torch.int32)
    assert bool((bits[got == 0] == 0).all()), what + ": a zero must come back as +0.0"
    assert bool((bits[nan] == 0x7FC00000).all()), what + ": a NaN must come back as the canonical quiet NaN"


def _bit_patterns(B, n, seed):
    """Uniformly random 32-bit patterns viewed as fp32, with every special planted once per row for good measure."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2 ** 31, 2 ** 31, (B, n), generator=g, dtype=torch.int64).to(torch.int32)
    if n >= 8:
        v[:, :8] = torch.tensor([0x7F800000, -0x00800000, 0x7FC00001, -0x00000001, -0x80000000, 0, 1, -0x7FFFFFFF], dtype=torch.int32)
        v = v[:, torch.randperm(n, generator=g)]
    return v.view(torch.float32)
