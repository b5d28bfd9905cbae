"""The row walk that lg_select_kth and lg_select_kth_grouped share (sel_walk_row, csrc/select_device.h) under every alignment: the
row's start at each of the four offsets from a 16-byte boundary, crossed with the side array's -- the keep bytes at byte offsets
0..3, the group ids at 0, 4, 8, 12 bytes.  Through the raw C entries: the wrappers of tube/calibrate.py may copy a side array to an
aligned one.  One full chunk and a tail, so that both ends and the interior run; the references and the comparison are those of
test_hip_select.py and test_hip_select_grouped.py."""
import ctypes as C

import pytest
import torch

from tests.select_ref import _assert_same, _bit_patterns
from tests.test_hip_select import _reference as _reference_plain
from tests.test_hip_select_grouped import _random_groups, _reference as _reference_grouped

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


def test_every_alignment_of_the_row_and_of_the_side_array():
    from legged_gym_dev_amd.lib import load
    from legged_gym_dev_amd.tube.calibrate import coverage_fractions
    lib = load()
    B, G, cov = 2, 3, ("0.5", "0.9")
    R = len(cov)
    n = lib.lg_select_chunk() + 5
    ld = n + 3
    v = _bit_patterns(B, n, 91)
    keep = torch.rand(n, generator=torch.Generator().manual_seed(92)) < 0.5
    group = _random_groups(n, G, 93)
    n_kept = int(keep.sum())
    ranks = torch.tensor([[1, n_kept // 3], [n_kept // 2, n_kept]])
    want_plain, _ = _reference_plain(v, ranks, keep)
    want_grouped = _reference_grouped(v, group, G, cov)

    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fr = coverage_fractions(cov)
    num, den = (C.c_int64 * R)(*[f[0] for f in fr]), (C.c_int64 * R)(*[f[1] for f in fr])
    dranks = ranks.to(DEV)
    ws = torch.empty(lib.lg_select_workspace(B, R) // 8, dtype=torch.int64, device=DEV)
    wsg = torch.empty(lib.lg_select_grouped_workspace(B, G, R) // 8, dtype=torch.int64, device=DEV)
    # what lies around the arrays would change the result if it were read: -inf is below every value, a kept byte, a group that exists
    vbuf = torch.full((B * ld + 4,), -INF, device=DEV)
    kbuf = torch.ones(n + 4, dtype=torch.uint8, device=DEV)
    gbuf = torch.zeros(n + 4, dtype=torch.int32, device=DEV)
    assert vbuf.data_ptr() % 16 == 0 and kbuf.data_ptr() % 4 == 0 and gbuf.data_ptr() % 16 == 0
    for row_off in range(4):
        vbuf.fill_(-INF)
        values = vbuf[row_off:row_off + B * ld].view(B, ld)
        values[:, :n] = v.to(DEV)
        assert values.data_ptr() % 16 == 4 * row_off
        for side_off in range(4):
            what = f"row + {4 * row_off} bytes, "
            kbuf.fill_(1)
            dkeep = kbuf[side_off:side_off + n]
            dkeep.copy_(keep.to(DEV))
            assert dkeep.data_ptr() % 4 == side_off
            out, n_got = torch.empty(B, R, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
            rc = lib.lg_select_kth(p(values), ld, B, n, p(dkeep), p(dranks), R, p(out), p(n_got), p(ws), stream)
            assert rc == 0, lib.lg_last_error().decode()
            _assert_same(out, want_plain, what + f"keep + {side_off} bytes")
            assert int(n_got) == n_kept, what + f"keep + {side_off} bytes"

            gbuf.zero_()
            dgroup = gbuf[side_off:side_off + n]
            dgroup.copy_(group.to(DEV))
            assert dgroup.data_ptr() % 16 == 4 * side_off
            out = torch.empty(B, G, R, device=DEV)
            counts, granks = torch.zeros(G, dtype=torch.int64, device=DEV), torch.zeros(G, R, dtype=torch.int64, device=DEV)
            rc = lib.lg_select_kth_grouped(p(values), ld, B, n, p(dgroup), G, num, den, R, p(out), p(counts), p(granks), p(wsg), stream)
            assert rc == 0, lib.lg_last_error().decode()
            _assert_same(out, want_grouped[0], what + f"group + {4 * side_off} bytes")
            assert torch.equal(counts.cpu(), want_grouped[1]) and torch.equal(granks.cpu(), want_grouped[2]), what + f"group + {4 * side_off} bytes"
