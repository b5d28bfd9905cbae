"""The GEMM launches of the PPO update against float64, launched as the product launches them (ppok_debug_gemm_args on a caller's
GemmArgs): two problems per launch with the smaller one at either z, every field in play, the kernel and the reduction slices read
back from the launcher.  Reference, input families, bounds and cases: tests/gemm_ref.py; the conditions those bounds rest on:
tests/test_ppo_gemm_host.py.

Every buffer lies between guard bands, and rows longer than their payload carry pad columns: inputs hold NaN there (a read of
a pad column or past an end poisons the result), outputs a sentinel that must survive the launch.

Measured E_k / E_y (rand family, activation codes 0, 3, 4; E = max |. - ref| / S over both problems of a launch; the largest ratio
over the launches of a kernel path, MI355X):
    k_gemm, fp32 B          64 x 64 tiles 1.39 (23 launches)    128 x 128 tiles 0.88 (6)
    k_gemm, planes path 1   64 x 64 tiles 1.04 (15)             128 x 128 tiles 0.78 (2)
    k_gemm, planes path 2   64 x 64 tiles 1.07 (9)              128 x 128 tiles 0.74 (2)
    k_gemm_glds             0.92 (8)
    k_gemm_dw_t             64 x 64 tiles 0.73 (43)             128 x 128 tiles 0.19 (4)
Asserted: E_k <= 3 E_y + 2^-24 (gemm_ref.PRECISION_M: twice 1.39, rounded up to one digit).  No path comes near the
sqrt(6) that six term products per element would suggest at worst, let alone 4.  The structural bound is used to 1.8 % at worst.

At the commit before the tile-map fix of k_gemm_dw_t (the remapped tile, not blockIdx.x, decides whether a workgroup belongs to the
problem) every weight-gradient launch here whose two problems differ in tile count AND whose slice count is a multiple of 8 failed
-- 186 of the 288 weight-gradient runs, in every family: the smaller problem received about half (a quarter for
512/256 against 256/128 widths) of its reduction slices -- while those with 1, 3, 7 or 49 slices or equal tile counts passed.
"""
import ctypes

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

GUARD = 64                            # floats on either side of every buffer (a multiple of 4: the payload keeps its 16-byte alignment)
SENTINEL = -12345.0
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    lib = load()
    assert gr.bind(lib) == ctypes.sizeof(gr.GemmArgs), "GemmArgs: the ctypes mirror and the library disagree"
    return lib


def test_gemm_args_mirror_has_the_library_size(lib):
    assert lib.ppok_debug_gemm_args_size() == ctypes.sizeof(gr.GemmArgs)


class Buf:
    """A [rows][cols] payload on rows of `ld` floats, `off` floats past a 16-byte boundary, between guard bands: everything that is
    not payload holds `fill`."""

    def __init__(self, payload, ld, fill, off=0):
        rows, cols = payload.shape
        assert ld >= cols
        self.rows, self.cols, self.ld, self.lo = rows, cols, ld, GUARD + off
        flat = torch.full((self.lo + rows * ld + GUARD,), float(fill))
        flat[self.lo:self.lo + rows * ld].view(rows, ld)[:, :cols] = payload
        self.mask = torch.zeros(flat.shape, dtype=torch.bool)
        self.mask[self.lo:self.lo + rows * ld].view(rows, ld)[:, :cols] = True
        self.fill = float(fill)
        self.flat = flat.to(DEV)
        self.ptr = self.flat.data_ptr() + 4 * self.lo

    def payload(self):
        return self.flat[self.lo:self.lo + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def untouched(self):
        """True when nothing outside the payload was written."""
        return bool((self.flat[~self.mask.to(DEV)] == self.fill).all())


def _marshal(case, probs):
    """GemmArgs of the case on the device, and the buffers it points into (kept alive by the caller)."""
    kind, nz = case["kind"], len(probs)
    g = gr.GemmArgs()
    keep = []
    nan = float("nan")
    offA, offB = int("A" in case["offset"]), int("B" in case["offset"])
    ex = case["ld_extra"]
    outs = []
    # the weight planes of both problems in one image: plane p of problem z at base + p * pl_stride + seg[z]
    seg, Ws = [0], []
    for z, p in enumerate(probs):
        Kp = case["kpl"][z] or p["K"]
        W = torch.zeros(p["N"], Kp) if kind == 0 else p["b"]
        if kind == 0:
            W[:, :p["K"]] = p["b"].t()
        Ws.append(W)
        seg.append(seg[-1] + (W.numel() + 7) // 8 * 8)
    if case["planes"]:
        stride = seg[-1]
        image = torch.zeros(3, stride + 8, dtype=torch.bfloat16)
        for z, W in enumerate(Ws):
            image[:, seg[z]:seg[z] + W.numel()] = gr.split_planes(W.contiguous()).reshape(3, -1)
        image = image[:, :stride].contiguous().view(torch.int16).reshape(-1)
        image = torch.cat([image, torch.zeros(8, dtype=torch.int16)]).to(DEV)
        keep.append(image)
        g.pl_stride = stride
    for z, p in enumerate(probs):
        M, N, K = p["M"], p["N"], p["K"]
        Kp = case["kpl"][z]
        if kind == 2:
            A, B = Buf(p["a"].t(), M, nan, offA), Buf(p["b"], N, nan, offB)
            C = Buf(p["C0"], p["nstore"], SENTINEL)
            g.nstore[z] = case["nstore"][z]
        else:
            # padded first layer: the minibatch rows are Kpl long with ZERO pad columns (the product's contract)
            A = Buf(torch.cat([p["a"], torch.zeros(M, Kp - K)], 1) if Kp else p["a"], Kp or K, nan, offA)
            B = Buf(p["b"].t() if kind == 0 else p["b"], K if kind == 0 else N, nan, offB)
            C = Buf(torch.full((M, N), SENTINEL), N + ex, SENTINEL)
        g.A[z], g.B[z], g.C[z] = A.ptr, B.ptr, C.ptr
        g.M[z], g.N[z], g.K[z] = M, N, K
        g.lda[z], g.ldb[z], g.ldc[z] = A.ld, B.ld, C.ld
        keep += [A, B]
        out = dict(C=C, colsum=None)
        if kind == 0:
            g.Kpl[z], g.ldbpl[z] = Kp, Kp
            if p["bias"] is not None:
                bias = Buf(p["bias"][None], N, nan)
                g.bias[z] = bias.ptr
                keep.append(bias)
        if kind == 1:
            aux = Buf(p["aux"], N + 2 * ex, nan)
            g.aux[z], g.ldaux[z] = aux.ptr, aux.ld
            keep.append(aux)
            if p["colsum0"] is not None:
                out["colsum"] = Buf(p["colsum0"][None], N, SENTINEL)
                g.colsum[z] = out["colsum"].ptr
        if case["planes"]:
            g.Bpl[z] = keep[0].data_ptr() + 2 * seg[z]
            if kind == 0 and not Kp:
                assert B.ld == Ws[z].shape[1]
        outs.append(out)
    g.elu = case["act"]
    return g, outs, keep


RATIOS = {}                           # kernel -> largest E_k / E_y seen in this session (printed by the measurement run)


@pytest.mark.parametrize("run", gr.runs(), ids=gr.run_id)
def test_gemm_launch_matches_float64(lib, run):
    case, fam = run
    kind, nz = case["kind"], len(case["probs"])
    probs = [gr.build_problem(case, z, fam) for z in range(nz)]
    g, outs, keep = _marshal(case, probs)
    info = (ctypes.c_int * 2)(0, 0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ppok_debug_gemm_args(ctypes.byref(g), nz, kind, case["splits"], st, info) == 0
    torch.cuda.synchronize()
    assert (info[0], info[1]) == (case["kernel"], case["slices"]), \
        f"launched {gr.KERNEL_NAMES.get(info[0], info[0])} with {info[1]} slices, the case names {gr.KERNEL_NAMES[case['kernel']]} with {case['slices']}"
    e_k = e_y = 0.0
    for z, p in enumerate(probs):
        ref = gr.reference(case, p, DEV)
        C, cs = outs[z]["C"], outs[z]["colsum"]
        got = C.payload().double()
        assert C.untouched(), f"z={z}: written outside C[M][{C.cols}] (pad columns of the rows, or past an end)"
        assert bool(torch.isfinite(got).all()), f"z={z}: non-finite result (a pad column or a guard band was read)"
        diff = (got - ref["out"]).abs()
        if cs is not None:
            assert cs.untouched(), f"z={z}: written outside colsum[N]"
            cgot = cs.payload().double()[0]
        if fam != "rand":
            bad = int((diff != 0).sum())
            assert bad == 0, (f"z={z} {p['M']}x{p['N']}x{p['K']}: {bad} of {diff.numel()} elements differ from the exact result, "
                              f"max |diff| {float(diff.max())}, sum |got - before| / sum |ref - before| {_moved(got, ref['out'], p):.4f}")
            if cs is not None:
                assert torch.equal(cgot, ref["colsum"]), f"z={z}: colsum differs from the exact column sums"
            continue
        bound = gr.structural_bound(case, p, ref, info[1])
        worst = float((diff / bound.clamp_min(1e-300)).max())
        print(f"STRUCT {run_label(run)} z={z} worst diff/bound {worst:.4f}")
        assert bool((diff <= bound).all()), f"z={z}: structural bound exceeded {worst:.3f}x"
        if cs is not None:       # against the kernel's own C: what the column sums add, M + 8 roundings
            own = p["colsum0"].to(DEV).double() + got.sum(0)
            cb = (p["M"] + 8) * gr.U * (got.abs().sum(0) + p["colsum0"].to(DEV).double().abs())
            assert bool(((cgot - own).abs() <= cb).all()), f"z={z}: colsum off by {float(((cgot - own).abs() / cb.clamp_min(1e-300)).max()):.3f}x its bound"
        if case["act"] in (0, 3, 4):
            Y = gr.yardstick(case, p, DEV).double()
            S = ref["S"].clamp_min(1e-300)
            e_k = max(e_k, float((diff / S).max()))
            e_y = max(e_y, float(((Y - ref["out"]).abs() / S).max()))
    if fam == "rand" and case["act"] in (0, 3, 4):
        ratio = e_k / e_y if e_y > 0 else float("inf") if e_k > 0 else 0.0
        RATIOS[info[0]] = max(RATIOS.get(info[0], 0.0), ratio)
        print(f"RATIO {gr.KERNEL_NAMES[info[0]]} | {run_label(run)} E_k {e_k:.3e} E_y {e_y:.3e} ratio {ratio:.3f}")
        assert e_k <= gr.PRECISION_M * e_y + gr.U, (e_k, e_y, ratio)


def _moved(got, ref, p):
    """How much of what the launch had to add arrived (weight gradient: 1 = all of it, 0.5 = half the slices)."""
    before = p["C0"].to(DEV).double() if p["C0"] is not None else torch.zeros_like(ref)
    return float((got - before).abs().sum()) / max(float((ref - before).abs().sum()), 1e-300)


def run_label(run):
    return gr.run_id(run)
