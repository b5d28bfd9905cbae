"""Float64 reference, input families and the case list for the GEMM launches of the PPO update (csrc/ppo_gemm.hip), as the product
launches them: one or two problems per launch (actor on blockIdx.z = 0, critic on 1), every GemmArgs field in play, through
ppok_debug_gemm_args.  tests/test_ppo_gemm_host.py checks on the CPU that the inputs have the properties the bounds below rest on;
tests/test_hip_ppo_gemm.py runs the cases on the GPU.

Logical form of every problem: a [M][K], b [K][N], P = a . b, K the reduction length.  In memory (GemmArgs):
  kind 0 forward          A [M][K], B [N][K] (= b^T),  C [M][N] = act(P + bias[n])
  kind 1 input gradient   A [M][K], B [K][N],          C [M][N] = P * act'(aux[m][n]);  colsum[n] += sum_m C[m][n]
  kind 2 weight gradient  A [K][M] (= a^T), B [K][N],  C [M][nstore] += P[:, :nstore]   (split-K float atomics over the slices)

Input families -- none of their bounds comes from the library under test:
  int       every operand entry an integer in [-15, 15]; bias / colsum / C before the launch integers in [-1000, 1000].  Every term
            product and every partial sum is an integer below 2^24, so fp32 is exact in any order: the result must EQUAL the
            reference.  A wrong tile, a dropped k-tail, a missed or doubled slice, a stale pad column: a nonzero difference.
  planes_a  a has entries +-(1 + n 2^-16), 0 <= n < 2^16 (17 significant bits: the h, m and l bf16 terms are all live), b entries in
  planes_b  {-1, 0, 1} with at most 120 nonzero along k per output element; planes_b the other way round.  bias / C before are
            multiples of 2^-16 below 16.  All partial sums are multiples of 2^-16 below 256 = 24 bits: exact again.  Pins the routing
            of each operand's m and l planes through staging, the transposing LDS reads and the weight-plane images.
  deep_a    as planes_a / planes_b with entries +-(1 + n 2^-22), 0 <= n < 2^22 (23 significant bits) and ONE nonzero along k per output
  deep_b    element, bias / C before multiples of 2^-22 below 2: sums are multiples of 2^-22 below 4, exact.  Added because the host test
            shows that h + m already carry all 17 bits of the planes_* entries (their l term is zero throughout): these make l live.
  rand      randn scaled by 2^randint(-12, 12) per reduction index, the inverse scale on the other operand.  Two bounds, with
            S = |a| . |b| (+ |bias| or |C before|) in float64:
              structural  |C - ref| <= (6 K + slices + 8) 2^-24 S: one rounding per accumulated term product and per atomic, the
                          dropped term products <= 2^-23 (ppo_split_bf16.h)
              precision   E_k <= PRECISION_M E_y + 2^-24, E = max |. - ref| / S, the yardstick Y the textbook fp32 evaluation
                          (yardstick(): acc += a[:, k, None] * b[None, k, :] in torch.float32)
"""
import ctypes
import zlib

import torch

F64 = torch.float64
U = 2.0 ** -24                       # unit roundoff of fp32

# kernel codes reported by the launchers (GK_* of csrc/ppo_gemm.hip)
GEMM_SMALL, GEMM_BIG, PL1_SMALL, PL1_BIG, PL2_SMALL, PL2_BIG, GLDS, DW_SMALL, DW_BIG, REF = range(1, 11)
KERNEL_NAMES = {GEMM_SMALL: "k_gemm 64x64", GEMM_BIG: "k_gemm 128x128", PL1_SMALL: "k_gemm planes-1 64x64", PL1_BIG: "k_gemm planes-1 128x128",
                PL2_SMALL: "k_gemm planes-2 64x64", PL2_BIG: "k_gemm planes-2 128x128", GLDS: "k_gemm_glds", DW_SMALL: "k_gemm_dw_t 64x64",
                DW_BIG: "k_gemm_dw_t 128x128", REF: "k_gemm_ref"}

# E_k <= PRECISION_M * E_y + 2^-24: twice the largest E_k / E_y measured per kernel path on the MI355X
# -- 1.39 (k_gemm 64 x 64 tiles, fp32 B) -- rounded up to one digit; the table is in the docstring of tests/test_hip_ppo_gemm.py.  E_k and
# E_y are maxima over the elements of BOTH problems of a launch: one figure per launch.
PRECISION_M = 3.0

ALL = ("int", "planes_a", "planes_b", "deep_a", "deep_b", "rand")


class GemmArgs(ctypes.Structure):
    """Mirror of GemmArgs (csrc/ppo_device.h); ppok_debug_gemm_args_size() must equal ctypes.sizeof of it."""
    _fields_ = [(n, ctypes.c_void_p * 2) for n in ("A", "B", "bias", "aux", "C", "colsum")] + \
               [(n, ctypes.c_int * 2) for n in ("M", "N", "K", "lda", "ldb", "ldc", "ldaux")] + \
               [("elu", ctypes.c_int), ("Bpl", ctypes.c_void_p * 2), ("pl_stride", ctypes.c_int64)] + \
               [(n, ctypes.c_int * 2) for n in ("Kpl", "ldbpl", "nstore")] + \
               [("det_base", ctypes.c_void_p), ("det64", ctypes.c_void_p), ("det_n", ctypes.c_int64)]


def bind(lib):
    """Declares the two debug entries on a loaded library; returns sizeof(GemmArgs) as the library was compiled."""
    lib.ppok_debug_gemm_args.argtypes = [ctypes.POINTER(GemmArgs), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_int)]
    lib.ppok_debug_gemm_args.restype = ctypes.c_int
    lib.ppok_debug_gemm_args_size.restype = ctypes.c_int
    return lib.ppok_debug_gemm_args_size()
EXPF_RTOL, EXPF_ATOL = 2e-4, 2e-5     # activations on __expf (codes 1, 2, 5, 6): test_other_activations_forward_and_gradients
SELU_L, SELU_A = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


# ------------------------------------------------------------------------------------------------ the dispatch arithmetic, restated
def dw_splits(probs):
    """Reduction slices the product picks for a weight-gradient launch (dw_splits of csrc/ppo_gemm.hip)."""
    tiles = rows = 0
    for M, N, K in probs:
        t = 128 if (M > 64 and N > 64) else 64
        tiles = max(tiles, -(-M // t) * -(-N // t))
        rows = max(rows, K)
    s = min(-(-384 // tiles), max(rows // 256, 1))
    if s >= 8:
        s &= ~7
    return max(s, 1)


def k_tiles_per_slice(K, slices):
    """k-tiles of 32 in a full slice, and the number of slices that are not empty (k_slice)."""
    per = -(-(-(-K // slices)) // 32) * 32
    return per // 32, -(-K // per)


# ------------------------------------------------------------------------------------------------ activations in float64
def act_fwd64(code, v):
    if code == 1:
        return torch.where(v > 0, v, torch.expm1(v))
    if code == 2:
        return torch.where(v > 0, SELU_L * v, SELU_L * SELU_A * torch.expm1(v))
    if code == 3:
        return v.clamp_min(0)
    if code == 4:
        return torch.where(v > 0, v, 0.01 * v)
    if code == 5:
        return torch.tanh(v)
    if code == 6:
        return torch.sigmoid(v)
    return v


def act_slope64(code, v):
    """d act / d v at the pre-activation v."""
    one = torch.ones_like(v)
    if code == 1:
        return torch.where(v > 0, one, torch.exp(v))
    if code == 2:
        return torch.where(v > 0, SELU_L * one, SELU_L * SELU_A * torch.exp(v))
    if code == 3:
        return (v > 0).to(v.dtype)
    if code == 4:
        return torch.where(v > 0, one, 0.01 * one)
    if code == 5:
        return 1 - torch.tanh(v) ** 2
    if code == 6:
        s = torch.sigmoid(v)
        return s * (1 - s)
    return one


ACT_LIPSCHITZ = {0: 1.0, 1: 1.0, 2: SELU_L * SELU_A, 3: 1.0, 4: 1.0, 5: 1.0, 6: 0.25}


def act_bwd64(code, a):
    """The derivative through the activation's OUTPUT a, as the backward epilogue takes it."""
    one = torch.ones_like(a)
    if code == 1:
        return torch.where(a > 0, one, a + 1)
    if code == 2:
        return torch.where(a > 0, SELU_L * one, a + SELU_L * SELU_A)
    if code == 3:
        return (a > 0).to(a.dtype)
    if code == 4:
        return torch.where(a > 0, one, 0.01 * one)
    if code == 5:
        return 1 - a * a
    if code == 6:
        return a * (1 - a)
    return one


# ------------------------------------------------------------------------------------------------ the split into bf16 planes
def split_planes(w):
    """The three bf16 terms of fp32 w (round to nearest even at each level, as v_cvt_pk_bf16_f32 in split2): [3, ...] bfloat16."""
    h = w.to(torch.bfloat16)
    r = w - h.float()
    m = r.to(torch.bfloat16)
    l = (r - m.float()).to(torch.bfloat16)
    return torch.stack([h, m, l])


# ------------------------------------------------------------------------------------------------ inputs
def _three_plane(shape, g, bits=16):
    n = torch.randint(0, 1 << bits, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (sign * (1 + n * 2.0 ** -bits)).float()


def _ternary(lines, K, g, cap=120):
    """[lines][K] in {-1, 0, 1}: dense for K <= cap, else `cap` places per line (their own for every line) hold +-1."""
    t = torch.randint(-1, 2, (lines, K), generator=g).float()
    if K > cap:
        rank = torch.rand(lines, K, generator=g).argsort(dim=1).argsort(dim=1)
        t = torch.where(rank < cap, torch.where(t == 0, torch.ones_like(t), t), torch.zeros_like(t))
    return t


def build_problem(case, z, fam):
    """Problem z of the case with the inputs of family `fam`, on the CPU: logical a [M][K], b [K][N] (fp32), and what the epilogue
    reads -- bias [N] or None (kind 0), aux [M][N] and colsum before the launch [N] or None (kind 1), C before the launch [M][nstore]
    (kind 2).  Seeded by (label, z, family)."""
    M, N, K = case["probs"][z]
    kind, act = case["kind"], case["act"]
    g = torch.Generator().manual_seed(zlib.crc32(f"{case['label']}/{z}/{fam}".encode()))
    if fam == "int":
        a = torch.randint(-15, 16, (M, K), generator=g).float()
        b = torch.randint(-15, 16, (K, N), generator=g).float()
        addend = lambda *s: torch.randint(-1000, 1001, s, generator=g).float()
    elif fam in ("planes_a", "planes_b", "deep_a", "deep_b"):
        bits, cap, top = (16, 120, 1 << 20) if fam.startswith("planes") else (22, 1, 1 << 23)
        if fam.endswith("_a"):
            a, b = _three_plane((M, K), g, bits), _ternary(N, K, g, cap).t().contiguous()
        else:
            a, b = _ternary(M, K, g, cap), _three_plane((K, N), g, bits)
        addend = lambda *s: (torch.randint(-top + 1, top, s, generator=g).double() * 2.0 ** -bits).float()
    else:
        scale = torch.exp2(torch.randint(-12, 12, (K,), generator=g).float())
        a = torch.randn(M, K, generator=g) * scale
        b = torch.randn(K, N, generator=g) / scale[:, None]
        addend = lambda *s: torch.randn(*s, generator=g)
    p = dict(M=M, N=N, K=K, a=a, b=b, bias=None, aux=None, colsum0=None, C0=None, nstore=case["nstore"][z] or N)
    if kind == 0 and case["bias"][z]:
        p["bias"] = addend(N)
    if kind == 1:
        p["aux"] = (torch.rand(M, N, generator=g, dtype=F64) * 3 - 1).float()        # (-1, 2): both branches of every act_bwd
        if fam in ("int", "rand"):                                                   # (a sum over M rows of the plane families' C
            p["colsum0"] = addend(N)                                                 # is not exact in fp32: no colsum there)
    if kind == 2:
        p["C0"] = addend(M, p["nstore"])
    return p


def reference(case, p, dev="cpu"):
    """Float64 on `dev`: out (what C must hold after the launch), pre (before the activation; kind 0), factor (act'(aux); kind 1), S
    (|a| . |b| + |bias| or |C before|, per stored element) and colsum (kind 1, with colsum0)."""
    kind, act = case["kind"], case["act"]
    a, b = p["a"].to(dev, F64), p["b"].to(dev, F64)
    P, S = a @ b, a.abs() @ b.abs()
    r = {}
    if kind == 0:
        if p["bias"] is not None:
            bias = p["bias"].to(dev, F64)
            P, S = P + bias, S + bias.abs()
        r.update(pre=P, out=act_fwd64(act, P), S=S)
    elif kind == 1:
        f = act_bwd64(act, p["aux"].to(dev, F64))
        r.update(factor=f, out=P * f, S=S)
        if p["colsum0"] is not None:
            r["colsum"] = p["colsum0"].to(dev, F64) + r["out"].sum(0)
    else:
        C0 = p["C0"].to(dev, F64)
        ns = p["nstore"]
        r.update(out=C0 + P[:, :ns], S=S[:, :ns] + C0.abs())
    return r


def yardstick(case, p, dev):
    """The textbook fp32 evaluation of the same launch on `dev`: a loop over k of rank-one updates in torch.float32, then the epilogue
    in fp32."""
    kind, act = case["kind"], case["act"]
    a, b = p["a"].to(dev), p["b"].to(dev)
    acc = torch.zeros(p["M"], p["N"], device=dev)
    for k in range(p["K"]):
        acc += a[:, k, None] * b[None, k, :]
    if kind == 0:
        if p["bias"] is not None:
            acc = acc + p["bias"].to(dev)
        return act_fwd64(act, acc)
    if kind == 1:
        return acc * act_bwd64(act, p["aux"].to(dev))
    return p["C0"].to(dev) + acc[:, :p["nstore"]]


def structural_bound(case, p, ref, slices):
    """Per stored element, float64.  (6 K + slices + 8) 2^-24 S before the activation.  Behind it: times the activation's slope at
    the reference where the whole interval ref +- bound lies on one branch, times its Lipschitz constant where the interval holds
    the kink at 0 (relu, lrelu, elu, selu) or for the smooth ones; codes on __expf add rtol 2e-4 / atol 2e-5 of the result.  Input
    gradient: times |act'(aux)|, which fp32 evaluates with up to three roundings of its own."""
    kind, act = case["kind"], case["act"]
    B = (6 * p["K"] + slices + 8) * U * ref["S"]
    if kind == 0:
        return bound_through_activation(act, ref["pre"], ref["out"], B)
    if kind == 1:
        B = B * ref["factor"].abs() + 4 * U * ref["out"].abs()
    if act in (1, 2, 5, 6):
        B = B + EXPF_RTOL * ref["out"].abs() + EXPF_ATOL
    return B


def bound_through_activation(act, pre, out, B):
    """The slope and kink rule of structural_bound on its own: B bounds the error of the pre-activation `pre` (float64 reference, `out`
    = act(pre)); returns the bound behind the activation of code `act`, the __expf terms included."""
    if act:
        slope = act_slope64(act, pre).abs()
        if act in (5, 6):                       # smooth: the largest slope on the interval is at its end nearer 0
            near = torch.where(pre.abs() > B, pre - torch.sign(pre) * B, torch.zeros_like(pre))
            slope = act_slope64(act, near).abs()
        else:
            slope = torch.where(pre.abs() > B, torch.maximum(slope, act_slope64(act, pre + B).abs()),
                                torch.full_like(pre, ACT_LIPSCHITZ[act]))
        B = B * slope + U * out.abs()
    if act in (1, 2, 5, 6):
        B = B + EXPF_RTOL * out.abs() + EXPF_ATOL
    return B


# ------------------------------------------------------------------------------------------------ cases
def _case(label, kind, probs, kernel, slices=1, **kw):
    c = dict(label=label, kind=kind, probs=tuple(tuple(p) for p in probs), kernel=kernel, slices=slices, splits=0, act=0,
             bias=(True, False), planes=False, kpl=(0, 0), nstore=(0, 0), ld_extra=0, offset="", families=None)
    c.update(kw)
    if c["families"] is None:
        c["families"] = ALL if c["act"] == 0 else ("int", "rand") if c["act"] == 3 else ("rand",)
    return c


def _both(label, kind, small, large, kernel, slices=1, **kw):
    """The pair with the smaller problem once at z = 0 and once at z = 1; per-problem options are given as (small's, large's)."""
    out = []
    for tag, order in (("z0small", (0, 1)), ("z1small", (1, 0))):
        kws = dict(kw)
        for k in ("nstore", "kpl", "bias"):
            if k in kw:
                kws[k] = tuple(kw[k][i] for i in order)
        out.append(_case(f"{label}-{tag}", kind, [(small, large)[i] for i in order], kernel, slices, **kws))
    return out


def _cases():
    c = []
    I = ("int",)
    # ---------------------------------------------------------------- weight gradient: (M, N, K = minibatch rows)
    # the launches that lost slices before the tile-map fix, the product's own split (splits = 0) on unequal pairs.  The three at the
    # benchmark's 24 576 rows run the int family alone (the structural test; a float64 product and a 24 576-step yardstick per family
    # would take seconds each): the same launch arithmetic runs in every family at 2048 rows below
    c += _both("dw-priv-65-169-l0-24576", 2, (512, 96, 24576), (512, 192, 24576), DW_BIG, 48, nstore=(65, 169), families=I)
    c += _both("dw-widths-512-256-l1-24576", 2, (128, 256, 24576), (256, 512, 24576), DW_BIG, 48, families=I)
    c += _both("dw-lstm-wih-65-169-h64-24576", 2, (256, 96, 24576), (256, 192, 24576), DW_BIG, 96, nstore=(65, 169), families=I)
    c += _both("dw-priv-48-100-l0-2048", 2, (64, 64, 2048), (64, 128, 2048), DW_SMALL, 8, nstore=(48, 100))
    c += _both("dw-widths-64-128-l1-2048", 2, (32, 64, 2048), (32, 128, 2048), DW_SMALL, 8)
    c += _both("dw-widths-64-128-l1-2047", 2, (32, 64, 2047), (32, 128, 2047), DW_SMALL, 7)
    # product splits at 2047 / 2048 / 4096 rows: 7, 8, 16 slices -- both xcd_tile branches
    c += _both("dw-64x64-64x128-2047", 2, (64, 64, 2047), (64, 128, 2047), DW_SMALL, 7)
    c += _both("dw-64x64-64x128-2048", 2, (64, 64, 2048), (64, 128, 2048), DW_SMALL, 8)
    c += _both("dw-64x64-64x128-4096", 2, (64, 64, 4096), (64, 128, 4096), DW_SMALL, 16)
    # forced splits 1, 3, 8, 16; 1, 2 and 3 k-tiles per slice (both parities of the PD = 2 prefetch); K = 300 in 8 slices of 64 rows
    # leaves three empty trailing slices; K = 777 no multiple of 32
    c += _both("dw-split1-k96", 2, (32, 64, 96), (32, 128, 96), DW_SMALL, 1, splits=1)
    c += _both("dw-split3-k777", 2, (64, 64, 777), (64, 128, 777), DW_SMALL, 3, splits=3)
    c += _both("dw-split8-k256-1tile", 2, (64, 64, 256), (64, 128, 256), DW_SMALL, 8, splits=8)
    c += _both("dw-split8-k512-2tiles", 2, (32, 64, 512), (32, 128, 512), DW_SMALL, 8, splits=8)
    c += _both("dw-split8-k768-3tiles", 2, (64, 64, 768), (64, 128, 768), DW_SMALL, 8, splits=8)
    c += _both("dw-split16-k1000", 2, (64, 64, 1000), (64, 128, 1000), DW_SMALL, 16, splits=16)
    c += _both("dw-split8-k300-empty-slices", 2, (64, 64, 300), (64, 128, 300), DW_SMALL, 8, splits=8)
    # 16 against 4 small tiles; 128 x 128 tiles (big_tiles * splits >= 192, both dimensions > 64) with 48 slices and with 49 (other branch)
    c += _both("dw-256x256-128x128-split8", 2, (128, 128, 512), (256, 256, 512), DW_SMALL, 8, splits=8)
    c += _both("dw-big-256x256-128x128-split48", 2, (128, 128, 1536), (256, 256, 1536), DW_BIG, 48, splits=48)
    c += _both("dw-big-250x200-100x130-split49", 2, (100, 130, 1573), (250, 200, 1573), DW_BIG, 49, splits=49)
    # unequal pairs whose tile counts are equal; equal pairs; one problem
    c += _both("dw-equal-tiles-40x50-64x64", 2, (40, 50, 2048), (64, 64, 2048), DW_SMALL, 8)
    c.append(_case("dw-equal-pair-128x64", 2, [(128, 64, 2048)] * 2, DW_SMALL, 8))
    c.append(_case("dw-one-problem-96x160", 2, [(96, 160, 555)], DW_SMALL, 2))
    # load forms: 16-byte (above), element-wise by M = 77, by N = 1 and by a base pointer one float off
    c += _both("dw-elementwise-m77", 2, (77, 64, 300), (77, 128, 300), DW_SMALL, 8, splits=8)
    c += _both("dw-elementwise-n1", 2, (64, 1, 2048), (128, 1, 2048), DW_SMALL, 8)
    c += _both("dw-elementwise-offset-a", 2, (64, 64, 2048), (64, 128, 2048), DW_SMALL, 8, offset="A")
    c += _both("dw-elementwise-offset-b", 2, (64, 64, 520), (64, 128, 520), DW_SMALL, 3, splits=3, offset="B")
    # nstore: 96 columns computed, 65 stored on rows of 65 floats
    c += _both("dw-nstore-65-of-96", 2, (64, 96, 2048), (128, 192, 2048), DW_SMALL, 8, nstore=(65, 169))
    c.append(_case("dw-nstore-65-of-96-one", 2, [(40, 96, 333)], DW_SMALL, 3, splits=3, nstore=(65, 0)))

    # ---------------------------------------------------------------- forward: (M, N, K)
    for act in range(7):                       # every activation at one ragged and one interior shape; bias on z = 0, off on z = 1
        c.append(_case(f"fwd-act{act}-ragged", 0, [(65, 77, 45), (33, 50, 129)], GEMM_SMALL, act=act))
        c.append(_case(f"fwd-act{act}-interior-planes", 0, [(128, 64, 64), (64, 128, 64)], PL1_SMALL, act=act, planes=True))
    # load forms of k_gemm on fp32 B: interior (above: no), here interior / masked 16-byte / element-wise
    c += _both("fwd-interior", 0, (64, 64, 64), (128, 128, 96), GEMM_SMALL)
    c += _both("fwd-masked-k72", 0, (63, 60, 72), (130, 68, 72), GEMM_SMALL)
    c += _both("fwd-elementwise-k65", 0, (64, 64, 65), (70, 128, 65), GEMM_SMALL, bias=(False, True))
    c += _both("fwd-elementwise-offset", 0, (64, 64, 64), (64, 128, 64), GEMM_SMALL, offset="AB")
    # 128 x 128 tiles from 192 of them: 8 x 24 and 7 x 28 (row-tile counts 8 and 7: the two xcd_tile branches of this family)
    c += _both("fwd-big-8x24", 0, (300, 200, 45), (1021, 3067, 45), GEMM_BIG, families=("int", "rand"))
    c += _both("fwd-big-7x28", 0, (128, 3584, 64), (896, 3584, 64), GEMM_BIG, families=("int", "rand"))
    # the weight planes as B: small and big tiles (N no multiple of 128: not the LDS-DMA kernel), k-tail of 8
    c += _both("fwd-planes-small-k72", 0, (65, 72, 72), (100, 136, 72), PL1_SMALL, planes=True)
    c += _both("fwd-planes-small-7-row-tiles", 0, (64, 8, 48), (445, 8, 48), PL1_SMALL, planes=True)
    c += _both("fwd-planes-small-8-row-tiles", 0, (64, 8, 48), (512, 8, 48), PL1_SMALL, planes=True)
    c += _both("fwd-planes-big-8x24", 0, (129, 264, 72), (1000, 3064, 72), PL1_BIG, planes=True, families=("int", "planes_b", "deep_b", "rand"))
    # LDS-DMA forward: N a multiple of 128, K of 32, M > 64; ragged last row tile, M = 65, 7 and 8 row tiles
    c += _both("fwd-glds-m65-m200", 0, (65, 128, 32), (200, 256, 32), GLDS, planes=True)
    c += _both("fwd-glds-7-row-tiles", 0, (130, 128, 96), (893, 128, 96), GLDS, planes=True)
    c += _both("fwd-glds-8-row-tiles", 0, (1, 128, 64), (1024, 128, 64), GLDS, planes=True, bias=(False, True))
    # padded first layer: K = 65 against plane rows (and minibatch rows) of Kpl = ldbpl = 96
    c += _both("fwd-kpl-65-of-96-glds", 0, (100, 128, 65), (300, 256, 65), GLDS, planes=True, kpl=(96, 96))
    c += _both("fwd-kpl-65-of-96-planes", 0, (100, 72, 65), (300, 256, 65), PL1_SMALL, planes=True, kpl=(96, 96))
    # one problem qualifies for a faster path alone: the launch must refuse it for both
    c += _both("fwd-glds-refused-by-n72", 0, (100, 72, 64), (200, 128, 64), PL1_SMALL, planes=True)
    c += _both("fwd-glds-refused-by-k40", 0, (100, 128, 40), (200, 128, 64), PL1_SMALL, planes=True)
    c += _both("fwd-planes-refused-by-k45", 0, (100, 128, 45), (200, 128, 64), GEMM_SMALL, planes=True)
    c.append(_case("fwd-one-problem-k129", 0, [(77, 130, 129)], GEMM_SMALL))

    # ---------------------------------------------------------------- input gradient: (M, N, K = the layer's outputs)
    for act in range(7):
        c.append(_case(f"dx-act{act}-ragged", 1, [(63, 40, 72), (129, 77, 16)], GEMM_SMALL, act=act, ld_extra=3))
        c.append(_case(f"dx-act{act}-interior-planes", 1, [(128, 64, 64), (64, 128, 32)], PL2_SMALL, act=act, planes=True))
    c += _both("dx-f32-m1-m65", 1, (1, 8, 16), (65, 264, 384), GEMM_SMALL, ld_extra=5)
    c += _both("dx-f32-elementwise-offset", 1, (63, 40, 72), (129, 264, 72), GEMM_SMALL, offset="AB")
    c += _both("dx-f32-big", 1, (129, 40, 16), (12288, 264, 16), GEMM_BIG, families=("int", "rand"), ld_extra=4)
    c += _both("dx-planes-m1-m65", 1, (1, 8, 16), (65, 264, 384), PL2_SMALL, planes=True, ld_extra=8)
    c += _both("dx-planes-m63-m129", 1, (63, 40, 72), (129, 264, 72), PL2_SMALL, planes=True)
    c += _both("dx-planes-7-8-row-tiles", 1, (445, 8, 16), (512, 40, 16), PL2_SMALL, planes=True)
    c += _both("dx-planes-big", 1, (129, 40, 72), (12288, 264, 72), PL2_BIG, planes=True, families=("int", "planes_b", "deep_b", "rand"), ld_extra=8)
    c += _both("dx-planes-refused-by-n77", 1, (63, 77, 16), (129, 264, 16), GEMM_SMALL, planes=True)
    return tuple(c)


CASES = _cases()


def case_id(c):
    return c["label"]


def runs():
    """(case, family) of every launch the GPU test makes."""
    return [(c, f) for c in CASES for f in c["families"]]


def run_id(r):
    return f"{r[0]['label']}/{r[1]}"
