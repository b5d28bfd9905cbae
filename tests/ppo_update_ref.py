"""Test-only case matrix and float64 reference for one whole feed-forward PPO minibatch of the HIP learner: lg_ppo_minibatch_backward
= sched::forward, the head, sched::backward (legged_gym_dev_amd/csrc/ppo_sched.hip, ppo_api.hip) -- the code that decides which
operand, leading dimension, pad width, plane image, aux, colsum and nstore every GEMM launch gets, and with them which kernel the
launchers of csrc/ppo_gemm.hip pick.  Plain torch, no GPU needed: tests/test_ppo_update_host.py checks on the CPU what the bands rest
on, tests/test_hip_ppo_update.py runs the cases through the library.

Built on tests/ppo_loss_ref.py: the same row steering (every row to a (ratio, advantage, v_new - v_old, v_new - return) target off
every branch boundary), the same reference (oracle.ppo_torch.PPO.minibatch_loss on a float64 model and bit-identical inputs), the same
bands.  Added: a privileged critic (OC != O, observations of its own), a relative-norm band on EVERY parameter tensor of both nets
and std (blocks()), and per case the kernel and reduction slices of every GEMM launch of the pass, in launch order (TRACES), which
the GPU test compares with the launch trace of the library (ppok_debug_gemm_trace).
"""
import functools

import torch

from tests import ppo_loss_ref as plr

ALG = plr.ALG
SEED = 15
# The fp32 restatement of the reference (reference(..., dtype=torch.float32)) may use at most this share of any band: the chains are
# up to five layers and 6145 rows long, and the library measured up to 1.4x its fp32 yardstick per GEMM launch
# (tests/test_hip_ppo_gemm.py), which leaves a factor of about three.
FP32_SHARE = 0.25

# kernel codes of the launch trace (GK_* of csrc/ppo_gemm.hip) under the short names TRACES uses
KERNELS = {"g32s": 1, "g32b": 2, "pl1s": 3, "pl1b": 4, "pl2s": 5, "pl2b": 6, "glds": 7, "dws": 8, "dwb": 9, "ref": 10}
KERNEL_NAMES = {"g32s": "k_gemm fp32-operand 64x64", "g32b": "k_gemm fp32-operand 128x128", "pl1s": "k_gemm planes-1 64x64",
                "pl1b": "k_gemm planes-1 128x128", "pl2s": "k_gemm planes-2 64x64", "pl2b": "k_gemm planes-2 128x128",
                "glds": "k_gemm_glds", "dws": "k_gemm_dw_t 64x64", "dwb": "k_gemm_dw_t 128x128", "ref": "k_gemm_ref"}
KINDS = "fxw"                                           # forward, input gradient (dX), weight gradient (dW): kinds 0, 1, 2

PRODUCT = (512, 256, 128)


def _case(hidden, R, O=48, OC=None, critic=None, activation="elu", A=12, nmb=1, mb=0, seed=SEED):
    return dict(hidden=tuple(hidden), critic=None if critic is None else tuple(critic), activation=activation, O=O, OC=OC, A=A, R=R,
                nmb=nmb, mb=mb, seed=seed)


def _cases():
    out = []
    # depth 1 .. 4 on the fused heads: net128 ([128], [64, 128], [.., 128, 128]) and fused32 ([.., 32]); the generic head (k_loss after
    # head GEMMs) at depth 3 below: unequal widths, widths 24 / 20, every activation but elu.  sched::backward walks
    # nl - 1 - skip_head .. 0, the fused head is handed b_off[nl - 2], forward takes nl from the first net
    for hidden in ((128,), (64, 128), (96, 64, 32), (128, 96, 64, 32)):
        out.append(_case(hidden, 193))
    out.append(_case((512, 256, 128, 128), 300))
    # the product net: a padded first layer with nstore on dW1 (48 -> 64, 235 -> 256); a second row tile of one row (65, 129), off
    # the 128- and 256-row grids (300, 1000); 6145 = 48 * 128 + 1: 49 x 4 = 196 >= 192 tiles of 128 x 128 for dX of the 512-wide
    # layer, 24 reduction slices x 8 tiles for its dW, the last row tile one row
    for O in (48, 235):
        for R in (65, 129, 300, 1000, 6145):
            out.append(_case(PRODUCT, R, O=O))
    # privileged critic; in the second shape the two problems of dW1 have different tile counts (64 x 96 against 64 x 192) and the
    # slice count is a multiple of 8: the shape of the tile-map bug of k_gemm_dw_t
    out.append(_case(PRODUCT, 300, O=65, OC=169))
    out.append(_case((64, 64, 32), 2049, O=65, OC=169))
    # unequal widths: every launch carries two problems of different shapes, the head is generic
    out.append(_case((256, 256, 128), 2049, critic=(128, 128, 64)))
    # widths off every 128 grid: no LDS-DMA forward.  40 and 24 are multiples of 8, all that planes_ok asks: still the weight planes
    # on every launch.  44 and 20 are not: fp32-operand k_gemm for the forward and the input gradients that chunk those widths
    out.append(_case((96, 40, 24), 300, O=169))
    out.append(_case((96, 44, 20), 300, O=169))
    # every activation
    for act in ("elu", "selu", "relu", "lrelu", "tanh", "sigmoid"):
        out.append(_case((256, 128, 64), 300, activation=act))
    for act in ("tanh", "relu"):
        out.append(_case(PRODUCT, 6145, activation=act))
    # the second minibatch of two, gathered ahead into the other buffer set by the optimiser step of the first
    out.append(_case(PRODUCT, 300, O=65, nmb=2, mb=1))
    return out


def case_id(c):
    s = "x".join(map(str, c["hidden"]))
    if c["critic"]:
        s += "-c" + "x".join(map(str, c["critic"]))
    s += f"-{c['activation']}-O{c['O']}"
    if c["OC"]:
        s += f"-OC{c['OC']}"
    s += f"-R{c['R']}"
    if c["nmb"] > 1:
        s += f"-mb{c['mb']}of{c['nmb']}"
    return s


CASES = _cases()
BY_ID = {case_id(c): c for c in CASES}
assert len(BY_ID) == len(CASES)
# deterministic mode (set_deterministic(True)): depth 4, the privileged R = 2049 case, the product net at R = 1000
DETERMINISTIC = ("128x96x64x32-elu-O48-R193", "64x64x32-elu-O65-OC169-R2049", "512x256x128-elu-O48-R1000")

# What lg_ppo_minibatch_backward launches per case, in launch order: kind:kernel[/slices] with kind f (forward), x (input gradient),
# w (weight gradient, with its reduction slices); every launch carries both nets (nz = 2).  The forward runs layer 0 .. (the head
# layer only when the head is generic); the backward alternates w, x from the top layer down and ends on the first layer's w.
_P3 = "f:glds f:glds f:glds"
TRACES = {
    "128-elu-O48-R193": "f:glds w:dws/1",
    "64x128-elu-O48-R193": "f:pl1s f:glds w:dws/1 x:pl2s w:dws/1",
    "96x64x32-elu-O48-R193": "f:pl1s f:pl1s f:pl1s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
    "128x96x64x32-elu-O48-R193": "f:glds f:pl1s f:pl1s f:pl1s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
    "512x256x128x128-elu-O48-R300": "f:glds f:glds f:glds f:glds w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
}
for _O in (48, 235):
    for _R, _s in ((65, 1), (129, 1), (300, 1), (1000, 3)):
        TRACES[f"512x256x128-elu-O{_O}-R{_R}"] = f"{_P3} w:dws/{_s} x:pl2s w:dws/{_s} x:pl2s w:dws/{_s}"
TRACES.update({
    "512x256x128-elu-O48-R6145": _P3 + " w:dws/24 x:pl2s w:dwb/24 x:pl2b w:dws/24",
    "512x256x128-elu-O235-R6145": _P3 + " w:dws/24 x:pl2s w:dwb/24 x:pl2b w:dwb/24",
    "512x256x128-elu-O65-OC169-R300": _P3 + " w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
    "64x64x32-elu-O65-OC169-R2049": "f:pl1s f:pl1s f:pl1s w:dws/8 x:pl2s w:dws/8 x:pl2s w:dws/8",
    "256x256x128-c128x128x64-elu-O48-R2049": "f:glds f:glds f:pl1s f:pl1s w:dws/8 x:pl2s w:dws/8 x:pl2s w:dws/8 x:pl2s w:dws/8",
    "96x40x24-elu-O169-R300": "f:pl1s f:pl1s f:pl1s f:pl1s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
    "96x44x20-elu-O169-R300": "f:pl1s f:pl1s f:g32s f:g32s w:dws/1 x:g32s w:dws/1 x:g32s w:dws/1 x:pl2s w:dws/1",
    "256x128x64-elu-O48-R300": "f:glds f:glds f:pl1s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
    "512x256x128-tanh-O48-R6145": _P3 + " f:pl1s w:dws/24 x:pl2s w:dws/24 x:pl2s w:dwb/24 x:pl2b w:dws/24",
    "512x256x128-relu-O48-R6145": _P3 + " f:pl1s w:dws/24 x:pl2s w:dws/24 x:pl2s w:dwb/24 x:pl2b w:dws/24",
    "512x256x128-elu-O65-R300-mb1of2": _P3 + " w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1",
})
for _a in ("selu", "relu", "lrelu", "tanh", "sigmoid"):
    TRACES[f"256x128x64-{_a}-O48-R300"] = "f:glds f:glds f:pl1s f:pl1s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1 x:pl2s w:dws/1"


def parse_trace(s):
    """TRACES notation -> [(kind, nz, kernel code, slices)], the rows ppok_debug_gemm_trace reports."""
    out = []
    for tok in s.split():
        kind, rest = tok.split(":")
        name, _, slices = rest.partition("/")
        out.append((KINDS.index(kind), 2, KERNELS[name], int(slices) if slices else 1))
    return out


def format_trace(rows):
    names = {v: k for k, v in KERNELS.items()}
    return " ".join(f"{KINDS[k]}:{names.get(kern, kern)}" + (f"/{sl}" if k == 2 else "") for k, nz, kern, sl in rows)


def paths_of(c):
    """The kernel paths of a case as (kernel name, slice class) pairs, for the table of paths reached."""
    out = set()
    for kind, nz, kern, sl in parse_trace(TRACES[case_id(c)]):
        name = {v: k for k, v in KERNELS.items()}[kern]
        out.add(KERNEL_NAMES[name] + ((" 1 slice" if sl == 1 else " 8+ slices" if sl >= 8 else " 2-7 slices") if name == "dws" else ""))
    return out


@functools.lru_cache(maxsize=None)
def _build_cached(cid):
    c = BY_ID[cid]
    return plr._build(c["O"], c["A"], c["hidden"], c["activation"], c["R"] * c["nmb"], c["seed"], c["critic"], plr.TABLE, OC=c["OC"])


def build_for(c):
    """The case of one CASES entry: R * num_mini_batches rows of storage (ppo_loss_ref.build_case, with critic observations of their
    own when OC is set).  Cached: callers must not write into the tensors."""
    return _build_cached(case_id(c))


def alg_for(c):
    """One minibatch: the configuration of tests/test_hip_ppo_loss.py.  Two: a fixed learning rate of 1e-6, so that the optimiser
    step between the two backward passes moves no parameter by more than 1e-6 (Adam's step is at most the learning rate) and the
    rows of the second minibatch stay on their side of every branch boundary; the reference is computed on the stepped parameters."""
    if c["nmb"] == 1:
        return dict(ALG)
    return dict(ALG, num_mini_batches=c["nmb"], schedule="fixed", learning_rate=1e-6)


def policy_for(c):
    return {"actor_hidden_dims": list(c["hidden"]), "critic_hidden_dims": list(c["critic"] or c["hidden"]), "activation": c["activation"],
            "init_noise_std": 1.0}


def reference(case, alg, rows=None, dtype=torch.float64, params=None):
    """ppo_loss_ref.reference (oracle.ppo_torch.PPO.minibatch_loss on a model of `dtype`); `params`: another parameter set than the
    case's own (the stepped parameters the second minibatch of two runs on)."""
    if params is not None:
        case = dict(case, params=params)
    return plr.reference(case, alg, rows, dtype)


@functools.lru_cache(maxsize=None)
def reference_cached(cid):
    """The float64 reference over all rows of a one-minibatch case (a few GFLOP at 6145 rows): once per session."""
    c = BY_ID[cid]
    assert c["nmb"] == 1
    return reference(build_for(c), alg_for(c))


def blocks(case):
    """EVERY parameter tensor: std, then weight and bias of every layer of both nets, in ActorCritic.parameters() order."""
    m = case["meta"]
    names = ["std"]
    for net, hid in (("actor", m["hidden"]), ("critic", m["critic_hidden"])):
        for l in range(len(hid) + 1):
            names += [f"{net}.{2 * l}.weight", f"{net}.{2 * l}.bias"]
    return names


def band_errors(got, ref, case):
    """Every band as name -> (error, bound): those of ppo_loss_ref.band_errors (element-wise rtol 2e-3 + atol 2e-4 max|ref| over the
    whole vector, relative norm of the whole vector, KL, the two loss means), and the relative-norm bound -- 2e-4, 3e-4 for an
    activation other than elu -- on each tensor of blocks() alone.  A tensor whose float64 gradient is exactly zero must come out
    exactly zero (ppo_loss_ref._rel)."""
    assert list(ref["grads"]) == blocks(case), "blocks() leaves out a tensor"
    out = plr.band_errors(got, ref, case)
    nb = out["grad.norm"][1]
    tensors = {"grad.norm." + k: (plr._rel(got["grads"][k].double(), ref["grads"][k]), nb) for k in blocks(case)}
    head = {k: v for k, v in out.items() if not k.startswith("grad.norm.")}
    return {**{k: head[k] for k in ("grad.elementwise", "grad.norm")}, **tensors, **{k: head[k] for k in ("kl", "value_loss", "surrogate_loss")}}


def accepted_by_hip_ppo(c):
    """The size rules of HipPPO / lg_ppo_create, restated: None, or what the case breaks."""
    from legged_gym_dev_amd import capi
    from legged_gym_dev_amd.rl import ppo as hip_ppo
    critic = c["critic"] or c["hidden"]
    if len(critic) != len(c["hidden"]) or not 1 <= len(c["hidden"]) <= capi.MAX_HIDDEN:
        return "depth"
    if not 1 <= c["A"] <= 16:
        return "num_actions"
    if c["activation"] not in hip_ppo._ACTIVATIONS:
        return "activation"
    if min(c["hidden"] + tuple(critic)) < 1 or c["O"] < 1 or (c["OC"] is not None and c["OC"] < 1):
        return "width"
    if c["R"] < 1 or c["nmb"] < 1 or not 0 <= c["mb"] < c["nmb"]:
        return "rows"
    return None
