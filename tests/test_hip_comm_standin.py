"""GPU: the multi-rank NATIVE collective path (lg_comm_*, lg_ppo_set_comm, lg_ppo_allreduce_adv_moments, lg_ppo_broadcast_params)
with 2 to 4 ranks over a stand-in transport.

The pool gives a session one GPU, where RCCL runs one rank and every collective is the identity.  comm_api.cpp resolves its eight
RCCL entry points by dlopen; LG_RCCL_LIB puts tests/comm_standin/standin.hip under them: ranks are threads of one process on
cuda:0, a collective is events, stream waits, one summing kernel and asynchronous copies on the stream the caller hands in, and
nothing in it synchronises a stream or the device.  The product's own stream order (ppo_sched.hip: reduce_layer_bucket's wait for the
weight-gradient GEMM, the fused head's bucket from the main stream, the learner stream's wait for the last bucket) and its bucket
extents then decide the numbers.  A delay kernel in front of every copy-back (2000 us) makes a learner stream that does not wait
read unreduced gradients for certain rather than by luck -- as far as the hardware queues allow: streams share them, and what a
stream enqueues behind a delayed copy-back in its own queue comes after it, waited for or not.  So the children run on 32 queues,
and (b) repeats the attached pass on four learner streams per rank (tests/comm_standin_worker.py::mode_buckets).  Every case runs
in a fresh child (the library caches its RCCL handle per process); one child at a time.

(a) the transport alone, exact on small integers, with its error paths (count mismatch, capacity, a rank that never arrives);
(b) one minibatch's buckets on every head path: all ranks hold the same bits, equal to the float64 sum of the ranks' own gradients
    within the project's gradient bands, and the transport saw one group per layer with lg_ppo_debug_bucket_extents' counts;
(c) a whole update (2 epochs x 2 minibatches, broadcast and advantage moments through the library's entries) against the explicit
    host sum of tests/test_hip_ppo.py::test_two_rank_update_equals_single_process_update;
(d) one iteration of the product runner, two rank threads, against tests/test_hip_multi_rank.py::_emulate.

Run-to-run noise of the float-atomic gradient sums in (b): two unattached repeats of the same minibatch, summed over the ranks in
float64, compared under the same bands.  Each case prints it and asserts that it is at least 10x below every band.  Largest values
measured on an MI355X over the 12 cases x 2 delays, as the fraction of the band used: 8.1e-4 over everything (the relative norm of
the critic's last-hidden bias block, 1.6e-7 of 2e-4, W = 4, [96, 40]); element-wise 1.1e-4, whole vector 2.7e-4, std 6.0e-4, KL
sum 3.3e-4; the first-layer weight blocks repeat bit for bit.  The comparison itself used at most 1.1e-3 of a band.
"""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from tests import comm_standin_worker as csw
from tests import ppo_loss_ref as plr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NETS = ([96, 40], [64, 32], [64, 64], [32, 128])             # per-layer head, fused 32, fused 64, k_head_net + finish
BUCKET_CASES = {2: [(h, 48) for h in NETS] + [(h, 65) for h in NETS], 4: [(h, 48) for h in NETS]}
NORM_BAND = 2e-4


def _child(mode, **args):
    """One fresh worker process; returns what it wrote."""
    csw.build_standin()
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.npz")
        try:
            # 32 hardware queues for the child: with the runtime's default of 4, four ranks' delayed copy-backs occupy every queue, and
            # whatever a learner stream enqueues next -- waited for or not -- comes behind one of them (measured: without the learner
            # stream's wait, every W = 4 case still passed on 4 queues)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "comm_standin_worker.py"), mode, out, json.dumps(args)],
                               capture_output=True, text=True, timeout=300, env=dict(os.environ, GPU_MAX_HW_QUEUES="32"))
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"worker {mode} {args} was killed at its time limit; nothing more is started on the GPU:\n{(e.stdout or '')[-2000:]}", 3)
        if p.returncode < 0 or p.returncode in (134, 139):       # abort or fault: the session ends here
            pytest.exit(f"worker {mode} {args} died with {p.returncode}; nothing more is started on the GPU:\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", 3)
        assert p.returncode == 0, f"worker {mode} {args} exited with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}"
        return dict(np.load(out))


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("W", [2, 3])
def test_transport_is_exact(W):
    r = _child("transport", W=W)
    ramps = {n: [csw.ramp(k, n) for k in range(W)] for n in csw.TRANSPORT_COUNTS + (csw.GROUP_BUFFER,)}
    for delay in (0, 2000):
        for k in range(W):
            pre = f"d{delay}_r{k}_"
            for n in csw.TRANSPORT_COUNTS:
                np.testing.assert_array_equal(r[pre + f"allreduce_{n}"], sum(ramps[n]), err_msg=pre + str(n))
                for root in (0, 1):
                    np.testing.assert_array_equal(r[pre + f"broadcast{root}_{n}"], ramps[n][root], err_msg=pre + f"root {root} {n}")
            want = ramps[csw.GROUP_BUFFER][k].copy()              # outside the four extents the buffer keeps this rank's values
            for o, c in csw.GROUP_EXTENTS:
                want[o:o + c] = sum(x[o:o + c] for x in ramps[csw.GROUP_BUFFER])
            np.testing.assert_array_equal(r[pre + "group"], want, err_msg=pre + "group")
            log = r[pre + "log"]
            lone = [(op, n, 0) for n in csw.TRANSPORT_COUNTS for op in (1, 2, 2)]
            assert [tuple(x[:3]) for x in log] == lone + [(1, c, 1) for _, c in csw.GROUP_EXTENTS]
            assert len(set(log[-4:, 3])) == 1 and len(set(log[:, 3])) == len(lone) + 1      # the four extents were one group


def test_transport_errors_do_not_hang():
    r = _child("errors")
    for k in range(2):                                           # a count mismatch: an error on both ranks that names both sides, at once
        m = str(r["mismatch_msg"][k])
        assert "disagree" in m and "rank 0 issued" in m and "count=4" in m and "rank 1 issued" in m and "count=5" in m, m
        assert float(r["mismatch_s"][k]) < 5.0
        assert str(r["after_mismatch_msg"][k]) == ""
        np.testing.assert_array_equal(r["after_mismatch"][k], np.full(4, 3.0, np.float32))
        assert "capacity" in str(r["capacity_msg"][k]), r["capacity_msg"][k]
    assert "2 to 8 ranks" in str(r["one_rank_msg"])
    m = str(r["lone_msg"])                                       # a rank that never arrives: which rank, which call, after the limit
    assert "rank 1 did not arrive at ncclAllReduce(count=4) within 300 ms" in m, m
    assert 0.25 < float(r["lone_s"]) < 5.0
    assert "rank 1 did not arrive" in str(r["lone_again_msg"]) and float(r["lone_again_s"]) < 0.25


# ------------------------------------------------------------------ (b)
@functools.lru_cache(maxsize=None)
def _buckets(W):
    return _child("buckets", W=W, cases=BUCKET_CASES[W])


def _bands(got, ref, tag, r):
    """name -> (error, bound) of a flat [gradients | KL sum | pad] vector against a float64 one: the gradient bands of
    tests/test_hip_ppo.py through ppo_loss_ref.band_errors (element-wise rtol 2e-3 + atol 2e-4 max|ref| as the fraction of the band
    used, relative norm 2e-4 on the whole vector and on each of ppo_loss_ref.blocks(), std among them), and the relative-norm band on
    the KL sum."""
    P = int(r[tag + "_num_params"])
    hidden = [int(x) for x in tag.split("_")[0][1:].split("x")]
    case = {"meta": {"hidden": hidden, "critic_hidden": hidden, "activation": "elu"}}
    views = lambda v: {str(n): torch.from_numpy(v[o:o + s].copy()) for n, o, s in zip(r[tag + "_names"], r[tag + "_offsets"], r[tag + "_sizes"])}  # noqa: E731
    assert sum(int(s) for s in r[tag + "_sizes"]) == P
    pack = lambda v: {"grads": views(v), "kl": 0.0, "value_loss": 0.0, "surrogate_loss": 0.0}                          # noqa: E731
    errs = {k: v for k, v in plr.band_errors(pack(got), pack(ref.astype(np.float64)), case).items() if k.startswith("grad")}
    errs["kl_sum"] = (abs(float(got[P]) - float(ref[P])) / abs(float(ref[P])), NORM_BAND)
    return errs


@pytest.mark.parametrize("delay", [0, 2000])
@pytest.mark.parametrize("W,hidden,O", [(W, h, O) for W in (2, 4) for h, O in BUCKET_CASES[W]],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_minibatch_buckets_reduce_over_ranks(W, hidden, O, delay):
    r = _buckets(W)
    tag = "h" + "x".join(map(str, hidden)) + f"_o{O}"
    pre = f"{tag}_d{delay}_"
    G, g, n1, n2 = (r[pre + k] for k in ("G", "g", "n1", "n2"))
    ext = r[tag + "_extents"]                                     # rows (layer, k, offset, count)
    P, nr, nl = int(r[tag + "_num_params"]), G.shape[2], len(hidden) + 1          # G: (rank, learner stream, element)
    assert G.shape[:2] == (W, csw.LEARNER_STREAMS)
    assert nr == P + 2 and np.isfinite(G).all() and np.isfinite(g).all()
    # conditions: the ranks' own gradients differ where it matters, so an element left out of the reduction differs between ranks
    for a in range(W - 1):
        for l, k, o, c in ext:
            last = o + c - 1 if o + c - 1 != P + 1 else P         # grads[P + 1] is the pad behind the KL sum: zero on every rank
            assert g[a][o] != g[a + 1][o] and g[a][last] != g[a + 1][last], (a, l, k)
        assert (g[a] == g[a + 1]).mean() < 0.01
    assert np.all(g[:, P + 1] == 0)
    # ... and two unattached repeats differ by the float-atomic noise alone, at least 10x below every band
    noise = _bands(n1.astype(np.float64).sum(0), n2.astype(np.float64).sum(0), tag, r)
    print("standin_bucket_noise", W, tag, delay, {k: "%.3g/%.3g" % v for k, v in noise.items()},
          "worst fraction %.3g" % max(e / b for e, b in noise.values()))
    assert all(e <= 0.1 * b for e, b in noise.values()), noise
    # on every learner stream the attached pass ran on: every rank holds the same bits once that stream is done ...
    ref = g.astype(np.float64).sum(0)
    worst = {}
    for j in range(csw.LEARNER_STREAMS):
        for a in range(1, W):
            np.testing.assert_array_equal(G[a][j], G[0][j], err_msg=f"rank {a}, learner stream {j}")
        # ... which are the sum of the ranks' own gradients
        errs = _bands(G[0][j], ref, tag, r)
        over = {k: v for k, v in errs.items() if not v[0] <= v[1]}
        assert not over, (j, over)
        worst = {k: max(v, worst.get(k, v)) for k, v in errs.items()}
    print("standin_bucket_errors", W, tag, delay, {k: "%.3g/%.3g" % v for k, v in worst.items()},
          "worst fraction %.3g" % max(e / b for e, b in worst.values()))
    # the transport saw one group per layer, head first, with the extents the library reports
    want = [(1, int(c), 1, j * nl + nl - 1 - int(l)) for j in range(csw.LEARNER_STREAMS) for l in range(nl - 1, -1, -1)
            for ll, k, o, c in ext if ll == l]
    for a in range(W):
        assert [tuple(int(v) for v in x) for x in r[pre + f"log{a}"]] == want, (a, r[pre + f"log{a}"], want)


# ------------------------------------------------------------------ (c)
@functools.lru_cache(maxsize=None)
def _update():
    return _child("update", cases=[[64, 32], [32, 128]])


@pytest.mark.parametrize("delay", [0, 2000])
@pytest.mark.parametrize("hidden", [[64, 32], [32, 128]], ids=lambda h: "x".join(map(str, h)))
def test_update_over_standin_equals_explicit_host_sum(hidden, delay):
    r = _update()
    tag = "h" + "x".join(map(str, hidden))
    pre = f"{tag}_d{delay}_"
    p0 = r[tag + "_p0"]
    assert not np.array_equal(r[tag + "_host_params"][0], p0[: r[tag + "_host_params"].shape[1]])
    for k in range(2):                                           # lg_ppo_broadcast_params: rank 0's (different) parameters, exactly
        np.testing.assert_array_equal(r[pre + "bcast"][k], p0, err_msg=f"rank {k}")
    part = r[pre + "partial"]                                    # lg_ppo_allreduce_adv_moments: the fp32 sum in rank order, exactly
    assert not np.array_equal(part[0], part[1])
    for k in range(2):
        np.testing.assert_array_equal(r[pre + "partial_sum"][k], part[0] + part[1], err_msg=f"rank {k}")
    params = r[pre + "params"]
    np.testing.assert_array_equal(params[1], params[0])          # the ranks stay in lock-step exactly
    np.testing.assert_array_equal(r[tag + "_host_params"][1], r[tag + "_host_params"][0])
    ref = r[tag + "_host_params"][0]
    d = np.abs(params[0].astype(np.float64) - ref)
    print("standin_update", tag, delay, "worst fraction of rtol 2e-4 / atol 2e-6 used: %.3g" % float((d / (2e-6 + 2e-4 * np.abs(ref))).max()))
    np.testing.assert_allclose(params[0], ref, rtol=2e-4, atol=2e-6)
    assert np.all(np.abs(r[pre + "lr"] - r[tag + "_host_lr"]) < 1e-12) and r[pre + "lr"][0] == r[pre + "lr"][1]


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("task", ["anymal_c_flat", "anymal_c_rough"])
def test_runner_over_standin_equals_thread_emulation(task):
    r = _child("runner", task=task)
    a = r["standin_params_it1"]
    np.testing.assert_array_equal(a[1], a[0])
    assert np.isfinite(a).all()
    for key in ("friction", "base_mass_delta", "env_origins"):    # the shards themselves are reproduced exactly
        np.testing.assert_array_equal(r["standin_" + key], r["emu_" + key], err_msg=key)
    assert not np.array_equal(r["standin_friction"][0], r["standin_friction"][1])
    rel = np.linalg.norm(r["emu_params_it1"][0] - a[0]) / np.linalg.norm(a[0])
    print("standin_runner", task, "relative norm of the parameter difference after one iteration: %.3g" % rel)
    assert rel < 1e-5, rel
    log = r["log0"]                                              # 1 advantage-moment reduce, then 20 minibatches x 3 layer groups
    assert tuple(log[0][:3]) == (1, 4, 0) and len(set(log[1:, 3])) == 60 and np.all(log[1:, 2] == 1)
