"""The multi-rank native collective path over the stand-in transport (not a test module: started by
tests/test_hip_comm_standin.py, one fresh process per call, because the library resolves its RCCL once per process and the rest of
the suite binds the real one).

The process imports torch, points LG_RCCL_LIB at tests/comm_standin/_build/librccl_standin.so, runs the ranks of a communicator as
threads on cuda:0 -- each on a stream of its own -- and writes what the parent asserts on to an .npz.

    python tests/comm_standin_worker.py <mode> <out.npz> '<json arguments>'

modes: transport (lg_comm_* alone), errors (mismatch, capacity, a rank that never arrives), buckets (one minibatch's gradient
buckets), update (a whole update), runner (one iteration of the product runner).
"""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the libraries: they bind to the HIP runtime instance torch loaded)

STANDIN_DIR = os.path.join(ROOT, "tests", "comm_standin")
STANDIN_SO = os.path.join(STANDIN_DIR, "_build", "librccl_standin.so")
EXPORTS = ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllReduce", "ncclBroadcast", "ncclGroupStart", "ncclGroupEnd",
           "ncclGetErrorString")
N_PER_RANK, A, T = 64, 12, 8
TRANSPORT_COUNTS = (1, 4, 1000, (1 << 16) + 1)
GROUP_BUFFER, GROUP_EXTENTS = 70000, ((0, 1), (5, 4), (17, 1000), (1100, (1 << 16) + 1))    # (offset, count): gaps stay untouched
SCRATCH_FLOATS = 1 << 20
LEARNER_STREAMS = 4                                        # the attached pass of (b) runs on that many streams per rank, see mode_buckets


def build_standin(force=False):
    srcs = [os.path.join(STANDIN_DIR, f) for f in ("standin.hip", "Makefile")]
    if not force and os.path.isfile(STANDIN_SO) and all(os.path.getmtime(STANDIN_SO) >= os.path.getmtime(s) for s in srcs):
        return STANDIN_SO
    subprocess.check_call(["make", "-C", STANDIN_DIR, "-s"])
    return STANDIN_SO


def ramp(r, n):
    """What rank r holds before a collective: small integers, so every sum is exact."""
    return (np.arange(n, dtype=np.int64) % 251 * (r + 1) + r).astype(np.float32)


class _Ctl:
    """The stand-in's own controls (the same library instance comm_api.cpp opened: one file, one handle)."""

    def __init__(self):
        self.so = C.CDLL(STANDIN_SO)
        self.so.standin_call_log.restype = C.c_int64
        self.so.standin_call_log.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.c_int64, C.c_int]

    def delay(self, us):
        assert self.so.standin_set_delay_us(int(us)) == 0

    def timeout_ms(self, ms):
        assert self.so.standin_set_timeout_ms(int(ms)) == 0

    def log(self, uid, rank, reset=False):
        cap = 256
        buf = (C.c_int64 * (4 * cap))()
        n = self.so.standin_call_log(uid, rank, buf, cap, int(reset))
        assert 0 <= n <= cap, n
        return np.array(buf[: 4 * n], dtype=np.int64).reshape(n, 4)


def _new_uid(lib):
    buf = (C.c_char * 128)()
    lib.lg_comm_get_unique_id.argtypes = [C.c_void_p]
    assert lib.lg_comm_get_unique_id(buf) == 0, lib.lg_last_error().decode()
    return bytes(buf)


def _comms(W, uid=None):
    """One NativeComm per rank over the stand-in.  Its ncclCommInitRank only registers the rank, so they can be made one after the
    other on one thread."""
    from legged_gym_dev_amd.lib import load
    from legged_gym_dev_amd.rl.comm import NativeComm
    uid = uid or _new_uid(load())
    return uid, [NativeComm(r, W, unique_id=uid) for r in range(W)]


def run_ranks(W, fn, limit=120.0):
    """fn(r) on W threads, each under a torch stream of its own; returns their results.  A rank that raises leaves its peers to the
    stand-in's rendezvous limit, which returns them an error: nothing here waits forever."""
    outs, errs = [None] * W, [None] * W

    def body(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                outs[r] = fn(r)
            s.synchronize()
        except BaseException as e:          # noqa: BLE001
            errs[r] = e
    ths = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(W)]
    for t in ths:
        t.start()
    end = time.monotonic() + limit
    for t in ths:
        t.join(max(0.0, end - time.monotonic()))
    if any(t.is_alive() for t in ths):
        print("rank threads still running after", limit, "s", flush=True)
        os._exit(3)
    for e in errs:
        if e is not None:
            raise e
    return outs


def _stream_sync():
    torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------------ (a) the transport on its own
def mode_transport(W):
    from legged_gym_dev_amd.lib import load
    lib, ctl = load(), _Ctl()
    vp = C.c_void_p
    lib.lg_comm_group_allreduce_.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.c_int, vp]
    uid, comms = _comms(W)
    out = {}
    for delay in (0, 2000):
        ctl.delay(delay)

        def rank(r, delay=delay):
            comm, res = comms[r], {}
            dev = lambda a: torch.from_numpy(a).cuda()          # noqa: E731
            for n in TRANSPORT_COUNTS:
                x = dev(ramp(r, n))
                comm.all_reduce(x)
                res[f"allreduce_{n}"] = x.cpu().numpy()
                for root in (0, 1):
                    y = dev(ramp(r, n))
                    comm.broadcast(y, root)
                    res[f"broadcast{root}_{n}"] = y.cpu().numpy()
            z = dev(ramp(r, GROUP_BUFFER))
            bufs = (vp * 4)(*[z.data_ptr() + 4 * o for o, _ in GROUP_EXTENTS])
            cnts = (C.c_int64 * 4)(*[c for _, c in GROUP_EXTENTS])
            rc = lib.lg_comm_group_allreduce_(comm.ctx, bufs, cnts, 4, vp(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, lib.lg_last_error().decode()
            res["group"] = z.cpu().numpy()
            return res
        for r, res in enumerate(run_ranks(W, rank)):
            for k, v in res.items():
                out[f"d{delay}_r{r}_{k}"] = v
            out[f"d{delay}_r{r}_log"] = ctl.log(uid, r, reset=True)
    ctl.delay(0)
    for c in comms:
        c.close()
    return out


def mode_errors():
    from legged_gym_dev_amd.lib import LeggedHipError, load
    from legged_gym_dev_amd.rl.comm import NativeComm
    lib, ctl = load(), _Ctl()
    out = {}

    def failing(r, comm, n):
        x = torch.zeros(n, device="cuda") + (r + 1)
        t0 = time.monotonic()
        try:
            comm.all_reduce(x)
            msg = ""
        except LeggedHipError as e:
            msg = str(e)
        return msg, time.monotonic() - t0, x.cpu().numpy()

    uid, comms = _comms(2)
    # the ranks disagree on the count: an error on both, at once
    res = run_ranks(2, lambda r: failing(r, comms[r], 4 + r))
    out["mismatch_msg"] = np.array([m for m, _, _ in res])
    out["mismatch_s"] = np.array([s for _, s, _ in res])
    # ... and the communicator still carries the next, agreeing call
    res = run_ranks(2, lambda r: failing(r, comms[r], 4))
    out["after_mismatch_msg"] = np.array([m for m, _, _ in res])
    out["after_mismatch"] = np.stack([x for _, _, x in res])
    # one float above the scratch capacity
    res = run_ranks(2, lambda r: failing(r, comms[r], SCRATCH_FLOATS + 1))
    out["capacity_msg"] = np.array([m for m, _, _ in res])
    for c in comms:
        c.close()
    # rank counts outside 2 .. 8
    try:
        NativeComm(0, 1, unique_id=_new_uid(lib))
        out["one_rank_msg"] = np.array("")
    except LeggedHipError as e:
        out["one_rank_msg"] = np.array(str(e))
    # a rank that never arrives: the other one gets its answer after the time limit (shortened for this one check)
    ctl.timeout_ms(300)
    lone = NativeComm(0, 2, unique_id=_new_uid(lib))
    res = run_ranks(1, lambda r: failing(0, lone, 4))
    out["lone_msg"], out["lone_s"] = np.array(res[0][0]), np.array(res[0][1])
    res = run_ranks(1, lambda r: failing(0, lone, 4))              # the communicator stays broken, and says why at once
    out["lone_again_msg"], out["lone_again_s"] = np.array(res[0][0]), np.array(res[0][1])
    ctl.timeout_ms(30000)
    lone.close()
    return out


# ------------------------------------------------------------------ shards of one learner
def _shards(W, hidden, O, nmb, epochs, seed=5):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    from tests.test_hip_ppo import ALG, POLICY
    policy = dict(POLICY, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden))
    alg = dict(ALG, num_mini_batches=nmb, num_learning_epochs=epochs)
    torch.manual_seed(seed)
    sh = [HipPPO(N_PER_RANK, O, None, A, policy, alg, T, device="cuda:0", seed=seed, world_size=W, rank=r) for r in range(W)]
    sd = sh[0].state_dict()
    for s in sh[1:]:
        s.load_state_dict(sd)
    return sh


def _rollout_data(W, O, seed=8):
    """What the envs 'said' over the global W * 64 envs, as tests/test_hip_ppo.py::test_two_rank_update_equals_single_process_update
    draws it; rank r takes rows [64 r, 64 (r + 1))."""
    N = W * N_PER_RANK
    g = torch.Generator(device="cuda").manual_seed(seed)
    steps = []
    for _ in range(T):
        obs = torch.randn(N, O, device="cuda", generator=g)
        noise = torch.randn(N, A, device="cuda", generator=g)
        rew = torch.randn(N, device="cuda", generator=g)
        dones = (torch.rand(N, device="cuda", generator=g) < 0.1).to(torch.uint8)
        tos = ((torch.rand(N, device="cuda", generator=g) < 0.5) & (dones > 0)).to(torch.uint8)
        steps.append((obs, noise, rew, dones, tos))
    last = torch.randn(N, O, device="cuda", generator=g)
    torch.cuda.synchronize()
    return steps, last


def _fill(s, r, data):
    """rank r's rollout and lg_ppo_compute_returns (the advantage moments are left unreduced in adv_partial)."""
    steps, last = data
    sl = slice(r * N_PER_RANK, (r + 1) * N_PER_RANK)
    s.inject_noise(1)
    for obs, noise, rew, dones, tos in steps:
        s.t["noise"].copy_(noise[sl])
        s.act(obs[sl].contiguous())
        s.process_env_step(rew[sl].contiguous(), dones[sl].contiguous(), {"time_outs": tos[sl].contiguous()})
    keep = last[sl].contiguous()
    s._call("compute_returns", C.c_void_p(keep.data_ptr()))
    _stream_sync()


def _host_sum(sh, name, n=None):
    torch.cuda.synchronize()
    tot = sh[0].t[name][:n].clone()
    for s in sh[1:]:
        tot += s.t[name][:n]
    for s in sh:
        s.t[name][:n].copy_(tot)
    torch.cuda.synchronize()
    return tot


def _layout(hip):
    names = list(hip.param_views)
    base = hip.t["params"].data_ptr()
    return (np.array(names), np.array([(hip.param_views[k].data_ptr() - base) // 4 for k in names], np.int64),
            np.array([hip.param_views[k].numel() for k in names], np.int64))


def _extents(hip, nl):
    rows = []
    offs, cnts = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    for l in range(nl):
        n = hip.lib.lg_ppo_debug_bucket_extents(hip.ctx, l, offs, cnts)
        rows += [(l, k, offs[k], cnts[k]) for k in range(n)]
    return np.array(rows, np.int64)


# ------------------------------------------------------------------ (b) one minibatch's buckets
def mode_buckets(W, cases):
    ctl = _Ctl()
    out = {}
    learner_streams = [[torch.cuda.Stream() for _ in range(LEARNER_STREAMS)] for _ in range(W)]
    for hidden, O in cases:
        tag = "h" + "x".join(map(str, hidden)) + f"_o{O}"
        sh = _shards(W, hidden, O, nmb=2, epochs=1)
        data = _rollout_data(W, O)
        for r, s in enumerate(sh):
            _fill(s, r, data)
        _host_sum(sh, "adv_partial")
        # One step away from the rollout's parameters, the same on every rank, as from an update's second minibatch on: on the
        # rollout's own parameters mu_new = mu_old bit for bit, and the KL sum is the same rounding residue on every rank -- an
        # element that could be left out of the reduction unnoticed.
        P = sh[0].num_params
        step = 0.02 * torch.randn(P, device="cuda", generator=torch.Generator(device="cuda").manual_seed(13))
        for s in sh:
            s.t["params"][:P].add_(step)
            s.params_changed()
            s._call("normalize_advantages")
            s._call("begin_update")
        torch.cuda.synchronize()
        uid, comms = _comms(W)
        nr = sh[0].num_reduce
        out[f"{tag}_names"], out[f"{tag}_offsets"], out[f"{tag}_sizes"] = _layout(sh[0])
        out[f"{tag}_num_params"] = np.int64(sh[0].num_params)
        out[f"{tag}_extents"] = _extents(sh[0], len(hidden) + 1)
        for delay in (0, 2000):
            ctl.delay(delay)
            for r in range(W):
                ctl.log(uid, r, reset=True)

            def rank(r):
                hip, comm = sh[r], comms[r]
                grads, res = hip.t["grads"][:nr], []
                # The attached pass runs once on each of this rank's learner streams.  Streams share a few hardware queues, and on
                # a stream that happens to sit in the queue of the communicator's stream everything enqueued later -- the marker of
                # a stream synchronisation too -- comes behind the delayed copy-back, waited for or not; consecutive streams of
                # the pool sit in different queues, so at most one of the four can hide a missing wait.
                for ls in learner_streams[r]:
                    with torch.cuda.stream(ls):
                        hip.use_current_stream()
                        comm.attach(hip)
                        hip._call("minibatch_backward", 0, 0)
                        _stream_sync()                           # the learner's stream only: the reduced buckets are its business
                        res.append(grads.clone())
                        comm.lib.lg_ppo_set_comm(hip.ctx, None)
                        for _ in range(3 if ls is learner_streams[r][-1] else 0):   # own gradients; twice more for the run-to-run noise
                            hip._call("minibatch_backward", 0, 0)
                            _stream_sync()
                            res.append(grads.clone())
                        _stream_sync()
                return [torch.stack(res[:LEARNER_STREAMS]).cpu().numpy()] + [x.cpu().numpy() for x in res[LEARNER_STREAMS:]]
            res = run_ranks(W, rank)
            for k, name in enumerate(("G", "g", "n1", "n2")):
                out[f"{tag}_d{delay}_{name}"] = np.stack([res[r][k] for r in range(W)])
            for r in range(W):
                out[f"{tag}_d{delay}_log{r}"] = ctl.log(uid, r)
        ctl.delay(0)
        torch.cuda.synchronize()
        for c in comms:
            c.close()
        for s in sh:
            s.close()
    return out


# ------------------------------------------------------------------ (c) a whole update
def _perturb_rank0(sh):
    g = torch.Generator(device="cuda").manual_seed(21)
    P = sh[0].num_params
    sh[0].t["params"][:P].add_(0.01 * torch.randn(P, device="cuda", generator=g))
    sh[0].params_changed()
    torch.cuda.synchronize()
    return sh[0].t["params"].clone()


def mode_update(cases):
    ctl = _Ctl()
    W, O, out = 2, 48, {}
    for hidden in cases:
        tag = "h" + "x".join(map(str, hidden))
        data = _rollout_data(W, O)
        # the explicit host sum of test_two_rank_update_equals_single_process_update, ranks one after the other
        sh = _shards(W, hidden, O, nmb=2, epochs=2)
        p0 = _perturb_rank0(sh)
        out[f"{tag}_p0"] = p0.cpu().numpy()
        sh[1].t["params"].copy_(p0)
        sh[1].params_changed()
        for r, s in enumerate(sh):
            _fill(s, r, data)
        _host_sum(sh, "adv_partial")
        for s in sh:
            s._call("normalize_advantages")
            s._call("begin_update")
        for epoch in range(2):
            for mb in range(2):
                for s in sh:
                    s._call("minibatch_backward", epoch, mb)
                _host_sum(sh, "grads", sh[0].num_reduce)
                for s in sh:
                    s._call("minibatch_step")
        for s in sh:
            s._call("end_update")
        torch.cuda.synchronize()
        out[f"{tag}_host_params"] = np.stack([s.t["params"][: s.num_params].cpu().numpy() for s in sh])
        out[f"{tag}_host_lr"] = np.array([s.learning_rate for s in sh])
        for s in sh:
            s.close()
        # the same shards, every exchange through the library's own entries over the stand-in, ranks side by side
        for delay in (0, 2000):
            sh = _shards(W, hidden, O, nmb=2, epochs=2)
            p0b = _perturb_rank0(sh)
            assert torch.equal(p0b, p0)
            uid, comms = _comms(W)
            ctl.delay(delay)

            def rank(r):
                hip, comm, lib = sh[r], comms[r], comms[r].lib
                lib.lg_ppo_allreduce_adv_moments.argtypes = [C.c_void_p, C.c_void_p]
                lib.lg_ppo_broadcast_params.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
                hip.use_current_stream()
                assert lib.lg_ppo_broadcast_params(hip.ctx, comm.ctx, 0) == 0, lib.lg_last_error().decode()
                _stream_sync()
                res = {"bcast": hip.t["params"].cpu().numpy()}
                _fill(hip, r, data)
                res["partial"] = hip.t["adv_partial"].cpu().numpy()
                assert lib.lg_ppo_allreduce_adv_moments(hip.ctx, comm.ctx) == 0, lib.lg_last_error().decode()
                _stream_sync()
                res["partial_sum"] = hip.t["adv_partial"].cpu().numpy()
                hip._call("normalize_advantages")
                comm.attach(hip)
                hip.update()
                _stream_sync()
                res["params"] = hip.t["params"][: hip.num_params].cpu().numpy()
                res["lr"] = np.float64(hip.learning_rate)
                return res
            res = run_ranks(W, rank)
            for k in res[0]:
                out[f"{tag}_d{delay}_{k}"] = np.stack([res[r][k] for r in range(W)])
            ctl.delay(0)
            torch.cuda.synchronize()
            for c in comms:
                c.close()
            for s in sh:
                s.close()
    return out


# ------------------------------------------------------------------ (d) the runner
class _RunnerComm:
    """What the runner is handed.  While the runners are constructed -- one after the other on the main thread, for the reason
    tests/test_hip_multi_rank.py::_ThreadComm gives -- the initial broadcast is the direct copy and attach() is only noted; from
    go_native() on it is the product's NativeComm over the stand-in: attached, overlapped, all_reduce = lg_comm_allreduce_sum."""
    overlapped = True

    def __init__(self, rank, shared):
        self.rank, self.world_size, self.sh = rank, shared["world"], shared
        self.native = self._ppo = None

    def broadcast(self, t, src=0):
        assert self.native is None and src == 0
        if self.rank == 0:
            self.sh["src"] = t
        else:
            t.copy_(self.sh["src"])
        torch.cuda.synchronize()

    def attach(self, ppo):
        self._ppo = ppo

    def go_native(self, uid):
        from legged_gym_dev_amd.rl.comm import NativeComm
        self.native = NativeComm(self.rank, self.world_size, unique_id=uid)
        self.native.attach(self._ppo)

    def all_reduce(self, t):
        self.native.all_reduce(t)


def mode_runner(task):
    from legged_gym_dev_amd.lib import load
    from tests import multi_rank_worker as w
    from tests.test_hip_multi_rank import _emulate
    keys = ("params_it1", "friction", "base_mass_delta", "env_origins")
    out = {}
    emu = _emulate(task, N_PER_RANK, 1)
    for k in keys:
        out["emu_" + k] = np.stack([e[k] for e in emu])
    W = 2
    shared = {"world": W}
    comms = [_RunnerComm(r, shared) for r in range(W)]
    built = [w.build(task, N_PER_RANK, r, W, comm=comms[r]) for r in range(W)]
    uid = _new_uid(load())
    for c in comms:
        c.go_native(uid)
    assert all(b[1].comm is comms[r] and b[1]._grad_reduce is None for r, b in enumerate(built))
    errs, firsts = [], [None] * W

    def learn(r):                                               # as _emulate runs its ranks: the runner's own (default) stream
        try:
            torch.cuda.set_device(0)
            firsts[r] = w.learn_with_first_snapshot(built[r][1], 1)
        except BaseException as e:          # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=learn, args=(r,), daemon=True) for r in range(W)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(200)
    if any(t.is_alive() for t in ths):
        print("runner threads still running", flush=True)
        os._exit(3)
    if errs:
        raise errs[0]
    snaps = [dict(w.snapshot(*built[r]), params_it1=firsts[r]) for r in range(W)]
    for k in keys:
        out["standin_" + k] = np.stack([s[k] for s in snaps])
    out["log0"] = _Ctl().log(uid, 0)
    torch.cuda.synchronize()
    for c in comms:
        c.native.close()
    for env, runner in built:
        env.close()
        runner.ppo.close()
    return out


MODES = {"transport": mode_transport, "errors": mode_errors, "buckets": mode_buckets, "update": mode_update, "runner": mode_runner}


def main():
    mode, out, args = sys.argv[1], sys.argv[2], json.loads(sys.argv[3]) if len(sys.argv) > 3 else {}
    os.environ["LG_RCCL_LIB"] = build_standin()
    torch.cuda.set_device(0)
    res = MODES[mode](**args)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
