#!/usr/bin/env python3
"""Timing of the batched k-th selection (k_select_pass in csrc/select_kernels.hip, tube/calibrate.py select_kth) against torch.kthvalue and against
torch.sort + gather on the device, on resident data, and of calibrate_tube.py --sim end to end on the default model.

Shapes (B, n), R ranks per row:
    (1, 1 638 400)  R = 1     one column of one 8192 x 200 epoch
    (64, 1 638 400) R = 1     a level-conditioned model scored at 64 levels
    (50, 389 120)   R = 2     the one-shot shape of DESIGN.md section 10.1: 50 steps ahead, two coverages
    (2, 12 800)     R = 1     a test-sized set

Median of 3 after a warm-up run, every timing closed by a device synchronise.  The selection reads the values four times (once per
8-bit digit); "of HBM" is 4 B n 4 bytes / time as a fraction of the 6.29 TB/s a float4 copy reaches on this part.  A set that fits
the 256 MB last-level cache can exceed what HBM alone would give: the column is a rate, not a claim about where the bytes came from.

    python tools/bench_tube_calibrate.py > profiles/tube_calibrate_bench.txt
"""
import argparse
import contextlib
import io
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
import torch  # noqa: E402

from legged_gym_dev_amd.tube.calibrate import conformal_rank, select_kth  # noqa: E402

HBM_RATE = 6.29e12
SHAPES = [(1, 1638400, 1), (64, 1638400, 1), (50, 389120, 2), (2, 12800, 1)]


def timed(fn, reps=3):
    fn()                                               # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), out


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip_end_to_end", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    print(f"batched k-th selection, {torch.cuda.get_device_name(0)}; median of 3 after a warm-up run, each timing closed by a device synchronise")
    print(f"{'shape':>18s} {'R':>2s} {'HIP ms':>9s} {'kthvalue ms':>12s} {'ratio':>6s} {'sort ms':>9s} {'ratio':>6s} {'4 reads':>10s} {'of HBM':>7s}   runs (HIP ms)")
    ms = lambda r: " ".join(f"{x * 1e3:.3f}" for x in r)
    for B, n, R in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + n)
        v = torch.randn(B, n, device=dev, generator=g).abs_()          # scores of a tube: same sign, a few binades
        ranks = [conformal_rank(n, c) for c in ((0.9, 0.95) if R == 2 else (0.9,))]
        rk = torch.tensor(ranks, device=dev).expand(B, R).contiguous()
        idx = (rk - 1)

        def hip():
            return select_kth(v, rk)[0]

        def kth():
            return torch.stack([torch.kthvalue(v, k, dim=1).values for k in ranks], dim=1)

        def srt():
            return torch.sort(v, dim=1).values.gather(1, idx)

        want = srt()
        assert torch.equal(hip(), want) and torch.equal(kth(), want)
        del want
        th, rh = timed(hip)
        tk, _ = timed(kth)
        ts, _ = timed(srt)
        rate = 4 * B * n * 4 / th
        print(f"{f'({B}, {n})':>18s} {R:2d} {th * 1e3:9.3f} {tk * 1e3:12.3f} {tk / th:6.2f} {ts * 1e3:9.3f} {ts / th:6.2f} {rate / 1e12:7.2f} TB/s "
              f"{rate / HBM_RATE:7.2f}   [{ms(rh)}]")
        del v
        torch.cuda.empty_cache()
    if not a.skip_end_to_end:
        import calibrate_tube
        import train_tube
        tmp = tempfile.mkdtemp()
        try:
            run = os.path.join(tmp, "run")
            quiet(train_tube.main, ["--sim", "--sim_refresh", "0", "--num_epochs", "1", "--seed", "3", "--device", dev, "--out", run])
            te, re_ = timed(lambda: quiet(calibrate_tube.main, ["--run", run, "--sim", "--checkpoint", "latest", "--device", dev]))
            c = quiet(calibrate_tube.main, ["--run", run, "--sim", "--checkpoint", "latest", "--device", dev])
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print(f"\ncalibrate_tube.py --sim end to end on the default model (load, simulate 8192 x 200 fresh robots, build the rows, predict, roll "
              f"out, select, write calibration.json): {te * 1e3:.1f} ms   [{ms(re_)}]; n = {c.n}, ranks {c.ranks}")
    sys.stdout.flush()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_select"], capture_output=True, text=True).stdout
    print("\n" + res)


if __name__ == "__main__":
    main()
