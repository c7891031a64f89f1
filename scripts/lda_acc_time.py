"""Cost of LdaStats.accumulate (kctc_lda_accumulate, csrc/lda_stats.hip) at one
configs[1]-sized batch: R = 32 000 rows, C = 41 classes, D = 360 (get_lda.sh's
default splice of +-4 over 40-dim features) and D = 40 (no splice).  bench.py
is not involved.

Device time between two events (torch.cuda.Event: hipEvent) around `--calls`
stream-ordered calls, after a warm-up, in `--blocks` blocks.  Two reference
points: the same update (second moment, class sums, counts) in numpy fp64 on
the CPUs the job may use, and the achieved FLOP/s.  FLOPs counted: the useful
ones, 2 R (D (D + 1) / 2 + D) -- the lower triangle of the second moment and
one class sum per row; the kernel itself issues more (whole 64 x 64 diagonal
tiles, dense one-hot tiles).

  python scripts/lda_acc_time.py [--calls 20] [--blocks 3] [--out profiles/lda_acc_time.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--R", type=int, default=32000)
    ap.add_argument("--C", type=int, default=41)
    ap.add_argument("--dims", type=int, nargs="+", default=[360, 40])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from conftest import load_kctc
    k = load_kctc()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    R, C = args.R, args.C
    say(f"LdaStats.accumulate: R = {R}, C = {C}, {args.blocks} blocks of {args.calls} calls after {args.warmup} "
        f"warm-up calls; device time between hipEvents; {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(1)
    for D in args.dims:
        x = rng.standard_normal((R, D)).astype(np.float32)
        ids = rng.integers(0, C, R).astype(np.int32)
        xd, idd = torch.from_numpy(x).to(dev), torch.from_numpy(ids).to(dev)
        h = k.LdaStats(D, C)
        for _ in range(args.warmup):
            h.accumulate(xd, idd)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                h.accumulate(xd, idd)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.calls)
        flop = 2.0 * R * (D * (D + 1) / 2 + D)
        med = float(np.median(ms))
        # the same update in numpy fp64
        x64 = x.astype(np.float64)
        t_np = []
        for _ in range(3):
            t0 = time.perf_counter()
            second = x64.T @ x64
            first = np.zeros((C, D))
            np.add.at(first, ids, x64)
            zero = np.bincount(ids, minlength=C).astype(np.float64)
            t_np.append((time.perf_counter() - t0) * 1e3)
        n = args.warmup + args.blocks * args.calls
        z, f, s = h.stats()
        err = max(np.abs(s / n - second).max() / np.abs(second).max(), np.abs(f / n - first).max() / np.abs(first).max())
        assert np.array_equal(z, n * zero) and err < 1e-12, err
        say(f"D = {D}: blocks {', '.join(f'{m:.3f}' for m in ms)} ms/call, median {med:.3f} ms "
            f"= {flop / med / 1e9:.2f} useful TFLOP/s fp64 ({flop / 1e9:.2f} GFLOP per call); "
            f"numpy fp64 on {os.environ.get('OMP_NUM_THREADS', '?')} CPUs: {min(t_np):.1f} ms (best of 3), "
            f"{min(t_np) / med:.0f}x the device time")
        h.close()
    say("fraction of the fp64-MFMA peak: the micro-architecture notes this project works from state no fp64 matrix "
        "rate, so only FLOP/s are reported")
    if args.out:
        with open(args.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
