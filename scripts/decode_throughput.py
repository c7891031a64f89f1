"""Decode-side throughput: frames / s of CtcDecodableAmNnet over a test set, one
utterance at a time (Nnet.decodable, what the reference's mini_batch = 1
evaluation does) against variable-length batches (Nnet.decodable_batch).

The model is BASELINE configs[1]'s topology (5 x BLSTM-512, 40-dim features,
41 targets) plus the SoftmaxComponent the recipe appends for decoding; the
test set 64 seeded utterances of 1800..2000 frames, resident in HBM.  Every
mode is warmed up with one whole pass of the set (every batch shape of the
timed window, so that no buffer grows inside it) and then timed over whole
passes of the set until `--seconds` have gone by, between device
synchronisations (each call of either entry point also returns its rows to
the host, so the figure is what a decoder's feature loop would see).

  python scripts/decode_throughput.py [--seconds 4] [--repeats 3] [--batches 8,16,32]
  python scripts/decode_throughput.py --loop-only      # Nnet.decodable only: runs on older trees too

Prints one line per (mode, repeat) and a JSON summary line; with batches, then
one profiled pass at batch 16 and the kctc_nnet_profile families of the
length-aware path next to the recurrences'."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FAMILIES = ["layer_rnn_forward", "rnn_fwd_rec", "gemm_fwd_proj", "x3_pack", "seq_align", "seq_unalign",
            "seq_decodable", "affine"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="8,16,32")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--blank-threshold", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from conftest import load_kctc
    k = load_kctc()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    D, A = 40, 41
    cfg = k.recipe_config(num_rnn=args.layers, input_dim=D, hidden=args.hidden, num_targets=A, rnn_mode=2)
    net = k.Nnet(cfg + f"SoftmaxComponent dim={A}\n", seed=1)
    rng = np.random.default_rng(20161015)
    lens = rng.integers(1800, 2001, args.utts)
    utts = [torch.from_numpy(rng.standard_normal((int(L), D)).astype(np.float32)).to(dev) for L in lens]
    frames = int(lens.sum())
    thr = args.blank_threshold

    def one_pass(batch):
        if batch == 0:
            for f in utts:
                net.decodable(f, f.shape[0], 1.0, thr)
        else:
            net.decodable_batch(utts, 1.0, thr, batch_size=batch)

    def window(batch):
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        while True:
            one_pass(batch)
            done += frames
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= args.seconds:
                return done / dt

    modes = [0] if args.loop_only else [0] + [int(b) for b in args.batches.split(",") if b]
    name = lambda b: "loop" if b == 0 else f"batch{b}"
    for b in modes:
        one_pass(b)
    fps = {name(b): [] for b in modes}
    for r in range(args.repeats):  # alternating: the host and the device are shared
        for b in modes:
            fps[name(b)].append(window(b))
            print(f"repeat {r} {name(b)}: {fps[name(b)][-1]:.0f} frames/s", flush=True)
    out = {"utts": args.utts, "frames": frames, "seconds": args.seconds,
           "frames_per_s": {m: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
                            for m, v in fps.items()}}
    if not args.loop_only and 16 in modes:
        net.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one_pass(16)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        out["profile_batch16_ms"] = {"wall": wall, **{f: net.profile(f)[0] for f in FAMILIES}}
        net.set_profiling(False)
    print(json.dumps(out), flush=True)
    net.close()


if __name__ == "__main__":
    main()
