"""ms / step of the BASELINE configs[1] network (5 x BLSTM-512, T_max 2000,
N 16, 40-dim features, 41 targets) with and without
steps/ctc/train.sh --dropout-proportion 0.2, i.e. a DropoutComponent between
every RNN and its ClipGradient.  bench.py is not involved.

Both networks live in one process and are timed in alternating blocks (the
host is shared: only a difference seen in every pair of blocks counts).  Each
block is `--steps` pipelined train steps on minibatches resident in HBM,
after a warm-up, between device synchronisations.  Then one profiled pass per
network prints the kctc_nnet_profile families (ms per step), which split the
difference into the dropout kernels and the lost forward chain
(fwd_proj_stream / x3_pack_chain gone, gemm_fwd_proj / x3_pack on the main
stream instead).

  python scripts/dropout_step_time.py [--steps 20] [--blocks 3] [--proportion 0.2]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FAMILIES = ["layer_rnn_forward", "rnn_fwd_rec", "gemm_fwd_proj", "x3_pack", "fwd_proj_stream", "fwd_proj_rows",
            "x3_pack_chain", "x3_pack_w_fwd", "dropout", "layer_ctc", "argmax", "scale", "clip_gradient",
            "layer_rnn_backward_data", "rnn_bwd_rec", "gemm_bwd_data", "bwd_data_stream", "x3_pack_bwd_stream",
            "layer_rnn_backward_weights", "x3_pack_w", "gemm_bwd_w", "gemm_bwd_r", "affine", "update"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--proportion", type=float, default=0.2)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--layers", type=int, default=5)
    args = ap.parse_args()
    import torch
    from conftest import load_kctc
    k = load_kctc()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    T, N, D, A = args.T, args.N, 40, 41
    kw = dict(num_rnn=args.layers, input_dim=D, hidden=args.hidden, num_targets=A, rnn_mode=2, learning_rate=5e-4)
    nets = {"plain": k.Nnet(k.recipe_config(**kw), seed=1),
            "dropout": k.Nnet(k.recipe_config(dropout_proportion=args.proportion, **kw), seed=1)}
    batches = []
    for step in range(4):
        feats, nf, fl, ll = k.synth_minibatch(20161015 + step, T, N, D, A, 0.125)
        batches.append((torch.from_numpy(feats).to(dev), nf, fl, ll))
    torch.cuda.synchronize()

    def block(net, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            f, nf, fl, ll = batches[i % len(batches)]
            net.train_step_async(f, T, N, nf, fl, ll)
        net.train_flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for net in nets.values():
        block(net, args.warmup)
    ms = {name: [] for name in nets}
    for b in range(args.blocks):
        for name, net in nets.items():
            ms[name].append(block(net, args.steps))
        print(f"block {b}: " + ", ".join(f"{name} {ms[name][-1]:.2f} ms/step" for name in nets), flush=True)
    for name in nets:
        print(f"{name}: median {np.median(ms[name]):.2f} ms/step over {args.blocks} blocks of {args.steps} steps "
              f"(min {min(ms[name]):.2f}, max {max(ms[name]):.2f})")
    print(f"difference of the medians: {np.median(ms['dropout']) - np.median(ms['plain']):.2f} ms/step")
    prof = {}
    for name, net in nets.items():
        net.set_profiling(True)
        block(net, args.steps)
        prof[name] = {f: net.profile(f) for f in FAMILIES}
        net.set_profiling(False)
    print("family: ms/step (launches/step) plain | dropout")
    for f in FAMILIES:
        (a, na), (b, nb) = prof["plain"][f], prof["dropout"][f]
        if na or nb:
            print(f"  {f}: {a / args.steps:.3f} ({na / args.steps:.1f}) | {b / args.steps:.3f} ({nb / args.steps:.1f})")
    for net in nets.values():
        net.close()


if __name__ == "__main__":
    main()
