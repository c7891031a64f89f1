"""ms / step of the BASELINE configs[1] network (5 x BLSTM-512, T_max 2000,
N 16, 40-dim features, 41 targets) with and without the front end of
steps/ctc/train.sh --model-type FT: AffineComponent 40 -> hidden_dim,
RectifiedLinearComponent, ClipGradientComponent in front of the first RNN,
which then is a hidden_dim-input layer with an input derivative.  bench.py is
not involved.

Both networks live in one process and are timed in alternating blocks (the
host is shared: only a difference seen in every pair of blocks counts).  Each
block is `--steps` pipelined train steps on minibatches resident in HBM,
after a warm-up, between device synchronisations.  Then one profiled pass per
network prints the kctc_nnet_profile families (ms per step), which split the
difference into the new kernels (relu, relu_backprop, the hidden affine's
share of affine) and the bottom RNN's new work (gemm_bwd_data /
bwd_data_stream, the wider forward projection and weight GEMMs).

The streaming yardstick: the forward-only length-aware pass
(kctc_nnet_propagate_seq) of the plain network is profiled in the same job;
relu / relu_backprop are given as bytes moved over time against its
seq_align rate, twice: inside the FT step, where relu_backprop runs while the
side stream carries the bottom RNN's weight-gradient passes, and alone, in a
network without any RNN (Splice, Affine 40 -> hidden_dim, RectifiedLinear,
ClipGradient, Affine -> 41: nothing runs beside the compute stream), profiled
in the same job.

The dx GEMM the bottom RNN gains runs on the third queue (the streamed GEMMs'),
which the profiler does not span: gemm_bwd_data / bwd_data_stream show no
launches in the streamed path, and its cost is seen in layer_rnn_backward_data,
which ends when the streamed GEMM has joined.

  python scripts/ft_step_time.py [--steps 20] [--blocks 3] [--hidden-dim 1024]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FAMILIES = ["layer_rnn_forward", "rnn_fwd_rec", "gemm_fwd_proj", "x3_pack", "fwd_proj_stream", "fwd_proj_rows",
            "x3_pack_chain", "x3_pack_w_fwd", "relu", "relu_backprop", "relu_stats_add", "layer_ctc", "argmax", "scale", "clip_gradient",
            "layer_rnn_backward_data", "rnn_bwd_rec", "gemm_bwd_data", "bwd_data_stream", "x3_pack_bwd_stream",
            "layer_rnn_backward_weights", "x3_pack_w", "gemm_bwd_w", "gemm_bwd_r", "affine", "update"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hidden-dim", type=int, default=1024)
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
    T, N, D, A, HD = args.T, args.N, 40, 41, args.hidden_dim
    kw = dict(num_rnn=args.layers, input_dim=D, hidden=args.hidden, num_targets=A, rnn_mode=2, learning_rate=5e-4)
    nets = {"plain": k.Nnet(k.recipe_config(**kw), seed=1),
            "ft": k.Nnet(k.recipe_config(model_type="FT", hidden_dim=HD, **kw), seed=1)}
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
    print(f"difference of the medians: {np.median(ms['ft']) - np.median(ms['plain']):.2f} ms/step")
    prof = {}
    for name, net in nets.items():
        net.set_profiling(True)
        block(net, args.steps)
        prof[name] = {f: net.profile(f) for f in FAMILIES}
        net.set_profiling(False)
    print("family: ms/step (launches/step) plain | ft")
    for f in FAMILIES:
        (a, na), (b, nb) = prof["plain"][f], prof["ft"][f]
        if na or nb:
            print(f"  {f}: {a / args.steps:.3f} ({na / args.steps:.1f}) | {b / args.steps:.3f} ({nb / args.steps:.1f})")

    # the yardstick: seq_align in the forward-only length-aware pass of the plain network, same job
    net = nets["plain"]
    f, nf, _, _ = batches[0]
    out = torch.empty((T * N, A), dtype=torch.float32, device=dev)
    lib = k.lib()
    reps = 3
    for profiled in (False, True):  # one pass to size the buffers, then the profiled ones
        net.set_profiling(profiled)
        for _ in range(reps if profiled else 1):
            if lib.kctc_nnet_propagate_seq(net.h, ctypes.c_void_p(f.data_ptr()), T, N, nf.ctypes.data,
                                           ctypes.c_void_p(out.data_ptr()), out.numel()):
                raise SystemExit("kctc_nnet_propagate_seq: " + lib.kctc_last_error().decode())
        torch.cuda.synchronize()
    t_align, n_align = net.profile("seq_align")
    net.set_profiling(False)
    rows, R, H = T * N, args.layers, args.hidden
    x_bytes = 2 * 4 * rows * (D + (R - 1) * 2 * H)  # the masked input copies, read + written
    g_bytes = 2 * 4 * rows * 8 * H * R               # G, both directions
    table = [("seq_align (inference)", (t_align, n_align), reps, x_bytes + g_bytes),
             ("relu (forward: read, write)", prof["ft"]["relu"], args.steps, 2 * 4 * rows * HD),
             ("relu_backprop (read y, dy; write dx; statistics)", prof["ft"]["relu_backprop"], args.steps,
              3 * 4 * rows * HD)]
    base = None
    print("pass: ms per pass (launches), GB per pass, GB/s, rate / seq_align's")
    for name, (t, n), passes, nbytes in table:
        if not n:
            print(f"  {name}: no launches")
            continue
        rate = nbytes * passes / (t * 1e-3) / 1e9
        base = base or rate
        print(f"  {name}: {t / passes:.3f} ms ({n / passes:.0f}), {nbytes / 1e9:.3f} GB, {rate:.0f} GB/s, "
              f"{rate / base:.2f}")
    # the new kernels alone: the front end without any RNN, nothing on the side stream
    alone = k.Nnet(k.recipe_config(num_rnn=0, model_type="FT", hidden_dim=HD, input_dim=D, num_targets=A,
                                   learning_rate=5e-4), seed=1)
    block(alone, args.warmup)
    alone.set_profiling(True)
    block(alone, args.steps)
    pa = {f: alone.profile(f) for f in ("relu", "relu_backprop", "relu_stats_add")}
    alone.set_profiling(False)
    alone.close()
    print("alone (no RNN in the network): ms per pass (launches), GB/s, rate / seq_align's")
    for name, nbytes in (("relu", 2 * 4 * rows * HD), ("relu_backprop", 3 * 4 * rows * HD)):
        t, n = pa[name]
        if not n:
            print(f"  {name}: no launches")
            continue
        rate = nbytes * args.steps / (t * 1e-3) / 1e9
        print(f"  {name}: {t / args.steps:.3f} ms ({n / args.steps:.0f}), {rate:.0f} GB/s, {rate / base:.2f}")
    t, n = pa["relu_stats_add"]
    print(f"  relu_stats_add (inside relu_backprop): {t / args.steps:.3f} ms ({n / args.steps:.0f})")
    for net in nets.values():
        net.close()


if __name__ == "__main__":
    main()
