"""Cost of length-aware training (kctc_nnet_set_length_aware) on the BASELINE
configs[1] network (5 x BLSTM-512, T_max 2000, N 16, 40-dim features, 41
targets) over kctc_synth_minibatch batches (T_n in [1800, 2000]).  bench.py is
not involved.

Two networks with the same parameters live in one process, one in the default
mode and one length-aware, and are timed in alternating blocks (the host is
shared: only a difference seen in every pair of blocks counts).  Each block is
`--steps` pipelined train steps on minibatches resident in HBM, after a
warm-up, between device synchronisations.  Then one profiled pass per network
prints the kctc_nnet_profile families (ms per step): what the length-aware
step loses (the streamed projections, dx GEMMs and weight gradients, the
forward-time packs) and what it adds (the seq_* passes).

Kernel-rate yardstick: the same network's length-aware FORWARD-ONLY pass
(kctc_nnet_propagate_seq) is profiled in the same job; its seq_align /
seq_unalign launches move the same images as seq_align_train /
seq_unalign_train, and seq_align_dy / seq_unalign_dgates have the same access
pattern on the dy / dGates images.  Every family's bytes (each image read once
and written once) over its device time is printed as GB/s and as a fraction
of seq_align's rate.

  python scripts/seq_train_time.py [--steps 10] [--blocks 3]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FAMILIES = ["layer_rnn_forward", "rnn_fwd_rec", "gemm_fwd_proj", "x3_pack", "fwd_proj_stream", "fwd_proj_rows",
            "x3_pack_chain", "x3_pack_w_fwd", "seq_align_train", "seq_unalign_train", "layer_ctc", "argmax", "scale",
            "clip_gradient", "layer_rnn_backward_data", "rnn_bwd_rec", "seq_align_dy", "seq_unalign_dgates",
            "gemm_bwd_data", "bwd_data_stream", "x3_pack_bwd_stream", "layer_rnn_backward_weights", "x3_pack_w",
            "gemm_bwd_w", "gemm_bwd_r", "affine", "update"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
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
    T, N, D, A, H = args.T, args.N, 40, 41, args.hidden
    cfg = k.recipe_config(num_rnn=args.layers, input_dim=D, hidden=H, num_targets=A, rnn_mode=2, learning_rate=5e-4)
    nets = {"default": k.Nnet(cfg, seed=1), "length_aware": k.Nnet(cfg, seed=1)}
    nets["length_aware"].set_length_aware(True)
    batches = []
    for step in range(4):
        feats, nf, fl, ll = k.synth_minibatch(20161015 + step, T, N, D, A, 0.125)
        batches.append((torch.from_numpy(feats).to(dev), nf, fl, ll))
    print("num_frames of batch 0:", batches[0][1].tolist())
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
    d, l = np.median(ms["default"]), np.median(ms["length_aware"])
    print(f"difference of the medians: {l - d:.2f} ms/step ({100 * (l / d - 1):.1f} %)")
    prof = {}
    for name, net in nets.items():
        net.set_profiling(True)
        block(net, args.steps)
        prof[name] = {f: net.profile(f) for f in FAMILIES}
        net.set_profiling(False)
    print("family: ms/step (launches/step) default | length_aware")
    for f in FAMILIES:
        (a, na), (b, nb) = prof["default"][f], prof["length_aware"][f]
        if na or nb:
            print(f"  {f}: {a / args.steps:.3f} ({na / args.steps:.1f}) | {b / args.steps:.3f} ({nb / args.steps:.1f})")

    # the yardstick: the forward-only length-aware pass of the same network, same job
    net = nets["length_aware"]
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
    infer = {fam: net.profile(fam) for fam in ("seq_align", "seq_unalign")}
    net.set_profiling(False)
    rows, R = T * N, args.layers
    x_bytes = 2 * 4 * rows * (D + (R - 1) * 2 * H)  # the masked input copies, read + written
    g_bytes = 2 * 4 * rows * 8 * H * R               # G / dGates (LSTM: E == DX), both directions
    y_bytes = 2 * 4 * rows * 2 * H * R               # y / dy
    table = [("seq_align (inference)", infer["seq_align"], reps, x_bytes + g_bytes),
             ("seq_unalign (inference)", infer["seq_unalign"], reps, y_bytes),
             ("seq_align_train", prof["length_aware"]["seq_align_train"], args.steps, x_bytes + g_bytes),
             ("seq_unalign_train", prof["length_aware"]["seq_unalign_train"], args.steps, y_bytes),
             ("seq_align_dy", prof["length_aware"]["seq_align_dy"], args.steps, y_bytes),
             ("seq_unalign_dgates", prof["length_aware"]["seq_unalign_dgates"], args.steps, g_bytes)]
    base = None
    print("pass: ms per network pass (launches), GB per network pass, GB/s, rate / seq_align's")
    for name, (t, n), passes, nbytes in table:
        if not n:
            print(f"  {name}: no launches")
            continue
        rate = nbytes * passes / (t * 1e-3) / 1e9
        base = base or rate
        print(f"  {name}: {t / passes:.3f} ms ({n / passes:.0f}), {nbytes / 1e9:.2f} GB, {rate:.0f} GB/s, "
              f"{rate / base:.2f}")
    for net in nets.values():
        net.close()


if __name__ == "__main__":
    main()
