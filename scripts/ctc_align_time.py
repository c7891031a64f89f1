"""Cost of the CTC forced alignment (mictc_ctc_align_async) at the BASELINE
configs[1] CTC shape: N = 16, T_n in [1800, 2000], L_n = T_n / 8, A = 41, the
lengths and labels of kctc_synth_minibatch, activations 3 * N(0,1).  bench.py
is not involved.

ctc_align is timed against the costs-only compute_ctc_loss (want_grad=False:
ctc_logz + the alpha recursion, the loss path's kernels as they are) on the
same batch and the same stream, in alternating blocks of `--calls` calls after
a warm-up (the host is shared: only a difference seen in every pair of blocks
counts).  Both calls end in a device-to-host copy of N doubles / floats and a
synchronisation, which the wall-clock figures include.  Then one profiled
pass prints the device time per launch of every ProfSpan family involved:
ctc_logz and ctc_alpha_beta for the loss; ctc_logz, ctc_viterbi and
ctc_backtrace for the alignment.  The spans are collected through a
one-layer network whose stream both calls run on.

  python scripts/ctc_align_time.py [--calls 20] [--blocks 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FAMILIES = ["ctc_logz", "ctc_alpha_beta", "ctc_grad", "ctc_viterbi", "ctc_backtrace"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--N", type=int, default=16)
    args = ap.parse_args()
    import torch
    from conftest import load_kctc
    k = load_kctc()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    T, N, A = args.T, args.N, 41
    _, nf, fl, ll = k.synth_minibatch(20161015, T, N, 40, A, 0.125, want_feats=False)
    print("input lengths:", nf.tolist())
    print("label lengths:", ll.tolist())
    rng = np.random.default_rng(1)
    acts = torch.from_numpy((rng.standard_normal((T, N, A)) * 3).astype(np.float32)).to(dev)
    # the network only lends its stream and its profiler to the two calls
    net = k.Nnet(k.recipe_config(num_rnn=1, input_dim=8, hidden=32, num_targets=A, rnn_mode=2), seed=1)
    stream = net.stream
    ws_loss = torch.empty(k.ctc_workspace_size(ll, nf, A), dtype=torch.uint8, device=dev)
    ws_ali = torch.empty(k.ctc_align_workspace_size(ll, nf, A), dtype=torch.uint8, device=dev)
    print(f"workspace: loss {ws_loss.numel() / 2**20:.1f} MiB, alignment {ws_ali.numel() / 2**20:.1f} MiB")

    def loss():
        return k.compute_ctc_loss(acts, fl, ll, nf, want_grad=False, stream=stream, workspace=ws_loss)[0]

    def align():
        return k.ctc_align(acts, fl, ll, nf, stream=stream, workspace=ws_ali)

    calls = {"loss_costs_only": loss, "align": align}

    def block(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    costs = loss()
    ali, scores = align()
    print("costs[:4]", costs[:4].tolist(), "-scores[:4]", (-scores[:4]).tolist())
    assert np.all(-scores >= costs - 1e-3 * np.abs(costs))  # the best path is no likelier than all paths together
    for fn in calls.values():
        block(fn, args.warmup)
    ms = {name: [] for name in calls}
    for b in range(args.blocks):
        for name, fn in calls.items():
            ms[name].append(block(fn, args.calls))
        print(f"block {b}: " + ", ".join(f"{name} {ms[name][-1]:.3f} ms/call" for name in calls), flush=True)
    for name in calls:
        print(f"{name}: median {np.median(ms[name]):.3f} ms/call over {args.blocks} blocks of {args.calls} calls "
              f"(min {min(ms[name]):.3f}, max {max(ms[name]):.3f}; wall clock, host work and the final copy included)")

    # device time per launch: one profiled pass each; a forward of the lending
    # network collects the spans (its own families are not among FAMILIES)
    x = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    for name, fn in calls.items():
        net.set_profiling(True)
        for _ in range(args.calls):
            fn()
        net.propagate_batch([x])
        prof = {f: net.profile(f) for f in FAMILIES}
        net.set_profiling(False)
        tot = sum(t for t, n in prof.values())
        print(f"{name}: device time {tot / args.calls:.3f} ms/call; per launch:")
        for f, (t, n) in prof.items():
            if n:
                print(f"  {f}: {t / n:.3f} ms ({n / args.calls:.0f} per call)")
    net.close()


if __name__ == "__main__":
    main()
