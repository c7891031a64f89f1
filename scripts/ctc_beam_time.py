"""Cost of the CTC prefix beam search (mictc_ctc_beam_search_async) at the
BASELINE configs[1] CTC shape: N = 16, T_n in [1800, 2000], A = 41, the
lengths of kctc_synth_minibatch, activations 3 * N(0,1) (a label on nearly
every frame: the longest hypotheses and the deepest node pool the shape can
give).  bench.py is not involved.

The search at beam 16 and beam 64 (symbols 40: every label of A = 41) is timed
against ctc_align on the same batch and the same stream, in alternating blocks
of `--calls` calls after a warm-up (the host is shared: only a difference seen
in every pair of blocks counts).  Every call ends in device-to-host copies and
a synchronisation, which the wall-clock figures include.  Then one profiled
pass prints the device time (hipEvent) per launch of every ProfSpan family
involved: ctc_logz, ctc_viterbi and ctc_backtrace for the alignment; ctc_logz,
ctc_beam_search and ctc_beam_backtrace for the search.  The spans are
collected through a one-layer network whose stream the calls run on.

  python scripts/ctc_beam_time.py [--calls 20] [--blocks 3]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
FAMILIES = ["ctc_logz", "ctc_viterbi", "ctc_backtrace", "ctc_beam_search", "ctc_beam_backtrace"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--beams", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--symbols", type=int, default=40)
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
    rng = np.random.default_rng(1)
    acts = torch.from_numpy((rng.standard_normal((T, N, A)) * 3).astype(np.float32)).to(dev)
    # the network only lends its stream and its profiler to the calls
    net = k.Nnet(k.recipe_config(num_rnn=1, input_dim=8, hidden=32, num_targets=A, rnn_mode=2), seed=1)
    stream = net.stream
    ws_ali = torch.empty(k.ctc_align_workspace_size(ll, nf, A), dtype=torch.uint8, device=dev)
    ws_beam = {b: torch.empty(k.ctc_beam_workspace_size(nf, A, b), dtype=torch.uint8, device=dev) for b in args.beams}
    print(f"workspace: alignment {ws_ali.numel() / 2**20:.1f} MiB, " +
          ", ".join(f"beam {b} {w.numel() / 2**20:.1f} MiB" for b, w in ws_beam.items()))

    def align():
        return k.ctc_align(acts, fl, ll, nf, stream=stream, workspace=ws_ali)

    def search(b):
        return lambda: k.ctc_beam_search(acts, nf, beam=b, symbols=args.symbols, stream=stream, workspace=ws_beam[b])

    calls = {"align": align}
    for b in args.beams:
        calls[f"beam{b}"] = search(b)

    def block(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for b in args.beams:
        hyps, scores = calls[f"beam{b}"]()
        print(f"beam {b}: hypothesis lengths {[len(h) for h in hyps[:4]]} scores {scores[:4].tolist()}")
    for fn in calls.values():
        block(fn, args.warmup)
    ms = {name: [] for name in calls}
    for blk in range(args.blocks):
        for name, fn in calls.items():
            ms[name].append(block(fn, args.calls))
        print(f"block {blk}: " + ", ".join(f"{name} {ms[name][-1]:.3f} ms/call" for name in calls), flush=True)
    for name in calls:
        print(f"{name}: median {np.median(ms[name]):.3f} ms/call over {args.blocks} blocks of {args.calls} calls "
              f"(min {min(ms[name]):.3f}, max {max(ms[name]):.3f}; wall clock, host work and the final copies included)")

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
