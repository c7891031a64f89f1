"""Cost of the graph search (kctc_wfst_decode_async) at the BASELINE configs[1]
CTC shape: N = 16, T_n in [1800, 2000], A = 41, the lengths of
kctc_synth_minibatch, log-likelihoods 3 * N(0,1) with +4 on blank through a
log-softmax.  bench.py is not involved.

Two graphs: the token loop (ctc_token_graph: 41 states, 1681 arcs) and a seeded
lexicon graph (ctc_lexicon_graph) of 20 000 random words of 2..8 labels with
random costs in [0, 5).  Each at (beam, max_active) = (15, 7000) and (15, 1000).
Device time by events around `--calls` calls on one stream after a warm-up, in
`--blocks` blocks; per configuration: ms per call, the mean |E_t| (tokens
expanded) and |Q_t| (tokens held) per frame from kctc_wfst_decode_counts, and
frames per second.

  python scripts/wfst_decode_time.py [--calls 5] [--blocks 3]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--words", type=int, default=20000)
    args = ap.parse_args()
    import torch
    from conftest import load_kctc
    k = load_kctc()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    T, N, A = args.T, args.N, 41
    _, nf, _, _ = k.synth_minibatch(20161015, T, N, 40, A, 0.125, want_feats=False)
    print("input lengths:", nf.tolist())
    rng = np.random.default_rng(1)
    x = rng.standard_normal((T, N, A)) * 3
    x[:, :, 0] += 4
    ll = torch.log_softmax(torch.from_numpy(x.astype(np.float32)).to(dev), dim=2).contiguous()
    lex = [(w + 1, rng.integers(1, A, size=int(rng.integers(2, 9))).tolist()) for w in range(args.words)]
    graphs = {"token loop": k.ctc_token_graph(A), f"lexicon {args.words}": k.ctc_lexicon_graph(lex, A, rng.random(args.words) * 5)}
    frames = int(nf.sum())
    for name, g in graphs.items():
        print(f"{name}: {g.info()}")
        for beam, ma in ((15.0, 7000), (15.0, 1000)):
            pool = k.wfst_default_pool_tokens(g, T, ma)
            ws = torch.empty(k.wfst_decode_workspace_size(g, nf, ma, pool), dtype=torch.uint8, device=dev)

            def call():
                return k.wfst_decode(ll, nf, g, beam=beam, max_active=ma, pool_tokens=pool, workspace=ws)

            for _ in range(args.warmup):
                words, ali, scores, status = call()
            e, q = k.wfst_decode_counts(ws, N)
            ms = []
            for _ in range(args.blocks):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                for _ in range(args.calls):
                    call()
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1) / args.calls)
            med = float(np.median(ms))
            print(f"  beam {beam:g} max_active {ma}: {med:.2f} ms/call (blocks {', '.join(f'{m:.2f}' for m in ms)}; "
                  f"events around {args.calls} calls, their result copies included), mean |E_t| {e.sum() / frames:.1f}, "
                  f"mean |Q_t| {q.sum() / (frames + N):.1f}, {frames / med * 1e3:.0f} frames/s, "
                  f"{med / T * 1e3:.1f} us per frame of the longest utterance; workspace {ws.numel() / 2**20:.0f} MiB; "
                  f"status {np.bincount(status + 2, minlength=4).tolist()} (-2, -1, 0, 1), "
                  f"words {[len(w) for w in words[:4]]}", flush=True)


if __name__ == "__main__":
    main()
