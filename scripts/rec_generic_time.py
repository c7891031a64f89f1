"""Times forward_training + backward_data of the shapes that run the generic
recurrences (csrc/rec_generic.hip: everything v6 does not compile), which no
bench.py workload reaches:

  python scripts/rec_generic_time.py [--reps 5]

Per shape: T = 256, D = H, bidirectional, one layer; one warm-up, then --reps
timed repetitions between hipEvents (through torch.cuda.Event); prints one
line with the median, min and max in ms and the forward's median alone.  For a same-box A/B of two library
builds run it as $CMD of scripts/gpu_ab_lib.sh."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
RELU, TANH, LSTM, GRU = 0, 1, 2, 3
T = 256
# (name, mode, H, N)
SHAPES = [
    ("lstm_H384_N16", LSTM, 384, 16),   # whole XCD slots
    ("tanh_H256_N16", TANH, 256, 16),
    ("tanh_H528_N2", TANH, 528, 2),     # no whole-slot partition: plain block mapping
    ("tanh_H1536_N16", TANH, 1536, 16),
    ("lstm_H640_N2", LSTM, 640, 2),
]


def main():
    import torch
    from conftest import load_kctc
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    k = load_kctc()
    dev = torch.device("cuda:0")
    for name, mode, H, N in SHAPES:
        r = k.Rnn(mode, H, H, 1, True)
        g = torch.Generator(device=dev).manual_seed(0)
        w = torch.randn(r.num_params, device=dev, generator=g) * 0.02
        x = torch.randn((T, N, H), device=dev, generator=g)
        dy = torch.randn((T, N, 2 * H), device=dev, generator=g)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        ws_b, res_b = r.sizes(T, N)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
        res = torch.empty(res_b, dtype=torch.uint8, device=dev)
        ms, fwd = [], []
        for rep in range(1 + args.reps):  # the first one: warm-up
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            r.forward_training(x, w, y, ws, res)
            e1.record()
            r.backward_data(y, dy, w, dx, ws, res)
            e2.record()
            torch.cuda.synchronize()
            assert r.device_status() == 0
            if rep:
                ms.append(e0.elapsed_time(e2))
                fwd.append(e0.elapsed_time(e1))
        ms.sort()
        fwd.sort()
        print(f"{name} T={T}: median {ms[len(ms) // 2]:.3f} ms (min {ms[0]:.3f}, max {ms[-1]:.3f}; forward alone "
              f"{fwd[len(fwd) // 2]:.3f}) checksum {float(y.double().sum()):.6e} {float(dx.double().sum()):.6e}")


if __name__ == "__main__":
    main()
