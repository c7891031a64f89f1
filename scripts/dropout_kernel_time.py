"""Launches DropoutComponent's forward and backward kernels (csrc/dropout.hip)
at [32000][1024] -- the layer output of BASELINE configs[1] (T_max 2000 x N 16,
BLSTM-512) -- beside scale_inplace (csrc/elementwise.hip k_scale; the same
bytes: one read and one write per element) on the same element count, for a
kernel trace:

  rocprofv3 --kernel-trace --stats -d OUT -o dropout --output-format csv -- \
      python scripts/dropout_kernel_time.py
  python scripts/dropout_kernel_time.py --summarise OUT

The second form reads the kernel trace written by the first and prints, per
kernel, the median time and the HBM bandwidth that 8 bytes per element
imply.  scale_inplace is reached through UpdatableComponent::Scale of an
AffineComponent with (1023 + 1) x 32000 parameters."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROWS, DIM, REPS = 32000, 1024, 20


def run():
    import torch
    from conftest import load_kctc
    k = load_kctc()
    dev = torch.device("cuda:0")
    x = torch.randn((ROWS, DIM), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    d = k.Component(f"DropoutComponent dim={DIM} dropout-proportion=0.2", seed=1)
    a = k.Component(f"AffineComponent input-dim={DIM - 1} output-dim={ROWS} learning-rate=0.001 param-stddev=0.01 "
                    "bias-stddev=0.01", seed=1)
    assert a.NumParameters() == ROWS * DIM
    for _ in range(3 + REPS):  # the first three of each: warm-up (dropped by --summarise)
        d.Propagate(ROWS, 1, x, y)
        d.Backprop(ROWS, 1, None, None, x, None, y)
        a.Scale(1.0)
    torch.cuda.synchronize()
    d.close()
    a.close()


def summarise(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {out_dir}")
    times = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Kernel_Name"]
        n = "dropout" if "k_dropout_vec" in name else "scale_inplace" if "k_scale" in name else None
        if n:
            times.setdefault(n, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    nbytes = 8.0 * ROWS * DIM
    med = {}
    for n, t in sorted(times.items()):
        t = sorted(t[6 if n == "dropout" else 3:])  # warm-up launches
        med[n] = t[len(t) // 2]
        print(f"{n}: {len(t)} launches, median {med[n]:.1f} us (min {t[0]:.1f}, max {t[-1]:.1f}), "
              f"{nbytes / med[n] * 1e-6:.2f} TB/s at 8 bytes per element")
    if len(med) == 2:
        print(f"dropout / scale_inplace = {med['dropout'] / med['scale_inplace']:.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", metavar="DIR")
    args = ap.parse_args()
    summarise(args.summarise) if args.summarise else run()
