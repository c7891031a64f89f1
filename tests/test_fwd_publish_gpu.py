"""The stacked forward recurrence (rec6_fwd.hip rnn_fwd_rec6, kPrecX3S) with 8-row
K partials: a wave folds accumulator register i against register i + 2, writes
8 rows of float4 partials, and only the element threads of rows 0..7 run the
reduction reads and the cell.

1. Layer (D = 40, H = 512, bidirectional, LSTM and GRU) against the fp64
   oracle under test_rnn_gpu.py's bars (norm-wise relative error <= 1e-5 on y,
   <= 1e-4 on dx and dw).  T = 4 takes both ring images and both tags, T = 9
   two full tag periods plus a step.  The library stacks for 8 < N <= 32:
   N = 9 is a full group plus one live row, N = 12 a full and a half-full
   group, N = 16 two full groups.  N = 8 and N = 1 are one group of 16 rows,
   which runs on the IO-wave forward (the same kernel template, 16-row
   partials).
2. The forward of the same layer XCD-pinned (KCTC_XCD6F=1, self-tagged
   hand-off) against unpinned (KCTC_XCD6F=0, flagged hand-off),
   KCTC_FWD_STREAM=0 in both: y and the reserve's gate activations and aux
   (cell state / GRU candidate input) bit for bit."""
import os

import numpy as np
import pytest

from conftest import rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

D, H = 40, 512


def _mk(kctc, gpu, mode, T, N, seed, wscale=0.15):
    import torch
    rng = np.random.default_rng(seed)
    r = kctc.Rnn(mode, D, H, 1, True)
    P = r.num_params
    w = (rng.standard_normal(P) * wscale).astype(np.float32)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    dy = rng.standard_normal((T, N, r.dirs * H)).astype(np.float32)
    ws_b, res_b = r.sizes(T, N)
    t = lambda a: torch.from_numpy(a).to(gpu)
    bufs = dict(w=t(w), x=t(x), dy=t(dy), y=torch.empty((T, N, r.dirs * H), device=gpu),
                dx=torch.empty((T, N, D), device=gpu), dw=torch.zeros(P, device=gpu),
                ws=torch.empty(ws_b, dtype=torch.uint8, device=gpu),
                res=torch.zeros(res_b, dtype=torch.uint8, device=gpu))
    return r, (w, x, dy), bufs


ORACLE = [(mode, T, N) for mode in (2, 3) for T in (4, 9) for N in (1, 8, 9, 12, 16)]


@pytest.mark.parametrize("case", ORACLE, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in ORACLE])
def test_layer_matches_oracle(kctc, gpu, oracle, case):
    import torch
    mode, T, N = case
    r, (w, x, dy), b = _mk(kctc, gpu, mode, T, N, seed=100 + sum(case))
    r.forward_training(b["x"], b["w"], b["y"], b["ws"], b["res"])
    r.backward_data(b["y"], b["dy"], b["w"], b["dx"], b["ws"], b["res"])
    r.backward_weights(b["x"], b["y"], b["dw"], b["ws"], b["res"])
    torch.cuda.synchronize()
    assert r.device_status() == 0
    y, dx, dw = b["y"].cpu().numpy(), b["dx"].cpu().numpy(), b["dw"].cpu().numpy()
    w64, x64 = w.astype(np.float64), x.astype(np.float64)
    ry, res = oracle.rnn_forward(mode, x64, w64, H, 1, r.dirs)
    rdx, rdw = oracle.rnn_backward(mode, x64, w64, ry, dy.astype(np.float64), res, H, 1, r.dirs)
    assert np.isfinite(ry).all() and np.isfinite(rdx).all() and np.isfinite(rdw).all()
    errs = {"y": rel_err(y, ry), "dx": rel_err(dx, rdx), "dw": rel_err(dw, rdw)}
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["y"] < 1e-5
    assert errs["dx"] < 1e-4
    assert errs["dw"] < 1e-4


def _forward(kctc, gpu, mode, T, N, pinned):
    """y, gate activations and aux of one forward."""
    import torch
    env = {"KCTC_FWD_STREAM": "0", "KCTC_XCD6F": "1" if pinned else "0"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        r, _, b = _mk(kctc, gpu, mode, T, N, seed=7 + mode + T + N)
        r.forward_training(b["x"], b["w"], b["y"], b["ws"], b["res"])
        torch.cuda.synchronize()
        assert r.device_status() == 0
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    # reserve (rnn_plan.hip rnn_reserve_layout): gate activations [T N][dirs nw H], then aux [T N][dirs H]
    nw = 4 if mode == 2 else 3
    n_act, n_aux = T * N * r.dirs * nw * H, T * N * r.dirs * H
    assert n_act % 64 == 0
    res = b["res"].cpu().numpy().view(np.float32)
    return b["y"].cpu().numpy(), res[:n_act].copy(), res[n_act:n_act + n_aux].copy()


PIN = [(mode, T, N) for mode in (2, 3) for N in (16, 9) for T in (2, 5, 9)]


@pytest.mark.parametrize("case", PIN, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in PIN])
def test_pinned_forward_bit_identical(kctc, gpu, case):
    mode, T, N = case
    y0, act0, aux0 = _forward(kctc, gpu, mode, T, N, pinned=False)
    y1, act1, aux1 = _forward(kctc, gpu, mode, T, N, pinned=True)
    np.testing.assert_array_equal(y1, y0)
    np.testing.assert_array_equal(act1, act0)
    np.testing.assert_array_equal(aux1, aux0)
