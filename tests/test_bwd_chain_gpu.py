"""The stacked backward recurrence (rec6_bwd.hip rnn_bwd_rec6, kPrecX3S) with
its operands prefetched two steps ahead and an element set of 8 rows: the
step loop rotates the operands in behind the hand-off wait (no wait on the
step's own stores at its end), dy waits one register stage longer for the
cell, and only the waves that hold live rows run the coefficients, the
reduction reads, the cell and the bookkeeping.

1. Layer (D = 40, H = 512, bidirectional, LSTM and GRU) against the fp64
   oracle under test_rnn_gpu.py's bars (norm-wise relative error < 1e-5 on y,
   < 1e-4 on dx and dw).  T = 1 has no hand-off and no prefetch behind the
   prologue's, T = 2 one rotation and nothing left to load, T = 3 the first
   in-loop prefetch, T = 4 both ring images and both tags, T = 6 and 9 the
   steady state and its last two steps.  The library stacks for 8 < N <= 32:
   N = 9 is a full group plus one live row, N = 12 a full and a half-full
   group, N = 16 two full groups.  N = 1 and N = 8 are one group of 16 rows
   (the plain split-fp16 kernel, which shares the loop).
2. The backward of the same layer XCD-pinned (KCTC_XCD6=1, self-tagged
   hand-off) against unpinned (KCTC_XCD6=0, flagged hand-off),
   KCTC_BWD_STREAM=0 in both: dx and the reserve's dGates (E; GRU also DX) and
   bias partials bit for bit.
3. One training step of two RNN components with dx streamed off the running
   backward recurrence (KCTC_BWD_STREAM=1: write-through dGates rows and the
   aggregated epoch) against dx after it (=0), T = 17, N = 16, under the
   tolerance of test_train_gpu.py::test_streamed_gemms_match_unstreamed."""
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


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


ORACLE = [(mode, T, N) for mode in (2, 3) for T in (1, 2, 3, 4, 6, 9) for N in (1, 8, 9, 12, 16)]


@pytest.mark.parametrize("case", ORACLE, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in ORACLE])
def test_layer_matches_oracle(kctc, gpu, oracle, case):
    import torch
    mode, T, N = case
    r, (w, x, dy), b = _mk(kctc, gpu, mode, T, N, seed=300 + sum(case))
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


def _backward(kctc, gpu, mode, T, N, pinned):
    """dx, the dGates rows and the bias partials of one backward."""
    import torch
    with _Env({"KCTC_BWD_STREAM": "0", "KCTC_XCD6": "1" if pinned else "0"}):
        r, _, b = _mk(kctc, gpu, mode, T, N, seed=11 + mode + T + N)
        r.forward_training(b["x"], b["w"], b["y"], b["ws"], b["res"])
        r.backward_data(b["y"], b["dy"], b["w"], b["dx"], b["ws"], b["res"])
        torch.cuda.synchronize()
        assert r.device_status() == 0
    # reserve (rnn_plan.hip rnn_reserve_layout), every part a multiple of 64 floats:
    # gate activations [T N][dirs nw H], aux [T N][dirs H], E (as the gate
    # activations), GRU: DX (the same), bias partials [N / 8 groups][dirs][2][nw H]
    al = lambda v: (v + 63) // 64 * 64
    nw = 4 if mode == 2 else 3
    n_act, n_aux = al(T * N * r.dirs * nw * H), al(T * N * r.dirs * H)
    n_bias = al(r.dirs * 2 * nw * H * ((N + 7) // 8))
    res = b["res"].cpu().numpy().view(np.float32)
    o = n_act + n_aux
    e = res[o:o + n_act].copy()
    o += n_act
    dxg = None
    if mode == 3:
        dxg = res[o:o + n_act].copy()
        o += n_act
    bias = res[o:o + n_bias].copy()
    assert np.abs(e).max() > 0 and np.abs(bias).max() > 0
    return b["dx"].cpu().numpy(), e, dxg, bias


PIN = [(mode, T, N) for mode in (2, 3) for N in (16, 9) for T in (2, 5, 9)]


@pytest.mark.parametrize("case", PIN, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in PIN])
def test_pinned_backward_bit_identical(kctc, gpu, case):
    mode, T, N = case
    dx0, e0, g0, b0 = _backward(kctc, gpu, mode, T, N, pinned=False)
    dx1, e1, g1, b1 = _backward(kctc, gpu, mode, T, N, pinned=True)
    np.testing.assert_array_equal(dx1, dx0)
    np.testing.assert_array_equal(e1, e0)
    if mode == 3:
        np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(b1, b0)


def _train(kctc, gpu, cfg, batch, env, steps=1):
    import torch
    feats, nf, fl, ll, T, N = batch
    with _Env(env):
        net = kctc.Nnet(cfg, seed=11)
        f = torch.from_numpy(feats).to(gpu)
        stats = [net.train_step(f, T, N, nf, fl, ll) for _ in range(steps)]
        objf = net.compute_objf(f, T, N, nf, fl, ll)[0]
        params = [net.get_params(c).astype(np.float64) for c in range(net.num_components) if net.num_params(c)]
        net.close()
    return stats, objf, params


@pytest.mark.parametrize("mode", [2, 3])
def test_streamed_dx_matches_unstreamed(kctc, gpu, mode):
    A, R, N, T = 41, 2, 16, 17
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, learning_rate=5e-4,
                             max_seq_length=T, rnn_mode=mode)
    feats, nf, fl, ll = kctc.synth_minibatch(7 + N, T, N, D, A, 0.125)
    batch = (feats, nf, fl, ll, T, N)
    a = _train(kctc, gpu, cfg, batch, {"KCTC_BWD_STREAM": "0"})
    b = _train(kctc, gpu, cfg, batch, {"KCTC_BWD_STREAM": "1"})
    tol = 2e-6
    np.testing.assert_allclose(b[1], a[1], rtol=tol)
    for x, y in zip(b[2], a[2]):
        err = rel_err(x, y)
        print(mode, f"{err:.2e}")
        assert err < tol / 2
