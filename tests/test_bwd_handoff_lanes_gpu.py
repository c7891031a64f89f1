"""The stacked backward recurrence (rec6_bwd.hip rnn_bwd_rec6, kPrecX3S) with
its hand-off on live lanes: the lower four waves load the partial dh, half a
wave per producer, and sum them into `red`; the upper four load nothing and
wait for their own stores in front of the step's first barrier instead of in
a poll.  Sums, exchange layout and results are those of the kernel before
(these tests pass on it too); they add the row groups and lengths
test_bwd_chain_gpu.py leaves out.

Shapes: D = 40, H = 512 (the only H the stacked kernel exists for),
bidirectional, LSTM and GRU.  Every case first asks the plan (test hooks
kctc_test_rec6_select and kctc_test_rec_plan) that the backward it is about to
run is the stacked variant, and in the pinned legs that it is XCD-pinned.
N = 17, 24 and 32 are left out: the plan of the build before this change is
not the stacked variant for them -- by default they run as groups of 16 (the
plain kernel), and with KCTC_REC_GS=8 their three or four groups of U = 16
would be 192 or 256 workgroups, above pick6's 128, so the plan is U = 32 plain
(rnn_plan.hip pick6: the stacked kernel runs at most two row groups, N <= 16).

1. Layer against the fp64 oracle under test_rnn_gpu.py's bars (norm-wise
   relative error < 1e-5 on y, < 1e-4 on dx and dw).  N = 10 and 15: a second
   group of 2 and of 7 live rows.  T = 5 and 8: both ring images and both tag
   values at least twice, an odd and an even last step.
2. Pinned (KCTC_XCD6=1, self-tagged hand-off) against unpinned (KCTC_XCD6=0,
   flagged), KCTC_BWD_STREAM=0 in both, the same N, T = 8: dx, the reserve's
   dGates (GRU: also DX) and the bias partials bit for bit.
3. One training step of two RNN components with dx streamed off the running
   backward recurrence (KCTC_BWD_STREAM=1) against dx after it (=0), N = 16,
   T = 64, three minibatch seeds, under the tolerance of
   test_bwd_chain_gpu.py::test_streamed_dx_matches_unstreamed (2e-6).  The
   streamed GEMM trusts the aggregated epoch for the write-through dGates rows
   of waves that no longer poll; T = 64 lets it consume many epochs while the
   recurrence runs."""
import numpy as np
import pytest

from conftest import rel_err
from test_bwd_chain_gpu import D, H, _backward, _Env, _mk, _train
from test_rec6_select_gpu import STACKED, X3, _select
from test_rec_plan_gpu import _plan

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

NS = (10, 15)


def _assert_stacked(kctc, mode, N, pinned=None):
    cfg = _select(kctc, mode, X3, H, N, False)[0]
    assert cfg == (16, 512, (N + 7) // 8, 8, STACKED), (mode, N, cfg)
    if pinned is not None:
        plan = _plan(kctc, mode, X3, H, N, False)
        assert plan[0] == 6 and plan[7] == (1 if pinned else 0), (mode, N, plan)
        assert (plan[5] != 0) == pinned, (mode, N, plan)


ORACLE = [(mode, T, N) for mode in (2, 3) for T in (5, 8) for N in NS]


@pytest.mark.parametrize("case", ORACLE, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in ORACLE])
def test_layer_matches_oracle(kctc, gpu, oracle, case):
    import torch
    mode, T, N = case
    _assert_stacked(kctc, mode, N)
    r, (w, x, dy), b = _mk(kctc, gpu, mode, T, N, seed=500 + sum(case))
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


PIN = [(mode, 8, N) for mode in (2, 3) for N in NS]


@pytest.mark.parametrize("case", PIN, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in PIN])
def test_pinned_backward_bit_identical(kctc, gpu, case):
    mode, T, N = case
    out = []
    for pinned in (False, True):
        with _Env({"KCTC_XCD6": "1" if pinned else "0"}):
            _assert_stacked(kctc, mode, N, pinned)
        out.append(_backward(kctc, gpu, mode, T, N, pinned=pinned))
    (dx0, e0, g0, b0), (dx1, e1, g1, b1) = out
    np.testing.assert_array_equal(dx1, dx0)
    np.testing.assert_array_equal(e1, e0)
    if mode == 3:
        np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(b1, b0)


STREAM = [(mode, seed) for mode in (2, 3) for seed in (23, 24, 25)]


@pytest.mark.parametrize("case", STREAM, ids=[f"m{c[0]}_s{c[1]}" for c in STREAM])
def test_streamed_dx_matches_unstreamed(kctc, gpu, case):
    mode, seed = case
    A, R, N, T = 41, 2, 16, 64
    _assert_stacked(kctc, mode, N, pinned=True)
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, learning_rate=5e-4,
                             max_seq_length=T, rnn_mode=mode)
    feats, nf, fl, ll = kctc.synth_minibatch(seed, T, N, D, A, 0.125)
    batch = (feats, nf, fl, ll, T, N)
    a = _train(kctc, gpu, cfg, batch, {"KCTC_BWD_STREAM": "0"})
    b = _train(kctc, gpu, cfg, batch, {"KCTC_BWD_STREAM": "1"})
    tol = 2e-6
    np.testing.assert_allclose(b[1], a[1], rtol=tol)
    for x, y in zip(b[2], a[2]):
        err = rel_err(x, y)
        print(case, f"{err:.2e}")
        assert err < tol / 2
