"""The stacked backward recurrence (rec6_bwd.hip rnn_bwd_rec6, kPrecX3S) with
its operand loads off the hand-off waves: waves 6 and 7 fetch every element's
operands three steps ahead into a ring of LDS slots (LDS-DMA), the element
waves read their slot under the hand-off loads, the dGates rows of a layer
without a streaming consumer leave through the LDS stage too, and the
aggregated epoch is stored by wave 4.  Values, sums and their order are those
of the kernel before (cases 1-3 pass on it too).

Shapes: D = 40, H = 512 (the only H the stacked kernel exists for),
bidirectional, LSTM and GRU.  Every case first asks the plan (test hooks
kctc_test_rec6_select and kctc_test_rec_plan) which backward it is about to
run.  The stacked variant exists for 8 < N <= 16 only (rnn_plan.hip
v6_group_rows: groups of 8 rows need N > 8; pick6 as in
test_bwd_handoff_lanes_gpu.py), so N = 3 -- one short group -- cannot run it:
that case asserts that the plan is the plain 16-row kernel (which shares the
step loop's source) and is checked against the oracle all the same, and
N = 11 is added as the stacked short group (a second group of 3 live rows).

1. Layer against the fp64 oracle under test_rnn_gpu.py's bars (norm-wise
   relative error < 1e-5 on y, < 1e-4 on dx and dw).  T = 1 is the prologue
   alone (flagged hand-off), T = 2, 3 the fetches of the prologue with every
   in-loop fetch past the end, T = 4 the first in-loop fetch that is read,
   T = 7 every slot of the ring twice, an odd and an even last step among
   them.  N = 9: a second group with one live row (the fetching twins of its
   dead rows load a live row); N = 16: two full groups.
2. Pinned (KCTC_XCD6=1, self-tagged hand-off) against unpinned (KCTC_XCD6=0,
   flagged), KCTC_BWD_STREAM=0 in both, T = 8, N = 9 and 16: dx, the reserve's
   dGates (GRU: also DX) and the bias partials bit for bit.  Without a stream
   the rows leave as 16-B chunks from the LDS stage on both paths.
3. One training step of two RNN components with dx streamed off the running
   backward recurrence (KCTC_BWD_STREAM=1) against dx after it (=0), N = 16,
   T = 64, three minibatch seeds, under the tolerance of
   test_bwd_chain_gpu.py::test_streamed_dx_matches_unstreamed (2e-6): the
   streamed GEMM trusts the epoch wave 4 stores for the rows behind it.
4. T = 7: the column maxima the recurrence leaves for the weight GEMMs' packs
   (test hook kctc_test_rnn_colmax_offset) and its bias partials equal to
   numpy's on the returned dGates -- the maxima exactly; the partials with the
   kernel's own order of fp32 additions (per row over the steps as the
   direction runs them, then over the group's rows), so exactly too."""
import numpy as np
import pytest

from conftest import rel_err
from test_bwd_chain_gpu import D, H, _backward, _Env, _mk, _train
from test_bwd_handoff_lanes_gpu import _assert_stacked
from test_rec6_select_gpu import PLAIN, X3, _select

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def _assert_variant(kctc, mode, N, pinned=None):
    if N > 8:
        _assert_stacked(kctc, mode, N, pinned)
    else:  # no groups of 8 rows at N <= 8: one group of 16 rows, the plain kernel
        cfg = _select(kctc, mode, X3, H, N, False)[0]
        assert cfg == (16, 512, 1, 16, PLAIN), (mode, N, cfg)


ORACLE = [(mode, T, N) for mode in (2, 3) for T in (1, 2, 3, 4, 7) for N in (3, 9, 11, 16)]


@pytest.mark.parametrize("case", ORACLE, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}" for c in ORACLE])
def test_layer_matches_oracle(kctc, gpu, oracle, case):
    import torch
    mode, T, N = case
    _assert_variant(kctc, mode, N)
    r, (w, x, dy), b = _mk(kctc, gpu, mode, T, N, seed=700 + sum(case))
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


PIN = [(mode, 8, N) for mode in (2, 3) for N in (9, 16)]


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


STREAM = [(mode, seed) for mode in (2, 3) for seed in (31, 32, 33)]


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


BOOK = [(mode, N) for mode in (2, 3) for N in (9, 16)]


@pytest.mark.parametrize("case", BOOK, ids=[f"m{c[0]}_N{c[1]}" for c in BOOK])
def test_column_maxima_and_bias_partials(kctc, gpu, case):
    import torch
    mode, N = case
    T, dirs, nw = 7, 2, 4 if mode == 2 else 3
    G = nw * H
    with _Env({"KCTC_BWD_STREAM": "0"}):
        _assert_stacked(kctc, mode, N, pinned=True)
        r, _, b = _mk(kctc, gpu, mode, T, N, seed=900 + mode + N)
        r.forward_training(b["x"], b["w"], b["y"], b["ws"], b["res"])
        r.backward_data(b["y"], b["dy"], b["w"], b["dx"], b["ws"], b["res"])
        torch.cuda.synchronize()
        assert r.device_status() == 0
    off = kctc.lib().kctc_test_rnn_colmax_offset(mode, X3, D, H, dirs, T, N)
    assert off > 0 and off % 4 == 0 and off + 4 * 2 * dirs * G <= b["ws"].numel()
    cm = b["ws"].cpu().numpy()[off:off + 4 * 2 * dirs * G].view(np.float32).reshape(2, dirs * G)
    # the reserve, as test_bwd_chain_gpu._backward reads it
    al = lambda v: (v + 63) // 64 * 64
    n_act, n_aux = al(T * N * dirs * G), al(T * N * dirs * H)
    res = b["res"].cpu().numpy().view(np.float32)
    o = n_act + n_aux
    e = res[o:o + T * N * dirs * G].reshape(T, N, dirs * G)
    o += n_act
    dxg = e
    if mode == 3:
        dxg = res[o:o + T * N * dirs * G].reshape(T, N, dirs * G)
        o += n_act
    groups = (N + 7) // 8
    bias = res[o:o + groups * dirs * 2 * G].reshape(groups, dirs, 2, G)
    assert np.abs(e).max() > 0
    np.testing.assert_array_equal(cm[0], np.abs(dxg).max(axis=(0, 1)))
    if mode == 3:
        np.testing.assert_array_equal(cm[1], np.abs(e).max(axis=(0, 1)))
    for g in range(groups):
        rows = range(8 * g, min(N, 8 * g + 8))
        for d in range(dirs):
            steps = range(T - 1, -1, -1) if d == 0 else range(T)
            for part, arr in ((0, dxg), (1, e)):
                want = np.zeros(G, np.float32)
                for n in rows:
                    acc = np.zeros(G, np.float32)
                    for t in steps:
                        acc = acc + arr[t, n, d * G:(d + 1) * G]
                    want = want + acc
                np.testing.assert_array_equal(bias[g, d, part], want, err_msg=f"group {g} dir {d} part {part}")
