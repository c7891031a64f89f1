"""krnnForwardTrainingSeq / krnnBackwardDataSeq / krnnBackwardWeightsSeq
(include/kaldi_rnn.h): a padded batch of N sequences trains as if every
sequence were run alone.

Reference: the fp64 oracle on each sequence alone (N = 1, T = len_n); y[:len_n, n]
and dx[:len_n, n] against that run, dw against the SUM of the runs' dw.  Bars
are test_rnn_gpu.py's (norm-wise relative error): y 1e-5, dx 1e-4, dw 1e-4 and
2e-4 per lin-layer block.  Padding rows of x and dy hold 1e3 and must not
matter; padding rows of y and dx must be +0."""
import functools

import numpy as np
import pytest

from conftest import rel_err
from test_rnn_seq_gpu import CASES as INFER_CASES

pytestmark = pytest.mark.gpu

LSTM, GRU, RELU, TANH = 2, 3, 0, 1

# the fp32 cases of the inference test (the bf16 one: test_seq_train_bf16_not_supported)
CASES = [c for c in INFER_CASES if c[8] is None]
assert [c[0] for c in CASES] == ["v4_lstm", "v3v4_relu", "generic_tanh", "v6_gru_one_group", "v6_lstm_two_groups_of_8",
                                 "v6_gru_stacked_layers", "v6_gru_row_groups_ragged", "v6_lstm_uni", "odd_input_dim"]


def _data(case):
    _, mode, T, lens, D, H, layers, bidir, _, _ = case
    N, dirs = len(lens), 2 if bidir else 1
    rng = np.random.default_rng(T + N + D + H)
    P = _oracle().params_size(mode, D, H, layers, dirs)
    w = (rng.standard_normal(P) * 0.15).astype(np.float32)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    dy = rng.standard_normal((T, N, dirs * H)).astype(np.float32)
    for n, L in enumerate(lens):  # the real rows only; what the padding holds is set per use
        x[L:, n] = 0
        dy[L:, n] = 0
    return w, x, dy


def _oracle():
    import oracle_lib
    return oracle_lib


def _oracle_run(mode, x, w, dy, H, layers, dirs):
    o = _oracle()
    x64, w64 = np.ascontiguousarray(x).astype(np.float64), w.astype(np.float64)
    ry, res = o.rnn_forward(mode, x64, w64, H, layers, dirs)
    rdx, rdw = o.rnn_backward(mode, x64, w64, ry, np.ascontiguousarray(dy).astype(np.float64), res, H, layers, dirs)
    return ry, rdx, rdw


@functools.lru_cache(maxsize=None)
def _reference(cid):
    """Per sequence alone: ([y_n], [dx_n], sum_n dw_n), and the padded batch's dw
    (zero padding: what the plain calls compute).  Computed once per case."""
    case = next(c for c in CASES if c[0] == cid)
    _, mode, T, lens, D, H, layers, bidir, _, _ = case
    dirs = 2 if bidir else 1
    w, x, dy = _data(case)
    ys, dxs, dw = [], [], 0.0
    for n, L in enumerate(lens):
        ry, rdx, rdw = _oracle_run(mode, x[:L, n:n + 1], w, dy[:L, n:n + 1], H, layers, dirs)
        ys.append(ry[:, 0])
        dxs.append(rdx[:, 0])
        dw = dw + rdw
    _, _, dw_padded = _oracle_run(mode, x, w, dy, H, layers, dirs)
    for a in ys + dxs + [dw, dw_padded]:
        a.setflags(write=False)
    return ys, dxs, dw, dw_padded


def _bufs(r, gpu, T, N, D):
    import torch
    ws_b, res_b = r.seq_train_sizes(T, N)
    return dict(y=torch.full((T, N, r.dirs * r.H), 7.0, device=gpu), dx=torch.full((T, N, D), 7.0, device=gpu),
                dw=torch.zeros(r.num_params, device=gpu), ws=torch.empty(ws_b, dtype=torch.uint8, device=gpu),
                res=torch.empty(res_b, dtype=torch.uint8, device=gpu))


def _run_seq(r, b, x, dy, w, lens):
    import torch
    r.forward_training_seq(x, lens, w, b["y"], b["ws"], b["res"])
    r.backward_data_seq(b["y"], dy, lens, w, b["dx"], b["ws"], b["res"])
    r.backward_weights_seq(x, b["y"], lens, b["dw"], b["ws"], b["res"])
    torch.cuda.synchronize()
    assert r.device_status() == 0
    return b["y"].cpu().numpy(), b["dx"].cpu().numpy(), b["dw"].cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_seq_train_matches_oracle_per_utterance(kctc, gpu, oracle, monkeypatch, case):
    import torch
    cid, mode, T, lens, D, H, layers, bidir, _, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N = len(lens)
    ys, dxs, rdw, rdw_padded = _reference(cid)
    # the inputs discriminate: run as a plain padded batch the reverse direction
    # crosses the padding first, and dw is another one (a hundred times the bar)
    if bidir:
        gap = rel_err(rdw_padded, rdw)
        print(f"{cid} padded-batch dw vs per-utterance sum: {gap:.2e}")
        assert gap > 1e-2, gap
    w, x, dy = _data(case)
    for n, L in enumerate(lens):
        x[L:, n] = 1e3  # padding rows: anything finite
        dy[L:, n] = 1e3
    r = kctc.Rnn(mode, D, H, layers, bidir)
    assert r.num_params == w.size
    b = _bufs(r, gpu, T, N, D)
    t = lambda a: torch.from_numpy(a).to(gpu)
    y, dx, dw = _run_seq(r, b, t(x), t(dy), t(w), lens)
    for n, L in enumerate(lens):
        ey, ex = rel_err(y[:L, n], ys[n]), rel_err(dx[:L, n], dxs[n])
        print(f"{cid} n={n} len={L} y {ey:.2e} dx {ex:.2e}")
        assert ey < 1e-5, (n, L, ey)
        assert ex < 1e-4, (n, L, ex)
        for a in (y, dx):  # exactly 0, no sign bit
            assert not a[L:, n].any(), (n, L)
            assert not np.signbit(a[L:, n]).any(), (n, L)
    ew = rel_err(dw, rdw)
    print(f"{cid} dw {ew:.2e}")
    assert ew < 1e-4, ew
    nlin = 2 * (4 if mode == LSTM else 3 if mode == GRU else 1)
    for pl in range(layers * r.dirs):
        for lin in range(nlin):
            for isb in (0, 1):
                off, (h, c) = r.lin_offset(pl, lin, isb)
                sl = slice(off, off + h * c)
                assert rel_err(dw[sl], rdw[sl]) < 2e-4, (pl, lin, isb)


@pytest.mark.parametrize("mode,T,N,D,H,layers", [(LSTM, 13, 4, 16, 32, 1), (GRU, 10, 9, 40, 256, 2)])
def test_seq_train_full_lengths_equal_plain_calls_bitwise(kctc, gpu, mode, T, N, D, H, layers):
    import torch
    rng = np.random.default_rng(5)
    r = kctc.Rnn(mode, D, H, layers, True)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(gpu)
    w = t(rng.standard_normal(r.num_params) * 0.15)
    x, dy = t(rng.standard_normal((T, N, D))), t(rng.standard_normal((T, N, 2 * H)))
    ws_b, res_b = r.sizes(T, N)
    ws, res = torch.empty(ws_b, dtype=torch.uint8, device=gpu), torch.empty(res_b, dtype=torch.uint8, device=gpu)
    y0, dx0, dw0 = torch.empty((T, N, 2 * H), device=gpu), torch.empty((T, N, D), device=gpu), torch.zeros(
        r.num_params, device=gpu)
    r.forward_training(x, w, y0, ws, res)
    r.backward_data(y0, dy, w, dx0, ws, res)
    r.backward_weights(x, y0, dw0, ws, res)
    b = _bufs(r, gpu, T, N, D)
    _run_seq(r, b, x, dy, w, [T] * N)
    assert torch.equal(y0, b["y"])
    assert torch.equal(dx0, b["dx"])
    assert torch.equal(dw0, b["dw"])


def test_seq_train_weights_accumulate(kctc, gpu):
    import torch
    mode, T, lens, D, H = LSTM, 11, [11, 4, 1, 8], 16, 32
    N = len(lens)
    rng = np.random.default_rng(3)
    r = kctc.Rnn(mode, D, H, 1, True)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(gpu)
    w = t(rng.standard_normal(r.num_params) * 0.15)
    x, dy = t(rng.standard_normal((T, N, D))), t(rng.standard_normal((T, N, 2 * H)))
    b = _bufs(r, gpu, T, N, D)
    _, _, dw1 = _run_seq(r, b, x, dy, w, lens)
    r.backward_weights_seq(x, b["y"], lens, b["dw"], b["ws"], b["res"])
    torch.cuda.synchronize()
    np.testing.assert_allclose(b["dw"].cpu().numpy(), 2 * dw1, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("bad", [0, 14])
def test_seq_train_bad_length_is_bad_param(kctc, gpu, bad):
    import torch
    T, N, D, H = 13, 3, 16, 32
    r = kctc.Rnn(LSTM, D, H, 1, True)
    b = _bufs(r, gpu, T, N, D)
    w = torch.zeros(r.num_params, device=gpu)
    x, dy = torch.zeros((T, N, D), device=gpu), torch.zeros((T, N, 2 * H), device=gpu)
    lens = [T, bad, 5]
    with pytest.raises(kctc.RnnError, match="bad parameter"):
        r.forward_training_seq(x, lens, w, b["y"], b["ws"], b["res"])
    with pytest.raises(kctc.RnnError, match="bad parameter"):
        r.backward_data_seq(b["y"], dy, lens, w, b["dx"], b["ws"], b["res"])
    with pytest.raises(kctc.RnnError, match="bad parameter"):
        r.backward_weights_seq(x, b["y"], lens, b["dw"], b["ws"], b["res"])


def test_seq_train_bf16_not_supported(kctc, gpu):
    import torch
    T, N, D, H = 12, 8, 40, 1024  # the inference test's v6_gru_bf16 shape
    r = kctc.Rnn(GRU, D, H, 1, True)
    r.set_precision("bf16")
    b = _bufs(r, gpu, T, N, D)
    w = torch.zeros(r.num_params, device=gpu)
    x, dy = torch.zeros((T, N, D), device=gpu), torch.zeros((T, N, 2 * H), device=gpu)
    lens = [12, 5, 1, 9, 12, 3, 7, 10]
    with pytest.raises(kctc.RnnError, match="not supported"):
        r.forward_training_seq(x, lens, w, b["y"], b["ws"], b["res"])
    with pytest.raises(kctc.RnnError, match="not supported"):
        r.backward_data_seq(b["y"], dy, lens, w, b["dx"], b["ws"], b["res"])
    with pytest.raises(kctc.RnnError, match="not supported"):
        r.backward_weights_seq(x, b["y"], lens, b["dw"], b["ws"], b["res"])
