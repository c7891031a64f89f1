"""krnnForwardInferenceSeq (include/kaldi_rnn.h): N sequences of different
lengths as one batch, each against the fp64 oracle run on that sequence alone.

y[:len_n, n] must match the oracle on x[:len_n, n] (test_rnn_gpu.py's bar,
norm-wise relative error < 1e-5; the bf16 case sketch_common.bf16_tol), every
padding row of y must be exactly 0, and the padding rows of x (filled with
1e3) must not matter."""
import numpy as np
import pytest

import sketch_common as S
from conftest import rel_err

pytestmark = pytest.mark.gpu

LSTM, GRU, RELU, TANH = 2, 3, 0, 1

CASES = [
    # (id, mode, T, lens, D, H, layers, bidir, prec, env)
    ("v4_lstm", LSTM, 23, [23, 7, 1, 16, 22], 24, 64, 1, True, None, {}),
    ("v3v4_relu", RELU, 15, [15, 4, 9, 1], 12, 32, 1, True, None, {}),
    ("generic_tanh", TANH, 5, [5, 3, 1], 12, 32, 1, True, None, {}),
    ("v6_gru_one_group", GRU, 21, [21, 20, 13, 5, 1, 21, 9], 64, 256, 1, True, None, {}),
    # row groups of 8 sequences (KCTC_REC_GS=8): 12 sequences are two groups
    ("v6_lstm_two_groups_of_8", LSTM, 18, [18, 1, 7, 12, 3, 18, 9, 2, 17, 5, 11, 14], 40, 512, 1, True, None,
     {"KCTC_REC_GS": "8"}),
    ("v6_gru_stacked_layers", GRU, 12, [12, 3, 7, 1, 9, 12, 5, 2, 11, 6, 8, 4, 10, 1, 12, 7], 40, 512, 2, True, None,
     {}),
    ("v6_gru_row_groups_ragged", GRU, 20, [20, 1, 13, 7, 19, 4, 16, 9, 2, 20, 11, 5, 18, 3, 14, 8, 6, 17, 10, 12],
     48, 256, 1, True, None, {}),
    ("v6_lstm_uni", LSTM, 16, [16, 3, 10, 1, 8], 48, 320, 1, False, None, {}),
    ("v6_gru_bf16", GRU, 12, [12, 5, 1, 9, 12, 3, 7, 10], 40, 1024, 1, True, "bf16", {}),
    # an input dim that is no multiple of 4: the input mask takes its element-wise path
    ("odd_input_dim", LSTM, 9, [9, 1, 4], 13, 32, 1, True, None, {}),
]


def _mk(kctc, gpu, mode, T, N, D, H, layers, bidir, seed, prec=None):
    import torch
    rng = np.random.default_rng(seed)
    r = kctc.Rnn(mode, D, H, layers, bidir)
    if prec is not None:
        r.set_precision(prec)
    w = (rng.standard_normal(r.num_params) * (0.05 if prec else 0.15)).astype(np.float32)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    ws = torch.empty(r.seq_workspace_size(T, N), dtype=torch.uint8, device=gpu)
    return r, w, x, ws


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_seq_matches_oracle_per_utterance(kctc, gpu, oracle, monkeypatch, case):
    import torch
    _, mode, T, lens, D, H, layers, bidir, prec, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N = len(lens)
    assert max(lens) == T and min(lens) == 1
    r, w, x, ws = _mk(kctc, gpu, mode, T, N, D, H, layers, bidir, seed=T + N + D + H, prec=prec)
    xp = x.copy()
    for n, L in enumerate(lens):
        xp[L:, n] = 1e3  # padding rows: anything finite
    y = torch.full((T, N, r.dirs * H), 7.0, device=gpu)
    r.forward_inference_seq(torch.from_numpy(xp).to(gpu), lens, torch.from_numpy(w).to(gpu), y, ws)
    torch.cuda.synchronize()
    assert r.device_status() == 0
    y = y.cpu().numpy()
    tol = S.bf16_tol(S.layer_stages("y", layers)) if prec else 1e-5
    w64 = w.astype(np.float64)
    for n, L in enumerate(lens):
        ry, _ = oracle.rnn_forward(mode, np.ascontiguousarray(x[:L, n:n + 1]).astype(np.float64), w64, H, layers,
                                   r.dirs)
        e = rel_err(y[:L, n], ry[:, 0])
        print(f"{case[0]} n={n} len={L} rel_err={e:.2e}")
        assert e < tol, (n, L, e)
        assert not y[L:, n].any(), (n, L)  # exactly 0 (also no -0.0 sign bits set: any() sees values only)
        assert not np.signbit(y[L:, n]).any()


@pytest.mark.parametrize("mode,T,N,D,H,layers,bidir", [(LSTM, 13, 4, 16, 32, 1, True), (GRU, 10, 9, 40, 256, 2, True)])
def test_seq_full_lengths_equal_forward_inference_bitwise(kctc, gpu, mode, T, N, D, H, layers, bidir):
    import torch
    r, w, x, ws = _mk(kctc, gpu, mode, T, N, D, H, layers, bidir, seed=5)
    xd, wd = torch.from_numpy(x).to(gpu), torch.from_numpy(w).to(gpu)
    y0 = torch.empty((T, N, r.dirs * H), device=gpu)
    r.forward_inference(xd, wd, y0, torch.empty(r.sizes(T, N)[0], dtype=torch.uint8, device=gpu))
    y1 = torch.empty_like(y0)
    r.forward_inference_seq(xd, [T] * N, wd, y1, ws)
    torch.cuda.synchronize()
    assert r.device_status() == 0
    assert torch.equal(y0, y1)


@pytest.mark.parametrize("bad", [0, 14])
def test_seq_bad_length_is_bad_param(kctc, gpu, bad):
    import torch
    T, N = 13, 3
    r, w, x, ws = _mk(kctc, gpu, LSTM, T, N, 16, 32, 1, True, seed=1)
    y = torch.empty((T, N, 64), device=gpu)
    with pytest.raises(kctc.RnnError, match="bad parameter"):
        r.forward_inference_seq(torch.from_numpy(x).to(gpu), [T, bad, 5], torch.from_numpy(w).to(gpu), y, ws)
