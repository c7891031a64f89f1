"""CPU-side checks of the length-aware training ABI (include/kaldi_rnn.h,
include/kaldi_ctc_train.h): the new symbols are exported and bound, and the
Seq workspace / reserve are at least the plain ones."""
import subprocess

import pytest

NEW_SYMBOLS = ["krnnGetTrainingSeqWorkspaceSize", "krnnGetTrainingSeqReserveSize", "krnnForwardTrainingSeq",
               "krnnBackwardDataSeq", "krnnBackwardWeightsSeq", "kctc_nnet_set_length_aware"]


def test_seq_train_symbols_exported(kctc):
    L = kctc.lib()
    declared = kctc.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", kctc.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in declared, s  # declared in include/*.h
        assert hasattr(L, s), s
        assert s in exported, s
    for m in ("forward_training_seq", "backward_data_seq", "backward_weights_seq", "seq_train_sizes"):
        assert hasattr(kctc.Rnn, m), m
    assert hasattr(kctc.Nnet, "set_length_aware")


@pytest.mark.parametrize("mode,D,H,layers,bidir,T,N", [
    (2, 24, 64, 1, True, 23, 5),
    (3, 40, 512, 2, True, 12, 16),
    (2, 48, 320, 1, False, 16, 5),
    (0, 12, 32, 1, True, 15, 4),
    (2, 40, 512, 1, True, 2000, 16),
])
def test_seq_train_sizes_cover_the_plain_ones(kctc, mode, D, H, layers, bidir, T, N):
    r = kctc.Rnn(mode, D, H, layers, bidir)
    ws, res = r.sizes(T, N)
    sws, sres = r.seq_train_sizes(T, N)
    dirs, nw = (2 if bidir else 1), {0: 1, 1: 1, 2: 4, 3: 3}[mode]
    rows = T * N
    # the plain reserve, the masked input and every stacked layer's shifted output
    assert sres >= res + 4 * rows * (D + layers * dirs * H)
    # the plain workspace; the dGates image(s) before the shift back and the aligned dy
    assert sws >= ws
    assert sws >= 4 * rows * dirs * H * ((2 if mode == 3 else 1) * nw + 1)
    assert r.seq_train_sizes(0, N) == (0, 0)
