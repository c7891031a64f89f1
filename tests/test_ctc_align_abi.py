"""CPU-side checks of the forced-alignment ABI (include/ctc.h,
include/kaldi_ctc_decode.h): the new symbols are declared, exported and bound,
the Python names exist, and the workspace query accounts for the log-probs and
the back-pointers."""
import subprocess

import numpy as np

NEW_SYMBOLS = ["mictc_get_align_workspace_size", "mictc_ctc_align_async", "mictc_set_align_kernel",
               "kctc_nnet_align", "kctc_nnet_align_egs"]


def test_align_symbols_exported(kctc):
    L = kctc.lib()
    declared = kctc.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", kctc.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in declared, s  # declared in include/*.h
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s  # bound with a signature
        assert s in exported, s
    for name in ("ctc_align", "ctc_align_kernel", "ctc_align_workspace_size", "read_int_vector_ark"):
        assert callable(getattr(kctc, name, None)), name
    for m in ("align", "align_egs"):
        assert hasattr(kctc.Nnet, m), m


def test_align_kernel_knob_round_trip(kctc):
    prev = kctc.ctc_align_kernel()
    assert prev == 1  # the default: the library picks by size
    assert kctc.ctc_align_kernel(0) == 1 and kctc.ctc_align_kernel() == 0
    assert kctc.ctc_align_kernel(prev) == 0 and kctc.ctc_align_kernel() == prev


def test_align_workspace_size(kctc):
    A = 41
    T, L = [2000, 1800], [250, 225]
    ws = kctc.ctc_align_workspace_size(L, T, A)
    lp = 4 * max(T) * len(T) * A
    bp = sum(t * ((2 * l + 1 + 63) // 64) * 16 for t, l in zip(T, L))  # 2 bits per state, 64-state blocks
    assert lp + bp <= ws <= lp + bp + 4 * max(T) * len(T) + 64 * 1024
    # far below the loss's workspace, which spills two fp32 columns per frame and state
    assert ws < kctc.ctc_workspace_size(L, T, A) / 2
    # invalid lengths: L > 639, negative T
    for ll, il in (([640], [2000]), ([3], [-1])):
        try:
            kctc.ctc_align_workspace_size(ll, il, A)
        except kctc.CtcError as e:
            assert e.status == 2
        else:
            raise AssertionError("expected CTC_STATUS_INVALID_VALUE")


def test_read_int_vector_ark(kctc, tmp_path):
    p = tmp_path / "ali.ark"
    vecs = {"utt-a": np.array([0, 3, 3, 0, 7], np.int32), "b": np.zeros(0, np.int32), "c.3": np.array([5], np.int32)}
    with open(p, "wb") as f:
        for k, v in vecs.items():
            f.write(k.encode() + b" \0B\x04" + np.int32(len(v)).tobytes() + v.tobytes())
    got = kctc.read_int_vector_ark("ark:" + str(p))
    assert list(got) == list(vecs)
    for k in vecs:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], vecs[k])
