"""CPU-side checks of the prefix-beam-search ABI (include/ctc.h,
include/kaldi_ctc_decode.h): the new symbols are declared, exported and bound,
the Python names exist with the documented defaults, and the workspace query
accounts for the log-probs and the prefix nodes and refuses what the search
refuses."""
import inspect
import subprocess

NEW_SYMBOLS = ["mictc_get_beam_workspace_size", "mictc_ctc_beam_search_async", "kctc_nnet_decode",
               "kctc_nnet_decode_egs"]


def test_beam_symbols_exported(kctc):
    L = kctc.lib()
    declared = kctc.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", kctc.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in declared, s  # declared in include/*.h
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s  # bound with a signature
        assert s in exported, s


def test_beam_python_signatures(kctc):
    sig = inspect.signature(kctc.ctc_beam_search)
    assert list(sig.parameters) == ["acts", "input_lengths", "beam", "symbols", "blank", "stream", "workspace"]
    assert [sig.parameters[k].default for k in ("beam", "symbols", "blank", "stream", "workspace")] == \
        [16, 40, 0, None, None]
    assert list(inspect.signature(kctc.ctc_beam_workspace_size).parameters) == ["input_lengths", "alphabet_size",
                                                                                 "beam"]
    sig = inspect.signature(kctc.Nnet.decode)
    assert list(sig.parameters) == ["self", "feats", "T", "N", "num_frames", "beam", "symbols"]
    assert sig.parameters["beam"].default == 16 and sig.parameters["symbols"].default == 40
    sig = inspect.signature(kctc.Nnet.decode_egs)
    assert list(sig.parameters) == ["self", "rspecifier", "wspecifier", "minibatch_size", "beam", "symbols"]
    assert [sig.parameters[k].default for k in ("minibatch_size", "beam", "symbols")] == [16, 16, 40]


def test_beam_workspace_size(kctc):
    A = 41
    T = [2000, 1800]
    for beam in (1, 16, 128):
        ws = kctc.ctc_beam_workspace_size(T, A, beam)
        lp = 4 * max(T) * len(T) * A
        nodes = 16 * sum(T) * beam  # (parent, symbol, length) of at most `beam` new prefixes a frame
        assert lp + nodes <= ws <= lp + nodes + 4 * max(T) * len(T) + 64 * 1024
    assert kctc.ctc_beam_workspace_size([0, 0], A, 16) > 0
    # beam outside [1, 128], alphabet_size < 2, a negative length
    for il, a, beam in ((T, A, 0), (T, A, 129), (T, 1, 16), ([5, -1], A, 16)):
        try:
            kctc.ctc_beam_workspace_size(il, a, beam)
        except kctc.CtcError as e:
            assert e.status == 2
        else:
            raise AssertionError("expected CTC_STATUS_INVALID_VALUE")
