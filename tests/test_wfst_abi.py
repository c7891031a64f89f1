"""CPU-side checks of the graph-search ABI (include/kaldi_ctc_decode.h): the
new symbols are declared, exported and bound, the Python names exist with the
documented defaults, the workspace query lies between the documented lower
bound and that bound plus the documented slack, and the invalid-value cases
return before anything touches a device (the pointers they are given are not
device memory: a launch or a copy would fail, not return 2)."""
import ctypes
import inspect
import subprocess

import numpy as np

NEW_SYMBOLS = ["kctc_graph_create", "kctc_graph_read_text", "kctc_graph_write_text", "kctc_graph_info",
               "kctc_graph_get", "kctc_graph_destroy", "kctc_wfst_decode_workspace_size", "kctc_wfst_decode_async",
               "kctc_wfst_decode_counts",
               "kctc_nnet_decode_graph", "kctc_nnet_decode_graph_egs"]


def test_wfst_symbols_exported(kctc):
    L = kctc.lib()
    declared = kctc.exported_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", kctc.LIB_PATH], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        assert s in exported, s


def test_wfst_python_signatures(kctc):
    sig = inspect.signature(kctc.wfst_decode)
    assert list(sig.parameters) == ["loglikes", "input_lengths", "graph", "beam", "max_active", "acoustic_scale",
                                    "pool_tokens", "stream", "workspace"]
    assert [sig.parameters[k].default for k in ("beam", "max_active", "acoustic_scale", "pool_tokens", "stream",
                                                "workspace")] == [15.0, 7000, 1.0, None, None, None]
    for name in ("read_text", "write_text", "num_states", "num_arcs", "eps_depth", "close"):
        assert hasattr(kctc.Graph, name), name
    sig = inspect.signature(kctc.Nnet.decode_graph)
    assert list(sig.parameters)[:6] == ["self", "feats", "T", "N", "num_frames", "graph"]
    assert sig.parameters["beam"].default == 15.0 and sig.parameters["max_active"].default == 7000
    assert list(inspect.signature(kctc.Nnet.decode_graph_egs).parameters)[:4] == ["self", "rspecifier",
                                                                                   "words_wspecifier", "graph"]
    assert list(inspect.signature(kctc.ctc_token_graph).parameters) == ["A", "blank"]
    assert list(inspect.signature(kctc.ctc_lexicon_graph).parameters) == ["lexicon", "A", "word_costs", "blank"]


def test_wfst_workspace_size(kctc):
    g = kctc.ctc_lexicon_graph([(1, [1, 2]), (2, [2, 3, 3]), (3, [3])], 5)
    S = g.num_states
    for lens, pool in (([2000, 1800], 100000), ([0], 1), ([7, 9, 3], 12345)):
        N, maxT = len(lens), max(lens)
        ws = kctc.wfst_decode_workspace_size(g, lens, 7000, pool)
        lower = N * (52 * S + 4 * (maxT + 2) + 8 * pool)
        assert lower <= ws <= lower + 4096 + 2592 * N, (ws, lower)
    # max_active outside [1, 2^20], pool_tokens < 1, a negative length, no utterance
    for lens, ma, pool in (([5], 0, 10), ([5], (1 << 20) + 1, 10), ([5], 10, 0), ([5, -1], 10, 10), ([], 10, 10)):
        try:
            kctc.wfst_decode_workspace_size(g, lens, ma, pool)
        except kctc.CtcError as e:
            assert e.status == 2
        else:
            raise AssertionError("expected invalid value")


def test_wfst_decode_invalid_values_enqueue_nothing(kctc):
    L = kctc.lib()
    g = kctc.ctc_token_graph(5)  # reads columns 0..4
    host = np.zeros(4096, np.float32)  # stands for every device pointer: never touched by a refused call
    p = host.ctypes.data
    lens = np.array([3, 2], np.int32)

    def call(graph=g.h, ll=p, il=lens.ctypes.data, A=5, N=2, scale=1.0, beam=15.0, ma=100, pool=100, words=p, wl=p,
             ali=p, scores=p, status=p, ws=p):
        return L.kctc_wfst_decode_async(graph, ll, il, A, N, scale, beam, ma, pool, words, wl, ali, scores, status, ws,
                                        None)

    bad = np.array([3, -2], np.int32)
    cases = dict(column=dict(A=4), length=dict(il=bad.ctypes.data), graph=dict(graph=None), loglikes=dict(ll=None),
                 lengths=dict(il=None), words=dict(words=None), words_len=dict(wl=None), ali=dict(ali=None),
                 scores=dict(scores=None), status=dict(status=None), workspace=dict(ws=None), beam0=dict(beam=0.0),
                 beam_nan=dict(beam=float("nan")), max_active0=dict(ma=0), max_active_big=dict(ma=(1 << 20) + 1),
                 pool0=dict(pool=0), N0=dict(N=0), scale_inf=dict(scale=float("inf")))
    for name, kw in cases.items():
        assert call(**kw) == 2, name
    assert (host == 0).all()
