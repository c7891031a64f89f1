"""kaldi-ctc_amd -- MI355X-native CTC acoustic-model training path.

Host-side mirror of the reference's interfaces over the C-ABI HIP library
libkaldictc_amd.so (built from csrc/ by the Makefile next to this file):

  * warp-ctc ABI (include/ctc.h): compute_ctc_loss / get_workspace_size /
    ctcGetStatusString -- replaces warp-ctc at src/ctc/ctc-nnet-update.cc:211-243.
  * cuDNN-shaped RNN ABI (include/kaldi_rnn.h) -- replaces the
    kaldi::cudnn::Recurrent* shim of src/cudamatrix/cudnn-recurrent.h.
  * nnet2 trainer ABI (include/kaldi_ctc_train.h) -- the NnetCtcUpdater /
    TrainNnetSimple step (src/ctc/ctc-nnet-update.cc:94-128,
    src/ctc/ctc-nnet-train.cc:181-284) on device buffers.
  * egs ABI (include/kaldi_ctc_egs.h) -- NnetCtcExample archives, the
    CompressedMatrix codec, NnetCtcExampleBackgroundReader and FormatNnetInput
    decoded on the GPU (src/ctc/ctc-nnet-example.cc, ctc-nnet-train.cc:31-183,
    ctc-nnet-update.cc:351-424, src/matrix/compressed-matrix.cc).

torch is used only as plumbing (device memory, streams, torch.distributed
rendezvous).  Every entry point fails loudly when the HIP library is missing;
there is no CPU fallback.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libkaldictc_amd.so")

CTC_CPU, CTC_GPU = 0, 1
CTC_STATUS = {0: "CTC_STATUS_SUCCESS", 1: "CTC_STATUS_MEMOPS_FAILED", 2: "CTC_STATUS_INVALID_VALUE",
              3: "CTC_STATUS_EXECUTION_FAILED", 4: "CTC_STATUS_UNKNOWN_ERROR"}

_lib = None


class CtcOptions(ctypes.Structure):
    """struct ctcOptions { ctcComputeLocation loc; union { unsigned num_threads;
    hipStream_t stream; }; int blank_label; }  (include/ctc.h)"""
    _fields_ = [("loc", ctypes.c_int), ("stream", ctypes.c_void_p), ("blank_label", ctypes.c_int)]


class CtcError(RuntimeError):
    def __init__(self, status, where):
        msg = lib().ctcGetStatusString(status).decode()
        super().__init__(f"ctcStatus_t {status} : \"{msg}\" returned from '{where}'")
        self.status = status


class KctcError(RuntimeError):
    pass


def build(verbose=False):
    import subprocess
    subprocess.run(["make", "-s" if not verbose else "-j8", "-j8", "-C", HERE], check=True)


def lib():
    """Load libkaldictc_amd.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KctcError(f"{LIB_PATH} is missing: run `make -C {HERE}` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, ip, sz = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t
    L.get_warpctc_version.restype = ctypes.c_int
    L.ctcGetStatusString.argtypes = [ctypes.c_int]
    L.ctcGetStatusString.restype = ctypes.c_char_p
    L.compute_ctc_loss.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, CtcOptions]
    L.compute_ctc_loss.restype = ctypes.c_int
    L.get_workspace_size.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, CtcOptions,
                                     ctypes.POINTER(sz)]
    L.get_workspace_size.restype = ctypes.c_int
    L.mictc_compute_ctc_loss_async.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int, ctypes.c_int,
                                               vp, vp, vp, ctypes.c_int]
    L.mictc_compute_ctc_loss_async.restype = ctypes.c_int
    L.mictc_set_frame_group.argtypes = [ctypes.c_int]
    L.mictc_set_frame_group.restype = ctypes.c_int
    L.mictc_set_win.argtypes = [ctypes.c_int]
    L.mictc_set_win.restype = ctypes.c_int
    _bind_optional(L)
    _lib = L
    return L


def _bind_optional(L):
    """Bindings for the RNN / trainer ABIs (added as those layers land)."""
    from . import _bindings  # noqa: F401  (relative import when loaded as a package)
    _bindings.bind(L)


def exported_symbols():
    """Symbols declared by include/*.h (checked by tests/test_abi.py)."""
    import re
    inc = os.path.join(os.path.dirname(HERE), "include")
    names = []
    for fn in sorted(os.listdir(inc)):
        if fn.endswith(".h"):
            txt = open(os.path.join(inc, fn)).read()
            txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
            txt = re.sub(r"^\s*typedef[^;]*;", "", txt, flags=re.M)  # function-pointer types are not symbols
            names += re.findall(r"^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b([a-zA-Z_]\w*)\s*\([^;{]*\)\s*;",
                                txt, flags=re.M)
    return sorted(set(n for n in names if n not in ("if", "while", "for", "return")))


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    raise TypeError(type(x))


def _stream_handle(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def ctc_frame_group(m=0):
    """Frames per barrier of the alpha/beta kernel (mictc_set_frame_group):
    sets it when m > 0; returns the previous value."""
    return lib().mictc_set_frame_group(int(m))


def ctc_window_kernel(on=-1):
    """Overlapping-window alpha/beta kernel on (1, default) / off (0: the
    long-label kernel for every batch) (mictc_set_win); returns the previous
    value (on < 0: query only)."""
    return lib().mictc_set_win(int(on))


def ctc_workspace_size(label_lengths, input_lengths, alphabet_size):
    ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    opts = CtcOptions(CTC_GPU, None, 0)
    out = ctypes.c_size_t()
    st = lib().get_workspace_size(ll.ctypes.data, il.ctypes.data, int(alphabet_size), len(ll),
                                  opts, ctypes.byref(out))
    if st != 0:
        raise CtcError(st, "get_workspace_size")
    return out.value


def compute_ctc_loss(acts, flat_labels, label_lengths, input_lengths, want_grad=True, blank=0,
                     stream=None, workspace=None):
    """warp-ctc compute_ctc_loss on a torch CUDA tensor acts [T, N, A] (float32).
    Returns (costs np.float32 [N], grads tensor or None)."""
    import torch
    assert acts.is_cuda and acts.dtype == torch.float32 and acts.is_contiguous()
    T, N, A = acts.shape
    fl = np.ascontiguousarray(flat_labels, dtype=np.int32)
    if fl.size == 0:
        fl = np.zeros(1, np.int32)
    ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    if workspace is None:
        workspace = torch.empty(ctc_workspace_size(ll, il, A), dtype=torch.uint8, device=acts.device)
    grads = torch.empty_like(acts) if want_grad else None
    costs = np.zeros(N, np.float32)
    opts = CtcOptions(CTC_GPU, _stream_handle(stream), blank)
    st = lib().compute_ctc_loss(acts.data_ptr(), _ptr(grads), fl.ctypes.data, ll.ctypes.data,
                                il.ctypes.data, A, N, costs.ctypes.data, workspace.data_ptr(), opts)
    if st != 0:
        raise CtcError(st, "compute_ctc_loss")
    return costs, grads


def ctc_align_kernel(on=-1):
    """One-state-per-thread Viterbi kernel for short label sequences on (1,
    default) / off (0: the 512-thread, 3-state kernel for every batch)
    (mictc_set_align_kernel); returns the previous value (on < 0: query only)."""
    return lib().mictc_set_align_kernel(int(on))


def ctc_align_workspace_size(label_lengths, input_lengths, alphabet_size):
    ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    out = ctypes.c_size_t()
    st = lib().mictc_get_align_workspace_size(ll.ctypes.data, il.ctypes.data, int(alphabet_size), len(ll),
                                              ctypes.byref(out))
    if st != 0:
        raise CtcError(st, "mictc_get_align_workspace_size")
    return out.value


def ctc_align(acts, flat_labels, label_lengths, input_lengths, blank=0, stream=None, workspace=None):
    """CTC forced alignment (mictc_ctc_align_async) of a torch CUDA tensor acts
    [T, N, A] (float32, un-normalised) to the given transcripts.  Returns
    (ali int32 CUDA tensor [T, N]: the symbol of every frame, blank included,
    -1 on the padding rows and for an utterance whose labels do not fit;
    scores np.float64 [N]: the log-probability of each path, -inf likewise)."""
    import torch
    assert acts.is_cuda and acts.dtype == torch.float32 and acts.is_contiguous()
    T, N, A = acts.shape
    fl = np.ascontiguousarray(flat_labels, dtype=np.int32)
    if fl.size == 0:
        fl = np.zeros(1, np.int32)
    ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    if len(il) != N or len(ll) != N or (N and int(il.max()) > T):
        raise CtcError(2, "ctc_align")
    if workspace is None:
        workspace = torch.empty(ctc_align_workspace_size(ll, il, A), dtype=torch.uint8, device=acts.device)
    # the call fills the rows below max(input_lengths); T may be longer
    ali = torch.full((T, N), -1, dtype=torch.int32, device=acts.device)
    scores = torch.empty(N, dtype=torch.float64, device=acts.device)
    s = _stream_handle(stream)
    if stream is not None:
        torch.cuda.current_stream().synchronize()  # ali's fill ran on the current stream
    st = lib().mictc_ctc_align_async(acts.data_ptr(), fl.ctypes.data, ll.ctypes.data, il.ctypes.data, A, N,
                                     ali.data_ptr(), scores.data_ptr(), workspace.data_ptr(), s, blank)
    if st != 0:
        raise CtcError(st, "mictc_ctc_align_async")
    if stream is not None:
        torch.cuda.synchronize()  # the scores' copy below runs on the current stream
    return ali, scores.cpu().numpy()


def ctc_beam_workspace_size(input_lengths, alphabet_size, beam):
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    out = ctypes.c_size_t()
    st = lib().mictc_get_beam_workspace_size(il.ctypes.data, int(alphabet_size), len(il), int(beam),
                                             ctypes.byref(out))
    if st != 0:
        raise CtcError(st, "mictc_get_beam_workspace_size")
    return out.value


def ctc_beam_search(acts, input_lengths, beam=16, symbols=40, blank=0, stream=None, workspace=None):
    """Lexicon-free CTC prefix beam search (mictc_ctc_beam_search_async) of a
    torch CUDA tensor acts [T, N, A] (float32, un-normalised): `beam` prefixes,
    each frame extending by its `symbols` most likely labels.  Returns (hyps:
    list of N int lists, the most likely label sequence the beam found for
    each utterance; scores np.float64 [N]: the log-probability the beam holds
    for it, a lower bound of its CTC log-probability)."""
    import torch
    assert acts.is_cuda and acts.dtype == torch.float32 and acts.is_contiguous()
    T, N, A = acts.shape
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    if len(il) != N or (N and int(il.max()) > T):
        raise CtcError(2, "ctc_beam_search")
    if workspace is None:
        workspace = torch.empty(ctc_beam_workspace_size(il, A, beam), dtype=torch.uint8, device=acts.device)
    max_t = int(il.max()) if N else 0
    hyp = torch.empty((N, max(max_t, 1)), dtype=torch.int32, device=acts.device)
    hyp_len = torch.empty(N, dtype=torch.int32, device=acts.device)
    scores = torch.empty(N, dtype=torch.float64, device=acts.device)
    st = lib().mictc_ctc_beam_search_async(acts.data_ptr(), il.ctypes.data, A, N, int(beam), int(symbols),
                                           hyp.data_ptr(), hyp_len.data_ptr(), scores.data_ptr(),
                                           workspace.data_ptr(), _stream_handle(stream), blank)
    if st != 0:
        raise CtcError(st, "mictc_ctc_beam_search_async")
    if stream is not None:
        torch.cuda.synchronize()  # the copies below run on the current stream
    hyp, hyp_len = hyp.cpu().numpy().reshape(-1), hyp_len.cpu().numpy()
    return [hyp[n * max_t:n * max_t + int(hyp_len[n])].tolist() for n in range(N)], scores.cpu().numpy()


class Graph:
    """A decoding graph (kctcGraph_t, include/kaldi_ctc_decode.h): a weighted
    finite-state transducer in the tropical semiring.  final_costs [S] (+inf:
    not final); src, ilabel, olabel, weight, dst: one entry per arc, any order
    (arc ids are the positions after a stable sort by src).  ilabel 0 is an
    epsilon arc; ilabel i >= 1 reads column ilabel_to_col[i] (default i - 1).
    Creation validates on the host and needs no GPU."""

    def __init__(self, final_costs=None, src=(), ilabel=(), olabel=(), weight=(), dst=(), start=0,
                 ilabel_to_col=None, _handle=None):
        self.h = None
        if _handle is not None:
            self.h = _handle
            return
        fin = np.ascontiguousarray(final_costs, dtype=np.float32)
        arrs = [np.ascontiguousarray(x, dtype=np.int32) for x in (src, ilabel, olabel, dst)]
        w = np.ascontiguousarray(weight, dtype=np.float32)
        if fin.ndim != 1 or any(x.ndim != 1 or x.size != w.size for x in arrs) or w.ndim != 1:
            raise KctcError("Graph: final_costs and the five arc arrays must be 1-D, the arc arrays of one length")
        col = None if ilabel_to_col is None else np.ascontiguousarray(ilabel_to_col, dtype=np.int32)
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_graph_create(ctypes.byref(h), fin.size, int(start), fin.ctypes.data, w.size,
                                        arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, w.ctypes.data,
                                        arrs[3].ctypes.data, None if col is None else col.ctypes.data,
                                        0 if col is None else col.size), "graph_create")
        self.h = h

    @classmethod
    def read_text(cls, path, ilabel_to_col=None):
        """OpenFst text form (fstprint without symbol tables)."""
        col = None if ilabel_to_col is None else np.ascontiguousarray(ilabel_to_col, dtype=np.int32)
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_graph_read_text(ctypes.byref(h), str(path).encode(),
                                           None if col is None else col.ctypes.data,
                                           0 if col is None else col.size), "graph_read_text")
        return cls(_handle=h)

    def write_text(self, path):
        _tcheck(lib().kctc_graph_write_text(self.h, str(path).encode()), "graph_write_text")

    def info(self):
        """dict(num_states, num_arcs, eps_depth, max_ilabel, max_col)"""
        s, d, il, c, a = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
        _tcheck(lib().kctc_graph_info(self.h, ctypes.byref(s), ctypes.byref(a), ctypes.byref(d), ctypes.byref(il),
                                      ctypes.byref(c)), "graph_info")
        return dict(num_states=s.value, num_arcs=a.value, eps_depth=d.value, max_ilabel=il.value, max_col=c.value)

    @property
    def num_states(self):
        return self.info()["num_states"]

    @property
    def num_arcs(self):
        return self.info()["num_arcs"]

    @property
    def eps_depth(self):
        return self.info()["eps_depth"]

    def arrays(self):
        """The stored graph: dict(start, final_costs, src, ilabel, olabel, weight,
        dst), the arcs in arc-id order."""
        i = self.info()
        S, NA = i["num_states"], i["num_arcs"]
        start = ctypes.c_int()
        fin = np.empty(S, np.float32)
        a = {k: np.empty(NA, np.int32) for k in ("src", "ilabel", "olabel", "dst")}
        w = np.empty(NA, np.float32)
        _tcheck(lib().kctc_graph_get(self.h, ctypes.byref(start), fin.ctypes.data, a["src"].ctypes.data,
                                     a["ilabel"].ctypes.data, a["olabel"].ctypes.data, w.ctypes.data,
                                     a["dst"].ctypes.data), "graph_get")
        return dict(start=start.value, final_costs=fin, weight=w, **a)

    def close(self):
        if self.h is not None:
            lib().kctc_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ctc_token_graph(A, blank=0):
    """The lexicon-free CTC label loop over A columns as a Graph: state 0 (start)
    is "after a blank or nothing", one state per label is "inside that label".
    ilabel = column + 1; entering a label emits it (olabel = the column when
    blank is 0, which is the project's symbol id, else column + 1); repeating
    it and blank emit nothing.  Every state is final.  Its best path is the
    collapsed frame-wise argmax."""
    if A < 2 or not 0 <= blank < A:
        raise KctcError("ctc_token_graph: need A >= 2 and a blank inside [0, A)")
    labels = [c for c in range(A) if c != blank]
    state = {c: 1 + k for k, c in enumerate(labels)}
    src, il, ol, dst = [], [], [], []
    for s in range(A):
        src.append(s); il.append(blank + 1); ol.append(0); dst.append(0)
        for c in labels:
            same = state[c] == s
            src.append(s); il.append(c + 1); ol.append(0 if same else (c if blank == 0 else c + 1)); dst.append(state[c])
    return Graph(np.zeros(A, np.float32), src, il, ol, np.zeros(len(src), np.float32), dst)


def ctc_lexicon_graph(lexicon, A, word_costs=None, blank=0):
    """A pronunciation trie composed with the CTC topology, as a Graph.
    lexicon: list of (word id >= 1, [columns != blank]) pronunciations;
    word_costs: None or one cost per entry.  It accepts exactly the frame label
    sequences whose CTC collapse is a concatenation of pronunciations.  Every
    trie node v has a state L(v) "inside v's label" (loops on that label) and a
    state B(v) "behind a blank inside the word".  A word ends on an epsilon arc
    (olabel = the word id, weight = its cost) from L(v) to the root copy
    R[label of v], which has the root's arcs except the one on that label: a
    word that starts with the label the last one ended on needs a blank first,
    which leads from R[x] to the root R.  R and every R[x] are final."""
    if A < 2 or not 0 <= blank < A:
        raise KctcError("ctc_lexicon_graph: need A >= 2 and a blank inside [0, A)")
    costs = [0.0] * len(lexicon) if word_costs is None else [float(c) for c in word_costs]
    if len(costs) != len(lexicon):
        raise KctcError("ctc_lexicon_graph: one cost per lexicon entry")
    children = [{}]  # trie: node -> {column: node}; node 0 is the root
    label = [-1]
    ends = [[]]
    for k, (word, pron) in enumerate(lexicon):
        if int(word) < 1 or len(pron) == 0 or any(not 0 <= c < A or c == blank for c in pron):
            raise KctcError(f"ctc_lexicon_graph: entry {k} needs a word id >= 1 and columns in [0, A) other than blank")
        v = 0
        for c in pron:
            c = int(c)
            if c not in children[v]:
                children[v][c] = len(children)
                children.append({})
                label.append(c)
                ends.append([])
            v = children[v][c]
        ends[v].append((int(word), costs[k]))
    nodes = len(children)
    used = sorted({label[v] for v in range(1, nodes) if ends[v]})
    root_copy = {x: 1 + k for k, x in enumerate(used)}  # R[x]; the root R is state 0
    base = 1 + len(used)
    L = lambda v: base + 2 * (v - 1)
    B = lambda v: base + 2 * (v - 1) + 1
    src, il, ol, w, dst = [], [], [], [], []

    def arc(s, i, o, c, d):
        src.append(s); il.append(i); ol.append(o); w.append(c); dst.append(d)

    arc(0, blank + 1, 0, 0.0, 0)
    for c, v in sorted(children[0].items()):
        arc(0, c + 1, 0, 0.0, L(v))
    for x, r in root_copy.items():
        arc(r, blank + 1, 0, 0.0, 0)
        for c, v in sorted(children[0].items()):
            if c != x:
                arc(r, c + 1, 0, 0.0, L(v))
    for v in range(1, nodes):
        arc(L(v), label[v] + 1, 0, 0.0, L(v))
        arc(L(v), blank + 1, 0, 0.0, B(v))
        arc(B(v), blank + 1, 0, 0.0, B(v))
        for c, u in sorted(children[v].items()):
            if c != label[v]:
                arc(L(v), c + 1, 0, 0.0, L(u))
            arc(B(v), c + 1, 0, 0.0, L(u))
        for word, cost in ends[v]:
            arc(L(v), 0, word, cost, root_copy[label[v]])
    S = base + 2 * (nodes - 1)
    fin = np.full(S, np.inf, np.float32)
    fin[:base] = 0.0
    return Graph(fin, src, il, ol, w, dst)


def wfst_decode_workspace_size(graph, input_lengths, max_active, pool_tokens):
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    out = ctypes.c_size_t()
    st = lib().kctc_wfst_decode_workspace_size(graph.h, il.ctypes.data, len(il), int(max_active), int(pool_tokens),
                                               ctypes.byref(out))
    if st != 0:
        raise CtcError(st, "kctc_wfst_decode_workspace_size")
    return out.value


def wfst_decode_counts(workspace, N, stream=None):
    """Per utterance of the last wfst_decode on `workspace`: (sum over the
    frames of |E_t|, sum over t = 0..T of |Q_t|) as two np.int64 [N]
    (kctc_wfst_decode_counts; synchronises the stream)."""
    e, q = np.zeros(N, np.int64), np.zeros(N, np.int64)
    _tcheck(lib().kctc_wfst_decode_counts(workspace.data_ptr(), int(N), _stream_handle(stream), e.ctypes.data,
                                          q.ctypes.data), "wfst_decode_counts")
    return e, q


def wfst_default_pool_tokens(graph, max_T, max_active):
    """Back-pointer records per utterance when the caller names none: room for
    min(num_states, 4 * max_active + 4096) tokens in every one of the max_T + 1
    token sets (a token set holds what max_active tokens reach over one
    emitting arc and the epsilon arcs behind it)."""
    return (int(max_T) + 1) * min(graph.num_states, 4 * int(max_active) + 4096)


def wfst_decode(loglikes, input_lengths, graph, beam=15.0, max_active=7000, acoustic_scale=1.0, pool_tokens=None,
                stream=None, workspace=None):
    """Viterbi token passing over `graph` (kctc_wfst_decode_async) for a torch
    CUDA tensor loglikes [T, N, A] (float32, time-major; rows behind an
    utterance's length are never read).  Returns (words: list of N int lists,
    the non-zero olabels of the best path; ali np.int32 [T, N]: the ilabel of
    every frame, -1 behind the utterance; scores np.float64 [N]: graph +
    acoustic + final cost; status np.int32 [N]: 1 a final state was reached,
    0 none was (best token, no final cost), -1 no token survived, -2 more than
    pool_tokens back-pointer records; a negative status gives no words, ali
    -1 and score +inf)."""
    import torch
    assert loglikes.is_cuda and loglikes.dtype == torch.float32 and loglikes.is_contiguous()
    T, N, A = loglikes.shape
    il = np.ascontiguousarray(input_lengths, dtype=np.int32)
    if len(il) != N or (N and int(il.max()) > T):
        raise CtcError(2, "wfst_decode")
    if loglikes.numel() == 0:  # only utterances without frames: the call still wants a device pointer
        loglikes = torch.zeros(1, dtype=torch.float32, device=loglikes.device)
    max_t = int(il.max()) if N else 0
    if pool_tokens is None:
        pool_tokens = wfst_default_pool_tokens(graph, max_t, max_active)
    if workspace is None:
        workspace = torch.empty(wfst_decode_workspace_size(graph, il, max_active, pool_tokens), dtype=torch.uint8,
                                device=loglikes.device)
    row = max_t + (max_t + 1) * graph.eps_depth
    words = torch.empty((N, max(row, 1)), dtype=torch.int32, device=loglikes.device)
    words_len = torch.empty(N, dtype=torch.int32, device=loglikes.device)
    ali = torch.empty((max(max_t, 1), N), dtype=torch.int32, device=loglikes.device)
    scores = torch.empty(N, dtype=torch.float64, device=loglikes.device)
    status = torch.empty(N, dtype=torch.int32, device=loglikes.device)
    st = lib().kctc_wfst_decode_async(graph.h, loglikes.data_ptr(), il.ctypes.data, A, N, float(acoustic_scale),
                                      float(beam), int(max_active), int(pool_tokens), words.data_ptr(),
                                      words_len.data_ptr(), ali.data_ptr(), scores.data_ptr(), status.data_ptr(),
                                      workspace.data_ptr(), _stream_handle(stream))
    if st != 0:
        raise CtcError(st, "kctc_wfst_decode_async")
    if stream is not None:
        torch.cuda.synchronize()  # the copies below run on the current stream
    words, words_len = words.cpu().numpy(), words_len.cpu().numpy()
    ali_out = np.full((T, N), -1, np.int32)
    ali_out[:max_t] = ali.cpu().numpy()[:max_t]
    return ([words[n, :int(words_len[n])].tolist() for n in range(N)], ali_out, scores.cpu().numpy(),
            status.cpu().numpy())


def read_int_vector_ark(path):
    """Binary Kaldi archive of Int32Vector (what Nnet.align_egs writes and
    ali-to-post reads) -> dict key -> np.int32 array, in archive order."""
    if str(path).startswith("ark:"):
        path = str(path)[4:]
    out = {}
    with open(path, "rb") as f:
        data = f.read()
    p = 0
    while p < len(data):
        sp = data.index(b" ", p)
        key = data[p:sp].decode()
        if data[sp + 1:sp + 3] != b"\0B" or data[sp + 3] != 4:
            raise KctcError(f"{path}: entry {key!r} is not a binary Int32Vector")
        n = int(np.frombuffer(data, np.int32, 1, sp + 4)[0])
        out[key] = np.frombuffer(data, np.int32, n, sp + 8).copy()
        p = sp + 8 + 4 * n
    return out


class RnnError(RuntimeError):
    pass


def _krnn_check(st, where):
    if st != 0:
        raise RnnError(f"{where}: {lib().krnnGetStatusString(st).decode()} ({st})")


class Rnn:
    """Thin Python view of the cuDNN-shaped RNN ABI (include/kaldi_rnn.h).

    Mirrors how CuDNNRecurrentComponent drives cudnn-recurrent.h: buffers are
    owned by the caller (torch CUDA tensors here), every call is stream-ordered.
    """
    RELU, TANH, LSTM, GRU = 0, 1, 2, 3

    def __init__(self, mode, input_dim, hidden_dim, num_layers=1, bidirectional=True):
        self.mode, self.D, self.H, self.L = mode, input_dim, hidden_dim, num_layers
        self.dirs = 2 if bidirectional else 1
        h = ctypes.c_void_p()
        _krnn_check(lib().krnnCreate(ctypes.byref(h), mode, input_dim, hidden_dim, num_layers,
                                     1 if bidirectional else 0), "krnnCreate")
        self.h = h

    def set_precision(self, prec):
        """krnnSetPrecision: 0 fp32-class, 1 (or "bf16") bf16 operands."""
        _krnn_check(lib().krnnSetPrecision(self.h, 1 if prec in (1, "bf16") else 0), "krnnSetPrecision")

    def __del__(self):
        try:
            if self.h:
                lib().krnnDestroy(self.h)
        except Exception:
            pass

    @property
    def num_params(self):
        return lib().krnnGetParamsSize(self.h) // 4

    def lin_offset(self, pseudo_layer, lin_id, is_bias):
        dims = (ctypes.c_int * 2)()
        off = lib().krnnGetLinLayerOffset(self.h, pseudo_layer, lin_id, is_bias, dims)
        if off < 0:
            raise RnnError("bad lin layer")
        return off, (dims[0], dims[1])

    def sizes(self, T, N):
        return (lib().krnnGetWorkspaceSize(self.h, T, N), lib().krnnGetTrainingReserveSize(self.h, T, N))

    def forward_training(self, x, w, y, workspace, reserve, stream=None):
        T, N = x.shape[0], x.shape[1]
        _krnn_check(lib().krnnForwardTraining(self.h, _stream_handle(stream), T, N, _ptr(x), _ptr(w),
                                              _ptr(y), _ptr(workspace), workspace.numel(),
                                              _ptr(reserve), reserve.numel()), "krnnForwardTraining")

    def forward_inference(self, x, w, y, workspace, stream=None):
        T, N = x.shape[0], x.shape[1]
        _krnn_check(lib().krnnForwardInference(self.h, _stream_handle(stream), T, N, _ptr(x), _ptr(w),
                                               _ptr(y), _ptr(workspace), workspace.numel()),
                    "krnnForwardInference")

    def seq_workspace_size(self, T, N):
        return lib().krnnGetInferenceSeqWorkspaceSize(self.h, T, N)

    def forward_inference_seq(self, x, seq_lengths, w, y, workspace, stream=None):
        """krnnForwardInferenceSeq: x [T, N, D] holds N sequences of (host)
        lengths seq_lengths[n] in [1, T]; y[:len_n, n] is what sequence n gets
        alone, y[len_n:, n] is 0.  workspace: seq_workspace_size(T, N) bytes."""
        T, N = x.shape[0], x.shape[1]
        lens = np.ascontiguousarray(seq_lengths, dtype=np.int32)
        if lens.shape != (N,):
            raise RnnError(f"seq_lengths has shape {lens.shape}, expected ({N},)")
        _krnn_check(lib().krnnForwardInferenceSeq(self.h, _stream_handle(stream), T, N, lens.ctypes.data, _ptr(x),
                                                  _ptr(w), _ptr(y), _ptr(workspace), workspace.numel()),
                    "krnnForwardInferenceSeq")

    def backward_data(self, y, dy, w, dx, workspace, reserve, stream=None):
        T, N = y.shape[0], y.shape[1]
        _krnn_check(lib().krnnBackwardData(self.h, _stream_handle(stream), T, N, _ptr(y), _ptr(dy),
                                           _ptr(w), _ptr(dx), _ptr(workspace), workspace.numel(),
                                           _ptr(reserve), reserve.numel()), "krnnBackwardData")

    def backward_weights(self, x, y, dw, workspace, reserve, stream=None):
        T, N = x.shape[0], x.shape[1]
        _krnn_check(lib().krnnBackwardWeights(self.h, _stream_handle(stream), T, N, _ptr(x), _ptr(y),
                                              _ptr(workspace), workspace.numel(), _ptr(dw),
                                              _ptr(reserve), reserve.numel()), "krnnBackwardWeights")

    def seq_train_sizes(self, T, N):
        """(workspace bytes, reserve bytes) of the length-aware training calls."""
        return (lib().krnnGetTrainingSeqWorkspaceSize(self.h, T, N), lib().krnnGetTrainingSeqReserveSize(self.h, T, N))

    def _seq_lens(self, seq_lengths, N):
        lens = np.ascontiguousarray(seq_lengths, dtype=np.int32)
        if lens.shape != (N,):
            raise RnnError(f"seq_lengths has shape {lens.shape}, expected ({N},)")
        return lens

    def forward_training_seq(self, x, seq_lengths, w, y, workspace, reserve, stream=None):
        """krnnForwardTrainingSeq: as forward_inference_seq, keeping in
        `reserve` what backward_data_seq / backward_weights_seq need
        (workspace, reserve: seq_train_sizes(T, N) bytes; the same
        seq_lengths go to all three calls)."""
        T, N = x.shape[0], x.shape[1]
        lens = self._seq_lens(seq_lengths, N)
        _krnn_check(lib().krnnForwardTrainingSeq(self.h, _stream_handle(stream), T, N, lens.ctypes.data, _ptr(x),
                                                 _ptr(w), _ptr(y), _ptr(workspace), workspace.numel(),
                                                 _ptr(reserve), reserve.numel()), "krnnForwardTrainingSeq")

    def backward_data_seq(self, y, dy, seq_lengths, w, dx, workspace, reserve, stream=None):
        """krnnBackwardDataSeq: dx[:len_n, n] is the input gradient sequence n
        gets alone, dx[len_n:, n] is 0; rows dy[len_n:, n] do not matter."""
        T, N = y.shape[0], y.shape[1]
        lens = self._seq_lens(seq_lengths, N)
        _krnn_check(lib().krnnBackwardDataSeq(self.h, _stream_handle(stream), T, N, lens.ctypes.data, _ptr(y),
                                              _ptr(dy), _ptr(w), _ptr(dx), _ptr(workspace), workspace.numel(),
                                              _ptr(reserve), reserve.numel()), "krnnBackwardDataSeq")

    def backward_weights_seq(self, x, y, seq_lengths, dw, workspace, reserve, stream=None):
        """krnnBackwardWeightsSeq: dw += the sum over n of the weight gradient
        of sequence n run alone."""
        T, N = x.shape[0], x.shape[1]
        lens = self._seq_lens(seq_lengths, N)
        _krnn_check(lib().krnnBackwardWeightsSeq(self.h, _stream_handle(stream), T, N, lens.ctypes.data, _ptr(x),
                                                 _ptr(y), _ptr(workspace), workspace.numel(), _ptr(dw),
                                                 _ptr(reserve), reserve.numel()), "krnnBackwardWeightsSeq")

    def device_status(self, stream=None):
        return lib().krnnGetDeviceStatus(self.h, _stream_handle(stream))


def add_mat_mat(C, A, B, transA=False, transB=False, alpha=1.0, beta=0.0, stream=None):
    """C = alpha op(A) op(B) + beta C on 2-D row-major torch CUDA tensors."""
    M, N = C.shape
    K = A.shape[0] if transA else A.shape[1]
    st = lib().kcm_add_mat_mat(_stream_handle(stream), int(transA), int(transB), M, N, K, alpha,
                               _ptr(A), A.stride(0), _ptr(B), B.stride(0), beta, _ptr(C), C.stride(0))
    if st != 0:
        raise KctcError(f"kcm_add_mat_mat failed ({st})")


def add_mat_mat_x3(C, A, B, transA=False, transB=False, alpha=1.0, beta=0.0, stream=None):
    """add_mat_mat on the split-fp16 matrix-core path (kcm_add_mat_mat_x3)."""
    import torch
    M, N = C.shape
    K = A.shape[0] if transA else A.shape[1]
    ws = torch.empty(lib().kcm_add_mat_mat_x3_workspace(M, N, K), dtype=torch.uint8, device=C.device)
    st = lib().kcm_add_mat_mat_x3(_stream_handle(stream), int(transA), int(transB), M, N, K, alpha,
                                  _ptr(A), A.stride(0), _ptr(B), B.stride(0), beta, _ptr(C), C.stride(0),
                                  _ptr(ws))
    if st != 0:
        raise KctcError(f"kcm_add_mat_mat_x3 failed ({st})")


def find_row_max_id(m, stream=None):
    """CuMatrix::FindRowMaxId of a 2-D torch CUDA float32 tensor -> int32
    CUDA tensor (kcm_find_row_max_id: the _find_row_max_id tie rule)."""
    import torch
    assert m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and m.dim() == 2
    ids = torch.empty(m.shape[0], dtype=torch.int32, device=m.device)
    st = lib().kcm_find_row_max_id(_stream_handle(stream), _ptr(m), m.shape[0], m.shape[1], _ptr(ids))
    if st != 0:
        raise KctcError(f"kcm_find_row_max_id failed ({st})")
    return ids


def _f32_dev(*tensors):
    import torch
    for t in tensors:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def clip_gradient_rows(deriv, threshold, num_clipped, stream=None):
    """kcm_clip_gradient_rows in place on a 2-D torch CUDA float32 tensor: rows
    with |row| >= threshold are rescaled to norm threshold, and num_clipped (a
    CUDA int32 tensor of one element) rises by their number."""
    import torch
    _f32_dev(deriv)
    assert deriv.dim() == 2 and num_clipped.is_cuda and num_clipped.dtype == torch.int32 and num_clipped.numel() == 1
    st = lib().kcm_clip_gradient_rows(_stream_handle(stream), _ptr(deriv), deriv.shape[0], deriv.shape[1],
                                      float(threshold), _ptr(num_clipped))
    if st != 0:
        raise KctcError(f"kcm_clip_gradient_rows failed ({st})")


def add_vec_clipped(w, dw, lr, clip, stream=None):
    """w += lr * clamp(dw, -clip, clip) on 1-D torch CUDA float32 tensors of one
    length (clip <= 0: no clamp) (kcm_add_vec_clipped)."""
    _f32_dev(w, dw)
    assert w.dim() == 1 and w.shape == dw.shape
    st = lib().kcm_add_vec_clipped(_stream_handle(stream), _ptr(w), _ptr(dw), w.numel(), float(lr), float(clip))
    if st != 0:
        raise KctcError(f"kcm_add_vec_clipped failed ({st})")


def add_row_sum_mat(out, X, alpha=1.0, beta=0.0, ws=None, stream=None):
    """CuVector::AddRowSumMat: out [cols] = alpha * (sum of the rows of X
    [rows, cols]) + beta * out; ws: >= 64 * cols floats of device scratch
    (allocated when None) (kcm_add_row_sum_mat)."""
    import torch
    _f32_dev(out, X)
    assert X.dim() == 2 and out.dim() == 1 and out.numel() == X.shape[1]
    if ws is None:
        ws = torch.empty(64 * X.shape[1], dtype=torch.float32, device=X.device)
    _f32_dev(ws)
    assert ws.numel() >= 64 * X.shape[1]
    st = lib().kcm_add_row_sum_mat(_stream_handle(stream), _ptr(X), X.shape[0], X.shape[1], float(alpha),
                                   float(beta), _ptr(out), _ptr(ws))
    if st != 0:
        raise KctcError(f"kcm_add_row_sum_mat failed ({st})")


# ---------------------------------------------------------------------------
# nnet2 trainer (include/kaldi_ctc_train.h)
# ---------------------------------------------------------------------------
def _tcheck(st, where):
    if st != 0:
        raise KctcError(f"{where}: {lib().kctc_last_error().decode()}")


def recipe_config(num_rnn=5, input_dim=40, hidden=512, num_targets=41, rnn_mode=2, bidirectional=True,
                  learning_rate=5e-4, max_seq_length=2000, clipping_threshold=30.0, param_stddev=0.02,
                  bias_stddev=0.2, num_layers=1, norm_based_clipping=True, splice_context=(0,),
                  dropout_proportion=0.0, model_type="google", hidden_dim=1024, lda_matrix=None, lda_dim=None):
    """Component config lines of the CTC recipe, as written by
    egs/wsj/s5/steps/ctc/nnet2/components.py:73-102 (AddRnnLayer ->
    CuDNNRecurrentComponent + ClipGradientComponent) and an output
    AffineComponent; Splice first (make_configs.py: context 0; any sorted
    offsets containing <= 0 and >= 0 values splice frames).
    dropout_proportion > 0 (train.sh --dropout-proportion) puts the generator's
    "DropoutComponent dim=<out> dropout-proportion=<P>" between every RNN and
    its ClipGradientComponent (components.py:67-71,94-95).
    lda_matrix (a path; train.sh --add-lda true) puts the generator's
    "FixedAffineComponent matrix=<path>" after the Splice (make_configs.py:
    262-265); its output dimension is lda_dim, or the spliced dimension when
    that is None (the generator's lda_dim <= 0) -- the matrix file decides, the
    argument only sizes the lines after it.  model_type="FT" (train.sh
    --model-type FT) puts "AffineComponent ... output-dim=<hidden_dim>
    bias-stddev=0", "RectifiedLinearComponent dim=<hidden_dim>" and a
    ClipGradientComponent in front of the first RNN (make_configs.py:268-280,
    components.py:37-55).  The defaults ("google", no LDA) give the text this
    function gave before these arguments existed."""
    if not 0.0 <= dropout_proportion < 1.0:
        raise ValueError("dropout_proportion must be in [0, 1)")
    if model_type not in ("google", "FT"):
        raise ValueError('model_type must be "google" or "FT"')
    ctx = [int(c) for c in splice_context]
    lines = [f"SpliceComponent input-dim={input_dim} context={':'.join(map(str, ctx))}"]
    dim = input_dim * len(ctx)
    clip = (f"clipping-threshold={clipping_threshold} "
            f"norm-based-clipping={'true' if norm_based_clipping else 'false'}")
    if lda_matrix is not None:
        if any(ch.isspace() for ch in str(lda_matrix)):
            raise ValueError("lda_matrix: a config line cannot hold a path with white space")
        lines.append(f"FixedAffineComponent matrix={lda_matrix}")
        if lda_dim is not None and int(lda_dim) > 0:
            dim = int(lda_dim)
    if model_type == "FT":
        if int(hidden_dim) <= 0:
            raise ValueError("hidden_dim must be positive")
        lines.append(f"AffineComponent input-dim={dim} output-dim={int(hidden_dim)} learning-rate={learning_rate} "
                     f"bias-stddev=0")
        dim = int(hidden_dim)
        lines.append(f"RectifiedLinearComponent dim={dim}")
        lines.append(f"ClipGradientComponent dim={dim} {clip}")
    out = hidden * (2 if bidirectional else 1)
    for _ in range(num_rnn):
        lines.append(f"CuDNNRecurrentComponent input-dim={dim} output-dim={hidden} "
                     f"bidirectional={'true' if bidirectional else 'false'} max-seq-length={max_seq_length} "
                     f"learning-rate={learning_rate} rnn-mode={rnn_mode} num-layers={num_layers} "
                     f"param-stddev={param_stddev} bias-stddev={bias_stddev}")
        if dropout_proportion > 0:
            lines.append(f"DropoutComponent dim={out} dropout-proportion={dropout_proportion}")
        lines.append(f"ClipGradientComponent dim={out} clipping-threshold={clipping_threshold} "
                     f"norm-based-clipping={'true' if norm_based_clipping else 'false'}")
        dim = out
    lines.append(f"AffineComponent input-dim={dim} output-dim={num_targets} learning-rate={learning_rate}")
    return "\n".join(lines) + "\n"


_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def write_kaldi_matrix(path, m, binary=False):
    """Write the 2-D array m as one Kaldi float matrix file (Matrix<float>::Write
    behind the stream header of WriteKaldiObject): what "FixedAffineComponent
    matrix=<path>" reads, e.g. an lda.mat whose last column is the bias.  Text
    mode writes 9 significant digits, so either mode gives float32(m) back
    exactly."""
    a = np.ascontiguousarray(m, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("write_kaldi_matrix: a 2-D array is needed")
    with open(path, "wb") as f:
        if binary:
            f.write(b"\0BFM " + b"\x04" + np.int32(a.shape[0]).tobytes() + b"\x04" + np.int32(a.shape[1]).tobytes())
            f.write(a.astype("<f4").tobytes())
        elif a.shape[1] == 0:
            f.write(b" [ ]\n")
        else:
            rows = ["\n  " + " ".join("%.9g" % float(x) for x in r) + " " for r in a]
            f.write((" [" + "".join(rows) + "]\n").encode())


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): counter = four uint32 arrays (or ints) of one
    shape, key = two uint32 ints -> four uint32 arrays of that shape."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(0xffffffff) for x in counter]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    mask, s32 = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c[0]
        p1 = np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0 = (k0 + _PHILOX_W0) & 0xffffffff
        k1 = (k1 + _PHILOX_W1) & 0xffffffff
    return [x.astype(np.uint32) for x in c]


def dropout_mask(seed, stream, draw, rows, dim, proportion, scale=0.0):
    """The multiplier [rows, dim] float32 that a DropoutComponent with stream
    identity (seed, stream) applies in its Propagate number `draw` (0-based)
    and in the Backprop after it -- the documented contract of csrc/dropout.h,
    restated in numpy:

    element i = r * dim + c uses word i % 4 of the Philox4x32-10 block with
    counter (v & 0xffffffff, v >> 32, draw, stream), v = i // 4, and key
    (seed & 0xffffffff, seed >> 32); it is kept iff word >= thr with
    thr = floor(float32(proportion) * 2**32) computed in double; the
    multiplier is low = float32(scale) where dropped and
    high = float32((1 - dp * low) / (1 - dp)) (in double, from the float32 dp
    and low) where kept.  In a network, component c has stream = c and the seed
    of Nnet(seed=...) / Nnet.set_dropout_seed; a standalone Component(line,
    seed) has stream 0."""
    dp, low = np.float32(proportion), np.float32(scale)
    if not 0.0 <= dp < 1.0 or not 0.0 <= low <= 1.0:
        raise ValueError("proportion must be in [0, 1) and scale in [0, 1]")
    n = int(rows) * int(dim)
    thr = np.uint32(int(np.floor(float(dp) * 4294967296.0)))
    high = np.float32((1.0 - float(dp) * float(low)) / (1.0 - float(dp)))
    v = np.arange((n + 3) // 4, dtype=np.uint64)
    seed = int(seed) & 0xffffffffffffffff
    words = philox4x32_10((v & np.uint64(0xffffffff), v >> np.uint64(32), int(draw) & 0xffffffff,
                           int(stream) & 0xffffffff), (seed & 0xffffffff, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    return np.where(w >= thr, high, low).astype(np.float32).reshape(int(rows), int(dim))


class Nnet:
    """nnet2 CTC model on one GPU (the C++ mirror of Nnet + NnetCtcUpdater)."""

    def __init__(self, config=None, seed=0, device=0, _handle=None):
        if _handle is not None:
            self.h = _handle
            return
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_nnet_create(ctypes.byref(h), config.encode(), seed, device), "kctc_nnet_create")
        self.h = h

    @classmethod
    def read(cls, path, device=0):
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_nnet_read(ctypes.byref(h), str(path).encode(), device), "kctc_nnet_read")
        return cls(_handle=h)

    def write(self, path, binary=False):
        """Nnet::Write (nnet-nnet.cc:170-183), Kaldi text or binary mode."""
        _tcheck(lib().kctc_nnet_write_kaldi(self.h, str(path).encode(), int(binary)), "kctc_nnet_write_kaldi")

    @classmethod
    def read_am(cls, path, device=0):
        """nnet2-ctc model file: CtcTransitionModel (kept opaque) + AmNnet (Nnet + priors)."""
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_am_nnet_read(ctypes.byref(h), str(path).encode(), device), "kctc_am_nnet_read")
        return cls(_handle=h)

    def write_am(self, path, binary=True):
        _tcheck(lib().kctc_am_nnet_write(self.h, str(path).encode(), int(binary)), "kctc_am_nnet_write")

    @property
    def priors(self):
        n = lib().kctc_am_nnet_num_priors(self.h)
        out = np.zeros(n, dtype=np.float32)
        _tcheck(lib().kctc_am_nnet_get_priors(self.h, out.ctypes.data, n), "kctc_am_nnet_get_priors")
        return out

    def set_priors(self, priors):
        p = np.ascontiguousarray(priors, dtype=np.float32)
        _tcheck(lib().kctc_am_nnet_set_priors(self.h, p.ctypes.data, p.size), "kctc_am_nnet_set_priors")

    def close(self):
        if getattr(self, "h", None):
            lib().kctc_nnet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_components(self):
        return lib().kctc_nnet_num_components(self.h)

    def info(self, c):
        buf = ctypes.create_string_buffer(1024)
        _tcheck(lib().kctc_nnet_component_info(self.h, c, buf, 1024), "component_info")
        return buf.value.decode()

    def num_params(self, c):
        return lib().kctc_nnet_num_params(self.h, c)

    def get_params(self, c):
        out = np.zeros(self.num_params(c), np.float32)
        _tcheck(lib().kctc_nnet_get_params(self.h, c, out.ctypes.data, out.size), "get_params")
        return out

    def get_grad(self, c):
        """The gradient component c's last update used (before its clip)."""
        out = np.zeros(self.num_params(c), np.float32)
        _tcheck(lib().kctc_nnet_get_grad(self.h, c, out.ctypes.data, out.size), "get_grad")
        return out

    def set_params(self, c, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        _tcheck(lib().kctc_nnet_set_params(self.h, c, a.ctypes.data, a.size), "set_params")

    def set_learning_rate(self, lr):
        _tcheck(lib().kctc_nnet_set_learning_rate(self.h, lr), "set_learning_rate")

    def clip_stats(self, c):
        a, b = ctypes.c_double(), ctypes.c_double()
        _tcheck(lib().kctc_nnet_clip_stats(self.h, c, ctypes.byref(a), ctypes.byref(b)), "clip_stats")
        return a.value, b.value

    def srand(self, seed):
        """srand(seed) of the trainer's rand() stream (nnet2-ctc-train-simple --srand)."""
        _tcheck(lib().kctc_nnet_srand(self.h, int(seed)), "srand")

    @property
    def rand_calls(self):
        n = ctypes.c_long()
        _tcheck(lib().kctc_nnet_rand_calls(self.h, ctypes.byref(n)), "rand_calls")
        return n.value

    def last_best_path(self, T, N):
        """FindRowMaxId ids [T*N] of the last finished minibatch."""
        out = np.empty(T * N, np.int32)
        _tcheck(lib().kctc_nnet_last_best_path(self.h, out.ctypes.data, out.size), "last_best_path")
        return out

    def last_costs(self, N):
        """Per-utterance CTC costs [N] of the last finished minibatch."""
        out = np.empty(N, np.float64)
        _tcheck(lib().kctc_nnet_last_costs(self.h, out.ctypes.data, N), "last_costs")
        return out

    def last_output(self, T, N, A):
        """Network output [T*N, A] of the last minibatch (host copy)."""
        out = np.empty((T * N, A), np.float32)
        _tcheck(lib().kctc_nnet_last_output(self.h, out.ctypes.data, out.size), "last_output")
        return out

    def _check_feats(self, feats, T, N):
        """feats must hold the FormatNnetInput rows of this network's context:
        T*N*(1 + left + right) rows of input_dim (the C ABI reads exactly that)."""
        l, r = self.context
        rows = T * N * (1 + l + r)
        if feats.dim() != 2 or feats.shape[0] != rows:
            raise KctcError(f"feats has shape {tuple(feats.shape)}; this network (context -{l}..+{r}) reads "
                            f"[T*N*{1 + l + r} = {rows}, input_dim] rows")
        if not feats.is_contiguous():
            raise KctcError("feats must be contiguous")

    def _step(self, fn, feats, T, N, num_frames, flat_labels, label_lengths):
        self._check_feats(feats, T, N)
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        fl = np.ascontiguousarray(flat_labels, dtype=np.int32)
        if fl.size == 0:
            fl = np.zeros(1, np.int32)
        ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
        o, a, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _tcheck(fn(self.h, _ptr(feats), T, N, nf.ctypes.data, fl.ctypes.data, ll.ctypes.data,
                   ctypes.byref(o), ctypes.byref(a), ctypes.byref(w)), fn.__name__)
        return o.value, a.value, w.value

    @property
    def context(self):
        """(left, right) context of the network (kctc_nnet_context); the input
        of a minibatch has (1 + left + right) rows per output frame."""
        l, r = ctypes.c_int(), ctypes.c_int()
        _tcheck(lib().kctc_nnet_context(self.h, ctypes.byref(l), ctypes.byref(r)), "context")
        return l.value, r.value

    def train_step(self, feats, T, N, num_frames, flat_labels, label_lengths):
        """DoBackprop on one minibatch; feats: device [T*N*num_splice, D] (the
        FormatNnetInput layout, num_splice = 1 + left + right of `context`).
        -> (objf, accuracy, weight)"""
        return self._step(lib().kctc_nnet_train_step, feats, T, N, num_frames, flat_labels, label_lengths)

    def train_step_async(self, feats, T, N, num_frames, flat_labels, label_lengths):
        """Queue a training step (feats must stay alive until its stats come
        back); returns the stats of the minibatch queued before the previous
        one once two are in flight, else None (kctc_nnet_train_step_async).
        feats: device [T*N*num_splice, D] as for train_step."""
        self._check_feats(feats, T, N)
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        fl = np.ascontiguousarray(flat_labels, dtype=np.int32)
        if fl.size == 0:
            fl = np.zeros(1, np.int32)
        ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
        h, o, a, w = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _tcheck(lib().kctc_nnet_train_step_async(self.h, _ptr(feats), T, N, nf.ctypes.data, fl.ctypes.data,
                                                 ll.ctypes.data, ctypes.byref(h), ctypes.byref(o),
                                                 ctypes.byref(a), ctypes.byref(w)), "train_step_async")
        return (o.value, a.value, w.value) if h.value else None

    def train_flush(self):
        """Stats of the queued minibatches, oldest first (kctc_nnet_train_flush)."""
        out = []
        while True:
            h, o, a, w = ctypes.c_int(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            _tcheck(lib().kctc_nnet_train_flush(self.h, ctypes.byref(h), ctypes.byref(o), ctypes.byref(a),
                                                ctypes.byref(w)), "train_flush")
            if not h.value:
                return out
            out.append((o.value, a.value, w.value))

    def compute_objf(self, feats, T, N, num_frames, flat_labels, label_lengths):
        """ComputeNnetObjf (no update); feats as for train_step."""
        return self._step(lib().kctc_nnet_compute_objf, feats, T, N, num_frames, flat_labels, label_lengths)

    @property
    def stream(self):
        return lib().kctc_nnet_stream(self.h)

    def set_profiling(self, on):
        _tcheck(lib().kctc_nnet_set_profiling(self.h, int(on)), "set_profiling")

    def profile(self, family):
        ms, n = ctypes.c_double(), ctypes.c_int()
        _tcheck(lib().kctc_nnet_profile(self.h, family.encode(), ctypes.byref(ms), ctypes.byref(n)), "profile")
        return ms.value, n.value

    def propagate(self, feats, T, N, out=None):
        """NnetComputation: network output [T*N, output_dim] (torch CUDA tensor)
        of feats [T*N*num_splice, D] (FormatNnetInput layout)."""
        import torch
        self._check_feats(feats, T, N)
        A = self.output_dim
        if out is None:
            out = torch.empty((T * N, A), dtype=torch.float32, device=feats.device)
        _tcheck(lib().kctc_nnet_propagate(self.h, _ptr(feats), T, N, _ptr(out), out.numel()), "propagate")
        return out

    def decodable(self, feats, T, prob_scale=1.0, blank_threshold=1.0):
        """CtcDecodableAmNnet of one utterance feats [T, D] (plain rows; padded
        for the network's context as pad_input = true) -> np [kept, A]."""
        if feats.dim() != 2 or feats.shape[0] != T or not feats.is_contiguous():
            raise KctcError(f"feats must be a contiguous [T={T}, input_dim] tensor, got {tuple(feats.shape)}")
        A = self.output_dim
        out = np.empty((T, A), np.float32)
        k = ctypes.c_int()
        _tcheck(lib().kctc_am_nnet_decodable(self.h, _ptr(feats), T, prob_scale, blank_threshold, out.ctypes.data,
                                             ctypes.byref(k)), "am_nnet_decodable")
        return out[:k.value].copy()

    @property
    def output_dim(self):
        return int(self.info(self.num_components - 1).split("output-dim=")[1].split(",")[0])

    @staticmethod
    def _pad_batch(group):
        """[T_n, D] CUDA tensors -> (time-major [T_max*N, D] tensor, T_max, lengths)."""
        import torch
        for f in group:
            if f.dim() != 2 or f.shape[0] < 1 or f.shape[1] != group[0].shape[1]:
                raise KctcError(f"every utterance must be a [T >= 1, input_dim] tensor, got {tuple(f.shape)}")
        nf = np.array([f.shape[0] for f in group], np.int32)
        padded = torch.nn.utils.rnn.pad_sequence(list(group))  # [T_max, N, D]
        return padded.reshape(-1, padded.shape[2]).contiguous(), int(nf.max()), nf

    def propagate_batch(self, feats_list, batch_size=16):
        """NnetComputation of utterances of different lengths, batch_size (<= 64)
        at a time as one variable-length batch (kctc_nnet_propagate_seq): a list,
        in input order, of [T_n, output_dim] CUDA tensors, each what
        propagate(feats, T_n, 1) gives for that utterance alone.  For networks
        without frame context (their input layout is that of propagate)."""
        import torch
        if self.context != (0, 0):
            raise KctcError("propagate_batch takes plain feature rows: the network must have no frame context")
        A, outs = self.output_dim, []
        for g0 in range(0, len(feats_list), batch_size):
            group = feats_list[g0:g0 + batch_size]
            feats, T, nf = self._pad_batch(group)
            N = len(group)
            out = torch.empty((T * N, A), dtype=torch.float32, device=feats.device)
            _tcheck(lib().kctc_nnet_propagate_seq(self.h, _ptr(feats), T, N, nf.ctypes.data, _ptr(out), out.numel()),
                    "propagate_seq")
            out = out.reshape(T, N, A)
            outs += [out[:nf[n], n].contiguous() for n in range(N)]
        return outs

    def decodable_batch(self, feats_list, prob_scale=1.0, blank_threshold=1.0, batch_size=16):
        """decodable() of any number of utterances ([T_n, D] CUDA tensors, plain
        rows), run batch_size (<= 64) at a time as variable-length batches
        (kctc_am_nnet_decodable_batch) -> list of np [kept_n, A] in input order."""
        A, outs = self.output_dim, []
        for g0 in range(0, len(feats_list), batch_size):
            group = feats_list[g0:g0 + batch_size]
            feats, T, nf = self._pad_batch(group)
            N = len(group)
            out = np.empty((int(nf.sum()), A), np.float32)
            rows = np.zeros(N, np.int32)
            _tcheck(lib().kctc_am_nnet_decodable_batch(self.h, _ptr(feats), T, N, nf.ctypes.data, prob_scale,
                                                       blank_threshold, out.ctypes.data, rows.ctypes.data),
                    "am_nnet_decodable_batch")
            ends = np.cumsum(rows)
            outs += [out[e - r:e].copy() for e, r in zip(ends, rows)]
        return outs

    def sum_posteriors(self, rspecifier, minibatch_size=16):
        """nnet-ctc-compute-from-egs | matrix-sum-rows | vector-sum over an egs
        archive -> (sum [output_dim] float64, frames, num_egs)."""
        A = self.output_dim
        s = np.zeros(A, np.float64)
        fr, ne = ctypes.c_long(), ctypes.c_long()
        _tcheck(lib().kctc_nnet_sum_posteriors(self.h, str(rspecifier).encode(), minibatch_size, s.ctypes.data, A,
                                               ctypes.byref(fr), ctypes.byref(ne)), "sum_posteriors")
        return s, fr.value, ne.value

    def align(self, feats, T, N, num_frames, flat_labels, label_lengths):
        """CTC forced alignment of a variable-length batch (kctc_nnet_align;
        feats as for train_step, N <= 64, every utterance as if run alone) ->
        (ali np.int32 [T, N]: the symbol of every frame, blank 0 included, -1
        for t >= num_frames[n] and for an utterance whose labels do not fit;
        scores np.float64 [N]: the log-probability of each path)."""
        self._check_feats(feats, T, N)
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        fl = np.ascontiguousarray(flat_labels, dtype=np.int32)
        if fl.size == 0:
            fl = np.zeros(1, np.int32)
        ll = np.ascontiguousarray(label_lengths, dtype=np.int32)
        if len(nf) != N or len(ll) != N or fl.size < int(ll.sum()):
            raise KctcError("align: num_frames / label_lengths must have N entries and flat_labels their sum")
        ali = np.empty((T, N), np.int32)
        scores = np.empty(N, np.float64)
        _tcheck(lib().kctc_nnet_align(self.h, _ptr(feats), T, N, nf.ctypes.data, fl.ctypes.data, ll.ctypes.data,
                                      ali.ctypes.data, scores.ctypes.data), "nnet_align")
        return ali, scores

    def align_egs(self, rspecifier, wspecifier, minibatch_size=16):
        """Aligns every example of an egs archive to its own labels and writes
        the Int32Vector table `wspecifier` (kctc_nnet_align_egs) ->
        dict(num_done, num_infeasible, tot_score, tot_frames)."""
        nd, ni, fr, sc = ctypes.c_long(), ctypes.c_long(), ctypes.c_long(), ctypes.c_double()
        _tcheck(lib().kctc_nnet_align_egs(self.h, str(rspecifier).encode(), str(wspecifier).encode(),
                                          int(minibatch_size), ctypes.byref(nd), ctypes.byref(ni), ctypes.byref(sc),
                                          ctypes.byref(fr)), "nnet_align_egs")
        return dict(num_done=nd.value, num_infeasible=ni.value, tot_score=sc.value, tot_frames=fr.value)

    def decode(self, feats, T, N, num_frames, beam=16, symbols=40):
        """Lexicon-free CTC prefix beam search of a variable-length batch
        (kctc_nnet_decode; feats as for train_step, N <= 64, every utterance as
        if run alone) -> (hyps: list of N int lists of symbol ids, blank 0
        never among them; scores np.float64 [N])."""
        self._check_feats(feats, T, N)
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        if len(nf) != N:
            raise KctcError("decode: num_frames must have N entries")
        hyp = np.empty((N, T), np.int32)
        hyp_len = np.empty(N, np.int32)
        scores = np.empty(N, np.float64)
        _tcheck(lib().kctc_nnet_decode(self.h, _ptr(feats), T, N, nf.ctypes.data, int(beam), int(symbols),
                                       hyp.ctypes.data, hyp_len.ctypes.data, scores.ctypes.data), "nnet_decode")
        return [hyp[n, :hyp_len[n]].tolist() for n in range(N)], scores

    def decode_egs(self, rspecifier, wspecifier, minibatch_size=16, beam=16, symbols=40):
        """Decodes every example of an egs archive and writes the hypotheses as
        the Int32Vector table `wspecifier` (kctc_nnet_decode_egs) ->
        (num_utts, num_labels, edit_distance): 1 - edit_distance / num_labels
        compares with compute_prob's best-path accuracy."""
        nu, nl, ed = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        _tcheck(lib().kctc_nnet_decode_egs(self.h, str(rspecifier).encode(), str(wspecifier).encode(),
                                           int(minibatch_size), int(beam), int(symbols), ctypes.byref(nu),
                                           ctypes.byref(nl), ctypes.byref(ed)), "nnet_decode_egs")
        return nu.value, nl.value, ed.value

    def decode_graph(self, feats, T, N, num_frames, graph, beam=15.0, max_active=7000, prob_scale=1.0,
                     acoustic_scale=1.0, pool_tokens=None):
        """The best path of nnet2-ctc-latgen-faster for a variable-length batch
        (kctc_nnet_decode_graph; feats as for train_step, N <= 64, every
        utterance as if run alone): the forward, (log(max(p, 1e-10)) - log
        prior) * prob_scale on the device, then wfst_decode over `graph` ->
        (words: list of N int lists, ali np.int32 [T, N], scores np.float64 [N],
        status np.int32 [N]) as wfst_decode returns them."""
        self._check_feats(feats, T, N)
        nf = np.ascontiguousarray(num_frames, dtype=np.int32)
        if len(nf) != N:
            raise KctcError("decode_graph: num_frames must have N entries")
        row = max(T + (T + 1) * graph.eps_depth, 1)
        words = np.empty((N, row), np.int32)
        words_len = np.empty(N, np.int32)
        ali = np.empty((T, N), np.int32)
        scores = np.empty(N, np.float64)
        status = np.empty(N, np.int32)
        _tcheck(lib().kctc_nnet_decode_graph(self.h, graph.h, _ptr(feats), T, N, nf.ctypes.data, prob_scale,
                                             acoustic_scale, beam, int(max_active),
                                             0 if pool_tokens is None else int(pool_tokens), words.ctypes.data, row,
                                             words_len.ctypes.data, ali.ctypes.data, scores.ctypes.data,
                                             status.ctypes.data), "nnet_decode_graph")
        return [words[n, :words_len[n]].tolist() for n in range(N)], ali, scores, status

    def decode_graph_egs(self, rspecifier, words_wspecifier, graph, ali_wspecifier=None, minibatch_size=16,
                         beam=15.0, max_active=7000, prob_scale=1.0, acoustic_scale=1.0, pool_tokens=None):
        """Decodes every example of an egs archive over `graph` and writes the
        words per key as the Int32Vector table `words_wspecifier` (Kaldi's
        words.tra as a table) and, if named, the per-frame ilabels to
        `ali_wspecifier` (kctc_nnet_decode_graph_egs) -> dict(num_done,
        num_final, num_failed, tot_score, tot_frames); utterances with a
        negative status are counted in num_failed and not written."""
        nd, nfin, nfail, fr, sc = ctypes.c_long(), ctypes.c_long(), ctypes.c_long(), ctypes.c_long(), ctypes.c_double()
        _tcheck(lib().kctc_nnet_decode_graph_egs(
            self.h, graph.h, str(rspecifier).encode(), str(words_wspecifier).encode(),
            None if ali_wspecifier is None else str(ali_wspecifier).encode(), int(minibatch_size), prob_scale,
            acoustic_scale, beam, int(max_active), 0 if pool_tokens is None else int(pool_tokens), ctypes.byref(nd),
            ctypes.byref(nfin), ctypes.byref(nfail), ctypes.byref(sc), ctypes.byref(fr)), "nnet_decode_graph_egs")
        return dict(num_done=nd.value, num_final=nfin.value, num_failed=nfail.value, tot_score=sc.value,
                    tot_frames=fr.value)

    def adjust_priors(self, posterior_sum=None, google_prior_const=0.0):
        """nnet-adjust-priors: priors = posterior_sum / its total, or (with
        google_prior_const) all ones with priors[0] = the constant."""
        A = self.output_dim
        if posterior_sum is None:
            if not google_prior_const:
                raise KctcError("adjust_priors needs a posterior sum or google_prior_const")
            s = np.zeros(A, np.float64)
        else:
            s = np.ascontiguousarray(posterior_sum, dtype=np.float64)
            if s.shape != (A,):
                raise KctcError(f"posterior sum has shape {s.shape}, expected ({A},)")
        _tcheck(lib().kctc_am_nnet_adjust_priors(self.h, s.ctypes.data, A, float(google_prior_const)),
                "adjust_priors")

    def insert(self, insert_at, config, seed=0):
        """nnet-insert (--randomize-next-component=false): the components of
        the config lines go before component insert_at (num_components: appended)."""
        _tcheck(lib().kctc_nnet_insert(self.h, int(insert_at), config.encode(), seed), "nnet_insert")

    def compute_prob(self, rspecifier):
        """nnet2-ctc-compute-prob -> dict(num_examples, tot_like, tot_accuracy, tot_weight)."""
        ne, l, a, w = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _tcheck(lib().kctc_nnet_compute_prob(self.h, str(rspecifier).encode(), ctypes.byref(ne), ctypes.byref(l),
                                             ctypes.byref(a), ctypes.byref(w)), "compute_prob")
        return {"num_examples": ne.value, "tot_like": l.value, "tot_accuracy": a.value, "tot_weight": w.value}

    def set_precision(self, prec):
        """0: fp32-class recurrences / gate GEMMs (default); 1 or "bf16": bf16
        operands, fp32 accumulation (kctc_nnet_set_precision)."""
        prec = 1 if prec in (1, "bf16") else 0
        _tcheck(lib().kctc_nnet_set_precision(self.h, prec), "set_precision")

    def set_length_aware(self, on=True):
        """kctc_nnet_set_length_aware: every utterance of a padded minibatch
        trains (and is scored by compute_objf / compute_prob) as if it were
        run alone; the gradient is the sum of the per-utterance gradients.
        Off by default; at most 64 utterances, fp32-class precision only."""
        _tcheck(lib().kctc_nnet_set_length_aware(self.h, 1 if on else 0), "set_length_aware")

    def set_momentum(self, m):
        _tcheck(lib().kctc_nnet_set_momentum(self.h, float(m)), "set_momentum")

    def set_dropout_seed(self, seed):
        """DropoutComponent c draws from stream (seed, c) of dropout_mask, from
        draw 0 again (kctc_nnet_set_dropout_seed)."""
        _tcheck(lib().kctc_nnet_set_dropout_seed(self.h, int(seed) & 0xffffffffffffffff), "set_dropout_seed")

    def remove_dropout(self):
        """nnet-am-copy --remove-dropout=true (Nnet::RemoveDropout) on the live
        network -> the number of components removed."""
        r = ctypes.c_int()
        _tcheck(lib().kctc_nnet_remove_dropout(self.h, ctypes.byref(r)), "remove_dropout")
        return r.value

    def set_dropout_scale(self, scale):
        """Nnet::SetDropoutScale: the dropped elements' multiplier of every DropoutComponent."""
        _tcheck(lib().kctc_nnet_set_dropout_scale(self.h, float(scale)), "set_dropout_scale")

    def train_simple(self, reader, max_minibatches=0):
        """TrainNnetSimple over an EgsReader -> dict(num_egs, tot_weight, tot_objf, tot_accuracy)."""
        ne, w, o, a = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _tcheck(lib().kctc_nnet_train_simple(self.h, reader._h, int(max_minibatches), ctypes.byref(ne),
                                             ctypes.byref(w), ctypes.byref(o), ctypes.byref(a)), "train_simple")
        return {"num_egs": ne.value, "tot_weight": w.value, "tot_objf": o.value, "tot_accuracy": a.value}

    def enable_dp(self, uid, rank, world):
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        _tcheck(lib().kctc_nnet_enable_dp(self.h, buf, rank, world), "enable_dp")

    def set_dp_mode(self, mode):
        """"grad" (sum the gradients every step) or "average" (independent steps,
        average_params() = nnet-am-average over the ranks)."""
        _tcheck(lib().kctc_nnet_set_dp_mode(self.h, {"grad": 0, "average": 1}[mode]), "set_dp_mode")

    def average_params(self):
        _tcheck(lib().kctc_nnet_average_params(self.h), "average_params")

    def enable_dp_host(self, allreduce, world):
        """Gradient exchange over a host transport: allreduce(np.float32 array)
        must sum it in place across the ranks (e.g. gloo)."""
        def cb(buf, n, user):
            allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
        self._dp_cb = _HOST_ALLREDUCE(cb)  # keep the thunk alive
        _tcheck(lib().kctc_nnet_enable_dp_host(self.h, ctypes.cast(self._dp_cb, ctypes.c_void_p), None, world),
                "enable_dp_host")


    def inject_step_error(self, word=1):
        """Test hook: the next minibatch starts with device error word `word`
        (as after a recurrence timeout): its updates are skipped -- on every
        data-parallel rank -- and the step raises."""
        _tcheck(lib().kctc_nnet_inject_step_error(self.h, int(word)), "inject_step_error")

    def get_component(self, c):
        """A copy of component c (Nnet::GetComponent(c).Copy())."""
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_nnet_get_component(self.h, int(c), ctypes.byref(h)), "kctc_nnet_get_component")
        return Component(_handle=h)

    def set_component(self, c, component):
        """Nnet::SetComponent(c, component.Copy())."""
        _tcheck(lib().kctc_nnet_set_component(self.h, int(c), component.h), "kctc_nnet_set_component")

    def scale_params(self, scale, skip_last_layer=False):
        _tcheck(lib().kctc_nnet_scale_params(self.h, float(scale), int(bool(skip_last_layer))), "scale_params")

    def add_params(self, alpha, other, skip_last_layer=False):
        _tcheck(lib().kctc_nnet_add_params(self.h, float(alpha), other.h, int(bool(skip_last_layer))), "add_params")

    def enable_cu_probe(self, blocks, usec):
        """CU-budget probe: every gradient bucket launches a kernel holding
        `blocks` whole CUs for `usec` us on a comm stream (blocks 0: off)."""
        _tcheck(lib().kctc_nnet_enable_cu_probe(self.h, int(blocks), float(usec)), "enable_cu_probe")


_HOST_ALLREDUCE = ctypes.CFUNCTYPE(None, ctypes.POINTER(ctypes.c_float), ctypes.c_long, ctypes.c_void_p)


# ---------------------------------------------------------------------------
# nnet2 Component plug-in point (include/kaldi_nnet2_component.h)
# ---------------------------------------------------------------------------
def _torch_sync():
    """The component ABI runs on its own stream: wait for torch's first."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.current_stream().synchronize()


class Component:
    """One nnet2 component on the GPU, with the reference's member names
    (src/nnet2/nnet-component.h:157-348): Propagate / Backprop / Copy /
    Write / ReadNew and, for UpdatableComponents, SetZero / DotProduct /
    PerturbParams / Scale / Add / Vectorize / UnVectorize.  Matrices are torch
    CUDA float32 tensors in the time-major [T*N(*num_splice), dim] layout;
    Backprop with a to_update component updates it at once, as the
    reference does (a SetZero(True) copy then holds the gradient)."""

    def __init__(self, config_line=None, seed=0, device=0, _handle=None):
        if _handle is not None:
            self.h = _handle
            return
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_component_init(ctypes.byref(h), config_line.encode(), int(seed), int(device)),
                "kctc_component_init")
        self.h = h

    @classmethod
    def ReadNew(cls, path, device=0):
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_component_read(ctypes.byref(h), str(path).encode(), int(device)), "kctc_component_read")
        return cls(_handle=h)

    def Write(self, path, binary=True):
        _tcheck(lib().kctc_component_write(self.h, str(path).encode(), int(bool(binary))), "kctc_component_write")

    def Copy(self):
        h = ctypes.c_void_p()
        _tcheck(lib().kctc_component_copy(self.h, ctypes.byref(h)), "kctc_component_copy")
        return Component(_handle=h)

    def close(self):
        if getattr(self, "h", None):
            lib().kctc_component_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Type(self):
        buf = ctypes.create_string_buffer(256)
        _tcheck(lib().kctc_component_type(self.h, buf, 256), "kctc_component_type")
        return buf.value.decode()

    def Info(self):
        buf = ctypes.create_string_buffer(1024)
        _tcheck(lib().kctc_component_info(self.h, buf, 1024), "kctc_component_info")
        return buf.value.decode()

    def _dims(self):
        i, o = ctypes.c_int(), ctypes.c_int()
        _tcheck(lib().kctc_component_dims(self.h, ctypes.byref(i), ctypes.byref(o)), "kctc_component_dims")
        return i.value, o.value

    def InputDim(self):
        return self._dims()[0]

    def OutputDim(self):
        return self._dims()[1]

    def Context(self):
        buf = (ctypes.c_int * 64)()
        n = ctypes.c_int()
        _tcheck(lib().kctc_component_context(self.h, buf, 64, ctypes.byref(n)), "kctc_component_context")
        return list(buf[:n.value])

    def NumSplice(self):
        ctx = self.Context()
        return ctx[-1] - ctx[0] + 1

    def _needs(self):
        i, o = ctypes.c_int(), ctypes.c_int()
        _tcheck(lib().kctc_component_backprop_needs(self.h, ctypes.byref(i), ctypes.byref(o)), "backprop_needs")
        return bool(i.value), bool(o.value)

    def BackpropNeedsInput(self):
        return self._needs()[0]

    def BackpropNeedsOutput(self):
        return self._needs()[1]

    def IsUpdatable(self):
        return bool(lib().kctc_component_is_updatable(self.h))

    def Propagate(self, T, N, inp, out=None):
        """out [T*N, OutputDim] = component(inp [T*N*NumSplice, InputDim])."""
        import torch
        if out is None:
            out = torch.empty((T * N, self.OutputDim()), dtype=torch.float32, device=inp.device)
        _torch_sync()
        _tcheck(lib().kctc_component_propagate(self.h, T, N, _ptr(inp), inp.numel(), _ptr(out), out.numel()),
                "kctc_component_propagate")
        return out

    def Backprop(self, T, N, in_value, out_value, out_deriv, to_update=None, in_deriv=None):
        """Backprop(in_info, out_info, in_value, out_value, out_deriv, to_update,
        in_deriv); in_deriv (a tensor to fill, or None) is returned."""
        _torch_sync()
        _tcheck(lib().kctc_component_backprop(
            self.h, T, N, _ptr(in_value), 0 if in_value is None else in_value.numel(),
            _ptr(out_value), 0 if out_value is None else out_value.numel(), _ptr(out_deriv), out_deriv.numel(),
            None if to_update is None else to_update.h, _ptr(in_deriv),
            0 if in_deriv is None else in_deriv.numel()), "kctc_component_backprop")
        return in_deriv

    # ---- UpdatableComponent ----
    def NumParameters(self):
        return lib().kctc_component_num_params(self.h)

    def Vectorize(self):
        out = np.zeros(self.NumParameters(), np.float32)
        _tcheck(lib().kctc_component_get_params(self.h, out.ctypes.data, out.size), "kctc_component_get_params")
        return out

    def UnVectorize(self, params):
        a = np.ascontiguousarray(params, dtype=np.float32)
        _tcheck(lib().kctc_component_set_params(self.h, a.ctypes.data, a.size), "kctc_component_set_params")

    def LearningRate(self):
        lr = ctypes.c_float()
        _tcheck(lib().kctc_component_learning_rate(self.h, ctypes.byref(lr)), "kctc_component_learning_rate")
        return lr.value

    def SetLearningRate(self, lr):
        _tcheck(lib().kctc_component_set_learning_rate(self.h, float(lr)), "kctc_component_set_learning_rate")

    def IsGradient(self):
        return bool(lib().kctc_component_is_gradient(self.h))

    def SetZero(self, treat_as_gradient):
        _tcheck(lib().kctc_component_set_zero(self.h, int(bool(treat_as_gradient))), "kctc_component_set_zero")

    def DotProduct(self, other):
        d = ctypes.c_double()
        _tcheck(lib().kctc_component_dot_product(self.h, other.h, ctypes.byref(d)), "kctc_component_dot_product")
        return d.value

    def PerturbParams(self, stddev):
        _tcheck(lib().kctc_component_perturb_params(self.h, float(stddev)), "kctc_component_perturb_params")

    def Scale(self, scale):
        _tcheck(lib().kctc_component_scale(self.h, float(scale)), "kctc_component_scale")

    def Add(self, alpha, other):
        _tcheck(lib().kctc_component_add(self.h, float(alpha), other.h), "kctc_component_add")

    def srand(self, seed):
        _tcheck(lib().kctc_component_srand(self.h, int(seed)), "kctc_component_srand")

    def nonlinear_stats(self):
        """(value_sum, deriv_sum, count) of a RectifiedLinearComponent or a
        SoftmaxComponent: the NonlinearComponent statistics as float64 arrays
        of the component's dimension (zeros for a vector not held yet) and the
        row count.  Other component types raise."""
        dim = self.InputDim()
        v, d = np.zeros(dim, np.float64), np.zeros(dim, np.float64)
        n = ctypes.c_double()
        _tcheck(lib().kctc_component_nonlinear_stats(self.h, v.ctypes.data, d.ctypes.data, dim, ctypes.byref(n)),
                "kctc_component_nonlinear_stats")
        return v, d, n.value


def set_perturb_seed(seed):
    """Seed of PerturbParams' noise stream (kctc_set_perturb_seed)."""
    _tcheck(lib().kctc_set_perturb_seed(int(seed)), "kctc_set_perturb_seed")


def average_models(nnets, weights=None, skip_last_layer=False):
    """nnet-am-average in process: nnets[0] = sum_i w[i] * nnets[i], with the
    weights normalised to sum to one as GetWeights does (nnet-am-average.cc:
    45-53; default 1/len(nnets)) through the components' Scale / Add."""
    arr = (ctypes.c_void_p * len(nnets))(*[n.h.value if hasattr(n.h, "value") else n.h for n in nnets])
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if w is not None and w.size != len(nnets):
        raise ValueError(f"average_models: {w.size} weights for {len(nnets)} models")
    _tcheck(lib().kctc_nnet_average_models(arr, None if w is None else w.ctypes.data, len(nnets),
                                           int(bool(skip_last_layer))), "kctc_nnet_average_models")


def set_cu_partition(part, nparts):
    """Ranks sharing one device: nnets created afterwards in this process run
    on CU share `part` of `nparts` (kctc_set_cu_partition)."""
    _tcheck(lib().kctc_set_cu_partition(int(part), int(nparts)), "kctc_set_cu_partition")


def cu_partition_probe(part, nparts):
    """The distinct CUs (XCC_ID << 16 | HW_ID[15:8]) a launch on CU share
    `part` of `nparts` runs on (kctc_cu_partition_probe)."""
    ids = np.zeros(4096, dtype=np.uint32)
    n = ctypes.c_int(0)
    _tcheck(lib().kctc_cu_partition_probe(int(part), int(nparts), ids.ctypes.data, ids.size, ctypes.byref(n)),
            "kctc_cu_partition_probe")
    return ids[:n.value].copy()


def softmax_rows(x, stream=None):
    """SoftmaxComponent forward of a 2-D torch CUDA tensor (kctc_softmax_rows)."""
    import torch
    out = torch.empty_like(x)
    _tcheck(lib().kctc_softmax_rows(_stream_handle(stream), _ptr(x), x.shape[0], x.shape[1], _ptr(out)),
            "kctc_softmax_rows")
    return out


def ctc_decodable(probs, priors=None, prob_scale=1.0, blank_threshold=1.0, floor=1e-10, stream=None):
    """CtcDecodableAmNnet's matrix from device probs [T, A] -> torch CUDA [kept, A]."""
    import torch
    T, A = probs.shape
    out = torch.empty_like(probs)
    scratch = torch.empty(lib().kctc_ctc_decodable_scratch_bytes(T), dtype=torch.uint8, device=probs.device)
    k = ctypes.c_int()
    _tcheck(lib().kctc_ctc_decodable(_stream_handle(stream), _ptr(probs), T, A, _ptr(priors), prob_scale,
                                     blank_threshold, floor, _ptr(out), _ptr(scratch), ctypes.byref(k)),
            "kctc_ctc_decodable")
    return out[:k.value]


def dp_unique_id():
    buf = ctypes.create_string_buffer(128)
    _tcheck(lib().kctc_dp_unique_id(buf), "kctc_dp_unique_id")
    return buf.raw


def synth_minibatch(seed, T_max, N, dim, A, label_ratio=0.125, want_feats=True):
    """BASELINE.md §2 synthetic minibatch, already in FormatNnetInput layout."""
    feats = np.empty((T_max * N, dim), np.float32) if want_feats else None
    nf = np.zeros(N, np.int32)
    ll = np.zeros(N, np.int32)
    fl = np.zeros(N * 639 + 1, np.int32)
    n = lib().kctc_synth_minibatch(seed, T_max, N, dim, A, label_ratio,
                                   feats.ctypes.data if feats is not None else None,
                                   nf.ctypes.data, fl.ctypes.data, ll.ctypes.data)
    return feats, nf, fl[:n].copy(), ll


def levenshtein(ref, hyp):
    """kaldi::LevenshteinEditDistance (unit costs) through kctc_levenshtein (host code)."""
    r = np.ascontiguousarray(ref, dtype=np.int32)
    h = np.ascontiguousarray(hyp, dtype=np.int32)
    return lib().kctc_levenshtein(r.ctypes.data, len(r), h.ctypes.data, len(h))


def format_input(utt_feats, T_max=None):
    """FormatNnetInput on a list of [T_n, dim] arrays -> [T_max*N, dim]."""
    N = len(utt_feats)
    dim = utt_feats[0].shape[1]
    nf = np.array([u.shape[0] for u in utt_feats], np.int32)
    T_max = int(T_max or nf.max())
    cat = np.ascontiguousarray(np.concatenate(utt_feats, 0), dtype=np.float32)
    out = np.empty((T_max * N, dim), np.float32)
    _tcheck(lib().kctc_format_input(cat.ctypes.data, nf.ctypes.data, N, dim, T_max, out.ctypes.data),
            "kctc_format_input")
    return out


def smoke_train_step(oracle_lib):
    """One tiny NnetCtcUpdater step (2 x BLSTM-32, N=3, T=24) on cuda:0,
    checked against the fp64 oracle (called from __graft_entry__.smoke())."""
    import torch
    R, H, D, A, T, N, lr = 2, 32, 16, 9, 24, 3, 0.01
    net = Nnet(recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, learning_rate=lr,
                             param_stddev=0.2), seed=11)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    params = [net.get_params(c).astype(np.float64) for c in upd]
    feats, nf, fl, ll = synth_minibatch(5, T, N, D, A, 0.2)
    objf, acc, wt = net.train_step(torch.from_numpy(feats).to("cuda:0"), T, N, nf, fl, ll)
    s = oracle_lib.NnetSpec()
    s.num_rnn, s.mode, s.hidden, s.dirs, s.layers_per_rnn = R, 2, H, 2, 1
    s.input_dim, s.num_targets = D, A
    s.clip_threshold, s.repair_threshold, s.repair_scale, s.repair_target = 30.0, 0.01, 1.0, 0.0
    s.rnn_clip_gradient, s.lr_rnn, s.lr_affine = 5.0, lr, lr
    Wa, ba = params[-1][:-A].reshape(A, -1).copy(), params[-1][-A:].copy()
    robjf, _, rwt = oracle_lib.train_step(s, params[:-1], Wa, ba, feats.reshape(T, N, D).astype(np.float64),
                                          nf, fl, ll, repair_draws=np.ones(R, np.float32))
    params[-1] = np.concatenate([Wa.ravel(), ba])
    assert abs(objf - robjf) <= 1e-5 * abs(robjf), (objf, robjf)
    for c, p in zip(upd, params):
        got = net.get_params(c).astype(np.float64)
        err = np.linalg.norm(got - p) / np.linalg.norm(p)
        assert err < 1e-5, (c, err)
    net.close()
    return objf, robjf


# ---------------------------------------------------------------------------
# egs: NnetCtcExample archives, CompressedMatrix, background reader, GPU format
# ---------------------------------------------------------------------------
def cm_compress(m):
    """CompressedMatrix::CopyFromMat of a float32 [rows, cols] matrix -> bytes
    (the in-memory image: 20-byte GlobalHeader + body)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    rows, cols = m.shape
    L = lib()
    out = np.zeros(max(L.kctc_cm_compressed_bytes(rows, cols), 0), dtype=np.uint8)
    if out.size == 0:
        return out
    _tcheck(L.kctc_cm_compress(m.ctypes.data, rows, cols, out.ctypes.data), "kctc_cm_compress")
    return out


def cm_decompress(img):
    """CompressedMatrix::CopyToMat of an image from cm_compress -> float32 [rows, cols]."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    hdr = np.frombuffer(img[:20].tobytes(), dtype=np.int32)
    rows, cols = int(hdr[3]), int(hdr[4])
    out = np.empty((rows, cols), dtype=np.float32)
    _tcheck(lib().kctc_cm_decompress(img.ctypes.data, out.ctypes.data), "kctc_cm_decompress")
    return out


def shuffle_egs(rspecifier, wspecifier, srand=0, buffer_size=0, frame_shift=0, frame_subsampling_factor=0):
    """nnet-ctc-shuffle-egs (src/ctcbin/nnet-ctc-shuffle-egs.cc:25-127) -> examples written."""
    n = ctypes.c_long()
    _tcheck(lib().kctc_egs_shuffle(rspecifier.encode(), wspecifier.encode(), srand, buffer_size, frame_shift,
                                   frame_subsampling_factor, ctypes.byref(n)), "kctc_egs_shuffle")
    return n.value


def sort_egs(rspecifier, wspecifier, srand=0, buffer_size=0):
    """nnet-ctc-sort-egs (src/ctcbin/nnet-ctc-sort-egs.cc:27-133) -> examples written."""
    n = ctypes.c_long()
    _tcheck(lib().kctc_egs_sort(rspecifier.encode(), wspecifier.encode(), srand, buffer_size, ctypes.byref(n)),
            "kctc_egs_sort")
    return n.value


class EgsWriter:
    """NnetCtcExampleWriter over a binary Kaldi archive (features compressed)."""

    def __init__(self, wspecifier):
        self._h = ctypes.c_void_p()
        _tcheck(lib().kctc_egs_writer_open(ctypes.byref(self._h), wspecifier.encode()), "kctc_egs_writer_open")

    def write(self, key, feats, labels, left_context=0, spk_info=None):
        f = np.ascontiguousarray(feats, dtype=np.float32)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        spk = None if spk_info is None else np.ascontiguousarray(spk_info, dtype=np.float32)
        _tcheck(lib().kctc_egs_write(self._h, key.encode(), f.ctypes.data, f.shape[0], f.shape[1],
                                     lab.ctypes.data, lab.size, left_context,
                                     None if spk is None else spk.ctypes.data, 0 if spk is None else spk.size),
                "kctc_egs_write")

    def close(self):
        if self._h:
            _tcheck(lib().kctc_egs_writer_close(self._h), "kctc_egs_writer_close")
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Minibatch:
    """One minibatch from EgsReader (still compressed until format())."""

    def __init__(self, handle):
        self._h = handle
        L = lib()
        N, T, D, tl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
        _tcheck(L.kctc_minibatch_info(handle, ctypes.byref(N), ctypes.byref(T), ctypes.byref(D), ctypes.byref(tl)),
                "kctc_minibatch_info")
        self.N, self.T_max, self.input_dim, self.total_labels = N.value, T.value, D.value, tl.value
        self.num_splice = L.kctc_minibatch_num_splice(handle)  # rows per output frame of the formatted input
        self.num_frames = np.zeros(self.N, dtype=np.int32)
        self.label_lengths = np.zeros(self.N, dtype=np.int32)
        self.flat_labels = np.zeros(max(self.total_labels, 1), dtype=np.int32)
        _tcheck(L.kctc_minibatch_labels(handle, self.num_frames.ctypes.data, self.label_lengths.ctypes.data,
                                        self.flat_labels.ctypes.data), "kctc_minibatch_labels")
        self.flat_labels = self.flat_labels[:self.total_labels]
        self.keys = [L.kctc_minibatch_key(handle, n).decode() for n in range(self.N)]

    def scratch_bytes(self):
        return int(lib().kctc_minibatch_scratch_bytes(self._h))

    def format(self, out, scratch, stream=None):
        """Stream-ordered FormatNnetInput on the GPU into out [T_max*N*num_splice, input_dim] (device)."""
        _tcheck(lib().kctc_minibatch_format(self._h, _ptr(out), _ptr(scratch), int(scratch.numel()),
                                            ctypes.c_void_p(_stream_handle(stream))), "kctc_minibatch_format")

    def free(self):
        if self._h:
            lib().kctc_minibatch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class EgsReader:
    """SequentialNnetCtcExampleReader + NnetCtcExampleBackgroundReader: iterate
    minibatches (skip rules of ctc-nnet-train.cc:84-95)."""

    def __init__(self, rspecifier, minibatch_size, max_frames=100000, nnet_left_context=0, nnet_right_context=0):
        self._h = ctypes.c_void_p()
        _tcheck(lib().kctc_egs_reader_open(ctypes.byref(self._h), rspecifier.encode(), minibatch_size, max_frames,
                                           nnet_left_context, nnet_right_context), "kctc_egs_reader_open")

    def __iter__(self):
        return self

    def __next__(self):
        mb = ctypes.c_void_p()
        _tcheck(lib().kctc_egs_reader_next(self._h, ctypes.byref(mb)), "kctc_egs_reader_next")
        if not mb.value:
            raise StopIteration
        return Minibatch(mb)

    def stats(self):
        r, k = ctypes.c_long(), ctypes.c_long()
        _tcheck(lib().kctc_egs_reader_stats(self._h, ctypes.byref(r), ctypes.byref(k)), "kctc_egs_reader_stats")
        return r.value, k.value

    def close(self):
        if self._h:
            lib().kctc_egs_reader_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# LDA feature transform (include/kaldi_lda.h): get_lda.sh inside the project
# ---------------------------------------------------------------------------
LDA_BLANK_SKIP, LDA_BLANK_CLASS, LDA_BLANK_FILL = 0, 1, 2
_LDA_POLICY = {"skip": LDA_BLANK_SKIP, "class": LDA_BLANK_CLASS, "fill": LDA_BLANK_FILL}


def _f64(a, shape, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{what}: shape {a.shape}, expected {shape}")
    return a


def _lda_result(dim, D, remove_offset, want_cholesky):
    rows = D if dim <= 0 else dim
    M = np.empty((max(rows, 0), D + (1 if remove_offset else 0)), np.float32)
    chol = np.empty((D, D), np.float64) if want_cholesky else None
    return M, chol


def estimate_feature_transform(zero, first, second, dim=-1, within_class_factor=0.001, remove_offset=True,
                               max_singular_value=5.0, want_cholesky=True):
    """nnet-get-feature-transform from host statistics (kctc_lda_estimate_from_stats;
    no device): zero [C], first [C][D], second [D][D] (read through its lower
    triangle) -> (M float32 [dim][D (+1 with remove_offset)], the lower-triangular
    Cholesky factor of the within-class covariance, or None)."""
    first = np.ascontiguousarray(first, dtype=np.float64)
    if first.ndim != 2:
        raise ValueError("estimate_feature_transform: first must be [C][D]")
    C, D = first.shape
    zero = _f64(zero, (C,), "zero")
    second = _f64(second, (D, D), "second")
    if dim > D:
        raise KctcError("kctc_lda_estimate_from_stats: output dimension above the feature dimension")
    M, chol = _lda_result(dim, D, remove_offset, want_cholesky)
    _tcheck(lib().kctc_lda_estimate_from_stats(zero.ctypes.data, first.ctypes.data, second.ctypes.data, D, C, int(dim),
                                               float(within_class_factor), int(bool(remove_offset)),
                                               float(max_singular_value), M.ctypes.data,
                                               None if chol is None else chol.ctypes.data),
            "kctc_lda_estimate_from_stats")
    return M, chol


class LdaStats:
    """LdaEstimate's accumulators (acc-lda / sum-lda-accs) with the sums kept on
    the device in fp64: accumulate() and acc_egs() run on the GPU, everything
    else (stats, set_stats, read, write, estimate) on the host."""

    def __init__(self, dim, num_classes, device=0):
        self._h = ctypes.c_void_p()
        self.dim, self.num_classes, self.device = int(dim), int(num_classes), int(device)
        _tcheck(lib().kctc_lda_create(ctypes.byref(self._h), self.dim, self.num_classes, self.device),
                "kctc_lda_create")

    def close(self):
        if self._h:
            lib().kctc_lda_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate(self, feats, classes, weights=None, stream=None):
        """feats [R][dim] float32, classes [R] int32 (id < 0: the row is skipped
        and may hold anything), weights [R] float32 or None: device tensors,
        contiguous.  Stream-ordered on `stream` (default: torch's current one)."""
        import torch
        for t, dt, what in ((feats, torch.float32, "feats"), (classes, torch.int32, "classes"),
                            (weights, torch.float32, "weights")):
            if t is None:
                continue
            if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
                raise ValueError(f"LdaStats.accumulate: {what} must be a contiguous {dt} device tensor")
        R = int(classes.shape[0])
        if tuple(feats.shape) != (R, self.dim) or (weights is not None and tuple(weights.shape) != (R,)):
            raise ValueError("LdaStats.accumulate: feats [R][dim], classes [R], weights [R]")
        _tcheck(lib().kctc_lda_accumulate(self._h, _stream_handle(stream), _ptr(feats), _ptr(classes), _ptr(weights), R),
                "kctc_lda_accumulate")

    def stats(self):
        """(zero [C], first [C][dim], second [dim][dim]) as float64; second is the
        full, exactly symmetric matrix.  Waits for the accumulate calls so far."""
        z = np.empty(self.num_classes, np.float64)
        f = np.empty((self.num_classes, self.dim), np.float64)
        s = np.empty((self.dim, self.dim), np.float64)
        _tcheck(lib().kctc_lda_get_stats(self._h, z.ctypes.data, f.ctypes.data, s.ctypes.data), "kctc_lda_get_stats")
        return z, f, s

    def set_stats(self, zero, first, second, add=False):
        z = _f64(zero, (self.num_classes,), "zero")
        f = _f64(first, (self.num_classes, self.dim), "first")
        s = _f64(second, (self.dim, self.dim), "second")
        _tcheck(lib().kctc_lda_set_stats(self._h, z.ctypes.data, f.ctypes.data, s.ctypes.data, int(bool(add))),
                "kctc_lda_set_stats")

    def write(self, path, binary=True):
        """LdaEstimate::Write: the file acc-lda writes (float, therefore lossy)."""
        _tcheck(lib().kctc_lda_write(self._h, str(path).encode(), int(bool(binary))), "kctc_lda_write")

    def read(self, path, add=False):
        """LdaEstimate::Read; add=True adds the file's statistics (sum-lda-accs)."""
        _tcheck(lib().kctc_lda_read(self._h, str(path).encode(), int(bool(add))), "kctc_lda_read")

    def acc_egs(self, egs_rspecifier, ali_rspecifier, context=(0,), blank_policy="skip"):
        """acc-lda over an egs archive and the alignment table Nnet.align_egs
        writes (kctc_lda_acc_egs) -> (examples used, examples without an
        alignment, mismatches, frames accumulated)."""
        ctx = np.ascontiguousarray(context, dtype=np.int32)
        policy = _LDA_POLICY[blank_policy] if isinstance(blank_policy, str) else int(blank_policy)
        out = [ctypes.c_long() for _ in range(4)]
        _tcheck(lib().kctc_lda_acc_egs(self._h, str(egs_rspecifier).encode(), str(ali_rspecifier).encode(),
                                       ctx.ctypes.data, ctx.size, policy, *[ctypes.byref(o) for o in out]),
                "kctc_lda_acc_egs")
        return tuple(o.value for o in out)

    def estimate(self, dim=-1, within_class_factor=0.001, remove_offset=True, max_singular_value=5.0):
        """nnet-get-feature-transform -> (M float32 [dim][D (+1)], Cholesky factor
        of the within-class covariance, lower-triangular float64)."""
        if dim > self.dim:
            raise KctcError("kctc_lda_estimate: output dimension above the feature dimension")
        M, chol = _lda_result(dim, self.dim, remove_offset, True)
        _tcheck(lib().kctc_lda_estimate(self._h, int(dim), float(within_class_factor), int(bool(remove_offset)),
                                        float(max_singular_value), M.ctypes.data, chol.ctypes.data),
                "kctc_lda_estimate")
        return M, chol

    @staticmethod
    def _test_batch_rows(rows):
        """Test hook (csrc/test_hooks.h): the spliced rows after which acc_egs hands
        a batch to accumulate, rows <= 0 for the default; returns the previous value."""
        return lib().kctc_lda_test_batch_rows(int(rows))

    def guards_intact(self):
        """Test hook (csrc/test_hooks.h): the guard words around the device arrays are untouched."""
        ok = ctypes.c_int()
        _tcheck(lib().kctc_lda_test_guards(self._h, ctypes.byref(ok)), "kctc_lda_test_guards")
        return bool(ok.value)
