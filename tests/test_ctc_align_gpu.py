"""CTC forced alignment kernels (include/ctc.h, mictc_ctc_align_async) against
the fp64 reference of tests/ctc_align_ref.py.

Inputs as in tests/test_ctc_gpu.py: activations 3 * N(0,1) fp32, labels with
and without repeats (probability 0.3) trimmed until L + repeats <= T, in
batches whose other utterances are 0..10 % shorter; the padding rows of the
activations hold NaN.  For every feasible utterance: the ids are valid and
collapse to the labels, the score is the fp64 log-probability of the returned
path and the reference's score (1e-4 relative, atol 1e-4: the project's bar
for CTC costs), and the path is the reference's path.  The last is demanded of
well-separated inputs only: each case first checks on the CPU that the
reference's path survives three draws of uniform +-1e-3 noise on every
log-prob, and fails (never skips) if the utterance of the listed shape does
not (the shorter utterances beside it are compared wherever they pass it:
all but two do).  Every shape runs on both Viterbi
kernels (one state per thread; 512 threads of 3 states)."""
import ctypes
import functools

import numpy as np
import pytest

import ctc_align_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0


@pytest.fixture(params=[1, 0], ids=lambda k: "auto" if k else "spt3")
def kernel(kctc, request):
    """1 (default): one state per thread up to S = 512, the 3-state kernel
    beyond.  0: the 3-state kernel for every batch."""
    prev = kctc.ctc_align_kernel(request.param)
    yield request.param
    kctc.ctc_align_kernel(prev)


def _labels(rng, L, A, repeats):
    out = []
    for i in range(L):
        if repeats and out and rng.random() < 0.3:
            out.append(out[-1])
            continue
        v = int(rng.integers(1, A))
        while not repeats and out and v == out[-1]:
            v = int(rng.integers(1, A))
        out.append(v)
    return out


def _separated(lp, labels, path, blank, rng):
    """the reference's path is unchanged under uniform +-1e-3 noise on every log-prob, three draws"""
    for _ in range(3):
        p2, _ = ref.viterbi(lp + rng.uniform(-1e-3, 1e-3, size=lp.shape), labels, blank)
        if not np.array_equal(p2, path):
            return False
    return True


@functools.lru_cache(maxsize=None)
def _case(T, N, L, A, rep, blank=0):
    """A seeded batch, the reference's result per utterance and whether each
    utterance passes the separation filter; computed once per shape and shared
    (read-only) by both kernels."""
    rng = np.random.default_rng([SEED, T, L, A, int(rep)])
    acts = (rng.standard_normal((T, N, A)) * 3).astype(np.float32)
    lens = [T - int(rng.integers(0, T // 10 + 1)) if n else T for n in range(N)]
    labels = []
    for t in lens:
        lab = _labels(rng, L, A, rep)
        while not ref.feasible(t, lab):
            lab.pop()
        if blank:  # labels drawn from [1, A) avoid blank 0; shift them below blank = A - 1
            lab = [v - 1 for v in lab]
        labels.append(lab)
    for n, t in enumerate(lens):
        acts[t:, n, :] = np.nan
    refs = []
    for n, t in enumerate(lens):
        path, score, lp = ref.align(acts[:t, n], labels[n], blank)
        refs.append((path, score, lp, _separated(lp, labels[n], path, blank, rng)))
    acts.setflags(write=False)
    return acts, labels, np.array(lens, np.int32), refs


def _flat(labels):
    return (np.array([v for l in labels for v in l], np.int32), np.array([len(l) for l in labels], np.int32))


def _align(kctc, gpu, acts, labels, lens, blank=0):
    import torch
    fl, ll = _flat(labels)
    ali, scores = kctc.ctc_align(torch.from_numpy(np.array(acts)).to(gpu), fl, ll, lens, blank=blank)
    torch.cuda.synchronize()
    return ali.cpu().numpy(), scores


def _check_utt(ali_n, score, labels, T, A, blank, r, listed=True):
    """listed: the utterance has the case's listed shape (utterance 0 of a
    batch), which must pass the separation filter; the 0..10 % shorter ones
    beside it are held to the same path wherever they pass it too (all but
    two of them do at seed 0)."""
    path, rscore, lp, separated = r
    assert np.all(ali_n[T:] == -1)
    got = ali_n[:T]
    assert np.all((got >= 0) & (got < A))
    assert ref.collapse(got, blank) == list(labels)
    mine = float(lp[np.arange(T), got].sum())  # fp64 log-probability of the returned path
    print(f"T={T} L={len(labels)} score {score:.9g} path-eval {mine:.9g} reference {rscore:.9g}")
    np.testing.assert_allclose(score, mine, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(score, rscore, rtol=1e-4, atol=1e-4)
    if listed:
        assert separated, "the case is not well separated: the reference's own path moves under 1e-3 noise"
    if separated:
        assert np.array_equal(got, path)
    else:
        print("  (a shorter utterance of the batch whose reference path moves under 1e-3 noise: validity and score only)")


SHAPES = [
    # T, N, L, A
    (1, 3, 0, 5),        # single frame, all blank
    (2, 3, 1, 5),
    (3, 3, 1, 5),
    (9, 3, 4, 5),
    (31, 3, 15, 41),     # T = 2L+1
    (32, 3, 10, 41),     # chunk depths
    (33, 3, 16, 41),     # chunk depths
    (65, 3, 32, 41),     # S = 65 crosses a wave
    (64, 3, 20, 130),    # A > 2 waves
    (140, 3, 65, 41),
    (560, 3, 255, 41),   # S = 511: the last size of the one-state kernel's 8 waves
    (560, 3, 256, 41),   # S = 513: the first size past it
    (700, 3, 300, 41),   # S = 601, past the loss's window kernel
    (1400, 3, 639, 41),  # S = 1279, the maximum
    (2000, 2, 250, 41),  # recipe length, offset accuracy
]


@pytest.mark.parametrize("rep", [False, True], ids=["norep", "rep"])
@pytest.mark.parametrize("T,N,L,A", SHAPES)
def test_align_matches_reference(kctc, gpu, kernel, T, N, L, A, rep):
    assert kctc.ctc_align_kernel() == kernel
    acts, labels, lens, refs = _case(T, N, L, A, rep)
    ali, scores = _align(kctc, gpu, acts, labels, lens)
    assert ali.shape == (T, N) and ali.dtype == np.int32 and scores.dtype == np.float64
    for n in range(N):
        _check_utt(ali[:, n], scores[n], labels[n], int(lens[n]), A, 0, refs[n], listed=n == 0)


@pytest.mark.parametrize("T,N,L,A", [(33, 3, 16, 41), (140, 3, 65, 41)])
def test_align_blank_last(kctc, gpu, kernel, T, N, L, A):
    acts, labels, lens, refs = _case(T, N, L, A, True, A - 1)
    ali, scores = _align(kctc, gpu, acts, labels, lens, blank=A - 1)
    for n in range(N):
        _check_utt(ali[:, n], scores[n], labels[n], int(lens[n]), A, A - 1, refs[n], listed=n == 0)


def test_align_single_path(kctc, gpu, kernel):
    """T == L without repeats and T == L + repeats with repeats: one path each"""
    A = 9
    labels = [[1, 2, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4], [1, 1, 2, 3, 3, 3, 4, 5, 5]]
    lens = np.array([12, 9 + 4], np.int32)
    rng = np.random.default_rng([SEED, 12, 13])
    acts = (rng.standard_normal((13, 2, A)) * 3).astype(np.float32)
    acts[12:, 0] = np.nan
    ali, scores = _align(kctc, gpu, acts, labels, lens)
    assert ali[:12, 0].tolist() == labels[0]
    assert ali[:, 1].tolist() == [1, 0, 1, 2, 3, 0, 3, 0, 3, 4, 5, 0, 5]
    for n in range(2):
        T = int(lens[n])
        path, score, lp = ref.align(acts[:T, n], labels[n])
        _check_utt(ali[:, n], scores[n], labels[n], T, A, 0, (path, score, lp, True))


@pytest.mark.parametrize("T,labels", [
    (5, [1, 2]),
    (4, [1, 1]),
    (40, [3, 1, 1, 2, 5, 5, 5, 4, 1, 6, 2, 2]),
])
def test_align_ties(kctc, gpu, kernel, T, labels):
    """all-zero activations: every path that fits scores the same, the tie rule picks one"""
    A = 7
    acts = np.zeros((T, 1, A), np.float32)
    ali, scores = _align(kctc, gpu, acts, [labels], np.array([T], np.int32))
    path, score, _ = ref.align(acts[:, 0], labels)
    if T == 5:
        assert path.tolist() == [1, 2, 0, 0, 0]
    if T == 4:
        assert path.tolist() == [1, 0, 1, 0]
    assert ali[:, 0].tolist() == path.tolist()
    np.testing.assert_allclose(scores[0], score, rtol=1e-6)


def test_align_infeasible_inside_a_batch(kctc, gpu, kernel):
    T, N, L, A = 33, 3, 16, 41
    acts, labels, lens, refs = _case(T, N, L, A, True)
    labels = list(labels)
    labels[1] = [2] * 20  # 20 labels + 19 repeats need 39 frames
    lens = lens.copy()
    lens[1] = 29
    assert not ref.feasible(29, labels[1])
    ali, scores = _align(kctc, gpu, acts, labels, lens)
    assert np.all(ali[:, 1] == -1) and scores[1] == -np.inf
    for n in (0, 2):
        _check_utt(ali[:, n], scores[n], labels[n], int(lens[n]), A, 0, refs[n], listed=n == 0)


def test_align_hygiene(kctc, gpu, kernel):
    """two calls give identical bytes, nothing is written past the outputs, invalid arguments are refused"""
    import torch
    T, N, L, A = 140, 3, 65, 41
    acts, labels, lens, _ = _case(T, N, L, A, True)
    fl, ll = _flat(labels)
    a = torch.from_numpy(np.array(acts)).to(gpu)
    ws = torch.empty(kctc.ctc_align_workspace_size(ll, lens, A), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream
    G = 16
    outs = []
    for call in range(2):
        ali = torch.full((T * N + G,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        sc = torch.full((N + G,), 12345.0, dtype=torch.float64, device=gpu)
        ws.fill_(call * 255)  # whatever the workspace holds
        st = kctc.lib().mictc_ctc_align_async(a.data_ptr(), fl.ctypes.data, ll.ctypes.data, lens.ctypes.data, A, N,
                                              ali.data_ptr(), sc.data_ptr(), ws.data_ptr(), stream, 0)
        assert st == 0
        torch.cuda.synchronize()
        ali, sc = ali.cpu().numpy(), sc.cpu().numpy()
        assert np.all(ali[T * N:] == 0x5A5A5A5A) and np.all(sc[N:] == 12345.0)
        outs.append((ali.tobytes(), sc.tobytes()))
    assert outs[0] == outs[1]

    ali = torch.full((T * N,), 7, dtype=torch.int32, device=gpu)
    sc = torch.full((N,), 7.0, dtype=torch.float64, device=gpu)

    def call(fl_, ll_, ws_ptr):
        return kctc.lib().mictc_ctc_align_async(a.data_ptr(), fl_.ctypes.data, ll_.ctypes.data, lens.ctypes.data, A, N,
                                                ali.data_ptr(), sc.data_ptr(), ws_ptr, stream, 0)

    bad = fl.copy()
    bad[3] = 0  # a label equal to blank
    assert call(bad, ll, ws.data_ptr()) == 2
    bad[3] = A  # out of range
    assert call(bad, ll, ws.data_ptr()) == 2
    long_ll = ll.copy()
    long_ll[0] = 640
    assert call(np.ones(640 + int(ll.sum()), np.int32), long_ll, ws.data_ptr()) == 2
    assert call(fl, ll, None) == 2
    torch.cuda.synchronize()
    assert torch.all(ali == 7) and torch.all(sc == 7.0)  # a refused call enqueues nothing
    size = ctypes.c_size_t()
    assert kctc.lib().mictc_get_align_workspace_size(long_ll.ctypes.data, lens.ctypes.data, A, N,
                                                     ctypes.byref(size)) == 2
