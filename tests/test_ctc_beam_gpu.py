"""CTC prefix beam search kernels (include/ctc.h, mictc_ctc_beam_search_async)
against the fp64 reference of tests/ctc_beam_ref.py.

Inputs as in tests/test_ctc_align_gpu.py: activations 3 * N(0,1) fp32 in
batches whose other utterances are 0..10 % shorter, NaN in the padding rows.
Two families: "flat" as drawn (a label on nearly every frame) and "blank" with
+4 on the blank column (blank wins many frames: fewer labels, repeats across
blanks).  For every utterance: the labels are in range and never blank,
len <= T, the row is -1 behind them; the score is at most the exact fp64 CTC
log-probability of the returned labels and agrees with the reference's score
(1e-4 relative, atol 1e-4: the project's bar for CTC costs); and the
hypothesis is the reference's.  The last is demanded of well-separated inputs
only: each case first checks on the CPU that the reference's hypothesis
survives three draws of uniform +-1e-3 noise on every log-prob, and fails
(never skips) if the utterance of the listed shape (utterance 0) does not; the
shorter utterances beside it are compared wherever they pass it.

Separation per shape at the seeds below, (utterances that pass) / (utterances),
flat then blank family:
  (T, A, beam, symbols)      flat   blank
  (1, 5, 4, 4)               3/3    3/3
  (2, 5, 4, 4)               3/3    3/3
  (5, 3, 64, 2)              3/3    3/3
  (9, 5, 4, 4)               3/3    3/3
  (33, 41, 8, 40)            3/3    2/3
  (65, 41, 16, 40)           3/3    3/3
  (64, 130, 16, 40)          3/3    3/3
  (140, 41, 32, 40)          3/3    3/3
  (140, 66, 128, 64)         3/3    2/3
  (300, 41, 64, 40)          2/3    3/3
  (2000, 41, 16, 40)         1/2    1/2   (seed 1: at seed 0 utterance 0 is not separated)
  (33, 41, 8, 40) blank 40   3/3    3/3
  (33, 41, 1, 40)            3/3    3/3
  (33, 41, 8, 1)             3/3    3/3
With 3 * N(0,1) over 40 labels the +4 on blank still leaves a label on about
three frames in four (1505 labels at T = 2000), not on one in three.
"""
import ctypes
import functools

import numpy as np
import pytest

import ctc_beam_ref as ref

pytestmark = pytest.mark.gpu

# (T, A, beam, symbols, family, blank) -> seed at which utterance 0 is well separated (default 0)
SEEDS = {(2000, 41, 16, 40, "flat", 0): 1, (2000, 41, 16, 40, "blank", 0): 1}


def _separated(lp, hyp, beam, symbols, blank, rng):
    """the reference's hypothesis is unchanged under uniform +-1e-3 noise on every log-prob, three draws"""
    for _ in range(3):
        h2, _ = ref.beam_search(lp + rng.uniform(-1e-3, 1e-3, size=lp.shape), beam, symbols, blank)
        if h2 != hyp:
            return False
    return True


@functools.lru_cache(maxsize=None)
def _case(T, N, A, beam, symbols, family, blank=0, lens=None):
    """A seeded batch, the reference's result per utterance and whether each
    utterance passes the separation filter; computed once per shape."""
    seed = SEEDS.get((T, A, beam, symbols, family, blank), 0)
    rng = np.random.default_rng([seed, T, A, beam, symbols, family == "blank", blank])
    acts = (rng.standard_normal((T, N, A)) * 3).astype(np.float32)
    if family == "blank":
        acts[:, :, blank] += 4
    if lens is None:
        lens = [T - int(rng.integers(0, T // 10 + 1)) if n else T for n in range(N)]
    for n, t in enumerate(lens):
        acts[t:, n, :] = np.nan
    refs = []
    for n, t in enumerate(lens):
        hyp, score, lp = ref.decode(acts[:t, n], beam, symbols, blank)
        refs.append((hyp, score, lp, t == 0 or _separated(lp, hyp, beam, symbols, blank, rng)))
    acts.setflags(write=False)
    return acts, np.array(lens, np.int32), refs


def _search(kctc, gpu, acts, lens, beam, symbols, blank=0):
    import torch
    hyps, scores = kctc.ctc_beam_search(torch.from_numpy(np.array(acts)).to(gpu), lens, beam=beam, symbols=symbols,
                                        blank=blank)
    assert len(hyps) == len(lens) and scores.dtype == np.float64 and scores.shape == (len(lens),)
    return hyps, scores


def _check_valid(hyp, score, lp, T, A, blank):
    """labels in range and never blank, len <= T, score <= the exact log-probability of the labels"""
    assert len(hyp) <= T
    assert all(0 <= v < A and v != blank for v in hyp)
    exact = ref.exact_logprob(lp, hyp, blank)
    print(f"T={T} len={len(hyp)} score {score:.9g} exact {exact:.9g}")
    assert score <= exact + 1e-4 + 1e-4 * abs(exact)
    return exact


def _check_utt(hyp, score, T, A, blank, r, listed):
    rhyp, rscore, lp, separated = r
    _check_valid(hyp, score, lp, T, A, blank)
    print(f"  reference len={len(rhyp)} score {rscore:.9g} separated {separated}")
    np.testing.assert_allclose(score, rscore, rtol=1e-4, atol=1e-4)
    if listed:
        assert separated, "the case is not well separated: the reference's own hypothesis moves under 1e-3 noise"
    if separated:
        assert hyp == rhyp
    return separated


SHAPES = [
    # T, N, A, beam, symbols, blank
    (1, 3, 5, 4, 4, 0),
    (2, 3, 5, 4, 4, 0),
    (5, 3, 3, 64, 2, 0),        # unpruned: must equal the brute force
    (9, 3, 5, 4, 4, 0),
    (33, 3, 41, 8, 40, 0),
    (65, 3, 41, 16, 40, 0),     # the emission chunk depth (32 frames)
    (64, 3, 130, 16, 40, 0),    # A spans more than 2 waves, K < A - 1
    (140, 3, 41, 32, 40, 0),    # more than 3 candidates per thread
    (140, 3, 66, 128, 64, 0),   # both limits at once: 33 candidates per thread
    (300, 3, 41, 64, 40, 0),
    (2000, 2, 41, 16, 40, 0),   # recipe length, offset accuracy
    (33, 3, 41, 8, 40, 40),     # blank = A - 1
    (33, 3, 41, 1, 40, 0),      # beam = 1
    (33, 3, 41, 8, 1, 0),       # symbols = 1
]


@pytest.mark.parametrize("family", ["flat", "blank"])
@pytest.mark.parametrize("T,N,A,beam,symbols,blank", SHAPES)
def test_beam_search_matches_reference(kctc, gpu, T, N, A, beam, symbols, blank, family):
    acts, lens, refs = _case(T, N, A, beam, symbols, family, blank)
    hyps, scores = _search(kctc, gpu, acts, lens, beam, symbols, blank)
    if (T, A, beam) == (5, 3, 64):  # nothing is pruned: the reference is the brute force's best transcript
        for n in range(N):
            table = ref.brute_force(refs[n][2])
            best = max(table, key=lambda k: table[k])
            assert tuple(refs[n][0]) == best and abs(refs[n][1] - table[best]) < 1e-9
    passed = sum(_check_utt(hyps[n], scores[n], int(lens[n]), A, blank, refs[n], listed=n == 0) for n in range(N))
    print(f"separated: {passed}/{N}")


def test_beam_search_empty_utterance_inside_a_batch(kctc, gpu):
    T, A, beam, symbols = 33, 41, 8, 40
    acts, lens, refs = _case(T, 3, A, beam, symbols, "blank", 0, (33, 0, 30))
    hyps, scores = _search(kctc, gpu, acts, lens, beam, symbols)
    assert hyps[1] == [] and scores[1] == 0.0
    for n in (0, 2):
        _check_utt(hyps[n], scores[n], int(lens[n]), A, 0, refs[n], listed=False)


def _raw_call(kctc, gpu, a, lens, A, N, beam, symbols, ws, blank=0, guard=16):
    """the C entry point with guard words behind every output -> (status, hyp, hyp_len, scores) as numpy"""
    import torch
    maxT = int(max(lens))
    hyp = torch.full((N * maxT + guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    hl = torch.full((N + guard,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    sc = torch.full((N + guard,), 12345.0, dtype=torch.float64, device=gpu)
    st = kctc.lib().mictc_ctc_beam_search_async(a.data_ptr(), lens.ctypes.data, A, N, beam, symbols, hyp.data_ptr(),
                                                hl.data_ptr(), sc.data_ptr(), ws.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream, blank)
    torch.cuda.synchronize()
    return st, hyp.cpu().numpy(), hl.cpu().numpy(), sc.cpu().numpy()


@pytest.mark.parametrize("T,A,beam,symbols", [(40, 7, 4, 6), (70, 41, 16, 40)])
def test_beam_search_ties(kctc, gpu, T, A, beam, symbols):
    """all-zero activations: every candidate of a frame ties.  Which prefixes
    survive is the kernel's own business; the result is valid, its score a
    lower bound, and two calls give identical bytes."""
    import torch
    N = 2
    lens = np.array([T, T - 3], np.int32)
    a = torch.zeros((T, N, A), dtype=torch.float32, device=gpu)
    ws = torch.zeros(kctc.ctc_beam_workspace_size(lens, A, beam), dtype=torch.uint8, device=gpu)
    outs = []
    for _ in range(2):
        st, hyp, hl, sc = _raw_call(kctc, gpu, a, lens, A, N, beam, symbols, ws)
        assert st == 0
        outs.append((hyp.tobytes(), hl.tobytes(), sc.tobytes()))
    assert outs[0] == outs[1]
    for n in range(N):
        t = int(lens[n])
        lp = np.full((t, A), -np.log(A))
        row = hyp[n * T:(n + 1) * T]
        assert 0 <= hl[n] <= t and np.all(row[hl[n]:] == -1)
        _check_valid(row[:hl[n]].tolist(), sc[n], lp, t, A, 0)


def test_beam_search_hygiene(kctc, gpu):
    """guard words, whatever the workspace holds, two calls, and every invalid argument"""
    import torch
    T, N, A, beam, symbols = 140, 3, 41, 32, 40
    acts, lens, refs = _case(T, N, A, beam, symbols, "blank")
    a = torch.from_numpy(np.array(acts)).to(gpu)
    ws = torch.empty(kctc.ctc_beam_workspace_size(lens, A, beam), dtype=torch.uint8, device=gpu)
    outs = []
    for call in range(2):
        ws.fill_(call * 255)
        st, hyp, hl, sc = _raw_call(kctc, gpu, a, lens, A, N, beam, symbols, ws)
        assert st == 0
        assert np.all(hyp[N * T:] == 0x5A5A5A5A) and np.all(hl[N:] == 0x5A5A5A5A) and np.all(sc[N:] == 12345.0)
        for n in range(N):
            row = hyp[n * T:(n + 1) * T]
            assert 0 <= hl[n] <= lens[n] and np.all(row[hl[n]:] == -1)  # -1 behind the labels and in the padding
            assert np.all((row[:hl[n]] > 0) & (row[:hl[n]] < A))
        outs.append((hyp.tobytes(), hl.tobytes(), sc.tobytes()))
    assert outs[0] == outs[1]

    hyp = torch.full((N * T,), 7, dtype=torch.int32, device=gpu)
    hl = torch.full((N,), 7, dtype=torch.int32, device=gpu)
    sc = torch.full((N,), 7.0, dtype=torch.float64, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(acts=a.data_ptr(), lens=lens.ctypes.data, A=A, N=N, beam=beam, symbols=symbols, hyp=hyp.data_ptr(),
                hl=hl.data_ptr(), sc=sc.data_ptr(), ws=ws.data_ptr(), blank=0)

    def call(**kw):
        g = dict(good, **kw)
        return kctc.lib().mictc_ctc_beam_search_async(g["acts"], g["lens"], g["A"], g["N"], g["beam"], g["symbols"],
                                                      g["hyp"], g["hl"], g["sc"], g["ws"], stream, g["blank"])

    neg = lens.copy()
    neg[1] = -1
    bad = [dict(beam=0), dict(beam=129), dict(symbols=0), dict(symbols=65), dict(A=1), dict(blank=-1), dict(blank=A),
           dict(lens=neg.ctypes.data), dict(N=0), dict(acts=None), dict(lens=None), dict(hyp=None), dict(hl=None),
           dict(sc=None), dict(ws=None)]
    for kw in bad:
        assert call(**kw) == 2, kw
    torch.cuda.synchronize()
    assert torch.all(hyp == 7) and torch.all(hl == 7) and torch.all(sc == 7.0)  # a refused call enqueues nothing
    size = ctypes.c_size_t()
    assert kctc.lib().mictc_get_beam_workspace_size(neg.ctypes.data, A, N, beam, ctypes.byref(size)) == 2
    assert kctc.lib().mictc_get_beam_workspace_size(lens.ctypes.data, A, N, beam, None) == 2
    assert call() == 0  # the same arguments, all valid
    torch.cuda.synchronize()
