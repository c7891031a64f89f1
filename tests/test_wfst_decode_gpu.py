"""The graph search kernels (include/kaldi_ctc_decode.h, kctc_wfst_decode_async)
against the fp64 reference of tests/wfst_ref.py.

Batches of N = 3: utterance 0 has the listed T, the others are 0..10 % shorter,
the padding rows hold NaN.  Log-likelihoods: 3 * N(0,1) through a log-softmax
("flat"), or with +4 on the blank column first ("blank").

For every utterance, without the reference: the status is the expected one;
ali names one ilabel per frame and -1 behind the utterance; a path of the graph
from the start state exists that carries exactly these ilabels and emits
exactly the returned words (ending on a final state when status is 1), and the
cheapest such path, scored in fp64 (wfst_ref.consistent_cost), costs what
`scores` says within rtol 1e-4 / atol 1e-4, the project's bar for CTC costs
(tests/test_ctc_beam_gpu.py).  Against the reference: the score within the same
tolerance, and the same words wherever the reference's own words survive three
draws of uniform +-1e-3 noise on every log-likelihood; utterance 0 of every
shape must pass that filter (the test fails, never skips, otherwise).

Separation at the seeds below, (utterances that pass) / (utterances):
  token loop (T, A)           flat   blank
  (1, 5)                      3/3    3/3
  (2, 5)                      3/3    3/3
  (9, 5)                      3/3    3/3
  (65, 41)                    3/3    3/3
  (64, 130)                   3/3    3/3
  (2000, 41)                  3/3    1/3   (flat: seed 2; at seeds 0 and 1 utterance 0 is not separated)
  linear (T, L): (9, 3) 3/3, (65, 20) 3/3
  random (S, T, max_active, beam): see RANDOM below, all 3/3 but (7, 9, 64, inf) 2/3; (200, 33, 4, 8)
  loses utterance 2 to the pruning (status -1) and (200, 9, 1, inf), at seed 4, utterance 2 likewise
  lexicon (20 words, 40 labels, T = 140): 3/3
(the counts are printed by every test; they are asserted for utterance 0 only)
"""
import functools

import numpy as np
import pytest

import ctc_align_ref
import wfst_ref as ref

pytestmark = pytest.mark.gpu

INF = np.inf
N = 3


def _loglikes(rng, T, A, family, lens=None):
    x = (rng.standard_normal((max(T, 1), N, A)) * 3).astype(np.float32)
    if family == "blank":
        x[:, :, 0] += 4
    ll = np.stack([ctc_align_ref.log_softmax64(x[:, n]) for n in range(N)], axis=1).astype(np.float32)
    if lens is None:
        lens = [T - int(rng.integers(0, T // 10 + 1)) if n else T for n in range(N)]
    for n, t in enumerate(lens):
        ll[t:, n, :] = np.nan
    return ll, np.array(lens, np.int32)


def _references(g, ll, lens, beam, max_active, rng, scale=1.0):
    refs = []
    for n, t in enumerate(lens):
        x = ll[:t, n].astype(np.float64)
        words, ali, score, status, _ = ref.decode(g, x, beam, max_active, scale)
        sep = True
        for _ in range(3):
            sep = sep and ref.decode(g, x + rng.uniform(-1e-3, 1e-3, size=x.shape), beam, max_active, scale)[0] == words
        refs.append((words, ali, score, status, sep))
    return refs


# case -> seed at which utterance 0 is well separated (and, with max_active = 1, survives); default 0
SEEDS = {("token", 2000, 41, "flat"): 2, ("random", 200, 9, 1, np.inf, False, False): 4}


@functools.lru_cache(maxsize=None)
def _case(kind, *p):
    """graph arrays, RefGraph, loglikes, lengths, (beam, max_active), references; once per shape"""
    col = None
    seed = SEEDS.get((kind,) + p, 0)
    if kind == "token":
        T, A, family = p
        rng = np.random.default_rng([1, seed, T, A, family == "blank"])
        gd, beam, ma = None, 15.0, 7000
    elif kind == "linear":
        T, L = p
        A, family = 8, "flat"
        rng = np.random.default_rng([2, seed, T, L])
        labels = rng.integers(1, A, size=L).tolist()
        for k in range(1, L, 3):
            labels[k] = labels[k - 1]  # repeats: a blank is forced between them
        gd, beam, ma = ref.linear_graph(labels), INF, 7000
    elif kind == "random":
        S, T, ma, beam, big, permute = p
        A, family = 6, "flat"
        rng = np.random.default_rng([3, seed, S, T, ma, int(min(beam, 1e6)), big, permute])
        gd = ref.random_graph(rng, S, A, 0 if big else None)
        if permute:  # a non-default ilabel_to_col into a wider row
            A = 11
            col = np.concatenate(([-7], rng.permutation(A)[:6])).astype(np.int32)
    elif kind == "lexicon":
        T, A, family = 140, 41, "blank"
        rng = np.random.default_rng([4])
        gd, beam, ma = None, 15.0, 1000
    ll, lens = _loglikes(rng, T, A, family)
    ll.setflags(write=False)
    return dict(kind=kind, p=p, gd=gd, col=col, ll=ll, lens=lens, beam=beam, ma=ma, A=A, rng=rng,
                labels=labels if kind == "linear" else None)


def _graphs(kctc, c):
    """(Graph, RefGraph, references) of a case; the references once per case"""
    if "g" not in c:
        if c["kind"] == "token":
            graph = kctc.ctc_token_graph(c["A"])
        elif c["kind"] == "lexicon":
            rng = np.random.default_rng(40)
            lex = [(w + 1, rng.integers(1, 41, size=int(rng.integers(2, 6))).tolist()) for w in range(20)]
            lex[1] = (2, lex[0][1][-1:] + lex[1][1])  # word 2 starts with the label word 1 ends on
            graph = kctc.ctc_lexicon_graph(lex, 41, rng.random(20))
        else:
            graph = kctc.Graph(**c["gd"], ilabel_to_col=c["col"])
        c["g"] = graph
        c["r"] = ref.RefGraph.from_graph(graph, c["col"])
        c["refs"] = _references(c["r"], c["ll"], c["lens"], c["beam"], c["ma"], c["rng"])
    return c["g"], c["r"], c["refs"]


def _decode(kctc, gpu, graph, ll, lens, beam, ma, **kw):
    import torch
    out = kctc.wfst_decode(torch.from_numpy(np.array(ll)).to(gpu), lens, graph, beam=beam, max_active=ma, **kw)
    words, ali, scores, status = out
    assert len(words) == len(lens) and ali.shape == (ll.shape[0], len(lens)) and ali.dtype == np.int32
    assert scores.dtype == np.float64 and scores.shape == (len(lens),) and status.shape == (len(lens),)
    return out


def _check_utt(r, ll, T, words, ali, score, status, expect, listed, scale=1.0):
    """validity without the reference, then the reference `expect`"""
    rwords, rali, rscore, rstatus, sep = expect
    print(f"T={T} status {status} (reference {rstatus}) words {len(words)} (reference {len(rwords)}) "
          f"score {score:.9g} reference {rscore:.9g} separated {sep}")
    assert status == rstatus
    assert (ali[T:] == -1).all()
    if status < 0:
        assert words == [] and (ali == -1).all() and score == INF
        return sep
    assert (ali[:T] >= 1).all()
    exact = ref.consistent_cost(r, ll[:T].astype(np.float64), ali[:T].tolist(), words, status == 1, scale)
    print(f"  cheapest path with these ilabels and words, fp64: {exact:.9g}")
    assert np.isfinite(exact), "no path of the graph carries these ilabels and words"
    np.testing.assert_allclose(score, exact, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(score, rscore, rtol=1e-4, atol=1e-4)
    if listed:
        assert sep, "the case is not well separated: the reference's own words move under 1e-3 noise"
    if sep:
        assert words == rwords
    return sep


def _run_case(kctc, gpu, c, **kw):
    graph, r, refs = _graphs(kctc, c)
    words, ali, scores, status = _decode(kctc, gpu, graph, c["ll"], c["lens"], c["beam"], c["ma"], **kw)
    passed = sum(_check_utt(r, c["ll"][:, n], int(c["lens"][n]), words[n], ali[:, n], scores[n], status[n], refs[n],
                            n == 0) for n in range(N))
    print(f"separated {passed}/{N}")
    return words, ali, scores, status


TOKEN = [(1, 5), (2, 5), (9, 5), (65, 41), (64, 130), (2000, 41)]


@pytest.mark.parametrize("family", ["flat", "blank"])
@pytest.mark.parametrize("T,A", TOKEN)
def test_token_loop(kctc, gpu, T, A, family):
    c = _case("token", T, A, family)
    words, ali, scores, status = _run_case(kctc, gpu, c)
    for n in range(N):
        t = int(c["lens"][n])
        assert status[n] == 1
        assert words[n] == ref.collapsed_argmax(c["ll"][:t, n])
        assert (ali[:t, n] - 1 == c["ll"][:t, n].argmax(axis=1)).all()


@pytest.mark.parametrize("T,L", [(9, 3), (65, 20)])
def test_linear_graph_is_forced_alignment(kctc, gpu, T, L):
    c = _case("linear", T, L)
    words, ali, scores, status = _run_case(kctc, gpu, c)
    for n in range(N):
        t = int(c["lens"][n])
        _, score = ctc_align_ref.viterbi(c["ll"][:t, n].astype(np.float64), c["labels"], 0)
        assert status[n] == 1 and words[n] == c["labels"]
        np.testing.assert_allclose(-scores[n], score, rtol=1e-4, atol=1e-4)


RANDOM = [
    # S, T, max_active, beam, a state with 300 emitting arcs, a non-default ilabel_to_col
    (1, 5, 1, INF, False, False),
    (7, 9, 64, INF, False, False),
    (200, 33, 4, 8.0, False, False),
    (200, 140, 64, 8.0, True, False),
    (3000, 65, 4096, INF, False, False),  # more states and more live tokens than threads
    (2000, 300, 256, 10.0, False, False),
    (200, 9, 1, INF, False, False),       # max_active = 1
    (200, 33, 64, 8.0, False, True),
]


@pytest.mark.parametrize("S,T,ma,beam,big,permute", RANDOM)
def test_random_graph(kctc, gpu, S, T, ma, beam, big, permute):
    c = _case("random", S, T, ma, beam, big, permute)
    graph, r, refs = _graphs(kctc, c)
    assert S < 4 or graph.eps_depth >= 3
    if big:
        assert np.bincount(r.src[r.emit], minlength=S).max() >= 300
    _run_case(kctc, gpu, c)
    if beam == INF and ma >= S:  # nothing pruned: the exact Viterbi
        for n in range(N):
            exact = ref.viterbi(r, c["ll"][:c["lens"][n], n].astype(np.float64))
            assert exact[3] == refs[n][3] and exact[2] == refs[n][2]


def test_lexicon_graph(kctc, gpu):
    c = _case("lexicon")
    graph, r, refs = _graphs(kctc, c)
    assert graph.eps_depth == 1
    words, *_ = _run_case(kctc, gpu, c)
    assert all(1 <= w <= 20 for n in range(N) for w in words[n])


@pytest.mark.parametrize("kind,p", [("random", RANDOM[4]), ("random", RANDOM[5]), ("token", (65, 41, "blank"))])
def test_second_call_identical_and_batch_equals_alone(kctc, gpu, kind, p):
    c = _case(kind, *p)
    graph, r, refs = _graphs(kctc, c)
    a = _decode(kctc, gpu, graph, c["ll"], c["lens"], c["beam"], c["ma"])
    b = _decode(kctc, gpu, graph, c["ll"], c["lens"], c["beam"], c["ma"])
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    for n in range(N):
        t = int(c["lens"][n])
        w1, a1, s1, st1 = _decode(kctc, gpu, graph, c["ll"][:t, n:n + 1], c["lens"][n:n + 1], c["beam"], c["ma"])
        assert w1[0] == a[0][n] and st1[0] == a[3][n]
        assert a1[:, 0].tobytes() == a[1][:t, n].tobytes()
        assert s1[0] == a[2][n]


def _chain_graph(kctc, finals):
    # 0 -1-> 1 -2-> 2 -1-> 3, an epsilon 1 -> 3 that emits word 9
    return kctc.Graph(finals, [0, 1, 2, 1], [1, 2, 1, 0], [5, 0, 6, 9], [0.5, 0.25, 1.0, 2.0], [1, 2, 3, 3])


def _explicit(kctc, gpu, graph, lens, A=3, seed=0, **kw):
    rng = np.random.default_rng([9, seed])
    T = max(max(lens), 1)
    ll, lens = _loglikes(rng, T, A, "flat", lens)
    r = ref.RefGraph.from_graph(graph)
    out = _decode(kctc, gpu, graph, ll, lens, kw.pop("beam", INF), kw.pop("ma", 100), **kw)
    expect = [ref.decode(r, ll[:t, n].astype(np.float64)) [:4] + (True,) for n, t in enumerate(lens)]
    return r, ll, lens, out, expect


def test_status_no_final_state(kctc, gpu):
    graph = _chain_graph(kctc, [INF] * 4)
    r, ll, lens, (words, ali, scores, status), expect = _explicit(kctc, gpu, graph, [3, 2, 1])
    for n in range(N):
        assert status[n] == 0
        _check_utt(r, ll[:, n], int(lens[n]), words[n], ali[:, n], scores[n], status[n], expect[n], False)
    assert words[0] == [5, 6] and words[2] in ([5], [5, 9])


def test_status_every_path_too_short(kctc, gpu):
    graph = _chain_graph(kctc, [INF, INF, INF, 0.0])
    r, ll, lens, (words, ali, scores, status), expect = _explicit(kctc, gpu, graph, [5, 3, 4])
    assert status.tolist() == [-1, 1, -1]
    for n in range(N):
        _check_utt(r, ll[:, n], int(lens[n]), words[n], ali[:, n], scores[n], status[n], expect[n], False)


def test_status_pool_exhausted_for_one_utterance(kctc, gpu):
    graph = kctc.ctc_token_graph(5)  # |Q_0| = 1, |Q_t| = 5: an utterance needs 1 + 5 T records
    r, ll, lens, full, expect = _explicit(kctc, gpu, graph, [4, 9, 3], A=5)
    words, ali, scores, status = _decode(kctc, gpu, graph, ll, lens, INF, 100, pool_tokens=30)
    assert status.tolist() == [1, -2, 1]
    assert words[1] == [] and (ali[:, 1] == -1).all() and scores[1] == INF
    for n in (0, 2):
        assert words[n] == full[0][n] and scores[n] == full[2][n] and (ali[:, n] == full[1][:, n]).all()
        _check_utt(r, ll[:, n], int(lens[n]), words[n], ali[:, n], scores[n], status[n], expect[n], False)
    exact = _decode(kctc, gpu, graph, ll, lens, INF, 100, pool_tokens=46)  # utterance 1 needs exactly 46
    assert exact[3].tolist() == [1, 1, 1] and exact[0][1] == full[0][1]


@pytest.mark.parametrize("lens", [[0, 3, 0], [0, 0, 0]])
def test_zero_frames(kctc, gpu, lens):
    # Q_0: 0 -eps:7-> 1 -eps-> 2 (final 0.5) -eps-> 3 (final 0), a dearer epsilon 0 -> 2
    graph = kctc.Graph([INF, INF, 0.5, 0.0, INF], [2, 0, 1, 0, 3, 0, 3], [0, 0, 0, 2, 1, 0, 2], [0, 7, 0, 0, 4, 0, 9],
                       [0.25, -1.5, 0.0, 2.0, 0.125, 1.0, 3.5], [3, 1, 2, 4, 3, 2, 0])
    r, ll, lens, (words, ali, scores, status), expect = _explicit(kctc, gpu, graph, lens)
    for n in range(N):
        _check_utt(r, ll[:, n], int(lens[n]), words[n], ali[:, n], scores[n], status[n], expect[n], False)
        if lens[n] == 0:
            assert status[n] == 1 and words[n] == [7] and scores[n] == -1.25
