"""The graph-search reference (tests/wfst_ref.py) checked against brute force
and against the two graph builders, on the CPU: unpruned it equals the minimum
over all A^T frame sequences (T <= 5, A = 3); pruning never lowers the cost;
ctc_token_graph decodes to the collapsed frame-wise argmax; ctc_lexicon_graph
equals a brute force over word sequences on a 4-word lexicon that holds a word
pair sharing a boundary label."""
import itertools

import numpy as np
import pytest

import ctc_align_ref
import wfst_ref as ref


def _ll(rng, T, A, blank_boost=0.0):
    x = rng.standard_normal((T, A)) * 3
    x[:, 0] += blank_boost
    return ctc_align_ref.log_softmax64(x.astype(np.float32))


@pytest.mark.parametrize("T", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_unpruned_equals_brute_force(T, seed):
    rng = np.random.default_rng([seed, T])
    g = ref.RefGraph(**ref.random_graph(rng, 7, 3))
    ll = _ll(rng, T, 3)
    words, ali, score, status, arcs = ref.viterbi(g, ll)
    bf = ref.brute_force(g, ll)
    if status == 1:
        np.testing.assert_allclose(score, bf, rtol=1e-12, atol=1e-12)
        c, _ = ref.path_cost(g, ll, arcs)
        np.testing.assert_allclose(c, score, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref.consistent_cost(g, ll, ali, words), score, rtol=1e-12, atol=1e-12)
    else:
        assert bf == np.inf  # no path ends on a final state


def test_some_brute_force_case_reaches_a_final_state():
    hits = 0
    for T in (1, 2, 3, 5):
        for seed in (0, 1, 2):
            rng = np.random.default_rng([seed, T])
            g = ref.RefGraph(**ref.random_graph(rng, 7, 3))
            hits += ref.viterbi(g, _ll(rng, T, 3))[3] == 1
    assert hits >= 4


@pytest.mark.parametrize("seed", range(4))
def test_pruned_cost_not_below_unpruned(seed):
    rng = np.random.default_rng([seed, 77])
    g = ref.RefGraph(**ref.random_graph(rng, 60, 5))
    ll = _ll(rng, 20, 5)
    exact = ref.viterbi(g, ll)
    for beam, ma in ((2.0, None), (np.inf, 3), (4.0, 8)):
        pruned = ref.decode(g, ll, beam, ma)
        if pruned[3] == exact[3] == 1:
            assert pruned[2] >= exact[2] - 1e-9
        if pruned[3] >= 0:
            c, _ = ref.path_cost(g, ll, pruned[4], with_final=pruned[3] == 1)
            np.testing.assert_allclose(c, pruned[2], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T,A,boost", [(1, 5, 0), (9, 5, 0), (40, 12, 4), (65, 41, 4)])
def test_token_graph_is_collapsed_argmax(kctc, T, A, boost):
    rng = np.random.default_rng([T, A])
    ll = _ll(rng, T, A, boost)
    graph = kctc.ctc_token_graph(A)
    assert graph.num_states == A and graph.eps_depth == 0
    g = ref.RefGraph.from_graph(graph)
    words, ali, score, status, _ = ref.viterbi(g, ll)
    assert status == 1
    assert words == ref.collapsed_argmax(ll)
    assert (ali - 1 == ll.argmax(axis=1)).all()
    np.testing.assert_allclose(score, -ll.max(axis=1).sum(), rtol=1e-12)


LEXICON = [(1, [1, 2]), (2, [2, 1]), (3, [2]), (4, [1, 2, 2])]  # 1 ends on 2 and 2, 3 start with 2


def _ctc_cost(ll, labels):
    if len(labels) == 0:
        return -ll[:, 0].sum()
    _, score = ctc_align_ref.viterbi(ll, labels, 0)
    return -score


@pytest.mark.parametrize("T", [1, 3, 4, 6])
@pytest.mark.parametrize("seed", [0, 1])
def test_lexicon_graph_equals_word_brute_force(kctc, T, seed):
    rng = np.random.default_rng([seed, T, 5])
    ll = _ll(rng, T, 3, 1.0)
    wcost = [0.3, 0.1, 0.7, 0.2]
    graph = kctc.ctc_lexicon_graph(LEXICON, 3, wcost)
    assert graph.eps_depth == 1
    g = ref.RefGraph.from_graph(graph)
    words, ali, score, status, _ = ref.viterbi(g, ll)
    assert status == 1
    best = np.inf
    for n in range(T + 1):
        for seq in itertools.product(range(4), repeat=n):
            labels = [c for k in seq for c in LEXICON[k][1]]
            c = _ctc_cost(ll, labels) + sum(wcost[k] for k in seq)
            best = min(best, c)
    np.testing.assert_allclose(score, best, rtol=1e-6, atol=1e-6)  # word costs are stored as floats
    # the returned words, aligned and priced on their own, cost what the search says
    assert _ctc_cost(ll, [c for w in words for c in LEXICON[w - 1][1]]) + sum(wcost[w - 1] for w in words) == \
        pytest.approx(best, abs=1e-6)


def test_lexicon_graph_boundary_label_needs_blank(kctc):
    """frames "2 2" are one word 3, not two; "2 blank 2" are two"""
    graph = kctc.ctc_lexicon_graph([(3, [2])], 3)
    g = ref.RefGraph.from_graph(graph)
    assert ref.consistent_cost(g, np.zeros((2, 3)), [3, 3], [3]) == 0.0
    assert ref.consistent_cost(g, np.zeros((2, 3)), [3, 3], [3, 3]) == np.inf
    assert ref.consistent_cost(g, np.zeros((3, 3)), [3, 1, 3], [3, 3]) == 0.0
    assert ref.consistent_cost(g, np.zeros((1, 3)), [1], []) == 0.0
