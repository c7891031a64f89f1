"""The fp64 reference of the prefix beam search (tests/ctc_beam_ref.py) against
a brute force over all alignments, its score against the exact CTC
log-probability, and beam = 1 on hand-made rows where the best path and the
best transcript differ."""
import numpy as np
import pytest

import ctc_beam_ref as ref


def _lp(T, A, seed, blank_bias=0.0):
    rng = np.random.default_rng([7, T, A, seed])
    acts = rng.standard_normal((T, A)) * 3
    acts[:, 0] += blank_bias
    return ref.log_softmax64(acts)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("bias", [0.0, 4.0])
def test_unpruned_search_is_the_brute_force(T, seed, bias):
    """A = 3, T <= 5: at most 1 + 2 + ... + 2^5 = 63 prefixes exist, beam 64 prunes nothing"""
    lp = _lp(T, 3, seed, bias)
    hyp, score = ref.beam_search(lp, 64, 2)
    table = ref.brute_force(lp)
    best = max(table, key=lambda k: table[k])
    assert tuple(hyp) == best
    assert abs(score - table[best]) < 1e-9
    assert abs(ref.exact_logprob(lp, hyp) - table[best]) < 1e-9
    # the alpha recursion against the brute force for every label sequence
    for k, v in table.items():
        assert abs(ref.exact_logprob(lp, list(k)) - v) < 1e-9, k


def test_unpruned_search_blank_last():
    lp = _lp(5, 3, 3)
    hyp, score = ref.beam_search(lp, 64, 2, blank=2)
    table = ref.brute_force(lp, blank=2)
    best = max(table, key=lambda k: table[k])
    assert tuple(hyp) == best and abs(score - table[best]) < 1e-9


@pytest.mark.parametrize("beam", [1, 2, 3, 5])
@pytest.mark.parametrize("symbols", [1, 2, 4])
@pytest.mark.parametrize("bias", [0.0, 4.0])
def test_pruned_score_is_a_lower_bound(beam, symbols, bias):
    lp = _lp(12, 5, beam * 10 + symbols, bias)
    hyp, score = ref.beam_search(lp, beam, symbols)
    assert all(0 < v < 5 for v in hyp) and len(hyp) <= 12
    assert score <= ref.exact_logprob(lp, hyp) + 1e-9


def test_beam_one_best_path_and_best_transcript_differ():
    """Two frames, A = 3.  The best path is blank, blank (0.4 * 0.4 = 0.16 -> the
    empty transcript), but label 1 collects 1-blank, blank-1 and 1-1:
    0.3 * 0.4 + 0.4 * 0.3 + 0.3 * 0.3 = 0.33.  A full search returns [1].
    beam = 1 keeps only the empty prefix after frame 0 (0.4 against 0.3), so
    after frame 1 it holds the better of "" (0.16) and "1" reached from ""
    (0.4 * 0.3 = 0.12): the empty transcript with score log 0.16."""
    p = np.array([[0.4, 0.3, 0.3], [0.4, 0.3, 0.3]])
    lp = np.log(p)
    hyp, score = ref.beam_search(lp, 64, 2)
    assert hyp == [1] and abs(score - np.log(0.33)) < 1e-12
    hyp, score = ref.beam_search(lp, 1, 2)
    assert hyp == [] and abs(score - np.log(0.16)) < 1e-12
    assert ref.collapse(np.argmax(lp, axis=1)) == []

    # three frames 1, 1, then a weak blank between them: the best path 1 1 1
    # collapses to [1]; beam 1 follows the prefix [1] and adds up its stay mass
    p = np.array([[0.1, 0.8, 0.1], [0.45, 0.5, 0.05], [0.1, 0.8, 0.1]])
    lp = np.log(p)
    hyp, score = ref.beam_search(lp, 1, 2)
    # frame 0: "1" (0.8).  frame 1: "1" stays with b = 0.36, nb = 0.4.  frame 2:
    # "1" b = 0.076, nb = 0.8 * 0.4 = 0.32 -> 0.396 against "1 1" = 0.8 * 0.36 = 0.288
    assert hyp == [1] and abs(score - np.log(0.396)) < 1e-12
    assert score <= ref.exact_logprob(lp, hyp)


def test_merge_adds_the_extension_to_the_entry_it_equals():
    """after frame 0 the beam holds "" and "1"; in frame 1 the extension "" + 1 is the entry "1" """
    p = np.array([[0.5, 0.5], [0.5, 0.5]])
    hyp, score = ref.beam_search(np.log(p), 4, 1)
    # "1": 1-blank, blank-1, 1-1 = 0.75; "": 0.25; "1 1" needs a blank between: impossible in 2 frames
    assert hyp == [1] and abs(score - np.log(0.75)) < 1e-12


def test_empty_utterance():
    hyp, score, _ = ref.decode(np.zeros((0, 5), np.float32), 4, 4)
    assert hyp == [] and score == 0.0
    assert ref.exact_logprob(np.zeros((0, 5)), []) == 0.0
