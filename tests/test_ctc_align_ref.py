"""The alignment reference (tests/ctc_align_ref.py) against brute force: on
tiny cases its score is the maximum over every path that collapses to the
labels, and on all-zero activations its path is the one the tie rule
dictates."""
import itertools

import numpy as np
import pytest

import ctc_align_ref as ref


def _tiny_cases():
    rng = np.random.default_rng(11)
    cases = []
    for i in range(30):
        T = int(rng.integers(1, 7))
        L = int(rng.integers(0, 4))
        labels = [int(v) for v in rng.integers(1, 3, size=L)]  # A = 3: repeats are frequent
        acts = (rng.standard_normal((T, 3)) * 3).astype(np.float32)
        cases.append((acts, labels))
    return cases


def test_reference_matches_brute_force():
    n_feasible = n_infeasible = 0
    for acts, labels in _tiny_cases():
        T, A = acts.shape
        path, score, lp = ref.align(acts, labels)
        best = -np.inf
        for p in itertools.product(range(A), repeat=T):
            if ref.collapse(p) == labels:
                best = max(best, float(sum(lp[t, a] for t, a in enumerate(p))))
        if not ref.feasible(T, labels):
            n_infeasible += 1
            assert best == -np.inf  # the feasibility rule is exact: no path collapses to the labels
            assert score == -np.inf and np.all(path == -1)
            continue
        n_feasible += 1
        assert ref.collapse(path) == labels
        assert np.isclose(score, best, rtol=1e-12, atol=1e-12)
        assert np.isclose(sum(lp[t, a] for t, a in enumerate(path)), score, rtol=1e-12, atol=1e-12)
    assert n_feasible >= 10 and n_infeasible >= 3  # both kinds are among the 30


@pytest.mark.parametrize("T,labels,expect", [
    (5, [1, 2], [1, 2, 0, 0, 0]),
    (4, [1, 1], [1, 0, 1, 0]),
])
def test_reference_tie_rule(T, labels, expect):
    path, score, _ = ref.align(np.zeros((T, 3), np.float32), labels)
    assert path.tolist() == expect
    assert np.isclose(score, -T * np.log(3.0), rtol=1e-12)
