"""Self-checks of tests/lda_ref.py, the numpy restatement of LdaEstimate /
FeatureTransformEstimate that the LDA tests compare with: the transform
whitens the within-class covariance and diagonalises the between-class one,
the offset column removes the mean, and the reference's SVD route and the
eigh route give the same matrix."""
import numpy as np
import pytest

import lda_ref


def _sampled(D, C, R, seed):
    x, cls = lda_ref.sampled_data(D, C, R, seed)
    return lda_ref.accumulate(x, cls, None, C)


@pytest.mark.parametrize("D,C", [(1, 3), (7, 12), (40, 9), (40, 60)])
def test_transform_whitens_within_and_diagonalises_between(D, C):
    zero, first, second = _sampled(D, C, 4000, seed=D + C)
    total, between, mean, count = lda_ref.get_stats(zero, first, second)
    assert count == 4000
    m = lda_ref.estimate_internal(total, between, mean, within_class_factor=1.0, max_singular_value=0.0)
    a, off = m[:, :D], m[:, D]
    np.testing.assert_allclose(a @ (total - between) @ a.T, np.eye(D), atol=1e-9)
    b = a @ between @ a.T
    d = np.diag(b)
    np.testing.assert_allclose(b, np.diag(d), atol=1e-9)
    assert np.all(np.diff(d) <= 1e-9)                      # descending
    assert np.all(d[min(D, C - 1):] < 1e-9)                # rank of the between-class covariance
    np.testing.assert_allclose(off, -a @ mean, rtol=0, atol=1e-12)


@pytest.mark.parametrize("D", [1, 2, 7, 40, 120])
def test_svd_route_equals_eigh_route(D):
    zero, first, second = lda_ref.separated_stats(D, seed=D)
    for kw in ({}, {"within_class_factor": 1.0, "max_singular_value": 0.0}, {"dim": max(1, D // 2)}):
        a = lda_ref.fix_signs(lda_ref.estimate(zero, first, second, route="eigh", **kw))
        b = lda_ref.fix_signs(lda_ref.estimate(zero, first, second, route="svd", **kw))
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-10 * np.abs(a).max())


def test_separated_stats_have_the_eigenvalues_they_were_built_with():
    zero, first, second = lda_ref.separated_stats(40, seed=1)
    total, between, _, _ = lda_ref.get_stats(zero, first, second)
    d, _, _ = lda_ref.whitened_eig(total, between)
    np.testing.assert_allclose(d, 4.0 * 0.9 ** np.arange(40), rtol=1e-9)


def test_mangle_and_policies():
    zero, first, second = _sampled(5, 3, 50, seed=2)
    z32, f32, p32 = lda_ref.mangle(zero, first, second)
    assert p32.shape == (15,) and z32.dtype == f32.dtype == p32.dtype == np.float32
    ali = [0, 0, 3, 0, 0, 5, -1, 0, 7, 0, 0]
    assert lda_ref.frame_classes(ali, "skip").tolist() == [-1, -1, 3, -1, -1, 5, -1, -1, 7, -1, -1]
    assert lda_ref.frame_classes(ali, "class").tolist() == ali
    assert lda_ref.frame_classes(ali, "fill").tolist() == [3, 3, 3, 5, 5, 5, -1, 7, 7, 7, 7]
    assert lda_ref.frame_classes([0, 0], "fill").tolist() == [-1, -1]
    x = np.arange(8, dtype=np.float64).reshape(4, 2)
    s = lda_ref.splice(x, (-1, 0, 2))
    assert s.shape == (4, 6)
    assert s[0].tolist() == [0, 1, 0, 1, 4, 5] and s[3].tolist() == [4, 5, 6, 7, 6, 7]
