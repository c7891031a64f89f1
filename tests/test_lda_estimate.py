"""The host half of the LDA estimate (include/kaldi_lda.h), no GPU:
estimate_feature_transform against tests/lda_ref.py, LdaEstimate's accumulator
files, and the argument checks.

Tolerance of the row comparison: the reference rounded to float32, within 8
float32 ulps of each row's largest magnitude.  Rows are eigenvectors, so the
fixtures (lda_ref.separated_stats) are built with eigenvalues 4 * 0.9^k -- a
relative gap of 0.1 between neighbours -- and every case checks that gap
(>= 0.05) and that the reference's own two routes agree within a tenth of the
tolerance before it compares anything."""
import ctypes
import os

import numpy as np
import pytest

import lda_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lda_accs_small.bin")


def _row_tol(ref32):
    return 8.0 * np.spacing(np.abs(ref32).max(axis=1).astype(np.float32)).astype(np.float64)[:, None]


def _check_against_ref(kctc, stats, **kw):
    zero, first, second = stats
    D = first.shape[1]
    target = D if kw.get("dim", -1) <= 0 else kw["dim"]
    total, between, _, _ = lda_ref.get_stats(zero, first, second)
    d, _, _ = lda_ref.whitened_eig(total, between)
    k = np.arange(min(target, D - 1))
    assert np.all((d[k] - d[k + 1]) >= 0.05 * d[k]), "fixture: eigenvalues not separated"
    ref = lda_ref.fix_signs(lda_ref.estimate(zero, first, second, route="eigh", **kw))
    ref32 = ref.astype(np.float32).astype(np.float64)
    tol = _row_tol(ref32)
    other = lda_ref.fix_signs(lda_ref.estimate(zero, first, second, route="svd", **kw))
    assert np.all(np.abs(other - ref) <= 0.1 * tol), "fixture: the reference's two routes disagree"
    M, chol = kctc.estimate_feature_transform(zero, first, second, **kw)
    assert M.dtype == np.float32 and M.shape == ref.shape
    got = lda_ref.fix_signs(M)
    err = np.abs(got - ref32)
    assert np.all(err <= tol), (float((err / tol).max()), kw)
    L, _ = lda_ref.within_cholesky(total, between)
    assert np.all(np.triu(chol, 1) == 0)
    np.testing.assert_allclose(chol, L, rtol=0, atol=1e-12 * np.abs(L).max())
    return M


@pytest.mark.parametrize("D", [1, 2, 7, 40, 120])
@pytest.mark.parametrize("half", [False, True])
def test_estimate_matches_reference_every_option(kctc, D, half):
    stats = lda_ref.separated_stats(D, seed=10 + D)      # includes a class with zero count
    dim = max(1, D // 2) if half else -1
    for wcf in (1.0, 0.001):
        for remove_offset in (True, False):
            for max_sv in (0.0, 5.0):
                _check_against_ref(kctc, stats, dim=dim, within_class_factor=wcf, remove_offset=remove_offset,
                                   max_singular_value=max_sv)


@pytest.mark.parametrize("D", [7, 40])
def test_estimate_where_the_ceiling_bites(kctc, D):
    stats = lda_ref.separated_stats(D, seed=3, cov_scale=0.01)
    plain = lda_ref.estimate(*stats, within_class_factor=1.0, max_singular_value=0.0, remove_offset=False)
    assert np.linalg.svd(plain, compute_uv=False).max() > 5.0
    for wcf in (1.0, 0.001):
        M = _check_against_ref(kctc, stats, within_class_factor=wcf, max_singular_value=5.0)
        s = np.linalg.svd(M[:, :D].astype(np.float64), compute_uv=False)
        assert s.max() <= 5.0 * (1 + 1e-6) and np.sum(s > 5.0 * (1 - 1e-6)) >= 1


@pytest.mark.parametrize("D", [2, 7, 40])
def test_estimate_takes_the_smoothing_retry(kctc, D):
    stats = lda_ref.separated_stats(D, seed=5, dead_dim=True)
    total, between, _, _ = lda_ref.get_stats(*stats)
    assert lda_ref.within_cholesky(total, between)[1], "fixture: Cholesky did not fail"
    _check_against_ref(kctc, stats)
    _check_against_ref(kctc, stats, dim=max(1, D // 2), within_class_factor=1.0, max_singular_value=0.0)


def test_estimate_invariants_where_eigenvalues_coincide(kctc):
    """4 classes in 12 dimensions: 9 eigenvalues are zero and their rows are any
    basis of the null space, so the invariants are compared, not the rows.
    Bound: M is float32, so M W M^T is off by at most 2 * 2^-24 * |M| |W| |M|^T
    (two roundings of M per term), plus fp64 noise."""
    x, cls = lda_ref.sampled_data(12, 4, 3000, seed=8)
    zero, first, second = lda_ref.accumulate(x, cls, None, 4)
    total, between, mean, _ = lda_ref.get_stats(zero, first, second)
    M, _ = kctc.estimate_feature_transform(zero, first, second, within_class_factor=1.0, max_singular_value=0.0)
    a = M[:, :12].astype(np.float64)
    for cov, want in ((total - between, np.eye(12)), (between, None)):
        got = a @ cov @ a.T
        bound = 2.0 * 2.0 ** -24 * (np.abs(a) @ np.abs(cov) @ np.abs(a).T) + 1e-10
        if want is None:
            d = lda_ref.whitened_eig(total, between)[0]
            want = np.diag(np.where(np.arange(12) < 3, d, 0.0))
        assert np.all(np.abs(got - want) <= bound)
    off_bound = 2.0 ** -24 * (np.abs(a) @ np.abs(mean) + np.abs(M[:, 12])) + 1e-12
    assert np.all(np.abs(M[:, 12] + a @ mean) <= off_bound)


def test_handle_estimate_equals_module_function(kctc):
    stats = lda_ref.separated_stats(7, seed=2)
    h = kctc.LdaStats(7, len(stats[0]))
    h.set_stats(*stats)
    for got, want in zip(h.stats(), stats):
        assert np.array_equal(got, want)
    M1, c1 = h.estimate(dim=3)
    M2, c2 = kctc.estimate_feature_transform(*stats, dim=3)
    assert np.array_equal(M1, M2) and np.array_equal(c1, c2) and M1.shape == (3, 8)
    h.close()


# ---- accumulator files ------------------------------------------------------
def _sampled_stats(D, C, seed):
    x, cls = lda_ref.sampled_data(D, C + 1, 500, seed)
    cls[cls == C] = 0                                   # class C never occurs
    return lda_ref.accumulate(x, cls, None, C + 1)


def _unmangled(z32, f32, p32):
    """LdaEstimate::Read's arithmetic on the stored floats"""
    D = f32.shape[1]
    s = np.zeros((D, D))
    s[np.tril_indices(D)] = p32.astype(np.float64)
    s = s + np.tril(s, -1).T
    z, f = z32.astype(np.float64), f32.astype(np.float64)
    for c in range(len(z)):
        if z[c] != 0.0:
            s += (1.0 / z[c]) * np.outer(f[c], f[c])
    return z, f, s


@pytest.mark.parametrize("binary", [True, False])
def test_write_then_read_reproduces_the_stored_floats(kctc, tmp_path, binary):
    D, C = 9, 5
    stats = _sampled_stats(D, C, seed=4)
    h = kctc.LdaStats(D, C + 1)
    h.set_stats(*stats)
    path = str(tmp_path / "lda.acc")
    h.write(path, binary=binary)
    z32, f32, p32 = lda_ref.mangle(*stats)
    if binary:
        assert open(path, "rb").read() == lda_ref.accs_bytes(z32, f32, p32)
    else:
        assert open(path, "rb").read() == lda_ref.accs_text(z32, f32, p32)
    g = kctc.LdaStats(D, C + 1)
    g.read(path)
    # what was stored, exactly: mangling the read-back statistics gives the same floats
    want = _unmangled(z32, f32, p32)
    for got, w in zip(g.stats(), want):
        np.testing.assert_allclose(got, w, rtol=1e-15, atol=0)
    z2, f2, p2 = lda_ref.mangle(*g.stats())
    assert np.array_equal(z2, z32) and np.array_equal(f2, f32)
    np.testing.assert_allclose(p2, p32, rtol=2.0 ** -23, atol=0)   # mangling again rounds the sums once more
    once = g.stats()
    g.read(path, add=True)
    for got, w in zip(g.stats(), once):
        assert np.array_equal(got, 2.0 * w)
    g.read(path)                                         # add=False replaces
    for got, w in zip(g.stats(), once):
        assert np.array_equal(got, w)
    bad = kctc.LdaStats(D + 1, C + 1)
    with pytest.raises(kctc.KctcError, match="classes of dimension"):
        bad.read(path)


def _golden_numbers():
    """counts that are powers of two and small integers: every step of the
    mangling is exact, so the file reads back to these numbers bit for bit"""
    zero = np.array([2.0, 0.0, 4.0])
    first = np.array([[2.0, -4.0, 6.0], [0.0, 0.0, 0.0], [4.0, 8.0, -12.0]])
    packed = np.array([1.5, -0.25, 2.0, 0.5, 0.125, 3.0])
    return zero, first, packed


def test_golden_accs_file(kctc, tmp_path):
    zero, first, packed = _golden_numbers()
    z32, f32, p32 = zero.astype(np.float32), first.astype(np.float32), packed.astype(np.float32)
    data = open(GOLDEN, "rb").read()
    assert data == lda_ref.accs_bytes(z32, f32, p32)
    assert data.startswith(b"\0B<LDAACCS> <VECSIZE> \x04\x03\0\0\0<NUMCLASSES> \x04\x03\0\0\0<ZERO_ACCS> FV \x04\x03\0\0\0")
    assert data.endswith(b"</LDAACCS> ") and len(data) == 196
    h = kctc.LdaStats(3, 3)
    h.read(GOLDEN)
    z, f, s = h.stats()
    wz, wf, ws = _unmangled(z32, f32, p32)
    assert np.array_equal(z, wz) and np.array_equal(f, wf) and np.array_equal(s, ws)
    assert s[0, 0] == 1.5 + 2.0 * 2.0 / 2.0 + 4.0 * 4.0 / 4.0 and s[2, 1] == 0.125 - 4.0 * 6.0 / 2.0 - 8.0 * 12.0 / 4.0
    out = str(tmp_path / "again.bin")
    h.write(out, binary=True)
    assert open(out, "rb").read() == data


# ---- argument checks -------------------------------------------------------
def test_invalid_arguments_are_errors(kctc):
    zero, first, second = lda_ref.separated_stats(4, seed=1)
    C = len(zero)
    with pytest.raises(kctc.KctcError, match="output dimension"):
        kctc.estimate_feature_transform(zero, first, second, dim=5)
    with pytest.raises(kctc.KctcError, match="count"):
        kctc.estimate_feature_transform(np.zeros(C), first, second)
    for which in range(3):
        bad = [zero.copy(), first.copy(), second.copy()]
        bad[which].flat[0] = np.nan if which != 1 else np.inf
        with pytest.raises(kctc.KctcError, match="not finite"):
            kctc.estimate_feature_transform(*bad)
    L = kctc.lib()
    M = np.zeros((4, 5), np.float32)
    args = [zero.ctypes.data, first.ctypes.data, second.ctypes.data, 4, C, 5, 0.001, 1, 5.0, M.ctypes.data, None]
    assert L.kctc_lda_estimate_from_stats(*args) != 0 and b"output dimension" in L.kctc_last_error()
    args[5] = -1
    assert L.kctc_lda_estimate_from_stats(*args) == 0
    for k in (0, 1, 2, 9):
        a = list(args)
        a[k] = None
        assert L.kctc_lda_estimate_from_stats(*a) != 0 and b"null" in L.kctc_last_error()
    h = ctypes.c_void_p()
    assert L.kctc_lda_create(None, 4, 2, 0) != 0
    for dim, classes in ((0, 2), (2049, 2), (4, 0), (4, 16385)):
        assert L.kctc_lda_create(ctypes.byref(h), dim, classes, 0) != 0 and b"outside" in L.kctc_last_error()
    for dim, classes in ((-1, 2), (4, -5), (2049, 16385)):        # refused before anything is sized by them
        assert L.kctc_lda_create(ctypes.byref(h), dim, classes, 0) != 0 and b"outside" in L.kctc_last_error()
    with pytest.raises(kctc.KctcError, match="outside"):
        kctc.LdaStats(2049, 3)
    s = kctc.LdaStats(4, C)
    assert L.kctc_lda_get_stats(s._h, None, None, None) != 0
    assert L.kctc_lda_estimate(s._h, -1, 0.001, 1, 5.0, None, None) != 0
    with pytest.raises(kctc.KctcError, match="count"):
        s.estimate()                                     # nothing accumulated
    assert s.guards_intact()                             # nothing on a device yet
    s.close()
