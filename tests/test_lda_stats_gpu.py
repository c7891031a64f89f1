"""LdaStats.accumulate (include/kaldi_lda.h, csrc/lda_stats.hip) against
tests/lda_ref.py in fp64, at the smallest shapes where the 64 x 64 tiling, the
32-row stages and the 1024-row chunks can go wrong.

Tolerance (derived): every term w x_i x_j is rounded at most once in fp64 and
the sums differ from numpy's only in order, so elementwise
    |got - ref| <= (R + 4) * 2^-53 * sum_r |w_r x_ri x_rj|
and the same with |w_r x_ri| (rows of the class) for the class sums and |w_r|
for the counts; the counts are exact for integer-valued weights."""
import ctypes

import numpy as np
import pytest

import lda_ref

pytestmark = pytest.mark.gpu

DS = [1, 15, 16, 17, 40, 100, 360]
RS = [0, 1, 3, 63, 64, 65, 1000, 5000]      # 5000: five row chunks, the partial-sum path
CS = [1, 2, 41, 300]


def _inputs(D, R, seed):
    """rows, raw class draws, which rows are skipped (about a third, filled with
    NaN and Inf), and the weight variants"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, D)).astype(np.float32)
    draw = rng.integers(0, 1 << 20, R)
    skip = rng.random(R) < 1.0 / 3.0
    x[skip] = np.nan
    x[skip, ::2] = np.inf
    weights = {"none": None,
               "integer": rng.integers(0, 4, R).astype(np.float32),            # exact zeros among them
               "fraction": (rng.random(R) * (rng.random(R) > 0.2)).astype(np.float32)}
    return x, draw, skip, weights


def _ids(draw, skip, C):
    ids = (draw % max(1, C - 1)).astype(np.int32)   # C >= 2: class C - 1 never occurs
    ids[skip] = np.where(np.arange(len(ids)) % 2 == 0, -1, -7)[skip]
    return ids


def _dev(gpu, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _check(got, x, ids, w, C, R, exact_counts, cache=None):
    """cache: the second moments do not depend on C (the same rows are kept)"""
    zero, first, second = got
    keep = ids >= 0
    xa = np.abs(np.where(keep[:, None], x, 0.0))
    if cache is not None and "rs" in cache:
        rs, as_ = cache["rs"], cache["as"]
        xk = np.where(keep[:, None], x, 0.0).astype(np.float64)
        wk = np.where(keep, 1.0 if w is None else w, 0.0).astype(np.float64)
        rz, az = np.zeros(C), np.zeros(C)
        np.add.at(rz, ids[keep], wk[keep])
        az = rz.copy()
        onehot = np.zeros((len(ids), C))
        onehot[np.flatnonzero(keep), ids[keep]] = wk[keep]
        rf, af = onehot.T @ xk, onehot.T @ xa
    else:
        rz, rf, rs = lda_ref.accumulate(x, ids, w, C)
        az, af, as_ = lda_ref.accumulate(xa, ids, w, C)
        if cache is not None:
            cache["rs"], cache["as"] = rs, as_
    eps = (R + 4) * 2.0 ** -53
    assert np.array_equal(second, second.T)
    assert np.all(np.abs(second - rs) <= eps * as_), float(np.max(np.abs(second - rs) / np.maximum(eps * as_, 1e-300)))
    assert np.all(np.abs(first - rf) <= eps * af)
    if exact_counts:
        assert np.array_equal(zero, rz)
    else:
        assert np.all(np.abs(zero - rz) <= eps * az)
    assert np.all(np.isfinite(second)) and np.all(np.isfinite(first))


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("D", DS)
def test_accumulate_matches_reference(kctc, gpu, D, R):
    x, draw, skip, weights = _inputs(D, R, seed=1000 * D + R)
    xd = _dev(gpu, x)
    caches = {}
    for C in CS:
        ids = _ids(draw, skip, C)
        idd = _dev(gpu, ids)
        for name, w in weights.items():
            cache = caches.setdefault(name, {})
            h = kctc.LdaStats(D, C)
            h.accumulate(xd, idd, _dev(gpu, w))
            got = h.stats()
            assert h.guards_intact()
            _check(got, x, ids, w, C, R, exact_counts=name != "fraction", cache=cache)
            if C >= 2:
                assert got[0][C - 1] == 0 and not got[1][C - 1].any()
            h.close()


@pytest.mark.parametrize("D,R1,R2,C", [(17, 65, 1000, 41), (360, 3, 5000, 2), (40, 1024, 1025, 300)])
def test_two_calls_against_one_on_the_concatenation(kctc, gpu, D, R1, R2, C):
    x, draw, skip, weights = _inputs(D, R1 + R2, seed=D + R1)
    ids, w = _ids(draw, skip, C), weights["fraction"]
    two, one = kctc.LdaStats(D, C), kctc.LdaStats(D, C)
    two.accumulate(_dev(gpu, x[:R1]), _dev(gpu, ids[:R1]), _dev(gpu, w[:R1]))
    two.accumulate(_dev(gpu, x[R1:]), _dev(gpu, ids[R1:]), _dev(gpu, w[R1:]))
    one.accumulate(_dev(gpu, x), _dev(gpu, ids), _dev(gpu, w))
    for h in (two, one):
        _check(h.stats(), x, ids, w, C, R1 + R2, exact_counts=False)
        assert h.guards_intact()


def test_repeated_call_sequence_gives_identical_bytes(kctc, gpu):
    D, C = 100, 41
    parts = [_inputs(D, R, seed=R) for R in (5000, 65, 1000)]
    out = []
    for _ in range(2):
        h = kctc.LdaStats(D, C)
        for x, draw, skip, weights in parts:
            h.accumulate(_dev(gpu, x), _dev(gpu, _ids(draw, skip, C)), _dev(gpu, weights["fraction"]))
        out.append([a.tobytes() for a in h.stats()])
        again = [a.tobytes() for a in h.stats()]        # reading is not destructive
        assert again == out[-1]
        h.close()
    assert out[0] == out[1]


def test_many_classes_and_a_second_pass(kctc, gpu):
    """C at its limit; 1295 tiles leave 6 chunks to a pass, so 6149 rows take two
    launch pairs"""
    D, C, R = 300, 16384, 6149
    x, draw, skip, weights = _inputs(D, R, seed=9)
    ids = _ids(draw, skip, C)
    ids[np.flatnonzero(~skip)[0]] = C - 2
    h = kctc.LdaStats(D, C)
    h.accumulate(_dev(gpu, x), _dev(gpu, ids), None)
    _check(h.stats(), x, ids, None, C, R, exact_counts=True)
    assert h.guards_intact()
    h.close()


def test_out_of_range_ids_are_skipped_rows(kctc, gpu):
    D, C, R = 16, 3, 64
    x, draw, skip, _ = _inputs(D, R, seed=4)
    ids = _ids(draw, skip, C)
    wild = ids.copy()
    wild[skip] = np.where(np.arange(R) % 2 == 0, C, 1 << 30)[skip]   # ids >= C: selected out as well
    a, b = kctc.LdaStats(D, C), kctc.LdaStats(D, C)
    a.accumulate(_dev(gpu, x), _dev(gpu, ids))
    b.accumulate(_dev(gpu, x), _dev(gpu, wild))
    assert all(np.array_equal(p, q) for p, q in zip(a.stats(), b.stats()))


def test_bad_arguments_enqueue_nothing(kctc, gpu):
    import torch
    L = kctc.lib()
    with pytest.raises(kctc.KctcError, match="outside"):
        kctc.LdaStats(2049, 3)
    with pytest.raises(kctc.KctcError, match="outside"):
        kctc.LdaStats(3, 16385)
    D, C, R = 17, 5, 65
    x, draw, skip, _ = _inputs(D, R, seed=2)
    xd, idd = _dev(gpu, x), _dev(gpu, _ids(draw, skip, C))
    h = kctc.LdaStats(D, C)
    h.accumulate(xd, idd)
    before = [a.tobytes() for a in h.stats()]
    stream = torch.cuda.current_stream().cuda_stream
    assert L.kctc_lda_accumulate(h._h, stream, xd.data_ptr(), idd.data_ptr(), None, -1) != 0
    assert b"negative" in L.kctc_last_error()
    assert L.kctc_lda_accumulate(h._h, stream, None, idd.data_ptr(), None, R) != 0
    assert b"null" in L.kctc_last_error()
    assert L.kctc_lda_accumulate(h._h, stream, xd.data_ptr(), None, None, R) != 0
    assert L.kctc_lda_accumulate(None, stream, xd.data_ptr(), idd.data_ptr(), None, R) != 0
    assert L.kctc_lda_accumulate(h._h, stream, None, None, None, 0) == 0      # R = 0: a no-op
    torch.cuda.synchronize()
    assert [a.tobytes() for a in h.stats()] == before and h.guards_intact()
    with pytest.raises(ValueError):
        h.accumulate(xd[:, :5], idd)                     # not [R][dim]
    h.close()
