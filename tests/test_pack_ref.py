"""pack_ref.py, the numpy restatement of the pack passes, checked on the CPU:
the split reproduces its input to fp32 class, and the layout, the shift and
the zero pad land where a 3 x 5 example written out by hand says."""
import numpy as np
import pytest

import pack_ref


def test_split_reproduces_input():
    """x = 2^e v with max |x| < 2^14: hi = fp16(x) is off by <= 2^-11 |x| (or
    2^-25, a subnormal hi), lo = fp16(x - hi) by <= 2^-11 |x - hi| <= 2^-22 |x|
    (or 2^-25), and 2^-25 / 2^13 = 2^-38: 2^-e (hi + lo) is within 2^-21 of
    the row maximum with room to spare."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((40, 100)).astype(np.float32)
    X *= (10.0 ** rng.uniform(-12, 6, 40)).astype(np.float32)[:, None]
    X *= (10.0 ** rng.uniform(-8, 0, X.shape) * (rng.random(X.shape) < 0.2) + (rng.random(X.shape) < 0.8)).astype(
        np.float32)
    X[7] = 0
    P, e = pack_ref.x3p_rows(X)
    assert P.shape == (40, 4, 64) and P.dtype == np.uint16 and e.dtype == np.int32
    mx = np.abs(X).max(axis=1).astype(np.float64)
    scaled = np.ldexp(mx, e)
    assert e[7] == 14 and np.all((scaled[mx > 0] >= 2.0 ** 13) & (scaled[mx > 0] < 2.0 ** 14))
    back = pack_ref.x3p_unpack(P, e)
    assert np.all(back[:, 100:] == 0)
    assert np.all(np.abs(back[:, :100] - X) <= 2.0 ** -21 * mx[:, None])
    assert np.any(np.abs(back[:, :100] - X) > 0)  # the lo halves carry something: hi alone is 2^-11
    hi_only = np.ldexp(P.view(np.float16)[:, :, :32].astype(np.float64), -e[:, None, None]).reshape(40, -1)[:, :100]
    assert np.max(np.abs(hi_only - X) / np.where(mx > 0, mx, 1)[:, None]) > 2.0 ** -14


def test_bound_sets_the_exponent():
    X = np.array([[0.25, -0.5, 0.125]], np.float32)
    P, e = pack_ref.x3p_rows(X, bound=1.0)
    assert e.tolist() == [13]  # frexp(1.0) = (0.5, 1)
    assert P.view(np.float16)[0, 0, :4].tolist() == [2048.0, -4096.0, 1024.0, 0.0]


# X [3][5] with X[k][c] = (10 k + c + 1) / 8192; under a bound of 1 (e = 13)
# the scaled values are the integers 10 k + c + 1, exact in fp16 (lo = 0)
X35 = (np.array([[1, 2, 3, 4, 5], [11, 12, 13, 14, 15], [21, 22, 23, 24, 25]], np.float64) / 8192).astype(np.float32)
Z = [0.0]


@pytest.mark.parametrize("shift,want", [
    (0, [[1, 11, 21], [2, 12, 22], [3, 13, 23], [4, 14, 24], [5, 15, 25]]),
    (1, [[0, 1, 11], [0, 2, 12], [0, 3, 13], [0, 4, 14], [0, 5, 15]]),
    (-1, [[11, 21, 0], [12, 22, 0], [13, 23, 0], [14, 24, 0], [15, 25, 0]]),
    (2, [[0, 0, 1], [0, 0, 2], [0, 0, 3], [0, 0, 4], [0, 0, 5]]),
    (3, [[0, 0, 0]] * 5),
    (-3, [[0, 0, 0]] * 5),
])
def test_cols_shift_and_pad_by_hand(shift, want):
    P, e = pack_ref.x3p_cols(X35, shift=shift, bound=1.0)
    assert P.shape == (5, 1, 64) and e.tolist() == [13] * 5
    h = P.view(np.float16)[:, 0, :]
    for c in range(5):
        assert h[c, :32].tolist() == [float(v) for v in want[c]] + Z * 29  # hi, then the pad up to the block
        assert h[c, 32:].tolist() == Z * 32  # lo
    B = pack_ref.bf16_cols(X35 * 8192, shift=shift)
    assert B.shape == (5, 1, 64)
    f = (B.astype(np.uint32) << 16).view(np.float32)[:, 0, :]
    for c in range(5):
        assert f[c].tolist() == [float(v) for v in want[c]] + Z * 61


def test_rows_layout_by_hand():
    P, e = pack_ref.x3p_rows(X35, bound=1.0)
    assert P.shape == (3, 1, 64)
    h = P.view(np.float16)[:, 0, :]
    for r in range(3):
        assert h[r].tolist() == [float(10 * r + c + 1) for c in range(5)] + Z * 59
    # exponents from the data: the row maxima 5, 15, 25 (/ 8192) scale to [2^13, 2^14)
    P, e = pack_ref.x3p_rows(X35)
    assert e.tolist() == [24, 23, 22]
    assert P.view(np.float16)[:, 0, 4].tolist() == [5 * 2048.0, 15 * 1024.0, 25 * 512.0]
    # a second k block starts at k = 32: hi of k = 32 at half 64, its lo at 96
    row = np.arange(1, 34, dtype=np.float32)[None, :] / 8192
    P, _ = pack_ref.x3p_rows(row, bound=1.0)
    assert P.shape == (1, 2, 64)
    flat = P.view(np.float16).reshape(-1)
    assert flat[:32].tolist() == [float(v) for v in range(1, 33)] and flat[64] == 33.0
    assert np.all(flat[32:64] == 0) and np.all(flat[65:] == 0)
    B = pack_ref.bf16_rows(X35 * 8192)
    assert (B.astype(np.uint32) << 16).view(np.float32)[2, 0, :6].tolist() == [21.0, 22.0, 23.0, 24.0, 25.0, 0.0]


def test_bf16_rounds_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.5, np.inf], np.float32)
    # ties go to the even upper half: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6; just above a tie rounds up
    assert pack_ref.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xC020, 0x7F80]
