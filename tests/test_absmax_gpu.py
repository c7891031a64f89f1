"""absmax_f32 (csrc/gemm.hip) through the kcm_test_absmax hook: the row and
column maxima of |X| as float bits, bit-equal to np.abs(X).max(axis).

A block covers 64 rows and walks the columns 1024 at a time; beyond 64 rows
the blocks' column maxima merge by atomicMax on the float bits, beyond 1024
columns a row's maximum does.  x3p_pack_cols takes its exponents from cmax.

The data has a maximum that is a negative entry, an all-zero row and column,
-0.0, a column whose maximum is an fp32 subnormal and +inf in one column.  No
NaN: fmaxf drops it and no caller defines that case."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

SENTINEL = 0xDEADBEEF
GUARD = 32
ROWS = [1, 63, 65, 130]
COLS = [1, 63, 64, 65, 1024, 1025, 2100]


def make(rng, rows, cols):
    X = rng.standard_normal((rows, cols)).astype(np.float32)
    X[0, 0] = -1000.0  # the maximum of row 0 and of column 0 is a negative entry
    if rows > 1:
        X[1, :] = 0.0  # an all-zero row
    if cols > 1:
        X[:, 1] = 0.0  # an all-zero column
        X[rows - 1, 1] = -0.0
    if cols > 2:
        X[:, 2] = 0.0  # a column whose maximum is an fp32 subnormal
        X[rows // 2, 2] = -1e-40
        assert 0 < abs(X[rows // 2, 2]) < np.finfo(np.float32).tiny
    if cols > 3:
        X[rows - 1, cols - 1] = np.inf
    return X


def run(kctc, gpu, X, ldx, want_r, want_c, sX=0, sR=0, sC=0):
    """X [batch][rows][cols]; returns the (rmax, cmax) buffers, guard included."""
    import torch
    batch, rows, cols = X.shape
    # the row padding holds a value that would win any maximum it leaked into (fmaxf would drop a NaN)
    buf = np.full((batch - 1) * sX + rows * ldx + GUARD, 3e38, np.float32)
    for b in range(batch):
        buf[b * sX:b * sX + rows * ldx].reshape(rows, ldx)[:, :cols] = X[b]
    dX = torch.from_numpy(buf).to(gpu)
    mk = lambda n: torch.from_numpy(np.full(n, SENTINEL, np.uint32).view(np.int32)).to(gpu)
    dR = mk((batch - 1) * sR + rows + GUARD) if want_r else None
    dC = mk((batch - 1) * sC + cols + GUARD) if want_c else None
    rc = kctc.lib().kcm_test_absmax(None, dX.data_ptr(), ldx, rows, cols, dR.data_ptr() if want_r else None,
                                    dC.data_ptr() if want_c else None, batch, sX, sR, sC)
    assert rc == 0
    back = lambda t: t.cpu().numpy().view(np.uint32) if t is not None else None
    return back(dR), back(dC)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_absmax(kctc, gpu, rows, cols):
    X = make(np.random.default_rng(rows * 10000 + cols), rows, cols)[None]
    ref_r, ref_c = bits(np.abs(X[0]).max(axis=1)), bits(np.abs(X[0]).max(axis=0))
    for want_r, want_c in [(True, False), (False, True), (True, True)]:
        r, c = run(kctc, gpu, X, cols + 3, want_r, want_c)
        if want_r:
            np.testing.assert_array_equal(r[:rows], ref_r)
            assert np.all(r[rows:] == SENTINEL)
        if want_c:
            np.testing.assert_array_equal(c[:cols], ref_c)
            assert np.all(c[cols:] == SENTINEL)


@pytest.mark.parametrize("rows,cols", [(65, 63), (130, 1025)])
def test_absmax_batch(kctc, gpu, rows, cols):
    """batch = 2 with all three strides.  cmax is overwritten inside [0, cols)
    of each batch (no stale sentinel survives the merge) and untouched past
    the range absmax_f32 clears, strideC (batch - 1) + cols; rmax is untouched
    between the batches' rows."""
    rng = np.random.default_rng(rows + cols)
    X = np.stack([make(rng, rows, cols), 3.0 * make(rng, rows, cols)])
    ldx, sX, sR, sC = cols + 5, rows * (cols + 5) + 7, rows + 2, cols + 9
    r, c = run(kctc, gpu, X, ldx, True, True, sX, sR, sC)
    for b in range(2):
        np.testing.assert_array_equal(r[b * sR:b * sR + rows], bits(np.abs(X[b]).max(axis=1)))
        np.testing.assert_array_equal(c[b * sC:b * sC + cols], bits(np.abs(X[b]).max(axis=0)))
    assert np.all(r[rows:sR] == SENTINEL) and np.all(r[sR + rows:] == SENTINEL)
    assert np.all(c[sC + cols:] == SENTINEL)
