"""The operand pack passes (csrc/x3p_pack.hip: x3p_pack_rows, x3p_pack_cols,
bf16_pack_rows, bf16_pack_cols) through the kcm_test_pack hook, bit for bit
against their numpy restatement in pack_ref.py: the packed halves as uint16,
the exponents as int32.  Through a GEMM's accuracy bar a lost lo half or a
misplaced pad only looks like slightly worse precision.

Rows (or columns) span 1e-12 .. 1e6 as in test_gemm_x3_matches_numpy, a fifth
of the elements are up to 1e-8 smaller again, so that lo and hi halves reach
the fp16 subnormals and zero, and one row (column) is all zero.  The source's
row padding holds NaN, the output buffers 0xFFFF halves (a NaN) and a guard
tail that must stay as it was."""
import numpy as np
import pytest

import pack_ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

X3P_ROWS, X3P_COLS, BF16_ROWS, BF16_COLS = 0, 1, 2, 3
FILL16, FILL_E, GUARD = 0xFFFF, -7777, 256
ROW_KINDS = [("x3p", X3P_ROWS), ("bf16", BF16_ROWS)]
COL_KINDS = [("x3p", X3P_COLS), ("bf16", BF16_COLS)]


def data(rng, rows, cols, axis, unit=False):
    """rows x cols values whose scale varies along `axis` (0: per row, 1: per
    column); unit: inside (-1, 1), for a bound of 1."""
    if unit:
        X = rng.uniform(-1, 1, (rows, cols)) * 10.0 ** rng.uniform(-8, 0, (rows, cols))
    else:
        X = rng.standard_normal((rows, cols))
        scale = 10.0 ** rng.uniform(-12, 6, rows if axis == 0 else cols)
        X = X * (scale[:, None] if axis == 0 else scale[None, :])
        small = rng.random((rows, cols)) < 0.2
        X = np.where(small, X * 10.0 ** rng.uniform(-8, 0, (rows, cols)), X)
    X = X.astype(np.float32)
    n = rows if axis == 0 else cols
    if n > 1:
        if axis == 0:
            X[n // 2, :] = 0
        else:
            X[:, n // 2] = 0
    return X


def source(mats, base, ldx, sX):
    """The flat source buffer of mats [batch][rows][cols], NaN wherever no element lies."""
    batch, rows, cols = mats.shape
    buf = np.full(base + (batch - 1) * sX + rows * ldx + 8, np.nan, np.float32)
    for b in range(batch):
        o = base + b * sX
        buf[o:o + rows * ldx].reshape(rows, ldx)[:, :cols] = mats[b]
    return buf


def run(kctc, gpu, kind, buf, base, ldx, R, KC, out_n, e_n, shift=0, bound=0.0, batch=1, sX=0, sOut=0, sE=0,
        cmax=None, avoid=False, rc_want=0):
    """-> (out as uint16, eout as int32 or None), each with its guard tail."""
    import torch
    dX = torch.from_numpy(buf).to(gpu)
    dO = torch.from_numpy(np.full(out_n + GUARD, FILL16, np.uint16).view(np.int16)).to(gpu)
    x3p = kind in (X3P_ROWS, X3P_COLS)
    dE = torch.from_numpy(np.full(e_n + GUARD, FILL_E, np.int32)).to(gpu) if x3p else None
    dM = torch.from_numpy(np.ascontiguousarray(cmax, np.float32).view(np.int32)).to(gpu) if cmax is not None else None
    dA = torch.zeros(2, dtype=torch.int32, device=gpu) if avoid else None  # the avoid word and the item counter
    rc = kctc.lib().kcm_test_pack(None, kind, dX.data_ptr() + 4 * base, ldx, R, KC, shift, bound, batch, sX, sOut, sE,
                                  dO.data_ptr(), dE.data_ptr() if x3p else None,
                                  dM.data_ptr() if dM is not None else None, dA.data_ptr() if avoid else None,
                                  dA.data_ptr() + 4 if avoid else None)
    assert rc == rc_want
    if avoid:
        assert dA.cpu().numpy()[0] == 0  # the word is only read
    return dO.cpu().numpy().view(np.uint16), dE.cpu().numpy() if x3p else None


def check(got, parts, n, fill):
    """got == the buffer of n `fill` values (+ guard) with each (offset, values) of parts laid in."""
    want = np.full(n + GUARD, fill, got.dtype)
    for off, vals in parts:
        want[off:off + vals.size] = vals.ravel()
    np.testing.assert_array_equal(got, want)


def pack_rows(kctc, gpu, kind, mats, ldx, base=0, sX=0, gap=0, bound=0.0):
    batch, R, K = mats.shape
    ref = [pack_ref.x3p_rows(m, bound) if kind == X3P_ROWS else (pack_ref.bf16_rows(m), None) for m in mats]
    per = ref[0][0].size
    assert per == R * -(-K // (32 if kind == X3P_ROWS else 64)) * 64
    sOut, sE = (per + gap, R + gap) if batch > 1 else (0, 0)
    out_n, e_n = (batch - 1) * sOut + per, (batch - 1) * sE + R
    out, e = run(kctc, gpu, kind, source(mats, base, ldx, sX), base, ldx, R, K, out_n, e_n, bound=bound, batch=batch,
                 sX=sX, sOut=sOut, sE=sE)
    check(out, [(b * sOut, ref[b][0]) for b in range(batch)], out_n, FILL16)
    if kind == X3P_ROWS:
        check(e, [(b * sE, ref[b][1]) for b in range(batch)], e_n, FILL_E)


@pytest.mark.parametrize("K", [5, 33, 256, 257, 1000, 4096])
@pytest.mark.parametrize("name,kind", ROW_KINDS)
def test_pack_rows(kctc, gpu, name, kind, K):
    """Each register width of the row kernels (256 .. 4096 values a row) and
    the zero pad up to the k block; K % 4 decides the load path."""
    rng = np.random.default_rng(K)
    for R in (1, 4, 5, 130):
        pack_rows(kctc, gpu, kind, data(rng, R, K, 0)[None], K)


@pytest.mark.parametrize("K,ldx,base", [(257, 260, 0), (256, 259, 0), (256, 256, 1), (1000, 1004, 0)])
@pytest.mark.parametrize("name,kind", ROW_KINDS)
def test_pack_rows_load_paths(kctc, gpu, name, kind, K, ldx, base):
    """16-B loads with a scalar tail (K = 257 in rows 260 apart), scalar loads
    through ldx % 4 and through a base one float off 16 B."""
    pack_rows(kctc, gpu, kind, data(np.random.default_rng(ldx + base), 5, K, 0)[None], ldx, base=base)


@pytest.mark.parametrize("sX", [5 * 260 + 4, 5 * 260 + 5])
@pytest.mark.parametrize("name,kind", ROW_KINDS)
def test_pack_rows_batch(kctc, gpu, name, kind, sX):
    """batch = 2 with sX, sOut and sE; an sX that is no multiple of 4 turns the 16-B loads off."""
    rng = np.random.default_rng(sX)
    pack_rows(kctc, gpu, kind, np.stack([data(rng, 5, 257, 0), data(rng, 5, 257, 0)]), 260, sX=sX, gap=64)


@pytest.mark.parametrize("R,K", [(5, 257), (130, 33)])
def test_pack_rows_bound(kctc, gpu, R, K):
    """bound = 1: every row gets e = 13 whatever it holds."""
    pack_rows(kctc, gpu, X3P_ROWS, data(np.random.default_rng(R), R, K, 0, unit=True)[None], K, bound=1.0)


@pytest.mark.parametrize("name,kind", ROW_KINDS)
def test_pack_rows_too_long(kctc, gpu, name, kind):
    """A row holds at most 4096 values: K = 4097 is refused and nothing is written."""
    X = data(np.random.default_rng(1), 1, 4097, 0)[None]
    out, e = run(kctc, gpu, kind, source(X, 0, 4097, 0), 0, 4097, 1, 4097, 130 * 64, 1, rc_want=1)
    check(out, [], 130 * 64, FILL16)
    if e is not None:
        check(e, [], 1, FILL_E)


def pack_cols(kctc, gpu, kind, X, ldx, base, shift, bound=0.0, avoid=False):
    R, Cn = X.shape
    cmax = np.abs(X).max(axis=0) if kind == X3P_COLS and not bound > 0 else None
    if kind == X3P_COLS:
        ref, ref_e = pack_ref.x3p_cols(X, shift, cmax, bound)
    else:
        ref, ref_e = pack_ref.bf16_cols(X, shift), None
    assert ref.size == Cn * -(-R // (32 if kind == X3P_COLS else 64)) * 64
    out, e = run(kctc, gpu, kind, source(X[None], base, ldx, 0), base, ldx, R, Cn, ref.size, Cn, shift=shift,
                 bound=bound, cmax=cmax, avoid=avoid)
    check(out, [(0, ref)], ref.size, FILL16)
    if kind == X3P_COLS:
        check(e, [(0, ref_e)], Cn, FILL_E)
    return out, e


def cols_cases(kctc, gpu, kind, R, Cn):
    rng = np.random.default_rng(1000 * R + Cn + kind)
    X = data(rng, R, Cn, 1)
    ld4 = (Cn + 3) // 4 * 4
    for shift in (0, 3, -3, R, -R):
        out, _ = pack_cols(kctc, gpu, kind, X, ld4, 0, shift)  # 16-B loads
        pack_cols(kctc, gpu, kind, X, ld4 + 1, 0, shift)       # scalar loads through ldx % 4
        if abs(shift) == R:
            assert not np.any(out[:-GUARD])                    # every packed value is zero
    pack_cols(kctc, gpu, kind, X, ld4, 1, 3)                   # scalar loads through the base


@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
@pytest.mark.parametrize("R", [1, 31, 32, 33, 70])
def test_pack_cols_x3p(kctc, gpu, R, Cn):
    """The k axis is X's rows: R around the 32-k block, the shift with zero
    fill at both ends, exponents from the column maxima (np.abs(X).max(0), so
    that a failure points at the pack and not at absmax)."""
    cols_cases(kctc, gpu, X3P_COLS, R, Cn)


@pytest.mark.parametrize("Cn", [1, 63, 65, 130])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 130])
def test_pack_cols_bf16(kctc, gpu, R, Cn):
    cols_cases(kctc, gpu, BF16_COLS, R, Cn)


@pytest.mark.parametrize("shift", [0, 3, -3])
def test_pack_cols_bound(kctc, gpu, shift):
    """bound = 1 and no cmax: the weight gradient's call on frame chunks (shift = +N and -N)."""
    X = data(np.random.default_rng(shift + 5), 70, 65, 1, unit=True)
    _, e = pack_cols(kctc, gpu, X3P_COLS, X, 68, 0, shift, bound=1.0)
    assert np.all(e[:65] == 13)


def test_pack_cols_avoid(kctc, gpu):
    """The counter-driven PackAvoid grid with a zeroed word (no block leaves):
    Cn = 130, R = 700 is 3 x 22 = 66 items, more than one run of 8 a block;
    bit-equal to the plain launch (and both to the restatement).  Non-zero
    words depend on the device's XCD partition and are left out."""
    X = data(np.random.default_rng(700), 700, 130, 1)
    plain = pack_cols(kctc, gpu, X3P_COLS, X, 132, 0, 3)
    avoid = pack_cols(kctc, gpu, X3P_COLS, X, 132, 0, 3, avoid=True)
    np.testing.assert_array_equal(avoid[0], plain[0])
    np.testing.assert_array_equal(avoid[1], plain[1])
