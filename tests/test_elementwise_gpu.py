"""The three small CuMatrix entries of include/kaldi_cumatrix.h that only the
train step reached: kcm_add_vec_clipped (k_clip_sgd), kcm_clip_gradient_rows
(k_rownorm_clip) and kcm_add_row_sum_mat (k_sum_rows + k_sum_partials),
against fp64 / exact integer references.

Every buffer a kernel writes lies inside a larger allocation whose margins (64
floats before and after) hold a sentinel that must survive."""
import numpy as np
import pytest

import clip_ref as cr
from clip_ref import ClipCfg

pytestmark = pytest.mark.gpu

MARGIN = 64
SENT = 12345.678
U = 2.0 ** -23


class Guarded:
    """A 1-D float32 (or int32) device view of n elements, `offset` elements
    past a 256-byte boundary, between two sentinel margins."""

    def __init__(self, gpu, n, offset=0, dtype=None):
        import torch
        dtype = dtype or torch.float32
        self.sent = SENT if dtype == torch.float32 else 123456789
        self.buf = torch.full((MARGIN + offset + n + MARGIN,), self.sent, dtype=dtype, device=gpu)
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.hi = MARGIN + offset, MARGIN + offset + n
        self.view = self.buf[self.lo:self.hi]
        assert self.view.data_ptr() % 16 == (4 * offset) % 16

    def set(self, a):
        import torch
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))
        return self

    def get(self):
        """The view's contents (numpy), after checking both margins."""
        import torch
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert bool((h[:self.lo] == self.sent).all()) and bool((h[self.hi:] == self.sent).all()), \
            "a write outside the buffer"
        return h[self.lo:self.hi].numpy().copy()


# ---------------------------------------------------------------------------
# kcm_add_vec_clipped: w += lr * clamp(dw, +-clip)
# ---------------------------------------------------------------------------
N_CAP = 4 * 256 * 4096 + 7        # one vector trip past the 4096-block grid cap, and a scalar tail of 3


def _vec_inputs(n, clip, seed):
    rng = np.random.default_rng([seed, n])
    w = rng.standard_normal(n).astype(np.float32)
    dw = rng.standard_normal(n).astype(np.float32)
    special = [clip, -clip, np.inf, -np.inf] if clip > 0 else [0.5, -0.5]
    # planted over the vector body, the last vector and the tail
    for k, i in enumerate(sorted(set([0, 1, n // 2, n - 6, n - 5, n - 2, n - 1]) & set(range(n)))):
        dw[i] = special[k % len(special)]
    return w, dw


def _check_add_vec(kctc, gpu, n, off_w, off_dw, lr, clip, seed=1):
    w0, dw = _vec_inputs(n, clip, seed)
    w = Guarded(gpu, n, off_w).set(w0)
    d = Guarded(gpu, n, off_dw).set(dw)
    kctc.add_vec_clipped(w.view, d.view, lr, clip)
    got = w.get().astype(np.float64)
    np.testing.assert_array_equal(d.get().view(np.uint32), dw.view(np.uint32))     # dw is read only
    x = dw.astype(np.float64)
    if clip > 0:
        x = np.clip(x, -float(np.float32(clip)), float(np.float32(clip)))
        assert np.isfinite(x).all() and (np.abs(x[np.isinf(dw)]) == np.float32(clip)).all()
    prod = float(np.float32(lr)) * x
    ref = w0.astype(np.float64) + prod
    # one rounding of the product and one of the sum (fused or not), factor 2 in hand
    bound = U * (np.abs(prod) + np.abs(ref))
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert np.isfinite(got).all() and (err <= bound).all(), (n, off_w, off_dw, lr, clip, worst)
    return worst        # measured on MI355X: at most 0.499 of the bound (n = 4194311)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, N_CAP])
def test_add_vec_clipped_sizes(kctc, gpu, n):
    worst = max(_check_add_vec(kctc, gpu, n, 0, 0, lr, 0.5) for lr in (-0.01, 0.3))
    print(f"add_vec_clipped n={n}: worst error / bound {worst:.3f}")


def test_add_vec_clipped_alignment_clip_and_sign(kctc, gpu):
    """n = 1025: w and dw each aligned or one float past 16 bytes (a misaligned
    pointer selects the scalar path), clip > 0 / 0 / < 0 (the last two: no
    clamp), lr of both signs."""
    worst = 0.0
    for off_w in (0, 1):
        for off_dw in (0, 1):
            for clip in (0.5, 0.0, -1.0):
                for lr in (0.3, -0.01):
                    worst = max(worst, _check_add_vec(kctc, gpu, 1025, off_w, off_dw, lr, clip, seed=2))
    print(f"add_vec_clipped alignments: worst error / bound {worst:.3f}")
    # no clamp really means none: a value of 100 moves w by lr * 100
    w = Guarded(gpu, 5).set(np.zeros(5, np.float32))
    d = Guarded(gpu, 5).set(np.full(5, 100.0, np.float32))
    kctc.add_vec_clipped(w.view, d.view, 0.5, -1.0)
    np.testing.assert_array_equal(w.get(), np.full(5, 50.0, np.float32))


def test_add_vec_clipped_empty_and_null(kctc, gpu):
    import torch
    w = Guarded(gpu, 4).set(np.arange(4, dtype=np.float32))
    d = Guarded(gpu, 4).set(np.ones(4, np.float32))
    s = torch.cuda.current_stream().cuda_stream
    L = kctc.lib()
    assert L.kcm_add_vec_clipped(s, w.view.data_ptr(), d.view.data_ptr(), 0, 1.0, 0.5) == 0
    assert L.kcm_add_vec_clipped(s, None, d.view.data_ptr(), 4, 1.0, 0.5) == 1
    assert L.kcm_add_vec_clipped(s, w.view.data_ptr(), None, 4, 1.0, 0.5) == 1
    np.testing.assert_array_equal(w.get(), np.arange(4, dtype=np.float32))


# ---------------------------------------------------------------------------
# kcm_clip_gradient_rows
# ---------------------------------------------------------------------------
CLIP_CASES = [(r, d, 0) for r, d in cr.SHAPES] + [(5, 64, 1), (33, 256, 1)]   # (rows, dim, base offset in floats)


@pytest.mark.parametrize("rows,dim,offset", CLIP_CASES, ids=[f"{r}x{d}+{o}" for r, d, o in CLIP_CASES])
def test_clip_gradient_rows(kctc, gpu, rows, dim, offset):
    """Rows as in tests/test_clipgrad_gpu.py plus the exact-tie row; the device
    counter starts non-zero and rises by exactly the number of rows at or
    above the threshold in each of two calls; offset 1 with dim % 4 == 0
    takes the scalar path over rows the vector path would otherwise take."""
    import torch
    thr = cr.THRESHOLD
    tie = cr.tie_row_of(rows)
    od = cr.make_deriv(rows, dim, 41, tie_row=tie)
    ref = cr.clip_backprop(od, od, ClipCfg(thr, True, 1.0, 0.0, 0.0), (0, 0), None, 1.0)
    k = int(ref.clipped_rows.sum())
    cnt = Guarded(gpu, 1, dtype=torch.int32)
    cnt.view.fill_(1000)
    for call in (1, 2):
        g = Guarded(gpu, rows * dim, offset).set(od)
        kctc.clip_gradient_rows(g.view.view(rows, dim), thr, cnt.view)
        got = g.get().reshape(rows, dim)
        assert int(cnt.get()[0]) == 1000 + call * k
        keep = ~ref.clipped_rows
        np.testing.assert_array_equal(got[keep].view(np.uint32), od[keep].view(np.uint32))
        if tie is not None:
            assert ref.clipped_rows[tie]
            np.testing.assert_array_equal(got[tie].view(np.uint32), od[tie].view(np.uint32))
        err = cr.row_rel_err(got, ref.deriv)
        assert np.isfinite(got).all() and err < 2e-6, err      # measured on MI355X: at most 8.5e-8 (1030 x 63)
    print(f"clip_gradient_rows {rows}x{dim}+{offset}: {k} rows clipped, row-wise error {err:.2e}")


def test_clip_gradient_rows_bad_arguments(kctc, gpu):
    import torch
    g = Guarded(gpu, 12).set(np.full(12, 100.0, np.float32))
    cnt = Guarded(gpu, 1, dtype=torch.int32)
    cnt.view.fill_(7)
    s = torch.cuda.current_stream().cuda_stream
    L = kctc.lib()
    p, c = g.view.data_ptr(), cnt.view.data_ptr()
    assert L.kcm_clip_gradient_rows(s, p, 3, 4, 0.0, c) == 1
    assert L.kcm_clip_gradient_rows(s, p, 3, 4, -1.0, c) == 1
    assert L.kcm_clip_gradient_rows(s, p, 3, 0, 4.0, c) == 1
    assert L.kcm_clip_gradient_rows(s, p, 3, -4, 4.0, c) == 1
    assert L.kcm_clip_gradient_rows(s, None, 3, 4, 4.0, c) == 1
    assert L.kcm_clip_gradient_rows(s, p, 3, 4, 4.0, None) == 1
    assert L.kcm_clip_gradient_rows(s, p, 0, 4, 4.0, c) == 0        # no rows: nothing to do
    np.testing.assert_array_equal(g.get(), np.full(12, 100.0, np.float32))
    assert int(cnt.get()[0]) == 7


# ---------------------------------------------------------------------------
# kcm_add_row_sum_mat: out = alpha * sum of rows + beta * out
# ---------------------------------------------------------------------------
# rows either side of every step of the partition count min(64, max(1, rows / 256)) and of its cap;
# cols either side of the 64-column block; each (alpha, beta) four or five times
AB = [(1.0, 0.0), (0.5, 2.0), (-1.0, 1.0)]
SUM_CASES = [(1, 1), (3, 41), (255, 63), (256, 64), (257, 65), (511, 300), (512, 41), (1000, 64), (1000, 300),
             (16383, 65), (16384, 63), (16389, 1), (20000, 65)]
SUM_CASES = [(r, c) + AB[i % 3] for i, (r, c) in enumerate(SUM_CASES)] + [(257, 65, 1.0, 0.0), (16389, 41, -1.0, 1.0)]


def _parts(rows):
    return min(64, max(1, rows // 256))


def _row_sum(kctc, gpu, X, out0, alpha, beta):
    rows, cols = X.shape
    import torch
    x = torch.from_numpy(X).to(gpu)
    res = []
    for _ in range(2):
        out = Guarded(gpu, cols).set(out0)
        ws = Guarded(gpu, 64 * cols)             # exactly the documented size
        kctc.add_row_sum_mat(out.view, x, alpha, beta, ws.view)
        res.append(out.get())
        ws.get()
    np.testing.assert_array_equal(res[0].view(np.uint32), res[1].view(np.uint32))    # fixed-order sums
    return res[0]


@pytest.mark.parametrize("rows,cols,alpha,beta", SUM_CASES, ids=[f"{r}x{c}-{a}-{b}" for r, c, a, b in SUM_CASES])
def test_add_row_sum_mat_exact(kctc, gpu, rows, cols, alpha, beta):
    """X integer-valued in [-8, 8], alpha and beta powers of two: every fp32
    sum is exact in any order, so the result equals the int64 reference to
    the bit and a dropped or doubled row cannot hide in a tolerance.  With
    beta = 0 the output starts as NaN."""
    rng = np.random.default_rng([rows, cols])
    X = rng.integers(-8, 9, size=(rows, cols)).astype(np.float32)
    out_int = rng.integers(-8, 9, size=cols).astype(np.float32)
    out0 = np.full(cols, np.nan, np.float32) if beta == 0 else out_int
    got = _row_sum(kctc, gpu, X, out0, alpha, beta)
    s = X.astype(np.int64).sum(axis=0).astype(np.float64)
    ref = alpha * s + (beta * out_int.astype(np.float64) if beta != 0 else 0.0)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, ref.astype(np.float32))
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()       # the reference itself is exact in fp32


def test_add_row_sum_mat_gaussian(kctc, gpu):
    """N(0,1) input against fp64 within the recursive-summation bound
    L * 2^-24 * |alpha| * sum|x| per column; L = the longest chain of additions:
    ceil(rows / (4 parts)) in a wave group, 3 across the groups, `parts` over
    the partials."""
    rows, cols, alpha = 16389, 65, 0.5
    X = np.random.default_rng(77).standard_normal((rows, cols)).astype(np.float32)
    got = _row_sum(kctc, gpu, X, np.full(cols, np.nan, np.float32), alpha, 0.0).astype(np.float64)
    x64 = X.astype(np.float64)
    ref = alpha * x64.sum(axis=0)
    parts = _parts(rows)
    L = -(-rows // (4 * parts)) + 3 + parts
    bound = L * 2.0 ** -24 * abs(alpha) * np.abs(x64).sum(axis=0)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"add_row_sum_mat gaussian: worst error / bound {ratio:.4f}")
    assert (np.abs(got - ref) <= bound).all(), ratio      # measured on MI355X: 0.0006 of the bound
