"""The fp32 GEMM (gemm_f32, csrc/gemm.hip) on its own, through the
kcm_test_gemm_f32 hook, which reaches every field of GemmArgs.

Exact cases: operands, C0 and biases are integers in [-4, 4], alpha in
{1, 0.5, -2}, beta in {0, 1, -0.5} and K <= 4096, so every product, partial
sum and epilogue term is a multiple of 0.5 below 2^24 in magnitude: exact in
fp32 in any summation order.  The result must equal the float64 reference
value for value (a dropped k element of one ragged tail or a bias skipped in
one column tile changes an element by at least 0.5).

Every buffer is laid out by the test.  The operand buffers hold NaN wherever
the GEMM has no business reading; C has a padded ldc and trailing guard rows,
the split-K workspace and the tile counter a guard tail, all holding one NaN
bit pattern that must come back bit for bit.

The tile is 128 x 128 x 32 and each case is the smallest shape on which its
path can still go wrong; the largest is 1300 x 800 x 32."""
import ctypes

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

NAN_BITS = 0x7FC0BEEF  # a quiet NaN with a payload nothing computes
GUARD = 64


def nan_buf(n):
    return np.full(n, NAN_BITS, np.int32)


def grid_idx(base, ld, rows, cols):
    return base + np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]


class Gemm:
    """One problem: the flat host buffers, the call and the float64 reference."""

    def __init__(self, M, N, K, ta=0, tb=0, alpha=1.0, beta=0.0, lda=None, ldb=None, ldc=None, a_base=0, b_base=0,
                 bias=False, bias2=False, batch=1, sA=0, sB=0, sC=None, sBias=0, split_k=1, max_blocks=0,
                 counter=False, garbage_c=False, normal=False, seed=0):
        self.M, self.N, self.K, self.ta, self.tb, self.alpha, self.beta = M, N, K, ta, tb, alpha, beta
        self.batch, self.sA, self.sB, self.sBias = batch, sA, sB, sBias
        self.split_k, self.max_blocks, self.counter = split_k, max_blocks, counter
        rng = np.random.default_rng(1000 * M + 10 * N + K + seed)
        draw = (lambda n: rng.standard_normal(n)) if normal else (lambda n: rng.integers(-4, 5, n))
        sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
        self.lda = lda if lda is not None else max(sa[1], 1)
        self.ldb = ldb if ldb is not None else max(sb[1], 1)
        self.ldc = ldc if ldc is not None else N + 3
        self.sC = sC if sC is not None else M * self.ldc
        self.a_base, self.b_base = a_base, b_base

        def operand(base, ld, shape, stride):
            idx = [grid_idx(base + b * stride, ld, *shape) for b in range(batch)]
            flat = np.concatenate([i.ravel() for i in idx])
            assert flat.size == 0 or flat.min() >= 0
            buf = nan_buf((int(flat.max()) + 1 if flat.size else 0) + GUARD)
            u = np.unique(flat)
            buf.view(np.float32)[u] = draw(u.size).astype(np.float32)
            return buf, [buf.view(np.float32)[i].astype(np.float64) for i in idx]

        self.A, a = operand(a_base, self.lda, sa, sA)
        self.B, b = operand(b_base, self.ldb, sb, sB)
        self.cidx = [grid_idx(bi * self.sC, self.ldc, M, N) for bi in range(batch)]
        allc = np.concatenate([i.ravel() for i in self.cidx])
        assert np.unique(allc).size == allc.size  # the batches' outputs do not overlap
        self.C = nan_buf(int(allc.max()) + 1 + 3 * self.ldc)
        self.valid = np.zeros(self.C.size, bool)
        self.valid[allc] = True
        if not garbage_c:
            self.C.view(np.float32)[allc] = draw(allc.size).astype(np.float32)
        else:
            assert beta == 0.0

        def bias_buf(on):
            if not on:
                return None, [np.zeros(N)] * batch
            # NaN also where a bias addressed by B's stride would lie
            buf = nan_buf((batch - 1) * max(sBias, sB) + N + GUARD)
            idx = [bi * sBias + np.arange(N) for bi in range(batch)]
            u = np.unique(np.concatenate(idx))
            buf.view(np.float32)[u] = draw(u.size).astype(np.float32)
            return buf, [buf.view(np.float32)[i].astype(np.float64) for i in idx]

        self.bias, v1 = bias_buf(bias)
        self.bias2, v2 = bias_buf(bias2)
        # float64 reference and, for the rounded case, the magnitude sum S of its terms
        self.ref, self.S = [], []
        for bi in range(batch):
            opa, opb = (a[bi].T if ta else a[bi]), (b[bi].T if tb else b[bi])
            c0 = self.C.view(np.float32)[self.cidx[bi]].astype(np.float64) if beta != 0.0 else np.zeros((M, N))
            self.ref.append(alpha * (opa @ opb) + beta * c0 + v1[bi][None, :] + v2[bi][None, :])
            self.S.append(abs(alpha) * (np.abs(opa) @ np.abs(opb)) + np.abs(beta * c0) + np.abs(v1[bi])[None, :] +
                          np.abs(v2[bi])[None, :])

    def run(self, kctc, gpu, ws_slabs=None):
        """Runs the GEMM; returns (C buffer as int32, split used).  Checks the
        workspace and counter guards on the way."""
        import torch
        dev = lambda x: None if x is None else torch.from_numpy(x).to(gpu)
        dA, dB, dC, db1, db2 = dev(self.A), dev(self.B), dev(self.C.copy()), dev(self.bias), dev(self.bias2)
        slabs = ws_slabs if ws_slabs is not None else (self.split_k if self.split_k > 1 else 0)
        ws_n = slabs * self.batch * self.M * self.N
        dws = dev(nan_buf(ws_n + GUARD)) if slabs else None
        dcnt = dev(nan_buf(16)) if self.counter else None
        used = ctypes.c_int(-1)
        ptr = lambda t, off=0: None if t is None else t.data_ptr() + 4 * off
        rc = kctc.lib().kcm_test_gemm_f32(
            None, self.ta, self.tb, self.M, self.N, self.K, self.alpha, self.beta, ptr(dA, self.a_base), self.lda,
            ptr(dB, self.b_base), self.ldb, ptr(dC), self.ldc, ptr(db1), ptr(db2), self.batch, self.sA, self.sB,
            self.sC, self.sBias, self.split_k, ptr(dws), self.max_blocks, ptr(dcnt), ctypes.byref(used))
        assert rc == 0
        if dws is not None:
            assert np.all(dws[ws_n:].cpu().numpy() == np.int32(NAN_BITS)), "split-K workspace guard"
        if dcnt is not None:
            cnt = dcnt.cpu().numpy()
            assert cnt[0] >= 0 and np.all(cnt[1:] == np.int32(NAN_BITS)), "tile counter guard"
        return dC.cpu().numpy(), used.value

    def expected(self):
        exp = self.C.copy()
        for bi in range(self.batch):
            exp.view(np.float32)[self.cidx[bi]] = self.ref[bi].astype(np.float32)
        return exp

    def check_exact(self, out):
        exp = self.expected()
        v = self.valid
        got = out.view(np.float32)[v]
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(got, exp.view(np.float32)[v])  # by value: -0 equals +0
        np.testing.assert_array_equal(out[~v], exp[~v])  # ldc padding and guard rows, bit for bit


def run_exact(kctc, gpu, **kw):
    g = Gemm(**kw)
    out, used = g.run(kctc, gpu)
    g.check_exact(out)
    return used


TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
AB = [(1.0, 0.0), (0.5, 1.0), (-2.0, -0.5)]  # (alpha, beta), cycled over the cases of a test


def lds(ta, tb, M, N, K, pad):
    """Leading dimensions of the stored operands, rounded up to a multiple of pad."""
    up = lambda x: (x + pad - 1) // pad * pad
    return up(M if ta else K), up(K if tb else N)


@pytest.mark.parametrize("layout", ["contiguous", "ld_mult4", "base_plus_1"])
@pytest.mark.parametrize("ta,tb", TRANS)
def test_ragged_tile(kctc, gpu, ta, tb, layout):
    """130 x 70 x 37: a ragged second row tile, a ragged column tile and a k
    tail of 5 = one whole float4 and one element.  contiguous: no ld is a
    multiple of 4, scalar loads; ld_mult4: vector loads, and the tail's last
    element goes through the scalar path inside a vector launch; base_plus_1:
    aligned ld from a base one float off 16 B, scalar loads again."""
    M, N, K = 130, 70, 37
    lda, ldb = lds(ta, tb, M, N, K, 1 if layout == "contiguous" else 4)
    if layout == "contiguous":
        assert lda % 4 and ldb % 4
    base = 1 if layout == "base_plus_1" else 0
    alpha, beta = AB[(2 * ta + tb) % 3]
    run_exact(kctc, gpu, M=M, N=N, K=K, ta=ta, tb=tb, alpha=alpha, beta=beta, lda=lda, ldb=ldb, ldc=N + 3 + (ta ^ tb),
              a_base=base, b_base=base, bias=True)


@pytest.mark.parametrize("K", [0, 1, 3, 4, 32, 33])
def test_small_k(kctc, gpu, K):
    """K = 0 leaves beta C0 + bias + bias2; also through the drop-in
    kcm_add_mat_mat, which accepts K = 0."""
    import torch
    for i, (ta, tb) in enumerate(TRANS):
        alpha, beta = AB[(i + K) % 3]
        lda, ldb = lds(ta, tb, 5, 9, max(K, 1), 4 if K % 2 == 0 else 1)
        run_exact(kctc, gpu, M=5, N=9, K=K, ta=ta, tb=tb, alpha=alpha, beta=beta, lda=lda, ldb=ldb, bias=True,
                  bias2=True, seed=i)
    if K == 0:
        C0 = np.arange(45, dtype=np.float32).reshape(5, 9) - 20
        C = torch.from_numpy(C0).to(gpu)
        kctc.add_mat_mat(C, torch.empty((5, 0), device=gpu), torch.empty((0, 9), device=gpu), alpha=0.5, beta=-0.5)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(C.cpu().numpy(), -0.5 * C0)
        # a split-K request has no chunk to size at K = 0: the epilogue alone
        g = Gemm(M=5, N=9, K=0, alpha=1.0, beta=1.0, bias=True, split_k=3)
        out, used = g.run(kctc, gpu)
        assert used == 1
        g.check_exact(out)


@pytest.mark.parametrize("ta,tb", TRANS)
def test_beta_zero_over_garbage(kctc, gpu, ta, tb):
    """beta = 0 must not read C: it is prefilled with NaN, the result is finite and exact."""
    run_exact(kctc, gpu, M=130, N=70, K=37, ta=ta, tb=tb, alpha=-2.0, beta=0.0, garbage_c=True, bias=bool(ta))
    run_exact(kctc, gpu, M=130, N=70, K=200, ta=ta, tb=tb, alpha=0.5, beta=0.0, garbage_c=True, split_k=3)


@pytest.mark.parametrize("bias,bias2", [(1, 0), (0, 1), (1, 1)])
def test_bias(kctc, gpu, bias, bias2):
    """N = 130: the second column tile is ragged."""
    for i, (ta, tb) in enumerate(TRANS):
        alpha, beta = AB[i % 3]
        run_exact(kctc, gpu, M=70, N=130, K=37, ta=ta, tb=tb, alpha=alpha, beta=beta, bias=bool(bias),
                  bias2=bool(bias2), seed=i)


@pytest.mark.parametrize("N,din", [(132, 40), (130, 37)])
def test_forward_projection_batch(kctc, gpu, N, din):
    """The RNN's input projection: both directions read the same frames
    (strideA = 0), weights and biases sit in one parameter block per direction
    (strideB = strideBias), and direction d writes columns [d N, d N + N) of
    rows 2 N wide (strideC = N, ldc = 2 N)."""
    M, pls = 70, N * din + 2 * N + (4 - (N * din + 2 * N) % 4) % 4 + (0 if N % 4 == 0 else 1)
    g = Gemm(M=M, N=N, K=din, ta=0, tb=1, lda=din, ldb=din, ldc=2 * N, batch=2, sA=0, sB=pls, sC=N, sBias=pls,
             bias=True, bias2=True)
    assert g.C.size == (M - 1) * 2 * N + N + N + 3 * 2 * N
    out, _ = g.run(kctc, gpu)
    g.check_exact(out)


def test_batch_bias_stride(kctc, gpu):
    """Biases follow strideBias, not the stride of B."""
    run_exact(kctc, gpu, M=5, N=130, K=8, tb=1, batch=2, sA=5 * 8, sB=130 * 8 + 8, sBias=130 + 5, bias=True,
              bias2=True, beta=1.0)


@pytest.mark.parametrize("H", [32, 30])
def test_wgrad_recurrent_batch(kctc, gpu, H):
    """dR of both directions as wgrad_f32 runs it: A = dGates^T [T n][2 G4]
    from frame 1 on for direction 0 and, a negative stride away, from frame 0
    and column G4 on for direction 1; B = y [T n][2 H] from frame 0 or from
    frame 1, column H; beta = 1.  H = 30 makes strideB = n ldy + H no multiple
    of 4: vector loads of B are off through the stride check."""
    T, n, G4 = 4, 3, 4 * H
    ldg, ldy = 2 * G4, 2 * H
    sB = n * ldy + H
    assert (sB % 4 == 0) == (H == 32)
    run_exact(kctc, gpu, M=G4, N=H, K=(T - 1) * n, ta=1, tb=0, beta=1.0, lda=ldg, ldb=ldy, ldc=H + 3, a_base=n * ldg,
              batch=2, sA=G4 - n * ldg, sB=sB, sC=G4 * (H + 3) + 5)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("K,split_k,used", [(200, 3, 3), (130, 5, 5), (65, 4, 3)])
def test_split_k(kctc, gpu, K, split_k, used, batch):
    """Chunks of ceil(K / split_k) rounded up to 32: 96 / 96 / 8, 32 x 4 + 2,
    and 32 / 32 / 1 -- fewer slabs than asked."""
    for i, (ta, tb) in enumerate(TRANS):
        got = run_exact(kctc, gpu, M=130, N=70, K=K, ta=ta, tb=tb, alpha=AB[i % 3][0], beta=1.0, bias=True,
                        bias2=bool(i & 1), batch=batch, sA=130 * K, sB=70 * K, sBias=70 + 1, split_k=split_k, seed=i)
        assert got == used


def test_split_k_picked(kctc, gpu):
    """split_k = -1 on 41 x 1024 x 1000, the affine weight gradient's shape class."""
    L = kctc.lib()
    want = L.kcm_test_gemm_pick_split(41, 1024, 1000, 1)
    assert want > 1
    g = Gemm(M=41, N=1024, K=1000, ta=1, tb=0, alpha=1.0, beta=1.0, ldc=1024 + 4, split_k=-1)
    out, used = g.run(kctc, gpu, ws_slabs=want)
    assert 1 < used <= want and used == L.kcm_test_gemm_split_used(1000, want)
    g.check_exact(out)


GRID = [
    ("remap_remainder", dict(M=300, N=400, K=37)),  # 12 work items: the XCD remap has a remainder
    ("covering", dict(M=1300, N=800, K=32)),
    ("persistent", dict(M=1300, N=800, K=32, max_blocks=8)),
    ("persistent_counter", dict(M=1300, N=800, K=32, max_blocks=8, counter=True)),
    ("clamp_to_8", dict(M=1300, N=800, K=32, max_blocks=3)),
    ("counter_split_batch", dict(M=300, N=260, K=200, max_blocks=8, counter=True, split_k=3, batch=2, sA=300 * 200,
                                 sB=260 * 200, sBias=260, beta=1.0)),
]


@pytest.mark.parametrize("name,kw", GRID, ids=[g[0] for g in GRID])
def test_grid_and_remap(kctc, gpu, name, kw):
    """Every work item exactly once: covering grids whose size is no multiple
    of 8, persistent grids that stride over the items, and items dealt from a
    tile counter, with split-K and a batch on top."""
    kw = dict(dict(alpha=0.5, beta=-0.5, tb=1, bias=True, bias2=True, ldc=kw["N"] + 4), **kw)
    run_exact(kctc, gpu, **kw)


@pytest.mark.parametrize("ta,tb", TRANS)
def test_rounded(kctc, gpu, ta, tb):
    """300 x 130 x 257 on standard normal data, alpha = 0.5, beta = -1.5, both
    biases: |C - ref| <= gamma S element by element, S = |alpha| (|A| |B|) +
    |beta C0| + |bias| + |bias2|, gamma = n u / (1 - n u), u = 2^-24, n = K +
    5: the bound for K products summed in any order plus the five epilogue
    roundings (Higham, Accuracy and Stability of Numerical Algorithms, 3.1).

    The bar is derived, not measured.  Measured worst |C - ref| / (gamma S)
    on an MI355X: 0.0189 (NN), 0.0166 (NT), 0.0187 (TN), 0.0158 (TT); with one
    k element of the ragged tail dropped the ratio is above 1."""
    M, N, K = 300, 130, 257
    g = Gemm(M=M, N=N, K=K, ta=ta, tb=tb, alpha=0.5, beta=-1.5, bias=True, bias2=True, normal=True)
    out, _ = g.run(kctc, gpu)
    exp = g.expected()
    np.testing.assert_array_equal(out[~g.valid], exp[~g.valid])
    u, n = 2.0 ** -24, K + 5
    gamma = n * u / (1 - n * u)
    got = out.view(np.float32)[g.cidx[0]].astype(np.float64)
    assert np.all(np.isfinite(got))
    worst = np.max(np.abs(got - g.ref[0]) / (gamma * g.S[0]))
    print(f"rounded ta={ta} tb={tb}: worst |C - ref| / (gamma S) = {worst:.4f}")
    assert worst <= 1.0
