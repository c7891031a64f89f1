"""RectifiedLinearComponent's kernels (csrc/nonlinear.hip) and
FixedAffineComponent through the component ABI (include/kaldi_nnet2_component.h).

ReLU is a select: forward and in_deriv are bit-equal to numpy's.  deriv_sum
counts positives (< 2^24 per column, so the fp32 slab partials are exact) and
is exact; value_sum is within 1e-5 relative of the fp64 column sums (fp32
partials, as the reference's AddRowSumMat; the project's bar for sums).
FixedAffine: 1e-5 norm-wise relative of fp64 (an exact-fp32 GEMM over K <= 440).

Shapes: one element; dim below a wave and odd (scalar path); dim = 64 with rows
not a multiple of the 4 waves; 4099 x 130 (dim % 4 != 0, dim / 4 past one lane
trip, more row slabs than one, rows % 16 != 0); 2051 x 1024 (four column tiles,
the recipe width)."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 37), (67, 64), (4099, 130), (2051, 1024)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _input(rows, dim, seed):
    """N(0,1) with exact zeros, -0.0 and denormals of both signs planted"""
    rng = np.random.default_rng([seed, rows, dim])
    x = rng.standard_normal((rows, dim)).astype(np.float32).ravel()
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)
    idx = rng.permutation(x.size)[:special.size]
    x[idx] = special[:idx.size]
    if x.size > 16:
        x[rng.permutation(x.size)[:x.size // 8]] = 0.0
    return x.reshape(rows, dim)


def _relu(kctc, dim):
    return kctc.Component(f"RectifiedLinearComponent dim={dim} ")  # the generator's line ends in a blank


@pytest.mark.parametrize("rows,dim", SHAPES)
def test_relu_forward_is_bit_exact(kctc, gpu, rows, dim):
    import torch
    c = _relu(kctc, dim)
    assert (c.BackpropNeedsInput(), c.BackpropNeedsOutput(), c.IsUpdatable()) == (False, True, False)
    x = _input(rows, dim, 1)
    want = np.where(x < 0, np.float32(0), x)
    xd = torch.from_numpy(x).to(gpu)
    out = c.Propagate(rows, 1, xd)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
    c.Propagate(rows, 1, xd, out=xd)  # in place
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(xd.cpu().numpy()), _bits(want))
    # a pointer that is only 4-byte aligned: the scalar kernel
    buf = torch.zeros(rows * dim + 1, dtype=torch.float32, device=gpu)
    off = buf[1:].view(rows, dim)
    off.copy_(torch.from_numpy(x))
    o2 = torch.full((rows * dim + 1,), 7.0, dtype=torch.float32, device=gpu)
    c.Propagate(rows, 1, off, out=o2[1:].view(rows, dim))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(o2[1:].cpu().numpy()).reshape(rows, dim), _bits(want))
    assert float(o2[0]) == 7.0


def _bwd_inputs(rows, dim):
    y = np.maximum(_input(rows, dim, 2), np.float32(0))  # a ReLU output: zeros (and -0.0 -> 0.0) and positives
    if y.size > 7:
        y.ravel()[::7] = np.float32(-0.0)
    dy = np.random.default_rng([3, rows, dim]).standard_normal((rows, dim)).astype(np.float32)
    return y, dy


@pytest.mark.parametrize("rows,dim", SHAPES)
def test_relu_backward_and_statistics(kctc, gpu, rows, dim):
    import torch
    y, dy = _bwd_inputs(rows, dim)
    want = np.where(y > 0, dy, np.float32(0))
    pos = (y > 0).sum(0).astype(np.float64)
    vsum = y.astype(np.float64).sum(0)
    yd, dyd = torch.from_numpy(y).to(gpu), torch.from_numpy(dy).to(gpu)
    c = _relu(kctc, dim)
    idv = torch.empty_like(dyd)
    c.Backprop(rows, 1, None, yd, dyd, to_update=c, in_deriv=idv)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(idv.cpu().numpy()), _bits(want))
    v, d, n = c.nonlinear_stats()
    np.testing.assert_array_equal(d, pos)
    assert n == rows
    np.testing.assert_allclose(v, vsum, rtol=1e-5)
    # to_update = None: the statistics stay; in place on out_deriv
    inplace = dyd.clone()
    c.Backprop(rows, 1, None, yd, inplace, to_update=None, in_deriv=inplace)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(inplace.cpu().numpy()), _bits(want))
    v1, d1, n1 = c.nonlinear_stats()
    np.testing.assert_array_equal(_bits64(v1), _bits64(v))
    np.testing.assert_array_equal(d1, d)
    assert n1 == n
    # in_deriv = None still updates; a second call accumulates
    c.Backprop(rows, 1, None, yd, dyd, to_update=c, in_deriv=None)
    v2, d2, n2 = c.nonlinear_stats()
    np.testing.assert_array_equal(d2, 2 * pos)
    assert n2 == 2 * rows
    np.testing.assert_allclose(v2, 2 * vsum, rtol=1e-5)
    # a fresh component, the same input: identical bits (no dependence on launch timing)
    f = _relu(kctc, dim)
    f.Backprop(rows, 1, None, yd, dyd, to_update=f, in_deriv=torch.empty_like(dyd))
    vf, df, nf = f.nonlinear_stats()
    np.testing.assert_array_equal(_bits64(vf), _bits64(v))
    np.testing.assert_array_equal(df, d)
    # another component as to_update gets the statistics, the backpropped one keeps its own
    g, t = _relu(kctc, dim), _relu(kctc, dim)
    g.Backprop(rows, 1, None, yd, dyd, to_update=t, in_deriv=None)
    assert t.nonlinear_stats()[2] == rows and g.nonlinear_stats()[2] == 0


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_relu_backward_on_4_byte_aligned_pointers(kctc, gpu):
    import torch
    rows, dim = 67, 64
    y, dy = _bwd_inputs(rows, dim)
    ybuf = torch.zeros(rows * dim + 1, dtype=torch.float32, device=gpu)
    yv = ybuf[1:].view(rows, dim)
    yv.copy_(torch.from_numpy(y))
    dyd = torch.from_numpy(dy).to(gpu)
    c = _relu(kctc, dim)
    idv = torch.empty_like(dyd)
    c.Backprop(rows, 1, None, yv, dyd, to_update=c, in_deriv=idv)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(idv.cpu().numpy()), _bits(np.where(y > 0, dy, np.float32(0))))
    v, d, n = c.nonlinear_stats()
    np.testing.assert_array_equal(d, (y > 0).sum(0))
    np.testing.assert_allclose(v, y.astype(np.float64).sum(0), rtol=1e-5)


def test_relu_rejects_bad_lines_and_other_types_have_no_statistics(kctc, gpu):
    for line in ("RectifiedLinearComponent", "RectifiedLinearComponent dim=0", "RectifiedLinearComponent dim=4 x=1"):
        with pytest.raises(kctc.KctcError):
            kctc.Component(line)
    with pytest.raises(kctc.KctcError, match="statistics"):
        kctc.Component("ClipGradientComponent dim=4").nonlinear_stats()
    v, d, n = kctc.Component("SoftmaxComponent dim=5").nonlinear_stats()
    assert v.shape == (5,) and not v.any() and n == 0


@pytest.mark.parametrize("rows,din,dout", [(67, 39, 20), (515, 440, 250)])
@pytest.mark.parametrize("binary", [False, True])
def test_fixed_affine_matches_fp64(kctc, gpu, tmp_path, rows, din, dout, binary):
    import torch
    rng = np.random.default_rng([rows, din, dout])
    m = (rng.standard_normal((dout, din + 1)) / np.sqrt(din)).astype(np.float32)
    path = tmp_path / "lda.mat"
    kctc.write_kaldi_matrix(path, m, binary=binary)
    c = kctc.Component(f"FixedAffineComponent matrix={path}")
    assert (c.InputDim(), c.OutputDim(), c.IsUpdatable()) == (din, dout, False)
    assert (c.BackpropNeedsInput(), c.BackpropNeedsOutput()) == (False, False)
    info = c.Info()
    assert f"input-dim={din}, output-dim={dout}" in info
    std = float(info.split("linear-params-stddev=")[1].split(",")[0])
    np.testing.assert_allclose(std, np.sqrt((m[:, :-1].astype(np.float64) ** 2).mean()), rtol=1e-4)
    bstd = float(info.split("bias-params-stddev=")[1])
    np.testing.assert_allclose(bstd, np.sqrt((m[:, -1].astype(np.float64) ** 2).mean()), rtol=1e-4)
    x = rng.standard_normal((rows, din)).astype(np.float32)
    dy = rng.standard_normal((rows, dout)).astype(np.float32)
    m64 = m.astype(np.float64)
    out = c.Propagate(rows, 1, torch.from_numpy(x).to(gpu))
    dx = torch.empty((rows, din), dtype=torch.float32, device=gpu)
    c.Backprop(rows, 1, None, None, torch.from_numpy(dy).to(gpu), in_deriv=dx)
    torch.cuda.synchronize()
    ef = rel_err(out.cpu().numpy(), x.astype(np.float64) @ m64[:, :-1].T + m64[:, -1])
    eb = rel_err(dx.cpu().numpy(), dy.astype(np.float64) @ m64[:, :-1])
    print(f"FixedAffine {rows}x{din}->{dout}: forward {ef:.2e}, backward {eb:.2e}")
    assert ef < 1e-5 and eb < 1e-5


def test_fixed_affine_rejects_bad_lines(kctc, gpu, tmp_path):
    ok = tmp_path / "ok.mat"
    kctc.write_kaldi_matrix(ok, np.ones((3, 4), np.float32))
    kctc.Component(f"FixedAffineComponent matrix={ok}")
    one = tmp_path / "one.mat"
    kctc.write_kaldi_matrix(one, np.ones((3, 1), np.float32))
    for line in ("FixedAffineComponent", f"FixedAffineComponent matrix={one}",
                 f"FixedAffineComponent matrix={ok} learning-rate=0.1",
                 f"FixedAffineComponent matrix={tmp_path / 'missing.mat'}"):
        with pytest.raises(kctc.KctcError):
            kctc.Component(line)
