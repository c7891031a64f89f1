"""AffineComponent as the recipe's hidden layer (--model-type FT: input-dim 40,
or the LDA dimension, output-dim hidden_dim = 1024, bias-stddev=0), at recipe
width and with rows in the thousands.

Its weight gradient is the GEMM M = out, N = in, K = T*N: few tiles and a long
K, so gemm_pick_split splits K and AffineComponent::Backprop sizes the split
workspace (split * M * N floats) beside the bias sum's; the tests assert that
the shapes do take that path.

Through the component ABI: Propagate, the gradient (Backprop into a
SetZero(true) copy: learning rate 1, so the copy holds the gradient) with and
without an input derivative, against numpy fp64.  Bar 1e-5 norm-wise relative:
gemm_f32 is an exact-fp32 GEMM, so the error is the fp32 accumulation's, about
sqrt(K) * 6e-8 = 4e-6 at K = 4100 (the bar of the FixedAffine and gemm_f32 tests).

In a whole step: the FT front alone with hidden_dim 1024 over 4000 rows (T =
500, N = 8), the hidden affine the first updatable component below a
1024-input BLSTM-64, against the fp64 chain of tests/front_end_ref.py, at the
bars of tests/test_front_end_gpu.py (costs 1e-5, gradients 1e-4)."""
import numpy as np
import pytest

import front_end_ref as F
from conftest import rel_err

pytestmark = pytest.mark.gpu

# (T, N, in, out): the recipe's 40 -> 1024; after an LDA to 30; a wide input; rows % 4 != 0
SHAPES = [(1025, 4, 40, 1024), (513, 4, 30, 1024), (343, 3, 440, 300)]


@pytest.mark.parametrize("T,N,din,dout", SHAPES)
def test_hidden_affine_component_at_recipe_width(kctc, gpu, T, N, din, dout):
    import torch
    rows = T * N
    assert kctc.lib().kcm_test_gemm_pick_split(dout, din, rows, 1) > 1  # the split-K workspace path
    c = kctc.Component(f"AffineComponent input-dim={din} output-dim={dout}  bias-stddev=0 ", seed=3)
    p = c.Vectorize().astype(np.float64)
    W, b = F.split_affine(p, dout)
    assert not b.any() and W.std() > 0
    rng = np.random.default_rng([T, N, din, dout])
    x = rng.standard_normal((rows, din)).astype(np.float32)
    dy = rng.standard_normal((rows, dout)).astype(np.float32)
    xd, dyd = torch.from_numpy(x).to(gpu), torch.from_numpy(dy).to(gpu)
    out = c.Propagate(T, N, xd)
    torch.cuda.synchronize()
    e = rel_err(out.cpu().numpy(), x.astype(np.float64) @ W.T + b)
    print(f"{din}->{dout} x {rows}: forward {e:.2e}")
    assert e < 1e-5, e
    want = np.concatenate([(dy.astype(np.float64).T @ x.astype(np.float64)).ravel(), dy.astype(np.float64).sum(0)])
    for with_dx in (False, True):  # the first updatable component computes no input derivative
        grad = c.Copy()
        grad.SetZero(True)
        dx = torch.empty((rows, din), dtype=torch.float32, device=gpu) if with_dx else None
        c.Backprop(T, N, xd, None, dyd, to_update=grad, in_deriv=dx)
        torch.cuda.synchronize()
        g = grad.Vectorize().astype(np.float64)
        eg, eb = rel_err(g[:-dout], want[:-dout]), rel_err(g[-dout:], want[-dout:])
        print(f"{din}->{dout} x {rows}: weight gradient {eg:.2e}, bias gradient {eb:.2e} (in_deriv: {with_dx})")
        assert eg < 1e-5 and eb < 1e-5, (eg, eb)
        if with_dx:
            ex = rel_err(dx.cpu().numpy(), dy.astype(np.float64) @ W)
            print(f"{din}->{dout} x {rows}: input derivative {ex:.2e}")
            assert ex < 1e-5, ex
    np.testing.assert_array_equal(c.Vectorize(), p.astype(np.float32))  # the component itself was not updated


def test_step_with_hidden_dim_1024_over_4000_rows(kctc, gpu, oracle):
    import torch
    HD, T, ctx = 1024, 500, (0,)
    lens = [500, 388, 451, 120, 500, 333, 479, 67]
    N = len(lens)
    assert kctc.lib().kcm_test_gemm_pick_split(HD, F.D0, T * N, 1) > 1
    # RNN init 0.05: its input gain stddev * sqrt(1024) = 1.6 is the recurrent gain 0.2 * sqrt(64) of the other tests
    cfg = lambda thr: F.config(kctc, None, thr, front_only=True, hdim=HD, param_stddev=0.05)
    net = kctc.Nnet(cfg(1.0), seed=5)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    assert upd[0] == 1 and net.info(1).startswith(f"AffineComponent, input-dim={F.D0}, output-dim={HD}")
    params = [net.get_params(c).astype(np.float64) for c in upd]
    net.close()
    xs, labels, fl, ll = F.minibatch(lens=lens, seed=7, ctx=ctx)
    x, nf = F.spliced(xs, lens, T, ctx=ctx), np.array(lens, np.int32)
    probe = F.chain_step(oracle, x, None, *params, nf, fl, ll, None, hdim=HD)
    thr = float(np.float32(np.median(probe["front_norms"])))
    st = F.chain_step(oracle, x, None, *params, nf, fl, ll, thr, hdim=HD)
    k = int(st["front_clipped"].sum())
    print(f"front threshold {thr!r}: {k} of {st['rows']} rows clip")
    assert 1 <= k <= st["rows"] - 1
    net = kctc.Nnet(cfg(thr), seed=5)
    p0 = net.get_params(upd[0])
    dev = torch.from_numpy(F.format_input(xs, lens, T, ctx=ctx)).to(gpu)
    objf, _, wt = net.train_step(dev, T, N, nf, fl, ll)
    assert wt == ll.sum()
    got = net.last_costs(N)
    print(f"costs rel err {np.abs(got / st['costs'] - 1).max():.2e}")
    np.testing.assert_allclose(got, st["costs"], rtol=1e-5)
    for name, c, g in zip(("hidden affine", "rnn", "output affine"), upd, st["grads"]):
        e = rel_err(net.get_grad(c).astype(np.float64), g)
        print(f"{name}: gradient rel err {e:.2e}")
        assert e < 1e-4, (name, e)
    want = np.float32(F.LR) * net.get_grad(upd[0])
    e = rel_err(net.get_params(upd[0]) - p0, want)
    print(f"hidden affine: update vs lr * grad {e:.2e}")
    assert e < 1e-6, e
    # the RectifiedLinear statistics at this width: counts exact, sums at the kernel test's bar
    relu = [c for c in range(net.num_components) if net.info(c).startswith("RectifiedLinearComponent")][0]
    v, d, n = net.get_component(relu).nonlinear_stats()
    assert n == st["rows"]
    np.testing.assert_allclose(v, st["relu_value_sum"], rtol=1e-5, atol=1e-5 * np.abs(st["relu_value_sum"]).max())
    print(f"deriv_sum: {int(np.abs(d - st['relu_deriv_sum']).sum())} of {int(d.sum())} positives differ")
    net.close()
