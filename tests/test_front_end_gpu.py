"""Whole train steps of the recipe's FT / LDA networks (include/kaldi_ctc_train.h:
FixedAffineComponent, hidden AffineComponent, RectifiedLinearComponent in front
of the first RNN) against the fp64 chain composed in tests/front_end_ref.py.

Bars: per-utterance costs 1e-5 relative, gradients (kctc_nnet_get_grad) 1e-4
norm-wise relative, the project's bars for a train step; fp32 identities
(params + lr * grad, the one-rank exchange) 1e-6 norm-wise: a handful of fp32
roundings (6e-8 each) per element, an fma or not.

The front ClipGradient's threshold is the oracle's median row norm of its
out_deriv, so about half of the rows clip; the tests assert on the oracle's
numbers that between 1 and rows - 1 do."""
import numpy as np
import pytest

import front_end_ref as F
from conftest import rel_err

pytestmark = pytest.mark.gpu

N = len(F.LENS)
BF16_H = 256  # bf16 recurrences exist for H in {256, 320, 512, 1024} only


@pytest.fixture(scope="module")
def lda_path(kctc, tmp_path_factory):
    p = tmp_path_factory.mktemp("front_end") / "lda.mat"
    kctc.write_kaldi_matrix(p, F.lda_matrix(), binary=True)
    return str(p)


def _indices(net):
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    relu = [c for c in range(net.num_components) if net.info(c).startswith("RectifiedLinearComponent")]
    assert len(upd) == 3 and len(relu) == 1
    return upd, relu[0]


def _feats(gpu, front_only, seed=1000, pad=0.0):
    import torch
    ctx = (0,) if front_only else F.CTX
    xs, labels, fl, ll = F.minibatch(seed=seed, ctx=ctx)
    dev = torch.from_numpy(F.format_input(xs, F.LENS, F.T, ctx=ctx, pad=pad)).to(gpu)
    return xs, labels, fl, ll, dev


@pytest.fixture(scope="module")
def refs(kctc, gpu, oracle, lda_path):
    """Per topology: the initial parameters, the front threshold (the oracle's
    median row norm) and the oracle's default step; computed once, read-only."""
    out = {}
    for front_only, hidden in ((False, F.H), (True, F.H), (False, BF16_H)):
        ctx = (0,) if front_only else F.CTX
        lda = None if front_only else F.lda_matrix()
        net = kctc.Nnet(F.config(kctc, lda_path, 1.0, front_only, hidden), seed=5)
        upd, _ = _indices(net)
        params = [net.get_params(c).astype(np.float64) for c in upd]
        net.close()
        xs, labels, fl, ll = F.minibatch(ctx=ctx)
        x = F.spliced(xs, F.LENS, F.T, ctx=ctx)
        nf = np.array(F.LENS, np.int32)
        probe = F.chain_step(oracle, x, lda, params[0], params[1], params[2], nf, fl, ll, None, hidden)
        thr = float(np.float32(np.median(probe["front_norms"])))
        step = F.chain_step(oracle, x, lda, params[0], params[1], params[2], nf, fl, ll, thr, hidden)
        for a in params + step["grads"]:
            a.setflags(write=False)
        key = front_only if hidden == F.H else "bf16"
        out[key] = dict(params=params, thr=thr, step=step, lda=lda, ctx=ctx, hidden=hidden)
    return out


def _net(kctc, lda_path, refs, key):
    """key: False (the whole network), True (the FT front alone) or "bf16" (the whole network at BLSTM-256)"""
    net = kctc.Nnet(F.config(kctc, lda_path, refs[key]["thr"], key is True, refs[key]["hidden"]), seed=5)
    return net, *_indices(net)


def _check_step(net, upd, ref, objf):
    st = ref["step"]
    k = int(st["front_clipped"].sum())
    print(f"front threshold {ref['thr']!r}: {k} of {st['rows']} rows clip")
    assert 1 <= k <= st["rows"] - 1
    got = net.last_costs(N)
    print(f"costs rel err {np.abs(got / st['costs'] - 1).max():.2e}")
    np.testing.assert_allclose(got, st["costs"], rtol=1e-5)
    np.testing.assert_allclose(objf, st["costs"].sum(), rtol=1e-5)
    for name, c, g in zip(("hidden affine", "rnn", "output affine"), upd, st["grads"]):
        e = rel_err(net.get_grad(c).astype(np.float64), g)
        print(f"{name}: gradient rel err {e:.2e}")
        assert e < 1e-4, (name, e)
    np.testing.assert_array_equal(net.last_best_path(F.T, N), st["ids"])


def test_default_step_matches_the_composed_fp64_chain(kctc, gpu, lda_path, refs):
    net, upd, _ = _net(kctc, lda_path, refs, False)
    assert net.context == (1, 1)
    assert "input-dim=39, output-dim=20" in net.info(1)
    _, _, fl, ll, dev = _feats(gpu, False)
    objf, _, wt = net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)
    assert wt == ll.sum()
    _check_step(net, upd, refs[False], objf)
    net.close()


def test_ft_front_alone_step_and_update(kctc, gpu, lda_path, refs):
    net, upd, _ = _net(kctc, lda_path, refs, True)
    assert net.context == (0, 0) and upd[0] == 1
    p0 = net.get_params(upd[0])
    _, _, fl, ll, dev = _feats(gpu, True)
    objf, _, _ = net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)
    _check_step(net, upd, refs[True], objf)
    want = p0 + np.float32(F.LR) * net.get_grad(upd[0])
    e = rel_err(net.get_params(upd[0]) - p0, want - p0)
    print(f"hidden affine: update vs lr * grad {e:.2e}")
    assert e < 1e-6, e
    net.close()


def test_length_aware_gradient_is_sum_of_single_utterance_gradients(kctc, gpu, oracle, lda_path, refs):
    ref = refs[False]
    xs, labels, _, _ = F.minibatch()
    total, costs = [np.zeros_like(g) for g in ref["step"]["grads"]], []
    for n, L in enumerate(F.LENS):
        one = F.chain_step(oracle, F.spliced([xs[n]], [L], L), ref["lda"], *ref["params"], np.array([L], np.int32),
                           np.array(labels[n], np.int32), np.array([len(labels[n])], np.int32), ref["thr"])
        total = [a + b for a, b in zip(total, one["grads"])]
        costs.append(one["costs"][0])
    net, upd, _ = _net(kctc, lda_path, refs, False)
    net.set_length_aware(True)
    _, _, fl, ll, dev = _feats(gpu, False, pad=1e3)  # padding rows hold 1e3: whatever the front end makes of them is dropped
    objf, _, _ = net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)
    for name, c, g, gd in zip(("hidden affine", "rnn", "output affine"), upd, total, ref["step"]["grads"]):
        e = rel_err(net.get_grad(c).astype(np.float64), g)
        print(f"{name}: length-aware vs per-utterance sum {e:.2e}; the padded step's gradient is {rel_err(gd, g):.2e} away")
        assert e < 1e-4, (name, e)
    got = net.last_costs(N)
    print(f"costs rel err {np.abs(got / np.array(costs) - 1).max():.2e}")
    np.testing.assert_allclose(got, costs, rtol=1e-5)
    np.testing.assert_allclose(objf, np.sum(costs), rtol=1e-5)
    net.close()


def test_bf16_step(kctc, gpu, lda_path, refs):
    """The issue's network at BLSTM-256: bf16 is refused at H = 64 (it exists on the v6
    recurrences only).

    The bound is sketch_common's error model, which assumes an init near the recipe's: a
    recurrence whose rounding errors decay (lam ~ 0.87 at param-stddev 0.02, H = 512).  The
    RNN here is initialised with param-stddev 0.1, the recurrent gain stddev * sqrt(H) = 1.6 of
    the H = 64 cases (front_end_ref.config), as the H = 256 case of tests/test_train_seq_gpu.py.
    Measured on an MI355X: objective 6.4e-5; hidden affine gradient 6.0e-3 (bound 1.5e-2, the
    model's expectation 5.0e-3), RNN 5.7e-3, output affine 2.3e-3.  With param-stddev 0.2 at
    H = 256 (gain 3.2, where the model's premise does not hold) the hidden affine's gradient
    was 5.0e-2 off, outside the bound; see DESIGN.md section 7c."""
    import sketch_common as S
    net, upd, _ = _net(kctc, lda_path, refs, "bf16")
    net.set_precision("bf16")
    _, _, fl, ll, dev = _feats(gpu, False)
    objf, _, _ = net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)
    st = refs["bf16"]["step"]
    k = int(st["front_clipped"].sum())
    assert 1 <= k <= st["rows"] - 1
    print(f"bf16 objective rel err {abs(objf / st['costs'].sum() - 1):.2e}")
    np.testing.assert_allclose(objf, st["costs"].sum(), rtol=1e-3)
    # the front end is exact fp32: the hidden affine inherits the bottom (here the only) RNN's dx error
    bound = S.bf16_tol(S.step_stages(1, "grad", 0))
    e = rel_err(net.get_grad(upd[0]).astype(np.float64), st["grads"][0])
    print(f"bf16 hidden affine gradient rel err {e:.2e} (bound {bound:.2e})")
    for name, c, g in zip(("rnn", "output affine"), upd[1:], st["grads"][1:]):
        print(f"bf16 {name} gradient rel err {rel_err(net.get_grad(c).astype(np.float64), g):.2e}")
    assert e < bound, (e, bound)
    net.close()


def test_momentum_statistics_and_parameters(kctc, gpu, lda_path, refs):
    m = 0.5
    ref = refs[False]
    net, upd, relu = _net(kctc, lda_path, refs, False)
    net.set_momentum(m)
    p0 = net.get_params(upd[0])
    stats, grads = [], []
    for seed in (1000, 1001):
        xs, _, fl, ll, dev = _feats(gpu, False, seed=seed)
        stats.append(F.relu_stats(F.spliced(xs, F.LENS, F.T), ref["lda"], net.get_params(upd[0])))
        net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)
        grads.append(net.get_grad(upd[0]))
    (v1, d1, r1), (v2, d2, r2) = stats
    v, d, count = net.get_component(relu).nonlinear_stats()
    # stats += delta; delta *= m after each minibatch: s1 + (m s1 + s2)
    e = rel_err(v, v1 + (m * v1 + v2))
    print(f"value_sum rel err {e:.2e}")
    assert e < 1e-5, e
    np.testing.assert_array_equal(d, d1 + (m * d1 + d2))
    assert count == r1 + (m * r1 + r2)
    lr = np.float32(F.LR)
    want = lr * grads[0] + (np.float32(m) * lr * grads[0] + lr * grads[1])
    e = rel_err(net.get_params(upd[0]) - p0, want)
    print(f"hidden affine after two momentum steps: {e:.2e}")
    assert e < 1e-6, e
    net.close()


def test_one_rank_communicator(kctc, gpu, lda_path, refs):
    _, _, fl, ll, dev = _feats(gpu, False)
    nf = np.array(F.LENS, np.int32)
    plain, upd, _ = _net(kctc, lda_path, refs, False)
    plain.train_step(dev, F.T, N, nf, fl, ll)
    dp, _, _ = _net(kctc, lda_path, refs, False)
    dp.enable_dp(kctc.dp_unique_id(), 0, 1)
    dp.train_step(dev, F.T, N, nf, fl, ll)
    for c in upd:
        eg = rel_err(dp.get_grad(c), plain.get_grad(c))
        ep = rel_err(dp.get_params(c), plain.get_params(c))
        print(f"component {c}: gradient {eg:.2e}, parameters {ep:.2e}")
        assert eg < 1e-6 and ep < 1e-6, (c, eg, ep)
    dp.close()
    # the buckets, in backprop order: output affine, RNN, hidden affine
    seen = []
    host, _, _ = _net(kctc, lda_path, refs, False)
    host.enable_dp_host(lambda a: seen.append(a.size), 1)
    host.train_step(dev, F.T, N, nf, fl, ll)
    assert seen == [plain.num_params(c) for c in reversed(upd)]
    for c in upd:
        assert rel_err(host.get_params(c), plain.get_params(c)) < 1e-6, c
    host.close()
    plain.close()


def test_average_params_over_two_declared_ranks(kctc, gpu, lda_path, refs):
    """kctc_nnet_average_params with world = 2 on one GPU: a host all-reduce that doubles its
    buffer stands for a second rank holding the same model.  Scale(1/2) then the sum give the
    model back: parameters exactly (a power of two), the RectifiedLinear statistics through
    their fp32 image (counts and integers below 2^24 exactly, the sums to fp32 rounding)."""
    net, upd, relu = _net(kctc, lda_path, refs, False)
    _, _, fl, ll, dev = _feats(gpu, False)
    net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)
    params = [net.get_params(c) for c in upd]
    v0, d0, n0 = net.get_component(relu).nonlinear_stats()
    assert n0 == F.T * N and d0.sum() > 0
    sizes = []

    def allreduce(a):
        sizes.append(a.size)
        a *= 2.0

    net.enable_dp_host(allreduce, 2)
    net.set_dp_mode("average")
    net.average_params()
    assert sorted(sizes) == sorted([net.num_params(c) for c in upd] + [2 * F.DH + 1])
    for c, p in zip(upd, params):
        np.testing.assert_array_equal(net.get_params(c), p)
    v, d, n = net.get_component(relu).nonlinear_stats()
    np.testing.assert_array_equal(d, d0)
    assert n == n0
    np.testing.assert_allclose(v, v0, rtol=2.0 ** -23)  # one rounding to fp32
    assert np.array_equal(v, (0.5 * v0).astype(np.float32).astype(np.float64) * 2.0)
    net.close()


def test_compute_objf_leaves_parameters_and_statistics(kctc, gpu, lda_path, refs):
    net, upd, relu = _net(kctc, lda_path, refs, False)
    _, _, fl, ll, dev = _feats(gpu, False)
    nf = np.array(F.LENS, np.int32)
    net.train_step(dev, F.T, N, nf, fl, ll)
    before = [net.get_params(c) for c in upd], net.get_component(relu).nonlinear_stats()
    assert before[1][2] == F.T * N and before[1][1].sum() > 0
    o1, _, _ = net.compute_objf(dev, F.T, N, nf, fl, ll)
    o2, _, _ = net.compute_objf(dev, F.T, N, nf, fl, ll)
    assert o1 == o2
    after = [net.get_params(c) for c in upd], net.get_component(relu).nonlinear_stats()
    for a, b in zip(before[0], after[0]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(before[1], after[1]):
        np.testing.assert_array_equal(a, b)
    net.close()


def test_plain_network_is_untouched_by_an_ft_network(kctc, gpu, lda_path, refs):
    """no shared state: the default recipe network's step is bit-identical before
    and after a FT network lived in the process"""
    import torch
    D, A, T, n = 24, 11, 30, 4
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=64, num_targets=A, learning_rate=0.02, param_stddev=0.2)
    feats, nf, fl, ll = kctc.synth_minibatch(5, T, n, D, A, 0.2)
    fd = torch.from_numpy(feats).to(gpu)

    def step():
        net = kctc.Nnet(cfg, seed=5)
        objf, _, _ = net.train_step(fd, T, n, nf, fl, ll)
        out = objf, [net.get_params(c) for c in range(net.num_components) if net.num_params(c)]
        net.close()
        return out

    o0, p0 = step()
    ft, _, _ = _net(kctc, lda_path, refs, False)
    _, _, fl2, ll2, dev = _feats(gpu, False)
    ft.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl2, ll2)
    ft.close()
    o1, p1 = step()
    assert o0 == o1
    for a, b in zip(p0, p1):
        np.testing.assert_array_equal(a, b)
