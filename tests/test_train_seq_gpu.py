"""Length-aware training (kctc_nnet_set_length_aware, include/kaldi_ctc_train.h):
a padded minibatch trains as if every utterance were a minibatch of its own.

Reference: the fp64 oracle's train step on each utterance alone (N = 1, T =
num_frames[n]) from the same parameters, with lr = 1, the RNN update clamp
out of reach and self-repair off, so that (new - old parameters) is the
gradient.  kctc_nnet_get_grad (the pre-clamp gradient) of every updatable
component must equal the SUM of those within 1e-4 (norm-wise relative, the
project's bar for gradients), the per-utterance costs within 1e-5 relative.
Padding rows of the features hold 1e3 in the length-aware steps."""
import functools

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

R, D, A, T, LR = 2, 24, 11, 30, 0.02
LENS4 = [30, 17, 9, 26]
LENS12 = [30, 5, 17, 9, 26, 30, 12, 3, 21, 28, 7, 15]  # two row groups of 8 (KCTC_REC_GS=8)

NETS = {
    # id: (mode, H, lens, param_stddev, clipping_threshold, env)
    "blstm64": (2, 64, LENS4, 0.2, 30.0, {}),
    "bgru48": (3, 48, LENS4, 0.2, 30.0, {}),
    "blstm256_two_groups_of_8": (2, 256, LENS12, 0.1, 30.0, {"KCTC_REC_GS": "8"}),
    # every row clipped: norm-based clipping works per row, so the sum over utterances still holds
    "blstm64_clip0.02": (2, 64, LENS4, 0.2, 0.02, {}),
}


def _config(kctc, mode, H, pstd, thr):
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode, learning_rate=LR,
                             clipping_threshold=thr, param_stddev=pstd)
    # no self-repair: it adds a term that is not a gradient (and draws from rand())
    assert "norm-based-clipping=" in cfg
    return cfg.replace("norm-based-clipping=", "self-repair-scale=0 norm-based-clipping=")


def _minibatch(lens, seed, pad):
    """feats [T, N, D] (rows t >= lens[n] hold `pad`), flat labels, label lengths"""
    rng = np.random.default_rng(seed)
    N = len(lens)
    feats = rng.standard_normal((T, N, D)).astype(np.float32)
    labels = []
    for n, L in enumerate(lens):
        feats[L:, n] = pad
        k = min(max(1, int(0.2 * L)), (L - 1) // 2)
        lab, prev = [], -1
        for _ in range(k):
            v = int(rng.integers(1, A))
            while v == prev:
                v = int(rng.integers(1, A))
            lab.append(v)
            prev = v
        labels.append(lab)
    fl = np.array([v for l in labels for v in l], np.int32)
    ll = np.array([len(l) for l in labels], np.int32)
    return feats, labels, fl, ll


def _spec(oracle, mode, H, thr):
    s = oracle.NnetSpec()
    s.num_rnn, s.mode, s.hidden, s.dirs, s.layers_per_rnn = R, mode, H, 2, 1
    s.input_dim, s.num_targets = D, A
    s.clip_threshold, s.repair_threshold, s.repair_scale, s.repair_target = thr, 0.01, 0.0, 0.0
    s.rnn_clip_gradient, s.lr_rnn, s.lr_affine = 1e30, 1.0, 1.0
    return s


def _oracle_delta(oracle, spec, params, feats, nf, fl, ll):
    """(new - old parameters per updatable component, costs [N], ids [T*N]) of one oracle step"""
    rnn_p = [p.copy() for p in params[:-1]]
    Wa = params[-1][:-A].reshape(A, -1).copy()
    ba = params[-1][-A:].copy()
    ex = {}
    oracle.train_step(spec, rnn_p, Wa, ba, np.ascontiguousarray(feats, dtype=np.float64), nf, fl, ll,
                      repair_draws=np.ones(R, np.float32), extras=ex)
    new = rnn_p + [np.concatenate([Wa.ravel(), ba])]
    return [a - b for a, b in zip(new, params)], ex["costs"], ex["ids"]


def _net(kctc, nid):
    mode, H, lens, pstd, thr, _ = NETS[nid]
    net = kctc.Nnet(_config(kctc, mode, H, pstd, thr), seed=5)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    return net, upd


@functools.lru_cache(maxsize=None)
def _reference(nid):
    """The oracle's side of a case, computed once: the parameters, the padded
    step's delta, the sum of the per-utterance deltas, the per-utterance costs
    and best-path ids."""
    import oracle_lib as oracle
    from conftest import load_kctc
    kctc = load_kctc()
    mode, H, lens, pstd, thr, _ = NETS[nid]
    net, upd = _net(kctc, nid)
    params = [net.get_params(c).astype(np.float64) for c in upd]
    feats, labels, fl, ll = _minibatch(lens, 1000, 0.0)
    spec = _spec(oracle, mode, H, thr)
    padded, _, _ = _oracle_delta(oracle, spec, params, feats, np.array(lens, np.int32), fl, ll)
    total, costs, ids = [np.zeros_like(p) for p in params], [], []
    for n, L in enumerate(lens):
        d, c, i = _oracle_delta(oracle, spec, params, feats[:L, n:n + 1], np.array([L], np.int32),
                                np.array(labels[n], np.int32), np.array([len(labels[n])], np.int32))
        total = [a + b for a, b in zip(total, d)]
        costs.append(c[0])
        ids.append(i)
    for a in padded + total:
        a.setflags(write=False)
    return padded, total, np.array(costs), ids


def _step(kctc, gpu, nid, length_aware, pad):
    """A fresh net's train step -> (net, gradients per updatable component, objf)"""
    import torch
    _, _, lens, _, _, _ = NETS[nid]
    net, upd = _net(kctc, nid)
    feats, _, fl, ll = _minibatch(lens, 1000, pad)
    net.set_length_aware(length_aware)
    objf, _, wt = net.train_step(torch.from_numpy(feats.reshape(T * len(lens), D)).to(gpu), T, len(lens),
                                 np.array(lens, np.int32), fl, ll)
    assert wt == ll.sum()
    return net, [net.get_grad(c).astype(np.float64) for c in upd], objf


@pytest.mark.parametrize("nid", list(NETS))
def test_length_aware_gradient_is_sum_of_per_utterance_gradients(kctc, gpu, oracle, monkeypatch, nid):
    mode, H, lens, pstd, thr, env = NETS[nid]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    N = len(lens)
    padded, total, costs, ids = _reference(nid)
    # get_grad's sign and scale: the default step against the oracle's padded step
    _, g_def, _ = _step(kctc, gpu, nid, False, 0.0)
    sign = []
    for i, (g, d) in enumerate(zip(g_def, padded)):
        k = float(np.dot(g, d) / np.dot(g, g))
        print(f"{nid} component {i}: oracle delta = {k:+.6f} * get_grad, rel err {rel_err(round(k) * g, d):.2e}")
        assert abs(abs(k) - 1.0) < 1e-3, (i, k)
        sign.append(round(k))
        assert rel_err(sign[i] * g, d) < 1e-4, i
    net, g_la, objf = _step(kctc, gpu, nid, True, 1e3)
    for i, (g, d, s) in enumerate(zip(g_la, total, sign)):
        e, gap = rel_err(s * g, d), rel_err(s * g_def[i], d)
        print(f"{nid} component {i}: length-aware vs per-utterance sum {e:.2e}; default vs the sum {gap:.2e}; "
              f"max |sum| {np.abs(d).max():.3g}")
        assert e < 1e-4, (i, e)
        # the inputs discriminate: the default (padded) gradient is another one, a hundred times the bar away
        assert gap > 1e-2, (i, gap)
    # the affine bias gradient is the column sum of the CTC derivative over ALL T*N rows: it equals the
    # per-utterance sum only if that derivative is zero on the padding rows
    eb = rel_err(sign[-1] * g_la[-1][-A:], total[-1][-A:])
    print(f"{nid} affine bias gradient vs per-utterance sum {eb:.2e}")
    assert eb < 1e-4, eb
    got = net.last_costs(N)
    print(f"{nid} costs rel err {np.abs(got / costs - 1).max():.2e}")
    np.testing.assert_allclose(got, costs, rtol=1e-5)
    np.testing.assert_allclose(objf, costs.sum(), rtol=1e-5)
    # best paths on the real rows: each utterance's own (fp32 against fp64 logits: a near-tie may flip a frame)
    best = net.last_best_path(T, N).reshape(T, N)
    for n, L in enumerate(lens):
        assert (best[:L, n] != ids[n]).sum() <= 1, n


def _objf_data(lens, pad):
    feats, labels, fl, ll = _minibatch(lens, 1000, pad)
    return feats, labels, fl, ll


def test_compute_objf_length_aware_is_sum_of_single_utterance_calls(kctc, gpu):
    import torch
    nid = "blstm64"
    lens = NETS[nid][2]
    N = len(lens)
    net, _ = _net(kctc, nid)
    feats, labels, fl, ll = _objf_data(lens, 1e3)
    net.set_length_aware(True)
    objf, acc, wt = net.compute_objf(torch.from_numpy(feats.reshape(T * N, D)).to(gpu), T, N, np.array(lens, np.int32),
                                     fl, ll)
    net.set_length_aware(False)
    tot, tacc = 0.0, 0.0
    for n, L in enumerate(lens):
        one = torch.from_numpy(np.ascontiguousarray(feats[:L, n])).to(gpu)
        o, a, _ = net.compute_objf(one, L, 1, np.array([L], np.int32), np.array(labels[n], np.int32),
                                   np.array([len(labels[n])], np.int32))
        tot += o
        tacc += a
    print(f"length-aware objf {objf!r}, sum of N = 1 calls {tot!r}")
    np.testing.assert_allclose(objf, tot, rtol=1e-5)
    assert abs(acc - tacc) <= 1
    assert wt == ll.sum()


def test_mode_off_after_length_aware_objf_restores_the_default_step_bitwise(kctc, gpu):
    import torch
    nid = "blstm64"
    lens = NETS[nid][2]
    N = len(lens)
    feats, _, fl, ll = _objf_data(lens, 0.0)
    fd = torch.from_numpy(feats.reshape(T * N, D)).to(gpu)
    nf = np.array(lens, np.int32)
    fresh, upd = _net(kctc, nid)
    fresh.train_step(fd, T, N, nf, fl, ll)
    net, _ = _net(kctc, nid)
    net.train_step(fd, T, N, nf, fl, ll)  # default state (chained projection, prepacks) exists
    net2, _ = _net(kctc, nid)
    for c in upd:  # back to the initial parameters, keeping the cached state
        net.set_params(c, net2.get_params(c))
    net.set_length_aware(True)
    net.compute_objf(fd, T, N, nf, fl, ll)
    net.set_length_aware(False)
    net.train_step(fd, T, N, nf, fl, ll)
    for c in upd:
        assert np.array_equal(net.get_params(c), fresh.get_params(c)), c


def test_length_aware_refuses_65_utterances_and_bf16(kctc, gpu):
    import torch
    nid = "blstm64"
    net, _ = _net(kctc, nid)
    net.set_length_aware(True)
    Tn, N = 6, 65
    feats = torch.zeros((Tn * N, D), device=gpu)
    nf, ll = np.full(N, Tn, np.int32), np.ones(N, np.int32)
    fl = np.ones(N, np.int32)
    with pytest.raises(kctc.KctcError, match="64"):
        net.train_step(feats, Tn, N, nf, fl, ll)
    with pytest.raises(kctc.KctcError, match="64"):
        net.compute_objf(feats, Tn, N, nf, fl, ll)
    with pytest.raises(kctc.KctcError, match="length-aware"):
        net.set_precision("bf16")
    net.set_length_aware(False)
    net.set_precision("bf16")
    with pytest.raises(kctc.KctcError, match="bf16"):
        net.set_length_aware(True)
    net.set_precision(0)
    net.set_length_aware(True)


def test_length_aware_refused_with_minibatches_in_flight(kctc, gpu):
    import torch
    nid = "blstm64"
    lens = NETS[nid][2]
    N = len(lens)
    net, _ = _net(kctc, nid)
    feats, _, fl, ll = _objf_data(lens, 0.0)
    fd = torch.from_numpy(feats.reshape(T * N, D)).to(gpu)
    assert net.train_step_async(fd, T, N, np.array(lens, np.int32), fl, ll) is None
    with pytest.raises(kctc.KctcError, match="in flight"):
        net.set_length_aware(True)
    assert len(net.train_flush()) == 1
    net.set_length_aware(True)


def test_length_aware_full_lengths_match_the_default_step(kctc, gpu):
    """All lengths T: the same function, other GEMM paths (nothing streamed) --
    no bitwise equality, 1e-6 norm-wise."""
    import torch
    nid = "blstm64"
    N = 4
    rng = np.random.default_rng(3)
    feats = torch.from_numpy(rng.standard_normal((T * N, D)).astype(np.float32)).to(gpu)
    nf = np.full(N, T, np.int32)
    ll = np.full(N, 5, np.int32)
    fl = np.tile(np.array([1, 4, 2, 7, 3], np.int32), N)
    out = []
    for on in (False, True):
        net, upd = _net(kctc, nid)
        net.set_length_aware(on)
        objf, _, _ = net.train_step(feats, T, N, nf, fl, ll)
        out.append((objf, [net.get_grad(c) for c in upd], [net.get_params(c) for c in upd]))
    (o0, g0, p0), (o1, g1, p1) = out
    np.testing.assert_allclose(o1, o0, rtol=1e-6)
    for i in range(len(g0)):
        print(f"component {i}: grad {rel_err(g1[i], g0[i]):.2e} params {rel_err(p1[i], p0[i]):.2e}")
        assert rel_err(g1[i], g0[i]) < 1e-6, i
        assert rel_err(p1[i], p0[i]) < 1e-6, i
