"""Variable-length batches on the decode side (include/kaldi_ctc_decode.h):
Nnet.propagate_batch / decodable_batch against the fp64 oracle run on every
utterance alone (RNN -> RNN -> affine -> softmax, then oracle.ctc_decodable).

The models' parameters are drawn here (numpy streams) and installed with
set_params, so the oracle side needs no GPU; MODELS' seeds were picked so that
no oracle probs[t, 0] lies within 1e-4 relative of the blank threshold (a frame
that close could be kept on one side and skipped on the other), which the
tests assert before comparing."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

D, A = 40, 11
THRESHOLDS = (1.0, 0.4)
MODELS = {
    # 2 x BLSTM-64 + affine + Softmax
    "h64": dict(H=64, lens=[41, 17, 33, 2, 41], seed=31),
    # H = 256: the v6 recurrences, which an ordinary Forward would chain
    "h256": dict(H=256, lens=[24, 9, 1, 24, 16, 20], seed=22),
}


def _cfg(kctc, H, ctx=(0,), dim=D):
    return kctc.recipe_config(num_rnn=2, input_dim=dim, hidden=H, num_targets=A, param_stddev=0.1,
                              splice_context=ctx) + f"SoftmaxComponent dim={A}\n"


def _params(oracle, H, seed, in_dim=D):
    """parameters of components 1, 3 (BLSTMs) and 5 (affine: [A][2H] then the bias)"""
    rng = np.random.default_rng([seed, 1])
    p = [(rng.standard_normal(oracle.params_size(2, d, H, 1, 2)) * 0.1).astype(np.float32) for d in (in_dim, 2 * H)]
    W = (rng.standard_normal((A, 2 * H)) * (6.0 / np.sqrt(2 * H))).astype(np.float32)
    b = (rng.standard_normal(A) * 0.3).astype(np.float32)
    b[0] += 1.9  # blank-heavy, as a trained CTC model: frames on both sides of the 0.4 threshold, and in
    # each model one short utterance with no frame below it (the keep-all rule)
    return p + [np.concatenate([W.ravel(), b])]


def _utts(seed, lens, dim=D):
    rng = np.random.default_rng([seed, 2])
    return [rng.standard_normal((L, dim)).astype(np.float32) for L in lens]


def _priors(seed):
    pr = (np.random.default_rng([seed, 3]).random(A) + 0.05).astype(np.float32)
    return pr / pr.sum()


def _oracle_probs(oracle, params, feats, H):
    T = feats.shape[0]
    x = feats.reshape(T, 1, -1).astype(np.float64)
    for w in params[:2]:
        x, _ = oracle.rnn_forward(2, x, w.astype(np.float64), H, 1, 2)
    aff = params[2].astype(np.float64)
    logits = x.reshape(T, -1) @ aff[:-A].reshape(A, -1).T + aff[-A:]
    return oracle.softmax_rows(logits.astype(np.float32))


@pytest.fixture(scope="module")
def refs(oracle):
    """per model: parameters, utterances, priors and the oracle's per-utterance probs (computed once)"""
    out = {}
    for name, m in MODELS.items():
        params = _params(oracle, m["H"], m["seed"])
        utts = _utts(m["seed"], m["lens"])
        out[name] = dict(params=params, utts=utts, priors=_priors(m["seed"]),
                         probs=[_oracle_probs(oracle, params, u, m["H"]) for u in utts])
    return out


def _net(kctc, name, ref):
    net = kctc.Nnet(_cfg(kctc, MODELS[name]["H"]), seed=1)
    for c, p in zip((1, 3, 5), ref["params"]):
        net.set_params(c, p)
    net.set_priors(ref["priors"])
    return net


def _assert_clear_of_threshold(probs_list, thr):
    for n, p in enumerate(probs_list):
        gap = np.abs(p[:, 0].astype(np.float64) - thr) / thr
        assert gap.min() > 1e-4, (n, int(gap.argmin()), float(gap.min()))


@pytest.mark.parametrize("name", list(MODELS))
def test_propagate_batch_matches_oracle_per_utterance(kctc, gpu, refs, name):
    import torch
    ref = refs[name]
    net = _net(kctc, name, ref)
    outs = net.propagate_batch([torch.from_numpy(u).to(gpu) for u in ref["utts"]])
    assert len(outs) == len(ref["utts"])
    for n, (o, r) in enumerate(zip(outs, ref["probs"])):
        assert tuple(o.shape) == r.shape
        e = rel_err(o.cpu().numpy(), r)
        print(f"{name} utt {n} len {r.shape[0]} rel_err {e:.2e}")
        assert e < 1e-5, (n, e)
    net.close()


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_decodable_batch_matches_oracle(kctc, gpu, oracle, refs, name, thr):
    import torch
    ref = refs[name]
    _assert_clear_of_threshold(ref["probs"], thr)
    net = _net(kctc, name, ref)
    f = [torch.from_numpy(u).to(gpu) for u in ref["utts"]]
    probs = [p.cpu().numpy() for p in net.propagate_batch(f)]
    outs = net.decodable_batch(f, prob_scale=0.9, blank_threshold=thr)
    kept = []
    for n, (o, p) in enumerate(zip(outs, probs)):
        r = oracle.ctc_decodable(p, ref["priors"], 0.9, thr, 1e-10)
        assert o.shape == r.shape, (n, o.shape, r.shape)
        np.testing.assert_allclose(o, r, rtol=1e-6, atol=1e-5)
        kept.append(o.shape[0])
    print(name, thr, "kept", kept, "of", [u.shape[0] for u in ref["utts"]])
    if thr < 1.0:  # the threshold does skip frames somewhere
        assert sum(kept) < sum(u.shape[0] for u in ref["utts"])
    else:
        assert kept == [u.shape[0] for u in ref["utts"]]
    net.close()


def test_utterance_does_not_depend_on_its_neighbours(kctc, gpu, refs):
    import torch
    ref = refs["h64"]
    net = _net(kctc, "h64", ref)
    f = [torch.from_numpy(u).to(gpu) for u in ref["utts"]]
    others = [torch.from_numpy(u).to(gpu) for u in _utts(99, [5, 41, 30])]
    for thr in THRESHOLDS:
        a = net.decodable_batch(f, 0.9, thr)[0]
        b = net.decodable_batch([f[0]] + others, 0.9, thr)[0]
        c = net.decodable_batch([f[0]], 0.9, thr)[0]
        assert a.shape == b.shape == c.shape
        np.testing.assert_allclose(b, a, rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(c, a, rtol=1e-6, atol=1e-5)
    net.close()


def test_spliced_model_gives_per_utterance_rows(kctc, gpu):
    import torch
    ctx, dim = (-2, 0, 1), 12
    net = kctc.Nnet(_cfg(kctc, 64, ctx, dim), seed=4)
    net.set_priors(_priors(5))
    f = [torch.from_numpy(u).to(gpu) for u in _utts(7, [30, 11, 4, 30], dim)]
    for thr in (1.0, 0.1):
        outs = net.decodable_batch(f, 0.9, thr)
        for u, o in zip(f, outs):
            one = net.decodable(u, u.shape[0], 0.9, thr)
            assert o.shape == one.shape
            np.testing.assert_allclose(o, one, rtol=1e-6, atol=1e-5)
    with pytest.raises(kctc.KctcError):
        net.propagate_batch(f)
    net.close()


def test_groups_come_back_in_input_order(kctc, gpu, refs):
    import torch
    ref = refs["h64"]
    net = _net(kctc, "h64", ref)
    f = [torch.from_numpy(u).to(gpu) for u in ref["utts"]]
    whole = net.decodable_batch(f, 0.9, 0.4, batch_size=16)
    pairs = net.decodable_batch(f, 0.9, 0.4, batch_size=2)
    assert len(pairs) == len(f) == 5
    for n, (a, b) in enumerate(zip(whole, pairs)):
        assert a.shape == b.shape, n
        np.testing.assert_allclose(b, a, rtol=1e-6, atol=1e-5)
    # distinct utterances: an order mix-up would show
    assert not np.allclose(whole[0][:2], whole[2][:2])
    net.close()


def test_bad_lengths_are_refused(kctc, gpu, refs):
    import torch
    net = _net(kctc, "h64", refs["h64"])
    with pytest.raises(kctc.KctcError):
        net.decodable_batch([torch.zeros((0, D), device=gpu)])
    net.close()
