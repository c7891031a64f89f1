"""Graph search at the network level (include/kaldi_ctc_decode.h:
kctc_nnet_decode_graph, kctc_nnet_decode_graph_egs) on the 2 x BLSTM-32 ->
affine to A = 11 network of tests/test_nnet_decode_gpu.py with utterances of
30 / 17 / 9 / 26 frames: Nnet.decode_graph is wfst_decode on the decodable rows
computed from propagate_batch's output, a final SoftmaxComponent changes
nothing, the priors are applied, a batch decodes as every utterance alone, and
an egs archive gives the word table and the alignment table in archive order
with the counts of per-utterance calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, D, H, A, T = 2, 24, 32, 11, 30
LENS = [30, 17, 9, 26]
BEAM, MAX_ACTIVE, PROB_SCALE = 12.0, 50, 0.8


def _config(kctc):
    return kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=2, learning_rate=0.02,
                              param_stddev=0.2)


def _feats(seed=3):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((T, len(LENS), D)).astype(np.float32)
    for n, t in enumerate(LENS):
        feats[t:, n] = 1e3
    return feats


def _dev(gpu, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)


def _lexicon(kctc):
    rng = np.random.default_rng(11)
    lex = [(w + 1, rng.integers(1, A, size=int(rng.integers(1, 4))).tolist()) for w in range(12)]
    return kctc.ctc_lexicon_graph(lex, A, rng.random(12) * 0.5)


def _decodable(kctc, gpu, net, feats, priors):
    """[T, N, A] rows (log(max(softmax, 1e-10)) - log prior) * PROB_SCALE from the batched forward, NaN padding"""
    import torch
    outs = net.propagate_batch([_dev(gpu, feats[:t, n]) for n, t in enumerate(LENS)])
    ll = torch.full((T, len(LENS), A), float("nan"), dtype=torch.float32, device=gpu)
    for n, t in enumerate(LENS):
        p = kctc.softmax_rows(outs[n])
        ll[:t, n] = kctc.ctc_decodable(p, None if priors is None else _dev(gpu, priors), prob_scale=PROB_SCALE)
    return ll.contiguous()


def _same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def test_decode_graph_is_wfst_decode_on_the_decodable_rows(kctc, gpu):
    feats = _feats()
    N = len(LENS)
    graph = _lexicon(kctc)
    net = kctc.Nnet(_config(kctc), seed=5)
    x = _dev(gpu, feats.reshape(T * N, D))
    kw = dict(beam=BEAM, max_active=MAX_ACTIVE, prob_scale=PROB_SCALE, acoustic_scale=1.5)
    got = net.decode_graph(x, T, N, LENS, graph, **kw)
    words, ali, scores, status = got
    assert ali.shape == (T, N) and scores.dtype == np.float64
    for n, t in enumerate(LENS):
        assert status[n] == 1 and (ali[:t, n] >= 1).all() and (ali[t:, n] == -1).all() and np.isfinite(scores[n])
    assert sum(len(w) for w in words) > 0
    want = kctc.wfst_decode(_decodable(kctc, gpu, net, feats, None), LENS, graph, beam=BEAM, max_active=MAX_ACTIVE,
                            acoustic_scale=1.5)
    _same(got, want)
    # a second call, and every utterance alone
    _same(net.decode_graph(x, T, N, LENS, graph, **kw), got)
    for n, t in enumerate(LENS):
        w1, a1, s1, st1 = net.decode_graph(_dev(gpu, feats[:t, n]), t, 1, [t], graph, **kw)
        assert w1[0] == words[n] and st1[0] == status[n] and np.array_equal(a1[:, 0], ali[:t, n])
        np.testing.assert_allclose(s1[0], scores[n], rtol=1e-6)

    # priors: applied as CtcDecodableAmNnet applies them, and they matter
    priors = np.random.default_rng(2).dirichlet(np.ones(A)).astype(np.float32)
    net.set_priors(priors)
    with_priors = net.decode_graph(x, T, N, LENS, graph, **kw)
    _same(with_priors, kctc.wfst_decode(_decodable(kctc, gpu, net, feats, priors), LENS, graph, beam=BEAM,
                                        max_active=MAX_ACTIVE, acoustic_scale=1.5))
    assert not np.array_equal(with_priors[2], scores)

    # the recipe's final.mdl ends in a SoftmaxComponent: no second softmax
    net.insert(net.num_components, f"SoftmaxComponent dim={A}")
    _same(net.decode_graph(x, T, N, LENS, graph, **kw), with_priors)

    # a graph that reads a column the network does not have is refused
    with pytest.raises(kctc.KctcError):
        net.decode_graph(x, T, N, LENS, kctc.ctc_token_graph(A + 1), **kw)
    net.close()


def test_decode_graph_egs_writes_both_tables(kctc, gpu, tmp_path):
    rng = np.random.default_rng(23)
    egs = "ark:" + str(tmp_path / "test.egs")
    wark, aark = "ark:" + str(tmp_path / "words.ark"), "ark:" + str(tmp_path / "ali.ark")
    examples = []
    with kctc.EgsWriter(egs) as w:
        for i, t in enumerate([30, 17, 12, 9, 26]):
            feats = rng.standard_normal((t, D)).astype(np.float32)
            lab = rng.integers(1, A, size=max(1, t // 5)).astype(np.int32)
            w.write(f"utt{i}", feats, lab)
            examples.append((f"utt{i}", kctc.cm_decompress(kctc.cm_compress(feats))))
    graph = _lexicon(kctc)
    net = kctc.Nnet(_config(kctc), seed=5)
    kw = dict(beam=BEAM, max_active=MAX_ACTIVE, prob_scale=PROB_SCALE)
    res = net.decode_graph_egs(egs, wark, graph, ali_wspecifier=aark, minibatch_size=2, **kw)
    wt, at = kctc.read_int_vector_ark(wark), kctc.read_int_vector_ark(aark)
    assert list(wt) == list(at) == [k for k, _ in examples]  # archive order
    tot, fin, frames = 0.0, 0, 0
    for key, feats in examples:
        t = feats.shape[0]
        words, ali, scores, status = net.decode_graph(_dev(gpu, feats), t, 1, [t], graph, **kw)
        assert status[0] >= 0
        assert wt[key].dtype == np.int32 and wt[key].tolist() == words[0]
        assert at[key].tolist() == ali[:, 0].tolist()
        tot += scores[0]
        fin += int(status[0] == 1)
        frames += t
    assert res["num_done"] == len(examples) and res["num_failed"] == 0
    assert res["num_final"] == fin and res["tot_frames"] == frames
    np.testing.assert_allclose(res["tot_score"], tot, rtol=1e-6)
    # without the alignment table; a pool that no utterance fits: counted, not written
    res2 = net.decode_graph_egs(egs, wark, graph, minibatch_size=3, pool_tokens=2, **kw)
    assert res2["num_done"] == 0 and res2["num_failed"] == len(examples) and res2["tot_frames"] == 0
    assert kctc.read_int_vector_ark(wark) == {}
    net.close()
