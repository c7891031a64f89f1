"""Prefix beam search at the network level (include/kaldi_ctc_decode.h:
kctc_nnet_decode, kctc_nnet_decode_egs) on the 2 x BLSTM-32 -> affine to
A = 11 network of tests/test_nnet_align_gpu.py with utterances of 30 / 17 / 9 /
26 frames: Nnet.decode is ctc_beam_search on propagate_batch's output, a final
SoftmaxComponent changes nothing, a batch decodes as every utterance alone,
and an egs archive gives the hypothesis table and the edit distance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, D, H, A, T = 2, 24, 32, 11, 30
LENS = [30, 17, 9, 26]
BEAM, SYMBOLS = 8, 10


def _config(kctc):
    return kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=2, learning_rate=0.02,
                              param_stddev=0.2)


def _feats(seed=3):
    """feats [T, N, D]; the padding rows hold 1e3"""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((T, len(LENS), D)).astype(np.float32)
    for n, t in enumerate(LENS):
        feats[t:, n] = 1e3
    return feats


def _dev(gpu, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)


def test_decode_is_beam_search_on_the_batched_forward(kctc, gpu):
    import torch
    feats = _feats()
    N = len(LENS)
    net = kctc.Nnet(_config(kctc), seed=5)
    x = _dev(gpu, feats.reshape(T * N, D))
    hyps, scores = net.decode(x, T, N, LENS, beam=BEAM, symbols=SYMBOLS)
    assert len(hyps) == N and scores.shape == (N,) and scores.dtype == np.float64
    for n, t in enumerate(LENS):
        assert len(hyps[n]) <= t and all(0 < v < A for v in hyps[n])
        assert np.isfinite(scores[n]) and scores[n] < 0
    # the same search on the variable-length forward's output
    outs = net.propagate_batch([_dev(gpu, feats[:t, n]) for n, t in enumerate(LENS)])
    acts = torch.zeros((T, N, A), dtype=torch.float32, device=gpu)
    for n, t in enumerate(LENS):
        acts[:t, n] = outs[n]
    h2, s2 = kctc.ctc_beam_search(acts.contiguous(), LENS, beam=BEAM, symbols=SYMBOLS)
    assert hyps == h2 and np.array_equal(scores, s2)
    # every utterance alone
    for n, t in enumerate(LENS):
        h1, s1 = net.decode(_dev(gpu, feats[:t, n]), t, 1, [t], beam=BEAM, symbols=SYMBOLS)
        assert h1[0] == hyps[n]
        np.testing.assert_allclose(s1[0], scores[n], rtol=1e-6)
    # a second call: identical
    h3, s3 = net.decode(x, T, N, LENS, beam=BEAM, symbols=SYMBOLS)
    assert h3 == hyps and np.array_equal(s3, scores)

    # the recipe's final.mdl ends in a SoftmaxComponent: the search runs on its input
    net.insert(net.num_components, f"SoftmaxComponent dim={A}")
    h4, s4 = net.decode(x, T, N, LENS, beam=BEAM, symbols=SYMBOLS)
    assert h4 == hyps and np.array_equal(s4, scores)
    net.close()


def test_decode_egs_writes_the_table_and_counts_errors(kctc, gpu, tmp_path):
    rng = np.random.default_rng(23)
    egs, ark = "ark:" + str(tmp_path / "test.egs"), "ark:" + str(tmp_path / "hyp.ark")
    examples = []
    with kctc.EgsWriter(egs) as w:
        for i, t in enumerate([30, 17, 12, 9, 26]):
            feats = rng.standard_normal((t, D)).astype(np.float32)
            lab = rng.integers(1, A, size=max(1, t // 5)).astype(np.int32)
            w.write(f"utt{i}", feats, lab)
            examples.append((f"utt{i}", kctc.cm_decompress(kctc.cm_compress(feats)), lab))
    net = kctc.Nnet(_config(kctc), seed=5)
    num_utts, num_labels, edit_distance = net.decode_egs(egs, ark, minibatch_size=2, beam=BEAM, symbols=SYMBOLS)
    table = kctc.read_int_vector_ark(ark)
    assert list(table) == [k for k, _, _ in examples]  # archive order
    errs = 0
    for key, feats, lab in examples:
        t = feats.shape[0]
        hyps, _ = net.decode(_dev(gpu, feats), t, 1, [t], beam=BEAM, symbols=SYMBOLS)
        assert table[key].dtype == np.int32 and table[key].tolist() == hyps[0]
        errs += kctc.levenshtein(lab, np.array(hyps[0], np.int32))
    assert num_utts == len(examples) and num_labels == sum(len(lab) for _, _, lab in examples)
    assert edit_distance == errs
    net.close()
