"""Forced alignment at the network level (include/kaldi_ctc_decode.h:
kctc_nnet_align, kctc_nnet_align_egs) on 2 x BLSTM-32 -> affine to A = 11 with
utterances of 30 / 17 / 9 / 26 frames (the shapes of
tests/test_train_seq_gpu.py): a batch aligns as every utterance alone, a final
SoftmaxComponent changes nothing, an egs archive gives the Int32Vector table,
and an alignment leaves no state behind."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R, D, H, A, T = 2, 24, 32, 11, 30
LENS = [30, 17, 9, 26]


def _config(kctc):
    return kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=2, learning_rate=0.02,
                              param_stddev=0.2)


def _labels(rng, k):
    lab, prev = [], -1
    for _ in range(k):
        v = int(rng.integers(1, A))
        while v == prev:
            v = int(rng.integers(1, A))
        lab.append(v)
        prev = v
    return lab


def _minibatch(seed=3):
    """feats [T, N, D] (padding rows hold 1e3), labels per utterance"""
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((T, len(LENS), D)).astype(np.float32)
    labels = []
    for n, t in enumerate(LENS):
        feats[t:, n] = 1e3
        labels.append(_labels(rng, max(1, t // 5)))
    return feats, labels


def _flat(labels):
    return (np.array([v for l in labels for v in l], np.int32), np.array([len(l) for l in labels], np.int32))


def _dev(gpu, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)


def _align_alone(kctc, gpu, net, feats_n, labels_n):
    """ctc_align on Nnet.propagate of one utterance (N = 1)"""
    import torch
    t = feats_n.shape[0]
    out = net.propagate(_dev(gpu, feats_n), t, 1)
    ali, scores = kctc.ctc_align(out.reshape(t, 1, A).contiguous(), np.array(labels_n, np.int32),
                                 [len(labels_n)], [t])
    torch.cuda.synchronize()
    return ali.cpu().numpy()[:, 0], scores[0]


def test_align_batch_equals_every_utterance_alone(kctc, gpu):
    feats, labels = _minibatch()
    fl, ll = _flat(labels)
    N = len(LENS)
    net = kctc.Nnet(_config(kctc), seed=5)
    ali, scores = net.align(_dev(gpu, feats.reshape(T * N, D)), T, N, LENS, fl, ll)
    assert ali.shape == (T, N) and ali.dtype == np.int32 and scores.shape == (N,)
    for n, t in enumerate(LENS):
        a1, s1 = _align_alone(kctc, gpu, net, feats[:t, n], labels[n])
        assert np.array_equal(ali[:t, n], a1)
        assert np.all(ali[t:, n] == -1)
        np.testing.assert_allclose(scores[n], s1, rtol=1e-6)
        assert np.isfinite(scores[n]) and scores[n] < 0
    # a second call: identical
    ali2, scores2 = net.align(_dev(gpu, feats.reshape(T * N, D)), T, N, LENS, fl, ll)
    assert np.array_equal(ali, ali2) and np.array_equal(scores, scores2)

    # the recipe's final.mdl ends in a SoftmaxComponent: the alignment runs on its input
    net.insert(net.num_components, f"SoftmaxComponent dim={A}")
    ali3, scores3 = net.align(_dev(gpu, feats.reshape(T * N, D)), T, N, LENS, fl, ll)
    assert np.array_equal(ali, ali3) and np.array_equal(scores, scores3)
    net.close()


def test_align_egs_writes_the_table(kctc, gpu, tmp_path):
    rng = np.random.default_rng(23)
    egs, ark = "ark:" + str(tmp_path / "train.egs"), "ark:" + str(tmp_path / "ali.ark")
    examples = []
    with kctc.EgsWriter(egs) as w:
        for i, t in enumerate([30, 17, 12, 9, 26]):
            feats = rng.standard_normal((t, D)).astype(np.float32)
            lab = [3] * 20 if i == 2 else _labels(rng, max(1, t // 5))  # example 2: 20 labels + 19 repeats in 12 frames
            w.write(f"utt{i}", feats, np.array(lab, np.int32))
            examples.append((f"utt{i}", kctc.cm_decompress(kctc.cm_compress(feats)), lab))
    net = kctc.Nnet(_config(kctc), seed=5)
    st = net.align_egs(egs, ark, minibatch_size=2)
    table = kctc.read_int_vector_ark(ark)
    assert list(table) == ["utt0", "utt1", "utt3", "utt4"]  # archive order, the infeasible one left out
    tot_score, tot_frames = 0.0, 0
    for key, feats, lab in examples:
        if key == "utt2":
            continue
        t = feats.shape[0]
        ali, scores = net.align(_dev(gpu, feats), t, 1, [t], np.array(lab, np.int32), [len(lab)])
        assert table[key].dtype == np.int32 and np.array_equal(table[key], ali[:, 0])
        tot_score += scores[0]
        tot_frames += t
    assert st["num_done"] == 4 and st["num_infeasible"] == 1 and st["tot_frames"] == tot_frames
    np.testing.assert_allclose(st["tot_score"], tot_score, rtol=1e-6)
    net.close()


def test_align_leaves_no_state_behind(kctc, gpu):
    feats, labels = _minibatch()
    fl, ll = _flat(labels)
    N = len(LENS)
    x = _dev(gpu, feats.reshape(T * N, D))
    plain_feats = feats.copy()
    for n, t in enumerate(LENS):
        plain_feats[t:, n] = 0
    y = _dev(gpu, plain_feats.reshape(T * N, D))
    nets = [kctc.Nnet(_config(kctc), seed=5) for _ in range(2)]
    nets[0].align(x, T, N, LENS, fl, ll)
    stats = [net.train_step(y, T, N, LENS, fl, ll) for net in nets]
    assert stats[0] == stats[1]
    for c in range(nets[0].num_components):
        if nets[0].num_params(c) > 0:
            assert np.array_equal(nets[0].get_params(c), nets[1].get_params(c)), c
    for net in nets:
        net.close()
