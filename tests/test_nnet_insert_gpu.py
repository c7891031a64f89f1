"""nnet-insert (InsertComponents, src/nnet2/nnet-functions.cc:39-55, with
--randomize-next-component=false) through Nnet.insert: the BLSTM that
steps/ctc/train.sh:357-384 adds every add_layers_period iterations, and the
SoftmaxComponent that train.sh:472-478 appends for decoding."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, H, A = 16, 32, 9


def _cfg(kctc, num_rnn):
    return kctc.recipe_config(num_rnn=num_rnn, input_dim=D, hidden=H, num_targets=A, learning_rate=0.01,
                              param_stddev=0.2)


def _infos(net):
    return [net.info(c) for c in range(net.num_components)]


def test_insert_grows_the_network_by_one_rnn(kctc, gpu):
    import torch
    two = _cfg(kctc, 2).splitlines()
    rnn_line, clip_line = two[3], two[4]
    assert rnn_line.startswith("CuDNNRecurrentComponent") and clip_line.startswith("ClipGradientComponent")
    net = kctc.Nnet(_cfg(kctc, 1), seed=3)
    assert net.num_components == 4
    old = {c: net.get_params(c) for c in (1, 3)}
    last_rnn = 1
    net.insert(last_rnn + 2, rnn_line + "\n" + clip_line, seed=8)
    direct = kctc.Nnet(_cfg(kctc, 2), seed=5)
    # the component order and infos of the two-RNN config
    assert net.num_components == direct.num_components == 6
    assert _infos(net) == _infos(direct)
    # the old components' parameters, bit for bit (the affine moved from 3 to 5)
    np.testing.assert_array_equal(net.get_params(1), old[1])
    np.testing.assert_array_equal(net.get_params(5), old[3])
    assert net.num_params(3) == direct.num_params(3) > 0
    assert np.isfinite(net.get_params(3)).all() and net.get_params(3).std() > 0.05  # initialised from the config
    # same parameters -> the same forward pass as the directly built network
    for c in (1, 3, 5):
        direct.set_params(c, net.get_params(c))
    T, N = 14, 3
    feats, nf, fl, ll = kctc.synth_minibatch(4, T, N, D, A, 0.2)
    f = torch.from_numpy(feats).to(gpu)
    assert torch.equal(net.propagate(f, T, N), direct.propagate(f, T, N))
    # and the grown network trains
    before = net.get_params(3).copy()
    objf, acc, wt = net.train_step(f, T, N, nf, fl, ll)
    objf2, _, wt2 = direct.train_step(f, T, N, nf, fl, ll)
    assert np.isfinite(objf) and wt == wt2 == ll.sum()
    np.testing.assert_allclose(objf, objf2, rtol=1e-6)
    assert not np.array_equal(net.get_params(3), before)
    for c in (1, 3, 5):  # the same step on the same parameters
        np.testing.assert_allclose(net.get_params(c), direct.get_params(c), rtol=1e-5, atol=1e-7)
    net.close()
    direct.close()


def test_insert_appends_the_softmax(kctc, gpu):
    import torch
    net = kctc.Nnet(_cfg(kctc, 1), seed=3)
    T = 11
    feats = np.random.default_rng(2).standard_normal((T, D)).astype(np.float32)
    f = torch.from_numpy(feats).to(gpu)
    logits = net.propagate(f, T, 1)
    net.insert(net.num_components, f"SoftmaxComponent dim={A}")
    assert net.num_components == 5 and net.info(4).startswith("SoftmaxComponent")
    probs = net.propagate(f, T, 1)
    assert torch.equal(probs, kctc.softmax_rows(logits))
    net.close()


def test_insert_refuses_mismatches(kctc, gpu):
    net = kctc.Nnet(_cfg(kctc, 1), seed=3)
    before = _infos(net)
    with pytest.raises(kctc.KctcError):  # its input dim is not the affine's output dim
        net.insert(net.num_components, f"SoftmaxComponent dim={A + 1}")
    with pytest.raises(kctc.KctcError):  # 2H -> A in the middle: the affine after it wants 2H
        net.insert(3, f"AffineComponent input-dim={2 * H} output-dim={A} learning-rate=0.01")
    with pytest.raises(kctc.KctcError):
        net.insert(-1, f"SoftmaxComponent dim={A}")
    with pytest.raises(kctc.KctcError):
        net.insert(net.num_components + 1, f"SoftmaxComponent dim={A}")
    with pytest.raises(kctc.KctcError):  # frame context anywhere but first
        net.insert(3, f"SpliceComponent input-dim={2 * H} context=-1:0")
    with pytest.raises(kctc.KctcError):
        net.insert(1, "")
    assert _infos(net) == before
    net.close()
