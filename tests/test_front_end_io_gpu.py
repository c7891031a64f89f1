"""Model I/O, averaging, nnet-insert and decoding of the recipe's FT / LDA
networks (RectifiedLinearComponent, FixedAffineComponent).

A FixedAffineComponent has no parameter accessor (it is not updatable): its
parameters are compared as the bytes of its binary Write.  The RectifiedLinear
statistics are fp64 and compared bit for bit; text mode writes them with 17
and the FixedAffine parameters with 9 significant digits, so text round trips
are exact too."""
import numpy as np
import pytest

import front_end_ref as F
from conftest import rel_err

pytestmark = pytest.mark.gpu

N = len(F.LENS)
THR = 0.05  # the front ClipGradient's threshold (any: nothing here depends on which rows clip)


@pytest.fixture(scope="module")
def lda_path(kctc, tmp_path_factory):
    p = tmp_path_factory.mktemp("front_end_io") / "lda.mat"
    kctc.write_kaldi_matrix(p, F.lda_matrix(), binary=False)
    return str(p)


def _net(kctc, lda_path, seed=5):
    return kctc.Nnet(F.config(kctc, lda_path, THR), seed=seed)


def _train(net, gpu, seed=1000):
    import torch
    xs, _, fl, ll = F.minibatch(seed=seed)
    dev = torch.from_numpy(F.format_input(xs, F.LENS, F.T)).to(gpu)
    net.train_step(dev, F.T, N, np.array(F.LENS, np.int32), fl, ll)


def _component_bytes(net, c, tmp_path):
    p = tmp_path / "component.bin"
    net.get_component(c).Write(p, binary=True)
    return p.read_bytes()


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


FIXED, HIDDEN, RELU, RNN = 1, 2, 3, 5


def _same_front_end(a, b, tmp_path):
    assert _component_bytes(a, FIXED, tmp_path) == _component_bytes(b, FIXED, tmp_path)
    sa, sb = a.get_component(RELU).nonlinear_stats(), b.get_component(RELU).nonlinear_stats()
    np.testing.assert_array_equal(_bits64(sa[0]), _bits64(sb[0]))
    np.testing.assert_array_equal(_bits64(sa[1]), _bits64(sb[1]))
    assert sa[2] == sb[2]


def test_fixed_affine_holds_the_matrix_file(kctc, gpu, lda_path, tmp_path):
    net = _net(kctc, lda_path)
    m = F.lda_matrix()
    want = (b"\0B<FixedAffineComponent> <LinearParams> FM \x04" + np.int32(F.DL).tobytes() + b"\x04" +
            np.int32(39).tobytes() + np.ascontiguousarray(m[:, :-1]).tobytes() + b"<BiasParams> FV \x04" +
            np.int32(F.DL).tobytes() + np.ascontiguousarray(m[:, -1]).tobytes() + b"</FixedAffineComponent> ")
    assert _component_bytes(net, FIXED, tmp_path) == want
    net.close()


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("trained", [False, True])
def test_round_trip_is_bit_exact(kctc, gpu, lda_path, tmp_path, binary, trained):
    net = _net(kctc, lda_path)
    if trained:
        _train(net, gpu)
        _train(net, gpu, seed=1001)
    p = tmp_path / "m.nnet"
    net.write(p, binary=binary)
    if not binary:
        text = p.read_text()
        assert "<RectifiedLinearComponent> <Dim> 48 <ValueSum> " in text and "<FixedAffineComponent> <LinearParams> " in text
        assert ("<ValueSum>  [ ]\n<DerivSum>  [ ]\n<Count> 0 </RectifiedLinearComponent>" in text) == (not trained)
    back = kctc.Nnet.read(p)
    assert back.num_components == net.num_components
    for c in range(net.num_components):
        assert back.info(c) == net.info(c), c
    _same_front_end(net, back, tmp_path)
    v, d, n = back.get_component(RELU).nonlinear_stats()
    assert n == (2 * F.T * N if trained else 0) and bool(d.any()) == trained and bool(v.any()) == trained
    if binary:
        for c in (HIDDEN, RNN):
            np.testing.assert_array_equal(back.get_params(c), net.get_params(c))
    # the second generation is the first, byte for byte
    p2 = tmp_path / "m2.nnet"
    back.write(p2, binary=binary)
    if binary:
        assert p2.read_bytes() == p.read_bytes()
    else:
        _same_front_end(kctc.Nnet.read(p2), back, tmp_path)
    back.close()
    net.close()


def test_hand_written_kaldi_text_model_reads(kctc, gpu, tmp_path):
    p = tmp_path / "hand.nnet"
    p.write_text("<Nnet> <NumComponents> 3 <Components> "
                 "<FixedAffineComponent> <LinearParams>  [\n  1 0 2 \n  0 1 -1 ]\n<BiasParams>  [ 0.5 -0.5 ]\n"
                 "</FixedAffineComponent> \n"
                 "<RectifiedLinearComponent> <Dim> 2 <ValueSum>  [ ]\n<DerivSum>  [ ]\n<Count> 0 "
                 "</RectifiedLinearComponent> \n"
                 "<RectifiedLinearComponent> <Dim> 2 <ValueSum>  [ 1.5 2.5 ]\n<DerivSum>  [ 3 4 ]\n<Count> 7 "
                 "</RectifiedLinearComponent> \n"
                 "</Components> </Nnet> ")
    import torch
    net = kctc.Nnet.read(p)
    assert net.num_components == 3
    assert net.info(0).startswith("FixedAffineComponent, input-dim=3, output-dim=2")
    v, d, n = net.get_component(1).nonlinear_stats()
    assert not v.any() and not d.any() and n == 0
    v, d, n = net.get_component(2).nonlinear_stats()
    assert v.tolist() == [1.5, 2.5] and d.tolist() == [3.0, 4.0] and n == 7
    x = torch.tensor([[1.0, 2.0, 3.0], [-1.0, 0.0, -4.0]], device=gpu)
    out = net.propagate(x, 2, 1).cpu().numpy()
    np.testing.assert_array_equal(out, np.maximum(np.array([[7.5, -1.5], [-8.5, 3.5]], np.float32), 0))
    net.close()


def test_average_models(kctc, gpu, lda_path, tmp_path):
    a, b = _net(kctc, lda_path, seed=5), _net(kctc, lda_path, seed=6)
    _train(a, gpu)
    _train(b, gpu, seed=1001)
    _train(b, gpu, seed=1002)
    fixed = _component_bytes(a, FIXED, tmp_path)
    pa = {c: a.get_params(c).astype(np.float64) for c in (HIDDEN, RNN)}
    pb = {c: b.get_params(c).astype(np.float64) for c in (HIDDEN, RNN)}
    sa, sb = a.get_component(RELU).nonlinear_stats(), b.get_component(RELU).nonlinear_stats()
    assert sa[2] == F.T * N and sb[2] == 2 * F.T * N
    kctc.average_models([a, b], weights=[0.25, 0.75])
    for c in (HIDDEN, RNN):
        e = rel_err(a.get_params(c), 0.25 * pa[c] + 0.75 * pb[c])
        print(f"component {c}: averaged parameters rel err {e:.2e}")
        assert e < 1e-6, (c, e)  # fp32 scale and axpy
    v, d, n = a.get_component(RELU).nonlinear_stats()
    np.testing.assert_allclose(v, 0.25 * sa[0] + 0.75 * sb[0], rtol=1e-14)  # fp64 on the device
    np.testing.assert_array_equal(d, 0.25 * sa[1] + 0.75 * sb[1])          # counts / 4: exact
    assert n == 0.25 * sa[2] + 0.75 * sb[2]
    assert _component_bytes(a, FIXED, tmp_path) == fixed
    # the pieces: scale and add leave FixedAffine alone and do not throw
    a.scale_params(2.0)
    a.add_params(-1.0, b)
    assert a.get_component(RELU).nonlinear_stats()[2] == 2 * n - sb[2]
    assert _component_bytes(a, FIXED, tmp_path) == fixed
    a.close()
    b.close()


def test_insert_keeps_the_front_end(kctc, gpu, lda_path, tmp_path):
    net = _net(kctc, lda_path)
    _train(net, gpu)
    twin = _net(kctc, lda_path)
    _train(twin, gpu)
    hidden = net.get_params(HIDDEN)
    C = net.num_components
    layer = kctc.recipe_config(num_rnn=1, input_dim=2 * F.H, hidden=F.H, num_targets=F.A,
                               learning_rate=F.LR).strip().split("\n")[1:3]
    net.insert(RNN + 2, "\n".join(layer) + "\n", seed=9)
    assert net.num_components == C + 2 and net.info(RNN + 2).startswith("CuDNNRecurrentComponent")
    _same_front_end(net, twin, tmp_path)
    np.testing.assert_array_equal(net.get_params(HIDDEN), hidden)
    _train(net, gpu, seed=1001)  # and it trains on
    assert net.get_component(RELU).nonlinear_stats()[2] == 2 * F.T * N
    net.close()
    twin.close()


def test_decodable_batch_equals_the_per_utterance_loop(kctc, gpu, lda_path):
    import torch
    net = kctc.Nnet(F.config(kctc, lda_path, THR) + f"SoftmaxComponent dim={F.A}\n", seed=5)
    rng = np.random.default_rng(4)
    feats = [torch.from_numpy(rng.standard_normal((t, F.D0)).astype(np.float32)).to(gpu) for t in F.LENS]
    batch = net.decodable_batch(feats, prob_scale=0.9, blank_threshold=1.0)
    for n, f in enumerate(feats):
        one = net.decodable(f, f.shape[0], prob_scale=0.9, blank_threshold=1.0)
        assert one.shape == batch[n].shape and one.shape[0] > 0
        e = rel_err(batch[n], one)
        print(f"utterance {n}: batch vs alone {e:.2e}")
        assert e < 1e-6, (n, e)
    net.close()
