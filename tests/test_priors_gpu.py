"""The average-posterior prior stage of steps/ctc/train.sh:469-510 --
nnet-ctc-compute-from-egs | matrix-sum-rows | vector-sum (Nnet.sum_posteriors)
and nnet-adjust-priors (Nnet.adjust_priors) -- against the fp64 oracle run on
every example alone."""
import numpy as np
import pytest

import test_decode_batch_gpu as B

pytestmark = pytest.mark.gpu

D, A, H = B.D, B.A, 64


@pytest.fixture(scope="module")
def archive(oracle, tmp_path_factory):
    """23 examples, T in 20..90, one written with left_context = 2; the
    oracle's summed softmax outputs over the frames the tool uses."""
    import conftest
    kctc = conftest.load_kctc()
    rng = np.random.default_rng(17)
    path = str(tmp_path_factory.mktemp("priors") / "train.egs")
    params = B._params(oracle, H, 41)
    tot, frames = np.zeros(A), 0
    with kctc.EgsWriter("ark:" + path) as w:
        for i in range(23):
            T = int(rng.integers(20, 91))
            lc = 2 if i == 9 else 0
            feats = rng.standard_normal((T, D)).astype(np.float32)
            w.write(f"utt{i:03d}", feats, rng.integers(1, A, 3).astype(np.int32), left_context=lc)
            # the network has no context of its own: the first left_context rows are dropped
            used = oracle.cm_decompress(oracle.cm_compress(feats))[lc:]
            tot += B._oracle_probs(oracle, params, used, H).astype(np.float64).sum(0)
            frames += used.shape[0]
    return dict(path="ark:" + path, params=params, sum=tot, frames=frames)


def _net(kctc, params):
    net = kctc.Nnet(B._cfg(kctc, H), seed=1)
    for c, p in zip((1, 3, 5), params):
        net.set_params(c, p)
    return net


def test_sum_posteriors_matches_oracle(kctc, gpu, archive):
    net = _net(kctc, archive["params"])
    s, frames, num_egs = net.sum_posteriors(archive["path"], minibatch_size=8)
    assert num_egs == 23
    assert frames == archive["frames"]
    print("max rel diff", np.max(np.abs(s - archive["sum"]) / archive["sum"]))
    np.testing.assert_allclose(s, archive["sum"], rtol=1e-4)
    np.testing.assert_allclose(s.sum(), frames, rtol=1e-5)  # posteriors: one per frame
    # the batching does not matter beyond rounding, and a rerun is bit-identical
    s1, f1, _ = net.sum_posteriors(archive["path"], minibatch_size=1)
    assert f1 == frames
    np.testing.assert_allclose(s1, s, rtol=1e-5)
    s2, _, _ = net.sum_posteriors(archive["path"], minibatch_size=8)
    np.testing.assert_array_equal(s2, s)
    net.close()


def test_adjust_priors_both_forms(kctc, gpu, archive, tmp_path):
    net = _net(kctc, archive["params"])
    s, _, _ = net.sum_posteriors(archive["path"], minibatch_size=8)
    net.adjust_priors(s)
    tot = 0.0
    for v in s:
        tot += float(v)
    want = (s / tot).astype(np.float32)
    np.testing.assert_array_equal(net.priors, want)
    np.testing.assert_allclose(net.priors.sum(), 1.0, rtol=1e-6)
    p1, p2 = tmp_path / "a.mdl", tmp_path / "b.mdl"
    net.write_am(p1, binary=True)
    n2 = kctc.Nnet.read_am(p1)
    np.testing.assert_array_equal(n2.priors, want)
    n2.write_am(p2, binary=True)
    assert p1.read_bytes() == p2.read_bytes()
    n2.close()
    # --google-prior-const: all ones, the blank's prior the constant, not normalised
    net.adjust_priors(google_prior_const=3.0)
    g = np.ones(A, np.float32)
    g[0] = 3.0
    np.testing.assert_array_equal(net.priors, g)
    net.write_am(p1, binary=True)
    n3 = kctc.Nnet.read_am(p1)
    np.testing.assert_array_equal(n3.priors, g)
    n3.write_am(p2, binary=True)
    assert p1.read_bytes() == p2.read_bytes()
    n3.close()
    with pytest.raises(kctc.KctcError):
        net.adjust_priors(np.zeros(A))
    np.testing.assert_array_equal(net.priors, g)  # unchanged by the refused call
    with pytest.raises(kctc.KctcError):
        net.adjust_priors(np.ones(A + 1))
    net.close()
