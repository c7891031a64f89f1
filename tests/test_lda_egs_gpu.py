"""get_lda.sh inside the project, end to end (include/kaldi_lda.h:
kctc_lda_acc_egs, kctc_lda_estimate) on the shapes of
tests/test_nnet_align_gpu.py: a 2 x BLSTM-32 net to A = 11, feature dim 24,
utterances of 30 / 17 / 9 / 26 frames; context -2..2, so 120-dimensional rows.

egs archive -> Nnet.align_egs -> LdaStats.acc_egs under every blank policy ->
estimate -> lda.mat -> the --add-lda network.  The statistics are compared with
tests/lda_ref.py on the project reader's own feature values within the
rounding bound of tests/test_lda_stats_gpu.py.

82 frames in 120 dimensions: the within-class covariance W is singular, the
estimate takes the reference's smoothing retry, and "M W M^T = identity times
the within_class_factor scaling" holds for the smoothed W' = L L^T that was
factored.  That identity is checked on the estimate without the singular-value
ceiling (with W null directions M has singular values ~ 1 / sqrt(smooth), so
the default ceiling bites and reshapes M); the default estimate is the one
written to lda.mat, and the FixedAffineComponent's output on the spliced rows
must have the within-class covariance A W A^T that lda_ref gives for that
matrix A."""
import numpy as np
import pytest

import lda_ref

pytestmark = pytest.mark.gpu

R, D, H, A = 2, 24, 32, 11
LENS = [30, 17, 9, 26]
LEFT = [0, 2, 0, 0]                 # utt1 carries two rows of left context
CTX = (-2, -1, 0, 1, 2)
SD = D * len(CTX)


def _labels(rng, k):
    lab, prev = [], -1
    for _ in range(k):
        v = int(rng.integers(1, A))
        while v == prev:
            v = int(rng.integers(1, A))
        lab.append(v)
        prev = v
    return lab


def _write_int_ark(path, table):
    with open(path, "wb") as f:
        for key, v in table.items():
            v = np.asarray(v, np.int32)
            f.write(key.encode() + b" \0B\x04" + np.int32(len(v)).tobytes() + v.tobytes())


@pytest.fixture(scope="module")
def world(kctc, gpu, tmp_path_factory):
    """the archive, the alignment table and the numpy side's rows, made once"""
    tmp = tmp_path_factory.mktemp("lda")
    rng = np.random.default_rng(23)
    egs, ark = "ark:" + str(tmp / "train.egs"), "ark:" + str(tmp / "ali.ark")
    utts = {}
    with kctc.EgsWriter(egs) as w:
        for i, (t, lc) in enumerate(zip(LENS, LEFT)):
            feats = rng.standard_normal((t + lc, D)).astype(np.float32)
            lab = _labels(rng, max(1, t // 5))
            w.write(f"utt{i}", feats, np.array(lab, np.int32), left_context=lc)
            utts[f"utt{i}"] = (kctc.cm_decompress(kctc.cm_compress(feats)), lab, lc)
    net = kctc.Nnet(kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=2,
                                       learning_rate=0.02, param_stddev=0.2), seed=5)
    st = net.align_egs(egs, ark, minibatch_size=2)
    net.close()
    assert st["num_done"] == 4
    table = kctc.read_int_vector_ark(ark)
    assert [len(table[k]) for k in utts] == LENS
    # an untrained model's best path need not hold a single blank: a second table with the
    # labels thinned to spikes (two frames of three blank, utt0 ending in blanks) for the policies
    spiky = {k: np.where(np.arange(len(v)) % 3 == 1, v, 0).astype(np.int32) for k, v in table.items()}
    spiky["utt0"][-4:] = 0
    _write_int_ark(str(tmp / "spiky.ark"), spiky)
    return {"tmp": tmp, "egs": egs, "ark": ark, "utts": utts, "table": table,
            "spiky_ark": "ark:" + str(tmp / "spiky.ark"), "spiky": spiky}


def _numpy_rows(world, table, policy):
    xs, ids = [], []
    for key, (feats, _, lc) in world["utts"].items():
        if key not in table or lc + len(table[key]) > feats.shape[0]:
            continue
        L = len(table[key])
        xs.append(lda_ref.splice(feats, CTX)[lc:lc + L])
        ids.append(lda_ref.frame_classes(table[key], policy))
    return np.concatenate(xs).astype(np.float32), np.concatenate(ids).astype(np.int32)


def _check_stats(got, x, ids):
    rz, rf, rs = lda_ref.accumulate(x, ids, None, A)
    az, af, as_ = lda_ref.accumulate(np.abs(x), ids, None, A)
    eps = (len(ids) + 4) * 2.0 ** -53
    assert np.array_equal(got[0], rz)
    assert np.all(np.abs(got[1] - rf) <= eps * af)
    assert np.all(np.abs(got[2] - rs) <= eps * as_) and np.array_equal(got[2], got[2].T)


@pytest.mark.parametrize("which", ["ark", "spiky_ark"])
@pytest.mark.parametrize("policy", ["skip", "class", "fill"])
def test_acc_egs_matches_numpy(kctc, gpu, world, policy, which):
    table = world["table"] if which == "ark" else world["spiky"]
    h = kctc.LdaStats(SD, A)
    used, no_ali, mismatch, frames = h.acc_egs(world["egs"], world[which], context=CTX, blank_policy=policy)
    x, ids = _numpy_rows(world, table, policy)
    assert (used, no_ali, mismatch, frames) == (4, 0, 0, int(np.sum(ids >= 0)))
    zero = h.stats()[0]
    if policy != "skip":
        assert frames == sum(LENS)
    if policy != "class":
        assert zero[0] == 0
    if which == "spiky_ark":
        blanks = sum(int(np.sum(v == 0)) for v in table.values())
        assert blanks > sum(LENS) // 2
        assert frames == sum(LENS) - (blanks if policy == "skip" else 0)
        assert zero[0] == (blanks if policy == "class" else 0)
    _check_stats(h.stats(), x, ids)
    assert h.guards_intact()
    # the default policy is skip
    if policy == "skip":
        g = kctc.LdaStats(SD, A)
        assert g.acc_egs(world["egs"], world[which], context=CTX) == (used, no_ali, mismatch, frames)
        assert all(np.array_equal(p, q) for p, q in zip(g.stats(), h.stats()))
    h.close()


def test_acc_egs_in_several_batches(kctc, gpu, world):
    """the driver hands a batch to accumulate every 8192 spliced rows; with the
    threshold at 20 the four examples go in three batches (30 | 17 + 9 | 26), so
    the grow-only buffers are reused at smaller and larger sizes and the row
    offsets restart.  Same rows, other chunks: within the bound, counters equal."""
    one = kctc.LdaStats(SD, A)
    want = one.acc_egs(world["egs"], world["spiky_ark"], context=CTX, blank_policy="fill")
    before = kctc.LdaStats._test_batch_rows(20)
    try:
        assert before == 8192
        h = kctc.LdaStats(SD, A)
        assert h.acc_egs(world["egs"], world["spiky_ark"], context=CTX, blank_policy="fill") == want
        assert h.acc_egs(world["egs"], world["ark"], context=CTX, blank_policy="class") == (4, 0, 0, sum(LENS))
    finally:
        assert kctc.LdaStats._test_batch_rows(0) == 20
    x1, i1 = _numpy_rows(world, world["spiky"], "fill")
    x2, i2 = _numpy_rows(world, world["table"], "class")
    _check_stats(h.stats(), np.concatenate([x1, x2]), np.concatenate([i1, i2]))
    assert h.guards_intact()
    z1, z = one.stats()[0], h.stats()[0]
    assert z.sum() == 2 * sum(LENS) and np.all(z >= z1)
    one.close()
    h.close()


def test_acc_egs_counters(kctc, gpu, world):
    table = dict(world["table"])
    del table["utt2"]                                              # one key missing from the table
    table["utt3"] = np.concatenate([table["utt3"], [0, 0, 0]])     # one alignment too long
    table["utt0"] = table["utt0"].copy()
    table["utt0"][4] = -1                                          # a foreign table's "no class"
    ark = str(world["tmp"] / "edited.ark")
    _write_int_ark(ark, table)
    h = kctc.LdaStats(SD, A)
    used, no_ali, mismatch, frames = h.acc_egs(world["egs"], "ark:" + ark, context=CTX, blank_policy="class")
    x, ids = _numpy_rows(world, table, "class")
    assert (used, no_ali, mismatch) == (2, 1, 1)
    assert frames == LENS[0] + LENS[1] - 1 == int(np.sum(ids >= 0))
    _check_stats(h.stats(), x, ids)
    with pytest.raises(kctc.KctcError, match="multiple"):
        kctc.LdaStats(SD + 1, A).acc_egs(world["egs"], world["ark"], context=CTX)
    with pytest.raises(kctc.KctcError, match="feature dimension"):
        kctc.LdaStats(SD, A).acc_egs(world["egs"], world["ark"], context=(-1, 0, 1))
    with pytest.raises(kctc.KctcError, match="num_classes"):
        kctc.LdaStats(SD, 1).acc_egs(world["egs"], world["ark"], context=CTX, blank_policy="class")
    h.close()


def test_estimate_builds_the_lda_network(kctc, gpu, world):
    import torch
    h = kctc.LdaStats(SD, A)
    h.acc_egs(world["egs"], world["spiky_ark"], context=CTX, blank_policy="fill")
    x, ids = _numpy_rows(world, world["spiky"], "fill")
    zero, first, second = lda_ref.accumulate(x, ids, None, A)
    total, between, mean, _ = lda_ref.get_stats(zero, first, second)
    Lw, smoothed = lda_ref.within_cholesky(total, between)
    assert smoothed                                                # fewer frames than dimensions
    d = lda_ref.whitened_eig(total, between)[0]

    # identity times the within_class_factor scaling, for the covariance that was factored
    wcf = 0.001
    M0, chol = h.estimate(dim=40, within_class_factor=wcf, max_singular_value=0.0)
    np.testing.assert_allclose(chol, Lw, rtol=0, atol=1e-9 * np.abs(Lw).max())
    a0 = M0[:, :SD].astype(np.float64)
    got = a0 @ (Lw @ Lw.T) @ a0.T
    bound = 2.0 * 2.0 ** -24 * (np.abs(a0) @ np.abs(Lw @ Lw.T) @ np.abs(a0).T) + 1e-9
    assert np.all(np.abs(got - np.diag((wcf + d[:40]) / (1.0 + d[:40]))) <= bound)

    # the recipe's defaults -> lda.mat -> the --add-lda network
    M, _ = h.estimate(dim=40)
    assert M.shape == (40, SD + 1) and np.all(np.isfinite(M))
    assert np.linalg.svd(M[:, :SD].astype(np.float64), compute_uv=False).max() <= 5.0 * (1 + 1e-5)
    path = str(world["tmp"] / "lda.mat")
    kctc.write_kaldi_matrix(path, M)
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=2, learning_rate=0.02,
                             param_stddev=0.2, splice_context=CTX, lda_matrix=path, lda_dim=40)
    net = kctc.Nnet(cfg, seed=5)
    assert net.context == (2, 2)
    feats, lab, _ = world["utts"]["utt0"]
    T = feats.shape[0]
    rows = np.stack([feats[np.clip(np.arange(T) + s, 0, T - 1)] for s in CTX], axis=1).reshape(T * len(CTX), D)
    dev = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(gpu)
    objf, _, weight = net.train_step(dev, T, 1, [T], np.array(lab, np.int32), [len(lab)])
    assert np.isfinite(objf) and objf > 0 and weight == len(lab)
    net.close()

    # the FixedAffineComponent's output has the within-class covariance lda_ref gives for this matrix:
    # y = A x + b in fp32 is off by at most g = (SD + 2) 2^-24 times p = |A| |x| + |b| per element, and
    # every term of the covariance is a mean of products of two such values
    comp = kctc.Component(f"FixedAffineComponent matrix={path}")
    keep = ids >= 0
    xk = np.ascontiguousarray(x[keep])
    y = comp.Propagate(len(xk), 1, torch.from_numpy(xk).to(gpu)).cpu().numpy().astype(np.float64)
    yz, yf, ys = lda_ref.accumulate(y, ids[keep], None, A)
    ytotal, ybetween, _, _ = lda_ref.get_stats(yz, yf, ys)
    a = M[:, :SD].astype(np.float64)
    want = a @ (total - between) @ a.T
    p = np.abs(xk).astype(np.float64) @ np.abs(a).T + np.abs(M[:, SD].astype(np.float64))
    g = (SD + 2) * 2.0 ** -24
    q = np.sqrt(np.mean(p * p, axis=0))
    # 3 g per product of two outputs (g^2 included); each of the four second-order terms (mean of y y^T,
    # m m^T twice, the class means' sum) is at most q_i q_j in magnitude by Cauchy-Schwarz / Jensen
    bound = 4.0 * 3.0 * g * np.outer(q, q)
    assert np.all(np.abs((ytotal - ybetween) - want) <= bound)
    assert np.abs((ytotal - ybetween) - want).max() < np.abs(want).max()    # the bound is not vacuous
    h.close()
