"""DropoutComponent on the GPU (csrc/dropout.hip, csrc/components.cpp): the mask is
the documented one (kaldi_ctc_amd.dropout_mask, a numpy restatement of
csrc/dropout.h) bit for bit, forward and backward; its statistics; the
reference's file format; and the trainer with DropoutComponents between every
RNN and its ClipGradient -- the plumbing at low = high = 1 against the fp64
oracle, real masks against the component ABI and against finite differences,
and Nnet::RemoveDropout.

Gradient check (test_real_masks_gradient; central differences of compute_objf
along a random parameter direction against <get_grad, direction>, masks
frozen by reseeding; bar 0.05, nnet-component-test.cc:186-188): the measured
relative errors of the network with dropout and of the control without go to
dropout_gradcheck.txt beside the component checks' log
(test_component_gpu.LOG; measured: 9.2e-4 with dropout, 2.9e-3 for the
control)."""
import os
import struct

import numpy as np
import pytest

from conftest import rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SEEDS = [7, 0x123456789abcdef]  # the second: a non-zero high key word


def _line(D, P=None, S=None):
    return f"DropoutComponent dim={D}" + (f" dropout-proportion={P}" if P is not None else "") + \
        (f" dropout-scale={S}" if S is not None else "")


def _ones(gpu, rows, D):
    import torch
    return torch.ones((rows, D), dtype=torch.float32, device=gpu)


# ---- 1. exact mask -----------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("rows,D,P,S", [(5, 7, 0.5, 0.0),          # one block, a tail of 3
                                        (33, 1023, 0.2, 0.0),      # rows not a multiple of the vector
                                        (512, 1024, 0.2, 0.25)])   # many blocks, non-zero low scale
def test_mask_is_the_documented_one(kctc, gpu, seed, rows, D, P, S):
    c = kctc.Component(_line(D, P, S), seed=seed)
    assert c.Type() == "DropoutComponent" and not c.IsUpdatable()
    assert (c.BackpropNeedsInput(), c.BackpropNeedsOutput()) == (False, False)
    x = _ones(gpu, rows, D)
    for draw in range(3):
        got = c.Propagate(rows, 1, x).cpu().numpy()
        np.testing.assert_array_equal(got, kctc.dropout_mask(seed, 0, draw, rows, D, P, S), err_msg=f"draw {draw}")
    c.close()


def test_mask_scales_the_input_and_misaligned_views(kctc, gpu):
    """out = in * m for a general input; a view that is not 16-byte aligned
    takes the element-wise kernel and gets the same mask"""
    import torch
    rows, D, P, S, seed = 9, 13, 0.3, 0.5, 11
    m = kctc.dropout_mask(seed, 0, 0, rows, D, P, S)
    x = torch.randn((rows * D + 1,), dtype=torch.float32, device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    for off in (0, 1):
        c = kctc.Component(_line(D, P, S), seed=seed)
        xin = x[off:off + rows * D]
        out = torch.empty((rows * D + 1,), dtype=torch.float32, device=gpu)[off:off + rows * D]
        c.Propagate(rows, 1, xin, out)
        np.testing.assert_array_equal(out.cpu().numpy().reshape(rows, D), xin.cpu().numpy().reshape(rows, D) * m)
        c.close()


# ---- 2. prefix property --------------------------------------------------------
def test_mask_does_not_depend_on_the_launch_shape(kctc, gpu):
    D, P = 1023, 0.4
    a = kctc.Component(_line(D, P), seed=21)
    b = kctc.Component(_line(D, P), seed=21)
    three = a.Propagate(3, 1, _ones(gpu, 3, D)).cpu().numpy()
    eight = b.Propagate(8, 1, _ones(gpu, 8, D)).cpu().numpy()
    np.testing.assert_array_equal(three, eight[:3])
    assert 0 < (three == 0).sum() < three.size
    a.close()
    b.close()


# ---- 3. backward ---------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [(5, 7), (33, 1023)])
def test_backprop_regenerates_the_last_mask(kctc, gpu, rows, D):
    import torch
    P, S, seed = 0.35, 0.25, SEEDS[1]
    c = kctc.Component(_line(D, P, S), seed=seed)
    x = _ones(gpu, rows, D)
    c.Propagate(rows, 1, x)
    c.Propagate(rows, 1, x)  # the last draw is 1
    m = kctc.dropout_mask(seed, 0, 1, rows, D, P, S)
    od = torch.randn((rows, D), dtype=torch.float32, device=gpu, generator=torch.Generator(device=gpu).manual_seed(2))
    want = od.cpu().numpy() * m
    for _ in range(2):  # no Propagate in between: the same mask again
        got = c.Backprop(rows, 1, None, None, od, None, torch.empty_like(od))
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    alias = od.clone()
    c.Backprop(rows, 1, None, None, alias, None, alias)  # in_deriv aliases out_deriv
    np.testing.assert_array_equal(alias.cpu().numpy(), want)
    # a copy carries seed, stream and draw counter: it reproduces the last mask
    cp = c.Copy()
    np.testing.assert_array_equal(cp.Backprop(rows, 1, None, None, od, None, torch.empty_like(od)).cpu().numpy(), want)
    cp.close()
    c.close()


def test_backprop_before_propagate_is_an_error(kctc, gpu):
    import torch
    c = kctc.Component(_line(8, 0.5), seed=1)
    od = _ones(gpu, 2, 8)
    with pytest.raises(kctc.KctcError):
        c.Backprop(2, 1, None, None, od, None, torch.empty_like(od))
    c.close()


# ---- 4. statistics of the contract ----------------------------------------------
def mask_statistics(P, d0, d1, d_other_seed):
    """[(name, worst |count - n p| / sqrt(n p (1 - p)))] for dropped-element
    indicator matrices: draw 0, draw 1, and draw 0 of another seed."""
    out = []

    def z(name, count, n, p):
        count = np.asarray(count, dtype=np.float64)
        out.append((name, float(np.max(np.abs(count - n * p)) / np.sqrt(n * p * (1 - p)))))

    rows, dim = d0.shape
    n = rows * dim
    same = P * P + (1 - P) * (1 - P)
    z("dropped, whole matrix", d0.sum(), n, P)
    z("dropped, every row", d0.sum(axis=1), dim, P)
    z("dropped, every column", d0.sum(axis=0), rows, P)
    z("agreements, draw 0 vs draw 1", (d0 == d1).sum(), n, same)
    z("agreements, seed s vs s + 1", (d0 == d_other_seed).sum(), n, same)
    z("horizontal pairs both dropped", (d0[:, 1:] & d0[:, :-1]).sum(), rows * (dim - 1), P * P)
    z("vertical pairs both dropped", (d0[1:] & d0[:-1]).sum(), (rows - 1) * dim, P * P)
    return out


@pytest.mark.parametrize("P", [0.2, 0.5])
def test_mask_statistics(kctc, gpu, P):
    """each count within 6 binomial standard deviations of its expectation (the
    numpy restatement alone stays inside 4 for seeds 20161015, 7 and
    0x123456789abcdef: 6 is a condition, not a measurement)"""
    rows, D, s = 512, 1024, 20161015
    x = _ones(gpu, rows, D)
    a = kctc.Component(_line(D, P), seed=s)
    b = kctc.Component(_line(D, P), seed=s + 1)
    d0 = a.Propagate(rows, 1, x).cpu().numpy() == 0
    d1 = a.Propagate(rows, 1, x).cpu().numpy() == 0
    e0 = b.Propagate(rows, 1, x).cpu().numpy() == 0
    a.close()
    b.close()
    stats = mask_statistics(P, d0, d1, e0)
    for name, dev in stats:
        print(f"P={P} {name}: {dev:.2f} sigma")
    for name, dev in stats:
        assert dev <= 6.0, (name, dev)


# ---- 5. I/O -------------------------------------------------------------------
def tok(t):
    return t.encode() + b" "


def i32(v):
    return b"\x04" + struct.pack("<i", v)


def f32(v):
    return b"\x04" + struct.pack("<f", v)


def dropout_bytes(dim, proportion, scale):
    """nnet-component.cc:3540-3549, binary mode"""
    return (tok("<DropoutComponent>") + tok("<Dim>") + i32(dim) + tok("<DropoutScale>") + f32(scale) +
            tok("<DropoutProportion>") + f32(proportion) + tok("</DropoutComponent>"))


def test_component_io(kctc, gpu, tmp_path):
    c = kctc.Component(_line(1024, 0.2, 0.25), seed=3)
    info = c.Info()
    assert "dropout-proportion=0.2" in info and "dropout-scale=0.25" in info and "dim=1024" in info
    pb, pt = tmp_path / "d.bin", tmp_path / "d.txt"
    c.Write(pb, binary=True)
    c.Write(pt, binary=False)
    assert pb.read_bytes() == b"\0B" + dropout_bytes(1024, 0.2, 0.25)
    assert pt.read_bytes().split() == b"<DropoutComponent> <Dim> 1024 <DropoutScale> 0.25 <DropoutProportion> 0.2 " \
                                      b"</DropoutComponent>".split()
    for p in (pb, pt):
        r = kctc.Component.ReadNew(p)
        assert r.Type() == "DropoutComponent" and r.Info() == info
        r.close()
    d = kctc.Component(_line(6))
    assert "dropout-proportion=0.5" in d.Info() and "dropout-scale=0" in d.Info()  # the reference's defaults
    d.close()
    c.close()


@pytest.mark.parametrize("line", ["DropoutComponent dropout-proportion=0.2",              # no dim
                                  "DropoutComponent dim=0",
                                  "DropoutComponent dim=8 dropout-proportion=1",
                                  "DropoutComponent dim=8 dropout-proportion=-0.1",
                                  "DropoutComponent dim=8 dropout-scale=1.5",
                                  "DropoutComponent dim=8 dropout-rate=0.2"])             # unknown key
def test_bad_lines_are_refused(kctc, gpu, line):
    with pytest.raises(kctc.KctcError):
        kctc.Component(line)


def test_am_model_with_dropout_round_trips(kctc, gpu, tmp_path):
    """a whole nnet2-ctc model with DropoutComponents: loaded, written back byte-identical"""
    import test_model_io_gpu as M
    rng = np.random.default_rng(4)
    comps, params = M.build_model(rng)  # Splice, RNN, Clip, RNN, Clip, Affine
    comps = comps[:2] + [dropout_bytes(64, 0.2, 0.0)] + comps[2:4] + [dropout_bytes(64, 0.3, 0.5)] + comps[4:]
    priors = rng.random(9).astype(np.float32)
    blob = b"\0B" + M.TRANS + M.nnet(comps) + M.fvec(priors)
    src, out = tmp_path / "final.mdl", tmp_path / "out.mdl"
    src.write_bytes(blob)
    net = kctc.Nnet.read_am(src)
    assert net.num_components == 8
    assert "dropout-proportion=0.2" in net.info(2) and "dropout-scale=0.5" in net.info(5)
    np.testing.assert_array_equal(net.get_params(1), params[1])
    np.testing.assert_array_equal(net.get_params(4), params[3])
    net.write_am(out, binary=True)
    assert out.read_bytes() == blob
    # nnet-am-copy --remove-dropout=true: the file of the stripped model is the file without them
    assert net.remove_dropout() == 2
    net.write_am(out, binary=True)
    assert out.read_bytes() == b"\0B" + M.TRANS + M.nnet(M.build_model(np.random.default_rng(4))[0]) + M.fvec(priors)
    net.close()


# ---- 6. identity scale against the oracle ----------------------------------------
def _identity_dropout(cfg, P):
    """dropout-scale=1.0 on every generated DropoutComponent line: low = high = 1"""
    key = f"dropout-proportion={P}"
    assert key in cfg
    return cfg.replace(key, key + " dropout-scale=1.0")


@pytest.mark.parametrize("mode,H,pstd,stream_all", [(2, 64, 0.2, False), (3, 48, 0.2, False), (2, 256, 0.1, False),
                                                    (2, 64, 0.2, True)])
def test_identity_dropout_train_steps_match_oracle(kctc, gpu, oracle, monkeypatch, mode, H, pstd, stream_all):
    """the network of test_train_gpu.test_train_steps_match_oracle with a
    DropoutComponent (multiplier 1 everywhere) between every RNN and its
    ClipGradient: the unchained paths compute what the oracle computes, at that
    test's tolerances, and dropout draws nothing from the rand() stream"""
    import torch
    from test_train_gpu import _oracle_spec, glibc_rand_uniforms
    if stream_all:
        monkeypatch.setenv("KCTC_STREAM_ALL", "1")
    R, D, A, T, N, lr, thr, steps = 2, 24, 11, 30, 4, 0.02, 30.0, 2
    cfg = _identity_dropout(kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode,
                                               learning_rate=lr, clipping_threshold=thr, param_stddev=pstd,
                                               dropout_proportion=0.3), 0.3)
    net = kctc.Nnet(cfg, seed=5)
    assert net.num_components == 3 * R + 2
    assert [net.info(c).split(",")[0] for c in range(1, 4)] == ["CuDNNRecurrentComponent", "DropoutComponent",
                                                                 "ClipGradientComponent"]
    net.srand(99)
    draws = glibc_rand_uniforms(99, steps * R)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    assert len(upd) == R + 1
    params = [net.get_params(c).astype(np.float64) for c in upd]
    spec = _oracle_spec(oracle, R, mode, H, 2, D, A, thr, lr)
    cnc, cc = np.zeros(R), np.zeros(R)
    for step in range(steps):
        feats, nf, fl, ll = kctc.synth_minibatch(1000 + step, T, N, D, A, 0.2)
        objf, acc, wt = net.train_step(torch.from_numpy(feats).to(gpu), T, N, nf, fl, ll)
        d = draws[step * R:(step + 1) * R][::-1]  # the trainer draws top clip component first
        aff = params[-1]
        Wa, ba = aff[:-A].reshape(A, -1).copy(), aff[-A:].copy()
        robjf, racc, rwt = oracle.train_step(spec, params[:-1], Wa, ba, feats.reshape(T, N, D).astype(np.float64),
                                             nf, fl, ll, repair_draws=np.array(d, np.float32),
                                             clip_num_clipped=cnc, clip_count=cc)
        params[-1] = np.concatenate([Wa.ravel(), ba])
        np.testing.assert_allclose(objf, robjf, rtol=1e-5)
        assert wt == rwt
        ids = net.last_best_path(T, N)
        np.testing.assert_array_equal(ids, oracle.find_row_max_id(net.last_output(T, N, A)))
        assert acc == oracle.accuracy(ids, T, N, nf, fl, ll)[0]
        assert abs(acc - racc) <= 1  # vs fp64 logits: a near-tie may flip one frame
    assert net.rand_calls == steps * R  # one RandUniform() per ClipGradient Backprop, nothing for dropout
    for c, p in zip(upd, params):
        assert rel_err(net.get_params(c).astype(np.float64), p) < 1e-5, c
    net.close()


# ---- 7. bf16 fall-back ---------------------------------------------------------
def test_bf16_identity_dropout_matches_no_dropout(kctc, gpu):
    """bf16: the RNN above a DropoutComponent packs its own input instead of
    reading the packed rows of the RNN below, and projects it itself; equal to
    the chained network up to test_streamed_gemms_match_unstreamed's bf16 bars"""
    import torch
    mode, H, T, N, R, D, A, lr = 2, 512, 12, 16, 2, 40, 41, 0.02
    kw = dict(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode, learning_rate=lr, param_stddev=0.05)
    feats, nf, fl, ll = kctc.synth_minibatch(78, T, N, D, A, 0.2)
    f = torch.from_numpy(feats).to(gpu)
    res = []
    for cfg in (kctc.recipe_config(**kw), _identity_dropout(kctc.recipe_config(dropout_proportion=0.3, **kw), 0.3)):
        net = kctc.Nnet(cfg, seed=16)
        net.set_precision("bf16")
        upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
        before = [net.get_params(c) for c in upd]
        o = net.compute_objf(f, T, N, nf, fl, ll)[0]
        net.train_step(f, T, N, nf, fl, ll)
        o2 = net.compute_objf(f, T, N, nf, fl, ll)[0]
        res.append((o, o2, before, [net.get_params(c).astype(np.float64) for c in upd]))
        net.close()
    for a, b in zip(res[0][2], res[1][2]):
        np.testing.assert_array_equal(a, b)  # the same initial parameters
    tol = 1e-4
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=tol)
    np.testing.assert_allclose(res[1][1], res[0][1], rtol=tol)
    for a, b in zip(res[1][3], res[0][3]):
        assert rel_err(a, b) < tol / 2


# ---- 8 / 9 / 10: real masks ------------------------------------------------------
D8, H8, A8, T8, N8, P8 = 24, 64, 11, 30, 4, 0.3


def _dropout_net(kctc, seed=5, **kw):
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D8, hidden=H8, num_targets=A8, learning_rate=0.02,
                             param_stddev=0.2, dropout_proportion=P8, **kw)
    net = kctc.Nnet(cfg, seed=seed)
    assert net.num_components == 8
    return net


def test_real_masks_forward(kctc, gpu):
    """Splice -> BLSTM -> Dropout -> Clip -> BLSTM -> Dropout -> Clip -> Affine:
    the trainer's forward == the same chain run component by component with
    each dropout replaced by a multiply with the documented mask"""
    import torch
    net = _dropout_net(kctc)
    s = 0xfeedface12345
    feats = kctc.synth_minibatch(31, T8, N8, D8, A8, 0.2)[0]
    f = torch.from_numpy(feats).to(gpu)
    net.set_dropout_seed(s)
    first = net.propagate(f, T8, N8).cpu().numpy()
    x = f
    for c in range(net.num_components):
        if "DropoutComponent" in net.info(c):
            m = kctc.dropout_mask(s, c, 0, T8 * N8, 2 * H8, P8, 0.0)
            x = x * torch.from_numpy(m).to(gpu)
        else:
            comp = net.get_component(c)
            x = comp.Propagate(T8, N8, x.contiguous())
            comp.close()
    assert rel_err(first, x.cpu().numpy()) < 2e-6
    # a copy of a network's DropoutComponent reproduces the network's last mask
    comp = net.get_component(5)
    od = _ones(gpu, T8 * N8, 2 * H8)
    np.testing.assert_array_equal(comp.Backprop(T8, N8, None, None, od, None, torch.empty_like(od)).cpu().numpy(),
                                  kctc.dropout_mask(s, 5, 0, T8 * N8, 2 * H8, P8, 0.0))
    comp.close()
    second = net.propagate(f, T8, N8).cpu().numpy()  # draw 1
    assert rel_err(second, first) > 1e-3
    net.set_dropout_seed(s)
    np.testing.assert_array_equal(net.propagate(f, T8, N8).cpu().numpy(), first)
    net.close()


def _directional_check(kctc, net, f, mb, seed, rng):
    """relative errors (for sign +1, -1 of get_grad) of the central difference of
    compute_objf along a random parameter direction against <get_grad, direction>"""
    nf, fl, ll = mb
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    theta = [net.get_params(c) for c in upd]
    net.set_dropout_seed(seed)
    objf = net.train_step(f, T8, N8, nf, fl, ll)[0]
    grad = [net.get_grad(c).astype(np.float64) for c in upd]
    direction = [rng.standard_normal(t.size) for t in theta]
    slope = sum(float(g @ d) for g, d in zip(grad, direction))
    eps = 3e-3 * abs(objf) / (2 * abs(slope))  # predicted change: 3e-3 of the objective
    vals = []
    for sgn in (1.0, -1.0):
        for c, t, d in zip(upd, theta, direction):
            net.set_params(c, (t.astype(np.float64) + sgn * eps * d).astype(np.float32))
        net.set_dropout_seed(seed)
        vals.append(net.compute_objf(f, T8, N8, nf, fl, ll)[0])
    for c, t in zip(upd, theta):
        net.set_params(c, t)
    observed, predicted = vals[0] - vals[1], 2 * eps * slope
    assert 1e-3 * abs(objf) <= abs(predicted) <= 1e-2 * abs(objf)
    return [abs(observed - sg * predicted) / abs(predicted) for sg in (1.0, -1.0)], objf, observed, predicted


def test_real_masks_gradient(kctc, gpu):
    """d objf / d params through real masks: the backward's regenerated mask is
    the derivative of the forward.  The control (the same network after
    remove_dropout) fixes the sign convention of get_grad and shows that the
    method resolves 0.05 at this shape."""
    import torch
    net = _dropout_net(kctc, clipping_threshold=1e30)
    feats, nf, fl, ll = kctc.synth_minibatch(32, T8, N8, D8, A8, 0.2)
    f = torch.from_numpy(feats).to(gpu)
    seed = 424242
    errs, objf, obs, pred = _directional_check(kctc, net, f, (nf, fl, ll), seed, np.random.default_rng(9))
    assert net.remove_dropout() == 2
    cerrs, cobjf, cobs, cpred = _directional_check(kctc, net, f, (nf, fl, ll), seed, np.random.default_rng(9))
    net.close()
    sign = int(np.argmin(cerrs))
    text = (f"dropout gradient check (BLSTM-{H8} x 2, T={T8}, N={N8}, P={P8}): objf {objf:.6g} observed {obs:.6g} "
            f"predicted {pred:.6g} rel err {errs[sign]:.3e}; control without dropout: objf {cobjf:.6g} observed "
            f"{cobs:.6g} predicted {cpred:.6g} rel err {cerrs[sign]:.3e} (get_grad sign {'+' if sign == 0 else '-'})")
    print(text)
    from test_component_gpu import LOG as component_log  # the folder the component checks write to
    log = os.path.join(os.path.dirname(component_log), "dropout_gradcheck.txt")
    os.makedirs(os.path.dirname(log), exist_ok=True)
    with open(log, "a") as fh:
        fh.write(text + "\n")
    assert cerrs[sign] <= 0.05, cerrs
    assert errs[sign] <= 0.05, errs
    assert abs(cobjf - objf) > 1e-3 * abs(cobjf)  # the masks were not the identity


def test_remove_dropout(kctc, gpu, tmp_path):
    import torch
    net = _dropout_net(kctc, seed=6)
    feats, nf, fl, ll = kctc.synth_minibatch(33, T8, N8, D8, A8, 0.2)
    f = torch.from_numpy(feats).to(gpu)
    net.train_step(f, T8, N8, nf, fl, ll)
    with_dropout = net.compute_objf(f, T8, N8, nf, fl, ll)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    assert upd == [1, 4, 7]
    params = [net.get_params(c) for c in upd]
    assert net.remove_dropout() == 2
    assert net.num_components == 6
    assert [net.info(c).split(",")[0] for c in range(6)] == \
        ["SpliceComponent", "CuDNNRecurrentComponent", "ClipGradientComponent", "CuDNNRecurrentComponent",
         "ClipGradientComponent", "AffineComponent"]
    for c, p in zip((1, 3, 5), params):
        np.testing.assert_array_equal(net.get_params(c), p)
    fresh = kctc.Nnet(kctc.recipe_config(num_rnn=2, input_dim=D8, hidden=H8, num_targets=A8, learning_rate=0.02,
                                         param_stddev=0.2), seed=1)
    for c, p in zip((1, 3, 5), params):
        fresh.set_params(c, p)
    stripped = net.compute_objf(f, T8, N8, nf, fl, ll)
    assert stripped == fresh.compute_objf(f, T8, N8, nf, fl, ll)  # bit-identical: the chain is back
    assert stripped[0] != with_dropout[0]
    assert net.remove_dropout() == 0
    assert net.num_components == 6
    # the stripped model evaluates, decodes and trains on
    rng = np.random.default_rng(3)
    path = str(tmp_path / "valid.egs")
    with kctc.EgsWriter("ark:" + path) as w:
        for i in range(3):
            w.write(f"utt{i}", rng.standard_normal((25 + i, D8)).astype(np.float32),
                    rng.integers(1, A8, 4).astype(np.int32))
    got, want = net.compute_prob("ark:" + path), fresh.compute_prob("ark:" + path)
    assert got["num_examples"] == 3 and got == want
    utt = torch.from_numpy(rng.standard_normal((40, D8)).astype(np.float32)).to(gpu)
    np.testing.assert_array_equal(net.decodable(utt, 40), fresh.decodable(utt, 40))
    assert net.train_step(f, T8, N8, nf, fl, ll)[0] == stripped[0]
    net.close()
    fresh.close()


def test_set_dropout_scale(kctc, gpu):
    """Nnet::SetDropoutScale: scale 1 makes every multiplier 1"""
    import torch
    net = _dropout_net(kctc, seed=6)
    f = torch.from_numpy(kctc.synth_minibatch(34, T8, N8, D8, A8, 0.2)[0]).to(gpu)
    a = net.propagate(f, T8, N8).cpu().numpy()
    net.set_dropout_scale(1.0)
    assert "dropout-scale=1" in net.info(2)
    b = net.propagate(f, T8, N8).cpu().numpy()
    np.testing.assert_array_equal(net.propagate(f, T8, N8).cpu().numpy(), b)  # no draw matters any more
    assert rel_err(a, b) > 1e-3
    assert net.remove_dropout() == 2
    assert rel_err(net.propagate(f, T8, N8).cpu().numpy(), b) < 2e-6  # chained again: other GEMM order
    net.close()
    net2 = _dropout_net(kctc)
    with pytest.raises(kctc.KctcError):
        net2.set_dropout_scale(1.5)
    net2.close()
