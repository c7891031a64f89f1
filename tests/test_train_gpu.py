"""The nnet2 CTC train step (include/kaldi_ctc_train.h) end to end on the GPU
vs the fp64 oracle (oracle_train_step: NnetCtcUpdater::ComputeForMinibatch
with the in-place SGD of the reference) and the torch-fp64 cfg0 golden.

Tolerances: objective 1e-5 relative; parameter updates (lr * clipped grad)
1e-4 relative norm-wise per component (north_star: grads within 1e-4)."""
import ctypes

import numpy as np
import pytest

from conftest import golden, rel_err

pytestmark = pytest.mark.gpu

def glibc_rand_uniforms(seed, n):
    """RandUniform() = (float)((rand() + 1.0) / (RAND_MAX + 2.0))
    (src/base/kaldi-math.h:151-153) after srand(seed), drawn from the host's
    own glibc -- the generator the reference process calls."""
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    return [float(np.float32((libc.rand() + 1.0) / (2147483647 + 2.0))) for _ in range(n)]


def test_train_step_cfg0_golden(kctc, gpu):
    """configs[0]: 1 x uni-LSTM-256, N=2, T_max=200, D=40, A=41 vs torch fp64."""
    import torch
    g = golden("step_cfg0")
    cfg = kctc.recipe_config(num_rnn=1, input_dim=40, hidden=256, num_targets=41, bidirectional=False,
                             learning_rate=float(g["lr"]))
    net = kctc.Nnet(cfg, seed=1)
    assert net.num_components == 4
    net.set_params(1, g["w0"])
    net.set_params(3, np.concatenate([g["Wa0"].ravel(), g["ba0"]]))
    T, N = int(g["T"]), int(g["N"])
    feats = torch.from_numpy(g["feats"].reshape(T * N, -1)).to(gpu)
    objf, acc, wt = net.train_step(feats, T, N, g["num_frames"], g["flat_labels"], g["label_lengths"])
    np.testing.assert_allclose(objf, g["costs"].sum(), rtol=1e-5)
    assert wt == g["label_lengths"].sum()
    assert rel_err(net.get_params(1) - g["w0"], g["w_delta"]) < 1e-4
    aff = net.get_params(3)
    assert rel_err(aff[:-41] - g["Wa0"].ravel(), g["Wa_delta"].ravel()) < 1e-4
    assert rel_err(aff[-41:] - g["ba0"], g["ba_delta"]) < 1e-4


def _oracle_spec(oracle, R, mode, H, dirs, D, A, thr, lr, repair_scale=1.0):
    s = oracle.NnetSpec()
    s.num_rnn, s.mode, s.hidden, s.dirs, s.layers_per_rnn = R, mode, H, dirs, 1
    s.input_dim, s.num_targets = D, A
    s.clip_threshold, s.repair_threshold, s.repair_scale, s.repair_target = thr, 0.01, repair_scale, 0.0
    s.rnn_clip_gradient, s.lr_rnn, s.lr_affine = 5.0, lr, lr
    return s


@pytest.mark.parametrize("mode,H,thr,steps,pstd", [
    (2, 64, 30.0, 2, 0.2),     # BLSTM, recipe clip threshold (rarely clips)
    (2, 64, 0.02, 3, 0.2),     # every row clipped -> self-repair active on draws <= 0.5
    (3, 48, 30.0, 2, 0.2),     # BGRU
    # recipe widths: v6 recurrences + packed split-fp16 GEMMs (layer 2 input 512).
    # Weights at 0.2 * sqrt(64 / H) so the recurrence is not driven into the
    # saturated, rounding-amplifying regime (at 0.2 even the all-fp32 path
    # differs from fp64 by ~1e-4 after two updates)
    (2, 256, 30.0, 2, 0.1),    # BLSTM-256
    (3, 256, 30.0, 2, 0.1),    # BGRU-256
])
def test_train_steps_match_oracle(kctc, gpu, oracle, mode, H, thr, steps, pstd):
    import torch
    R, D, A, T, N, lr = 2, 24, 11, 30, 4, 0.02
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode,
                             learning_rate=lr, clipping_threshold=thr, param_stddev=pstd)
    net = kctc.Nnet(cfg, seed=5)
    net.srand(99)
    draws = glibc_rand_uniforms(99, steps * R)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    params = [net.get_params(c).astype(np.float64) for c in upd]
    spec = _oracle_spec(oracle, R, mode, H, 2, D, A, thr, lr)
    cnc, cc = np.zeros(R), np.zeros(R)
    for step in range(steps):
        feats, nf, fl, ll = kctc.synth_minibatch(1000 + step, T, N, D, A, 0.2)
        objf, acc, wt = net.train_step(torch.from_numpy(feats).to(gpu), T, N, nf, fl, ll)
        # the trainer draws top clip component first
        d = draws[step * R:(step + 1) * R][::-1]
        rnn_p = [p for p in params[:-1]]
        aff = params[-1]
        Wa = aff[:-A].reshape(A, -1).copy()
        ba = aff[-A:].copy()
        robjf, racc, rwt = oracle.train_step(spec, rnn_p, Wa, ba, feats.reshape(T, N, D).astype(np.float64),
                                             nf, fl, ll, repair_draws=np.array(d, np.float32),
                                             clip_num_clipped=cnc, clip_count=cc)
        params[-1] = np.concatenate([Wa.ravel(), ba])
        np.testing.assert_allclose(objf, robjf, rtol=1e-5)
        assert wt == rwt
        # best path: the trainer's ids are _find_row_max_id of its own output
        # (bit-exact), and ComputeTotAccuracy on them is the oracle's exactly
        logits = net.last_output(T, N, A)
        ids = net.last_best_path(T, N)
        np.testing.assert_array_equal(ids, oracle.find_row_max_id(logits))
        assert acc == oracle.accuracy(ids, T, N, nf, fl, ll)[0]
        assert abs(acc - racc) <= 1  # vs fp64 logits: a near-tie may flip one frame
    assert net.rand_calls == steps * R  # one RandUniform() per ClipGradient Backprop
    for c, p in zip(upd, params):
        got = net.get_params(c).astype(np.float64)
        init = None
        assert rel_err(got, p) < 1e-5, c
    for i, c in enumerate([c for c in range(net.num_components) if "ClipGradient" in net.info(c)]):
        ncl, cnt = net.clip_stats(c)
        assert cnt == cc[i] and ncl == cnc[i]


@pytest.mark.parametrize("mode,H,T,N", [(2, 256, 24, 40), (3, 512, 16, 64), (2, 512, 20, 33)])
def test_train_step_row_groups_match_oracle(kctc, gpu, oracle, mode, H, T, N):
    """N > 16: the v6 recurrences run one independent recurrence per group of
    16 sequences (bias partial sums per group added in order, dGates column
    maxima combined by atomicMax); the GEMMs are not streamed."""
    import torch
    R, D, A, lr = 2, 24, 11, 0.02
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode,
                             learning_rate=lr, param_stddev=0.1 * np.sqrt(64 / H))
    net = kctc.Nnet(cfg, seed=15)
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    params = [net.get_params(c).astype(np.float64) for c in upd]
    spec = _oracle_spec(oracle, R, mode, H, 2, D, A, 30.0, lr)
    feats, nf, fl, ll = kctc.synth_minibatch(77, T, N, D, A, 0.2)
    objf, acc, wt = net.train_step(torch.from_numpy(feats).to(gpu), T, N, nf, fl, ll)
    Wa = params[-1][:-A].reshape(A, -1).copy()
    ba = params[-1][-A:].copy()
    robjf, racc, rwt = oracle.train_step(spec, params[:-1], Wa, ba, feats.reshape(T, N, D).astype(np.float64),
                                         nf, fl, ll, repair_draws=np.ones(R, np.float32))
    params[-1] = np.concatenate([Wa.ravel(), ba])
    np.testing.assert_allclose(objf, robjf, rtol=1e-5)
    assert wt == rwt
    ids = net.last_best_path(T, N)
    np.testing.assert_array_equal(ids, oracle.find_row_max_id(net.last_output(T, N, A)))
    for c, p in zip(upd, params):
        assert rel_err(net.get_params(c).astype(np.float64), p) < 1e-5, c


@pytest.mark.parametrize("mode,H,T,N", [(3, 1024, 16, 32), (2, 512, 12, 16)])
def test_train_step_bf16_matches_oracle(kctc, gpu, oracle, mode, H, T, N):
    """kctc_nnet_set_precision(1): bf16 recurrences and gate GEMMs, fp32
    master weights, affine / CTC / updates in fp32 (configs[4]).  Tolerance
    for bf16 operands: objective 1e-3 relative (measured ~1e-4); every
    component's update at the error model's bound for its stages
    (sketch_common.bf16_tol / step_stages)."""
    import torch
    R, D, A, lr = 2, 40, 41, 0.02
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode,
                             learning_rate=lr, param_stddev=0.05)
    net = kctc.Nnet(cfg, seed=16)
    net.set_precision("bf16")
    upd = [c for c in range(net.num_components) if net.num_params(c) > 0]
    params = [net.get_params(c).astype(np.float64) for c in upd]
    p0 = [p.copy() for p in params]
    spec = _oracle_spec(oracle, R, mode, H, 2, D, A, 30.0, lr)
    feats, nf, fl, ll = kctc.synth_minibatch(78, T, N, D, A, 0.2)
    objf, acc, wt = net.train_step(torch.from_numpy(feats).to(gpu), T, N, nf, fl, ll)
    Wa = params[-1][:-A].reshape(A, -1).copy()
    ba = params[-1][-A:].copy()
    robjf, racc, rwt = oracle.train_step(spec, params[:-1], Wa, ba, feats.reshape(T, N, D).astype(np.float64),
                                         nf, fl, ll, repair_draws=np.ones(R, np.float32))
    params[-1] = np.concatenate([Wa.ravel(), ba])
    np.testing.assert_allclose(objf, robjf, rtol=1e-3)
    assert wt == rwt
    ids = net.last_best_path(T, N)
    np.testing.assert_array_equal(ids, oracle.find_row_max_id(net.last_output(T, N, A)))
    import sketch_common as S
    for k, (c, p, q) in enumerate(zip(upd, params, p0)):
        e = rel_err(net.get_params(c).astype(np.float64) - q, p - q)
        bound = S.bf16_tol(S.step_stages(R, "affine" if k == R else "grad", k))
        print(c, f"{e:.2e} (bound {bound:.2e})")
        assert e < bound, (c, e, bound)


def test_train_loss_decreases_and_objf_only(kctc, gpu):
    import torch
    D, A, T, N = 40, 41, 120, 8
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=128, num_targets=A, learning_rate=2e-3)
    net = kctc.Nnet(cfg, seed=3)
    feats, nf, fl, ll = kctc.synth_minibatch(7, T, N, D, A, 0.125)
    f = torch.from_numpy(feats).to(gpu)
    o0, _, w = net.compute_objf(f, T, N, nf, fl, ll)
    o0b, _, _ = net.compute_objf(f, T, N, nf, fl, ll)
    assert o0 == o0b  # no update, deterministic
    for _ in range(20):
        net.train_step(f, T, N, nf, fl, ll)
    o1, _, _ = net.compute_objf(f, T, N, nf, fl, ll)
    assert o1 < 0.93 * o0, (o0, o1)


def test_model_write_read_roundtrip(kctc, gpu, tmp_path):
    import torch
    D, A, T, N = 16, 9, 20, 3
    net = kctc.Nnet(kctc.recipe_config(num_rnn=2, input_dim=D, hidden=32, num_targets=A), seed=2)
    p = tmp_path / "m.bin"
    net.write(p, binary=True)
    net2 = kctc.Nnet.read(p)
    assert net2.num_components == net.num_components
    for c in range(net.num_components):
        if net.num_params(c):
            np.testing.assert_array_equal(net.get_params(c), net2.get_params(c))
    feats, nf, fl, ll = kctc.synth_minibatch(3, T, N, D, A, 0.2)
    f = torch.from_numpy(feats).to(gpu)
    assert net.compute_objf(f, T, N, nf, fl, ll) == net2.compute_objf(f, T, N, nf, fl, ll)


@pytest.mark.parametrize("knob", ["KCTC_FWD_STREAM", "KCTC_BWD_STREAM"])
@pytest.mark.parametrize("mode,H,T,N,prec", [(2, 512, 300, 16, 0), (2, 256, 97, 5, 0), (3, 256, 64, 16, 0),
                                             # row groups (N > 16: ragged last group), bf16 images / operands
                                             (2, 256, 64, 40, 0), (3, 256, 50, 32, 0), (3, 256, 64, 16, 1),
                                             (2, 256, 48, 24, 1)])
def test_streamed_gemms_match_unstreamed(kctc, gpu, monkeypatch, knob, mode, H, T, N, prec):
    """GEMMs that run while the recurrence producing their rows is still going
    (knob=1, the default) against the same GEMMs after it (knob=0):
    KCTC_FWD_STREAM -- RNN -> ClipGradient -> RNN, the second RNN's input
    projection read off the first one's exchange images (h * 2^14 as fp16
    hi/lo; the packed copy carries h * 2^13); KCTC_BWD_STREAM -- dx of an RNN
    from its backward recurrence's dGates rows as they are flagged (per-
    direction partials added in a fixed order instead of beta-accumulated).
    Equal up to fp32 rounding; many row tiles, ragged N, LSTM and GRU."""
    import torch
    D, A = 40, 41
    cfg = kctc.recipe_config(num_rnn=3, input_dim=D, hidden=H, num_targets=A, rnn_mode=mode,
                             learning_rate=1e-3, param_stddev=0.05)
    feats, nf, fl, ll = kctc.synth_minibatch(17, T, N, D, A, 0.125)
    f = torch.from_numpy(feats).to(gpu)
    res = {}
    if N > 16 or prec:  # the general streaming path (off by default on these shapes)
        monkeypatch.setenv("KCTC_STREAM_ALL", "1")
    for flag in ("0", "1"):
        monkeypatch.setenv(knob, flag)
        net = kctc.Nnet(cfg, seed=8)
        if prec:
            net.set_precision("bf16")
        o = net.compute_objf(f, T, N, nf, fl, ll)[0]
        net.train_step(f, T, N, nf, fl, ll)
        o2 = net.compute_objf(f, T, N, nf, fl, ll)[0]
        res[flag] = (o, o2, [net.get_params(c).astype(np.float64) for c in range(net.num_components)
                             if net.num_params(c) > 0])
    # bf16: the same bf16 operands either way (h rounded once), fp32 sums in
    # another order (the direction-split projection adds two half-K partials);
    # a last-bit difference in a gate pre-activation can flip the bf16
    # rounding of an h, which the bf16 recurrence carries on (measured 2.5e-5
    # on the objective after a step; the bf16 path is held to the fp64
    # oracle in test_train_step_bf16_matches_oracle)
    tol = 1e-4 if prec else 2e-6
    np.testing.assert_allclose(res["1"][0], res["0"][0], rtol=tol)
    np.testing.assert_allclose(res["1"][1], res["0"][1], rtol=tol)
    for a, b in zip(res["1"][2], res["0"][2]):
        assert rel_err(a, b) < tol / 2


@pytest.mark.parametrize("knob", ["KCTC_FWD_STREAM", "KCTC_BWD_STREAM"])
@pytest.mark.parametrize("mode,H,T,N", [(2, 512, 300, 16), (3, 256, 64, 13)])
def test_streamed_gemms_group8(kctc, gpu, monkeypatch, knob, mode, H, T, N):
    """KCTC_REC_GS=8: the streamed GEMMs read two row groups' images / flags
    (readiness = the slower group) and equal the GEMMs run after the recurrence."""
    monkeypatch.setenv("KCTC_REC_GS", "8")
    test_streamed_gemms_match_unstreamed(kctc, gpu, monkeypatch, knob, mode, H, T, N, 0)


@pytest.mark.parametrize("mode,H,T,N", [(2, 512, 300, 16), (3, 256, 50, 32)])
def test_streamed_projection_whole_k(kctc, gpu, monkeypatch, mode, H, T, N):
    """KCTC_STREAM_DIRSPLIT=0: the streamed projection's tiles take the whole K
    (both producer directions) once a row tile is complete, instead of two
    half-K jobs per tile meeting in C."""
    monkeypatch.setenv("KCTC_STREAM_DIRSPLIT", "0")
    test_streamed_gemms_match_unstreamed(kctc, gpu, monkeypatch, "KCTC_FWD_STREAM", mode, H, T, N, 0)


@pytest.mark.parametrize("mode,H,T,N", [(2, 512, 20, 16), (3, 256, 24, 11)])
def test_train_step_group8_matches_oracle(kctc, gpu, oracle, monkeypatch, mode, H, T, N):
    """A whole train step with the recurrences in row groups of 8 sequences."""
    monkeypatch.setenv("KCTC_REC_GS", "8")
    test_train_step_row_groups_match_oracle(kctc, gpu, oracle, mode, H, T, N)


@pytest.mark.parametrize("H,T,N,chunks", [(512, 64, 16, 4), (256, 50, 7, 3), (256, 33, 12, 8)])
def test_wgrad_stream_matches_whole(kctc, gpu, monkeypatch, H, T, N, chunks):
    """The bottom component's weight gradients streamed off its running
    backward recurrence (frame chunks gated on its flags, KCTC_WGRAD_STREAM=1,
    the default) against the whole-sequence weight GEMMs after it (=0):
    equal up to fp32 rounding of the chunked sums."""
    import torch
    D, A = 40, 41
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=H, num_targets=A, rnn_mode=2,
                             learning_rate=1e-3, param_stddev=0.05)
    feats, nf, fl, ll = kctc.synth_minibatch(19, T, N, D, A, 0.125)
    f = torch.from_numpy(feats).to(gpu)
    monkeypatch.setenv("KCTC_WGRAD_CHUNKS", str(chunks))
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("KCTC_WGRAD_STREAM", flag)
        net = kctc.Nnet(cfg, seed=9)
        for _ in range(2):
            net.train_step(f, T, N, nf, fl, ll)
        res[flag] = (net.compute_objf(f, T, N, nf, fl, ll)[0],
                     [net.get_params(c).astype(np.float64) for c in range(net.num_components) if net.num_params(c) > 0])
    np.testing.assert_allclose(res["1"][0], res["0"][0], rtol=2e-6)
    for a, b in zip(res["1"][1], res["0"][1]):
        assert rel_err(a, b) < 1e-6


def test_bottom_wgrad_two_streams_bit_identical(kctc, gpu, monkeypatch):
    """The bottom component's weight GEMMs with dW beside dR on a second stream
    (KCTC_WGRAD_2S=1, the default) equal the one-stream order bit for bit:
    separate split slabs and tile counters, the same kernels and sums."""
    import torch
    D, A, T, N, H = 40, 41, 40, 16, 512
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=H, num_targets=A, learning_rate=1e-3,
                             param_stddev=0.05)
    feats, nf, fl, ll = kctc.synth_minibatch(29, T, N, D, A, 0.125)
    f = torch.from_numpy(feats).to(gpu)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("KCTC_WGRAD_2S", flag)
        net = kctc.Nnet(cfg, seed=12)
        for _ in range(2):
            net.train_step(f, T, N, nf, fl, ll)
        res[flag] = [net.get_params(c) for c in range(net.num_components) if net.num_params(c) > 0]
        net.close()
    for a, b in zip(res["0"], res["1"]):
        np.testing.assert_array_equal(a, b)


def test_rccl_dp_single_rank_matches_plain(kctc, gpu):
    """kctc_nnet_enable_dp at world size 1 builds the RCCL exchange
    (ncclCommInitRank on a one-rank communicator): every component's bucket is
    ncclAllReduce'd on the comm stream (forked after the side-stream weight
    GEMMs, joined before the updates) beside the streamed GEMMs and
    recurrences; a sum over one rank is the identity, so the updates equal
    the plain trainer's bit for bit."""
    import torch
    D, A, T, N, H = 40, 41, 64, 16, 256
    cfg = kctc.recipe_config(num_rnn=3, input_dim=D, hidden=H, num_targets=A, learning_rate=1e-3,
                             param_stddev=0.05)
    feats, nf, fl, ll = kctc.synth_minibatch(23, T, N, D, A, 0.125)
    f = torch.from_numpy(feats).to(gpu)
    nets = [kctc.Nnet(cfg, seed=4), kctc.Nnet(cfg, seed=4)]
    nets[1].enable_dp(kctc.dp_unique_id(), 0, 1)
    outs = [[net.train_step(f, T, N, nf, fl, ll) for _ in range(2)] for net in nets]
    assert outs[0] == outs[1]
    for c in range(nets[0].num_components):
        if nets[0].num_params(c):
            np.testing.assert_array_equal(nets[0].get_params(c), nets[1].get_params(c))


def test_rccl_model_averaging_single_rank(kctc, gpu):
    """Model-averaging mode over the RCCL communicator at world size 1: no
    gradient exchange during the steps, and averaging one model is the
    identity -- the parameters equal a plain trainer's bit for bit."""
    import torch
    D, A, T, N, H = 40, 41, 32, 4, 256
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=H, num_targets=A, learning_rate=1e-3,
                             param_stddev=0.05)
    feats, nf, fl, ll = kctc.synth_minibatch(23, T, N, D, A, 0.125)
    f = torch.from_numpy(feats).to(gpu)
    nets = [kctc.Nnet(cfg, seed=4), kctc.Nnet(cfg, seed=4)]
    nets[1].set_dp_mode("average")
    nets[1].enable_dp(kctc.dp_unique_id(), 0, 1)
    for net in nets:
        for _ in range(2):
            net.train_step(f, T, N, nf, fl, ll)
    nets[1].average_params()
    for c in range(nets[0].num_components):
        if nets[0].num_params(c):
            np.testing.assert_array_equal(nets[0].get_params(c), nets[1].get_params(c))
    for net in nets:
        net.close()


def test_async_steps_equal_sync_steps(kctc, gpu):
    """kctc_nnet_train_step_async / train_flush: the same updates and the same
    per-minibatch stats as kctc_nnet_train_step, reported one step late."""
    import torch
    D, A, T, N, H = 40, 41, 50, 4, 256
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=H, num_targets=A, learning_rate=1e-3,
                             param_stddev=0.05)
    batches = []
    for k in range(4):
        feats, nf, fl, ll = kctc.synth_minibatch(100 + k, T, N, D, A, 0.125)
        batches.append((torch.from_numpy(feats).to(gpu), nf, fl, ll))
    a, b = kctc.Nnet(cfg, seed=6), kctc.Nnet(cfg, seed=6)
    sync = [a.train_step(f, T, N, nf, fl, ll) for f, nf, fl, ll in batches]
    got = []
    for f, nf, fl, ll in batches:
        r = b.train_step_async(f, T, N, nf, fl, ll)
        if r is not None:
            got.append(r)
    assert len(got) == len(batches) - 1  # one queued ahead
    got += b.train_flush()
    assert got == sync
    assert b.train_flush() == []
    for c in range(a.num_components):
        if a.num_params(c):
            np.testing.assert_array_equal(a.get_params(c), b.get_params(c))


def test_multistep_trajectory_matches_oracle(kctc, gpu, oracle):
    """bench.py's objf-per-label trajectory swings by 10-100x from step to
    step (16.7 -> 1111 -> 336 -> ... at configs[1]).  That is the reference's
    own SGD on the synthetic data: the minibatch gradient is a SUM over all
    frames (6,400 here, 30,000 at configs[1]) at lr 5e-4, the affine update is
    not clipped, so the first steps over-shoot.  The fp64 oracle (the same
    recipe init, lr, clipping and self-repair semantics) follows the same
    trajectory: here 20.9 -> 48.7 -> 37.8 -> 9.2 per label, and the GPU
    matches it step by step."""
    import torch
    R, H, T, N, D, A, lr, steps = 2, 64, 400, 16, 40, 41, 5e-4, 4
    import sketch_common as S
    rnn = [S.recipe_rnn_params(oracle, 2, D if c == 0 else 2 * H, H, 77 + c) for c in range(R)]
    rng = np.random.default_rng([77, 9])
    Wa = (rng.standard_normal((A, 2 * H)) / np.sqrt(2 * H)).astype(np.float32)
    ba = rng.standard_normal(A).astype(np.float32)
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, learning_rate=lr)
    net = kctc.Nnet(cfg, seed=1)
    for c in range(R):
        net.set_params(1 + 2 * c, rnn[c])
    net.set_params(2 * R + 1, np.concatenate([Wa.ravel(), ba]))
    net.srand(0)
    spec = _oracle_spec(oracle, R, 2, H, 2, D, A, 30.0, lr)
    rp = [p.astype(np.float64) for p in rnn]
    Wd, bd = Wa.astype(np.float64), ba.astype(np.float64)
    cnc, cc = np.zeros(R), np.zeros(R)
    draws = glibc_rand_uniforms(0, steps * R)
    got, ref = [], []
    for step in range(steps):
        feats, nf, fl, ll = kctc.synth_minibatch(20161015 + step, T, N, D, A, 0.125)
        o, _, w = net.train_step(torch.from_numpy(feats).to(gpu), T, N, nf, fl, ll)
        d = np.array(draws[step * R:(step + 1) * R][::-1], np.float32)  # top clip component draws first
        ro, _, rw = oracle.train_step(spec, rp, Wd, bd, feats.reshape(T, N, D).astype(np.float64), nf, fl, ll,
                                      repair_draws=d, clip_num_clipped=cnc, clip_count=cc)
        assert w == rw
        got.append(o / w)
        ref.append(ro / rw)
    print("gpu", [round(x, 4) for x in got], "oracle fp64", [round(x, 4) for x in ref])
    np.testing.assert_allclose(got, ref, rtol=1e-4)
    assert max(ref) > 2 * ref[0]  # the over-shooting first steps


def test_two_nets_interleaved_on_one_device(kctc, gpu):
    """Two trainers on one device, their steps interleaved (A B A B), each
    bit-identical to its own run alone.  The streamed GEMMs and packs beside
    a recurrence wait on that launch's own residency count (rec_gate.hip
    beside_recurrence), so one net's launches never hold up the other's side
    streams (the round-5 gate waited on a device-wide registration count
    that every net's backward raised)."""
    import torch
    T, N, D, A, H = 300, 16, 40, 41, 512
    cfg = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=H, num_targets=A, learning_rate=1e-3)
    batches = []
    for s in range(4):
        feats, nf, fl, ll = kctc.synth_minibatch(40 + s, T, N, D, A, 0.125)
        batches.append((torch.from_numpy(feats).to(gpu), nf, fl, ll))

    def params(net):
        return [net.get_params(c) for c in range(net.num_components) if net.num_params(c) > 0]

    alone = []
    for seed, idx in ((3, (0, 1)), (4, (2, 3))):
        net = kctc.Nnet(cfg, seed=seed)
        for i in idx:
            f, nf, fl, ll = batches[i]
            net.train_step(f, T, N, nf, fl, ll)
        alone.append(params(net))
        net.close()
    a, b = kctc.Nnet(cfg, seed=3), kctc.Nnet(cfg, seed=4)
    for ia, ib in ((0, 2), (1, 3)):
        for net, i in ((a, ia), (b, ib)):
            f, nf, fl, ll = batches[i]
            net.train_step(f, T, N, nf, fl, ll)
    for net, ref in ((a, alone[0]), (b, alone[1])):
        for p, r in zip(params(net), ref):
            np.testing.assert_array_equal(p, r)
    a.close()
    b.close()
