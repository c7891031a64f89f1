"""Loop edges of the persistent recurrences (rec6_fwd.hip rnn_fwd_rec6 /
rec6_bwd.hip rnn_bwd_rec6) that the longer cases of test_rnn_gpu.py (T >= 9) never reach.

The step loops rotate the next step's operands (G row, dy / gates / cell
state) through registers behind the hand-off, and the self-tagged hand-off
goes through a ring of two step images whose tag is ((k >> 1) & 1):
  T = 1  no hand-off, no rotation: the loads before the loop feed the only step
  T = 2  one hand-off, one rotation and no load after it
  T = 3  both ring slots, one tag
  T = 5  every (slot, tag) pair of the two-image ring
N = 16 fills the 16-row group (two 8-row halves); N = 9 leaves the second
half with one live row.

Layer runs against the fp64 oracle under test_rnn_gpu.py's bars (norm-wise
relative error <= 1e-5 on y, <= 1e-4 on dx and dw; bf16: the error model of
sketch_common.bf16_tol), and XCD-pinned against unpinned training (where only
the way the bytes travel differs) bit for bit, as test_xcd_pin_gpu.py."""
import os

import numpy as np
import pytest

import sketch_common as S
from conftest import rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def _mk(kctc, gpu, mode, T, N, D, H, seed, wscale=0.15, prec=None):
    import torch
    rng = np.random.default_rng(seed)
    r = kctc.Rnn(mode, D, H, 1, True)
    if prec is not None:
        r.set_precision(prec)
    P = r.num_params
    w = (rng.standard_normal(P) * wscale).astype(np.float32)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    dy = rng.standard_normal((T, N, r.dirs * H)).astype(np.float32)
    ws_b, res_b = r.sizes(T, N)
    t = lambda a: torch.from_numpy(a).to(gpu)
    bufs = dict(w=t(w), x=t(x), dy=t(dy), y=torch.empty((T, N, r.dirs * H), device=gpu),
                dx=torch.empty((T, N, D), device=gpu), dw=torch.zeros(P, device=gpu),
                ws=torch.empty(ws_b, dtype=torch.uint8, device=gpu),
                res=torch.empty(res_b, dtype=torch.uint8, device=gpu))
    return r, (w, x, dy), bufs


def _run_gpu(r, b):
    import torch
    r.forward_training(b["x"], b["w"], b["y"], b["ws"], b["res"])
    r.backward_data(b["y"], b["dy"], b["w"], b["dx"], b["ws"], b["res"])
    r.backward_weights(b["x"], b["y"], b["dw"], b["ws"], b["res"])
    torch.cuda.synchronize()
    assert r.device_status() == 0
    return b["y"].cpu().numpy(), b["dx"].cpu().numpy(), b["dw"].cpu().numpy()


def _oracle(oracle, mode, w, x, dy, H, dirs):
    ry, res = oracle.rnn_forward(mode, x.astype(np.float64), w.astype(np.float64), H, 1, dirs)
    rdx, rdw = oracle.rnn_backward(mode, x.astype(np.float64), w.astype(np.float64), ry, dy.astype(np.float64),
                                   res, H, 1, dirs)
    return ry, rdx, rdw


SHORT = [(mode, T, N, 40, 512) for mode in (2, 3) for N in (16, 9) for T in (1, 2, 3, 5)]
SHORT.append((2, 4, 64, 40, 512))  # four row groups: U = 32 on 512-thread workgroups


@pytest.mark.parametrize("case", SHORT, ids=[f"m{c[0]}_T{c[1]}_N{c[2]}_H{c[4]}" for c in SHORT])
def test_short_matches_oracle(kctc, gpu, oracle, case):
    mode, T, N, D, H = case
    r, (w, x, dy), b = _mk(kctc, gpu, mode, T, N, D, H, seed=sum(case))
    y, dx, dw = _run_gpu(r, b)
    ry, rdx, rdw = _oracle(oracle, mode, w, x, dy, H, r.dirs)
    errs = {"y": rel_err(y, ry), "dx": rel_err(dx, rdx), "dw": rel_err(dw, rdw)}
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["y"] < 1e-5
    assert errs["dx"] < 1e-4
    assert errs["dw"] < 1e-4


def test_short_bf16_matches_oracle(kctc, gpu, oracle):
    """configs[4] width in bf16 (BGRU-1024, one row group), T = 4."""
    mode, T, N, D, H = 3, 4, 8, 40, 1024
    r, (w, x, dy), b = _mk(kctc, gpu, mode, T, N, D, H, seed=1078, wscale=0.05, prec="bf16")
    y, dx, dw = _run_gpu(r, b)
    ry, rdx, rdw = _oracle(oracle, mode, w, x, dy, H, r.dirs)
    errs = {"y": rel_err(y, ry), "dx": rel_err(dx, rdx), "dw": rel_err(dw, rdw)}
    print((mode, T, N, D, H), {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        assert e < S.bf16_tol(S.layer_stages(k, 1)), (k, e)


def _train(kctc, gpu, cfg, batch, env, steps=2):
    import torch
    feats, nf, fl, ll, T, N = batch
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        net = kctc.Nnet(cfg, seed=11)
        f = torch.from_numpy(feats).to(gpu)
        stats = [net.train_step(f, T, N, nf, fl, ll) for _ in range(steps)]
        params = [net.get_params(c) for c in range(net.num_components) if net.num_params(c)]
        net.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return stats, params


@pytest.mark.parametrize("var", ["KCTC_XCD6", "KCTC_XCD6F", "KCTC_XCD6F-stk"])
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("T", [3, 17])
def test_short_pinned_bit_identical(kctc, gpu, mode, T, var):
    """Two RNN components (both streamed GEMMs run beside the recurrences);
    one recurrence pinned against unpinned at a time, under the settings of
    test_xcd_pin_gpu.py that keep the GEMMs beside it the same in both runs
    (KCTC_XCD6F: the IO-wave forward feeding a streamed projection either way;
    KCTC_XCD6F-stk: the default stacked forward, projections after it).

    Toggling both pins at once with the default streams is not the comparison
    made there, and was not bit-identical (mode 2, T = 3: objf 220.98012161
    against 220.98012447); whether the round-6 tree does the same, and
    why, is open."""
    D, H, A, R, N = 40, 512, 41, 2, 16
    cfg = kctc.recipe_config(num_rnn=R, input_dim=D, hidden=H, num_targets=A, learning_rate=5e-4,
                             max_seq_length=T, rnn_mode=mode)
    feats, nf, fl, ll = kctc.synth_minibatch(7 + N, T, N, D, A, 0.125)
    batch = (feats, nf, fl, ll, T, N)
    env = {"KCTC_FWD_STREAM_PINNED": "1"}
    if var == "KCTC_XCD6F":
        env["KCTC_STK_FWD"] = "0"
    elif var == "KCTC_XCD6F-stk":
        env = {"KCTC_FWD_STREAM": "0"}
        var = "KCTC_XCD6F"
    a = _train(kctc, gpu, cfg, batch, dict(env, **{var: "0"}))
    b = _train(kctc, gpu, cfg, batch, dict(env, **{var: "1"}))
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
