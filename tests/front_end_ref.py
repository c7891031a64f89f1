"""The recipe's FT / LDA front end restated in numpy fp64 and composed with the
oracle's RNN and CTC (TEST INFRASTRUCTURE), and the network and minibatch the
front-end tests share.

Network (the shape family of tests/test_train_seq_gpu.py):
  Splice(-1,0,1) on 13-dim input -> FixedAffine 39 -> 20 -> Affine 20 -> 48
  (bias-stddev=0) -> RectifiedLinear -> ClipGradient -> BLSTM-64 -> ClipGradient
  -> Affine -> A = 11;  T = 30, N = 4, lengths 30 / 17 / 9 / 26.  The bf16 test
uses BLSTM-256 (`hidden`): the smallest width the bf16 recurrences exist for.
"front only": no Splice context, no FixedAffine (Affine 13 -> 48 first); `hdim`
sets another hidden_dim (the recipe's 1024).

chain_step() is one default (padded) minibatch: every component of the
reference's Backprop walk in fp64 -- numpy for Splice, FixedAffine, Affine and
ReLU, tests/clip_ref.py for the two ClipGradients (self-repair off),
oracle.rnn_forward / rnn_backward / ctc for the rest.  Gradients are the
trainer's: of minus the CTC cost, so that params += lr * grad."""
import numpy as np

import clip_ref

D0, CTX, DL, DH, H, A, T = 13, (-1, 0, 1), 20, 48, 64, 11, 30
LENS = [30, 17, 9, 26]
LR = 0.02
TOP_THRESHOLD = 30.0


def lda_matrix(seed=3):
    """[DL, 39 + 1] float32: the last column is the bias"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((DL, D0 * len(CTX) + 1)) / np.sqrt(D0 * len(CTX))
    m[:, -1] = 0.1 * rng.standard_normal(DL)
    return m.astype(np.float32)


def config(kctc, lda_path, front_threshold, front_only=False, hidden=H, hdim=DH, param_stddev=None):
    """The network's config text.  self-repair-scale=0 on both ClipGradient
    lines keeps the repair draw out (covered by the ClipGradient tests)."""
    # the same recurrent gain param_stddev * sqrt(H) = 1.6 at every width (0.1 at H = 256, as the
    # H = 256 case of tests/test_train_seq_gpu.py)
    cfg = kctc.recipe_config(num_rnn=1, input_dim=D0, hidden=hidden, num_targets=A, learning_rate=LR,
                             param_stddev=param_stddev or 0.2 * np.sqrt(H / hidden),
                             clipping_threshold=TOP_THRESHOLD, splice_context=(0,) if front_only else CTX,
                             model_type="FT", hidden_dim=hdim, lda_matrix=None if front_only else lda_path,
                             lda_dim=None if front_only else DL)
    lines = cfg.strip().split("\n")
    out, seen_clip = [], 0
    for line in lines:
        if line.startswith("ClipGradientComponent"):
            if seen_clip == 0:  # the front one: its own threshold, spelled exactly
                line = line.replace(f"clipping-threshold={TOP_THRESHOLD}", f"clipping-threshold={front_threshold!r}")
            seen_clip += 1
            line = line.replace("norm-based-clipping=", "self-repair-scale=0 norm-based-clipping=")
        out.append(line)
    assert seen_clip == 2
    return "\n".join(out) + "\n"


def minibatch(lens=LENS, seed=1000, d=D0, ctx=CTX):
    """Per-utterance frames xs[n] [len + L + R, d] float32, labels, flat labels, label lengths"""
    rng = np.random.default_rng(seed)
    L, R = -ctx[0], ctx[-1]
    xs = [rng.standard_normal((t + L + R, d)).astype(np.float32) for t in lens]
    labels = []
    for t in lens:
        k = min(max(1, int(0.2 * t)), (t - 1) // 2)
        lab, prev = [], -1
        for _ in range(k):
            v = int(rng.integers(1, A))
            while v == prev:
                v = int(rng.integers(1, A))
            lab.append(v)
            prev = v
        labels.append(lab)
    fl = np.array([v for lab in labels for v in lab], np.int32)
    ll = np.array([len(lab) for lab in labels], np.int32)
    return xs, labels, fl, ll


def format_input(xs, lens, Tmax, ctx=CTX, pad=0.0):
    """FormatNnetInput layout [Tmax * N * ns, d]: row (t*N + n)*ns + s = frame
    t + s of utterance n; the rows of frames t >= lens[n] hold `pad`."""
    ns = 1 - ctx[0] + ctx[-1]
    N, d = len(xs), xs[0].shape[1]
    out = np.full((Tmax * N * ns, d), pad, np.float32)
    for n, (x, tn) in enumerate(zip(xs, lens)):
        for t in range(tn):
            out[(t * N + n) * ns:(t * N + n + 1) * ns] = x[t:t + ns]
    return out


def spliced(xs, lens, Tmax, ctx=CTX):
    """The Splice output [Tmax, N, |ctx| d] in fp64 (zero rows past an utterance's frames)"""
    L = -ctx[0]
    N, d = len(xs), xs[0].shape[1]
    out = np.zeros((Tmax, N, len(ctx) * d))
    for n, (x, tn) in enumerate(zip(xs, lens)):
        for t in range(tn):
            out[t, n] = np.concatenate([x[t + L + c] for c in ctx])
    return out


def split_affine(p, out_dim):
    """AffineComponent's Vectorize order -> (W [out, in], b [out])"""
    p = np.asarray(p, np.float64)
    return p[:-out_dim].reshape(out_dim, -1), p[-out_dim:]


def clip_rows(d, thr):
    """norm-based ClipGradient backprop without repair -> (in_deriv, clipped-row mask)"""
    cfg = clip_ref.ClipCfg(thr, True, 0.01, 0.0, 0.0)
    r = clip_ref.clip_backprop(d, np.zeros_like(d), cfg, (0, 0), clip_ref.ZERO, 1.0, dtype=np.float64)
    return r.deriv, r.clipped_rows


def chain_step(oracle, x, lda, p_hidden, w_rnn, p_out, nf, fl, ll, front_threshold, hidden=H, hdim=DH):
    """x [T, N, din] fp64: the spliced input.  lda: the [DL, din + 1] matrix or
    None.  front_threshold None: the front ClipGradient passes its derivative
    through (used to find the threshold).  -> dict."""
    Tn, N, _ = x.shape
    rows = Tn * N
    z0 = x
    if lda is not None:
        lda = np.asarray(lda, np.float64)
        z0 = x @ lda[:, :-1].T + lda[:, -1]
    W, c = split_affine(p_hidden, hdim)
    z1 = z0 @ W.T + c
    h = np.where(z1 < 0, 0.0, z1)
    y, res = oracle.rnn_forward(2, np.ascontiguousarray(h), np.asarray(w_rnn, np.float64), hidden, 1, 2)
    Wa, ba = split_affine(p_out, A)
    logits = y @ Wa.T + ba
    costs, dcost = oracle.ctc(logits, fl, ll, nf)
    d = -dcost.reshape(rows, A)                                   # deriv->Scale(-1)
    g_out = np.concatenate([(d.T @ y.reshape(rows, 2 * hidden)).ravel(), d.sum(0)])
    dy, _ = clip_rows(d @ Wa, TOP_THRESHOLD)
    dh, g_rnn = oracle.rnn_backward(2, np.ascontiguousarray(h), np.asarray(w_rnn, np.float64), y,
                                    dy.reshape(Tn, N, 2 * hidden), res, hidden, 1, 2)
    dh = dh.reshape(rows, hdim)
    front_norms = np.linalg.norm(dh, axis=1)
    clipped = np.zeros(rows, bool)
    if front_threshold is not None:
        dh, clipped = clip_rows(dh, front_threshold)
    hr = h.reshape(rows, hdim)
    dz1 = np.where(hr > 0, dh, 0.0)
    g_hidden = np.concatenate([(dz1.T @ z0.reshape(rows, -1)).ravel(), dz1.sum(0)])
    return dict(costs=costs, ids=oracle.find_row_max_id(logits.reshape(rows, A).astype(np.float32)),
                grads=[g_hidden, g_rnn, g_out], front_norms=front_norms, front_clipped=clipped,
                relu_value_sum=hr.sum(0), relu_deriv_sum=(hr > 0).sum(0).astype(np.float64), rows=rows)


def relu_stats(x, lda, p_hidden):
    """(value_sum, deriv_sum, rows) of the RectifiedLinear output for input x [T, N, din]"""
    z0 = np.asarray(x, np.float64)
    if lda is not None:
        lda = np.asarray(lda, np.float64)
        z0 = z0 @ lda[:, :-1].T + lda[:, -1]
    W, c = split_affine(p_hidden, DH)
    h = np.maximum(z0 @ W.T + c, 0.0).reshape(-1, DH)
    return h.sum(0), (h > 0).sum(0).astype(np.float64), h.shape[0]
