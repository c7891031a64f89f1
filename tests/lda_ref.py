"""fp64 numpy restatement of the reference's LDA statistics and estimator:

  accumulate          LdaEstimate::Accumulate   (src/transform/lda-estimate.cc:45-55)
  get_stats           LdaEstimate::GetStats     (lda-estimate.cc:57-82)
  estimate_internal   FeatureTransformEstimate::EstimateInternal
                                                (src/nnet2/get-feature-transform.cc:40-127)
  mangle / accs_bytes LdaEstimate::Write        (lda-estimate.cc:237-260)

and of what the archive driver does around them (splice-feats' edge rule, the
blank policies).  The checker of tests/test_lda_*.py; np.linalg throughout."""
import numpy as np


def accumulate(feats, classes, weights, num_classes):
    """-> (zero [C], first [C][D], second [D][D]) of the rows with class >= 0"""
    x = np.asarray(feats, np.float64)
    cls = np.asarray(classes)
    keep = cls >= 0
    w = np.ones(len(cls)) if weights is None else np.asarray(weights, np.float64)
    x, cls, w = x[keep], cls[keep], w[keep]
    D = x.shape[1]
    zero = np.zeros(num_classes)
    first = np.zeros((num_classes, D))
    np.add.at(zero, cls, w)
    np.add.at(first, cls, x * w[:, None])
    second = (x * w[:, None]).T @ x
    return zero, first, second


def get_stats(zero, first, second):
    """-> (total_covar, between_covar, total_mean, count)"""
    zero, first, second = (np.asarray(a, np.float64) for a in (zero, first, second))
    count = zero.sum()
    mean = first.sum(0) * (1.0 / count)
    total = second * (1.0 / count) - np.outer(mean, mean)
    between = np.zeros_like(total)
    for c in range(len(zero)):
        if zero[c] != 0.0:
            cm = first[c] * (1.0 / zero[c])
            between += (zero[c] / count) * np.outer(cm, cm)
    between -= np.outer(mean, mean)
    return total, between, mean, count


def within_cholesky(total, between):
    """Cholesky factor of total - between, smoothed once as the reference does
    -> (L, smoothed?)"""
    wc = total - between
    try:
        return np.linalg.cholesky(wc), False
    except np.linalg.LinAlgError:
        smooth = float(np.float32(1.0e-03 * np.trace(wc) / wc.shape[0]))  # a BaseFloat
        return np.linalg.cholesky(wc + smooth * np.eye(wc.shape[0])), True


def whitened_eig(total, between, route="eigh"):
    """-> (d descending, U with the eigenvectors in its columns, L^-1)"""
    L, _ = within_cholesky(total, between)
    linv = np.linalg.inv(L)
    t = linv @ between @ linv.T
    t = 0.5 * (t + t.T)
    if route == "eigh":
        d, u = np.linalg.eigh(t)
        d, u = d[::-1], u[:, ::-1]
    else:  # the reference's Svd + SortSvd
        u, d, _ = np.linalg.svd(t)
    return d, u, linv


def estimate_internal(total, between, mean, dim=-1, within_class_factor=0.001, remove_offset=True,
                      max_singular_value=5.0, route="eigh"):
    """-> M float64 [dim][D (+1)]"""
    D = total.shape[0]
    target = D if dim <= 0 else dim
    assert target <= D
    d, u, linv = whitened_eig(total, between, route)
    m = (u.T @ linv)[:target]
    if within_class_factor != 1.0:
        m = m * np.sqrt((within_class_factor + d[:target]) / (1.0 + d[:target]))[:, None]
    if max_singular_value > 0.0:
        uu, s, vt = np.linalg.svd(m, full_matrices=False)
        if np.any(s > max_singular_value):
            m = uu @ (np.minimum(s, max_singular_value)[:, None] * vt)
    if remove_offset:
        m = np.concatenate([m, -(m @ mean)[:, None]], axis=1)
    return m


def estimate(zero, first, second, **kw):
    total, between, mean, _ = get_stats(zero, first, second)
    return estimate_internal(total, between, mean, **kw)


def fix_signs(m):
    """rows are defined up to sign: the largest-magnitude entry of each made positive"""
    m = np.array(m, np.float64)
    for r in m:
        if r[np.argmax(np.abs(r))] < 0:
            r *= -1.0
    return m


def mangle(zero, first, second):
    """what LdaEstimate::Write stores: float32 (zero, first, packed lower triangle
    of second - sum_c first_c first_c^T / zero_c)"""
    zero, first = np.asarray(zero, np.float64), np.asarray(first, np.float64)
    s = np.array(second, np.float64)
    for c in range(len(zero)):
        if zero[c] != 0.0:
            s += (-1.0 / zero[c]) * np.outer(first[c], first[c])
    return zero.astype(np.float32), first.astype(np.float32), s[np.tril_indices(s.shape[0])].astype(np.float32)


def accs_bytes(zero32, first32, packed32):
    """the binary <LDAACCS> file of the mangled float32 statistics, token by token"""
    C, D = first32.shape
    i32 = lambda v: b"\x04" + np.int32(v).tobytes()
    return (b"\0B<LDAACCS> <VECSIZE> " + i32(D) + b"<NUMCLASSES> " + i32(C)
            + b"<ZERO_ACCS> FV " + i32(C) + zero32.astype("<f4").tobytes()
            + b"<FIRST_ACCS> FM " + i32(C) + i32(D) + first32.astype("<f4").tobytes()
            + b"<SECOND_ACCS> FP " + i32(D) + packed32.astype("<f4").tobytes()
            + b"</LDAACCS> ")


def accs_text(zero32, first32, packed32):
    """the text <LDAACCS> file: the same tokens, numbers with 9 significant digits
    (enough to give every float back), Vector / Matrix / SpMatrix text layouts"""
    C, D = first32.shape
    num = lambda v: b"%.9g " % float(v)
    out = b"<LDAACCS> <VECSIZE> %d <NUMCLASSES> %d <ZERO_ACCS>  [ " % (D, C)
    out += b"".join(num(v) for v in zero32) + b"]\n<FIRST_ACCS>  ["
    for r in first32:
        out += b"\n  " + b"".join(num(v) for v in r)
    out += b"]\n<SECOND_ACCS> [\n"
    k = 0
    for r in range(D):
        out += b"".join(num(v) for v in packed32[k:k + r + 1]) + (b"]\n" if r == D - 1 else b"\n")
        k += r + 1
    return out + b"</LDAACCS> "


def splice(feats, context):
    """row t = the rows t + context[k] side by side, indices clamped to the ends"""
    T = feats.shape[0]
    return np.concatenate([feats[np.clip(np.arange(T) + c, 0, T - 1)] for c in context], axis=1)


def frame_classes(ali, policy):
    """skip: blank -> -1; class: as it is; fill: a blank takes the next non-blank
    label, trailing blanks the last one; -1 stays -1"""
    ali = np.asarray(ali, np.int64)
    ids = ali.copy()
    if policy == "skip":
        ids[ali == 0] = -1
    elif policy == "fill":
        nonblank = ali[ali > 0]
        nxt = int(nonblank[-1]) if len(nonblank) else -1
        for t in range(len(ali) - 1, -1, -1):
            if ali[t] > 0:
                nxt = int(ali[t])
            elif ali[t] == 0:
                ids[t] = nxt
    return ids


def separated_stats(D, seed=0, ratio=0.9, top=4.0, cov_scale=1.0, dead_dim=False, empty_class=True, n=50.0):
    """Statistics built, not sampled, so that the eigenvalues of L^-1 B L^-T are
    top * ratio^k: a shared full-rank within-class covariance W and 2 D' classes
    of n frames whose means are mean +- sqrt(D') * column k of L Q diag(sqrt(d)).
    dead_dim: the last dimension is identically zero (W singular: the smoothing
    retry); empty_class: one more class with no frames.  -> (zero, first, second)"""
    rng = np.random.default_rng(seed)
    De = D - 1 if dead_dim else D
    a = rng.standard_normal((De, De))
    W = cov_scale * (a @ a.T / De + 0.5 * np.eye(De))
    L = np.linalg.cholesky(W)
    q, _ = np.linalg.qr(rng.standard_normal((De, De)))
    d = top * ratio ** np.arange(De)
    G = (L @ q) * np.sqrt(d)
    mean = rng.standard_normal(De)
    means = np.concatenate([mean + np.sqrt(De) * G.T, mean - np.sqrt(De) * G.T])
    C = 2 * De
    zero = np.full(C, float(n))
    first = n * means
    second = n * C * (W + G @ G.T + np.outer(mean, mean))
    if dead_dim:
        first = np.pad(first, ((0, 0), (0, 1)))
        second = np.pad(second, ((0, 1), (0, 1)))
    if empty_class:
        zero = np.append(zero, 0.0)
        first = np.pad(first, ((0, 1), (0, 0)))
    return zero, np.ascontiguousarray(first), 0.5 * (second + second.T)


def sampled_data(D, C, R, seed=0):
    """class means plus a shared full-rank covariance -> (feats float32 [R][D], classes [R])"""
    rng = np.random.default_rng(seed)
    means = 2.0 * rng.standard_normal((C, D))
    mix = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    cls = rng.integers(0, C, R)
    return (means[cls] + rng.standard_normal((R, D)) @ mix).astype(np.float32), cls.astype(np.int32)
