"""fp64 numpy restatement of the CTC forced alignment (include/ctc.h,
mictc_ctc_align_async): log-softmax in fp64 from the fp32 activations, then
the max-product recursion over the blank-interleaved labels with its tie
rule, end rule and backtrace, exactly as the header states them."""
import numpy as np


def log_softmax64(acts):
    """acts [T, A] (any float type) -> fp64 log-softmax per row"""
    x = np.asarray(acts, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def feasible(T, labels):
    rep = sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1])
    return T > 0 and len(labels) + rep <= T


def collapse(path, blank=0):
    """remove repeats, then blanks"""
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out


def viterbi(lp, labels, blank=0, dtype=np.float64):
    """lp [T, A] log-probs, labels a list -> (path int32 [T], score) of the
    best path; an infeasible utterance gives (all -1, -inf).  dtype: the
    arithmetic of the recursion (fp64; fp32 to see what fp32 rounding does)."""
    lp = np.asarray(lp, dtype=dtype)
    T, L = lp.shape[0], len(labels)
    if not feasible(T, labels):
        return np.full(T, -1, np.int32), -np.inf
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    ninf = dtype(-np.inf)
    v = np.full(S, ninf, dtype)
    v[0] = lp[0, blank]
    if S > 1:
        v[1] = lp[0, ext[1]]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        c0 = v
        c1 = np.concatenate(([ninf], v[:-1]))
        c2 = np.where(skip, np.concatenate(([ninf, ninf], v[:-2]))[:S], ninf)
        best, b = c0.copy(), np.zeros(S, np.int8)
        m = c1 > best  # a later candidate wins only if it is strictly greater
        best[m], b[m] = c1[m], 1
        m = c2 > best
        best[m], b[m] = c2[m], 2
        v = (best + lp[t, ext]).astype(dtype)
        bp[t] = b
    s = S - 1
    if S > 1 and v[S - 2] > v[S - 1]:
        s = S - 2
    score = float(v[s])
    path = np.empty(T, np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = ext[s]
        s -= int(bp[t, s])
    return path, score


def align(acts, labels, blank=0):
    """acts [T, A] fp32 un-normalised -> (path, score, lp64)"""
    lp = log_softmax64(acts)
    path, score = viterbi(lp, labels, blank)
    return path, score, lp
