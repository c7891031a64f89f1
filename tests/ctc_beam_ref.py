"""fp64 numpy restatement of the CTC prefix beam search (include/ctc.h,
mictc_ctc_beam_search_async): log-softmax in fp64 from the fp32 activations,
then the stay / extend / merge / prune recursion exactly as the header states
it.  Prefixes are tuples and the beam is looked up through a dict of them, so
merging is exact.  Also here: the exact CTC log-probability of a label
sequence (fp64 alpha recursion) and a brute force over all A^T alignments."""
import itertools

import numpy as np

from ctc_align_ref import collapse, log_softmax64  # noqa: F401  (re-exported)


def top_symbols(row, symbols, blank):
    """the K = min(symbols, A-1) non-blank symbols of largest row[c], ties to the lower id, best first"""
    ids = np.array([a for a in range(len(row)) if a != blank])
    order = np.lexsort((ids, -row[ids]))  # by -lp, then by id
    return ids[order[:min(symbols, len(ids))]]


def beam_search(lp, beam, symbols, blank=0):
    """lp [T, A] fp64 log-probs -> (labels list, score = tot of the winner).
    Entries of probability zero never enter the beam; prune ties go to stay
    candidates before extensions and to the earlier beam entry (no caller may
    depend on that)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, A = lp.shape
    prefixes = [()]
    b = np.array([0.0])
    nb = np.array([-np.inf])
    for t in range(T):
        row = lp[t]
        C = top_symbols(row, symbols, blank)
        pos_of = {int(c): k for k, c in enumerate(C)}
        n = len(prefixes)
        last = np.array([p[-1] if p else -1 for p in prefixes])
        tot = np.logaddexp(b, nb)
        stay_b = row[blank] + tot
        stay_nb = np.where(last >= 0, row[np.maximum(last, 0)] + nb, -np.inf)
        ext = row[C][None, :] + np.where(C[None, :] == last[:, None], b[:, None], tot[:, None])  # [n, K]
        # merge: p + c that is already in the beam is that entry
        index = {p: i for i, p in enumerate(prefixes)}
        for q, p in enumerate(prefixes):
            if not p:
                continue
            par = index.get(p[:-1])
            k = pos_of.get(p[-1])
            if par is not None and k is not None:
                stay_nb[q] = np.logaddexp(stay_nb[q], ext[par, k])
                ext[par, k] = -np.inf
        cand = np.concatenate([np.logaddexp(stay_b, stay_nb), ext.reshape(-1)])
        order = np.argsort(-cand, kind="stable")
        order = order[:beam]
        order = order[cand[order] > -np.inf]
        new_p, new_b, new_nb = [], [], []
        for e in order:
            if e < n:
                new_p.append(prefixes[e])
                new_b.append(stay_b[e])
                new_nb.append(stay_nb[e])
            else:
                i, k = divmod(int(e) - n, len(C))
                new_p.append(prefixes[i] + (int(C[k]),))
                new_b.append(-np.inf)
                new_nb.append(ext[i, k])
        prefixes, b, nb = new_p, np.array(new_b), np.array(new_nb)
    tot = np.logaddexp(b, nb)
    w = int(np.argmax(tot))
    return list(prefixes[w]), float(tot[w])


def decode(acts, beam, symbols, blank=0):
    """acts [T, A] fp32 un-normalised -> (labels, score, lp64)"""
    acts = np.asarray(acts)
    if acts.shape[0] == 0:
        return [], 0.0, np.zeros(acts.shape, np.float64)
    lp = log_softmax64(acts)
    hyp, score = beam_search(lp, beam, symbols, blank)
    return hyp, score, lp


def exact_logprob(lp, labels, blank=0):
    """log sum over all alignments of lp [T, A] that collapse to labels (fp64 alpha recursion)"""
    lp = np.asarray(lp, dtype=np.float64)
    T, L = lp.shape[0], len(labels)
    if T == 0:
        return 0.0 if L == 0 else -np.inf
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = labels
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    a = np.full(S, -np.inf)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, ext[1]]
    for t in range(1, T):
        c1 = np.concatenate(([-np.inf], a[:-1]))
        c2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], a[:-2]))[:S], -np.inf)
        a = np.logaddexp(np.logaddexp(a, c1), c2) + lp[t, ext]
    return float(np.logaddexp(a[S - 1], a[S - 2]) if S > 1 else a[0])


def brute_force(lp, blank=0):
    """dict label tuple -> log-probability, over all A^T alignments of lp [T, A]"""
    lp = np.asarray(lp, dtype=np.float64)
    T, A = lp.shape
    out = {}
    for path in itertools.product(range(A), repeat=T):
        s = float(sum(lp[t, a] for t, a in enumerate(path)))
        k = tuple(collapse(path, blank))
        out[k] = np.logaddexp(out.get(k, -np.inf), s)
    return out
