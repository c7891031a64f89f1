"""fp64 numpy restatement of the graph search (include/kaldi_ctc_decode.h,
kctc_wfst_decode_async): token sets as dense cost / arc arrays, the closure,
the exact selection and the emission exactly as the header states them; an
exact dense Viterbi (beam inf, no max_active); a path scorer; a search of the
cheapest path that is consistent with given frame ilabels (and words), written
separately with dictionaries; and a brute force over all frame sequences."""
import itertools

import numpy as np

INF = np.inf


class RefGraph:
    """arcs sorted stably by src: the position is the arc id"""

    def __init__(self, final_costs, src, ilabel, olabel, weight, dst, start=0, ilabel_to_col=None):
        src = np.asarray(src, np.int64).reshape(-1)
        order = np.argsort(src, kind="stable")
        self.S = len(final_costs)
        self.start = int(start)
        self.fin = np.asarray(final_costs, np.float64)
        self.src = src[order]
        self.il = np.asarray(ilabel, np.int64).reshape(-1)[order]
        self.ol = np.asarray(olabel, np.int64).reshape(-1)[order]
        self.w = np.asarray(weight, np.float32).reshape(-1)[order].astype(np.float64)  # the graph stores floats
        self.dst = np.asarray(dst, np.int64).reshape(-1)[order]
        n_il = int(self.il.max()) + 1 if len(self.il) else 1
        self.col = np.arange(-1, n_il - 1) if ilabel_to_col is None else np.asarray(ilabel_to_col, np.int64)
        self.eps = np.flatnonzero(self.il == 0)
        self.emit = np.flatnonzero(self.il != 0)
        self.out = [[] for _ in range(self.S)]  # arc ids per state (for the dictionary search)
        for a, s in enumerate(self.src):
            self.out[s].append(a)

    @classmethod
    def from_graph(cls, g, ilabel_to_col=None):
        """from a kaldi_ctc_amd.Graph"""
        a = g.arrays()
        return cls(a["final_costs"], a["src"], a["ilabel"], a["olabel"], a["weight"], a["dst"], a["start"],
                   ilabel_to_col)

    def arrays(self):
        return dict(final_costs=self.fin.astype(np.float32), src=self.src, ilabel=self.il, olabel=self.ol,
                    weight=self.w.astype(np.float32), dst=self.dst, start=self.start)


def _relax(cost, arc, cand, ids, dst):
    """(cost, arc)[dst] <- the lexicographic minimum with the candidates; True if anything changed"""
    if len(cand) == 0:
        return False
    order = np.lexsort((ids, cand, dst))
    d = dst[order]
    first = np.ones(len(d), bool)
    first[1:] = d[1:] != d[:-1]
    d, c, a = d[first], cand[order][first], ids[order][first]
    better = (c < cost[d]) | ((c == cost[d]) & (a < arc[d]))
    cost[d[better]] = c[better]
    arc[d[better]] = a[better]
    return bool(better.any())


def _closure(g, cost, arc):
    while True:
        live = np.isfinite(cost[g.src[g.eps]])
        e = g.eps[live]
        if not _relax(cost, arc, cost[g.src[e]] + g.w[e], e, g.dst[e]):
            return


def decode(g, ll, beam=INF, max_active=None, acoustic_scale=1.0, stats=None):
    """ll [T, A] log-likelihoods -> (words, ali [T], score, status, arcs): the
    recursion of the header in fp64.  arcs: the arc ids of the path.  stats, if
    a dict, receives the mean |E_t| and |Q_t|."""
    ll = np.asarray(ll, np.float64)
    T = ll.shape[0]
    NONE = np.iinfo(np.int64).max
    cost = np.full(g.S, INF)
    arc = np.full(g.S, NONE)
    cost[g.start], arc[g.start] = 0.0, -1
    _closure(g, cost, arc)
    hist = [arc.copy()]
    nE = nQ = 0
    for t in range(T):
        live = np.flatnonzero(np.isfinite(cost))
        nQ += len(live)
        if len(live) == 0:
            break
        best = cost[live].min()
        inb = live[cost[live] <= best + beam]
        if max_active is not None and len(inb) > max_active:
            inb = inb[np.lexsort((inb, cost[inb]))[:max_active]]
        nE += len(inb)
        sel = np.zeros(g.S, bool)
        sel[inb] = True
        e = g.emit[sel[g.src[g.emit]]]
        ncost = np.full(g.S, INF)
        narc = np.full(g.S, NONE)
        _relax(ncost, narc, cost[g.src[e]] + g.w[e] - acoustic_scale * ll[t, g.col[g.il[e]]], e, g.dst[e])
        _closure(g, ncost, narc)
        cost, arc = ncost, narc
        hist.append(arc.copy())
    if stats is not None:
        stats.update(mean_E=nE / max(T, 1), mean_Q=nQ / max(T, 1))
    live = np.flatnonzero(np.isfinite(cost))
    if len(hist) <= T or len(live) == 0:
        return [], np.full(T, -1, np.int32), INF, -1, []
    fin = live[np.isfinite(g.fin[live])]
    if len(fin):
        tot = cost[fin] + g.fin[fin]
        s, status = int(fin[np.lexsort((fin, tot))[0]]), 1
        score = float(cost[s] + g.fin[s])
    else:
        s, status = int(live[np.lexsort((live, cost[live]))[0]]), 0
        score = float(cost[s])
    arcs, t = [], T
    while True:
        a = int(hist[t][s])
        if a < 0:
            break
        arcs.append(a)
        if g.il[a] != 0:
            t -= 1
        s = int(g.src[a])
    arcs.reverse()
    words = [int(g.ol[a]) for a in arcs if g.ol[a] != 0]
    ali = np.array([g.il[a] for a in arcs if g.il[a] != 0], np.int32)
    return words, ali, score, status, arcs


def viterbi(g, ll, acoustic_scale=1.0):
    """the exact search: nothing pruned"""
    return decode(g, ll, INF, None, acoustic_scale)


def path_cost(g, ll, arcs, acoustic_scale=1.0, with_final=True):
    """graph + acoustic (+ final) cost of a path given by arc ids from the start state, in fp64"""
    ll = np.asarray(ll, np.float64)
    s, t, c = g.start, 0, 0.0
    for a in arcs:
        assert g.src[a] == s, "the arcs do not chain"
        c += g.w[a]
        if g.il[a] != 0:
            c -= acoustic_scale * ll[t, g.col[g.il[a]]]
            t += 1
        s = int(g.dst[a])
    assert t == ll.shape[0], "the path does not consume every frame"
    return c + (g.fin[s] if with_final else 0.0), s


def consistent_cost(g, ll, ali, words=None, need_final=True, acoustic_scale=1.0):
    """The cost of the cheapest path from the start state whose emitting arcs
    carry exactly the ilabels `ali` (one per frame) and, if words is given,
    whose non-zero olabels are exactly `words`; with need_final it ends on a
    final state and includes the final cost.  inf: there is no such path.  A
    dictionary (state, words emitted) -> cost, independent of decode()."""
    ll = np.asarray(ll, np.float64)

    def step_ok(a, k):
        o = int(g.ol[a])
        if o == 0 or words is None:
            return k
        return k + 1 if k < len(words) and words[k] == o else None

    def closure(tok):
        work = list(tok)
        while work:
            s, k = work.pop()
            c = tok[(s, k)]
            for a in g.out[s]:
                if g.il[a] != 0:
                    continue
                k2 = step_ok(a, k)
                if k2 is None:
                    continue
                key = (int(g.dst[a]), k2)
                if c + g.w[a] < tok.get(key, INF):
                    tok[key] = c + g.w[a]
                    work.append(key)
        return tok

    tok = closure({(g.start, 0): 0.0})
    for t, i in enumerate(ali):
        nxt = {}
        for (s, k), c in tok.items():
            for a in g.out[s]:
                if g.il[a] != i:
                    continue
                k2 = step_ok(a, k)
                if k2 is None:
                    continue
                key = (int(g.dst[a]), k2)
                v = c + g.w[a] - acoustic_scale * ll[t, g.col[i]]
                if v < nxt.get(key, INF):
                    nxt[key] = v
        tok = closure(nxt)
    best = INF
    for (s, k), c in tok.items():
        if words is not None and k != len(words):
            continue
        if need_final:
            c = c + g.fin[s]
        best = min(best, c)
    return best


def brute_force(g, ll, acoustic_scale=1.0):
    """min over all frame-ilabel sequences of the cheapest consistent path that ends on a final state"""
    T = np.asarray(ll).shape[0]
    labels = sorted(set(int(i) for i in g.il if i != 0))
    return min((consistent_cost(g, ll, z, None, True, acoustic_scale) for z in itertools.product(labels, repeat=T)),
               default=INF)


def collapsed_argmax(ll, blank=0):
    path = np.asarray(ll).argmax(axis=1)
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(int(v))
        prev = v
    return out


# ---- graphs for the tests -----------------------------------------------------------
def linear_graph(labels, blank=0):
    """the CTC forced-alignment graph of one transcript (columns): states 0..2L, even = blank"""
    L = len(labels)
    S = 2 * L + 1
    src, il, ol, dst = [], [], [], []
    for s in range(S):
        c = blank if s % 2 == 0 else labels[s // 2]
        src.append(s); il.append(c + 1); ol.append(0); dst.append(s)  # stay
        if s + 1 < S:
            c1 = blank if (s + 1) % 2 == 0 else labels[(s + 1) // 2]
            src.append(s); il.append(c1 + 1); ol.append(c1 if (s + 1) % 2 else 0); dst.append(s + 1)
        if s % 2 == 1 and s + 2 < S and labels[s // 2] != labels[s // 2 + 1]:
            c2 = labels[s // 2 + 1]
            src.append(s); il.append(c2 + 1); ol.append(c2); dst.append(s + 2)
    # the first frame is consumed by an arc out of a start state in front of state 0
    src += [S, S] if L else [S]
    il += [blank + 1, labels[0] + 1] if L else [blank + 1]
    ol += [0, labels[0]] if L else [0]
    dst += [0, 1] if L else [0]
    fin = np.full(S + 1, INF, np.float32)
    fin[S - 1] = 0
    if L:
        fin[S - 2] = 0
    return dict(final_costs=fin, src=src, ilabel=il, olabel=ol, weight=np.zeros(len(src), np.float32), dst=dst,
                start=S)


def random_graph(rng, S, A, big_state=None, big_arcs=300):
    """Out-degree 1..4, about 30 % epsilon arcs (lower -> higher state id only,
    chains of depth >= 3 when S allows), some negative weights, dead ends, 20 %
    of the states final; big_state gets big_arcs emitting arcs."""
    src, il, ol, w, dst = [], [], [], [], []
    dead = set(rng.choice(S, size=S // 10, replace=False).tolist()) - {0} if S >= 10 else set()
    for s in range(S):
        if s in dead:
            continue
        for _ in range(int(rng.integers(1, 5))):
            eps = rng.random() < 0.3 and s + 1 < S
            src.append(s)
            il.append(0 if eps else int(rng.integers(1, A + 1)))
            ol.append(int(rng.integers(1, 50)) if rng.random() < 0.4 else 0)
            w.append(float(rng.normal(0.5, 1.0)))
            dst.append(int(rng.integers(s + 1, min(S, s + 20))) if eps else int(rng.integers(0, S)))
    if S >= 4:  # an epsilon chain of depth 3 out of the start state
        for s in range(3):
            src.append(s); il.append(0); ol.append(s + 1); w.append(0.1 * (s - 1)); dst.append(s + 1)
    if big_state is not None:
        for k in range(big_arcs):
            src.append(big_state); il.append(1 + k % A); ol.append(1 + k % 7); w.append(float(rng.random()))
            dst.append(int(rng.integers(0, S)))
    if S == 1:
        src, il, ol, w, dst = [0, 0], [1, 2], [0, 3], [0.25, 0.5], [0, 0]
    fin = np.where(rng.random(S) < 0.2, rng.random(S), INF).astype(np.float32)
    if S == 1:
        fin[0] = 0.5
    return dict(final_costs=fin, src=src, ilabel=il, olabel=ol, weight=np.asarray(w, np.float32), dst=dst, start=0)
