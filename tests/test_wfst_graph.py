"""The graph object (include/kaldi_ctc_decode.h, kctc_graph_*) on the CPU: the
OpenFst text round trip, the arc order of the stored graph, eps_depth, and one
case per refusal of kctc_graph_create."""
import numpy as np
import pytest

import wfst_ref as ref

INF = np.inf


def _chain():
    # 0 -eps-> 1 -eps-> 2 -eps-> 3 (depth 3), a side epsilon 0 -> 2, emitting arcs, arcs given out of order
    return dict(final_costs=[INF, INF, 0.5, 0.0, INF],
                src=[2, 0, 1, 0, 3, 0, 3], ilabel=[0, 0, 0, 2, 1, 0, 2], olabel=[0, 7, 0, 0, 4, 0, 9],
                weight=[0.25, -1.5, 0.0, 2.0, 0.125, 1.0, 3.5], dst=[3, 1, 2, 4, 3, 2, 0])


def test_arc_order_and_info(kctc):
    g = kctc.Graph(**_chain())
    assert (g.num_states, g.num_arcs, g.eps_depth) == (5, 7, 3)
    assert g.info()["max_ilabel"] == 2 and g.info()["max_col"] == 1
    a = g.arrays()
    # stable sort by src: state 0's arcs keep their input order
    assert a["src"].tolist() == [0, 0, 0, 1, 2, 3, 3]
    assert a["ilabel"].tolist() == [0, 2, 0, 0, 0, 1, 2]
    assert a["olabel"].tolist() == [7, 0, 0, 0, 0, 4, 9]
    assert a["dst"].tolist() == [1, 4, 2, 2, 3, 3, 0]
    assert a["weight"].tolist() == [-1.5, 2.0, 1.0, 0.0, 0.25, 0.125, 3.5]
    r = ref.RefGraph(**_chain())
    assert r.src.tolist() == a["src"].tolist() and r.dst.tolist() == a["dst"].tolist()
    g.close()
    g.close()


def test_ilabel_to_col(kctc):
    g = kctc.Graph(**_chain(), ilabel_to_col=[-1, 5, 3])  # entry 0 is never read
    assert g.info()["max_col"] == 5


def test_text_round_trip(kctc, tmp_path):
    rng = np.random.default_rng(3)
    d = ref.random_graph(rng, 40, 6)
    d["start"] = 17
    g = kctc.Graph(**d)
    p = tmp_path / "g.txt"
    g.write_text(p)
    h = kctc.Graph.read_text(p)
    a, b = g.arrays(), h.arrays()
    assert a["start"] == b["start"] == 17
    for k in ("final_costs", "src", "ilabel", "olabel", "weight", "dst"):
        assert np.array_equal(a[k], b[k]), k
    assert h.eps_depth == g.eps_depth


def test_read_text_defaults(kctc, tmp_path):
    p = tmp_path / "g.txt"
    p.write_text("2 0 1 5\n0 1 0 0 0.5\n1 2 3 0 -2\n1\n0 1.5\n")
    g = kctc.Graph.read_text(p)
    a = g.arrays()
    assert a["start"] == 2 and g.num_states == 3
    assert a["src"].tolist() == [0, 1, 2] and a["weight"].tolist() == [0.5, -2.0, 0.0]  # a missing weight is 0
    assert a["final_costs"].tolist() == [1.5, 0.0, INF]
    p.write_text("0 1 a b\n")
    with pytest.raises(kctc.KctcError, match="integer"):
        kctc.Graph.read_text(p)
    with pytest.raises(kctc.KctcError):
        kctc.Graph.read_text(tmp_path / "missing.txt")


def _bad(**changes):
    d = _chain()
    for k, v in changes.items():
        d[k] = v
    return d


REFUSALS = {
    "src out of range": _bad(src=[2, 0, 1, 0, 5, 0, 3]),
    "dst out of range": _bad(dst=[3, 1, 2, 4, 3, 2, -1]),
    "start out of range": _bad(start=5),
    "negative ilabel": _bad(ilabel=[0, 0, 0, 2, -1, 0, 2]),
    "negative olabel": _bad(olabel=[0, 7, 0, 0, -4, 0, 9]),
    "ilabel outside the column table": _bad(ilabel_to_col=[0, 0]),
    "infinite weight": _bad(weight=[0.25, -1.5, 0.0, INF, 0.125, 1.0, 3.5]),
    "nan weight": _bad(weight=[0.25, -1.5, 0.0, 2.0, np.nan, 1.0, 3.5]),
    "nan final cost": _bad(final_costs=[INF, INF, np.nan, 0.0, INF]),
    "-inf final cost": _bad(final_costs=[INF, INF, 0.5, -INF, INF]),
    "negative column": _bad(ilabel_to_col=[0, 2, -1]),
    "epsilon cycle": _bad(src=[2, 0, 1, 0, 3, 0, 3, 3], ilabel=[0, 0, 0, 2, 1, 0, 2, 0], olabel=[0] * 8,
                          weight=[0.0] * 8, dst=[3, 1, 2, 4, 3, 2, 0, 1]),
    "epsilon self-loop": _bad(src=[1], ilabel=[0], olabel=[0], weight=[1.0], dst=[1]),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_create_refuses(kctc, what):
    with pytest.raises(kctc.KctcError):
        kctc.Graph(**REFUSALS[what])


def test_builders_refuse(kctc):
    with pytest.raises(kctc.KctcError):
        kctc.ctc_token_graph(1)
    with pytest.raises(kctc.KctcError):
        kctc.ctc_lexicon_graph([(0, [1])], 3)
    with pytest.raises(kctc.KctcError):
        kctc.ctc_lexicon_graph([(1, [0])], 3)  # blank inside a pronunciation
    g = kctc.ctc_lexicon_graph([(1, [1, 2]), (2, [1])], 3)
    assert g.eps_depth == 1 and g.info()["max_col"] == 2
