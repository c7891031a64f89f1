"""ClipGradientComponent on the device (csrc/clipgrad.hip, k_rownorm_clip) through
the Component C ABI against tests/clip_ref.py, the numpy restatement of
ClipGradientComponent::Backprop + RepairGradients
(src/nnet2/nnet-cudnn-component.cc:921-1075).

Counters are read back from the component's text Write; the RandUniform()
draws of a handle come from its own glibc stream (comp.srand), the expected
ones from glibc_rand_uniforms.  Inputs are built so that fp32 and fp64 agree on
every discrete outcome (clip_ref.make_deriv), the engineered ties included.

Tolerance: 2e-6 against the fp64 restatement, norm-wise per call and row-wise
over the clipped or repaired rows; tests/test_clip_ref.py shows the
reference's own fp32 arithmetic within it (1.5e-7 at worst).  Counters, draws
and decisions are exact."""
import re

import numpy as np
import pytest

import clip_ref as cr
from clip_ref import ClipCfg, Counters
from conftest import rel_err
from test_train_gpu import glibc_rand_uniforms

pytestmark = pytest.mark.gpu

TOL = 2e-6
TAGS = ("NumElementsClipped", "NumElementsProcessed", "NumSelfRepaired", "NumBackpropped")


def parse_counters(text):
    return Counters(*(int(re.search(rf"<{t}>\s+(-?\d+)\s", text).group(1)) for t in TAGS))


def model_text(comp, tmp_path):
    p = tmp_path / "clip_counters.txt"
    comp.Write(p, binary=False)
    return p.read_text()


def counters(comp, tmp_path):
    return parse_counters(model_text(comp, tmp_path))


def proportion(comp):
    return float(re.search(r"clipped-proportion=([^,]+)", comp.Info()).group(1))


def make_comp(kctc, tmp_path, dim, cfg, num_clipped=0, count=0):
    """A component with settings cfg; with counts given, one read from a text
    model whose <NumElementsClipped> / <NumElementsProcessed> were edited."""
    comp = kctc.Component(cr.config_line(dim, cfg))
    if not (num_clipped or count):
        return comp
    text = model_text(comp, tmp_path)
    comp.close()
    text = re.sub(r"(<NumElementsClipped>\s+)\d+", rf"\g<1>{num_clipped}", text)
    text = re.sub(r"(<NumElementsProcessed>\s+)\d+", rf"\g<1>{count}", text)
    p = tmp_path / "clip_edited.txt"
    p.write_text(text)
    comp = kctc.Component.ReadNew(p)
    assert counters(comp, tmp_path) == Counters(num_clipped, count, 0, 0)
    return comp


def backprop(comp, gpu, od, iv, to_update=None, alias=False):
    """in_deriv (numpy) of comp.Backprop on out_deriv od, in_value iv (numpy)."""
    import torch
    rows = od.shape[0]
    x = torch.from_numpy(iv).to(gpu)
    dy = torch.from_numpy(od).to(gpu)
    dx = dy if alias else torch.full_like(dy, float("nan"))
    comp.Backprop(rows, 1, x, None, dy, to_update, dx)
    torch.cuda.synchronize()
    if not alias:
        assert torch.equal(dy.cpu(), torch.from_numpy(od))      # out_deriv is read only
    return dx.cpu().numpy()


def seed_where(pred, n):
    """The first srand seed whose first n RandUniform() draws satisfy pred."""
    for seed in range(1, 2000):
        draws = glibc_rand_uniforms(seed, n)
        if pred(draws):
            return seed, draws
    raise AssertionError("no seed found")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_deriv(got, res, name):
    """got vs the fp64 restatement res: norm-wise, and row-wise over the rows
    the call changed; -> the larger error."""
    e = rel_err(got, res.deriv)
    rows = np.ones(len(got), bool) if res.repaired else res.clipped_rows
    er = cr.row_rel_err(got[rows], res.deriv[rows])
    print(f"clipgrad {name}: norm-wise {e:.2e} row-wise {er:.2e}")
    assert np.isfinite(got).all(), name
    # measured on MI355X, the larger of the two: clipping alone 8.2e-8 (1030 x 63), active repair 8.3e-8,
    # the counter sequence 7.8e-8, element-wise mode with repair 8.0e-8
    assert e < TOL and er < TOL, (name, e, er)
    return max(e, er)


@pytest.mark.parametrize("rows,dim", cr.SHAPES, ids=[f"{r}x{d}" for r, d in cr.SHAPES])
@pytest.mark.parametrize("how", ["scale0", "none"])
def test_norm_based_no_repair(kctc, gpu, tmp_path, rows, dim, how):
    """Clipping alone, with self-repair-scale=0 (to_update = itself) or with
    to_update=None: the fp64 derivative, rows below the threshold untouched to
    the bit, the exact-tie row counted and unchanged, counters only on a
    to_update."""
    import torch
    cfg = ClipCfg(cr.THRESHOLD, True, 0.05, 0.0, 0.0 if how == "scale0" else 1.0)
    tie = cr.tie_row_of(rows)
    od, iv = cr.make_deriv(rows, dim, 11, tie_row=tie), cr.make_in_value(rows, dim, 11)
    comp = make_comp(kctc, tmp_path, dim, cfg)
    x = torch.from_numpy(iv).to(gpu)
    assert torch.equal(comp.Propagate(rows, 1, x), x)
    upd = cr.ZERO if how == "scale0" else None
    res = cr.clip_backprop(od, iv, cfg, (0, 0), upd, 0.1, to_update_is_self=upd is not None)
    assert not res.drew and not res.repaired
    got = backprop(comp, gpu, od, iv, comp if how == "scale0" else None)
    check_deriv(got, res, f"no repair {rows}x{dim} {how}")
    keep = ~res.clipped_rows
    np.testing.assert_array_equal(bits(got[keep]), bits(od[keep]))
    if tie is not None:
        assert res.clipped_rows[tie]
        np.testing.assert_array_equal(bits(got[tie]), bits(od[tie]))
    assert counters(comp, tmp_path) == (res.counters if upd is not None else cr.ZERO)
    # a second call accumulates (the per-step clip count starts from zero again)
    if upd is not None:
        res2 = cr.clip_backprop(od, iv, cfg, None, res.counters, 0.1, to_update_is_self=True)
        np.testing.assert_array_equal(bits(backprop(comp, gpu, od, iv, comp)), bits(got))
        assert counters(comp, tmp_path) == res2.counters
        assert res2.counters.num_clipped == 2 * int(res.clipped_rows.sum())
        assert proportion(comp) == pytest.approx(res2.counters.num_clipped / res2.counters.count, rel=1e-5)
    comp.close()


@pytest.mark.parametrize("norm_based", [True, False], ids=["norm", "element"])
def test_to_update_none_changes_no_counter(kctc, gpu, tmp_path, norm_based):
    """Backprop(..., to_update = NULL, ...) clips and changes no counter of any
    component (nnet-cudnn-component.cc:953-957, 965-968)."""
    rows, dim = 7, 65
    cfg = ClipCfg(cr.THRESHOLD, norm_based, 0.05, 0.0, 1.0)
    comp = make_comp(kctc, tmp_path, dim, cfg, 5, 16)
    other = comp.Copy()
    comp.srand(3)
    od, iv = cr.make_deriv(rows, dim, 13, clip_pattern=[True] * rows), cr.make_in_value(rows, dim, 13)
    before, info = model_text(comp, tmp_path), comp.Info()
    before_other = model_text(other, tmp_path)
    res = cr.clip_backprop(od, iv, cfg, (5, 16), None, 0.1)
    for _ in range(2):
        got = backprop(comp, gpu, od, iv, None)
        assert rel_err(got, res.deriv) < TOL
    assert model_text(comp, tmp_path) == before
    assert parse_counters(before) == Counters(5, 16, 0, 0)
    assert comp.Info() == info and proportion(comp) == pytest.approx(5 / 16)
    assert model_text(other, tmp_path) == before_other
    # a Copy() taken afterwards starts from the same counters
    c2 = comp.Copy()
    assert counters(c2, tmp_path) == Counters(5, 16, 0, 0)
    # ... and no draw was consumed: the next gated Backprop follows draw number 1
    seed, draws = seed_where(lambda d: d[0] <= 0.5 < d[1], 2)
    comp.srand(seed)
    for _ in range(2):
        backprop(comp, gpu, od, iv, None)
    res = cr.clip_backprop(od, iv, cfg, None, Counters(5, 16, 0, 0), draws[0], to_update_is_self=True)
    assert res.repaired
    got = backprop(comp, gpu, od, iv, comp)
    assert rel_err(got, res.deriv) < TOL
    assert counters(comp, tmp_path) == res.counters
    for c in (comp, other, c2):
        c.close()


CASES = cr.repair_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_active_repair(kctc, gpu, tmp_path, case):
    """One Backprop with an active self-repair at every shape, over
    self-repair-target in {0, 0.5, 3.0} and self-repair-scale in {1, 0.25}."""
    name, rows, dim, cfg, od, iv = case
    comp = make_comp(kctc, tmp_path, dim, cfg, *cr.PRIMED)
    seed, draws = seed_where(lambda d: d[0] <= 0.5, 1)
    comp.srand(seed)
    res = cr.clip_backprop(od, iv, cfg, None, Counters(*cr.PRIMED, 0, 0), draws[0], to_update_is_self=True)
    assert res.drew and res.repaired
    got = backprop(comp, gpu, od, iv, comp)
    check_deriv(got, res, f"active repair {name}")
    assert counters(comp, tmp_path) == res.counters
    # the same call on a second component of equal state: the same bits (fixed-order sums)
    comp2 = make_comp(kctc, tmp_path, dim, cfg, *cr.PRIMED)
    comp2.srand(seed)
    np.testing.assert_array_equal(bits(backprop(comp2, gpu, od, iv, comp2)), bits(got))
    # in_deriv aliasing out_deriv
    comp3 = make_comp(kctc, tmp_path, dim, cfg, *cr.PRIMED)
    comp3.srand(seed)
    np.testing.assert_array_equal(bits(backprop(comp3, gpu, od, iv, comp3, alias=True)), bits(got))
    # the other side of the draw: clipped only
    seed_hi, draws_hi = seed_where(lambda d: d[0] > 0.5, 1)
    comp3.srand(seed_hi)
    res_hi = cr.clip_backprop(od, iv, cfg, None, res.counters, draws_hi[0], to_update_is_self=True)
    assert res_hi.drew and not res_hi.repaired
    got_hi = backprop(comp3, gpu, od, iv, comp3)
    check_deriv(got_hi, res_hi, f"draw > 0.5 {name}")
    assert counters(comp3, tmp_path) == res_hi.counters
    for c in (comp, comp2, comp3):
        c.close()


def test_counter_sequence(kctc, gpu, tmp_path):
    """Eight calls of 8 rows on one component with to_update = itself,
    threshold 4, repair threshold 0.25: 0, 4, 1, 8, 8, ... rows clip, so the
    proportions are 0, 4/16 (a tie: no repair), 5/24, 13/32, 21/40, ...; after
    every call the derivative and the four counters are the restatement's, and
    NumSelfRepaired rises only on an active repair."""
    cfg, n = cr.SEQ_CFG, len(cr.SEQ_CLIPS)
    # the first four draws <= 0.5 (only the proportion gates there); later both sides occur
    seed, draws = seed_where(lambda d: max(d[:4]) <= 0.5 and min(d[4:]) <= 0.5 < max(d[4:]), n)
    comp = make_comp(kctc, tmp_path, cr.SEQ_DIM, cfg)
    comp.srand(seed)
    state, repaired, worst = cr.ZERO, [], 0.0
    for i, (od, iv) in enumerate(cr.sequence_inputs()):
        res = cr.clip_backprop(od, iv, cfg, None, state, draws[i], to_update_is_self=True)
        assert res.drew and int(res.clipped_rows.sum()) == cr.SEQ_CLIPS[i]
        got = backprop(comp, gpu, od, iv, comp)
        worst = max(worst, check_deriv(got, res, f"sequence call {i}"))
        now = counters(comp, tmp_path)
        assert now == res.counters, (i, now, res.counters)
        assert now.num_self_repaired - state.num_self_repaired == int(res.repaired)
        if not res.repaired:
            keep = ~res.clipped_rows
            np.testing.assert_array_equal(bits(got[keep]), bits(od[keep]))
        repaired.append(res.repaired)
        state = res.counters
    assert repaired[:4] == [False, False, False, True]
    assert True in repaired[4:] and False in repaired[4:]
    assert state.num_backpropped == n and state.count == 8 * n
    comp.close()


def test_proportion_compared_in_basefloat(kctc, gpu, tmp_path):
    """clipped_proportion is a BaseFloat quotient (:995-996): (float)1 / 100 is
    the float nearest 0.01, the default threshold 0.01f itself, so one clipped
    row in a hundred is a tie and does not repair; two in a hundred do."""
    rows, dim = 8, 65
    cfg = ClipCfg(cr.THRESHOLD, True, 0.01, 0.0, 1.0)
    od, iv = cr.make_deriv(rows, dim, 17, clip_pattern=[False] * rows), cr.make_in_value(rows, dim, 17)
    seed, draws = seed_where(lambda d: d[0] <= 0.5, 1)
    for num_clipped, expect in ((1, False), (2, True)):
        comp = make_comp(kctc, tmp_path, dim, cfg, num_clipped, 92)
        comp.srand(seed)
        res = cr.clip_backprop(od, iv, cfg, None, Counters(num_clipped, 92, 0, 0), draws[0], to_update_is_self=True)
        assert res.drew and res.repaired == expect
        got = backprop(comp, gpu, od, iv, comp)
        assert counters(comp, tmp_path) == res.counters
        check_deriv(got, res, f"proportion {num_clipped}/100")
        if not expect:
            np.testing.assert_array_equal(bits(got), bits(od))
        comp.close()


@pytest.mark.parametrize("way", ["scale0", "threshold1", "zero_count_other"])
def test_draw_accounting(kctc, gpu, tmp_path, way):
    """A Backprop whose gate fails before RandUniform() (self-repair-scale=0,
    repair threshold >= 1, count_ == 0) consumes no draw.  The handle's stream
    shows only in a later gated Backprop of the same handle, which the first
    two settings never reach (they are fixed per component): there the calls
    must never repair, and a network of such components must leave the
    trainer's counted stream untouched over two train steps.  With zero counts and to_update another
    component the handle's own count stays 0; the gated Backprop that follows
    (to_update = itself) must decide by draw number 1."""
    rows, dim = 7, 65
    od, iv = cr.make_deriv(rows, dim, 19, clip_pattern=[True] * rows), cr.make_in_value(rows, dim, 19)
    seed, draws = seed_where(lambda d: d[0] <= 0.5 and min(d[1:4]) > 0.5, 4)
    if way != "zero_count_other":
        cfg = ClipCfg(cr.THRESHOLD, True, 0.05, 0.0, 0.0) if way == "scale0" else \
            ClipCfg(cr.THRESHOLD, True, 1.0, 0.0, 1.0)
        comp = make_comp(kctc, tmp_path, dim, cfg, 64, 64)
        comp.srand(seed)
        state = Counters(64, 64, 0, 0)
        for _ in range(3):
            res = cr.clip_backprop(od, iv, cfg, None, state, draws[0], to_update_is_self=True)
            assert not res.drew and not res.repaired
            got = backprop(comp, gpu, od, iv, comp)
            assert rel_err(got, res.deriv) < TOL
            state = res.counters
            assert counters(comp, tmp_path) == state
        comp.close()
        # the same Backprop inside a network draws from the trainer's stream, whose calls are
        # counted: every row clips (threshold 0.02), and still nothing is drawn
        import torch
        extra = "self-repair-scale=0" if way == "scale0" else "self-repair-clipped-proportion-threshold=1.0"
        T, N, D, A = 24, 3, 16, 9
        lines = kctc.recipe_config(num_rnn=2, input_dim=D, hidden=32, num_targets=A, learning_rate=0.01,
                                   param_stddev=0.2, clipping_threshold=0.02).splitlines()
        net = kctc.Nnet("\n".join(l + " " + extra if l.startswith("ClipGradientComponent") else l
                                  for l in lines) + "\n", seed=11)
        feats, nf, fl, ll = kctc.synth_minibatch(5, T, N, D, A, 0.2)
        for _ in range(2):
            net.train_step(torch.from_numpy(feats).to(gpu), T, N, nf, fl, ll)
        assert net.rand_calls == 0
        for c in (2, 4):
            num_clipped, count = net.clip_stats(c)
            assert count == 2 * T * N and num_clipped > 0.5 * count     # (rows past an utterance's end are zero)
        net.close()
        return
    cfg = ClipCfg(cr.THRESHOLD, True, 0.05, 0.5, 1.0)
    comp = make_comp(kctc, tmp_path, dim, cfg)
    holder = comp.Copy()
    comp.srand(seed)
    state = cr.ZERO
    for _ in range(3):
        res = cr.clip_backprop(od, iv, cfg, (0, 0), state, draws[0])
        assert not res.drew and not res.repaired
        got = backprop(comp, gpu, od, iv, holder)
        assert rel_err(got, res.deriv) < TOL
        state = res.counters
        assert counters(holder, tmp_path) == state and counters(comp, tmp_path) == cr.ZERO
    res = cr.clip_backprop(od, iv, cfg, None, cr.ZERO, draws[0], to_update_is_self=True)
    assert res.drew and res.repaired        # draw 1 repairs, draws 2 .. 4 would not
    got = backprop(comp, gpu, od, iv, comp)
    check_deriv(got, res, "draw accounting")
    assert counters(comp, tmp_path) == res.counters
    comp.close()
    holder.close()


@pytest.mark.parametrize("own_clipped", [True, False], ids=["own-clipped", "holder-clipped"])
def test_to_update_is_a_copy(kctc, gpu, tmp_path, own_clipped):
    """The gradient-holder pattern: to_update is another component.  It
    receives the counters (NumSelfRepaired included), the backpropped
    component's own stay, and the repair decision uses the backpropped
    component's own proportion, not the holder's."""
    rows, dim = 8, 65
    cfg = ClipCfg(cr.THRESHOLD, True, 0.25, 0.5, 1.0)
    all_clip = cr.make_deriv(rows, dim, 23, clip_pattern=[True] * rows)
    no_clip = cr.make_deriv(rows, dim, 24, clip_pattern=[False] * rows)
    iv = cr.make_in_value(rows, dim, 23)
    seed, draws = seed_where(lambda d: max(d[:3]) <= 0.5, 3)
    comp = make_comp(kctc, tmp_path, dim, cfg)
    comp.srand(seed)
    own = cr.ZERO
    # prime the component itself: two calls with to_update = itself
    for i in range(2):
        od = all_clip if own_clipped else no_clip
        res = cr.clip_backprop(od, iv, cfg, None, own, draws[i], to_update_is_self=True)
        backprop(comp, gpu, od, iv, comp)
        own = res.counters
        assert counters(comp, tmp_path) == own
    # the holder: proportion 0 (fresh) against an own proportion of 1, or 1 against 0
    holder = make_comp(kctc, tmp_path, dim, cfg) if own_clipped else make_comp(kctc, tmp_path, dim, cfg, 16, 16)
    hstate = cr.ZERO if own_clipped else Counters(16, 16, 0, 0)
    od = no_clip if own_clipped else all_clip
    res = cr.clip_backprop(od, iv, cfg, (own.num_clipped, own.count), hstate, draws[2])
    assert res.drew and res.repaired == own_clipped
    got = backprop(comp, gpu, od, iv, holder)
    check_deriv(got, res, f"holder, own clipped {own_clipped}")
    assert counters(holder, tmp_path) == res.counters
    assert res.counters.num_self_repaired == hstate.num_self_repaired + int(own_clipped)
    assert counters(comp, tmp_path) == own
    comp.close()
    holder.close()


def test_zero_repair_matrix_and_zero_derivative(kctc, gpu, tmp_path):
    """Every |x| <= target: the repair matrix is zero and an active repair
    returns the clipped derivative to the bit.  out_deriv all zero with an
    active repair: all zero, finite."""
    rows, dim = 7, 65
    cfg = ClipCfg(cr.THRESHOLD, True, 0.05, 3.0, 1.0)
    seed, draws = seed_where(lambda d: max(d[:2]) <= 0.5, 2)
    od = cr.make_deriv(rows, dim, 29)
    iv = np.clip(cr.make_in_value(rows, dim, 29), -3.0, 3.0)
    assert (np.abs(iv) == 3.0).any()          # |x| == target is still zero
    plain = make_comp(kctc, tmp_path, dim, cfg)
    clipped_only = backprop(plain, gpu, od, iv, None)
    comp = make_comp(kctc, tmp_path, dim, cfg, *cr.PRIMED)
    comp.srand(seed)
    res = cr.clip_backprop(od, iv, cfg, None, Counters(*cr.PRIMED, 0, 0), draws[0], to_update_is_self=True)
    assert res.repaired
    got = backprop(comp, gpu, od, iv, comp)
    np.testing.assert_array_equal(bits(got), bits(clipped_only))
    assert rel_err(got, res.deriv) < TOL
    assert counters(comp, tmp_path) == res.counters and res.counters.num_self_repaired == 1
    zero = np.zeros((rows, dim), np.float32)
    iv2 = cr.make_in_value(rows, dim, 30)
    res2 = cr.clip_backprop(zero, iv2, cfg, None, res.counters, draws[1], to_update_is_self=True)
    assert res2.repaired and not res2.deriv.any()
    got = backprop(comp, gpu, zero, iv2, comp)
    assert np.isfinite(got).all() and not got.any()
    assert counters(comp, tmp_path) == res2.counters and res2.counters.num_self_repaired == 2
    comp.close()
    plain.close()


@pytest.mark.parametrize("rows,dim", [(1, 1), (7, 65), (64, 100), (1030, 63)])
def test_elementwise_mode(kctc, gpu, tmp_path, rows, dim):
    """norm-based-clipping=false, the component's default: np.clip to the bit
    (elements at +-threshold, -0.0 and +-inf included); the counters stay 0
    and no draw is consumed; with counters read from a model the repair fires
    on a draw <= 0.5 and matches the restatement."""
    thr = cr.THRESHOLD
    cfg = ClipCfg(thr, False, 0.25, 0.5, 1.0)
    od, iv = cr.elementwise_deriv(rows, dim, 5, thr), cr.make_in_value(rows, dim, 5)
    expect = np.clip(od, np.float32(-thr), np.float32(thr))
    seed, draws = seed_where(lambda d: d[0] <= 0.5 < d[1], 2)
    comp = kctc.Component(f"ClipGradientComponent dim={dim} clipping-threshold={thr} "
                          "self-repair-clipped-proportion-threshold=0.25 self-repair-target=0.5")
    assert "norm-based-clipping=false" in comp.Info()
    comp.srand(seed)
    for k, tu in enumerate((comp, None, comp)):
        got = backprop(comp, gpu, od, iv, tu, alias=(k == 2))
        np.testing.assert_array_equal(bits(got), bits(expect))
    assert counters(comp, tmp_path) == Counters(0, 0, 0, 2)
    # give the same handle counts: its next Backprop is gated and must use draw number 1
    donor = make_comp(kctc, tmp_path, dim, cfg, 30, 40)
    comp.Add(1.0, donor)
    assert counters(comp, tmp_path) == Counters(30, 40, 0, 2)
    res = cr.clip_backprop(od, iv, cfg, None, Counters(30, 40, 0, 2), draws[0], to_update_is_self=True)
    assert res.drew and res.repaired and res.counters == Counters(30, 40, 1, 3)
    got = backprop(comp, gpu, od, iv, comp)
    check_deriv(got, res, f"element-wise repair {rows}x{dim}")
    assert counters(comp, tmp_path) == res.counters
    # ... and draw number 2 (> 0.5) leaves the clamp alone
    got = backprop(comp, gpu, od, iv, comp)
    np.testing.assert_array_equal(bits(got), bits(expect))
    assert counters(comp, tmp_path) == Counters(30, 40, 1, 4)
    # the model read from text behaves the same
    donor.srand(seed)
    got = backprop(donor, gpu, od, iv, donor)
    res = cr.clip_backprop(od, iv, cfg, None, Counters(30, 40, 0, 0), draws[0], to_update_is_self=True)
    check_deriv(got, res, f"element-wise repair, read model {rows}x{dim}")
    assert counters(donor, tmp_path) == res.counters
    comp.close()
    donor.close()


def test_scale_and_add_move_the_counters(kctc, gpu, tmp_path):
    """ClipGradientComponent::Scale / Add (:1064-1073) act on num_clipped and
    count, and the next Backprop's repair decision follows the new counts:
    (8, 16) would repair after 8 unclipped rows (8/24); halved to (4, 8) the
    same call is the tie 4/16; with (12, 12) added it is 16/28."""
    rows, dim = 8, 65
    cfg = ClipCfg(cr.THRESHOLD, True, 0.25, 0.5, 1.0)
    od, iv = cr.make_deriv(rows, dim, 37, clip_pattern=[False] * rows), cr.make_in_value(rows, dim, 37)
    seed, draws = seed_where(lambda d: max(d[:2]) <= 0.5, 2)
    ctl = cr.clip_backprop(od, iv, cfg, None, Counters(8, 16, 0, 0), draws[0], to_update_is_self=True)
    assert ctl.repaired
    comp = make_comp(kctc, tmp_path, dim, cfg, 8, 16)
    comp.srand(seed)
    comp.Scale(0.5)
    assert counters(comp, tmp_path) == Counters(4, 8, 0, 0) and proportion(comp) == 0.5
    res = cr.clip_backprop(od, iv, cfg, None, Counters(4, 8, 0, 0), draws[0], to_update_is_self=True)
    assert res.drew and not res.repaired
    got = backprop(comp, gpu, od, iv, comp)
    np.testing.assert_array_equal(bits(got), bits(od))
    assert counters(comp, tmp_path) == res.counters == Counters(4, 16, 0, 1)
    other = make_comp(kctc, tmp_path, dim, cfg, 12, 12)
    comp.Add(1.0, other)
    assert counters(comp, tmp_path) == Counters(16, 28, 0, 1) and counters(other, tmp_path) == Counters(12, 12, 0, 0)
    res = cr.clip_backprop(od, iv, cfg, None, Counters(16, 28, 0, 1), draws[1], to_update_is_self=True)
    assert res.repaired
    got = backprop(comp, gpu, od, iv, comp)
    check_deriv(got, res, "after Scale and Add")
    assert counters(comp, tmp_path) == res.counters == Counters(16, 36, 1, 2)
    comp.close()
    other.close()
