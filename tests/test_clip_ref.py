"""tests/clip_ref.py checked on the host: a hand-worked example, two invariants
of the reference algorithm, and -- for every input set the GPU tests use -- the
fp32 restatement of the reference within the GPU tolerance of the fp64 one, so
that the tolerance is one a correct fp32 implementation reaches."""
import math

import numpy as np
import pytest

import clip_ref as cr
from clip_ref import ClipCfg, Counters
from conftest import rel_err

GPU_TOL = 2e-6      # tests/test_clipgrad_gpu.py, tests/test_elementwise_gpu.py


def test_hand_worked_3x2():
    """threshold 5, repair threshold 0.5, target 1, scale 1; to_update = this
    with (num_clipped, count) = (1, 1) before the call."""
    cfg = ClipCfg(5.0, True, 0.5, 1.0, 1.0)
    out_deriv = np.array([[3, 4], [6, 8], [0.75, 1.0]], np.float32)
    in_value = np.array([[2, -1], [0, 3], [-4, 0.5]], np.float32)
    # scaled squared norms 25/25 = 1 (a tie: clipped, factor 1), 100/25 = 4 (factor 1/2), 1.5625/25 (kept)
    clipped = np.array([[3, 4], [3, 4], [0.75, 1.0]])
    # counters: 2 rows clipped of 3 -> (3, 4): proportion 0.75 > 0.5
    # repair = max(|x| - 1, 0) * (x > 0 ? 1 : -1); x = 0 has sign -1 and magnitude 0
    repair = np.array([[1, -0.0], [-0.0, 2], [-3, 0.0]])
    dn = 5 + 5 + 1.25                       # sum of the clipped rows' norms
    rn = 1 + 2 + 3
    magnitude = 1.0 * 0.75 * (dn / 3)       # 2.8125
    scale = magnitude / (rn / 3)            # 1.40625
    assert (magnitude, scale) == (2.8125, 1.40625)
    added = clipped + (-scale / 0.5) * repair
    np.testing.assert_array_equal(added, [[0.1875, 4], [3, -1.625], [9.1875, 1.0]])
    dn2 = math.sqrt(0.1875 ** 2 + 16) + math.sqrt(9 + 1.625 ** 2) + math.sqrt(9.1875 ** 2 + 1)
    expect = added * (dn / dn2)

    r = cr.clip_backprop(out_deriv, in_value, cfg, None, Counters(1, 1, 0, 0), 0.5, to_update_is_self=True)
    assert r.drew and r.repaired                      # a draw of exactly 0.5 is not > 0.5
    assert r.counters == Counters(3, 4, 1, 1)
    assert list(r.clipped_rows) == [True, True, False]
    np.testing.assert_allclose(r.deriv, expect, rtol=1e-14, atol=0)
    r32 = cr.clip_backprop(out_deriv, in_value, cfg, None, Counters(1, 1, 0, 0), 0.5, dtype=np.float32,
                           to_update_is_self=True)
    assert r32.deriv.dtype == np.float32 and r32.counters == r.counters
    np.testing.assert_allclose(r32.deriv, expect, rtol=5e-7, atol=0)

    # the gate, in the reference's order
    none = cr.clip_backprop(out_deriv, in_value, cfg, (9, 9), None, 0.1)
    assert none.counters is None and not none.drew and not none.repaired
    np.testing.assert_array_equal(none.deriv, clipped)
    above = cr.clip_backprop(out_deriv, in_value, cfg, None, Counters(1, 1, 0, 0), 0.5000001, to_update_is_self=True)
    assert above.drew and not above.repaired and above.counters == Counters(3, 4, 0, 1)
    for c in (cfg._replace(repair_threshold=1.0), cfg._replace(repair_scale=0.0)):
        r = cr.clip_backprop(out_deriv, in_value, c, None, Counters(1, 1, 0, 0), 0.1, to_update_is_self=True)
        assert not r.drew and not r.repaired and r.counters == Counters(3, 4, 0, 1)
    # count_ is the backpropped component's own: zero here, whatever to_update holds
    other = cr.clip_backprop(out_deriv, in_value, cfg, (0, 0), Counters(5, 5, 0, 0), 0.1)
    assert not other.drew and other.counters == Counters(7, 8, 0, 1)
    # a tie of the proportion: (1 + 2) / (3 + 3) = 0.5 <= 0.5
    tie = cr.clip_backprop(out_deriv, in_value, cfg, None, Counters(1, 3, 0, 0), 0.1, to_update_is_self=True)
    assert tie.drew and not tie.repaired
    # ... and in BaseFloat: 1 / 100 is the float nearest 0.01, which is the threshold 0.01f
    c01 = cfg._replace(repair_threshold=0.01)
    for dt in (np.float32, np.float64):
        r = cr.clip_backprop(out_deriv[2:], in_value[2:], c01, None, Counters(1, 99, 0, 0), 0.1, dtype=dt,
                             to_update_is_self=True)
        assert r.drew and not r.repaired
    # element-wise mode: a clamp, counters untouched, no draw while count_ == 0
    e = cr.clip_backprop(out_deriv, in_value, cfg._replace(norm_based=False), None, cr.ZERO, 0.1,
                         to_update_is_self=True)
    np.testing.assert_array_equal(e.deriv, [[3, 4], [5, 5], [0.75, 1.0]])
    assert e.counters == Counters(0, 0, 0, 1) and not e.drew


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_invariants(dtype):
    tol = 1e-6 if dtype == np.float32 else 1e-13
    for name, rows, dim, cfg, od, iv in cr.repair_cases():
        plain = cr.clip_backprop(od, iv, cfg, cr.PRIMED, None, 0.25, dtype=dtype)
        rep = cr.clip_backprop(od, iv, cfg, None, Counters(*cr.PRIMED, 0, 0), 0.25, dtype=dtype,
                               to_update_is_self=True)
        assert rep.repaired, name
        before = np.linalg.norm(plain.deriv.astype(np.float64), axis=1).sum()
        after = np.linalg.norm(rep.deriv.astype(np.float64), axis=1).sum()
        assert abs(after - before) <= tol * before, (name, before, after)
        # rows below the threshold, no repair: unchanged to the bit
        keep = ~plain.clipped_rows
        np.testing.assert_array_equal(plain.deriv[keep], od.astype(dtype)[keep])
        t = cr.tie_row_of(rows)
        if t is not None:
            assert plain.clipped_rows[t]
            np.testing.assert_array_equal(plain.deriv[t], od[t])


def _both(od, iv, cfg, own, upd, draw, is_self):
    r64 = cr.clip_backprop(od, iv, cfg, own, upd, draw, to_update_is_self=is_self)
    r32 = cr.clip_backprop(od, iv, cfg, own, upd, draw, dtype=np.float32, to_update_is_self=is_self)
    assert (r32.counters, r32.drew, r32.repaired) == (r64.counters, r64.drew, r64.repaired)
    np.testing.assert_array_equal(r32.clipped_rows, r64.clipped_rows)
    return r64, max(rel_err(r32.deriv, r64.deriv), cr.row_rel_err(r32.deriv, r64.deriv))


def test_fp32_restatement_within_gpu_tolerance():
    worst = 0.0
    for name, rows, dim, cfg, od, iv in cr.repair_cases():
        r, e = _both(od, iv, cfg, None, Counters(*cr.PRIMED, 0, 0), 0.25, True)
        assert r.repaired and e < GPU_TOL, (name, e)
        worst = max(worst, e)
        r, e = _both(od, iv, cfg._replace(repair_scale=0.0), None, cr.ZERO, 0.25, True)
        assert not r.repaired and e < GPU_TOL, (name, e)
        worst = max(worst, e)
    state = cr.ZERO
    for i, (od, iv) in enumerate(cr.sequence_inputs()):
        r, e = _both(od, iv, cr.SEQ_CFG, None, state, 0.25, True)
        assert int(r.clipped_rows.sum()) == cr.SEQ_CLIPS[i]
        assert r.repaired == (i >= 3), i          # 0, 4/16 (tie), 5/24, then above 0.25
        assert e < GPU_TOL, (i, e)
        worst = max(worst, e)
        state = r.counters
    assert state == Counters(sum(cr.SEQ_CLIPS), 8 * len(cr.SEQ_CLIPS), len(cr.SEQ_CLIPS) - 3, len(cr.SEQ_CLIPS))
    # element-wise mode with counters read from a model
    cfg = ClipCfg(cr.THRESHOLD, False, 0.25, 0.5, 1.0)
    for rows, dim in ((7, 65), (64, 100)):
        od = cr.elementwise_deriv(rows, dim, 5, cr.THRESHOLD)
        r, e = _both(od, cr.make_in_value(rows, dim, 5), cfg, None, Counters(30, 40, 0, 0), 0.25, True)
        assert r.repaired and np.isfinite(r.deriv).all() and e < GPU_TOL, e
        worst = max(worst, e)
    print(f"fp32 restatement vs fp64: worst error {worst:.2e}")
    assert worst > 0       # the two are different computations
