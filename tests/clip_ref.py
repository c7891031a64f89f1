"""ClipGradientComponent::Backprop + RepairGradients restated in numpy
(TEST INFRASTRUCTURE), and the inputs the clip tests share.

clip_backprop() follows src/nnet2/nnet-cudnn-component.cc:921-1055 operation
by operation.  dtype=float64 is the oracle; dtype=float32 restates the
reference's own arithmetic: the matrices, the row sums of squares and every
element-wise step in fp32; CuVector::Sum() accumulates in double and returns
BaseFloat; clipped_proportion and magnitude are BaseFloat; AddMat / Scale
take their factor as BaseFloat.

The discrete parts are the same in both dtypes and are the reference's:
  * the gate short-circuits (threshold >= 1 || scale == 0 || count_ == 0 ||
    RandUniform() > 0.5), so a draw is consumed only when the first three
    conditions are false; count_ is the backpropped component's own, and it
    already holds this minibatch when to_update == this in norm-based mode;
  * clipped_proportion = static_cast<BaseFloat>(num_clipped_) / count_ is a
    BaseFloat quotient and is compared with the BaseFloat threshold by <=
    (no repair on a tie; 1 / 100 against 0.01 is a tie in BaseFloat);
  * a row is clipped when its scaled squared norm is not < 1 (ApplyFloor(1.0)
    counts the others);
  * element-wise mode never touches num_clipped or count.
"""
from collections import namedtuple

import numpy as np

ClipCfg = namedtuple("ClipCfg", "threshold norm_based repair_threshold repair_target repair_scale")
Counters = namedtuple("Counters", "num_clipped count num_self_repaired num_backpropped")
ClipResult = namedtuple("ClipResult", "deriv counters drew repaired clipped_rows")

ZERO = Counters(0, 0, 0, 0)
f32 = np.float32


def config_line(dim, cfg):
    return (f"ClipGradientComponent dim={dim} clipping-threshold={cfg.threshold!r} "
            f"norm-based-clipping={'true' if cfg.norm_based else 'false'} "
            f"self-repair-clipped-proportion-threshold={cfg.repair_threshold!r} "
            f"self-repair-target={cfg.repair_target!r} self-repair-scale={cfg.repair_scale!r}")


def _row_norms(m, dt):
    """AddDiagMat2(1.0, M, kNoTrans, 0.0) + ApplyPow(0.5), then Sum()."""
    v = np.sqrt(np.sum(m * m, axis=1, dtype=dt)).astype(dt)
    s = np.sum(v, dtype=np.float64)
    return float(f32(s)) if dt == np.float32 else float(s)


def clip_backprop(out_deriv, in_value, cfg, own, to_update, draw, dtype=np.float64, to_update_is_self=False):
    """One Backprop of a component with settings `cfg`.

    own: (num_clipped, count) of the backpropped component before the call
    (ignored when to_update_is_self: they are to_update's); to_update: the
    Counters of the to_update component, or None; draw: the RandUniform()
    value this call would consume.  -> ClipResult(in_deriv, to_update's new
    Counters or None, drew, repaired, mask of the clipped rows)."""
    dt = np.dtype(dtype).type
    d = np.array(out_deriv, dtype=f32).astype(dt)           # in_deriv->CopyFromMat(out_deriv)
    x = np.asarray(in_value, dtype=f32).astype(dt)
    rows = d.shape[0]
    thr = f32(cfg.threshold)
    clipped = np.zeros(rows, dtype=bool)
    upd = to_update
    if to_update_is_self:
        own = (to_update.num_clipped, to_update.count)
    if not thr > 0:
        return ClipResult(d, upd, False, False, clipped)
    if cfg.norm_based:
        alpha = dt(float(thr) ** -2.0)                        # pow(clipping_threshold_, -2) as Real
        scales = (alpha * np.sum(d * d, axis=1, dtype=dt)).astype(dt)
        clipped = ~(scales < 1)                               # ApplyFloor(1.0) floors the others
        scales = np.where(clipped, scales, dt(1))
        if clipped.any():
            scales = np.power(scales, dt(-0.5)).astype(dt)    # ApplyPow(-0.5)
            d = (d * scales[:, None]).astype(dt)              # MulRowsVec
            if upd is not None:
                upd = upd._replace(num_clipped=upd.num_clipped + int(clipped.sum()))
        if upd is not None:
            upd = upd._replace(count=upd.count + rows)
            if to_update_is_self:
                own = (upd.num_clipped, upd.count)
    else:
        d = np.maximum(np.minimum(d, dt(thr)), dt(-thr))      # ApplyCeiling, ApplyFloor
    if upd is None:
        return ClipResult(d, None, False, False, clipped)
    upd = upd._replace(num_backpropped=upd.num_backpropped + 1)

    # ---- RepairGradients ----
    num_clipped, count = own
    if f32(cfg.repair_threshold) >= 1.0 or f32(cfg.repair_scale) == 0.0 or count == 0:
        return ClipResult(d, upd, False, False, clipped)
    if f32(draw) > f32(0.5):
        return ClipResult(d, upd, True, False, clipped)
    prop32 = f32(num_clipped) / f32(count) if count > 0 else f32(0)
    if prop32 <= f32(cfg.repair_threshold):
        return ClipResult(d, upd, True, False, clipped)
    upd = upd._replace(num_self_repaired=upd.num_self_repaired + 1)
    sign = np.where(x > 0, dt(1), dt(-1))                     # ApplyHeaviside * 2 - 1
    repair = (np.maximum(np.abs(x) - dt(f32(cfg.repair_target)), dt(0)) * sign).astype(dt)
    dn = _row_norms(d, dt)
    rn = _row_norms(repair, dt)
    if dt == np.float32:
        magnitude = float(f32(float(f32(cfg.repair_scale) * prop32) * (dn / rows)))
    else:
        magnitude = float(f32(cfg.repair_scale)) * (num_clipped / count) * (dn / rows)
    scale = magnitude / (rn / rows) if rn != 0.0 else 0.0
    d = (d + dt(-scale / 0.5) * repair).astype(dt)            # AddMat(-scale / repair_probability, .)
    dn2 = _row_norms(d, dt)
    if dn2 != 0.0:
        d = (d * dt(dn / dn2)).astype(dt)                     # Scale
    return ClipResult(d, upd, True, True, clipped)


# ---------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------
# (rows, dim): dim below one wave; dim % 4 != 0 (scalar path); dim / 4 = 65 (a
# lane's second trip of the vector loop); the recipe width; rows % 4 in
# {0, 1, 2, 3}; several hundred row blocks
SHAPES = [(1, 1), (3, 3), (4, 63), (5, 64), (7, 65), (64, 100), (33, 256), (6, 260), (32, 1024), (1030, 63)]
THRESHOLD = 4.0            # a power of two: the tie row [4, 0, ...] has ss / thr^2 == 1 exactly
NORM_FACTORS = (0.25, 0.5, 2.0, 8.0)


def make_deriv(rows, dim, seed, threshold=THRESHOLD, clip_pattern=None, tie_row=None):
    """out_deriv [rows, dim] float32: every row a random direction scaled to a
    norm from NORM_FACTORS x threshold (so none is within 1e-3 relative of
    the threshold); clip_pattern[r] picks above (True) / below (False) the
    threshold for row r; tie_row (an index) becomes [threshold, 0, ...]."""
    rng = np.random.default_rng([seed, rows, dim])
    v = rng.standard_normal((rows, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if clip_pattern is None:
        fac = rng.choice(NORM_FACTORS, size=rows)
    else:
        fac = np.where(np.asarray(clip_pattern, dtype=bool), rng.choice(NORM_FACTORS[2:], size=rows),
                       rng.choice(NORM_FACTORS[:2], size=rows))
    d = (v * (fac * threshold)[:, None]).astype(f32)
    if tie_row is not None:
        d[tie_row] = 0
        d[tie_row, 0] = threshold
    return d


def make_in_value(rows, dim, seed):
    return (2.0 * np.random.default_rng([seed, rows, dim, 7]).standard_normal((rows, dim))).astype(f32)


def tie_row_of(rows):
    """The row that holds the exact tie in the shape-list inputs (None: too few rows)."""
    return 1 if rows >= 3 else None


REPAIR_SETTINGS = [(0.0, 1.0), (0.5, 1.0), (3.0, 1.0), (0.0, 0.25), (0.5, 0.25), (3.0, 0.25)]   # (target, scale)
PRIMED = (64, 64)          # (num_clipped, count) a component is read with: proportion 1 before the call
REPAIR_THRESHOLD = 0.05


def repair_cases():
    """The single-call active-repair cases: every shape with a setting from
    REPAIR_SETTINGS in turn, and every setting at 7 x 65.
    -> (id, rows, dim, ClipCfg, out_deriv, in_value)"""
    todo = [(s, REPAIR_SETTINGS[i % len(REPAIR_SETTINGS)]) for i, s in enumerate(SHAPES)]
    todo += [((7, 65), rs) for rs in REPAIR_SETTINGS if ((7, 65), rs) not in todo]
    out = []
    for (rows, dim), (target, scale) in todo:
        cfg = ClipCfg(THRESHOLD, True, REPAIR_THRESHOLD, target, scale)
        out.append((f"{rows}x{dim}-t{target}-s{scale}", rows, dim, cfg,
                    make_deriv(rows, dim, 31, tie_row=tie_row_of(rows)), make_in_value(rows, dim, 31)))
    return out


SEQ_DIM = 65
SEQ_CLIPS = (0, 4, 1, 8, 8, 8, 8, 8)    # rows clipped per call, 8 rows each: proportions 0, 4/16 (tie), 5/24, 13/32, ...
SEQ_CFG = ClipCfg(THRESHOLD, True, 0.25, 0.5, 1.0)


def sequence_inputs():
    """-> [(out_deriv, in_value)] of the calls of the counter-sequence test."""
    out = []
    for i, k in enumerate(SEQ_CLIPS):
        pattern = [r < k for r in range(8)]
        out.append((make_deriv(8, SEQ_DIM, 100 + i, clip_pattern=pattern), make_in_value(8, SEQ_DIM, 100 + i)))
    return out


def elementwise_deriv(rows, dim, seed, threshold):
    """Element-wise mode input: N(0, threshold^2) with elements exactly at
    +-threshold, -0.0, +0.0 and +-inf planted."""
    rng = np.random.default_rng([seed, rows, dim, 3])
    d = (threshold * rng.standard_normal((rows, dim))).astype(f32).ravel()
    special = [threshold, -threshold, -0.0, 0.0, np.inf, -np.inf, np.nextafter(f32(threshold), f32(np.inf)),
               np.nextafter(f32(threshold), f32(0))]
    idx = rng.permutation(d.size)[:len(special)]
    for i, s in zip(idx, special[:d.size]):
        d[i] = s
    return d.reshape(rows, dim)


def row_rel_err(got, ref):
    """max over rows of |got_r - ref_r| / |ref_r| (rows with |ref_r| = 0: the absolute error)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref, axis=1)
    err = np.linalg.norm(got - ref, axis=1) / np.where(den > 0, den, 1.0)
    return float(err.max()) if err.size else 0.0
