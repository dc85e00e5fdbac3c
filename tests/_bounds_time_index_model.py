"""The box AND time pruning of the chunk index, restated in numpy (include/pcq.h, pcq_scan_dev_indexed_bounds_time).

A chunk is 4096 consecutive points; the ragged tail behind the last whole chunk has no state.  Its box state comes from the
integer AABB of its positions against the inclusive box [lo, hi], its time state from _time_index_model.chunk_state, and the two
combine as box AND class combines its parts:

  NONE  either part is NONE
  ALL   both parts are ALL
  SCAN  everything else
"""
import numpy as np

import _time_index_model as tm

CHUNK = tm.CHUNK
SCAN, NONE, ALL = tm.SCAN, tm.NONE, tm.ALL


def box_state(xyz, lo, hi):
    """State of ONE chunk's positions (int32, n x 3) against the inclusive integer box [lo, hi]."""
    p = np.asarray(xyz).astype(np.int64)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    mn, mx = p.min(axis=0), p.max(axis=0)
    if np.any(lo > hi) or np.any(mx < lo) or np.any(mn > hi):
        return NONE
    return ALL if np.all(mn >= lo) and np.all(mx <= hi) else SCAN


def combined(b, t):
    if NONE in (b, t):
        return NONE
    return ALL if b == ALL and t == ALL else SCAN


def pairs(xyz, t, lo, hi, start, end):
    """[(box state, time state)] of the whole chunks."""
    return [(box_state(xyz[CHUNK * c: CHUNK * (c + 1)], lo, hi), tm.chunk_state(t[CHUNK * c: CHUNK * (c + 1)], start, end))
            for c in range(len(t) // CHUNK)]


def states(xyz, t, lo, hi, start, end):
    return [combined(b, s) for b, s in pairs(xyz, t, lo, hi, start, end)]


def classify(xyz, t, lo, hi, start, end):
    """(skipped, whole, scanned) of a pruned scan over the whole chunks."""
    s = states(xyz, t, lo, hi, start, end)
    return s.count(NONE), s.count(ALL), s.count(SCAN)


def select(xyz, t, lo, hi, start, end):
    """The matches: inside the inclusive box AND Range<f64>::contains (NaN -> False)."""
    x = np.asarray(xyz).astype(np.int64)
    box = np.all((x >= np.asarray(lo, dtype=np.int64)) & (x <= np.asarray(hi, dtype=np.int64)), axis=1)
    with np.errstate(invalid="ignore"):
        return box & (t >= start) & (t < end)
