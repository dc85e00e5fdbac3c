"""The time part of the chunk index, restated in numpy (include/pcq.h, pcq_scan_dev_indexed_time).

A chunk is 4096 consecutive times; the ragged tail behind the last whole chunk has no state.  The state of a chunk against
[start, end) is taken from three numbers alone — the minimum and the maximum of its non-NaN times and the number of its NaNs —
with IEEE float64 compares, as Range<f64>::contains compares:

  NONE  the range is empty (start >= end, or a NaN bound), or the chunk has no non-NaN time, or max < start, or min >= end
  ALL   the chunk has no NaN, and min >= start, and max < end
  SCAN  everything else
"""
import numpy as np

CHUNK = 4096
SCAN, NONE, ALL = 0, 1, 2


def chunk_state(t, start, end):
    """State of ONE chunk's times (float64) against [start, end)."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if not (start < end):  # start >= end, or either bound NaN
            return NONE
        ok = t[~np.isnan(t)]
        if ok.size == 0:
            return NONE
        mn, mx = ok.min(), ok.max()
        if mx < start or mn >= end:
            return NONE
        if ok.size == t.size and mn >= start and mx < end:
            return ALL
        return SCAN


def states(t, start, end):
    return [chunk_state(t[CHUNK * c: CHUNK * (c + 1)], start, end) for c in range(len(t) // CHUNK)]


def classify(t, start, end):
    """(skipped, whole, scanned) of a pruned scan over the whole chunks of t."""
    s = states(t, start, end)
    return s.count(NONE), s.count(ALL), s.count(SCAN)
