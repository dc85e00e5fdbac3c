"""The chunk index beyond one trip of its loops, and at random: the model of the chunk states, the two big sets and the random draw.

Restated from adhoc-queries-pointclouds_amd/csrc (test_index_chunks_plan.py reads the constants back out of the sources):
  chunks        chunk_index.hip:43-45 (16 tiles of 256 points = 4096; class chunks of 65536), index_plan.h:18, :63-65 (whole chunks
                of boxes and time records, every class chunk, the last one partial)
  grid          chunk_index.hip:595-596: min(chunks, CUs x 8) workgroups; every builder and every pruned count walks
                `for (ch = blockIdx.x; ch < nchunks; ch += gridDim.x)`
  class count   chunk_index.hip:300-312: ONE block of 256 threads striding over the class chunks
  emit stats    chunk_index.hip:520-521: min(ceil(chunks / 256), CUs) blocks of 256 threads
  states        pcq_internal.h:220-248 (index_box_state, index_class_state, index_time_state, index_combined_state)
  plan          index_plan.h:31-60: what each kind prunes with, what the parts cover, which predicates fall through

The model.  A chunk's state comes from its records alone: the integer AABB of its 4096 positions against the inclusive i64 box (a
box that is empty after the clamp to the i32 range matches nothing), one histogram bin against the chunk's point count, {min, max
of the non-NaN times, NaN count} against [t0, t1) in IEEE compares, and the combination of two parts.  `classify` counts the states
in the kind's own unit (class chunks for CLASS, 4096-point chunks otherwise), `select` is the per-point truth over ALL points, the
ragged tail included.  Both read the finished arrays; nothing is derived from how the data was constructed.  `Model` takes three
deliberate mistakes as switches, so that the plan test can show that the random set would notice them.

The big set, for a device of `cus` CUs: C = 2 * 8 * cus + 37 whole chunks and a tail of 1234 points.  Every workgroup of the index's
grid (8 * cus) makes two trips round its chunk loop and 37 make three: the smallest count at which a stride that is wrong only
from its second application on can change an answer (2 * grid + 1), with 37 workgroups rather than one on the third trip.  Chunk
c's contents are its own: its x values fill the slab [64 s, 64 s + 63] with s = c * 1009 mod C (so that a box's x interval picks
chunks out of all three trips), y and z are random in [0, 999]; its times lie in [10 c, 10 c + 9.5], with one NaN in the chunks
c = 3 mod 7 and nothing but NaNs in the chunks c = 5 mod 11 short of the last; class chunk k holds class 7 alone (k = 0 mod 3), a mix without it
(1 mod 3) or a mix with it (2 mod 3), and class 33 at every 1000th byte of the mixes.  The extremes of every chunk and the classes
of its first bytes are planted, so that BigPlan can state every chunk's records and two known points per chunk from sizes alone:
the plan test proves the conditions on the queries for 64, 256 and 304 CUs from that, and proves on the real 64-CU arrays that the
stated records are the measured ones.  The tail shares the slab of chunk C - 1.

The class-only set: 8 * cus + 37 whole class chunks and one of 12345 bytes.  k_index_build_class makes a second trip in 37 (38 with
the partial chunk) workgroups and k_index_count_class's 256 threads make nine strides at 256 CUs.  A third trip of the builder
would double the upload for a loop whose body does not depend on the trip: it is left out.

The random draw: 1 to 40 whole chunks and a tail, every chunk of a kind of its own per column, queries with faces taken from the
drawn chunks' own records.  draw(seed) is a pure function of BASE + PCQ_TEST_SEED_BASE + seed.
"""
import functools
import math
import os
from collections import namedtuple

import numpy as np

CHUNK = 4096
CLASS_CHUNK = 65536
EMIT_TILE = 2048
GRID_PER_CU = 8          # workgroups per CU of the index's grid
COUNT_CLASS_BLOCK = 256  # threads of k_index_count_class's one block
STATS_BLOCK = 256        # threads per block of k_index_emit_stats
SCAN, NONE, ALL = 0, 1, 2
STATES = (NONE, ALL, SCAN)
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
FULL = ([I32_MIN] * 3, [I32_MAX] * 3)
KINDS = ("bounds", "class", "bounds_class", "time", "bounds_time")
TIME_KINDS = ("time", "bounds_time")
SCALE, OFFSET = (0.01, 0.02, 0.5), (10.0, -20.0, 3.0)
INF = float("inf")

# index_plan.h restated: parts, unit, the building call counts on its way, a count comes from the histograms, live predicates only
Plan = namedtuple("Plan", "parts unit counts_on_build from_hist live_only")
PLANS = {"bounds": Plan(("boxes",), CHUNK, True, False, False), "class": Plan(("hist",), CLASS_CHUNK, True, True, False),
         "bounds_class": Plan(("boxes", "hist"), CHUNK, False, False, False), "time": Plan(("times",), CHUNK, True, False, False),
         "bounds_time": Plan(("boxes", "times"), CHUNK, False, False, True)}

# One query.  `upto` / `cls_stride`: the columns it is asked of (None: all n points, packed); `buffer`: sent to a buffer collector too.
Query = namedtuple("Query", "kind name lo hi cls t0 t1 buffer upto cls_stride")


def Q(kind, name, lo=None, hi=None, cls=None, t0=None, t1=None, buffer=False, upto=None, cls_stride=None):
    if kind in ("bounds", "bounds_class", "bounds_time"):
        lo, hi = [int(v) for v in lo], [int(v) for v in hi]
    return Query(kind, name, lo, hi, None if cls is None else int(cls), None if t0 is None else float(t0), None if t1 is None else float(t1),
                 buffer, upto, cls_stride)


def chunks_of(kind, n):
    """index_chunks of the kind's unit"""
    return (n + CLASS_CHUNK - 1) // CLASS_CHUNK if kind == "class" else n // CHUNK


def grid_of(cus, chunks, per_cu=GRID_PER_CU):
    return min(chunks, cus * per_cu)


def stats_blocks(cus, chunks):
    return min((chunks + STATS_BLOCK - 1) // STATS_BLOCK, cus)


def clamped(lo, hi):
    """The box after the clamp to the i32 range, or None where it is empty then (pcq_make_dev_pred)"""
    lo, hi = [max(int(v), I32_MIN) for v in lo], [min(int(v), I32_MAX) for v in hi]
    return None if any(a > b for a, b in zip(lo, hi)) else (lo, hi)


def live(q):
    """False: a predicate that can match nothing by its own values (an empty box; an empty or NaN range)"""
    if q.lo is not None and clamped(q.lo, q.hi) is None:
        return False
    return q.t0 is None or q.t0 < q.t1


def covered(q, n, aligned=True):
    """index_covers restated for packed columns at the alignments the tests upload them with, and the plan's live_only"""
    pl = PLANS[q.kind]
    m = n if q.upto is None else q.upto
    ok = aligned
    if "boxes" in pl.parts or "times" in pl.parts:
        ok = ok and m >= CHUNK
    if "hist" in pl.parts:
        ok = ok and m > 0 and (q.cls_stride or 1) == 1
    if "times" in pl.parts:
        ok = ok and (q.cls_stride or 8) == 8
    return ok and not (pl.live_only and not live(q))


# ---------------------------------------------------------------------------------------------------------------------------------
# records and states
# ---------------------------------------------------------------------------------------------------------------------------------
class Data:
    """Columns of n points (any of them None) with their chunk records, measured once"""

    def __init__(self, xyz=None, cls=None, t=None):
        self.xyz, self.cls, self.t = xyz, cls, t
        self.n = len(next(a for a in (xyz, cls, t) if a is not None))
        self._bins = {}

    def prefix(self, m):
        return Data(*(None if a is None else a[:m] for a in (self.xyz, self.cls, self.t)))

    @functools.cached_property
    def boxes(self):
        """(mn, mx), each [chunks, 3] in int64"""
        c = self.n // CHUNK
        p = self.xyz[:c * CHUNK].reshape(c, CHUNK, 3)
        return p.min(axis=1).astype(np.int64), p.max(axis=1).astype(np.int64)

    @functools.cached_property
    def times(self):
        """(mn, mx, nans) per chunk: the extremes over the non-NaN times, +inf / -inf where a chunk has none"""
        c = self.n // CHUNK
        t = self.t[:c * CHUNK].reshape(c, CHUNK)
        nan = np.isnan(t)
        return np.where(nan, np.inf, t).min(axis=1), np.where(nan, -np.inf, t).max(axis=1), nan.sum(axis=1)

    def class_points(self):
        cc = chunks_of("class", self.n)
        return np.minimum(CLASS_CHUNK, self.n - CLASS_CHUNK * np.arange(cc, dtype=np.int64))

    def bins(self, c):
        """The histogram bin of class c per class chunk"""
        if c not in self._bins:
            whole = self.n // CLASS_CHUNK
            b = np.count_nonzero(self.cls[:whole * CLASS_CHUNK].reshape(whole, CLASS_CHUNK) == c, axis=1).astype(np.int64)
            if self.n % CLASS_CHUNK:
                b = np.append(b, np.count_nonzero(self.cls[whole * CLASS_CHUNK:] == c))
            self._bins[c] = b
        return self._bins[c]


class Model:
    """pcq_internal.h:220-248 on arrays of records.  The switches are deliberate mistakes (test_index_chunks_plan.py)."""

    def __init__(self, open_face=None, ignore_nans=False, ignore_partial=False):
        self.open_face, self.ignore_nans, self.ignore_partial = open_face, ignore_nans, ignore_partial

    def box(self, mn, mx, lo, hi):
        box = clamped(lo, hi)
        if box is None:
            return np.full(len(mn), NONE)
        lo, hi = np.asarray(box[0], dtype=np.int64), np.asarray(box[1], dtype=np.int64)
        if self.open_face is not None:  # the mistake: the upper face of one axis exclusive
            hi = hi.copy()
            hi[self.open_face] -= 1
        disjoint = ((mx < lo) | (mn > hi)).any(axis=1)
        inside = ((mn >= lo) & (mx <= hi)).all(axis=1)
        return np.where(disjoint, NONE, np.where(inside, ALL, SCAN))

    def time(self, mn, mx, nans, t0, t1):
        if not t0 < t1:
            return np.full(len(mn), NONE)
        if self.ignore_nans:  # the mistake
            nans = np.zeros_like(nans)
        none = (nans == CHUNK) | (mx < t0) | (mn >= t1)
        whole = (nans == 0) & (mn >= t0) & (mx < t1)
        return np.where(none, NONE, np.where(whole, ALL, SCAN))

    def cls(self, bins, points):
        if self.ignore_partial:  # the mistake
            points = np.full(len(points), CLASS_CHUNK)
        return np.where(bins == 0, NONE, np.where(bins == points, ALL, SCAN))

    @staticmethod
    def combined(a, b):
        return np.where((a == NONE) | (b == NONE), NONE, np.where((a == ALL) & (b == ALL), ALL, SCAN))

    def states(self, q, rec):
        """rec: an object with boxes, times, bins(c), class_points() (Data, BigPlan)"""
        if q.kind == "class":
            return self.cls(rec.bins(q.cls), rec.class_points())
        if q.kind == "time":
            return self.time(*rec.times, q.t0, q.t1)
        b = self.box(*rec.boxes, q.lo, q.hi)
        if q.kind == "bounds":
            return b
        if q.kind == "bounds_time":
            return self.combined(b, self.time(*rec.times, q.t0, q.t1))
        k = self.cls(rec.bins(q.cls), rec.class_points())
        return self.combined(b, k[np.arange(len(b)) // (CLASS_CHUNK // CHUNK)])


TRUE = Model()


def counts3(states):
    """(skipped, whole, scanned)"""
    return tuple(int(np.count_nonzero(states == s)) for s in STATES)


def classify(kind, data, q, model=TRUE):
    assert q.kind == kind
    return counts3(model.states(q, data))


def in_box(xyz, lo, hi):
    box = clamped(lo, hi)
    if box is None:
        return np.zeros(len(xyz), dtype=bool)
    sel = np.ones(len(xyz), dtype=bool)
    for a in range(3):  # (the clamped faces are i32 values: the compares are on the stored integers)
        v = xyz[:, a]
        sel &= (v >= np.int32(box[0][a])) & (v <= np.int32(box[1][a]))
    return sel


def in_range(t, t0, t1):
    """Range<f64>::contains: a NaN anywhere gives False"""
    with np.errstate(invalid="ignore"):
        return (t >= t0) & (t < t1)


def select(kind, data, q):
    """The matches among ALL points of data, per point"""
    assert q.kind == kind
    if kind == "class":
        return data.cls == q.cls
    if kind == "time":
        return in_range(data.t, q.t0, q.t1)
    sel = in_box(data.xyz, q.lo, q.hi)
    if kind == "bounds_class":
        sel &= data.cls == q.cls
    if kind == "bounds_time":
        sel &= in_range(data.t, q.t0, q.t1)
    return sel


def expect_records(kind, xyz, cls, sel, point_dtype):
    """The buffer collector's records in file order: x * scale + offset (unfused), the class byte (a time record has none), no colour"""
    idx = np.flatnonzero(sel)
    out = np.zeros(len(idx), dtype=point_dtype)
    for a, k in enumerate("xyz"):
        out[k] = xyz[idx, a].astype(np.float64) * SCALE[a] + OFFSET[a]
    if kind not in TIME_KINDS:
        out["classification"] = cls[idx]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the big set
# ---------------------------------------------------------------------------------------------------------------------------------
SLAB = 64
TAIL = 1234
YZ = 1000
RARE, RARE_EVERY = 33, 1000
ABSENT = 77
MIX = {1: (1, 2, 9, 1), 2: (1, 7, 2, 9)}  # the classes of a mixed class chunk of type k % 3, as its first bytes hold them
BIG_SEED = 4111


def class_type_bins(types, points, c):
    """A histogram bin per class chunk that has the state the construction gives class c there (its value only where it is 0 or all)"""
    if c == 7:
        return np.where(types == 0, points, np.where(types == 1, 0, 1))
    if c in (1, 2, 9, RARE):
        return np.where(types == 0, 0, 1)
    return np.zeros(len(types), dtype=np.int64)


class BigPlan:
    """Sizes, every chunk's records and two known points per chunk, from `cus` alone"""

    def __init__(self, cus, per_cu=GRID_PER_CU, halve=False):
        self.cus = cus
        self.grid = cus * per_cu                       # what the widest index launch has, if the set has that many chunks
        self.C = C = 2 * GRID_PER_CU * cus + 37        # (the set does not follow `per_cu`: that is the mutation)
        if halve:
            self.C = C = C // 2
        self.n = C * CHUNK + TAIL
        self.class_chunks = chunks_of("class", self.n)
        mult = next(m for m in (1009, 1013, 1019, 1021) if math.gcd(m, C) == 1)
        c = np.arange(C + 1, dtype=np.int64)           # (index C: the tail)
        self.slab = (c * mult) % C
        self.slab[C] = self.slab[C - 1]
        x0 = SLAB * self.slab
        self.boxes = (np.stack([x0[:C], np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)], axis=1),
                      np.stack([x0[:C] + SLAB - 1, np.full(C, YZ - 1), np.full(C, YZ - 1)], axis=1))
        self.all_nan = (c % 11 == 5) & (c < C - 1)       # (never the last chunk: its times are queried)
        self.one_nan = (c % 7 == 3) & ~self.all_nan & (c < C)
        self.times = (np.where(self.all_nan[:C], np.inf, 10.0 * c[:C]), np.where(self.all_nan[:C], -np.inf, 10.0 * c[:C] + 9.5),
                      np.where(self.all_nan[:C], CHUNK, self.one_nan[:C].astype(np.int64)))
        self.class_types = np.arange(self.class_chunks) % 3
        # the two known points of chunk c: local indices 0 and 1
        self.kx = np.stack([np.stack([x0, np.zeros(C + 1, dtype=np.int64), np.zeros(C + 1, dtype=np.int64)], axis=1),
                            np.stack([x0 + SLAB - 1, np.full(C + 1, YZ - 1), np.full(C + 1, YZ - 1)], axis=1)], axis=1)   # [C + 1, 2, 3]
        self.kt = np.stack([10.0 * c, 10.0 * c + 9.5], axis=1)
        self.kt[self.all_nan] = np.nan
        ktype = self.class_types[(c * CHUNK) // CLASS_CHUNK]
        self.kc = np.stack([np.where(ktype == 0, 7, 1), np.where(ktype == 0, 7, np.where(ktype == 1, 2, 7))], axis=1)

    def class_points(self):
        return np.minimum(CLASS_CHUNK, self.n - CLASS_CHUNK * np.arange(self.class_chunks, dtype=np.int64))

    def bins(self, c):
        return class_type_bins(self.class_types, self.class_points(), c)

    def known_matches(self, q):
        """[C + 1, 2]: whether the known points of each chunk (the tail last) match"""
        sel = np.ones((self.C + 1, 2), dtype=bool)
        if q.lo is not None:
            box = clamped(q.lo, q.hi)
            sel &= False if box is None else ((self.kx >= np.asarray(box[0])) & (self.kx <= np.asarray(box[1]))).all(axis=2)
        if q.cls is not None:
            sel &= self.kc == q.cls
        if q.t0 is not None:
            sel &= in_range(self.kt, q.t0, q.t1)
        return sel

    def trip(self, chunk):
        return chunk // self.grid


@functools.lru_cache(maxsize=None)
def big_plan(cus):
    return BigPlan(cus)


def plant_classes(cls, types, n):
    """Class 33 at every 1000th byte of the mixed class chunks, then the mix's classes at the first bytes of every 4096 points"""
    i = np.arange(7, n, RARE_EVERY)
    i = i[types[i // CLASS_CHUNK] != 0]
    cls[i] = RARE
    starts = np.arange(0, n, CHUNK)
    st = types[starts // CLASS_CHUNK]
    for ty, mix in MIX.items():
        for j, v in enumerate(mix):
            at = starts[st == ty] + j
            cls[at[at < n]] = v


def mixed_classes(rng, types_per_byte_chunk, n):
    """n class bytes: per 65536, class 7 alone, a mix without it or a mix with it, by the chunk's type"""
    cls = rng.integers(0, 4, n, dtype=np.uint8)
    out = np.empty(n, dtype=np.uint8)
    lut = {0: np.full(4, 7, dtype=np.uint8), 1: np.asarray(MIX[1], dtype=np.uint8), 2: np.asarray(MIX[2], dtype=np.uint8)}
    whole = n // CLASS_CHUNK
    a, b = cls[:whole * CLASS_CHUNK].reshape(whole, CLASS_CHUNK), out[:whole * CLASS_CHUNK].reshape(whole, CLASS_CHUNK)
    for ty in (0, 1, 2):
        rows = types_per_byte_chunk[:whole] == ty
        b[rows] = lut[ty][a[rows]]
    if n % CLASS_CHUNK:
        out[whole * CLASS_CHUNK:] = lut[int(types_per_byte_chunk[whole])][cls[whole * CLASS_CHUNK:]]
    plant_classes(out, types_per_byte_chunk, n)
    return out


@functools.lru_cache(maxsize=1)
def big_data(cus):
    p = big_plan(cus)
    C, n = p.C, p.n
    rng = np.random.default_rng(BIG_SEED)
    per = np.minimum(np.arange(n) // CHUNK, C)          # the chunk of every point, the tail as chunk C
    xyz = np.empty((n, 3), dtype=np.int32)
    xyz[:, 0] = SLAB * p.slab[per] + rng.integers(0, SLAB, n)
    xyz[:, 1] = rng.integers(0, YZ, n)
    xyz[:, 2] = rng.integers(0, YZ, n)
    t = 10.0 * per + rng.uniform(0.0, 9.5, n)
    starts = np.arange(C + 1) * CHUNK
    for j in (0, 1):
        xyz[starts + j] = p.kx[:, j]
        t[starts + j] = 10.0 * np.arange(C + 1) + (0.0, 9.5)[j]
    t[starts[:C][p.one_nan[:C]] + 2] = np.nan
    t[np.repeat(p.all_nan[:C], CHUNK).nonzero()[0]] = np.nan
    cls = mixed_classes(rng, p.class_types, n)
    return Data(xyz, cls, t)


def x_slabs(a, b, cut=0):
    """The x interval of the slabs a .. b; `cut` moves both faces into their slabs"""
    return SLAB * a + cut, SLAB * b + SLAB - 1 - cut


def big_queries(kind, p):
    """The fixed queries of a kind for the set of plan p"""
    C = p.C
    s1 = int(p.slab[C - 1])
    w = max(1, (3 * C) // 400)                              # a window of about 1.5 % of the slabs around chunk C - 1's (and the tail's)
    na, nb = max(0, s1 - w), min(C - 1, s1 + w)
    wide, wide2, narrow = x_slabs(C // 5, C // 2, cut=10), x_slabs(C // 10, C // 2), x_slabs(na, nb)
    top = I32_MAX

    def box(xr, yhi=top):
        return [xr[0], I32_MIN, I32_MIN], [xr[1], yhi, top]

    c_last = int(p.kc[C - 1, 0])                            # the class of chunk C - 1's first point
    c_tail = int(p.kc[C, 0])
    t_wide = (10.0 * (3 * C // 10) + 3.0, 10.0 * (C - 10) + 7.0)       # NONE, SCAN and ALL chunks on the third trip too
    t_late = (10.0 * (C - 1 - w) + 3.0, 10.0 * C + 5.0)     # the last chunks and the start of the tail
    t_late2 = (10.0 * (C - 1 - w), 10.0 * C + 0.5)
    if kind == "bounds":
        return [Q(kind, "wide", *box(wide)), Q(kind, "wide_lower_y", *box(wide2, 499)), Q(kind, "narrow", *box(narrow), buffer=True),
                Q(kind, "narrow_lower_y", *box(narrow, 499), buffer=True), Q(kind, "everything", *FULL),
                Q(kind, "nothing", [SLAB * (C + 5), 0, 0], [SLAB * (C + 9), YZ, YZ], buffer=True)]
    if kind == "class":
        return [Q(kind, "fills_chunks", cls=7), Q(kind, "mixed", cls=1), Q(kind, "rare", cls=RARE, buffer=True), Q(kind, "absent", cls=ABSENT, buffer=True),
                Q(kind, "mixed9", cls=9), Q(kind, "zero", cls=0)]
    if kind == "bounds_class":
        return [Q(kind, "wide_7", *box(wide), cls=7), Q(kind, "wide_lower_y_1", *box(wide2, 499), cls=1),
                Q(kind, "narrow_last", *box(narrow), cls=c_last, buffer=True), Q(kind, "narrow_lower_y_tail", *box(narrow, 499), cls=c_tail, buffer=True),
                Q(kind, "everything_7", *FULL, cls=7), Q(kind, "wide_absent", *box(wide), cls=ABSENT, buffer=True)]
    if kind == "time":
        return [Q(kind, "wide", t0=t_wide[0], t1=t_wide[1]), Q(kind, "late", t0=t_late[0], t1=t_late[1], buffer=True),
                Q(kind, "late_whole", t0=t_late2[0], t1=t_late2[1], buffer=True), Q(kind, "everything", t0=-INF, t1=INF),
                Q(kind, "from_the_middle", t0=10.0 * (C // 2) + 9.5, t1=INF), Q(kind, "nothing", t0=-5.0, t1=0.0, buffer=True)]
    assert kind == "bounds_time"
    return [Q(kind, "wide_wide", *box(wide), t0=t_wide[0], t1=t_wide[1]), Q(kind, "lower_y_wide", *box(wide2, 499), t0=t_wide[0], t1=t_wide[1]),
            Q(kind, "lower_y_late", *box((I32_MIN, top), 499), t0=t_late[0], t1=t_late[1], buffer=True),
            Q(kind, "narrow_everywhen", *box(narrow), t0=-INF, t1=INF, buffer=True), Q(kind, "everything", *FULL, t0=-INF, t1=INF),
            Q(kind, "wide_before", *box(wide), t0=-5.0, t1=0.0, buffer=True)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the big class-only set
# ---------------------------------------------------------------------------------------------------------------------------------
CLASS_ONLY_REST = 12345


class ClassOnlyPlan:
    def __init__(self, cus, per_cu=GRID_PER_CU, halve=False):
        self.cus = cus
        self.grid = cus * per_cu
        whole = GRID_PER_CU * cus + 37
        if halve:
            whole //= 2
        self.n = whole * CLASS_CHUNK + CLASS_ONLY_REST
        self.C = self.class_chunks = whole + 1
        self.class_types = np.arange(self.class_chunks) % 3

    def class_points(self):
        return np.minimum(CLASS_CHUNK, self.n - CLASS_CHUNK * np.arange(self.class_chunks, dtype=np.int64))

    def bins(self, c):
        return class_type_bins(self.class_types, self.class_points(), c)

    def trip(self, chunk):
        return chunk // self.grid


@functools.lru_cache(maxsize=None)
def class_only_plan(cus):
    return ClassOnlyPlan(cus)


def class_only_data(cus):
    p = class_only_plan(cus)
    return Data(cls=mixed_classes(np.random.default_rng(BIG_SEED + 1), p.class_types, p.n))


def class_only_queries():
    return [Q("class", "mixed", cls=1), Q("class", "absent", cls=ABSENT), Q("class", "fills_chunks", cls=7), Q("class", "rare", cls=RARE, buffer=True)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the random draw
# ---------------------------------------------------------------------------------------------------------------------------------
BASE = 76000
SEED_BASE = int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
SEEDS = range(32)
TAILS = (0, 1, 63, 2047, 2048, 2049, 4095)
POS_KINDS = ("slab", "full", "identical", "limits")
TIME_CHUNK_KINDS = ("ramp", "constant", "one_nan", "all_nan", "infs", "zeros")
CLASS_POOL = np.asarray([0, 1, 2, 6, 9, 200, 255], dtype=np.uint8)  # (77 is never drawn)

Case = namedtuple("Case", "seed n data pos_kinds time_kinds class_kinds queries order")


def draw_positions(rng, kind, m):
    if kind == "full":
        return rng.integers(I32_MIN, I32_MAX + 1, (m, 3)).astype(np.int32)
    if kind == "identical":
        return np.tile(rng.integers(-60000, 60000, 3), (m, 1)).astype(np.int32)
    base, width = int(rng.integers(-50000, 50000)), int(rng.integers(1, 200))
    p = np.stack([base + rng.integers(0, width, m), rng.integers(-1000, 1000, m), rng.integers(-1000, 1000, m)], axis=1).astype(np.int32)
    if kind == "limits":
        for v in (I32_MIN, I32_MAX):
            p[rng.integers(0, m), rng.integers(0, 3)] = v
    return p


def draw_times(rng, kind, m):
    if kind == "all_nan":
        return np.full(m, np.nan)
    if kind == "constant":
        return np.full(m, float(rng.integers(0, 100000)) / 8)
    if kind == "zeros":
        return rng.choice(np.asarray([-0.0, 0.0, 5e-324, -5e-324]), m)
    t = float(rng.integers(0, 100000)) + np.arange(m) * float(rng.choice([0.001, 0.125, 1.0]))
    if kind == "one_nan":
        t[rng.integers(0, m)] = np.nan
    if kind == "infs":
        for v in ((np.inf,), (-np.inf,), (np.inf, -np.inf))[int(rng.integers(0, 3))]:
            t[rng.integers(0, m)] = v
    return t


def pieces(n):
    """(first, count) of the whole chunks and the tail"""
    return [(a, min(CHUNK, n - a)) for a in range(0, n, CHUNK)]


def draw(seed):
    rng = np.random.default_rng(BASE + SEED_BASE + seed)
    n = int(rng.integers(1, 41)) * CHUNK + int(rng.choice(TAILS))
    pk, tk, xs, ts = [], [], [], []
    for first, m in pieces(n):
        pk.append(str(rng.choice(POS_KINDS, p=[0.4, 0.2, 0.2, 0.2])))
        tk.append(str(rng.choice(TIME_CHUNK_KINDS, p=[0.35, 0.13, 0.13, 0.13, 0.13, 0.13])))
        xs.append(draw_positions(rng, pk[-1], m))
        ts.append(draw_times(rng, tk[-1], m))
    cls, ck = np.empty(n, dtype=np.uint8), []
    for first in range(0, n, CLASS_CHUNK):
        m = min(CLASS_CHUNK, n - first)
        ck.append(str(rng.choice(["single", "mixed"])))
        members = rng.choice(CLASS_POOL, 1 if ck[-1] == "single" else int(rng.integers(2, 5)), replace=False)
        cls[first:first + m] = rng.choice(members, m)
    data = Data(np.ascontiguousarray(np.concatenate(xs)), cls, np.concatenate(ts))
    queries = {kind: draw_queries(rng, kind, data, seed) for kind in KINDS}
    return Case(seed, n, data, pk, tk, ck, queries, [str(k) for k in rng.permutation(KINDS)])


def box_faces(rng, data, limit_free=False):
    """Boxes with faces from the records of one drawn chunk: its AABB; lo = mx on one axis (touching), lo = mx + 1, hi = mx - 1.
    limit_free: an axis whose mx + 1 is still an i32 value (so that no box is emptied by the clamp)"""
    mn, mx = data.boxes
    c = int(rng.integers(0, len(mn)))
    a = int(rng.integers(0, 3))
    if limit_free and mx[c, a] == I32_MAX:
        free = [(cc, aa) for cc in range(len(mn)) for aa in range(3) if mx[cc, aa] < I32_MAX and mx[cc, aa] > I32_MIN]
        c, a = free[int(rng.integers(0, len(free)))]
    lo, hi = [int(v) for v in mn[c]], [int(v) for v in mx[c]]

    def one(face, v):
        b = [list(FULL[0]), list(FULL[1])]
        b[face][a] = v
        return b

    return {"aabb": [lo, hi], "touching": one(0, hi[a]), "beyond": one(0, hi[a] + 1), "short": one(1, hi[a] - 1)}


def random_box(rng, data):
    i, j = rng.integers(0, data.n, 2)
    p = data.xyz[[i, j]].astype(np.int64)
    return [int(v) for v in p.min(axis=0) - rng.integers(0, 500, 3)], [int(v) for v in p.max(axis=0) + rng.integers(0, 500, 3)]


def time_faces(rng, data, strict=False):
    """Ranges with bounds from the records of one drawn chunk (one with a non-NaN time, where there is one).  strict: a chunk
    with finite mn < mx (so that none of the ranges but start_is_end and nan_bound is empty), or [0, 1] where there is none"""
    mn, mx, nans = data.times
    some = np.flatnonzero(np.isfinite(mn) & np.isfinite(mx) & (mn < mx)) if strict else np.flatnonzero(nans < CHUNK)
    c = int(rng.choice(some)) if len(some) else 0
    a, b = (float(mn[c]), float(mx[c])) if len(some) or not strict else (0.0, 1.0)
    return {"mn_mx": (a, b), "mn_above_mx": (a, float(np.nextafter(b, np.inf))), "from_mx": (b, INF), "start_is_end": (a, a),
            "nan_bound": (float("nan"), b) if rng.integers(0, 2) else (a, float("nan")), "whole_line": (-INF, INF), "before_mn": (-INF, a),
            "zeros": (-0.0, 5e-324)}


def random_range(rng, data):
    finite = data.t[np.isfinite(data.t)]
    v = float(rng.choice(finite)) if len(finite) else 0.0
    return v - float(rng.choice([0.25, 3.0, 1000.0])), v + float(rng.choice([0.25, 3.0, 1000.0]))


def class_choices(rng, data):
    """(a class that fills a class chunk, or the first point's; one that no point has; one of a random point)"""
    full = [int(data.cls[f]) for f in range(0, data.n, CLASS_CHUNK) if np.all(data.cls[f:f + CLASS_CHUNK] == data.cls[f])]
    return (full[int(rng.integers(0, len(full)))] if full else int(data.cls[0])), ABSENT, int(data.cls[rng.integers(0, data.n)])


def draw_queries(rng, kind, data, seed):
    """About eight covered queries and exactly one that the plan sends to the plain scan (the last)"""
    n = data.n
    if kind in ("bounds", "bounds_class", "bounds_time"):
        f = box_faces(rng, data, limit_free=kind == "bounds_time")
        rb = random_box(rng, data)
        lo_above_hi = [f["aabb"][0], [f["aabb"][0][0] - 1] + f["aabb"][1][1:]]
        by_clamp = [[2 ** 31, I32_MIN, I32_MIN], [2 ** 40, I32_MAX, I32_MAX]]
    if kind in TIME_KINDS:
        r = time_faces(rng, data, strict=kind == "bounds_time")
        rr = random_range(rng, data)
    if kind in ("class", "bounds_class"):
        c_full, c_absent, c_some = class_choices(rng, data)
    if kind == "bounds":
        qs = [Q(kind, name, *f[name], buffer=True) for name in ("aabb", "touching", "beyond", "short")]
        qs += [Q(kind, "full", *FULL, buffer=True), Q(kind, "lo_above_hi", *lo_above_hi, buffer=True), Q(kind, "emptied_by_clamp", *by_clamp, buffer=True),
               Q(kind, "random", *rb, buffer=True), Q(kind, "no_whole_chunk", *rb, buffer=True, upto=CHUNK - 1)]
    elif kind == "time":
        qs = [Q(kind, name, t0=r[name][0], t1=r[name][1], buffer=True) for name in r]
        qs += [Q(kind, "random", t0=rr[0], t1=rr[1], buffer=True), Q(kind, "no_whole_chunk", t0=-INF, t1=INF, buffer=True, upto=CHUNK - 1)]
    elif kind == "class":
        qs = [Q(kind, name, cls=c, buffer=True) for name, c in (("fills_a_chunk", c_full), ("absent", c_absent), ("zero", 0), ("last", 255), ("some", c_some))]
        qs.append(Q(kind, "every_second_byte", cls=c_some, buffer=True, upto=n // 2, cls_stride=2))
    elif kind == "bounds_class":
        qs = [Q(kind, "aabb_full", *f["aabb"], cls=c_full, buffer=True), Q(kind, "touching_some", *f["touching"], cls=c_some, buffer=True),
              Q(kind, "beyond_some", *f["beyond"], cls=c_some, buffer=True), Q(kind, "short_full", *f["short"], cls=c_full, buffer=True),
              Q(kind, "full_zero", *FULL, cls=0, buffer=True), Q(kind, "full_full", *FULL, cls=c_full, buffer=True),
              Q(kind, "lo_above_hi_some", *lo_above_hi, cls=c_some, buffer=True), Q(kind, "random_last", *rb, cls=255, buffer=True),
              Q(kind, "random_absent", *rb, cls=c_absent, buffer=True), Q(kind, "no_whole_chunk", *FULL, cls=c_some, buffer=True, upto=CHUNK - 1)]
    else:
        qs = [Q(kind, "aabb_mn_mx", *f["aabb"], t0=r["mn_mx"][0], t1=r["mn_mx"][1], buffer=True),
              Q(kind, "aabb_mn_above_mx", *f["aabb"], t0=r["mn_above_mx"][0], t1=r["mn_above_mx"][1], buffer=True),
              Q(kind, "touching_whole_line", *f["touching"], t0=-INF, t1=INF, buffer=True),
              Q(kind, "beyond_whole_line", *f["beyond"], t0=-INF, t1=INF, buffer=True),
              Q(kind, "short_from_mx", *f["short"], t0=r["from_mx"][0], t1=r["from_mx"][1], buffer=True),
              Q(kind, "full_whole_line", *FULL, t0=-INF, t1=INF, buffer=True), Q(kind, "full_before_mn", *FULL, t0=r["before_mn"][0], t1=r["before_mn"][1], buffer=True),
              Q(kind, "random_random", *rb, t0=rr[0], t1=rr[1], buffer=True), Q(kind, "full_zeros", *FULL, t0=r["zeros"][0], t1=r["zeros"][1], buffer=True)]
        dead = [Q(kind, "dead_lo_above_hi", *lo_above_hi, t0=-INF, t1=INF, buffer=True), Q(kind, "dead_by_clamp", *by_clamp, t0=rr[0], t1=rr[1], buffer=True),
                Q(kind, "dead_start_is_end", *FULL, t0=r["start_is_end"][0], t1=r["start_is_end"][1], buffer=True),
                Q(kind, "dead_nan_bound", *FULL, t0=r["nan_bound"][0], t1=r["nan_bound"][1], buffer=True)]
        qs.append(dead[seed % 4])
    return qs


@functools.lru_cache(maxsize=None)
def case(seed):
    return draw(seed)


def columns_of(q, data):
    """The Data a query is asked of: all points, a prefix, or every second class byte of a prefix"""
    if q.upto is None:
        return data
    if q.cls_stride == 2:
        return Data(data.xyz[:q.upto], np.ascontiguousarray(data.cls[:2 * q.upto:2]), None)
    return data.prefix(q.upto)


# ---------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------------------
def expected_stats(q, data, parts_built, count):
    """pcq_index_stats of a covered scan of `data` (include/pcq.h), and the parts it leaves built: the call that builds a
    one-part kind's part reads every chunk; a class count is answered from the histograms; everything else is classified"""
    pl = PLANS[q.kind]
    chunks = chunks_of(q.kind, data.n)
    missing = [p for p in pl.parts if p not in parts_built]
    parts_built.update(pl.parts)
    if pl.counts_on_build and missing:
        return dict(chunks=chunks, skipped=0, whole=0, scanned=chunks, built=1)
    if count and pl.from_hist:
        return dict(chunks=chunks, skipped=0, whole=chunks, scanned=0, built=0)
    s, w, r = classify(q.kind, data, q)
    return dict(chunks=chunks, skipped=s, whole=w, scanned=r, built=1 if missing else 0)


def predicate(P, q):
    """binding.Predicate of a query"""
    return {"bounds": lambda: P.bounds(q.lo, q.hi), "class": lambda: P.classification(q.cls), "bounds_class": lambda: P.bounds_class(q.lo, q.hi, q.cls),
            "time": lambda: P.time_range(q.t0, q.t1), "bounds_time": lambda: P.bounds_time(q.lo, q.hi, q.t0, q.t1)}[q.kind]()


def columns(binding, kind, d_xyz, d_cls, d_t, n, cls_stride=None):
    """The kind's columns over device copies of the positions, the class bytes and the times"""
    if kind in TIME_KINDS:
        return binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=SCALE, offset=OFFSET)
    return binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, cls_stride=cls_stride or 1, scale=SCALE, offset=OFFSET)


def indexed_entry(ctx, kind):
    return {"bounds": ctx.scan_dev_indexed, "class": ctx.scan_dev_indexed, "bounds_class": ctx.scan_dev_indexed_combined,
            "time": ctx.scan_dev_indexed_time, "bounds_time": ctx.scan_dev_indexed_bounds_time}[kind]


def count_of(ctx, kind, cols, pred, ix=None):
    """The count of one scan into a fresh count collector: through the kind's indexed entry, or (ix None) by pcq_scan_dev"""
    cc = ctx.count_collector()
    try:
        if ix is None:
            ctx.scan_dev(cols, pred, cc)
        else:
            indexed_entry(ctx, kind)(cols, pred, ix, cc)
        return cc.point_count()
    finally:
        cc.free()
