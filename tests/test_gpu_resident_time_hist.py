"""host/resident.cpp: when was this box scanned, from one pass over a dataset kept in HBM.
pcq_query_resident_count_bounds_by_time must give, for every bin b of the caller's edge table, what
pcq_query_resident_count_bounds_time gives for [edges[b], edges[b + 1]) — zeros included — with the same points_scanned.

Six small LAST files with time blocks, written by tests/_resident_files.py (images of tests/_time_images.py):
formats 1 and 6 (whose time blocks lie at n*20 and n*22 behind the point data's start) and 3; 3*4096+17, 4096, 100, 0, 513 and
2*4096+5 points; differing scales and offsets; one file far from the others, whose header misses the boxes of the others.  Times
are uniform in [1000, 2000), sorted per file.  A handful of bins are also checked against the oracle's box AND time search, and all
of them against numpy on the stored integers.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _host  # noqa: E402
import _resident_files as rf  # noqa: E402
import _time_images as ti  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

PCQ_ERR_ARG, PCQ_ERR_PANIC = pkg.PCQ_ERR_ARG, pkg.PCQ_ERR_PANIC
COLOUR, TIME = pkg.PCQ_RESIDENT_COLOUR, pkg.PCQ_RESIDENT_TIME
BINS_MAX = 1024  # include/pcq.h: PCQ_TIME_BINS_MAX
ISO = (0.01, 0.01, 0.01)
# (format, points, scale, offset); ints are x, y in [-5000, 5000), z in [-1000, 1000)
FILES = [(1, 3 * 4096 + 17, ti.SCALE, ti.OFFSET),               # world x [50, 150), y [-300, -100), z [-42.5, 57.5); times at n*20
         (6, 4096, ISO, (0.0, 0.0, 0.0)),                        # x, y [-50, 50), z [-10, 10); times at n*22
         (3, 100, (0.001, 0.001, 0.001), (100.0, -200.0, 0.0)),  # x [95, 105), y [-205, -195), z [-1, 1)
         (1, 0, ISO, (0.0, 0.0, 0.0)),
         (6, 513, ti.SCALE, ti.OFFSET),                          # a whole step and one point
         (1, 2 * 4096 + 5, ISO, (5000.0, 0.0, 0.0))]             # x [4950, 5050): no box below but "every" and "far" meets it
FAR_FILE = 5
BIG = 1e6
BOXES = {"every": ((-BIG, -BIG, -BIG), (BIG, BIG, BIG)),                # meets every header
         "near": ((-200.0, -400.0, -100.0), (200.0, 100.0, 100.0)),      # every file but the far one, all their points
         "slab": ((100.003, -BIG, -BIG), (101.003, BIG, BIG)),           # a thin slab
         "far": ((4990.0, -20.0, -5.0), (5010.0, 20.0, 5.0)),            # the far file alone, some of its points
         "missed": ((500.003, -260.0, -30.0), (600.003, -140.0, 40.0))}  # every header misses it
INF, NAN = float("inf"), float("nan")
TABLES = {"ten": np.linspace(1000.0, 2000.0, 11),
          "one": np.asarray([1200.0, 1700.0]),
          "uneven": np.asarray([-INF, 1000.0, 1000.0, 1250.5, 1250.5, 1250.5, 1600.0, 1999.0, INF]),
          "inner": np.sort(np.random.default_rng(5).uniform(1100.0, 1900.0, 66))}


class Q:
    def __init__(self):
        self.lib = _host.lib()

    err = staticmethod(_host.err)
    load = staticmethod(_host.load)

    def one_range(self, r, box, start, end):
        m, s = C.c_uint64(7), C.c_uint64(7)
        rc = self.lib.pcq_query_resident_count_bounds_time(r, (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]), start, end, C.byref(m), C.byref(s))
        return rc, m.value, s.value

    def by_time(self, r, box, edges, sentinel=77, scanned=True):
        nbins = len(edges) - 1
        hist, s = (C.c_uint64 * (nbins + 4))(*[sentinel + c for c in range(nbins + 4)]), C.c_uint64(sentinel)
        rc = self.lib.pcq_query_resident_count_bounds_by_time(r, (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]),
                                                              (C.c_double * len(edges))(*edges), nbins, hist, C.byref(s) if scanned else None)
        assert list(hist)[nbins:] == [sentinel + c for c in range(nbins, nbins + 4)]  # no word beyond the bins
        return rc, list(hist)[:nbins], s.value


@pytest.fixture(scope="module")
def q():
    return Q()


def corpus(d):
    return rf.write_files(d, FILES, 970)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files, and per file what tests/_resident_files.py holds of it."""
    paths, held = corpus(tmp_path_factory.mktemp("resident_time_hist"))
    for (fmt, n, _, _), h in zip(FILES, held):
        assert ti.time_offset(fmt) == (22 if fmt >= 6 else 20)
        if n:  # the time block is where the loader looks for it
            at = (375 if fmt >= 6 else 227) + n * ti.time_offset(fmt)
            assert np.array_equal(np.frombuffer(h.image[at:at + 8 * n].tobytes(), dtype=np.float64), h.t)
    return paths, held


def meets(h, box):
    """The header early-out: the file's world AABB meets the box (inclusive)."""
    if not len(h.xyz):
        return False
    w = ti.world(h.xyz, h.scale, h.offset)
    return bool(np.all(w.min(axis=0) <= np.asarray(box[1])) and np.all(w.max(axis=0) >= np.asarray(box[0])))


def numpy_hist(held, box, edges):
    """Per bin, the stored integer coordinates inside the local box of pcq_box_to_local and e[b] <= t < e[b + 1], over the files
    whose headers meet the box"""
    out = np.zeros(len(edges) - 1, dtype=np.int64)
    for h in held:
        if not meets(h, box):
            continue
        lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
        x = h.xyz.astype(np.int64)
        sel = np.all((x >= np.asarray(lmin, dtype=np.int64)) & (x <= np.asarray(lmax, dtype=np.int64)), axis=1)
        out += np.asarray([int((sel & ti.select(h.t, edges[b], edges[b + 1])).sum()) for b in range(len(edges) - 1)])
    return out


@pytest.fixture(scope="module", params=[TIME, TIME | COLOUR], ids=["time", "time_and_colour"])
def dataset(request, q, files):
    r = q.load(files[0], request.param)
    yield r
    q.lib.pcq_query_resident_free(r)


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("name", list(BOXES))
def test_every_bin_is_the_box_and_time_count_of_its_range(q, files, dataset, name, table):
    _, held = files
    box, edges = BOXES[name], TABLES[table]
    rc, hist, scanned = q.by_time(dataset, box, edges)
    assert rc == 0, q.err()
    want_scanned = sum(len(h.xyz) for h in held if meets(h, box))
    for b in range(len(edges) - 1):
        rc, m, s = q.one_range(dataset, box, float(edges[b]), float(edges[b + 1]))
        assert rc == 0, q.err()
        assert hist[b] == m, (name, table, b, hist[b], m)
        assert s == scanned == want_scanned
    assert hist == numpy_hist(held, box, edges).tolist()
    n = [len(h.xyz) for h in held]
    if name == "every":
        assert scanned == sum(n)
        if table in ("ten", "uneven"):
            assert sum(hist) == sum(n)
    elif name == "near":
        assert scanned == sum(n) - n[FAR_FILE]
        if table in ("ten", "uneven"):
            assert sum(hist) == scanned
    elif name == "slab":
        assert 0 < sum(hist) < scanned
    elif name == "far":
        assert scanned == n[FAR_FILE] and 0 < sum(hist) < scanned
    else:
        assert scanned == 0 and sum(hist) == 0
    if table == "uneven":
        assert hist[1] == hist[3] == hist[4] == 0  # equal edges


def test_a_handful_of_bins_against_the_oracle(q, files, dataset, oracle):
    _, held = files
    box, edges = BOXES["slab"], TABLES["ten"]
    rc, hist, _ = q.by_time(dataset, box, edges)
    assert rc == 0, q.err()
    for b in (0, 3, 4, 9):
        c = oracle.count_collector()
        for h in held:
            if not len(h.xyz):
                continue
            assert oracle.search_bounds_time(h.image, "last", box[0], box[1], float(edges[b]), float(edges[b + 1]), c) == 0, oracle.err()
        assert c.point_count() == hist[b], b
        c.free()
    assert sum(hist[b] for b in (0, 3, 4, 9)) > 0


def test_more_bins_than_one_launch_holds(q, files, dataset):
    """PCQ_TIME_BINS_MAX + 3 bins: two groups, the second of three bins."""
    _, held = files
    nbins = BINS_MAX + 3
    edges = np.linspace(1000.0, 2000.0, nbins + 1)
    for name in ("near", "slab"):
        rc, hist, scanned = q.by_time(dataset, BOXES[name], edges)
        assert rc == 0, q.err()
        want = numpy_hist(held, BOXES[name], edges).tolist()
        assert hist == want and hist[-3:] == want[-3:] and hist[BINS_MAX - 1] == want[BINS_MAX - 1]
        if name == "near":  # (17 014 points over 1027 bins: the second group's three bins hold points; the slab's 144 points need not)
            assert all(h > 0 for h in hist[-3:]) and hist[BINS_MAX - 1] > 0
        for b in (0, BINS_MAX - 1, BINS_MAX, nbins - 1):
            rc, m, s = q.one_range(dataset, BOXES[name], float(edges[b]), float(edges[b + 1]))
            assert rc == 0 and m == hist[b] and s == scanned
        assert sum(hist) > 0


def test_points_scanned_may_be_null_and_a_missed_box_gives_zeros(q, dataset):
    rc, hist, s = q.by_time(dataset, BOXES["slab"], TABLES["ten"], scanned=False)
    assert rc == 0 and s == 77 and sum(hist) > 0
    rc, hist, s = q.by_time(dataset, BOXES["missed"], TABLES["ten"])
    assert rc == 0 and s == 0 and hist == [0] * 10


def test_failures_leave_the_histogram_untouched(q, files, dataset):
    untouched = [77 + c for c in range(10)]
    bad = ((5.0, 0.0, 0.0), (4.0, 1.0, 1.0))
    assert q.one_range(dataset, bad, 1000.0, 2000.0) == (PCQ_ERR_PANIC, 7, 7)
    rc, hist, s = q.by_time(dataset, bad, TABLES["ten"])
    assert rc == PCQ_ERR_PANIC and hist == untouched and s == 77
    for e in ([1000.0, NAN] + [2000.0] * 9, [2000.0, 1000.0] + [2000.0] * 9):
        rc, hist, s = q.by_time(dataset, BOXES["every"], e)
        assert rc == PCQ_ERR_ARG and hist == untouched and s == 77
    # a dataset without time blocks: PCQ_ERR_ARG with the loader's hint, before the box's own error
    r2 = q.load(files[0], COLOUR)
    try:
        for box in (BOXES["every"], bad):
            rc, hist, s = q.by_time(r2, box, TABLES["ten"])
            assert rc == PCQ_ERR_ARG and b"PCQ_RESIDENT_TIME" in q.err() and hist == untouched and s == 77
    finally:
        q.lib.pcq_query_resident_free(r2)
    rc, hist, _ = q.by_time(dataset, BOXES["every"], TABLES["ten"])
    assert rc == 0 and sum(hist) > 0
