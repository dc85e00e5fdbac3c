"""host/resident.cpp: GPS time queries over a dataset kept in HBM.  pcq_query_resident_load_with(.., PCQ_RESIDENT_TIME) loads
every file's time block where the LAST time search finds it, and pcq_query_resident_search_time must equal the per-file
searches (pcq_query_search_file_time, --optimized) over the same files, in load order, into one collector: the count, the
records byte for byte and in order, the grid cells and their winners.  Count and buffer collectors go through the time part
of each file's chunk index; the old loaders and searches behave as before."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _host  # noqa: E402
import _time_images as ti  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "adhoc-queries-pointclouds_amd")

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
POINT_DTYPE = pkg.POINT_DTYPE
PCQ_ERR_ARG, PCQ_ERR_FORMAT = pkg.PCQ_ERR_ARG, pkg.PCQ_ERR_FORMAT
COLOUR, TIME = pkg.PCQ_RESIDENT_COLOUR, pkg.PCQ_RESIDENT_TIME
FILES = [(1, 3 * 4096 + 17), (3, 4096), (6, 100), (7, 0)]  # (format, points)
GRID = ((40.0, -320.0, -60.0), (160.0, -80.0, 120.0), 2.0)
RANGES = [(1200.0, 1300.0), (1000.0, 1500.0), (1999.0, 2001.0), (-np.inf, np.inf), (1500.0, 1500.0), (5.0, 6.0), (np.nan, 1.0)]


class Q:
    """include/pcq_query.h through the package's view; the shared calls are tests/_host.py's"""

    def __init__(self):
        self.lib = _host.lib()

    d3 = staticmethod(_host.d3)
    err = staticmethod(_host.err)
    stats = staticmethod(_host.last_stats)

    @staticmethod
    def collector(kind, device=0):
        return _host.collector(kind, GRID, device)

    @staticmethod
    def result(h, kind):
        """count, or the records (buffer: file order), or (sorted cell keys, winners in key order); frees the collector"""
        try:
            return _host.result(h, kind)
        finally:
            _host.free_collector(h)

    @staticmethod
    def load(paths, blocks, device=0):
        return _host.try_load(paths, blocks, device, preset=99)


@pytest.fixture(scope="module")
def q():
    return Q()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """LAST files of formats 1, 3, 6 and 7 with sorted GPS times in [1000, 2000), and what they hold."""
    d = tmp_path_factory.mktemp("resident_time")
    paths, held = [], []
    for fmt, n in FILES:
        xyz, cls, rgb, t = ti.points(n, 600 + fmt)
        p = str(d / f"f{fmt}.last")
        ti.last_image(fmt, xyz, cls, rgb, t).tofile(p)
        paths.append(p)
        held.append((xyz, t))
    return paths, held


def per_file(q, paths, kind, start, end):
    h = q.collector(kind)
    for path in paths:
        assert q.lib.pcq_query_search_file_time(path.encode(), start, end, 1, h) == 0, q.err()
    return q.result(h, kind)


def resident(q, r, kind, start, end):
    h = q.collector(kind)
    assert q.lib.pcq_query_resident_search_time(r, start, end, h) == 0, q.err()
    return q.result(h, kind)


@pytest.fixture(scope="module")
def expected(q, files):
    """The per-file searches, once per (range, collector); counts and records against numpy as well."""
    paths, held = files
    out = {}
    for ri, (start, end) in enumerate(RANGES):
        for kind in ("count", "buffer", "grid"):
            out[ri, kind] = per_file(q, paths, kind, start, end)
        want = b"".join(ti.expect_records(xyz, ti.select(t, start, end), POINT_DTYPE).tobytes() for xyz, t in held)
        assert out[ri, "buffer"] == want and out[ri, "count"] == len(want) // 31, (start, end)
    assert 0 < out[0, "count"] < out[1, "count"] < out[3, "count"] == sum(n for _, n in FILES)
    return out


@pytest.mark.parametrize("blocks", [TIME, TIME | COLOUR])
def test_resident_time_search_equals_the_per_file_searches(q, files, expected, blocks):
    paths, _ = files
    rc, r = q.load(paths, blocks)
    assert rc == 0, q.err()
    chunks = sum(n // 4096 for _, n in FILES)
    try:
        for ri, (start, end) in enumerate(RANGES):
            for kind in ("count", "buffer", "grid"):
                for rep in range(2):  # the second time through the built parts
                    assert resident(q, r, kind, start, end) == expected[ri, kind], (start, end, kind, rep)
                    st = q.stats(r)
                    if kind == "grid":
                        assert not any(st.values()), st  # grid collectors use no index
                    else:
                        # (the file of 100 points falls through to the plain scan, the empty one is skipped)
                        assert st["chunks"] == chunks == st["skipped"] + st["whole"] + st["scanned"], st
                        assert st["built"] == (2 if (ri, kind, rep) == (0, "count", 0) else 0), (ri, kind, rep, st)
        # a repeated count query is pruned
        for rep in range(2):
            assert resident(q, r, "count", *RANGES[0]) == expected[0, "count"]
            st = q.stats(r)
            assert st["built"] == 0 and st["skipped"] > 0 and st["chunks"] == chunks, st
    finally:
        q.lib.pcq_query_resident_free(r)


def test_old_searches_on_a_dataset_loaded_with_times_behave_as_before(q, files):
    paths, held = files
    rc, r = q.load(paths, TIME | COLOUR)
    assert rc == 0, q.err()
    rc2, r2 = q.load(paths, TIME)
    assert rc2 == 0, q.err()
    try:
        bmin, bmax = (90.0, -250.0, 0.0), (120.0, -150.0, 20.0)
        m, s = C.c_uint64(7), C.c_uint64(7)
        for kind in ("count", "buffer"):
            h = q.collector(kind)
            size = C.c_int(-1)
            for p in paths:
                assert q.lib.pcq_query_search_file_bounds(p.encode(), q.d3(bmin), q.d3(bmax), 1, h, C.byref(size)) == 0, q.err()
            want = q.result(h, kind)
            h = q.collector(kind)
            assert q.lib.pcq_query_resident_search_bounds(r, q.d3(bmin), q.d3(bmax), h) == 0, q.err()
            assert q.result(h, kind) == want and len(want if kind == "buffer" else [0] * want) > 0
            if kind == "count":
                for rr in (r, r2):
                    assert q.lib.pcq_query_resident_count_bounds(rr, q.d3(bmin), q.d3(bmax), C.byref(m), C.byref(s)) == 0, q.err()
                    assert m.value == want
        h = q.collector("count")
        for p in paths:
            assert q.lib.pcq_query_search_file_class(p.encode(), 6, 1, h) == 0, q.err()
        want = q.result(h, "count")
        assert want == sum(int((ti.points(n, 600 + fmt)[1] == 6).sum()) for fmt, n in FILES) > 0
        for rr in (r, r2):
            assert q.lib.pcq_query_resident_count_class(rr, 6, C.byref(m), C.byref(s)) == 0 and m.value == want
            h = q.collector("count")
            assert q.lib.pcq_query_resident_search_class(rr, 6, h) == 0, q.err()
            assert q.result(h, "count") == want
        # without the colour blocks the other searches still refuse collectors that hold points; the time search serves them
        h = q.collector("buffer")
        assert q.lib.pcq_query_resident_search_bounds(r2, q.d3(bmin), q.d3(bmax), h) == PCQ_ERR_ARG
        assert b"without its colour blocks" in q.err()
        assert q.lib.pcq_query_resident_search_time(r2, 1200.0, 1300.0, h) == 0, q.err()
        assert q.result(h, "buffer") == per_file(q, paths, "buffer", 1200.0, 1300.0)
    finally:
        q.lib.pcq_query_resident_free(r)
        q.lib.pcq_query_resident_free(r2)


def test_errors(q, files, tmp_path):
    paths, _ = files
    xyz, cls, rgb, t = ti.points(500, 9)
    bad = str(tmp_path / "no_times.last")
    ti.last_image(2, xyz, cls, rgb, t).tofile(bad)
    for blocks in (TIME, TIME | COLOUR):
        rc, r = q.load([paths[0], bad, paths[1]], blocks)
        assert rc == PCQ_ERR_FORMAT and r.value is None
        assert q.err() == f"File {bad} does not contain GPS times!".encode()
    above = str(tmp_path / "format_11.last")
    ti.last_image(1, xyz, cls, rgb, t, fmt_byte=11).tofile(above)
    rc, r = q.load([above], TIME)
    assert rc == PCQ_ERR_FORMAT and b"Invalid LAS format 11" in q.err()
    short = str(tmp_path / "short.last")
    ti.last_image(1, xyz, cls, rgb, t)[:-8].tofile(short)  # the time block ends the body of a format-1 file
    rc, r = q.load([short], TIME)
    assert rc == -5, q.err()
    rc, r = q.load([bad], COLOUR)  # the same file without the TIME bit: loaded as before
    assert rc == 0, q.err()
    h = q.collector("count")
    assert q.lib.pcq_query_resident_search_time(r, 0.0, 1.0, h) == PCQ_ERR_ARG
    assert b"PCQ_RESIDENT_TIME" in q.err()
    assert q.result(h, "count") == 0
    q.lib.pcq_query_resident_free(r)
    arr = (C.c_char_p * 1)(paths[0].encode())
    hp = C.c_void_p()
    assert q.lib.pcq_query_resident_load_points(0, arr, 1, C.byref(hp)) == 0, q.err()
    h = q.collector("buffer")
    assert q.lib.pcq_query_resident_search_time(hp, 0.0, 1.0, h) == PCQ_ERR_ARG
    assert q.result(h, "buffer") == b""
    q.lib.pcq_query_resident_free(hp)
