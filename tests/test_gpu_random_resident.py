"""Seeded random parity of the count queries over a dataset resident in HBM with numpy (_random_resident.py; its seeds are proven on
the CPU by test_random_batches_plan.py).  PCQ_TEST_SEED_BASE moves the whole seed range for a soak run.

Per seed: 2 .. 6 LAST files are written and loaded with their time blocks (pcq_query_resident_load_with), and each of the ten
count entries of include/pcq_query.h and the two mean-height rasters of pcq_query_stats.h and pcq_query_classes.h is asked once with a world-space query drawn around the files' own points.  Every call
has to return 0 (the generator draws only what the entries accept) and every output word has to be numpy's: the matches, the
histograms, every raster cell — both rasters have more cells than one launch holds, in some seeds rows longer than a launch —
the world z of the height raster bit for bit with NaN where no point lies, the mean-height rasters' counts as integers and their
means as f64 bit patterns (NaN is an answer), and points_scanned / points_read.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _random_resident as rr  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
PCQ_RESIDENT_TIME = pkg.PCQ_RESIDENT_TIME
SENTINEL = 77


class Q:
    def __init__(self):
        self.lib = pkg.load_query_library()

    def err(self):
        return self.lib.pcq_query_last_error()


@pytest.fixture(scope="module")
def q():
    return Q()


d3 = pkg.d3


def u64s(n):
    """n output words preset to distinct non-zero values"""
    a = (SENTINEL + 3 * np.arange(n)).astype(np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def ask(q, r, entry, qu):
    """The entry's outputs as _random_resident.answer names them"""
    lib = q.lib
    m, s = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    out = {}
    if entry == "bounds":
        rc = lib.pcq_query_resident_count_bounds(r, d3(qu.bmin), d3(qu.bmax), C.byref(m), C.byref(s))
    elif entry == "class":
        rc = lib.pcq_query_resident_count_class(r, qu.cls, C.byref(m), C.byref(s))
    elif entry == "bounds_class":
        rc = lib.pcq_query_resident_count_bounds_class(r, d3(qu.bmin), d3(qu.bmax), qu.cls, C.byref(m), C.byref(s))
    elif entry == "bounds_time":
        rc = lib.pcq_query_resident_count_bounds_time(r, d3(qu.bmin), d3(qu.bmax), qu.t0, qu.t1, C.byref(m), C.byref(s))
    elif entry == "many":
        n = len(qu.bmin)
        lo = (C.c_double * (3 * n))(*[float(v) for b in qu.bmin for v in b])
        hi = (C.c_double * (3 * n))(*[float(v) for b in qu.bmax for v in b])
        (mm, pm), (ss, ps) = u64s(n), u64s(n)
        rc = lib.pcq_query_resident_count_bounds_many(r, n, lo, hi, pm, ps, C.byref(m))
        return rc, dict(matches=mm.astype(np.int64), scanned=ss.astype(np.int64), read=m.value)
    elif entry == "by_class":
        hist, ph = u64s(256)
        rc = lib.pcq_query_resident_count_bounds_by_class(r, d3(qu.bmin), d3(qu.bmax), ph, C.byref(s))
        out["hist"] = hist.astype(np.int64)
    elif entry == "by_time":
        e = np.ascontiguousarray(qu.edges, dtype=np.float64)
        hist, ph = u64s(len(e) - 1)
        rc = lib.pcq_query_resident_count_bounds_by_time(r, d3(qu.bmin), d3(qu.bmax), e.ctypes.data_as(C.POINTER(C.c_double)), len(e) - 1, ph, C.byref(s))
        out["hist"] = hist.astype(np.int64)
    elif entry == "raster":
        words, pw = u64s(qu.nx * qu.ny)
        rc = lib.pcq_query_resident_count_bounds_raster(r, d3(qu.bmin), qu.zmax, qu.cell, qu.nx, qu.ny, pw, C.byref(s))
        out["raster"] = words.astype(np.int64)
    elif entry == "zrange":
        zlo, zhi = np.full(qu.nx * qu.ny, 0.5), np.full(qu.nx * qu.ny, -0.25)
        dd = C.POINTER(C.c_double)
        rc = lib.pcq_query_resident_bounds_zrange_raster(r, d3(qu.bmin), qu.zmax, qu.cell, qu.nx, qu.ny, zlo.ctypes.data_as(dd), zhi.ctypes.data_as(dd),
                                                         C.byref(s))
        out["zlo"], out["zhi"] = zlo, zhi
    elif entry in ("zmean", "zmean_classes"):
        count, pc = u64s(qu.nx * qu.ny)
        zmean = np.full(qu.nx * qu.ny, -0.25)
        pm = zmean.ctypes.data_as(C.POINTER(C.c_double))
        if entry == "zmean":
            rc = lib.pcq_query_resident_bounds_zmean_raster(r, d3(qu.bmin), qu.zmax, qu.cell, qu.nx, qu.ny, pc, pm, C.byref(s))
        else:
            words = [sum(1 << (v % 32) for v in qu.classes if v // 32 == w) for w in range(8)]
            rc = lib.pcq_query_resident_bounds_zmean_raster_classes(r, d3(qu.bmin), qu.zmax, qu.cell, qu.nx, qu.ny, (C.c_uint32 * 8)(*words), pc, pm,
                                                                    C.byref(s))
        out["count"], out["zmean"] = count.astype(np.int64), zmean
    else:
        flat = [float(v) for p in qu.xy for v in p]
        rc = lib.pcq_query_resident_count_polygon(r, len(qu.xy), (C.c_double * len(flat))(*flat), qu.zmin, qu.zmax, C.byref(m), C.byref(s))
    if "hist" not in out and "raster" not in out and "zlo" not in out and "count" not in out:
        out["matches"] = m.value
    out["scanned"] = s.value
    return rc, out


def differences(got, want):
    """What differs, output by output: the f64 words of the height raster are compared as bits (NaN is an answer)"""
    bad = []
    for key, w in want.items():
        g = got[key]
        if isinstance(w, np.ndarray):
            a, b = (g.view(np.uint64), w.view(np.uint64)) if w.dtype == np.float64 else (g, w)
            at = np.flatnonzero(a != b)
            if len(at):
                bad.append(f"{key}: {len(at)} of {len(w)} words, (word, got, want) {[(int(i), g[i].item(), w[i].item()) for i in at[:4]]}")
        elif int(g) != int(w):
            bad.append(f"{key}: got {int(g)}, want {int(w)}")
    return bad


def load(q, tmp_path, c):
    paths = []
    for k, f in enumerate(c.files):
        p = str(tmp_path / f"s{c.seed}_f{k}_{f.fmt}_{f.n}.last")
        rr.image(f).tofile(p)
        paths.append(p)
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    r = C.c_void_p()
    assert q.lib.pcq_query_resident_load_with(0, arr, len(paths), PCQ_RESIDENT_TIME, C.byref(r)) == 0, q.err()
    return r


@pytest.mark.parametrize("seed", rr.SEEDS)
@pytest.mark.parametrize("entry", ["zmean", "zmean_classes"])
def test_the_mean_height_rasters_against_numpy(q, tmp_path, entry, seed):
    """The two entries that joined later, each alone on a freshly loaded dataset and asked twice: the second call meets the first
    call's tables and partials, and has to give the same words"""
    c = rr.case(seed)
    r = load(q, tmp_path, c)
    wrong = []
    try:
        for visit in range(2):
            rc, got = ask(q, r, entry, c.q[entry])
            assert rc == 0, f"seed {seed}, {entry}: refused with {rc}: {q.err()}"
            wrong += [f"{entry}, call {visit}: {d}" for d in differences(got, c.answer[entry])]
    finally:
        q.lib.pcq_query_resident_free(r)
    what = [(f.fmt, f.n, f.scale, f.offset, "lying" if f.lying else "") for f in c.files]
    assert not wrong, (f"seed {seed} (PCQ_TEST_SEED_BASE {rr.SEED_BASE}), files (format, n, scale, offset) {what}, classes "
                       f"{getattr(c.q[entry], 'classes', None)}: " + "; ".join(wrong))


@pytest.mark.parametrize("seed", rr.SEEDS)
def test_every_count_entry_against_numpy(q, tmp_path, seed):
    c = rr.case(seed)
    paths = []
    for k, f in enumerate(c.files):
        p = str(tmp_path / f"s{seed}_f{k}_{f.fmt}_{f.n}.last")
        rr.image(f).tofile(p)
        paths.append(p)
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    r = C.c_void_p()
    assert q.lib.pcq_query_resident_load_with(0, arr, len(paths), PCQ_RESIDENT_TIME, C.byref(r)) == 0, q.err()
    wrong = []
    try:
        for entry in rr.ENTRIES:
            rc, got = ask(q, r, entry, c.q[entry])
            if rc != 0:
                wrong.append(f"{entry}: refused with {rc}: {q.err()}")
                continue
            wrong += [f"{entry}: {d}" for d in differences(got, c.answer[entry])]
    finally:
        q.lib.pcq_query_resident_free(r)
    what = [(f.fmt, f.n, f.scale, f.offset, "lying" if f.lying else "") for f in c.files]
    assert not wrong, f"seed {seed} (PCQ_TEST_SEED_BASE {rr.SEED_BASE}), files (format, n, scale, offset) {what}: " + "; ".join(wrong)
