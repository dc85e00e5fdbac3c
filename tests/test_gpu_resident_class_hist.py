"""host/resident.cpp: what is in this box, by class, from one pass over a dataset kept in HBM.
pcq_query_resident_count_bounds_by_class must give, for every class byte c in 0..255, what
pcq_query_resident_count_bounds_class gives for c — zeros included — with the same points_scanned, and its bins must sum to what
pcq_query_resident_count_bounds counts.

The five small LAST files of tests/_resident_files.py (FIVE_FILES), with classes of its own: formats 1, 3 and 6; 3*4096+17, 4096, 100, 0
and 2*4096+5 points; differing scales and offsets, one of them anisotropic; and one file whose header bounds are tighter than its
points, so that the header early-out (last.rs:92-94) is observable.  Classes are drawn from {0, 1, 2, 5, 6, 255}.
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

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

PCQ_ERR_PANIC = pkg.PCQ_ERR_PANIC
TIME = pkg.PCQ_RESIDENT_TIME
CLASSES = (0, 1, 2, 5, 6, 255)
FILES = rf.FIVE_FILES
meets = rf.meets
LYING = rf.LYING
BIG = 1e6
BOXES = {"every": ((-BIG, -BIG, -BIG), (BIG, BIG, BIG)),                # meets every header
         "single": ((-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)),            # a single file
         "missed": ((500.003, -260.0, -30.0), (600.003, -140.0, 40.0)),  # every header misses it
         "slab": ((100.003, -BIG, -BIG), (101.003, BIG, BIG)),           # a thin slab
         "lie": ((320.0, -50.0, -10.0), (340.0, 50.0, 10.0))}            # the lying file's points outside its header


class Q:
    def __init__(self):
        self.lib = _host.lib()

    err = staticmethod(_host.err)
    load = staticmethod(_host.load)
    bounds = staticmethod(_host.bounds)

    def one_class(self, r, box, c):
        m, s = C.c_uint64(7), C.c_uint64(7)
        rc = self.lib.pcq_query_resident_count_bounds_class(r, (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]), c, C.byref(m), C.byref(s))
        return rc, m.value, s.value

    def by_class(self, r, box, sentinel=77, scanned=True):
        hist, s = (C.c_uint64 * 256)(*[sentinel + c for c in range(256)]), C.c_uint64(sentinel)
        rc = self.lib.pcq_query_resident_count_bounds_by_class(r, (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]), hist,
                                                               C.byref(s) if scanned else None)
        return rc, list(hist), s.value


@pytest.fixture(scope="module")
def q():
    return Q()


def corpus(d):
    return rf.write_files(d, FILES, 950, LYING, classes=CLASSES)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files, and per file what tests/_resident_files.py holds of it."""
    return corpus(tmp_path_factory.mktemp("resident_class_hist"))


def numpy_hist(held, box):
    """bincount of the class bytes of the stored integer coordinates inside the local box of pcq_box_to_local, over the files
    whose headers meet the box"""
    out = np.zeros(256, dtype=np.int64)
    for h in held:
        if not meets(h, box) or not len(h.xyz):
            continue
        lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
        x = h.xyz.astype(np.int64)
        sel = np.all((x >= np.asarray(lmin, dtype=np.int64)) & (x <= np.asarray(lmax, dtype=np.int64)), axis=1)
        out += np.bincount(h.cls[sel], minlength=256)
    return out


@pytest.fixture(scope="module", params=["load", "load_with_time"])
def dataset(request, q, files):
    r = q.load(files[0], None if request.param == "load" else TIME)
    yield r
    q.lib.pcq_query_resident_free(r)


@pytest.mark.parametrize("name", list(BOXES))
def test_every_bin_is_the_combined_count_of_its_class(q, files, dataset, name):
    _, held = files
    box = BOXES[name]
    rc, hist, scanned = q.by_class(dataset, box)
    assert rc == 0, q.err()
    want_scanned = sum(len(h.xyz) for h in held if meets(h, box))
    for c in range(256):
        rc, m, s = q.one_class(dataset, box, c)
        assert rc == 0, q.err()
        assert hist[c] == m, (name, c, hist[c], m)
        assert s == scanned == want_scanned
    rc, m, s = q.bounds(dataset, box)
    assert rc == 0 and sum(hist) == m and s == scanned
    assert hist == numpy_hist(held, box).tolist()
    assert all(hist[c] == 0 for c in range(256) if c not in CLASSES)
    # the boxes are what they are meant to be
    n = [len(h.xyz) for h in held]
    if name == "every":
        assert sum(hist) == sum(n) == scanned and all(hist[c] > 0 for c in CLASSES)
    elif name == "single":
        assert scanned == n[1] and 0 < sum(hist) < n[1]
    elif name == "missed":
        assert scanned == 0 and sum(hist) == 0
    elif name == "slab":
        assert 0 < sum(hist) < scanned
    else:  # the lying file: its points match in integer space, its header says no, and the header decides
        h = held[LYING]
        lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
        x = h.xyz.astype(np.int64)
        assert np.all((x >= np.asarray(lmin)) & (x <= np.asarray(lmax)), axis=1).sum() > 0
        assert not any(meets(f, box) for f in held) and scanned == 0 and sum(hist) == 0


def test_points_scanned_may_be_null(q, dataset):
    rc, hist, s = q.by_class(dataset, BOXES["slab"], scanned=False)
    assert rc == 0 and s == 77 and sum(hist) > 0


def test_a_box_that_panics_leaves_the_histogram_untouched(q, dataset):
    bad = ((5.0, 0.0, 0.0), (4.0, 1.0, 1.0))
    assert q.one_class(dataset, bad, 2) == (PCQ_ERR_PANIC, 7, 7)
    rc, hist, s = q.by_class(dataset, bad)
    assert rc == PCQ_ERR_PANIC and hist == [77 + c for c in range(256)] and s == 77
    rc, hist, _ = q.by_class(dataset, BOXES["every"])
    assert rc == 0 and sum(hist) > 0
