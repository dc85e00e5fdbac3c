"""host/resident.cpp: how many points lie inside this outline, from one pass over a dataset kept in HBM.
pcq_query_resident_count_polygon must give the rule of include/pcq.h (tests/_polygon_rule.py) applied per surviving file to the stored
integers: the vertices numpy.rint((x - offset) / scale) in the file's lattice, the z range of pcq_box_to_local of the outline's world
box, the header early-out applied — with the points_scanned of pcq_query_resident_count_bounds for that world box.

The five small LAST files of tests/_resident_files.py (FIVE_FILES): formats 1, 3 and 6; 3*4096+17, 4096, 100, 0 and
2*4096+5 points; differing scales and offsets, one of them anisotropic; and one file whose header bounds are tighter than its
points, so that the header early-out (last.rs:92-94) is observable.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _polygon_rule as rule  # noqa: E402
import _host  # noqa: E402
import _resident_files as rf  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")

PCQ_ERR_PANIC, PCQ_ERR_UNSUPPORTED = pkg.PCQ_ERR_PANIC, pkg.PCQ_ERR_UNSUPPORTED
FILES = rf.FIVE_FILES
meets = rf.meets
LYING, FINE = rf.LYING, 2
# (vertices, zmin, zmax)
OUTLINES = {"every": ([(-40.0, -310.0), (160.0, -280.0), (340.0, -40.0), (330.0, 45.0), (0.0, 30.0), (-45.0, -100.0)], -1e6, 1e6),  # meets every header
            "single": ([(-20.0, -20.0), (25.005, -10.0), (10.0, 30.015), (-15.0, 12.5)], -5.0, 5.0),                              # a single file
            "missed": ([(500.0, -260.0), (600.0, -250.0), (550.0, -100.0)], -30.0, 40.0),                                        # every header misses it
            "lie": ([(320.0, -40.0), (345.0, -30.0), (340.0, 40.0), (322.0, 20.0)], -10.0, 10.0)}                                # the lying file's hidden points


def world_box(outline):
    xy, zmin, zmax = outline
    v = np.asarray(xy, dtype=np.float64)
    return (v[:, 0].min(), v[:, 1].min(), zmin), (v[:, 0].max(), v[:, 1].max(), zmax)


class Q:
    def __init__(self):
        self.lib = _host.lib()

    err = staticmethod(_host.err)
    load = staticmethod(_host.load)
    bounds = staticmethod(_host.bounds)

    def polygon(self, r, outline, sentinel=77, scanned=True):
        xy, zmin, zmax = outline
        flat = [float(c) for p in xy for c in p]
        m, s = C.c_uint64(sentinel), C.c_uint64(sentinel + 1)
        rc = self.lib.pcq_query_resident_count_polygon(r, len(xy), (C.c_double * len(flat))(*flat), zmin, zmax, C.byref(m),
                                                       C.byref(s) if scanned else None)
        return rc, m.value, s.value


@pytest.fixture(scope="module")
def q():
    return Q()


def corpus(d):
    return rf.write_files(d, FILES, 950, LYING)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files, and per file what tests/_resident_files.py holds of it."""
    return corpus(tmp_path_factory.mktemp("resident_polygon"))


def lattice(xy, h):
    """numpy.rint((w - offset) / scale): two f64 operations in this order, ties to even"""
    v = np.asarray(xy, dtype=np.float64)
    return np.stack([np.rint((v[:, a] - np.float64(h.offset[a])) / np.float64(h.scale[a])) for a in range(2)], axis=1).astype(np.int64)


def rule_count(held, outline, header=True):
    """The rule over the files whose headers meet the outline's world box, on the stored integers"""
    box = world_box(outline)
    total = 0
    for h in held:
        if (header and not meets(h, box)) or not len(h.xyz):
            continue
        lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
        v = lattice(outline[0], h)
        lo, hi = [int(v[:, 0].min()), int(v[:, 1].min()), lmin[2]], [int(v[:, 0].max()), int(v[:, 1].max()), lmax[2]]
        total += int(rule.counted(h.xyz, lo, hi, v.tolist()).sum())
    return total


@pytest.fixture(scope="module")
def dataset(q, files):
    r = q.load(files[0])
    yield r
    q.lib.pcq_query_resident_free(r)


@pytest.mark.parametrize("name", list(OUTLINES))
def test_matches_are_the_rule_on_the_files_integers(q, files, dataset, name):
    _, held = files
    outline = OUTLINES[name]
    box = world_box(outline)
    rc, got, scanned = q.polygon(dataset, outline)
    assert rc == 0, q.err()
    want = rule_count(held, outline)
    assert got == want
    rc, m, s = q.bounds(dataset, box)
    assert rc == 0 and s == scanned == sum(len(h.xyz) for h in held if meets(h, box))
    n = [len(h.xyz) for h in held]
    if name == "every":
        assert scanned == sum(n) and 0 < got < sum(n)
        assert all(rule_count([h], outline) > 0 for h in held if len(h.xyz))  # every file with points contributes
    elif name == "single":
        assert scanned == n[1] and 100 < got < n[1]
    elif name == "missed":
        assert scanned == 0 and got == 0
    else:  # the lying file: its points match in integer space, its header says no, and the header decides
        assert rule_count([held[LYING]], outline, header=False) > 0
        assert not any(meets(f, box) for f in held) and scanned == 0 and got == 0
    rc, again, _ = q.polygon(dataset, outline, scanned=False)  # points_scanned not wanted
    assert rc == 0 and again == got


def test_orientation_and_start_do_not_matter(q, files, dataset):
    xy, zmin, zmax = OUTLINES["every"]
    _, want, _ = q.polygon(dataset, OUTLINES["every"])
    for other in (xy[::-1], xy[2:] + xy[:2]):
        rc, got, _ = q.polygon(dataset, (other, zmin, zmax))
        assert rc == 0 and got == want


def test_errors_leave_the_outputs_alone(q, files, dataset):
    paths, held = files
    xy, zmin, zmax = OUTLINES["every"]
    rc, m, s = q.polygon(dataset, (xy, 5.0, -5.0), sentinel=41)  # zmin > zmax
    assert rc == PCQ_ERR_PANIC and (m, s) == (41, 42), q.err()
    # an outline 2^31 steps wide in the 0.001-scale file's lattice; the files before it in load order take it
    half = 2**30 * 0.001
    wide = [(100.0 - half, -1000.0), (100.0 + half, -1000.0), (100.0, 1000.0)]
    v = lattice(wide, held[FINE])
    assert int(v[:, 0].max() - v[:, 0].min()) == 2**31
    for k in range(FINE):
        u = lattice(wide, held[k])
        assert int(u[:, 0].max() - u[:, 0].min()) < 2**31 - 1 and np.abs(u).max() < 2**31 - 1
    rc, m, s = q.polygon(dataset, (wide, -1e6, 1e6), sentinel=43)
    assert rc == PCQ_ERR_UNSUPPORTED and (m, s) == (43, 44), q.err()
    assert os.path.basename(paths[FINE]).encode() in q.err(), q.err()
    # one step narrower is asked of every file
    narrower = [(100.0 - half + 0.001, -1000.0), (100.0 + half, -1000.0), (100.0, 1000.0)]
    assert int(np.ptp(lattice(narrower, held[FINE])[:, 0])) == 2**31 - 1
    rc, m, s = q.polygon(dataset, (narrower, -1e6, 1e6))
    assert rc == 0 and m == rule_count(held, (narrower, -1e6, 1e6)) > 0, q.err()
