"""host/resident.cpp: many boxes in one pass over a dataset kept in HBM.  pcq_query_resident_count_bounds_many must give, for
every box, what pcq_query_resident_count_bounds gives for it alone — matches and points_scanned, element by element — whatever
the number of boxes (one group of up to eight per launch), and points_read must be the points of the files met by any box of a
group, summed over the groups.

The five small LAST files of tests/_resident_files.py (FIVE_FILES): formats 1, 3 and 6; 3*4096+17, 4096, 100, 0 and 2*4096+5 points; differing scales and
offsets, one of them anisotropic (the box conversion of last.rs:100-102 then moves a min corner); and one file whose header
bounds are tighter than its points, so that the header early-out (last.rs:92-94) is observable: a box that meets those points
but not the header counts nothing.
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

PCQ_ERR_PANIC = pkg.PCQ_ERR_PANIC
COLOUR, TIME = pkg.PCQ_RESIDENT_COLOUR, pkg.PCQ_RESIDENT_TIME
FILES = rf.FIVE_FILES
meets = rf.meets
LYING = rf.LYING
A, B, CC, E = 0, 1, 2, 4
BIG = 1e6
BOXES = [((-BIG, -BIG, -BIG), (BIG, BIG, BIG)),                          # 0 meets every header
         ((-20.0, -20.0, -5.0), (20.0, 20.0, 5.0)),                      # 1 a single file
         ((500.003, -260.0, -30.0), (600.003, -140.0, 40.0)),            # 2 every header misses it
         ((100.003, -BIG, -BIG), (101.003, BIG, BIG)),                   # 3 a thin slab
         ((-BIG, -BIG, -BIG), (BIG, BIG, BIG)),                          # 4 = 0
         ((100.003, -BIG, -BIG), (101.003, BIG, BIG)),                   # 5 = 3
         ((320.0, -50.0, -10.0), (340.0, 50.0, 10.0)),                   # 6 meets the lying file's points, not its header
         ((90.0, -210.0, -50.0), (110.0, -190.0, 50.0)),                 # 7 two files, and not the one at the origin
         ((260.0, -40.0, -8.0), (290.0, 40.0, 8.0))]                     # 8 the lying file inside its header
BOXES += [((60.0 + 10 * j, -280.0 + 5 * j, -30.0), (90.0 + 10 * j, -150.0 + 5 * j, 40.0)) for j in range(8)]
EVERY, SINGLE, MISSED, SLAB, LIE, TWO = 0, 1, 2, 3, 6, 7
assert len(BOXES) == 17


class Q:
    def __init__(self):
        self.lib = _host.lib()

    err = staticmethod(_host.err)
    load = staticmethod(_host.load)

    def one(self, r, box):
        m, s = C.c_uint64(7), C.c_uint64(7)
        rc = self.lib.pcq_query_resident_count_bounds(r, (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1]), C.byref(m), C.byref(s))
        return rc, m.value, s.value

    def many(self, r, boxes, sentinel=77):
        n = len(boxes)
        lo = (C.c_double * (3 * n))(*[v for b in boxes for v in b[0]])
        hi = (C.c_double * (3 * n))(*[v for b in boxes for v in b[1]])
        m, s = (C.c_uint64 * n)(*[sentinel] * n), (C.c_uint64 * n)(*[sentinel] * n)
        read = C.c_uint64(sentinel)
        rc = self.lib.pcq_query_resident_count_bounds_many(r, n, lo, hi, m, s, C.byref(read))
        return rc, list(m), list(s), read.value


@pytest.fixture(scope="module")
def q():
    return Q()


def corpus(d):
    return rf.write_files(d, FILES, 900, LYING)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The files, and per file what tests/_resident_files.py holds of it."""
    return corpus(tmp_path_factory.mktemp("resident_multi"))


def integer_matches(h, box):
    """numpy's count of the stored integer coordinates inside the local box of pcq_box_to_local, header or no header"""
    lmin, lmax = pkg.box_to_local(list(box[0]), list(box[1]), list(h.scale), list(h.offset))
    x = h.xyz.astype(np.int64)
    return int(np.all((x >= np.asarray(lmin, dtype=np.int64)) & (x <= np.asarray(lmax, dtype=np.int64)), axis=1).sum())


def expected_read(held, boxes):
    return sum(sum(len(h.xyz) for h in held if any(meets(h, b) for b in boxes[g:g + 8])) for g in range(0, len(boxes), 8))


@pytest.fixture(scope="module")
def dataset(q, files):
    r = q.load(files[0])
    yield r
    q.lib.pcq_query_resident_free(r)


@pytest.fixture(scope="module")
def single(q, files, dataset):
    """Every box alone through the existing entry, checked against numpy and the headers."""
    paths, held = files
    out = []
    for box in BOXES:
        rc, m, s = q.one(dataset, box)
        assert rc == 0, q.err()
        assert m == sum(integer_matches(h, box) for h in held if meets(h, box)), box
        assert s == sum(len(h.xyz) for h in held if meets(h, box)), box
        out.append((m, s))
    return out


def test_the_boxes_are_what_they_are_meant_to_be(files, single):
    _, held = files
    n = [len(h.xyz) for h in held]
    assert single[EVERY] == (sum(n), sum(n)) and single[4] == single[EVERY] and single[5] == single[SLAB]
    assert single[SINGLE][1] == n[B] and single[SINGLE][0] > 0
    assert single[MISSED] == (0, 0)
    assert 0 < single[SLAB][0] < single[SLAB][1]
    # the lying file: its points match in integer space, its header says no, and the header decides
    assert integer_matches(held[LYING], BOXES[LIE]) > 0 and not any(meets(h, BOXES[LIE]) for h in held) and single[LIE] == (0, 0)
    # not vacuous: one box counts in two files and leaves a third unscanned
    assert integer_matches(held[A], BOXES[TWO]) > 0 and integer_matches(held[CC], BOXES[TWO]) > 0 and not meets(held[B], BOXES[TWO])
    assert single[TWO][1] == n[A] + n[CC]
    # the anisotropic file: the reference's conversion is not the exact one on the min corner of y or z
    lmin, _ = pkg.box_to_local(list(BOXES[TWO][0]), list(BOXES[TWO][1]), list(ti.SCALE), list(ti.OFFSET))
    exact = [(BOXES[TWO][0][a] - ti.OFFSET[a]) / ti.SCALE[a] for a in range(3)]
    assert any(abs(lmin[a] - exact[a]) > 2 for a in (1, 2)), (lmin, exact)


@pytest.mark.parametrize("nboxes", [1, 3, 8, 9, 17])
def test_many_equals_the_single_box_entry(q, files, dataset, single, nboxes):
    _, held = files
    rc, m, s, read = q.many(dataset, BOXES[:nboxes])
    assert rc == 0, q.err()
    assert m == [x[0] for x in single[:nboxes]], [a - x[0] for a, x in zip(m, single)]
    assert s == [x[1] for x in single[:nboxes]]
    assert read == expected_read(held, BOXES[:nboxes])
    if nboxes == 17:  # (the third group is the last box alone: it meets one file, and only that file is read for it)
        assert [k for k, h in enumerate(held) if len(h.xyz) and meets(h, BOXES[16])] == [A]
        assert read == expected_read(held, BOXES[:16]) + len(held[A].xyz)


def test_reordering_the_boxes_permutes_the_answers(q, files, dataset, single):
    _, held = files
    order = [(5 * i + 3) % 17 for i in range(17)]
    assert sorted(order) == list(range(17))
    boxes = [BOXES[i] for i in order]
    rc, m, s, read = q.many(dataset, boxes)
    assert rc == 0, q.err()
    assert m == [single[i][0] for i in order] and s == [single[i][1] for i in order]
    assert read == expected_read(held, boxes)
    # a group no file meets is no launch at all
    rc, m, s, read = q.many(dataset, [BOXES[MISSED], BOXES[LIE]])
    assert (rc, m, s, read) == (0, [0, 0], [0, 0], 0)


def test_a_box_that_panics_fails_the_call_and_writes_nothing(q, dataset, single):
    bad = ((5.0, 0.0, 0.0), (4.0, 1.0, 1.0))
    assert q.one(dataset, bad) == (PCQ_ERR_PANIC, 7, 7)
    boxes = BOXES[:5] + [bad] + BOXES[5:8]
    rc, m, s, read = q.many(dataset, boxes)
    assert rc == PCQ_ERR_PANIC and m == [77] * 9 and s == [77] * 9 and read == 77
    rc, m, s, _ = q.many(dataset, BOXES[:9])
    assert rc == 0 and m == [x[0] for x in single[:9]] and s == [x[1] for x in single[:9]]


def test_a_dataset_with_colour_and_time_blocks_answers_the_same_and_the_old_entries_are_unchanged(q, files, single):
    paths, held = files
    r = q.load(paths, COLOUR | TIME)
    try:
        def old():
            out = []
            for box in (BOXES[EVERY], BOXES[SLAB], BOXES[TWO]):
                lo, hi = (C.c_double * 3)(*box[0]), (C.c_double * 3)(*box[1])
                m, s = C.c_uint64(7), C.c_uint64(7)
                assert q.lib.pcq_query_resident_count_bounds(r, lo, hi, C.byref(m), C.byref(s)) == 0, q.err()
                out.append((m.value, s.value))
                assert q.lib.pcq_query_resident_count_bounds_class(r, lo, hi, 2, C.byref(m), C.byref(s)) == 0, q.err()
                out.append((m.value, s.value))
                assert q.lib.pcq_query_resident_count_bounds_time(r, lo, hi, 1200.0, 1700.0, C.byref(m), C.byref(s)) == 0, q.err()
                out.append((m.value, s.value))
            return out

        before = old()
        assert before[0] == single[EVERY] and 0 < before[1][0] < before[0][0] and 0 < before[2][0] < before[0][0]
        for nboxes in (17, 3):
            rc, m, s, read = q.many(r, BOXES[:nboxes])
            assert rc == 0, q.err()
            assert m == [x[0] for x in single[:nboxes]] and s == [x[1] for x in single[:nboxes]]
            assert read == expected_read(held, BOXES[:nboxes])
        assert old() == before
    finally:
        q.lib.pcq_query_resident_free(r)
