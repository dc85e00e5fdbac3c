"""What keeps test_gpu_world_box.py honest, without a GPU: the reference of _world_box.py against the oracle's LAZER search
on every finite corpus the GPU cases use, the conditions under which a case can fail at all (a contracted rebuild gives
another count and other records, with points that change sides in every range the case names), the collision box, and
the non-finite and degenerate cases against masks written out by hand."""
import numpy as np
import pytest

import _world_box as wb
from _collector_model import feed

CASES = wb.face_cases()
IDS = [c.name for c in CASES]
MI355X_CUS = 256  # (the GPU test takes the number from device_info(); the construction is checked here for this one)


def oracle_check(oracle, corpus, box, block=4096, grid=True):
    """answer() against oracle.search_lazer_bounds on the corpus as a LAZER image: count, record bytes, grid cells and winners
    (grid=False: a corpus that only the count and buffer collectors see)."""
    wmin, wmax = box
    assert oracle.aabb_intersects(list(corpus.hdr.min), list(corpus.hdr.max), wmin, wmax)  # (the early-out does not answer for the scan)
    lz = corpus.lazer(oracle, block)
    a = wb.answer(corpus, box)
    oc, ob = oracle.count_collector(), oracle.buffer_collector()
    og, fed = oracle.grid_collector(*wb.GRID_BOX, wb.GRID_CELL), oracle.grid_collector(*wb.GRID_BOX, wb.GRID_CELL)
    try:
        for c in (oc, ob, og) if grid else (oc, ob):
            assert oracle.search_lazer_bounds(lz, wmin, wmax, c) == 0, oracle.err()
        assert oc.point_count() == a.count
        assert ob.points().tobytes() == a.records.tobytes()
        if grid:
            feed(fed, a.records)
            assert np.array_equal(fed.grid_cells(), og.grid_cells()) and fed.points().tobytes() == og.points().tobytes()
    finally:
        for c in (oc, ob, og, fed):
            c.free()
    return a


def non_vacuous(corpus, case, ranges):
    """The stated condition: a restatement with fused() gives another count and other records than the reference, at
    least 8 points change sides, and every named range holds some of them (the case's copies; two to a range)."""
    a, f = wb.answer(corpus, case), wb.answer(corpus, case, restated="fused")
    changed = np.flatnonzero(a.mask ^ f.mask)
    assert a.count != f.count and a.records.tobytes() != f.records.tobytes(), case.name
    assert len(changed) >= 8 and np.isin(corpus.placed, changed).all(), (case.name, len(changed))
    assert (a.mask[corpus.placed] == case.kept).all()  # kept by the reference where the face is the two-rounding value
    for name, (first, end) in ranges.items():
        assert int(((changed >= first) & (changed < end)).sum()) >= 2, (case.name, name)
    # every face of the box holds a point exactly on it: an inclusive compare turned exclusive loses a match
    w = corpus.world()[a.idx]
    for ax in range(3):
        for side, face in (("min", case.wmin[ax]), ("max", case.wmax[ax])):
            assert (w[:, ax] == face).any() or ((ax, side) == (case.axis, case.side) and not case.kept), (case.name, ax, side)
    return a


def test_the_headers_have_sensitive_integers_of_both_signs():
    for a in range(3):
        xs = np.arange(wb.LO[a], wb.LO[a] + wb.SPAN[a])
        idx, sign = wb.sensitive(xs, wb.SCALE[a], wb.OFFSET[a])
        print("axis", a, "sensitive", len(idx), "of", len(xs), "fused above", int((sign > 0).sum()), "below", int((sign < 0).sum()))
        assert len(idx) > len(xs) // 20 and (sign > 0).sum() > 50 and (sign < 0).sum() > 50
        two = np.array([wb.two_roundings(x, wb.SCALE[a], wb.OFFSET[a]) for x in xs[idx]])
        one = np.array([wb.fused(x, wb.SCALE[a], wb.OFFSET[a]) for x in xs[idx]])
        assert np.all(np.abs(one - two) <= 2.0 ** -44)  # the last places (far less than a step of the scale: no other integer comes near)
    w = wb.world(np.array([[7, -3, 11]]), wb.SCALE, wb.OFFSET)[0]
    assert tuple(w) == tuple(wb.two_roundings(v, s, o) for v, s, o in zip((7, -3, 11), wb.SCALE, wb.OFFSET))
    assert len({c.x for c in CASES}) == 12 and all(c.face == (c.two if c.kept else c.fused) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_count_corpora(oracle, case):
    corpus, ranges = wb.count_corpus(oracle, case)
    oracle_check(oracle, corpus, (case.wmin, case.wmax))
    non_vacuous(corpus, case, ranges)
    big, ranges = wb.second_trip_corpus(oracle, case, MI355X_CUS)
    assert big.n > 2 * 4 * 256 * MI355X_CUS
    oracle_check(oracle, big, (case.wmin, case.wmax), block=65536, grid=False)
    non_vacuous(big, case, ranges)


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_buffer_corpora(oracle, case, colour):
    corpus, ranges = wb.buffer_corpus(oracle, case, colour)
    a = non_vacuous(corpus, case, ranges)
    oracle_check(oracle, corpus, (case.wmin, case.wmax), block=1000)
    # the three whole tiles hold what their writers take, under the reference and under the restatement alike
    for mask in (a.mask, wb.answer(corpus, case, restated="fused").mask):
        per_tile = np.add.reduceat(mask.astype(np.int64), np.arange(0, corpus.n, wb.EMIT_TILE))
        assert 18 <= per_tile[1] <= 22 and 278 <= per_tile[2] <= 282 and per_tile[0] > 300 and 0 < per_tile[3], per_tile
        for (sparse_max, park_max), writers in wb.BUFFER_SETTINGS.items():
            got = tuple("parked" if m <= park_max else "sparse" if m <= sparse_max else "dense" for m in per_tile[:3])
            assert got == writers, (sparse_max, park_max, per_tile)
    assert {w for ws in wb.BUFFER_SETTINGS.values() for w in ws} == {"parked", "sparse", "dense"}


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_grid_corpora(oracle, case, colour):
    corpus, ranges = wb.grid_corpus(oracle, case, colour)
    a = oracle_check(oracle, corpus, (case.wmin, case.wmax))
    non_vacuous(corpus, case, ranges)
    # ... and the grid notices: fed the restatement's records, the oracle's grid holds other winners
    g, h = oracle.grid_collector(*wb.GRID_BOX, wb.GRID_CELL), oracle.grid_collector(*wb.GRID_BOX, wb.GRID_CELL)
    try:
        feed(g, a.records)
        feed(h, wb.answer(corpus, case, restated="fused").records)
        assert 100 < g.point_count() < a.count
        assert g.points().tobytes() != h.points().tobytes(), case.name
    finally:
        g.free(), h.free()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layout_and_host_corpora(oracle, case):
    corpus, ranges = wb.layout_corpus(oracle, case)
    oracle_check(oracle, corpus, (case.wmin, case.wmax), block=2048)
    non_vacuous(corpus, case, ranges)
    # the same columns as AoS records: positions, class and colour where the format has them
    for fmt in (0, 2, 3, 5):
        rl, _, coff, kof = wb.ti.FORMATS[fmt]
        rec = corpus.las_records(fmt)
        assert rec.shape == (corpus.n, rl) and np.array_equal(rec[:, :12].copy().view("<i4"), corpus.xyz) and np.array_equal(rec[:, kof], corpus.cls)
        assert coff is None or np.array_equal(rec[:, coff:coff + 6].copy().view("<u2"), corpus.rgb)
    if case.sign < 0 and case.side == "min":  # one case per axis goes through the host entries
        host, ranges = wb.host_corpus(oracle, case)
        oracle_check(oracle, host, (case.wmin, case.wmax))
        non_vacuous(host, case, ranges)
        for cp in wb.HOST_CHUNK_POINTS:
            for bpp in (12, 13, 19):
                c = wb.host_chunks(cp, bpp, host.n)
                assert c < host.n and {c - 1, c} <= set(host.placed.tolist()), (cp, bpp, c)


def test_collision_box_keeps_several_integers(oracle):
    corpus, box = wb.collision_corpus(oracle)
    a = oracle_check(oracle, corpus, box)
    xs = np.unique(corpus.xyz[a.idx, 0])
    print(len(xs), "distinct integers from", xs.min(), "to", xs.max(), "share", box[0][0], ":", a.count, "points")
    assert len(xs) >= 3 and xs.min() <= 1234 <= xs.max() and a.count >= 8
    assert len(np.unique(corpus.world()[a.idx, 0])) == 1
    assert not a.mask.all()


# which of the sixteen points each case keeps, worked out by hand from the rule (point k lies at (10, 20, 30) + SIXTEEN[k] / 2
# under the plain header; see the comments)
BY_HAND = {
    "plain box": {0, 1, 2, 4, 5, 6},                          # [10, 12] x [20, 22] x [30, 32], faces inclusive
    "NaN scale on x": {0, 1, 2, 4, 5, 6, 7, 10, 15},           # x is NaN everywhere (NaN * 0 too): only y and z decide
    "NaN offset on y": {0, 1, 2, 4, 5, 6, 8, 11, 14},          # y is NaN everywhere: only x and z decide
    "NaN min face on z": {0, 1, 2, 4, 5, 6, 12, 13},           # z has no lower face: 12 (z 27) and 13 (z 29) come in
    "NaN max face on x": {0, 1, 2, 4, 5, 6, 7},                # x has no upper face: 7 (x 13) comes in
    "all faces infinite": set(range(16)),
    "some faces infinite": {0, 1, 2, 4, 5, 6, 8, 10, 15},      # x <= 12, y >= 20, z in [30, 32]
    "min above max on x": set(),                              # every x is below 12 or above 10; nothing panics
    "min equals max on a point": {1},
    "scale 0 on z": {0, 1, 2, 4, 5, 6, 9, 12, 13},             # z is 30 everywhere: only x and y decide
    "scale inf on x": {0, 5, 6},                              # x = 0 gives NaN (kept), any other x +-inf; then y and z
    "offset -0.0, faces +0.0": {0, 5, 6},                      # x = 0 gives -0.0, which is neither below nor above +0.0
    "i32 extremes on the faces": {0, 1, 4, 5, 6, 7, 10},       # +-2147483647.5 lie on the x faces
    "i32 extremes one step outside": {0, 1, 4, 5, 6},
}


@pytest.mark.parametrize("name", list(wb.SPECIAL))
def test_special_cases_by_hand(name):
    points, scale, offset, wmin, wmax = wb.SPECIAL[name]
    assert set(BY_HAND) == set(wb.SPECIAL)
    w = wb.world(points, scale, offset)
    got = wb.keeps(w, wmin, wmax)
    assert set(np.flatnonzero(got).tolist()) == BY_HAND[name], name
    if name == "offset -0.0, faces +0.0":
        assert np.signbit(w[0, 0]) and w[0, 0] == 0.0
    if name == "scale inf on x":
        assert np.isnan(w[0, 0]) and w[1, 0] == np.inf and w[3, 0] == -np.inf
    if name.startswith("i32 extremes"):
        assert w[7, 0] == 2147483647.5 and w[10, 0] == -2147483647.5
    # the rule of the Python model the lifecycle scenarios use is this one
    import _collector_model as cm
    ds = cm.Dataset("d", points, np.zeros(16, np.uint8), np.zeros((16, 3), np.uint16), np.zeros(16), scale, offset)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(cm.select(ds, {"kind": "BOUNDS_F64", "wmin": list(wmin), "wmax": list(wmax)}), got)
