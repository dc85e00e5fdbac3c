"""All twelve batched kinds on one context: every kind after every kind, read call by call or only at the end.

Box, class, box AND class, box AND time, multi-box, class histogram, time histogram and density raster share the context's
segment table, partials and scratch stream (_batch_all_kinds.py).  A sequence of 65 calls holds every one of the 64 ordered
pairs of these eight kinds; the segment set alternates between 7 and 23 segments from call to call, one segment's predicate
changes from one visit of a kind to its next, and so do nqueries, the edges, the raster's shape and the cell widths.  Every call
adds into a region of its own, preset to distinct non-zero words: the difference is numpy's answer over the kind's words (1,
nqueries, 256, nbins or nx * ny) and nothing behind them.

A second sequence of 158 calls does the same for all twelve kinds, with the height raster, the mean-height raster, its
class-filtered twin and the polygon count: 145 calls hold the 144 ordered pairs, and thirteen more hold what no pair of visits
gives by itself (plan12).  The height raster folds, so its regions are preset on both sides of the data; the mean-height rasters
write two arrays.

read="each" reads a call's region before the next call (what every other batch test does).  read="end" issues all calls
back to back on the context's stream, without a host read or a synchronisation of the test's in between, and reads once.
The library itself serialises here: every call's table differs from the one in HBM, so pcq_upload_segment_table waits for the
stream before it touches the pinned table, and pcq_ensure_partials waits for the device before it frees.  What this mode
pins is that those waits of the library's are enough when the test adds none: a table of another layout, a regrown table
or regrown partials, or another slice count never reach a launch that has not run.  A launch that really stays queued (an
identical repeat, which uploads nothing) is the matter of test_gpu_batch_streams.py — and of the seven calls of the second
sequence that share one raster table byte for byte: three kernels, three finishes and three slice counts over one upload.

The time histogram's last visit (call 64) repeats call 63 — the same set, the same predicates, the same edges — with one
edge moved by one ulp: the upload's compare has to see one bit behind the table.

Each test has a context of its own, so the table buffer and the partials start at their first sizes.
"""
import sys
import time

import numpy as np
import pytest

import _batch_all_kinds as ak
from _batch_all_kinds import KINDS, KINDS8, LARGE, MULTI, NAMES, ORDER, ORDER12, POLYGON, RASTER, SMALL, TAIL, TIME_HIST, ZRANGE, ZSUM, ZSUM_CLASSES

pytestmark = pytest.mark.gpu

CHAIN = slice(len(ORDER12) - len(TAIL), len(ORDER12) - len(TAIL) + 7)  # the calls over one raster table
BODY = len(ORDER12) - len(TAIL)


def plan():
    """The query of every call: the kind's next visit, on the small set at even calls and the large one at odd calls; the time
    histogram's one-ulp visit stays on its predecessor's set, with its predecessor's predicates"""
    visits, out = [0] * len(KINDS8), []
    for call, kind in enumerate(ORDER):
        if kind == ak.TIME_HIST and visits[kind] == ak.ULP_VISIT:
            assert ORDER[call - 1] == kind and out[-1].visit == ak.ULP_VISIT - 1
            out.append(ak.query(kind, out[-1].set, ak.ULP_VISIT, ak.ULP_VISIT - 1))
        else:
            out.append(ak.query(kind, call % 2, visits[kind]))
        visits[kind] += 1
    return out


def plan12():
    """The query of every call of the second sequence.  The first 145: the kind's next visit, on the small set at even calls and
    the large one at odd calls (the time histogram's one-ulp visit, which belongs behind its predecessor, is left out).  Then
    - seven calls of the three kinds that share PCQ_SEGMENTS_RASTER on the large set, with the predicates of one visit, a z slab
      included, and one shape: their tables are equal byte for byte, so only the first of them uploads;
    - the class-filtered mean-height raster twice with one table and two class sets;
    - polygon, time histogram, polygon on the large set: three trailers of three sizes behind three tables;
    - the last polygon call again with vertex 1 of one segment's outline moved along its horizontal edge: one edge of the trailer
      changes, the number of edges does not."""
    visits, out = [0] * len(KINDS), []
    for call, kind in enumerate(ORDER12[:BODY]):
        if kind == TIME_HIST and visits[kind] == ak.ULP_VISIT:
            visits[kind] += 1
        out.append(ak.query(kind, call % 2, visits[kind]))
        visits[kind] += 1
    at = max(visits[RASTER], visits[ZRANGE], visits[ZSUM])
    for kind in TAIL[:7]:
        out.append(ak.query(kind, LARGE, visits[kind], at, shape=ak.CHAIN_SHAPE, slab=True))
        visits[kind] += 1
    one = -(-visits[ZSUM_CLASSES] // len(ak.CLASS_SETS)) * len(ak.CLASS_SETS)  # (the sets of one class and of all but two)
    out += [ak.query(ZSUM_CLASSES, SMALL, one, one, shape=ak.CHAIN_SHAPE), ak.query(ZSUM_CLASSES, SMALL, one + 3, one, shape=ak.CHAIN_SHAPE)]
    out += [ak.query(POLYGON, LARGE, visits[POLYGON]), ak.query(TIME_HIST, LARGE, visits[TIME_HIST]), ak.query(POLYGON, LARGE, visits[POLYGON] + 1),
            ak.query(POLYGON, LARGE, visits[POLYGON] + 1, moved=True)]
    assert tuple(q.kind for q in out) == ORDER12
    return out


def describe(call, q, order=ORDER):
    after = NAMES[order[call - 1]] if call else None
    return f"call {call}: kind {NAMES[q.kind]} after kind {after}, visit {q.visit}, set {('small', 'large')[q.set]}"


def test_the_order_holds_every_ordered_pair_and_the_queries_tell_calls_apart():
    assert len(ORDER) == 65 and set(zip(ORDER, ORDER[1:])) == {(a, b) for a in KINDS8 for b in KINDS8}
    queries = plan()
    for q in queries:
        ak.check_not_vacuous(q)
    assert {(q.kind, q.set) for q in queries} == {(k, s) for k in KINDS8 for s in (SMALL, LARGE)}  # every kind on both sets
    assert {q.words for q in queries if q.kind == MULTI} == set(range(1, 9))
    # the one-ulp visit differs from the call before it in one edge and in nothing else: same set, same predicates, same size
    last, ulp = queries[-2], queries[-1]
    assert (ulp.kind, ulp.visit, ulp.set, ulp.varied, ulp.table_bytes) == (ak.TIME_HIST, ak.ULP_VISIT, last.set, last.visit, last.table_bytes)
    assert [bytes(p) for p in ulp.args[0]] == [bytes(p) for p in last.args[0]] and (ulp.args[1] != last.args[1]).sum() == 1
    # the multi-box table of the large set outgrows the table buffer's first size; the small set's does not
    assert ak.PITCH[MULTI] * len(ak.SET_SIZES[LARGE]) > ak.TABLE_BYTES_INITIAL >= ak.PITCH[MULTI] * len(ak.SET_SIZES[SMALL])
    assert any(q.kind == MULTI and q.set == LARGE and q.table_bytes > ak.TABLE_BYTES_INITIAL for q in queries)
    # ... and does so before any table with 1024 edges behind it
    first_multi = min(c for c, q in enumerate(queries) if q.kind == MULTI and q.set == LARGE and q.table_bytes > ak.TABLE_BYTES_INITIAL)
    assert all(q.table_bytes <= ak.TABLE_BYTES_INITIAL for q in queries[:first_multi])


def test_the_second_order_holds_every_ordered_pair_of_the_twelve_and_its_tail_holds_the_shared_tables():
    assert len(ORDER12) == 158 and set(zip(ORDER12[:BODY], ORDER12[1:BODY])) == {(a, b) for a in KINDS for b in KINDS}
    queries = plan12()
    for q in queries:
        ak.check_not_vacuous(q)
    assert {(q.kind, q.set) for q in queries[:BODY]} == {(k, s) for k in KINDS for s in (SMALL, LARGE)}  # every kind on both sets
    # the launch-level parameters the new kinds are asked with
    shapes = {k: {tuple(q.args[2:4]) for q in queries if q.kind == k} for k in (ZRANGE, ZSUM, ZSUM_CLASSES)}
    assert {(64, 64), (1, 1), (3, 5), (1, 37)} <= shapes[ZRANGE] and max(x * y for x, y in shapes[ZRANGE]) == ak.ZRANGE_CELLS_MAX
    assert (64, 32) in shapes[ZSUM] and (64, 32) in shapes[ZSUM_CLASSES] and max(x * y for x, y in shapes[ZSUM]) == ak.ZSUM_CELLS_MAX
    sets = {tuple(q.args[4]) for q in queries if q.kind == ZSUM_CLASSES}
    assert {(2,), tuple(range(256)), (0, 255), tuple(c for c in range(256) if c not in (1, 2))} <= sets
    polygons = [q for q in queries if q.kind == POLYGON]
    assert {3, 4, 5, 255, 256} <= {len(q.args[1][0]) for q in polygons}
    assert all(a.table_bytes != b.table_bytes for a, b in zip(polygons[:-1], polygons[1:-1]))  # the trailer's size changes from visit to visit
    # on the large set with 256 vertices the table with its trailer outgrows the table buffer, whatever came before
    big = [q for q in polygons if q.set == LARGE and len(q.args[1][0]) == ak.POLYGON_VERTS_MAX]
    assert big and big[0].table_bytes == max(q.table_bytes for q in queries) > ak.TABLE_BYTES_INITIAL
    assert big[0].table_bytes == (ak.PITCH[POLYGON] + 16 * 256) * len(ak.SET_SIZES[LARGE])

    # seven calls over one raster table: RASTER -> ZRANGE -> ZSUM -> RASTER, and ZSUM -> ZRANGE, ZRANGE -> RASTER
    chain = queries[CHAIN]
    assert [q.kind for q in chain] == [RASTER, ZRANGE, ZSUM, RASTER, ZSUM, ZRANGE, RASTER]
    assert {(a.kind, b.kind) for a, b in zip(chain, chain[1:])} >= {(RASTER, ZRANGE), (ZRANGE, ZSUM), (ZSUM, RASTER), (ZSUM, ZRANGE), (ZRANGE, RASTER)}
    tables = [ak.raster_table(q) for q in chain]
    assert all(t == tables[0] for t in tables) and len(tables[0]) == 72 * len(ak.SET_SIZES[LARGE])
    assert all(q.set == chain[0].set and tuple(q.args[2:4]) == ak.CHAIN_SHAPE and q.args[1] == chain[0].args[1] for q in chain)
    assert all([bytes(p) for p in q.args[0]] == [bytes(p) for p in chain[0].args[0]] for q in chain)
    assert ak.CHAIN_SHAPE[0] * ak.CHAIN_SHAPE[1] <= ak.ZSUM_CELLS_MAX
    assert ak.raster_table(queries[CHAIN.start - 1]) != tables[0] if queries[CHAIN.start - 1].kind in (RASTER, ZRANGE, ZSUM) else True
    assert len({q.slices for q in chain}) == 2 and chain[2].slices == 2 * chain[0].slices  # (the partials are laid out anew from call to call)
    # one table, one answer: the density raster's words are the mean-height raster's counts, and the cells it reaches the height raster's
    assert np.array_equal(chain[0].want, chain[2].want[:chain[0].words]) and chain[2].want[chain[0].words:].any()
    assert np.array_equal(chain[0].want > 0, chain[1].want[:chain[0].words] <= chain[1].want[chain[0].words:]) and 0 < (chain[0].want > 0).sum() < chain[0].words

    # the class-filtered table twice, with two sets
    a, b = queries[CHAIN.stop:CHAIN.stop + 2]
    assert a.kind == b.kind == ZSUM_CLASSES and a.set == b.set and a.table_bytes == b.table_bytes and a.args[1:4] == b.args[1:4]
    assert [bytes(p) for p in a.args[0]] == [bytes(p) for p in b.args[0]]
    assert set(a.args[4]) != set(b.args[4]) and a.want.any() and b.want.any() and not np.array_equal(a.want, b.want)

    # POLYGON -> TIME_HIST -> POLYGON: three trailers of three sizes
    p1, th, p2, moved = queries[CHAIN.stop + 2:]
    assert (p1.kind, th.kind, p2.kind, moved.kind) == (POLYGON, TIME_HIST, POLYGON, POLYGON)
    trailers = [16 * len(p1.args[1]) * len(p1.args[1][0]), 8 * (len(th.args[1]) + 1), 16 * len(p2.args[1]) * len(p2.args[1][0])]
    assert len(set(trailers)) == 3 and [p1.table_bytes, th.table_bytes, p2.table_bytes] == [
        ak.PITCH[q.kind] * len(ak.SET_SIZES[q.set]) + t for q, t in zip((p1, th, p2), trailers)]

    # two polygon visits that differ in one vertex, which changes one edge; the same number of edges
    assert (moved.set, moved.table_bytes) == (p2.set, p2.table_bytes) and [bytes(p) for p in moved.args[0]] == [bytes(p) for p in p2.args[0]]
    differ = [k for k, (u, v) in enumerate(zip(p2.args[1], moved.args[1])) if u != v]
    assert differ == [ak.VARIED]
    u, v = p2.args[1][ak.VARIED], moved.args[1][ak.VARIED]
    assert [j for j in range(len(u)) if u[j] != v[j]] == [1]
    eu, ev = ak.travelling_edges(u), ak.travelling_edges(v)
    assert len(eu) == len(ev) and sum(x != y for x, y in zip(eu, ev)) == 1
    assert moved.want[0] != p2.want[0]


def run(queries, order, read):
    """The calls on a context of its own; returns (Dev's regrowths of the table buffer, of the partials)"""
    began = time.perf_counter()
    ctx = ak.pkg.Context(0)
    try:
        dev = ak.Dev(ctx, queries)
        try:
            cus = ctx.device_info()["compute_units"]
            tables, partials = ak.regrowths(dev, queries, cus)
            print(f"\n{cus} CUs; the table buffer regrows at (call, bytes) {tables}; the partials at (call, words asked, words) {partials}",
                  file=sys.stderr)
            failures = []
            ready = time.perf_counter()
            if read == "each":
                for call, q in enumerate(queries):
                    dev.launch(q, call)
                    bad = dev.wrong(dev.region(call), q, call)
                    assert bad is None, f"{describe(call, q, order)}: {bad}"
            else:
                for call, q in enumerate(queries):
                    dev.launch(q, call)
                issued = time.perf_counter()
                words = dev.regions()
                print(f"read=end: context and upload {1e3 * (ready - began):.1f} ms, {len(queries)} calls {1e3 * (issued - ready):.1f} ms, "
                      f"the read {1e3 * (time.perf_counter() - issued):.1f} ms", file=sys.stderr)
                for call, q in enumerate(queries):
                    bad = dev.wrong(words[call], q, call)
                    if bad is not None:
                        failures.append(f"{describe(call, q, order)}: {bad}")
                assert not failures, f"{len(failures)} of {len(queries)} calls wrong, the first: {failures[0]}"
        finally:
            dev.free()
    finally:
        ctx.close()
    print(f"read={read}: {1e3 * (time.perf_counter() - began):.1f} ms", file=sys.stderr)
    return tables, partials


@pytest.mark.parametrize("read", ["each", "end"])
def test_every_kind_after_every_kind_on_one_context(read):
    queries = plan()
    tables, partials = run(queries, ORDER, read)
    assert any(queries[call].kind == MULTI for call, _ in tables), "no multi-box table outgrows the table buffer"
    assert any(call > 0 for call, _, _ in partials), "the partials never regrow behind the first call"


@pytest.mark.parametrize("read", ["each", "end"])
def test_every_kind_of_the_twelve_after_every_kind_on_one_context(read):
    queries = plan12()
    tables, partials = run(queries, ORDER12, read)
    assert any(queries[call].kind == POLYGON and len(queries[call].args[1][0]) == 256 for call, _ in tables), \
        "no polygon table of 256 vertices outgrows the table buffer"
    assert any(queries[call].kind in (ZRANGE, ZSUM, ZSUM_CLASSES) for call, _, _ in partials), "no height or mean-height raster makes the partials regrow"
