"""All eight batched kinds on one context: every kind after every kind, read call by call or only at the end.

Box, class, box AND class, box AND time, multi-box, class histogram, time histogram and density raster share the context's
segment table, partials and scratch stream (_batch_all_kinds.py).  A sequence of 65 calls holds every one of the 64 ordered
pairs of kinds; the segment set alternates between 7 and 23 segments from call to call, one segment's predicate changes from
one visit of a kind to its next, and so do nqueries, the edges, the raster's shape and the cell widths.  Every call adds into
a region of its own, preset to distinct non-zero words: the difference is numpy's answer over the kind's words (1, nqueries,
256, nbins or nx * ny) and nothing behind them.

read="each" reads a call's region before the next call (what every other batch test does).  read="end" issues all 65 calls
back to back on the context's stream, without a host read or a synchronisation of the test's in between, and reads once.
The library itself serialises here: every call's table differs from the one in HBM, so pcq_upload_segment_table waits for the
stream before it touches the pinned table, and pcq_ensure_partials waits for the device before it frees.  What this mode
pins is that those waits of the library's are enough when the test adds none: a table of another layout, a regrown table
or regrown partials, or another slice count never reach a launch that has not run.  A launch that really stays queued (an
identical repeat, which uploads nothing) is the matter of test_gpu_batch_streams.py.

The time histogram's last visit (call 64) repeats call 63 — the same set, the same predicates, the same edges — with one
edge moved by one ulp: the upload's compare has to see one bit behind the table.

Each test has a context of its own, so the table buffer and the partials start at their first sizes.
"""
import sys
import time

import pytest

import _batch_all_kinds as ak
from _batch_all_kinds import KINDS, LARGE, MULTI, NAMES, ORDER, SMALL

pytestmark = pytest.mark.gpu


def plan():
    """The query of every call: the kind's next visit, on the small set at even calls and the large one at odd calls; the time
    histogram's one-ulp visit stays on its predecessor's set, with its predecessor's predicates"""
    visits, out = [0] * len(KINDS), []
    for call, kind in enumerate(ORDER):
        if kind == ak.TIME_HIST and visits[kind] == ak.ULP_VISIT:
            assert ORDER[call - 1] == kind and out[-1].visit == ak.ULP_VISIT - 1
            out.append(ak.query(kind, out[-1].set, ak.ULP_VISIT, ak.ULP_VISIT - 1))
        else:
            out.append(ak.query(kind, call % 2, visits[kind]))
        visits[kind] += 1
    return out


def describe(call, q):
    after = NAMES[ORDER[call - 1]] if call else None
    return f"call {call}: kind {NAMES[q.kind]} after kind {after}, visit {q.visit}, set {('small', 'large')[q.set]}"


def test_the_order_holds_every_ordered_pair_and_the_queries_tell_calls_apart():
    assert len(ORDER) == 65 and set(zip(ORDER, ORDER[1:])) == {(a, b) for a in KINDS for b in KINDS}
    queries = plan()
    for q in queries:
        ak.check_not_vacuous(q)
    assert {(q.kind, q.set) for q in queries} == {(k, s) for k in KINDS for s in (SMALL, LARGE)}  # every kind on both sets
    assert {q.words for q in queries if q.kind == MULTI} == set(range(1, 9))
    # the one-ulp visit differs from the call before it in one edge and in nothing else: same set, same predicates, same size
    last, ulp = queries[-2], queries[-1]
    assert (ulp.kind, ulp.visit, ulp.set, ulp.varied, ulp.table_bytes) == (ak.TIME_HIST, ak.ULP_VISIT, last.set, last.visit, last.table_bytes)
    assert [bytes(p) for p in ulp.args[0]] == [bytes(p) for p in last.args[0]] and (ulp.args[1] != last.args[1]).sum() == 1
    # the multi-box table of the large set outgrows the table buffer's first size; the small set's does not
    assert ak.PITCH[MULTI] * len(ak.SET_SIZES[LARGE]) > ak.TABLE_BYTES_INITIAL >= ak.PITCH[MULTI] * len(ak.SET_SIZES[SMALL])
    assert any(q.kind == MULTI and q.set == LARGE and q.table_bytes > ak.TABLE_BYTES_INITIAL for q in queries)


@pytest.mark.parametrize("read", ["each", "end"])
def test_every_kind_after_every_kind_on_one_context(read):
    began = time.perf_counter()
    queries = plan()
    ctx = ak.pkg.Context(0)
    try:
        dev = ak.Dev(ctx, len(queries))
        try:
            cus = ctx.device_info()["compute_units"]
            tables, partials = ak.regrowths(dev, queries, cus)
            print(f"\n{cus} CUs; the table buffer regrows at (call, bytes) {tables}; the partials at (call, words asked, words) {partials}",
                  file=sys.stderr)
            assert any(queries[call].kind == MULTI for call, _ in tables), "no multi-box table outgrows the table buffer"
            assert any(call > 0 for call, _, _ in partials), "the partials never regrow behind the first call"
            failures = []
            ready = time.perf_counter()
            if read == "each":
                for call, q in enumerate(queries):
                    dev.launch(q, call)
                    bad = dev.wrong(dev.region(call), q, call)
                    assert bad is None, f"{describe(call, q)}: {bad}"
            else:
                for call, q in enumerate(queries):
                    dev.launch(q, call)
                issued = time.perf_counter()
                words = dev.regions()
                print(f"read=end: context and upload {1e3 * (ready - began):.1f} ms, 65 calls {1e3 * (issued - ready):.1f} ms, "
                      f"the read {1e3 * (time.perf_counter() - issued):.1f} ms", file=sys.stderr)
                for call, q in enumerate(queries):
                    bad = dev.wrong(words[call], q, call)
                    if bad is not None:
                        failures.append(f"{describe(call, q)}: {bad}")
                assert not failures, f"{len(failures)} of {len(queries)} calls wrong, the first: {failures[0]}"
        finally:
            dev.free()
    finally:
        ctx.close()
    print(f"read={read}: {1e3 * (time.perf_counter() - began):.1f} ms", file=sys.stderr)
