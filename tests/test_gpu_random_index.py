"""Seeded random parity of the four indexed entries with numpy (_index_chunks.py: draw; its seeds are proven on the CPU by
test_index_chunks_plan.py).  PCQ_TEST_SEED_BASE moves the whole seed range for a soak run.

Per seed: 1 to 40 chunks and a tail are uploaded once, and ONE index object serves all five kinds in an order drawn from the
seed, so the boxes, the histograms and the time records are built by whichever kind needs them first and shared by the others.
Every query runs three times — a count collector on the kind's indexed entry, a count collector on pcq_scan_dev, a buffer
collector on the indexed entry — and every count and every record is numpy's, the records byte for byte.  After every covered
query the statistics are exact: chunks = n // 4096 (class: ceil(n / 65536)), (skipped, whole, scanned) the model's, built = 1
only on the call that built a part; the call that builds a one-part kind's part reads every chunk (scanned = chunks) and a class
count is answered from the histograms (whole = chunks), as include/pcq.h says.  Each kind's last query is one the plan sends to
the plain scan — for box AND time a predicate that can match nothing, for the others (whose plans cover every predicate)
columns without a whole chunk or with every second class byte — and must leave all-zero statistics: a silent fall-through of
any other query fails.
"""
import importlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _index_chunks as ic  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
POINT_DTYPE = binding.POINT_DTYPE


def records_of(ctx, kind, cols, pred, ix):
    gb = ctx.buffer_collector()
    try:
        ic.indexed_entry(ctx, kind)(cols, pred, ix, gb)
        pts = gb.points()
        assert gb.point_count() == len(pts)
        return pts.tobytes()
    finally:
        gb.free()


@pytest.mark.parametrize("seed", ic.SEEDS)
def test_every_kind_through_one_index_against_numpy(gpu_ctx, seed):
    ctx = gpu_ctx
    c = ic.case(seed)
    d = c.data
    phase = seed % 16  # the class bytes at any alignment
    blocks = [ctx.alloc(a.nbytes + 64) for a in (d.xyz, d.cls, d.t)]
    ix = ctx.index_new()
    built = set()
    try:
        d_xyz, d_cls, d_t = blocks[0], blocks[1] + phase, blocks[2]
        assert d_xyz % 16 == 0 and d_t % 16 == 0
        for ptr, a in zip((d_xyz, d_cls, d_t), (d.xyz, d.cls, d.t)):
            ctx.to_device(ptr, a)
        for kind in c.order:
            for q in c.queries[kind]:
                what = f"seed {seed} (PCQ_TEST_SEED_BASE {ic.SEED_BASE}), n {c.n}, {kind} {q}"
                asked = ic.columns_of(q, d)
                cols = ic.columns(binding, kind, d_xyz, d_cls, d_t, asked.n, q.cls_stride)
                pred = ic.predicate(pkg.Predicate, q)
                sel = ic.select(kind, asked, q)
                is_covered = ic.covered(q, c.n)
                assert is_covered == (q is not c.queries[kind][-1])
                got = ic.count_of(ctx, kind, cols, pred, ix)
                st = ctx.index_stats(ix)
                assert got == int(sel.sum()), (what, got, int(sel.sum()))
                if is_covered:
                    assert st == ic.expected_stats(q, d, built, count=True), (what, st)
                else:
                    assert not any(st.values()), (what, st)
                assert ic.count_of(ctx, kind, cols, pred) == got, what
                rec = records_of(ctx, kind, cols, pred, ix)
                st = ctx.index_stats(ix)
                assert rec == ic.expect_records(kind, asked.xyz, asked.cls, sel, POINT_DTYPE).tobytes(), what
                if is_covered:
                    assert st == ic.expected_stats(q, d, built, count=False), (what, st)
                    assert st["chunks"] == ic.chunks_of(kind, c.n) and st["built"] == 0
                else:
                    assert not any(st.values()), (what, st)
        assert built == {"boxes", "hist", "times"}
    finally:
        ctx.index_free(ix)
        for b in blocks:
            ctx.free(b)
