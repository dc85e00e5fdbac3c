"""The chunk index with more chunks than workgroups (_index_chunks.py, proven on the CPU by test_index_chunks_plan.py).

One upload of the big set, sized from the device's compute units: C = 2 * 8 * CUs + 37 chunks of 4096 points and a tail of 1234, so
that every workgroup of the index's grid (min(chunks, 8 * CUs)) goes round `for (ch = blockIdx.x; ch < nchunks; ch += gridDim.x)`
twice and 37 go round three times: in the builders (k_index_build_bounds, k_index_build_time: s_mn / s_mx reused behind the
barriers), in the pruned counts (k_index_count_bounds, _bounds_class, _bounds_time, k_index_count_time: a workgroup that skips,
counts whole and scans in one launch, thread 0's `total += CHUNK_POINTS` on a later trip) and in the finish over 8 * CUs partials.
k_index_emit_stats runs with several blocks.  Per kind, through its own entry and on one index object: the building call and
every later query with a count collector, against numpy and the model's exact (skipped, whole, scanned); the same on the first
grid * 4096 points alone through a second index object, which fails only where the first trip is wrong — together they tell a bad
stride from a bad body; and the queries of at most 2 % matches with ONE buffer collector, every scan's records behind the ones
before, byte for byte, with the statistics k_index_emit_stats classifies.  A class count is answered from the histograms
(include/pcq.h: whole = chunks), so the class kind's exact statistics are those of its buffer scans.

The smallest set at which an assertion can still fail: a full launch differs from its first trip from grid + 1 chunks on, a stride
that is wrong only from its second application on needs 2 * grid + 1; this set has 2 * grid + 37.  The class histograms' builder
has one workgroup per 65536 points, so its second trip needs the class-only set: 8 * CUs + 37 class chunks and a partial one (a
third trip would double the upload for a loop whose body does not depend on the trip).  There k_index_count_class's one block of
256 threads strides over the chunks nine times at 256 CUs.  The positions of its one buffer scan are written on the device.

Not covered: the second pass of k_index_emit_stats's own loop needs more than 256 * CUs chunks (268 M points at 256 CUs).
"""
import importlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _index_chunks as ic  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
POINT_DTYPE = binding.POINT_DTYPE
CLASS_PHASE = 3


class Big:
    """The big set on the device"""

    def __init__(self, ctx):
        began = time.perf_counter()
        self.ctx = ctx
        self.cus = ctx.device_info()["compute_units"]
        self.plan, self.data = ic.big_plan(self.cus), ic.big_data(self.cus)
        d = self.data
        self.blocks = [ctx.alloc(a.nbytes + 64) for a in (d.xyz, d.cls, d.t)]
        self.d_xyz, self.d_cls, self.d_t = self.blocks[0], self.blocks[1] + CLASS_PHASE, self.blocks[2]
        assert self.d_xyz % 16 == 0 and self.d_t % 16 == 0 and self.d_cls % 16 == CLASS_PHASE
        for ptr, a in zip((self.d_xyz, self.d_cls, self.d_t), (d.xyz, d.cls, d.t)):
            ctx.to_device(ptr, a)
        self.sel = {}
        print(f"big set: {self.cus} CUs, {self.plan.C} chunks, {d.n} points, built and uploaded in {time.perf_counter() - began:.2f} s")

    def cols(self, kind, n):
        return ic.columns(binding, kind, self.d_xyz, self.d_cls, self.d_t, n)

    def select(self, q):
        key = (q.kind, q.name)
        if key not in self.sel:
            self.sel[key] = ic.select(q.kind, self.data, q)
        return self.sel[key]

    def free(self):
        for b in self.blocks:
            self.ctx.free(b)


@pytest.fixture(scope="module")
def big(gpu_ctx):
    b = Big(gpu_ctx)
    yield b
    b.free()


def counts_through(ctx, kind, cols, data, sels, queries, what):
    """The building call and every later query with a count collector on one fresh index object over `data` (the columns' points)"""
    ix = ctx.index_new()
    built = set()
    try:
        for k, q in enumerate([queries[0]] + queries):
            got = ic.count_of(ctx, kind, cols, ic.predicate(pkg.Predicate, q), ix)
            st = ctx.index_stats(ix)
            want = ic.expected_stats(q, data, built, count=True)
            assert got == int(sels[q.name][:data.n].sum()), (what, kind, q.name, k, got)
            assert st == want, (what, kind, q.name, k, st, want)
            assert st["built"] == (1 if k == 0 else 0)
            if k == 0 and len(ic.PLANS[kind].parts) == 1:
                assert st["scanned"] == st["chunks"] == ic.chunks_of(kind, data.n)
    finally:
        ctx.index_free(ix)


def records_through(ctx, kind, cols, data, sels, queries, xyz=None):
    """The buffer queries into ONE collector through one index object (built by the first of them): every scan's records follow
    the ones before, and the statistics of every scan are the model's"""
    ix = ctx.index_new()
    gb = ctx.buffer_collector()
    built = set()
    want = b""
    try:
        for q in [q for q in queries if q.buffer] * 2:  # (the second round: every query with the parts built)
            indexed = ic.indexed_entry(ctx, kind)
            indexed(cols, ic.predicate(pkg.Predicate, q), ix, gb)
            sel = sels[q.name]
            want += ic.expect_records(kind, data.xyz if xyz is None else xyz, data.cls, sel, POINT_DTYPE).tobytes()
            assert gb.point_count() == len(want) // 31, (kind, q.name)
            st, exp = ctx.index_stats(ix), ic.expected_stats(q, data, built, count=False)
            assert st == exp, (kind, q.name, st, exp)
        assert gb.points().tobytes() == want, kind
        assert len(want) > 0
    finally:
        gb.free()
        ctx.index_free(ix)


def run_kind(big, kind):
    ctx, p, d = big.ctx, big.plan, big.data
    queries = ic.big_queries(kind, p)
    sels = {q.name: big.select(q) for q in queries}
    began = time.perf_counter()
    counts_through(ctx, kind, big.cols(kind, d.n), d, sels, queries, "every trip")
    m = p.grid * ic.CHUNK  # the first trip alone: a part is keyed by pointer and n, so this is another index
    counts_through(ctx, kind, big.cols(kind, m), d.prefix(m), sels, queries, "the first trip alone")
    records_through(ctx, kind, big.cols(kind, d.n), d, sels, queries)
    print(f"{kind}: the GPU calls and their checks took {time.perf_counter() - began:.2f} s")


def test_bounds(big):
    run_kind(big, "bounds")


def test_class(big):
    run_kind(big, "class")


def test_bounds_class(big):
    run_kind(big, "bounds_class")


def test_time(big):
    run_kind(big, "time")


def test_bounds_time(big):
    run_kind(big, "bounds_time")


def test_class_only_set_the_histogram_builder_on_its_second_trip(gpu_ctx):
    import torch
    ctx = gpu_ctx
    cus = ctx.device_info()["compute_units"]
    began = time.perf_counter()
    p, d = ic.class_only_plan(cus), ic.class_only_data(cus)
    queries = ic.class_only_queries()
    sels = {q.name: ic.select("class", d, q) for q in queries}
    block = ctx.alloc(d.n + 64)
    try:
        d_cls = block + CLASS_PHASE
        ctx.to_device(d_cls, d.cls)
        print(f"class-only set: {p.class_chunks} class chunks, {d.n} bytes, built and uploaded in {time.perf_counter() - began:.2f} s")
        # counts need no positions: the building count, the later ones, and the first `grid` class chunks alone
        cols = binding.make_columns(cls=d_cls, n=d.n)
        counts_through(ctx, "class", cols, d, sels, queries, "every trip")
        m = p.grid * ic.CLASS_CHUNK
        counts_through(ctx, "class", binding.make_columns(cls=d_cls, n=m), d.prefix(m), sels, queries, "the first trip alone")
        # one buffer scan of the rare class: point i lies at (i, -i, i mod 1024), written on the device
        i = torch.arange(d.n, dtype=torch.int32, device="cuda:0")
        xyz = torch.stack([i, -i, i & 1023], dim=1).contiguous()
        del i
        torch.cuda.synchronize()
        assert xyz.shape == (d.n, 3) and xyz.data_ptr() % 16 == 0
        idx = np.flatnonzero(sels["rare"]).astype(np.int64)
        h_xyz = np.stack([idx, -idx, idx & 1023], axis=1).astype(np.int32)
        rare = ic.Data(h_xyz, d.cls[idx])
        cols = binding.make_columns(xyz=xyz.data_ptr(), cls=d_cls, n=d.n, scale=ic.SCALE, offset=ic.OFFSET)
        ix, gb = ctx.index_new(), ctx.buffer_collector()
        try:
            built = set()
            for k in range(2):
                ctx.scan_dev_indexed(cols, ic.predicate(pkg.Predicate, queries[-1]), ix, gb)
                st, exp = ctx.index_stats(ix), ic.expected_stats(queries[-1], d, built, count=False)
                assert st == exp, (k, st, exp)
            one = ic.expect_records("class", rare.xyz, rare.cls, np.ones(len(idx), dtype=bool), POINT_DTYPE).tobytes()
            assert len(idx) > 1000 and gb.points().tobytes() == one + one
        finally:
            gb.free()
            ctx.index_free(ix)
            del xyz
    finally:
        ctx.free(block)
    print(f"class-only set: {time.perf_counter() - began:.2f} s in all")
