"""On-the-fly chunk index (improvements.md:3-10): indexed count scans give exactly the
counts of the plain scans and of the oracle, and on spatially coherent data most chunks are not read."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")


def upload(ctx, arr, pad=0):
    arr = np.ascontiguousarray(arr)
    base = ctx.alloc(arr.nbytes + 64 + pad)
    ctx.to_device(base + pad, arr)
    return base, base + pad


def count(ctx, cols, pred, ix=None):
    cc = ctx.count_collector()
    if ix is None:
        ctx.scan_dev(cols, pred, cc)
    else:
        ctx.scan_dev_indexed(cols, pred, ix, cc)
    n = cc.point_count()
    cc.free()
    return n


@pytest.mark.parametrize("n", [4095, 4096, 4097, 50_000, 1_000_003])
@pytest.mark.parametrize("coherent", [False, True])
def test_indexed_bounds_count_equals_plain_and_oracle(oracle, gpu_ctx, n, coherent):
    spec = specs._spec(321 + n, n, 1, (0.01,) * 3, (0.0,) * 3, (-50000, -50000, -1000), (100001, 100001, 2001),
                       classes=[(1, 0.5), (2, 0.3), (6, 0.2)])
    xyz, cls = oracle.synth_columns(spec)
    if coherent:  # scan-line like order: sorted by x, so a chunk covers a thin x slab
        order = np.argsort(xyz[:, 0], kind="stable")
        xyz, cls = xyz[order], cls[order]
    base, dptr = upload(gpu_ctx, xyz)
    cols = binding.make_columns(xyz=dptr, n=n, scale=list(spec.scale), offset=list(spec.offset))
    ix = gpu_ctx.index_new()
    try:
        rng = np.random.default_rng(n)
        boxes = [([-2 ** 31] * 3, [2 ** 31 - 1] * 3), ([0, 0, 0], [0, 0, 0]), ([60000, 0, 0], [70000, 10, 10])]
        for _ in range(8):
            lo = rng.integers(-50000, 50000, 3)
            hi = lo + rng.integers(0, 60000, 3)
            boxes.append((list(lo), list(hi)))
        for k, (lo, hi) in enumerate(boxes):
            pred = pkg.Predicate.bounds(lo, hi)
            want = int(np.sum(np.all((xyz >= np.array(lo)) & (xyz <= np.array(hi)), axis=1)))
            assert count(gpu_ctx, cols, pred) == want
            assert count(gpu_ctx, cols, pred, ix) == want, (n, coherent, k)
            st = gpu_ctx.index_stats(ix)
            if n >= 4096:
                assert st["chunks"] == n // 4096
                assert st["built"] == (1 if k == 0 else 0)
                if k > 0:
                    assert st["skipped"] + st["whole"] + st["scanned"] == st["chunks"]
        if coherent and n >= 50_000:  # a thin x slab: almost every chunk is skipped or counted whole
            lo, hi = [-10000, -2 ** 31, -2 ** 31], [10000, 2 ** 31 - 1, 2 ** 31 - 1]
            pred = pkg.Predicate.bounds(lo, hi)
            assert count(gpu_ctx, cols, pred, ix) == int(np.sum((xyz[:, 0] >= lo[0]) & (xyz[:, 0] <= hi[0])))
            st = gpu_ctx.index_stats(ix)
            assert st["scanned"] <= 2 and st["whole"] >= 1 and st["skipped"] >= 1
    finally:
        gpu_ctx.index_free(ix)
        gpu_ctx.free(base)


def test_index_falls_through_for_unaligned_or_tiny_columns_and_rebuilds(oracle, gpu_ctx):
    spec = specs._spec(5, 20_000, 1, (0.01,) * 3, (0.0,) * 3, (-500, -500, -100), (1001, 1001, 201))
    xyz, _ = oracle.synth_columns(spec)
    pred = pkg.Predicate.bounds([-100, -100, -50], [100, 300, 50])
    want = int(np.sum(np.all((xyz >= [-100, -100, -50]) & (xyz <= [100, 300, 50]), axis=1)))
    ix = gpu_ctx.index_new()
    bases = []
    try:
        for pad in (4, 0, 8):  # unaligned -> plain scan; aligned -> build; other block -> rebuild
            base, dptr = upload(gpu_ctx, xyz, pad=pad)
            bases.append(base)
            cols = binding.make_columns(xyz=dptr, n=spec.n, scale=list(spec.scale), offset=list(spec.offset))
            for _ in range(2):
                assert count(gpu_ctx, cols, pred, ix) == want
        base, dptr = upload(gpu_ctx, xyz[:100])
        bases.append(base)
        cols = binding.make_columns(xyz=dptr, n=100)
        assert count(gpu_ctx, cols, pred, ix) == int(np.sum(np.all((xyz[:100] >= [-100, -100, -50]) & (xyz[:100] <= [100, 300, 50]), axis=1)))
    finally:
        gpu_ctx.index_free(ix)
        for b in bases:
            gpu_ctx.free(b)


@pytest.mark.parametrize("n", [1, 65_535, 65_536, 65_537, 500_009])
def test_indexed_class_count(oracle, gpu_ctx, n):
    spec = specs.synth_doc(n)[2]
    _, cls = oracle.synth_columns(spec)
    base, dptr = upload(gpu_ctx, cls, pad=3)
    cols = binding.make_columns(cls=dptr, n=n)
    ix = gpu_ctx.index_new()
    try:
        for k, c in enumerate([6, 1, 2, 5, 7, 9, 19, 0, 255, 6]):
            pred = pkg.Predicate.classification(c)
            assert count(gpu_ctx, cols, pred, ix) == int((cls == c).sum()) == count(gpu_ctx, cols, pred)
            st = gpu_ctx.index_stats(ix)
            assert st["built"] == (1 if k == 0 else 0)
            if k > 0:
                assert st["scanned"] == 0 and st["whole"] == st["chunks"]  # answered from the histograms
    finally:
        gpu_ctx.index_free(ix)
        gpu_ctx.free(base)


def test_indexed_count_validates_its_columns_first(oracle, gpu_ctx):
    """An indexed bounds count over a layout the index covers (resident, 16-byte aligned, two whole chunks) launches its own
    kernels on the columns it is handed: like every scan it refuses what pcq_validate_scan refuses — here a first_index
    above 2^62 — before it counts anything or builds the index."""
    spec = specs._spec(99, 8192, 1, (0.01,) * 3, (0.0,) * 3, (-500, -500, -100), (1001, 1001, 201))
    xyz, _ = oracle.synth_columns(spec)
    base, dptr = upload(gpu_ctx, xyz)
    assert dptr % 16 == 0
    cols = binding.make_columns(xyz=dptr, n=8192, first_index=2 ** 62 + 1, scale=list(spec.scale), offset=list(spec.offset))
    ix = gpu_ctx.index_new()
    cc = gpu_ctx.count_collector()
    try:
        with pytest.raises(pkg.PcqError) as e:
            gpu_ctx.scan_dev_indexed(cols, pkg.Predicate.bounds([-2 ** 31] * 3, [2 ** 31 - 1] * 3), ix, cc)
        assert e.value.code == binding.PCQ_ERR_ARG
        assert cc.point_count() == 0
        assert gpu_ctx.index_stats(ix) == {"chunks": 0, "skipped": 0, "whole": 0, "scanned": 0, "built": 0}
    finally:
        cc.free()
        gpu_ctx.index_free(ix)
        gpu_ctx.free(base)
