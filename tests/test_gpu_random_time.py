"""Randomised GPU parity of the GPS time search and the combined searches (PCQ_PRED_TIME, _BOUNDS_CLASS, _BOUNDS_TIME).

* Files: the random LAS / LAST images of test_gpu_random.build() (formats 0-10, LAS 1.2 and 1.4 headers, extra bytes, VLR
  padding, odd record lengths, legacy count 0, extreme coordinates, header boxes that do not match the data) with GPS times
  written at +20 / +22 — drawn from an RNG of their own, so the images of the existing seeds are unchanged underneath.
  Every search goes through the C view (libpcq_query.so -> HIP) and through the oracle (oracle/pcq_oracle.c)
  into count, buffer and grid collectors: the status always, and on success the count, the records byte for byte in file
  order and the grid's keys and winners.
* Layouts: pcq_scan_dev counts of the three kinds against numpy at every position phase (the head peel), class phase,
  time-body phase mod 16 and at sizes around K1's tile (256 points) and step (512), K3's step (512 times) and the head / tail
  lanes, so that every (head peel, time-body phase) pair reaches K1's pipelined path and its leftover tiles; records and grids
  on a subset; strided LAS-like records of random lengths.
* The CLI: `query` against `query_oracle` on random directories of LAS and LAST files.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _oracle  # noqa: E402
import _time_images as ti  # noqa: E402
from test_gpu_combined import BOX, Dev, Query  # noqa: E402
from test_gpu_combined import run_all as run_combined  # noqa: E402
from test_gpu_host import Q  # noqa: E402
from test_gpu_random import build, random_box, sorted_grid  # noqa: E402
from test_gpu_time import run_all as run_time  # noqa: E402

pytestmark = pytest.mark.gpu

import importlib  # noqa: E402

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

SEED_BASE = int(os.environ.get("PCQ_TEST_SEED_BASE", "0"))  # a soak run: other seeds than the committed ones
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY = os.path.join(ROOT, "adhoc-queries-pointclouds_amd", "host", "query")
QUERY_ORACLE = os.path.join(ROOT, "oracle", "query_oracle")
TIME_AT = {1: 20, 3: 20, 4: 20, 5: 20, 6: 22, 7: 22, 8: 22, 9: 22, 10: 22}  # las.rs:305-330
DBL_MAX = np.finfo(np.float64).max
NAN_PAYLOAD = np.array([0x7FF8000000001234, 0xFFF0000000000001], dtype=np.uint64).view(np.float64)  # quiet with payload, negative signalling
SPECIALS = np.concatenate([[np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 1e-310,
                            DBL_MAX, -DBL_MAX], NAN_PAYLOAD])


def view_q():
    q = Q()
    return q


def draw_times(trng, n):
    """Sorted acquisition times, the same shuffled, all equal, or sorted with the IEEE specials injected."""
    kind = int(trng.integers(0, 4))
    if kind == 2:
        return np.full(n, trng.choice([0.0, -0.0, 1.5e8, 5e-324, 318_000_000.25])), kind
    t = trng.uniform(-1e6, 4e8) + np.cumsum(trng.exponential(trng.choice([1e-6, 1e-3, 1.0]), n))
    if kind == 1:
        trng.shuffle(t)
    if kind == 3 or trng.random() < 0.3:
        pick = trng.random(n) < trng.choice([0.01, 0.1, 0.4])
        t[pick] = trng.choice(SPECIALS, int(pick.sum()))
    return t, kind


def ranges_for(trng, t):
    """[start, end) pairs: taken from the file's own times (and their neighbours one ulp away), infinite and NaN ends, empty
    and reversed; the file is given the ends of the first range and their neighbours at random places."""
    finite = t[np.isfinite(t)]
    if len(finite):
        a, b = np.sort(trng.choice(finite, 2))
    else:
        a, b = -1.0, 1.0
    for v in (a, b):
        if len(t):
            with np.errstate(over="ignore"):
                nb = np.array([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])
            t[trng.integers(0, len(t), 3)] = nb
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, -np.inf)
    with np.errstate(over="ignore"):  # (DBL_MAX -> inf)
        pool = [(up(a), b), (a, up(b)), (dn(a), dn(b)), (up(a), dn(b)), (-np.inf, b), (a, np.inf), (-np.inf, np.inf), (np.nan, b),
                (a, np.nan), (a, a), (b, a), (-DBL_MAX, DBL_MAX), (-0.0, 0.0), (0.0, 5e-324)]
    picks = [pool[i] for i in trng.choice(len(pool), 3, replace=False)]
    return [(float(a), float(b))] + [(float(s), float(e)) for s, e in picks]


def add_times(image, meta, trng, transposed):
    fmt, n, rl, otp = meta["fmt"], meta["n"], meta["rl"], meta["otp"]
    t, kind = draw_times(trng, n)
    ranges = ranges_for(trng, t)
    if fmt in TIME_AT and n:
        raw = np.ascontiguousarray(t.astype("<f8")).view(np.uint8)
        body = image[otp:]
        toff = TIME_AT[fmt]
        if transposed:  # the time block of the transposed record
            body[toff * n:(toff + 8) * n] = raw
        else:
            body.reshape(n, rl)[:, toff:toff + 8] = raw.reshape(n, 8)
    meta["times"] = kind
    return ranges


def maybe_invert(rng, bmin, bmax):
    if rng.random() < 0.15:
        a = int(rng.integers(0, 3))
        bmin, bmax = list(bmin), list(bmax)
        bmin[a], bmax[a] = bmax[a] + 1.0, bmin[a]
    return bmin, bmax


def compare(q, oracle, path, kind, args, grid_box, cell, what):
    """One search into a count, a buffer and a grid collector on both sides."""
    start, end = args.get("start", 0.0), args.get("end", 0.0)
    bmin, bmax, cls = args.get("bmin"), args.get("bmax"), args.get("cls", 0)

    def product(h):
        if kind == _oracle.QUERY_TIME:
            return q.lib.pcq_query_search_file_time(path.encode(), start, end, 1, h)
        if kind == _oracle.QUERY_BOUNDS_CLASS:
            return q.lib.pcq_query_search_file_bounds_class(path.encode(), q.d3(bmin), q.d3(bmax), cls, 1, h)
        return q.lib.pcq_query_search_file_bounds_time(path.encode(), q.d3(bmin), q.d3(bmax), start, end, 1, h)

    hc, hb = q.collector("count"), q.collector("buffer")
    if bmin is not None and any(a > b for a, b in zip(bmin, bmax)):
        # the C view builds the query's AABB first (AABB::from_min_max, which the reference's callers cannot get past):
        # a box with min > max on an axis panics before any file is opened
        try:
            assert product(hc) == product(hb) == _oracle.ERR_PANIC, what
        finally:
            q.free(hc), q.free(hb)
        return
    oc, ob = oracle.count_collector(), oracle.buffer_collector()
    try:
        rc_o = oracle.search_file_range(path, kind, bmin, bmax, cls, start, end, oc)
        assert oracle.search_file_range(path, kind, bmin, bmax, cls, start, end, ob) == rc_o
        rc_c, rc_b = product(hc), product(hb)
        assert rc_c == rc_b == rc_o, (what, rc_o, oracle.err(), q.lib.pcq_query_last_error())
        if rc_o == 0:
            assert q.count(hc) == oc.point_count(), what
            assert q.points(hb).tobytes() == ob.points().tobytes(), what
    finally:
        q.free(hc), q.free(hb), oc.free(), ob.free()
    try:
        og = oracle.grid_collector(grid_box[0], grid_box[1], cell)
    except _oracle.OracleError:
        return
    h = C.c_void_p()
    rc_new = q.lib.pcq_query_collector_new_grid(0, q.d3(grid_box[0]), q.d3(grid_box[1]), cell, C.byref(h))
    if rc_new != 0:  # -11: 64 key bits / non-finite bounds, the documented unsupported corner
        assert rc_new == -11, what
        og.free()
        return
    try:
        rc_o = oracle.search_file_range(path, kind, bmin, bmax, cls, start, end, og)
        assert product(h) == rc_o, what
        if rc_o == 0:
            gk, gp = sorted_grid(q, h)
            assert np.array_equal(gk, og.grid_cells()), what
            assert gp.tobytes() == og.points().tobytes(), what
    finally:
        q.free(h), og.free()


@pytest.mark.parametrize("seed", range(120))
def test_random_files_time_and_combined(oracle, tmp_path, seed):
    rng = np.random.default_rng(1000 + SEED_BASE + seed)  # the same files as test_gpu_random's seeds
    trng = np.random.default_rng(50_000 + SEED_BASE + seed)  # the times, queries and cuts of this test
    q = view_q()
    transposed = bool(seed % 2)
    image, world, meta = build(rng, transposed)
    ranges = add_times(image, meta, trng, transposed)
    if meta["n"] and trng.random() < 0.1:  # truncated: both sides must fail alike (or find the missing bytes unneeded)
        image = image[:len(image) - int(trng.integers(1, 3 * meta["rl"]))]
        meta["cut"] = True
    path = str(tmp_path / ("f.last" if transposed else "f.las"))
    image.tofile(path)
    for k, (start, end) in enumerate(ranges):
        bmin, bmax = maybe_invert(trng, *random_box(trng, world))
        grid_box = random_box(trng, world)
        qbox = (bmin, bmax) if all(a <= b for a, b in zip(bmin, bmax)) else grid_box  # (a grid over the query box, if it is one)
        cell = float(trng.choice([0.05, 1.0, 12.5, 1000.0, 1e9]))
        what = dict(meta, start=start, end=end, bmin=bmin, bmax=bmax)
        compare(q, oracle, path, _oracle.QUERY_TIME, dict(start=start, end=end), grid_box, cell, what)
        compare(q, oracle, path, _oracle.QUERY_BOUNDS_TIME, dict(start=start, end=end, bmin=bmin, bmax=bmax), qbox, cell, what)
        if k < 2:
            cls = int(trng.choice([0, 1, 2, 6, 134, 255, 19]))
            compare(q, oracle, path, _oracle.QUERY_BOUNDS_CLASS, dict(bmin=bmin, bmax=bmax, cls=cls), qbox, cell, dict(what, cls=cls))


@pytest.mark.parametrize("fmt,layout", [(5, "las"), (10, "last")])
def test_random_files_across_staging_chunks(oracle, tmp_path, fmt, layout):
    """Files of 2.3 M points: several staging chunks of the host path (1 Mi points each) under one search."""
    n = 2_300_011
    trng = np.random.default_rng(60_000 + SEED_BASE + fmt)
    xyz, cls, rgb, _ = ti.points(n, 70 + fmt)
    t, _ = draw_times(trng, n)
    ranges = ranges_for(trng, t)
    img = ti.las_image(fmt, xyz, cls, rgb, t) if layout == "las" else ti.last_image(fmt, xyz, cls, rgb, t)
    path = str(tmp_path / f"f.{layout}")
    img.tofile(path)
    del img
    q = view_q()
    world = ti.world(xyz[::97])
    for start, end in ranges[:2]:
        bmin, bmax = random_box(trng, world)
        what = (fmt, layout, start, end, bmin, bmax)
        compare(q, oracle, path, _oracle.QUERY_TIME, dict(start=start, end=end), (bmin, bmax), 50.0, what)
        compare(q, oracle, path, _oracle.QUERY_BOUNDS_TIME, dict(start=start, end=end, bmin=bmin, bmax=bmax), (bmin, bmax), 50.0, what)
        compare(q, oracle, path, _oracle.QUERY_BOUNDS_CLASS, dict(bmin=bmin, bmax=bmax, cls=2), (bmin, bmax), 50.0, what)


@pytest.mark.parametrize("name", ["tiny_fmt4.las", "tiny_fmt9.last"])
def test_golden_time_and_combined_files(name):
    """The hand-derived known answers of tests/golden/make_golden.py (NaN and +-0.0 times) through the C view."""
    from test_oracle_time_combined import GOLDEN, f_of, golden_records, golden_time
    g, _ = golden_time()
    path = os.path.join(GOLDEN, name)
    q = view_q()
    runs = [(lambda h, c=c: q.lib.pcq_query_search_file_time(path.encode(), f_of(c["start"]), f_of(c["end"]), 1, h), c) for c in g["time"]]
    runs += [(lambda h, c=c: q.lib.pcq_query_search_file_bounds_time(path.encode(), q.d3(c["bmin"]), q.d3(c["bmax"]), f_of(c["start"]),
                                                                      f_of(c["end"]), 1, h), c) for c in g["bounds_time"]]
    runs += [(lambda h, c=c: q.lib.pcq_query_search_file_bounds_class(path.encode(), q.d3(c["bmin"]), q.d3(c["bmax"]), c["class"], 1, h), c)
             for c in g["bounds_class"]]
    for search, case in runs:
        hc, hb = q.collector("count"), q.collector("buffer")
        try:
            assert search(hc) == search(hb) == 0, (case, q.lib.pcq_query_last_error())
            assert q.count(hc) == len(case["indices"]), case
            assert q.points(hb).tobytes() == golden_records(case["records"]).tobytes(), case
        finally:
            q.free(hc), q.free(hb)


# ---------------------------------------------------------------------------------------------------------------------
# device layouts through pcq_scan_dev, against numpy
# ---------------------------------------------------------------------------------------------------------------------
XYZ_PHASES = [0, 4, 8, 12, 2]  # the head peel takes 0..3 points; +2 is not 4-byte aligned: the strided kernel
SIZES = [1, 3, 255, 256, 257, 511, 512, 513, 771, 1023, 1025, 4096 + 259]  # 771 .. 1023: one step and one leftover tile
BIG = 1_048_909  # 4097 tiles behind any head peel: 2048 pipelined steps and one leftover tile, and a ragged tail
TQ = (-0.5, 0.5)


def _data(n, seed):
    xyz, cls, rgb, _ = ti.points(n, seed)
    return xyz, cls, rgb, ti.adversarial_times(n, *TQ, seed)


@pytest.mark.parametrize("xyz_phase", XYZ_PHASES)
def test_bounds_class_count_at_every_layout(gpu_ctx, xyz_phase):
    dev = Dev(gpu_ctx)
    try:
        for n in SIZES:
            xyz, cls, _, t = _data(n, n + xyz_phase)
            d_xyz = dev.put(xyz, pad=xyz_phase)
            for cph in range(16):
                d_cls = dev.put(cls, pad=cph)
                cols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
                run_combined(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), [Query(*BOX, cls=2), Query([-5000] * 3, [5000] * 3, cls=6)],
                             xyz, cls, None, t, kinds=("count",))
            dev.free()
    finally:
        dev.free()


@pytest.mark.parametrize("xyz_phase", XYZ_PHASES)
def test_bounds_time_count_at_every_layout(gpu_ctx, xyz_phase):
    """Time bases at 16-byte phases 0 and 8 and one only 4-byte aligned: with the head peel (xyz_phase / 4 points) the
    body of the times starts at 0 or 8 mod 16 for every peel, in the pipelined steps and in the leftover tile."""
    dev = Dev(gpu_ctx)
    queries = [Query(*BOX, start=TQ[0], end=TQ[1]), Query([-5000] * 3, [5000] * 3, start=-np.inf, end=0.0)]
    try:
        for n in SIZES + [BIG]:
            xyz, cls, _, t = _data(n, 3 * n + xyz_phase)
            d_xyz = dev.put(xyz, pad=xyz_phase)
            for tph in (0, 8, 4):
                d_t = dev.put(t, pad=tph)
                cols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
                run_combined(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(cols, p, g), queries, xyz, cls, None, t, kinds=("count",))
            dev.free()
    finally:
        dev.free()


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513, 514, 1023, 1024, 1025, 4096 + 131, BIG])
def test_time_count_at_k3_steps_and_tail_lanes(gpu_ctx, n):
    """K3 takes a head time in front of the first 16-byte aligned one, vectors of two, and one tail time: n of both
    parities at both 8-byte phases, and the unaligned column (the strided kernel)."""
    xyz, _, _, t = _data(n, 11 * n)
    t[-1] = 0.25  # the tail time is a match
    t[0] = -0.25  # and so is the head time
    dev = Dev(gpu_ctx)
    try:
        for tph in (0, 8, 3):
            d_t = dev.put(t, pad=tph)
            cols = binding.make_columns(cls=d_t, n=n, cls_stride=8)
            for start, end in (TQ, (-0.25, 0.2500000000000001), (0.25, np.inf)):
                cc = gpu_ctx.count_collector()
                gpu_ctx.scan_dev(cols, pkg.Predicate.time_range(start, end), cc)
                assert cc.point_count() == int(ti.select(t, start, end).sum()), (tph, start, end)
                cc.free()
    finally:
        dev.free()


@pytest.mark.parametrize("xyz_phase,tph", [(0, 8), (4, 0), (8, 8), (12, 0)])
def test_records_and_grids_at_8_mod_16_time_bodies(oracle, gpu_ctx, xyz_phase, tph):
    """Buffer and grid collectors at the layouts whose time body sits at 8 mod 16 (and one class column at every peel)."""
    dev = Dev(gpu_ctx)
    try:
        for n in (771, 4096 + 259, 70_001):
            xyz, cls, rgb, t = _data(n, 5 * n + xyz_phase)
            d_xyz, d_t, d_cls = dev.put(xyz, pad=xyz_phase), dev.put(t, pad=tph), dev.put(cls, pad=xyz_phase // 4 + 5)
            tcols = binding.make_columns(xyz=d_xyz, cls=d_t, n=n, cls_stride=8, scale=list(ti.SCALE), offset=list(ti.OFFSET))
            ccols = binding.make_columns(xyz=d_xyz, cls=d_cls, n=n, scale=list(ti.SCALE), offset=list(ti.OFFSET))
            run_combined(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), [Query(*BOX, start=TQ[0], end=TQ[1])], xyz, cls, None, t, oracle)
            run_time(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), xyz, t, [TQ, (0.0, np.inf)], oracle)
            run_combined(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(ccols, p, g), [Query(*BOX, cls=6)], xyz, cls, None, t, oracle)
            dev.free()
    finally:
        dev.free()


@pytest.mark.parametrize("seed", range(6))
def test_interleaved_records_of_random_length(oracle, gpu_ctx, seed):
    """LAS-like records of 28..90 bytes with the class at +15 and the time at a random offset: the strided kernels."""
    rng = np.random.default_rng(80_000 + SEED_BASE + seed)
    rl = int(rng.integers(28, 91))
    toff = int(rng.integers(16, rl - 7))
    n = int(rng.choice([257, 4096 + 3, 40_001]))
    xyz, cls, rgb, t = _data(n, 90 + seed)
    rec = np.zeros((n, rl), dtype=np.uint8)
    rec[:, :] = rng.integers(0, 256, (n, rl), dtype=np.uint8)
    rec[:, 0:12] = xyz.astype("<i4").view(np.uint8).reshape(n, 12)
    rec[:, 15] = cls
    rec[:, toff:toff + 8] = t.astype("<f8").view(np.uint8).reshape(n, 8)
    dev = Dev(gpu_ctx)
    try:
        for pad in (0, int(rng.integers(1, 16))):
            base = dev.put(rec.reshape(-1), pad=pad)
            sc = dict(scale=list(ti.SCALE), offset=list(ti.OFFSET))
            tcols = binding.make_columns(xyz=base, cls=base + toff, n=n, xyz_stride=rl, cls_stride=rl, **sc)
            ccols = binding.make_columns(xyz=base, cls=base + 15, n=n, xyz_stride=rl, cls_stride=rl, **sc)
            run_time(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), xyz, t, [TQ, (-np.inf, -0.0)], oracle)
            run_combined(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(tcols, p, g), [Query(*BOX, start=TQ[0], end=TQ[1])], xyz, cls, None, t, oracle)
            run_combined(gpu_ctx, lambda p, g: gpu_ctx.scan_dev(ccols, p, g), [Query(*BOX, cls=2)], xyz, cls, None, t, oracle)
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------------------------------
# the CLI against the oracle's CLI
# ---------------------------------------------------------------------------------------------------------------------
def _cli(exe, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=e)
    return r.returncode, sorted(line for line in r.stdout.splitlines() if not line.startswith("Searched ")), r.stderr


@pytest.fixture(scope="module")
def random_dir(tmp_path_factory):
    """Six random LAS and LAST files with GPS times (formats 1, 3-10), and the world box of the first."""
    d = tmp_path_factory.mktemp("rdir")
    k, seed, first = 0, 0, None
    while k < 6:
        rng = np.random.default_rng(20_000 + SEED_BASE + seed)
        trng = np.random.default_rng(30_000 + SEED_BASE + seed)
        seed += 1
        transposed = bool(k % 2)
        image, world, meta = build(rng, transposed)
        if meta["fmt"] not in TIME_AT or meta["n"] < 100:
            continue
        ranges = add_times(image, meta, trng, transposed)
        image.tofile(d / f"f{k}.{'last' if transposed else 'las'}")
        if first is None:
            first = (world, ranges[0])
        k += 1
    return str(d), first


@pytest.mark.parametrize("what", ["time", "class", "bounds_time"])
def test_cli_matches_oracle_cli_on_random_files(random_dir, tmp_path, what):
    d, (world, (start, end)) = random_dir
    rng = np.random.default_rng(40_000 + SEED_BASE + len(what))
    bmin, bmax = random_box(rng, world)
    box = ";".join(repr(float(v)) for v in list(bmin) + list(bmax))
    trange = f"{start!r};{end!r}"
    q = {"time": ["--time", trange], "class": ["--combine", "--bounds", box, "--class", "2"],
         "bounds_time": ["--combine", "--bounds", box, "--time", trange]}[what]
    for mode in ([], ["--parallel"]):
        out = tmp_path / f"out{len(mode)}"
        out.mkdir()
        for extra in ([], ["-o", str(out)], ["--density", "1e7"]):
            args = ["-i", d, "--optimized"] + q + mode + extra
            got, want = _cli(QUERY, args), _cli(QUERY_ORACLE, args)
            assert got == want, (args, got, want)
            if not mode and not extra:
                assert _cli(QUERY, args, {"PCQ_CHUNK_POINTS": "4096"}) == want, args
