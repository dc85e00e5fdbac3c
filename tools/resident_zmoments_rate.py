"""Developer tool: the height-spread raster of a box on resident data — one pass that adds every point inside the box into the
count, the z sum and the two halves of the sum of z squared of its cell of an nx x ny raster over x and y.

(i)   FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13), twice: (g) in the generator's order (random
      inside a tile) and (s) in scan-strip order (strips 10 m wide in y and z, points sorted along x: the lanes of a wave mostly
      share a cell) — the data of resident_zsum_rate.py.  The ca13_XL box with z unbounded, which keeps every point.  Rasters of
      8 x 8 and 32 x 32 cells (PCQ_ZMOMENTS_CELLS_MAX) over the box's x and y.  Per order and raster two routes, timed with device
      events around the whole of each, alternated in one process on identical input, REPS rounds after 3 warm-up rounds; median,
      minimum and maximum, TB/s on 12 B/point:
        zmoments  ONE pcq_scan_dev_zmoments_raster_batch, its words zeroed by four fills;
        zsum      ONE pcq_scan_dev_zsum_raster_batch at the same cells, its words zeroed by two fills: the same loads, divisions
                  and z gather, two 64-bit LDS adds per point instead of four.
      The yardstick is TWO mean-height passes, which is what a caller could do instead (and still not have the spread).  The counts
      and sums must be the mean-height raster's, word for word, n * sum z^2 >= (sum z)^2 must hold in every cell in integers, and
      g and s must agree in every word.
(ii)  (not with PCQ_LAB=1) ONE tile — tile (1, 1) — as a LAST file of NB points in a resident dataset of the host layer
      (pcq_query_resident_load_points), 32 x 32 square cells over the lower left of it, z unbounded:
      pcq_query_resident_bounds_zstd_raster against the route it replaces, pcq_query_resident_search_bounds into a buffer collector,
      pcq_query_collector_points to host memory (31 B per match) and the reduction of the records on the host (three np.bincount).
      Wall time of the whole of each, alternated the same way; the route's share up to the end of the copy is reported beside it.
      The counts must agree exactly, the means to 1e-9 relative and the deviations to 1e-6 relative (the host route sums world z and
      z^2 in f64 and subtracts, the one pass integers).  Rule: the one pass's slowest round is below that route's fastest round.
(iii) with PCQ_LAB=1 (libpcq_lab.so accepts the option "zmoments_waves_per_cu"): the one pass of (i) at 4, 8, 12 and 16 workgroups
      per CU before the LDS limit (160 KiB / (32 nx ny): 5 at 1024 cells).
The last line restates the checks.  On a shared GPU run each part under a time limit of its own and chain them:
    timeout -k 10 900 python tools/resident_zmoments_rate.py && PCQ_LAB=1 timeout -k 10 900 python tools/resident_zmoments_rate.py
usage: resident_zmoments_rate.py [N [FILES [REPS [NB]]]]"""
import ctypes as C
import importlib, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
files = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
nb = int(sys.argv[4]) if len(sys.argv) > 4 else n
dev = torch.device("cuda:0")
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream
lab = os.environ.get("PCQ_LAB") == "1"
RASTERS = ((8, 8), (32, 32))


def spread(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "reps": len(v)}


def alternate(fns, reps, warm=3, events=True):
    """fns: name -> callable; one of each per round, device events (or the wall clock) around each, the first `warm` rounds dropped"""
    times = {k: [] for k in fns}
    for it in range(reps + warm):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record(); e1.synchronize()
                ms = e0.elapsed_time(e1)
            else:
                t0 = time.perf_counter()
                fn()
                ms = (time.perf_counter() - t0) * 1e3
            if it >= warm:
                times[k].append(ms)
    return {k: spread(v) for k, v in times.items()}


def tbps(points, ms):
    return points * 12 / (ms * 1e-3) / 1e12


checks = {}
with pkg.Context(0) as ctx:
    # ---- (i) one pass against the mean-height raster's, (iii) at other grids -------------------------------------------------
    tiles = specs.synth_ca13(points_per_file=n, files=files)
    bmin, bmax = specs.box("ca13_XL")
    keep, cols = [], {"g": [], "s": []}
    for spec in tiles:
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), None, stream)
        torch.cuda.synchronize()
        t = raw.view(n, 3)
        width, zwidth = int(10.0 / spec.scale[1]), int(10.0 / spec.scale[2])
        key = ((t[:, 1].long() // width) * 4096 + (t[:, 2].long() // zwidth + 2048)) * (1 << 32) + (t[:, 0].long() + (1 << 31))
        order = torch.argsort(key)
        del key
        strips = t[order].contiguous().view(-1)
        del order
        keep += [raw, strips]
        for name, buf in (("g", raw), ("s", strips)):
            assert buf.data_ptr() % 16 == 0
            cols[name].append(binding.make_columns(xyz=buf.data_ptr(), n=n, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    # every tile has the scale and offset of the first: one local box, one lattice (x, y and z)
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(tiles[0].scale), list(tiles[0].offset))
    assert all(pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) == (lmin, lmax) for s in tiles)
    words = [torch.zeros(1024, dtype=torch.int64, device=dev) for _ in range(4)]   # count, sum, low, high
    cnt2 = torch.zeros(1024, dtype=torch.int64, device=dev)
    zsum2 = torch.zeros(1024, dtype=torch.int64, device=dev)
    points = files * n
    assert points < 2**32  # (one launch: no word can wrap)
    for nx, ny in RASTERS:
        cw = [-(-(lmax[a] - lmin[a] + 1) // d) for a, d in ((0, nx), (1, ny))]
        lo, hi = [lmin[0], lmin[1], -2**40], [lmin[0] + nx * cw[0] - 1, lmin[1] + ny * cw[1] - 1, 2**40]
        preds = [pkg.Predicate.bounds(lo, hi)] * files
        cells = [cw] * files
        seen = {}
        for order in ("g", "s"):
            c = cols[order]

            def zmoments_pass():
                for w in words:
                    w.zero_()
                ctx.scan_dev_zmoments_raster_batch(c, preds, cells, nx, ny, *[w.data_ptr() for w in words], stream)

            def zsum_pass():
                cnt2.zero_(); zsum2.zero_()
                ctx.scan_dev_zsum_raster_batch(c, preds, cells, nx, ny, cnt2.data_ptr(), zsum2.data_ptr(), stream)

            zmoments_pass(); zsum_pass()
            torch.cuda.synchronize()
            w = nx * ny
            got = [a[:w].clone() for a in words]
            tag = f"{nx}x{ny}_{order}"
            checks[f"{tag}_counts_and_sums_are_the_mean_height_rasters"] = bool(torch.equal(got[0], cnt2[:w]) and torch.equal(got[1], zsum2[:w])) and \
                int(got[0].sum()) == points
            ints = [a.cpu().tolist() for a in got]
            spread_steps = [((cn * (h * 2**32 + l) - s * s) / (cn * cn)) ** 0.5 for cn, s, l, h in zip(*ints) if cn]
            checks[f"{tag}_n_sum_of_squares_at_least_the_squared_sum"] = all(cn * (h * 2**32 + l) >= s * s and 0 <= l and 0 <= h
                                                                             for cn, s, l, h in zip(*ints))
            seen[order] = got
            if not lab:
                res = alternate({"zmoments": zmoments_pass, "zsum": zsum_pass}, reps)
                for k in res:
                    res[k]["TBps_12B_per_point"] = tbps(points, res[k]["median_ms"])
                print("(i)", json.dumps({"nx_ny": [nx, ny], "order": order, "files": files, "points_per_file": n, "cells_hit": len(spread_steps),
                                          "largest_cell": int(got[0].max()), "std_lattice_steps_lowest": min(spread_steps),
                                          "std_lattice_steps_highest": max(spread_steps),
                                          "zmoments_over_zsum": res["zmoments"]["median_ms"] / res["zsum"]["median_ms"],
                                          "zmoments_over_two_zsum": res["zmoments"]["median_ms"] / (2 * res["zsum"]["median_ms"]), **res}), flush=True)
                checks[f"{tag}_below_two_mean_height_passes"] = res["zmoments"]["median_ms"] < 2 * res["zsum"]["median_ms"]
            else:
                sweep = {}
                for wv in (4, 8, 12, 16):
                    ctx.set_option("zmoments_waves_per_cu", wv)
                    r = alternate({"zmoments": zmoments_pass}, max(3, reps // 2), warm=1)["zmoments"]
                    torch.cuda.synchronize()
                    assert all(torch.equal(a[:w], b) for a, b in zip(words, got)), wv
                    sweep[f"w{wv}"] = [round(r["median_ms"], 3), round(r["min_ms"], 3), round(r["max_ms"], 3)]
                ctx.set_option("zmoments_waves_per_cu", 0)
                r = alternate({"zmoments": zmoments_pass}, max(3, reps // 2), warm=1)["zmoments"]
                sweep["shipped"] = [round(r["median_ms"], 3), round(r["min_ms"], 3), round(r["max_ms"], 3)]
                print("(iii)", json.dumps({"nx_ny": [nx, ny], "order": order, "lds_limit_waves_per_cu": 160 * 1024 // (32 * nx * ny),
                                            "median_min_max_ms": sweep}), flush=True)
        checks[f"{nx}x{ny}_orders_agree"] = all(torch.equal(a, b) for a, b in zip(seen["g"], seen["s"]))
    del keep, cols, words, cnt2, zsum2
    torch.cuda.empty_cache()
if lab:
    print("checks", json.dumps(checks), flush=True)
    sys.exit(0)

# ---- (ii) the host entry against a search into a buffer collector, the copy of its records and their reduction on the host ------
import _oracle  # only to WRITE the synthetic file (the generator lives in the oracle)
d = tempfile.mkdtemp(prefix="pcq_zmoments_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    oracle = _oracle.Oracle()
    s = specs.synth_ca13(points_per_file=nb, files=16)[5]  # tile (1, 1)
    path = os.path.join(d, "ca13_5.last")
    t0 = time.perf_counter()
    oracle.synth_write(s, path, threads=16)
    t1 = time.perf_counter()
    lib = pkg.load_query_library()
    vp, dd, pu64 = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    arr = (C.c_char_p * 1)(path.encode())
    h = vp()
    assert lib.pcq_query_resident_load_points(0, arr, 1, C.byref(h)) == 0, lib.pcq_query_last_error()
    print(f"(ii) wrote 1 file x {nb} points in {t1 - t0:.1f} s, loaded in {time.perf_counter() - t1:.1f} s", flush=True)
    # 32 x 32 cells of 36515 lattice steps of 0.01 m: PCQ_ZMOMENTS_CELLS_MAX cells, one launch; they cover the lower left quarter of
    # the tile (about a quarter of its points).  The origin half a step inside the tile, so that the truncating conversion to the
    # lattice lands on the tile's first value
    k, nx, ny = 36515, 32, 32
    cell = k * 0.01
    assert nx * k <= s.span[0] and ny * k <= s.span[1] and s.scale[0] == s.scale[1] == s.scale[2] == 0.01 and s.offset[2] == 0.0
    lo = (s.lo[0] * 0.01 + 0.005, s.lo[1] * 0.01 + 0.005, -1e9)
    hi = (lo[0] + nx * cell, lo[1] + ny * cell, 1e9)
    c_lo, c_hi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    count, zmean, zstd = np.zeros(nx * ny, dtype=np.uint64), np.zeros(nx * ny), np.zeros(nx * ny)
    scanned = C.c_uint64()
    cap = nb + 1024
    records = np.zeros(cap, dtype=pkg.POINT_DTYPE)
    got_n = C.c_uint64()
    lmin, _ = pkg.box_to_local(list(lo), list(hi), list(s.scale), list(s.offset))
    host = {"copied_ms": []}

    def one_pass():
        assert lib.pcq_query_resident_bounds_zstd_raster(h, c_lo, 1e9, cell, nx, ny, count.ctypes.data_as(pu64), zmean.ctypes.data_as(dd),
                                                         zstd.ctypes.data_as(dd), C.byref(scanned)) == 0, lib.pcq_query_last_error()

    def search_copy_and_reduce():
        t0 = time.perf_counter()
        coll = vp()
        assert lib.pcq_query_collector_new_buffer(0, C.byref(coll)) == 0, lib.pcq_query_last_error()
        try:
            assert lib.pcq_query_resident_search_bounds(h, c_lo, c_hi, coll) == 0, lib.pcq_query_last_error()
            assert lib.pcq_query_collector_points(coll, records.ctypes.data_as(vp), cap, C.byref(got_n)) == 0, lib.pcq_query_last_error()
        finally:
            lib.pcq_query_collector_free(coll)
        host["copied_ms"].append((time.perf_counter() - t0) * 1e3)
        # the records reduced on the host: the stored integers back from world x and y (scale 0.01, offset 0: exact below 2^31), the
        # cell from the lattice origin the prologue gives, the records beyond the last full cell dropped
        r = records[:got_n.value]
        cx = (np.rint(r["x"] / 0.01).astype(np.int64) - lmin[0]) // k
        cy = (np.rint(r["y"] / 0.01).astype(np.int64) - lmin[1]) // k
        sel = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        at = (cy * nx + cx)[sel]
        z = r["z"][sel]
        host["count"] = np.bincount(at, minlength=nx * ny)
        host["sum"] = np.bincount(at, weights=z, minlength=nx * ny)
        host["sq"] = np.bincount(at, weights=z * z, minlength=nx * ny)

    one_pass(); search_copy_and_reduce()
    liveh = host["count"] > 0
    nn = np.maximum(host["count"], 1)
    hmean = host["sum"] / nn
    hstd = np.sqrt(np.maximum(host["sq"] / nn - hmean * hmean, 0.0))
    checks["host_counts_agree"] = bool(np.array_equal(host["count"].astype(np.uint64), count))
    checks["host_means_agree_to_1e-9"] = bool(np.array_equal(np.isnan(zmean), ~liveh) and
                                              np.all(np.abs(zmean[liveh] - hmean[liveh]) <= 1e-9 * np.maximum(1.0, np.abs(hmean[liveh]))))
    checks["host_deviations_agree_to_1e-6"] = bool(np.array_equal(np.isnan(zstd), ~liveh) and
                                                   np.all(np.abs(zstd[liveh] - hstd[liveh]) <= 1e-6 * np.maximum(1.0, hstd[liveh])))
    res = alternate({"one_pass": one_pass, "search_copy_and_reduce": search_copy_and_reduce}, reps, events=False)
    checks["host_one_pass_faster_beyond_spread"] = res["one_pass"]["max_ms"] < res["search_copy_and_reduce"]["min_ms"]
    checks["host_speedup"] = res["search_copy_and_reduce"]["median_ms"] / res["one_pass"]["median_ms"]
    print("(ii)", json.dumps({"box": [list(lo), list(hi)], "nx_ny": [nx, ny], "cell_size": cell, "points_per_file": nb, "points_scanned": scanned.value,
                              "records": got_n.value, "record_bytes": got_n.value * 31, "cells_hit": int(liveh.sum()),
                              "std_z_lowest": float(np.nanmin(zstd)), "std_z_highest": float(np.nanmax(zstd)),
                              "search_and_copy_alone": spread(host["copied_ms"][-reps:]), "speedup": checks["host_speedup"], **res}), flush=True)
    lib.pcq_query_resident_free(h)
finally:
    shutil.rmtree(d, ignore_errors=True)
print("checks", json.dumps(checks), flush=True)
