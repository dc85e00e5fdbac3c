"""Developer tool: the canopy-height raster on resident data — one pass that folds every point inside the box into the minimum of its
cell when its class byte is in a LOW set and into the maximum of its cell when its class byte is in a HIGH set.

(i)   FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13 with the classes of synth-doc: 45 % class 2),
      twice: (g) in the generator's order and (s) in scan-strip order (strips 10 m wide in y and z, points sorted along x; the class
      bytes permuted with the points), the class block of every file 3 bytes off a dword.  The ca13_XL box with z unbounded, which
      keeps every point.  Rasters of 8 x 8 and 64 x 64 cells (PCQ_ZRANGE_CLASSES_CELLS_MAX) over the box's x and y.  Per order and
      raster six routes, timed with device events around the whole of each, alternated in one process on identical input, REPS rounds
      after 3 warm-up rounds; median, minimum and maximum:
        canopy       ONE pcq_scan_dev_zrange_raster_batch_classes, low {2}, high all but {7, 18}, its words preset by two fills;
        both_2       the same with both sets {2};
        full         the same with both sets full;
        zrange       ONE pcq_scan_dev_zrange_raster_batch at the same cells (12 B/point): the unfiltered pass;
        zsum_2       ONE pcq_scan_dev_zsum_raster_batch_classes, set {2} (at 64 x 64 cells: 64 x 32, that entry's limit);
        two_pass     zsum_2 then zrange: today's nearest substitute for a ground / surface model.
      `full` must give the unfiltered pass's words; the cells `both_2` marks must be those zsum_2 counts a point in.
(ii)  (not with PCQ_LAB=1) ONE tile — tile (1, 1) — as a LAST file of NB points in a resident dataset of the host layer
      (pcq_query_resident_load_points), 64 x 32 square cells over the lower half of it, z unbounded:
      pcq_query_resident_bounds_canopy_raster (ground {2}, surface all but {7, 18}) against the route it replaces, run twice by a
      caller: pcq_query_resident_search_bounds_class (class 2) into a buffer collector and pcq_query_collector_points to host memory
      (31 B per match) for the ground, and pcq_query_resident_search_bounds with the same copy for the surface (the class search takes
      one class; the caller drops 7 and 18 on the host).  Wall time of the whole of each, alternated the same way; the reduction of
      the records on the host is NOT timed.  zground must equal the minimum of the ground records' z per cell to 1e-9.
(iii) with PCQ_LAB=1 (libpcq_lab.so accepts the option "zrange_classes_waves_per_cu"): canopy, both_2 and full of (i), generator
      order, at 3 .. 16 workgroups per CU before the LDS limit (160 KiB / (256 + 8 nx ny): 4 at 4096 cells).
The last line restates the checks.
usage: resident_zrange_classes_rate.py [N [FILES [REPS [NB]]]]"""
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
RASTERS = ((8, 8), (64, 64))
ALL = tuple(range(256))
BUT_7_18 = tuple(c for c in range(256) if c not in (7, 18))
I32_MIN, I32_MAX = -2**31, 2**31 - 1


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


def doc_classes(spec, points):
    """the positions of ca13, the classes of synth-doc"""
    doc = specs.synth_doc(points_per_file=points, files=1)[0]
    spec.n_classes = doc.n_classes
    for j in range(8):
        spec.cls_val[j], spec.cls_cum16[j] = doc.cls_val[j], doc.cls_cum16[j]
    return spec


checks = {}
with pkg.Context(0) as ctx:
    # ---- (i) the pass against the unfiltered one, the class-filtered mean pass and the two together; (iii) at other grids ---------
    tiles = [doc_classes(s, n) for s in specs.synth_ca13(points_per_file=n, files=files)]
    bmin, bmax = specs.box("ca13_XL")
    keep, cols = [], {"g": [], "s": []}
    for spec in tiles:
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        cb = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), cb.data_ptr() + 3, stream)
        torch.cuda.synchronize()
        keep += [raw, cb]
        bufs = {"g": (raw, cb)}
        if not lab:
            t = raw.view(n, 3)
            width, zwidth = int(10.0 / spec.scale[1]), int(10.0 / spec.scale[2])
            key = ((t[:, 1].long() // width) * 4096 + (t[:, 2].long() // zwidth + 2048)) * (1 << 32) + (t[:, 0].long() + (1 << 31))
            order = torch.argsort(key)
            del key
            strips = t[order].contiguous().view(-1)
            scb = torch.empty(n + 16, dtype=torch.uint8, device=dev)
            scb[3:3 + n] = cb[3:3 + n][order]
            del order
            keep += [strips, scb]
            bufs["s"] = (strips, scb)
        for name, (pos, cl) in bufs.items():
            assert pos.data_ptr() % 16 == 0 and (cl.data_ptr() + 3) % 4 == 3
            cols[name].append(binding.make_columns(xyz=pos.data_ptr(), cls=cl.data_ptr() + 3, n=n, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(tiles[0].scale), list(tiles[0].offset))
    assert all(pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) == (lmin, lmax) for s in tiles)
    zmin = torch.zeros(4096, dtype=torch.int32, device=dev)
    zmax = torch.zeros(4096, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2048, dtype=torch.int64, device=dev)
    zsum = torch.zeros(2048, dtype=torch.int64, device=dev)
    points = files * n
    assert points < 2**32
    for nx, ny in RASTERS:
        sy = min(ny, 2048 // nx)  # the rows of the class-filtered mean pass at this raster
        cw = [-(-(lmax[a] - lmin[a] + 1) // d) for a, d in ((0, nx), (1, ny))]
        scw = [cw[0], -(-(lmax[1] - lmin[1] + 1) // sy)]
        lo, hi = [lmin[0], lmin[1], -2**40], [lmin[0] + nx * cw[0] - 1, lmin[1] + ny * cw[1] - 1, 2**40]
        shi = [hi[0], lmin[1] + sy * scw[1] - 1, 2**40]
        preds, spreds = [pkg.Predicate.bounds(lo, hi)] * files, [pkg.Predicate.bounds(lo, shi)] * files
        cells, scells = [cw] * files, [scw] * files
        for order in (("g",) if lab else ("g", "s")):
            c = cols[order]

            def canopy_pass(low, high):
                def f():
                    zmin.fill_(I32_MAX); zmax.fill_(I32_MIN)
                    ctx.scan_dev_zrange_raster_batch_classes(c, preds, cells, nx, ny, low, high, zmin.data_ptr(), zmax.data_ptr(), stream)
                return f

            def zrange_pass():
                zmin.fill_(I32_MAX); zmax.fill_(I32_MIN)
                ctx.scan_dev_zrange_raster_batch(c, preds, cells, nx, ny, zmin.data_ptr(), zmax.data_ptr(), stream)

            def zsum_2():
                cnt.zero_(); zsum.zero_()
                ctx.scan_dev_zsum_raster_batch_classes(c, spreds, scells, nx, sy, (2,), cnt.data_ptr(), zsum.data_ptr(), stream)

            def two_pass():
                zsum_2(); zrange_pass()

            w = nx * ny
            routes = {"canopy": canopy_pass((2,), BUT_7_18), "both_2": canopy_pass((2,), (2,)), "full": canopy_pass(ALL, ALL),
                      "zrange": zrange_pass, "zsum_2": zsum_2, "two_pass": two_pass}
            got = {}
            for k in ("canopy", "both_2", "full", "zrange"):
                routes[k]()
                torch.cuda.synchronize()
                got[k] = (zmin[:w].clone(), zmax[:w].clone())
            zsum_2()
            torch.cuda.synchronize()
            tag = f"{nx}x{ny}_{order}"
            checks[f"{tag}_full_sets_are_the_unfiltered_words"] = all(torch.equal(a, b) for a, b in zip(got["full"], got["zrange"]))
            if sy == ny:
                live = cnt[:w] != 0
                checks[f"{tag}_both_2_marks_the_cells_the_class_count_counts"] = bool(torch.equal(got["both_2"][0] != I32_MAX, live) and
                                                                                     torch.equal(got["both_2"][1] != I32_MIN, live))
            checks[f"{tag}_canopy_ground_is_both_2s"] = bool(torch.equal(got["canopy"][0], got["both_2"][0]) and
                                                             bool((got["canopy"][1] >= got["both_2"][1]).all()))
            if not lab:
                res = alternate(routes, reps)
                ratios = {f"{k}_over_{p}": res[k]["median_ms"] / res[p]["median_ms"] for k in ("canopy", "both_2", "full")
                          for p in ("zrange", "zsum_2", "two_pass")}
                print("(i)", json.dumps({"nx_ny": [nx, ny], "order": order, "files": files, "points_per_file": n, "zsum_2_cells": [nx, sy],
                                          "canopy_TBps_13B_per_point": points * 13 / (res["canopy"]["median_ms"] * 1e-3) / 1e12, **ratios, **res}),
                      flush=True)
            else:
                sweep = {}
                for wv in (3, 4, 5, 6, 8, 12, 16, 0):
                    if wv > 160 * 1024 // (256 + 8 * w) and wv != 0:
                        continue  # (above the LDS limit the entry runs the limit)
                    ctx.set_option("zrange_classes_waves_per_cu", wv)
                    r = alternate({k: routes[k] for k in ("canopy", "both_2", "full")}, max(3, reps // 2), warm=1)
                    torch.cuda.synchronize()
                    assert torch.equal(zmin[:w], got["full"][0]) and torch.equal(zmax[:w], got["full"][1]), wv
                    sweep[f"w{wv}" if wv else "shipped"] = {k: [round(v["median_ms"], 3), round(v["min_ms"], 3), round(v["max_ms"], 3)] for k, v in r.items()}
                print("(iii)", json.dumps({"nx_ny": [nx, ny], "order": order, "lds_limit_waves_per_cu": 160 * 1024 // (256 + 8 * w),
                                           "median_min_max_ms": sweep}), flush=True)
    del keep, cols, zmin, zmax, cnt, zsum
    torch.cuda.empty_cache()
if lab:
    print("checks", json.dumps(checks), flush=True)
    sys.exit(0)

# ---- (ii) the host entry against two searches into buffer collectors and the copies of their records ------------------------------
import _oracle  # only to WRITE the synthetic file (the generator lives in the oracle)
d = tempfile.mkdtemp(prefix="pcq_zrange_classes_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    oracle = _oracle.Oracle()
    s = doc_classes(specs.synth_ca13(points_per_file=nb, files=16)[5], nb)  # tile (1, 1)
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
    k, nx, ny = 36515, 64, 32  # (the cells of resident_zsum_classes_rate.py)
    cell = k * 0.01
    assert nx * k <= s.span[0] and ny * k <= s.span[1] and s.scale[0] == s.scale[1] == s.scale[2] == 0.01 and s.offset[2] == 0.0
    lo = (s.lo[0] * 0.01 + 0.005, s.lo[1] * 0.01 + 0.005, -1e9)
    hi = (lo[0] + nx * cell, lo[1] + ny * cell, 1e9)
    c_lo, c_hi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    gset = (C.c_uint32 * 8)(*binding.class_set_words((2,)))
    sset = (C.c_uint32 * 8)(*binding.class_set_words(BUT_7_18))
    zg, zs, zh = np.zeros(nx * ny), np.zeros(nx * ny), np.zeros(nx * ny)
    scanned = C.c_uint64()
    cap = nb + 1024
    records = np.zeros(cap, dtype=pkg.POINT_DTYPE)
    got_n = C.c_uint64()
    lmin, _ = pkg.box_to_local(list(lo), list(hi), list(s.scale), list(s.offset))
    host = {}

    def one_pass():
        assert lib.pcq_query_resident_bounds_canopy_raster(h, c_lo, 1e9, cell, nx, ny, gset, sset, zg.ctypes.data_as(dd), zs.ctypes.data_as(dd),
                                                           zh.ctypes.data_as(dd), C.byref(scanned)) == 0, lib.pcq_query_last_error()

    def search_and_copy(ground):
        def f():
            coll = vp()
            assert lib.pcq_query_collector_new_buffer(0, C.byref(coll)) == 0, lib.pcq_query_last_error()
            try:
                if ground:
                    assert lib.pcq_query_resident_search_bounds_class(h, c_lo, c_hi, 2, coll) == 0, lib.pcq_query_last_error()
                else:
                    assert lib.pcq_query_resident_search_bounds(h, c_lo, c_hi, coll) == 0, lib.pcq_query_last_error()
                assert lib.pcq_query_collector_points(coll, records.ctypes.data_as(vp), cap, C.byref(got_n)) == 0, lib.pcq_query_last_error()
            finally:
                lib.pcq_query_collector_free(coll)
            host["ground_records" if ground else "surface_records"] = got_n.value
        return f

    one_pass(); search_and_copy(True)()
    r = records[:got_n.value]
    cx = (np.rint(r["x"] / 0.01).astype(np.int64) - lmin[0]) // k
    cy = (np.rint(r["y"] / 0.01).astype(np.int64) - lmin[1]) // k
    sel = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
    at = (cy * nx + cx)[sel]
    by_cell = np.argsort(at, kind="stable")
    first = np.searchsorted(at[by_cell], np.arange(nx * ny))
    live = np.bincount(at, minlength=nx * ny) > 0
    hmin = np.full(nx * ny, np.nan)
    hmin[live] = np.minimum.reduceat(r["z"][sel][by_cell], first[live])
    checks["host_ground_agrees_to_1e-9"] = bool(np.array_equal(np.isnan(zg), ~live) and
                                                np.all(np.abs(zg[live] - hmin[live]) <= 1e-9 * np.maximum(1.0, np.abs(hmin[live]))))
    checks["host_height_is_the_difference"] = bool(np.array_equal(np.isnan(zh), np.isnan(zg) | np.isnan(zs)) and
                                                   np.array_equal(zh[~np.isnan(zh)], (zs - zg)[~np.isnan(zh)]))
    res = alternate({"one_pass": one_pass, "ground_search_and_copy": search_and_copy(True), "surface_search_and_copy": search_and_copy(False)},
                    reps, events=False)
    two = res["ground_search_and_copy"]["median_ms"] + res["surface_search_and_copy"]["median_ms"]
    checks["host_one_pass_faster_beyond_spread"] = res["one_pass"]["max_ms"] < res["ground_search_and_copy"]["min_ms"]
    checks["host_speedup_over_both_searches"] = two / res["one_pass"]["median_ms"]
    print("(ii)", json.dumps({"box": [list(lo), list(hi)], "nx_ny": [nx, ny], "cell_size": cell, "points_per_file": nb, "points_scanned": scanned.value,
                              "ground_records": host["ground_records"], "surface_records": host["surface_records"],
                              "cells_with_a_height": int((~np.isnan(zh)).sum()), "both_searches_and_copies_ms": two, **res}), flush=True)
    lib.pcq_query_resident_free(h)
finally:
    shutil.rmtree(d, ignore_errors=True)
print("checks", json.dumps(checks), flush=True)
