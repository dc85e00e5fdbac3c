"""Developer tool: the mean-height raster of a set of classes on resident data — one pass that adds every point inside the box whose
class byte is in the set into the count and the z sum of its cell of an nx x ny raster over x and y.

(i)   FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13 with the classes of synth-doc: 45 % class 2), in
      the generator's order, the class block of every file 3 bytes off a dword.  The ca13_XL box with z unbounded, which keeps every
      point.  Rasters of 8 x 8 and 64 x 32 cells (PCQ_ZSUM_CELLS_MAX) over the box's x and y.  Per raster four routes, timed with
      device events around the whole of each, alternated in one process on identical input, REPS rounds after 3 warm-up rounds;
      median, minimum and maximum:
        classes_2    ONE pcq_scan_dev_zsum_raster_batch_classes, set {2}, its words zeroed by two fills (13 B/point);
        classes_all  the same with all 256 classes;
        zsum         ONE pcq_scan_dev_zsum_raster_batch at the same cells, its words zeroed the same way (12 B/point): the unfiltered
                     pass;
        combined     ONE pcq_scan_dev_count_batch_combined for class 2 (13 B/point): the floor — the same bytes, a popcount.
      classes_all must give the unfiltered pass's words, the counts of classes_2 must add up to the floor's count.
(ii)  (not with PCQ_LAB=1) ONE tile — tile (1, 1) — as a LAST file of NB points in a resident dataset of the host layer
      (pcq_query_resident_load_points), 64 x 32 square cells over the lower half of it (about half its points), z unbounded:
      pcq_query_resident_bounds_zmean_raster_classes with the set {2} against the route it replaces,
      pcq_query_resident_search_bounds_class (class 2) into a buffer collector, pcq_query_collector_points to host memory (31 B per
      match) and the reduction of the records on the host (two np.bincount).  Wall time of the whole of each, alternated the same way.
      The counts must agree exactly and the means to 1e-9 relative.
(iii) with PCQ_LAB=1 (libpcq_lab.so accepts the option "zsum_classes_waves_per_cu"): classes_2 and classes_all of (i) at 3 .. 16
      workgroups per CU before the LDS limit (160 KiB / (256 + 16 nx ny): 4 at 2048 cells).
The last line restates the checks.
usage: resident_zsum_classes_rate.py [N [FILES [REPS [NB]]]]"""
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
RASTERS = ((8, 8), (64, 32))
ALL = tuple(range(256))


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


def doc_classes(spec):
    """the positions of ca13, the classes of synth-doc"""
    doc = specs.synth_doc(points_per_file=n, files=1)[0]
    spec.n_classes = doc.n_classes
    for j in range(8):
        spec.cls_val[j], spec.cls_cum16[j] = doc.cls_val[j], doc.cls_cum16[j]
    return spec


checks = {}
with pkg.Context(0) as ctx:
    # ---- (i) the filtered pass against the unfiltered one and the box AND class count, (iii) at other grids -------------------
    tiles = [doc_classes(s) for s in specs.synth_ca13(points_per_file=n, files=files)]
    bmin, bmax = specs.box("ca13_XL")
    keep, cols = [], []
    for spec in tiles:
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        cb = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), cb.data_ptr() + 3, stream)
        keep += [raw, cb]
        assert raw.data_ptr() % 16 == 0 and (cb.data_ptr() + 3) % 4 == 3
        cols.append(binding.make_columns(xyz=raw.data_ptr(), cls=cb.data_ptr() + 3, n=n, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(tiles[0].scale), list(tiles[0].offset))
    assert all(pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) == (lmin, lmax) for s in tiles)
    cnt = torch.zeros(2048, dtype=torch.int64, device=dev)
    zsum = torch.zeros(2048, dtype=torch.int64, device=dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    points = files * n
    assert points < 2**32  # (one launch: the sums cannot wrap)
    for nx, ny in RASTERS:
        cw = [-(-(lmax[a] - lmin[a] + 1) // d) for a, d in ((0, nx), (1, ny))]
        lo, hi = [lmin[0], lmin[1], -2**40], [lmin[0] + nx * cw[0] - 1, lmin[1] + ny * cw[1] - 1, 2**40]
        preds = [pkg.Predicate.bounds(lo, hi)] * files
        class2 = [pkg.Predicate.bounds_class(lo, hi, 2)] * files
        cells = [cw] * files

        def classes_pass(classes):
            def f():
                cnt.zero_(); zsum.zero_()
                ctx.scan_dev_zsum_raster_batch_classes(cols, preds, cells, nx, ny, classes, cnt.data_ptr(), zsum.data_ptr(), stream)
            return f

        def zsum_pass():
            cnt.zero_(); zsum.zero_()
            ctx.scan_dev_zsum_raster_batch(cols, preds, cells, nx, ny, cnt.data_ptr(), zsum.data_ptr(), stream)

        def combined():
            counter.zero_()
            ctx.scan_dev_count_batch_combined(cols, class2, counter.data_ptr(), stream)

        w = nx * ny
        routes = {"classes_2": classes_pass((2,)), "classes_all": classes_pass(ALL), "zsum": zsum_pass, "combined": combined}
        got = {}
        for k in ("classes_2", "classes_all", "zsum"):
            routes[k]()
            torch.cuda.synchronize()
            got[k] = (cnt[:w].clone(), zsum[:w].clone())
        combined()
        torch.cuda.synchronize()
        tag = f"{nx}x{ny}"
        checks[f"{tag}_all_classes_are_the_unfiltered_words"] = all(torch.equal(a, b) for a, b in zip(got["classes_all"], got["zsum"])) and \
            int(got["zsum"][0].sum()) == points
        checks[f"{tag}_class_2_counts_add_up_to_the_floors"] = int(got["classes_2"][0].sum()) == int(counter[0]) and 0 < int(counter[0]) < points
        if not lab:
            res = alternate(routes, reps)
            print("(i)", json.dumps({"nx_ny": [nx, ny], "files": files, "points_per_file": n, "class_2_share": int(counter[0]) / points,
                                      "classes_2_over_zsum": res["classes_2"]["median_ms"] / res["zsum"]["median_ms"],
                                      "classes_all_over_zsum": res["classes_all"]["median_ms"] / res["zsum"]["median_ms"],
                                      "classes_2_over_combined": res["classes_2"]["median_ms"] / res["combined"]["median_ms"],
                                      "classes_all_over_combined": res["classes_all"]["median_ms"] / res["combined"]["median_ms"],
                                      "classes_2_TBps_13B_per_point": points * 13 / (res["classes_2"]["median_ms"] * 1e-3) / 1e12, **res}), flush=True)
        else:
            sweep = {}
            for wv in (3, 4, 5, 6, 8, 12, 16, 0):
                if wv > 160 * 1024 // (256 + 16 * w) and wv != 0:
                    continue  # (above the LDS limit the entry runs the limit)
                ctx.set_option("zsum_classes_waves_per_cu", wv)
                r = alternate({"classes_2": routes["classes_2"], "classes_all": routes["classes_all"]}, max(3, reps // 2), warm=1)
                torch.cuda.synchronize()
                assert torch.equal(cnt[:w], got["classes_all"][0]) and torch.equal(zsum[:w], got["classes_all"][1]), wv
                sweep[f"w{wv}" if wv else "shipped"] = {k: [round(v["median_ms"], 3), round(v["min_ms"], 3), round(v["max_ms"], 3)] for k, v in r.items()}
            print("(iii)", json.dumps({"nx_ny": [nx, ny], "lds_limit_waves_per_cu": 160 * 1024 // (256 + 16 * w), "median_min_max_ms": sweep}), flush=True)
    del keep, cols, cnt, zsum, counter
    torch.cuda.empty_cache()
if lab:
    print("checks", json.dumps(checks), flush=True)
    sys.exit(0)

# ---- (ii) the host entry against a class search into a buffer collector, the copy of its records and their reduction on the host ----
import _oracle  # only to WRITE the synthetic file (the generator lives in the oracle)
d = tempfile.mkdtemp(prefix="pcq_zsum_classes_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    oracle = _oracle.Oracle()
    s = doc_classes(specs.synth_ca13(points_per_file=nb, files=16)[5])  # tile (1, 1)
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
    k, nx, ny = 36515, 64, 32  # (the cells of resident_zsum_rate.py)
    cell = k * 0.01
    assert nx * k <= s.span[0] and ny * k <= s.span[1] and s.scale[0] == s.scale[1] == s.scale[2] == 0.01 and s.offset[2] == 0.0
    lo = (s.lo[0] * 0.01 + 0.005, s.lo[1] * 0.01 + 0.005, -1e9)
    hi = (lo[0] + nx * cell, lo[1] + ny * cell, 1e9)
    c_lo, c_hi = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
    cset = (C.c_uint32 * 8)(*binding.class_set_words((2,)))
    count, zmean = np.zeros(nx * ny, dtype=np.uint64), np.zeros(nx * ny)
    scanned = C.c_uint64()
    cap = nb + 1024
    records = np.zeros(cap, dtype=pkg.POINT_DTYPE)
    got_n = C.c_uint64()
    lmin, _ = pkg.box_to_local(list(lo), list(hi), list(s.scale), list(s.offset))
    host = {"copied_ms": []}

    def one_pass():
        assert lib.pcq_query_resident_bounds_zmean_raster_classes(h, c_lo, 1e9, cell, nx, ny, cset, count.ctypes.data_as(pu64),
                                                                  zmean.ctypes.data_as(dd), C.byref(scanned)) == 0, lib.pcq_query_last_error()

    def search_copy_and_reduce():
        t0 = time.perf_counter()
        coll = vp()
        assert lib.pcq_query_collector_new_buffer(0, C.byref(coll)) == 0, lib.pcq_query_last_error()
        try:
            assert lib.pcq_query_resident_search_bounds_class(h, c_lo, c_hi, 2, coll) == 0, lib.pcq_query_last_error()
            assert lib.pcq_query_collector_points(coll, records.ctypes.data_as(vp), cap, C.byref(got_n)) == 0, lib.pcq_query_last_error()
        finally:
            lib.pcq_query_collector_free(coll)
        host["copied_ms"].append((time.perf_counter() - t0) * 1e3)
        r = records[:got_n.value]
        cx = (np.rint(r["x"] / 0.01).astype(np.int64) - lmin[0]) // k
        cy = (np.rint(r["y"] / 0.01).astype(np.int64) - lmin[1]) // k
        sel = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
        at = (cy * nx + cx)[sel]
        host["count"] = np.bincount(at, minlength=nx * ny)
        host["sum"] = np.bincount(at, weights=r["z"][sel], minlength=nx * ny)

    one_pass(); search_copy_and_reduce()
    hmean = host["sum"] / np.maximum(host["count"], 1)
    liveh = host["count"] > 0
    checks["host_counts_agree"] = bool(np.array_equal(host["count"].astype(np.uint64), count))
    checks["host_means_agree_to_1e-9"] = bool(np.array_equal(np.isnan(zmean), ~liveh) and
                                              np.all(np.abs(zmean[liveh] - hmean[liveh]) <= 1e-9 * np.maximum(1.0, np.abs(hmean[liveh]))))
    res = alternate({"one_pass": one_pass, "search_copy_and_reduce": search_copy_and_reduce}, reps, events=False)
    checks["host_one_pass_faster_beyond_spread"] = res["one_pass"]["max_ms"] < res["search_copy_and_reduce"]["min_ms"]
    checks["host_speedup"] = res["search_copy_and_reduce"]["median_ms"] / res["one_pass"]["median_ms"]
    print("(ii)", json.dumps({"box": [list(lo), list(hi)], "nx_ny": [nx, ny], "cell_size": cell, "points_per_file": nb, "points_scanned": scanned.value,
                              "records": got_n.value, "record_bytes": got_n.value * 31, "cells_hit": int(liveh.sum()),
                              "search_and_copy_alone": spread(host["copied_ms"][-reps:]), "speedup": checks["host_speedup"], **res}), flush=True)
    lib.pcq_query_resident_free(h)
finally:
    shutil.rmtree(d, ignore_errors=True)
print("checks", json.dumps(checks), flush=True)
