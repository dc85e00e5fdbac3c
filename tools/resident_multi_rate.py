"""Developer tool: many boxes in one pass on resident data — how many boxes a tile's wait for HBM hides.

(a) dense: FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13) and Q = 2, 4, 8 XL-like boxes (the
    ca13_XL box, shrunk by 10 m per query along x and y: every (file, box) pair is live).  ONE pcq_scan_dev_count_batch_multi
    against Q launches of pcq_scan_dev_count_batch in a row — the only way to the same Q answers without it — both timed with
    device events around the whole of it, alternated, REPS rounds after 3 warm-up rounds; median, minimum and maximum, TB/s on
    12 B/point (the one pass: of the data once; the Q launches: of the data Q times), counts compared.
    Rule, per Q: the one pass's slowest round is below the Q launches' fastest round.
(b) sparse: the same 16 tiles as LAST files of NB points each in a resident dataset of the host layer, and 8 boxes that each meet
    1 - 4 of the tiles: pcq_query_resident_count_bounds_many against 8 calls of pcq_query_resident_count_bounds, wall time of
    the whole call (these entries wait for their answer themselves), alternated the same way; matches, points_scanned compared.
(c) with PCQ_LAB=1 (libpcq_lab.so accepts the option "multi_waves_per_cu"): the one pass of (a) at 3 .. 24 workgroups per CU,
    for each Q; (b) is then left out.
The last line restates the checks.
usage: resident_multi_rate.py [N [FILES [REPS [NB]]]]"""
import ctypes as C
import importlib, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
files = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
nb = int(sys.argv[4]) if len(sys.argv) > 4 else 8_000_000
dev = torch.device("cuda:0")
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream


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


checks = {}
with pkg.Context(0) as ctx:
    # ---- (a) dense: one pass against Q launches ---------------------------------------------------------------------
    tiles = specs.synth_ca13(points_per_file=n, files=files)
    keep, cols = [], []
    for spec in tiles:
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), None, stream)
        keep.append(raw)
        cols.append(binding.make_columns(xyz=raw.data_ptr(), n=n, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    bmin, bmax = specs.box("ca13_XL")
    counter = torch.zeros(16, dtype=torch.int64, device=dev)

    def make_rows(nq):
        rows = []
        for spec in tiles:
            row = []
            for q in range(nq):
                lo = [bmin[0] + 10.0 * q, bmin[1] + 10.0 * q, bmin[2]]
                hi = [bmax[0] - 10.0 * q, bmax[1] - 10.0 * q, bmax[2]]
                row.append(pkg.Predicate.bounds(*pkg.box_to_local(lo, hi, list(spec.scale), list(spec.offset))))
            rows.append(row)
        return rows

    for nq in (2, 4, 8):
        rows = make_rows(nq)
        by_query = [[row[q] for row in rows] for q in range(nq)]

        def one_pass():
            counter.zero_()
            ctx.scan_dev_count_batch_multi(cols, rows, counter.data_ptr(), stream)

        def launches():
            counter.zero_()
            for q in range(nq):
                ctx.scan_dev_count_batch(cols, by_query[q], counter.data_ptr() + 8 * q, stream)

        got = {}
        for name, fn in (("one_pass", one_pass), ("launches", launches)):
            fn()
            torch.cuda.synchronize()
            got[name] = counter[:nq].tolist()
        assert got["one_pass"] == got["launches"] and all(c > 0 for c in got["one_pass"]), got
        res = alternate({"one_pass": one_pass, "launches": launches}, reps)
        res["one_pass"]["TBps_12B_per_point"] = files * n * 12 / (res["one_pass"]["median_ms"] * 1e-3) / 1e12
        res["launches"]["TBps_12B_per_point"] = nq * files * n * 12 / (res["launches"]["median_ms"] * 1e-3) / 1e12
        res["one_pass"]["Gpoint_boxes_per_s"] = nq * files * n / (res["one_pass"]["median_ms"] * 1e-3) / 1e9
        res["launches"]["Gpoint_boxes_per_s"] = nq * files * n / (res["launches"]["median_ms"] * 1e-3) / 1e9
        speedup = res["launches"]["median_ms"] / res["one_pass"]["median_ms"]
        checks[f"dense_Q{nq}_faster_beyond_spread"] = res["one_pass"]["max_ms"] < res["launches"]["min_ms"]
        checks[f"dense_Q{nq}_speedup"] = speedup
        print("(a)", json.dumps({"Q": nq, "files": files, "points_per_file": n, "matches": got["one_pass"], "speedup": speedup, **res}), flush=True)
    lab = os.environ.get("PCQ_LAB") == "1"
    if lab:  # ---- (c) the one pass at other grids ----------------------------------------------------------------------
        for nq in (2, 4, 8):
            rows = make_rows(nq)
            out = {}
            for w in (3, 4, 6, 8, 12, 16, 24):
                ctx.set_option("multi_waves_per_cu", w)
                r = alternate({"one_pass": lambda: ctx.scan_dev_count_batch_multi(cols, rows, counter.data_ptr(), stream)}, reps)["one_pass"]
                r["TBps_12B_per_point"] = files * n * 12 / (r["median_ms"] * 1e-3) / 1e12
                out[w] = r
            ctx.set_option("multi_waves_per_cu", 0)
            print("(c)", json.dumps({"Q": nq, "by_waves_per_cu": out}), flush=True)
    del keep, cols
    torch.cuda.empty_cache()
if lab:
    print("checks", json.dumps(checks), flush=True)
    sys.exit(0)

# ---- (b) sparse: count_bounds_many against 8 calls of count_bounds ------------------------------------------------------
import _oracle  # only to WRITE the synthetic files (the generator lives in the oracle)
d = tempfile.mkdtemp(prefix="pcq_multi_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    oracle = _oracle.Oracle()
    tiles = specs.synth_ca13(points_per_file=nb, files=16)
    paths = []
    for i, s in enumerate(tiles):
        p = os.path.join(d, f"ca13_{i}.last")
        oracle.synth_write(s, p, threads=16)
        paths.append(p)
    lib = pkg.load_query_library()
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    h = C.c_void_p()
    assert lib.pcq_query_resident_load(0, arr, len(paths), C.byref(h)) == 0, lib.pcq_query_last_error()
    # tile (tx, ty) is x in [x0 + tx wx, x0 + (tx + 1) wx), y alike (metres); boxes of 1x1, 2x1, 1x2 and 2x2 tiles, well inside them
    hf = [specs.header_fields(s) for s in tiles]
    x0, y0 = hf[0]["min"][0], hf[0]["min"][1]
    wx, wy = hf[1]["min"][0] - x0, hf[4]["min"][1] - y0
    shapes = [(0, 0, 1, 1), (3, 3, 1, 1), (1, 0, 2, 1), (0, 2, 1, 2), (2, 2, 2, 2), (1, 1, 2, 2), (2, 0, 1, 1), (0, 1, 2, 1)]
    boxes = [((x0 + (tx + 0.2) * wx, y0 + (ty + 0.2) * wy, 0.0), (x0 + (tx + sx - 0.2) * wx, y0 + (ty + sy - 0.2) * wy, 480.0))
             for tx, ty, sx, sy in shapes]
    met = [sum(specs.aabb_intersects(f["min"], f["max"], b[0], b[1]) for f in hf) for b in boxes]
    assert met == [sx * sy for _, _, sx, sy in shapes] and min(met) == 1 and max(met) == 4, met
    nbx = len(boxes)
    lo = (C.c_double * (3 * nbx))(*[v for b in boxes for v in b[0]])
    hi = (C.c_double * (3 * nbx))(*[v for b in boxes for v in b[1]])
    m_many, s_many, read = (C.c_uint64 * nbx)(), (C.c_uint64 * nbx)(), C.c_uint64()
    m_one, s_one = (C.c_uint64 * nbx)(), (C.c_uint64 * nbx)()

    def many():
        assert lib.pcq_query_resident_count_bounds_many(h, nbx, lo, hi, m_many, s_many, C.byref(read)) == 0, lib.pcq_query_last_error()

    def calls():
        for q, b in enumerate(boxes):
            m, s = C.c_uint64(), C.c_uint64()
            assert lib.pcq_query_resident_count_bounds(h, (C.c_double * 3)(*b[0]), (C.c_double * 3)(*b[1]), C.byref(m), C.byref(s)) == 0
            m_one[q], s_one[q] = m.value, s.value

    many(); calls()
    assert list(m_many) == list(m_one) and list(s_many) == list(s_one) and all(c > 0 for c in m_many), (list(m_many), list(m_one))
    res = alternate({"many": many, "calls": calls}, reps, events=False)
    union = sum(any(specs.aabb_intersects(f["min"], f["max"], b[0], b[1]) for b in boxes) for f in hf)
    assert read.value == union * nb
    speedup = res["calls"]["median_ms"] / res["many"]["median_ms"]
    checks["sparse_faster_beyond_spread"] = res["many"]["max_ms"] < res["calls"]["min_ms"]
    checks["sparse_speedup"] = speedup
    print("(b)", json.dumps({"boxes": nbx, "tiles_met_per_box": met, "points_per_file": nb, "points_read_many": read.value,
                             "points_scanned_calls": sum(s_one), "matches": list(m_many), "speedup": speedup, **res}), flush=True)
    lib.pcq_query_resident_free(h)
finally:
    shutil.rmtree(d, ignore_errors=True)
print("checks", json.dumps(checks), flush=True)
