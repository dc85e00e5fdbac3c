"""Developer tool: box AND GPS time range (PCQ_PRED_BOUNDS_TIME) on resident data — what the batched launch and the two index
parts together buy.

(a) FILES resident synthetic files of N points each (positions of synth_ca13, times 0, 1, 2, ... as f64, the time blocks at 0 and
    8 modulo 16 in turn): pcq_scan_dev_count_batch_bounds_time over all of them against the only way to get that answer without
    it, a loop of pcq_scan_dev with PCQ_PRED_BOUNDS_TIME per file into one device counter; both timed with device events around
    the whole query, alternated, after 3 warm-up rounds; per point and against the 8 TB/s peak on 20 B/point.
(b) one file of N points in acquisition order — x slabs, y inside a slab (the order of tools/index_rate.py), the times 0, 1, 2, ...
    along it: coherent in space and in time at once — and the same points and times shuffled together.  An x slab of 1.5 f N
    consecutive points of the ordered file AND a range of 1.5 f N times that overlap in f N points, f = 0.1 %, 1 %, 10 %: each
    side alone keeps half as much again.  Count and records through pcq_scan_dev_indexed_bounds_time against pcq_scan_dev,
    alternated, medians of REPS rounds after 3 warm-up rounds with their minimum and maximum; counts and records compared, index
    statistics printed.  The last line restates the checks on the ratios.
usage: resident_bounds_time_rate.py [N [FILES [REPS]]]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
files = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
dev = torch.device("cuda:0")
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream


def spread(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "reps": len(v)}


def alternate(fns, reps, warm=3):
    """fns: name -> callable; one of each per round, device events around each, the first `warm` rounds dropped"""
    times = {k: [] for k in fns}
    for it in range(reps + warm):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record(); e1.synchronize()
            if it >= warm:
                times[k].append(e0.elapsed_time(e1))
    return {k: spread(v) for k, v in times.items()}


def faster_beyond_spread(r):
    """the indexed scans' slowest round is faster than the plain scans' fastest"""
    return r["indexed"]["max_ms"] < r["plain"]["min_ms"]


with pkg.Context(0) as ctx:
    spec = specs.synth_ca13(points_per_file=n)[5]
    sc = dict(scale=list(spec.scale), offset=list(spec.offset))
    lo = [spec.lo[a] for a in range(3)]
    hi = [spec.lo[0] + spec.span[0] // 2] + [spec.lo[a] + spec.span[a] for a in (1, 2)]
    line = torch.arange(n + 2, dtype=torch.float64, device=dev)

    # ---- (a) batched against the per-file loop --------------------------------------------------------------------
    keep, cols = [], []
    for f in range(files):
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), None, stream)
        t = line.clone()
        keep += [raw, t]
        cols.append(binding.make_columns(xyz=raw.data_ptr(), cls=t.data_ptr() + 8 * (f % 2), n=n, cls_stride=8, **sc))
    torch.cuda.synchronize()
    preds = [pkg.Predicate.bounds_time(lo, hi, float(n // 4), float(n // 4 + n // 2))] * files
    counter = torch.zeros(2, dtype=torch.int64, device=dev)
    cc = ctx.count_collector(device_counter=counter.data_ptr())
    got = {}

    def batched():
        counter.zero_()
        ctx.scan_dev_count_batch_bounds_time(cols, preds, counter.data_ptr(), stream)

    def loop():
        counter.zero_()
        for c, p in zip(cols, preds):
            ctx.scan_dev(c, p, cc, stream)

    for name, fn in (("batched", batched), ("per_file_loop", loop)):
        fn()
        torch.cuda.synchronize()
        got[name] = int(counter[0].item())
    assert got["batched"] == got["per_file_loop"], got
    res = alternate({"batched": batched, "per_file_loop": loop}, reps)
    for k, v in res.items():
        v["ns_per_Mpoint"] = v["median_ms"] * 1e6 / (files * n / 1e6)
        v["TBps_20B_per_point"] = files * n * 20 / (v["median_ms"] * 1e-3) / 1e12
        v["fraction_of_8TBps"] = v["TBps_20B_per_point"] / 8.0
    print("(a)", json.dumps({"files": files, "points_per_file": n, "matches": got["batched"],
                             "batched_over_loop": res["batched"]["median_ms"] / res["per_file_loop"]["median_ms"], **res}), flush=True)
    cc.free()
    raw0 = keep[0]
    del keep, cols
    torch.cuda.empty_cache()

    # ---- (b) through the chunk index against the plain scan -------------------------------------------------------
    pts = raw0.view(n, 3)
    key = ((pts[:, 0].long() - int(spec.lo[0])) * 2048 // int(spec.span[0])) * (1 << 32) + (pts[:, 1].long() - int(spec.lo[1]))
    order = torch.argsort(key)
    coh = pts[order].contiguous()          # acquisition order: point i was taken at time i
    coh_t = line[:n].contiguous()
    del key, order
    perm = torch.randperm(n, device=dev)
    shuf, shuf_t = coh[perm].contiguous(), coh_t[perm].contiguous()
    del perm
    torch.cuda.synchronize()
    checks = {}
    for label, p, t in (("ordered", coh, coh_t), ("shuffled", shuf, shuf_t)):
        cols1 = binding.make_columns(xyz=p.data_ptr(), cls=t.data_ptr(), n=n, cls_stride=8, **sc)
        ix = ctx.index_new()
        for frac in (0.001, 0.01, 0.1):
            a, m = int(n * 0.37), int(n * frac)
            # the slab: the x values of the ordered file's points a .. a + 1.5 m (whole slabs: a little more at either end)
            x0, x1 = int(coh[a, 0].item()), int(coh[a + m + m // 2, 0].item())
            pred = pkg.Predicate.bounds_time([x0, -2 ** 31, -2 ** 31], [x1, 2 ** 31 - 1, 2 ** 31 - 1], float(a + m // 2), float(a + 2 * m))
            out = {}
            for kind in ("count", "records"):
                mk = ctx.count_collector if kind == "count" else ctx.buffer_collector
                g = {False: mk(), True: mk()}

                def run(indexed):
                    g[indexed].reset()
                    if indexed: ctx.scan_dev_indexed_bounds_time(cols1, pred, ix, g[indexed], stream)
                    else: ctx.scan_dev(cols1, pred, g[indexed], stream)

                r = alternate({"plain": lambda: run(False), "indexed": lambda: run(True)}, reps)
                assert g[False].point_count() == g[True].point_count() > 0, (label, frac, kind)
                if kind == "records":
                    assert g[False].points().tobytes() == g[True].points().tobytes(), (label, frac)
                st = ctx.index_stats(ix)
                out[kind] = {"matches": g[True].point_count(), "plain": r["plain"], "indexed": r["indexed"],
                             "speedup": r["plain"]["median_ms"] / r["indexed"]["median_ms"],
                             "chunks": st["chunks"], "skipped": st["skipped"], "whole": st["whole"], "scanned": st["scanned"]}
                for x in g.values(): x.free()
                if label == "ordered":
                    checks[f"ordered_x{frac}_{kind}_faster_beyond_spread"] = faster_beyond_spread(r)
                checks[f"{label}_x{frac}_{kind}_speedup"] = out[kind]["speedup"]
            print("(b)", label, f"x{frac}", json.dumps(out), flush=True)
        ctx.index_free(ix)
    print("checks", json.dumps(checks), flush=True)
