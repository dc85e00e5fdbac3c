"""Developer tool: the time histogram of a box on resident data — one pass that bins the GPS time of every point inside the box,
against the only other way to the same answer: one box AND time pass per bin.

FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13) with f64 times
(a) acquisition-ordered: file f holds f * N .. (f + 1) * N - 1 seconds in point order, so a wave's tile lies in one bin, and
(b) shuffled: a random permutation of (a) within each file, so neighbouring points lie in unrelated bins,
and a box that keeps every point.  The edges divide the whole time line [0, FILES * N) evenly into nbins = 8, 64, 1024 bins.
Per kind of times and nbins the routes, each timed with device events around the whole of it, alternated in one process, REPS
rounds after 3 warm-up rounds; median, minimum and maximum, TB/s on 20 B/point:
  hist        ONE pcq_scan_dev_time_hist_batch;
  one_range   ONE pcq_scan_dev_count_batch_bounds_time (the first bin's range): the floor — the same bytes, two compares
              instead of a bin;
  per_range   (nbins = 8 only) one pcq_scan_dev_count_batch_bounds_time per bin: what a caller did before.
The histogram is compared with the per-range counts (nbins = 8) and must sum to the number of points (every nbins).
ratio_to_one_pass = hist / one_range.  Rule: for nbins = 8, hist's slowest round is below per_range's fastest round, on (a) and (b).
(c) with PCQ_LAB=1 (libpcq_lab.so accepts the option "time_hist_waves_per_cu"): the one pass on (a) and (b) with 8 and 1024 bins at
    3 .. 16 workgroups per CU.
The last line restates the checks.
usage: resident_time_hist_rate.py [N [FILES [REPS]]]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
files = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
dev = torch.device("cuda:0")
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream
lab = os.environ.get("PCQ_LAB") == "1"
FULL = ([-2**40] * 3, [2**40] * 3)
BINS = (8, 64, 1024)


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


def tbps(passes, ms):
    return passes * files * n * 20 / (ms * 1e-3) / 1e12


checks = {}
with pkg.Context(0) as ctx:
    tiles = specs.synth_ca13(points_per_file=n, files=files)
    keep, cols = [], {"a": [], "b": []}
    gen = torch.Generator(device=dev); gen.manual_seed(33)
    for f, spec in enumerate(tiles):
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), cls.data_ptr(), stream)
        ta = torch.arange(f * n, (f + 1) * n, dtype=torch.float64, device=dev)
        tb = ta[torch.randperm(n, device=dev, generator=gen)]
        keep += [raw, ta, tb]
        del cls
        for name, t in (("a", ta), ("b", tb)):
            cols[name].append(binding.make_columns(xyz=raw.data_ptr(), cls=t.data_ptr(), n=n, cls_stride=8, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    boxes = [pkg.Predicate.bounds(*FULL) for _ in tiles]
    hist = torch.zeros(max(BINS), dtype=torch.int64, device=dev)
    counter = torch.zeros(max(BINS), dtype=torch.int64, device=dev)

    for name, what in (("a", "acquisition-ordered"), ("b", "shuffled within each file")):
        c = cols[name]
        for nbins in BINS:
            edges = np.linspace(0.0, float(files) * n, nbins + 1)
            ranges = [[pkg.Predicate.bounds_time(*FULL, float(edges[b]), float(edges[b + 1])) for _ in tiles] for b in range(nbins if nbins == 8 else 1)]

            def one_hist():
                hist.zero_()
                ctx.scan_dev_time_hist_batch(c, boxes, edges, hist.data_ptr(), stream)

            def one_range():
                counter.zero_()
                ctx.scan_dev_count_batch_bounds_time(c, ranges[0], counter.data_ptr(), stream)

            def per_range():
                counter.zero_()
                for b in range(nbins):
                    ctx.scan_dev_count_batch_bounds_time(c, ranges[b], counter.data_ptr() + 8 * b, stream)

            one_hist()
            torch.cuda.synchronize()
            h = hist.tolist()
            assert sum(h[:nbins]) == files * n and not any(h[nbins:]), (nbins, sum(h))
            routes = {"hist": one_hist, "one_range": one_range}
            if nbins == 8:
                per_range()
                torch.cuda.synchronize()
                assert counter.tolist()[:nbins] == h[:nbins], (h[:nbins], counter.tolist()[:nbins])
                routes["per_range"] = per_range
            res = alternate(routes, reps)
            res["hist"]["TBps_20B_per_point"] = tbps(1, res["hist"]["median_ms"])
            res["one_range"]["TBps_20B_per_point"] = tbps(1, res["one_range"]["median_ms"])
            ratio = res["hist"]["median_ms"] / res["one_range"]["median_ms"]
            checks[f"{name}_{nbins}_ratio_to_one_pass"] = ratio
            checks[f"{name}_{nbins}_hist_TBps"] = res["hist"]["TBps_20B_per_point"]
            line = {"times": what, "files": files, "points_per_file": n, "nbins": nbins, "ratio_to_one_pass": ratio}
            if nbins == 8:
                res["per_range"]["TBps_20B_per_point"] = tbps(nbins, res["per_range"]["median_ms"])
                checks[f"{name}_8_hist_faster_than_per_range_beyond_spread"] = res["hist"]["max_ms"] < res["per_range"]["min_ms"]
                checks[f"{name}_8_speedup"] = line["speedup"] = res["per_range"]["median_ms"] / res["hist"]["median_ms"]
            print(f"({name})", json.dumps({**line, **res}), flush=True)
    if lab:  # ---- (c) the one pass at other grids ------------------------------------------------------------------------------
        for nbins in (8, 1024):
            edges = np.linspace(0.0, float(files) * n, nbins + 1)
            out = {"a": {}, "b": {}}
            for w in (3, 4, 5, 6, 8, 10, 12, 16):
                ctx.set_option("time_hist_waves_per_cu", w)
                r = alternate({k: (lambda k=k: ctx.scan_dev_time_hist_batch(cols[k], boxes, edges, hist.data_ptr(), stream)) for k in ("a", "b")},
                              max(3, reps // 2))
                for k in ("a", "b"):
                    r[k]["TBps_20B_per_point"] = tbps(1, r[k]["median_ms"])
                    out[k][w] = r[k]
            ctx.scan_dev_time_hist_batch(cols["b"], boxes, edges, hist.zero_().data_ptr(), stream)
            torch.cuda.synchronize()
            assert hist.sum().item() == files * n, nbins
            print("(c)", json.dumps({"nbins": nbins, "by_waves_per_cu": out}), flush=True)
        ctx.set_option("time_hist_waves_per_cu", 0)
    del keep, cols
print("checks", json.dumps(checks), flush=True)
