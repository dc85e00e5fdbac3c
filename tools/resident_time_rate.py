"""Developer tool: GPS time ranges (PCQ_PRED_TIME) on a resident time column — what the time part of the chunk index buys.

One file of N points: positions of synth_ca13, times 0, 1, 2, ... as f64, once in that (acquisition) order and once shuffled.
Ranges [t0, t0 + frac * N) keeping about 0.1 %, 1 % and 10 % of the 4096-point chunks of the sorted column (and the same share
of the points of either).  Count and records through pcq_scan_dev_indexed_time against pcq_scan_dev — the only path without
the index — alternated, timed with device events around each scan, medians of REPS rounds after 3 warm-up rounds with their
minimum and maximum; counts and records compared, index statistics printed.  The last line restates the checks on the ratios.
usage: resident_time_rate.py [N [REPS]]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
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


def within_spread(r):
    """the two sets of rounds overlap, or the indexed median is the smaller"""
    return r["indexed"]["median_ms"] <= r["plain"]["median_ms"] or r["indexed"]["min_ms"] <= r["plain"]["max_ms"]


with pkg.Context(0) as ctx:
    spec = specs.synth_ca13(points_per_file=n)[5]
    sc = dict(scale=list(spec.scale), offset=list(spec.offset))
    raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
    ctx.synth_fill(spec, 0, n, raw.data_ptr(), None, stream)
    sorted_t = torch.arange(n, dtype=torch.float64, device=dev)
    shuffled_t = sorted_t[torch.randperm(n, device=dev)].contiguous()
    torch.cuda.synchronize()
    checks = {}
    for label, t in (("sorted", sorted_t), ("shuffled", shuffled_t)):
        cols = binding.make_columns(xyz=raw.data_ptr(), cls=t.data_ptr(), n=n, cls_stride=8, **sc)
        ix = ctx.index_new()
        for frac in (0.001, 0.01, 0.1):
            t0 = float(int(n * 0.37))
            pred = pkg.Predicate.time_range(t0, t0 + float(int(n * frac)))
            out = {}
            for kind in ("count", "records"):
                mk = ctx.count_collector if kind == "count" else ctx.buffer_collector
                g = {False: mk(), True: mk()}

                def run(indexed):
                    g[indexed].reset()
                    if indexed: ctx.scan_dev_indexed_time(cols, pred, ix, g[indexed], stream)
                    else: ctx.scan_dev(cols, pred, g[indexed], stream)

                r = alternate({"plain": lambda: run(False), "indexed": lambda: run(True)}, reps)
                assert g[False].point_count() == g[True].point_count() == int(n * frac), (label, frac, kind)
                if kind == "records":
                    assert g[False].points().tobytes() == g[True].points().tobytes(), (label, frac)
                st = ctx.index_stats(ix)
                out[kind] = {"matches": g[True].point_count(), "plain": r["plain"], "indexed": r["indexed"],
                             "speedup": r["plain"]["median_ms"] / r["indexed"]["median_ms"],
                             "chunks": st["chunks"], "skipped": st["skipped"], "whole": st["whole"], "scanned": st["scanned"]}
                for x in g.values(): x.free()
                if (label, frac) == ("sorted", 0.01):
                    checks[f"sorted_1pct_{kind}_faster_beyond_spread"] = faster_beyond_spread(r)
                    checks[f"sorted_1pct_{kind}_speedup"] = out[kind]["speedup"]
                if label == "shuffled":
                    if kind == "records":
                        checks[f"shuffled_x{frac}_records_within_spread"] = within_spread(r)
                    checks[f"shuffled_x{frac}_{kind}_speedup"] = out[kind]["speedup"]
            print(label, f"x{frac}", json.dumps(out), flush=True)
        ctx.index_free(ix)
    print("checks", json.dumps(checks), flush=True)
