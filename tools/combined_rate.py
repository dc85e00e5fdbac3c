"""Developer tool: rates of the combined searches (PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_BOUNDS_TIME) next to the bounds search.

Over one resident LAST-like dataset of n points (default 163 M): the synthetic positions of tools/time_rate.py, class bytes
(i mod 7) and GPS times gps = i * 0.001, in HBM:
  * count: K1 (bounds, 12 B/point) and K1 with its second column (bounds AND class 13 B/point, bounds AND time 20 B/point),
    timed with device events after warm-up, each against the 8 TB/s peak on its algorithmic bytes;
  * records: buffer collector, the box keeping about half of the points and the attribute about 1 / 7 or 10 % of those;
  * density: grid collector with 100 m cells over the file's box.
--cli DIR: `query --combine` per file with PCQ_TIMING=1 next to the bounds-only search (the first run warms the page cache).
Kernel times come from a separate run under rocprofv3 --kernel-trace --stats."""
import importlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

args = [a for a in sys.argv[1:] if not a.startswith("--")]
CLI = sys.argv[sys.argv.index("--cli") + 1] if "--cli" in sys.argv else None
if CLI:
    args = [a for a in args if a != CLI]
n = int(args[0]) if args else 163_000_000
dev = torch.device("cuda:0")


def timed(fn, reps, warm=2):
    ts = []
    for it in range(reps + warm):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record(); e1.synchronize()
        if it >= warm:
            ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


out = {"n": n}
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream
with pkg.Context(0) as ctx:
    spec = specs.synth_ca13(points_per_file=n)[5]
    raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
    ctx.synth_fill(spec, 0, n, raw.data_ptr(), None, stream)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    cls = (idx % 7).to(torch.uint8)
    gps = idx.to(torch.float64) * 0.001
    del idx
    torch.cuda.synchronize()
    sc = dict(scale=list(spec.scale), offset=list(spec.offset))
    ccols = binding.make_columns(xyz=raw.data_ptr(), cls=cls.data_ptr(), n=n, **sc)
    tcols = binding.make_columns(xyz=raw.data_ptr(), cls=gps.data_ptr(), n=n, cls_stride=8, **sc)
    lo = [spec.lo[a] for a in range(3)]
    hi = [spec.lo[0] + spec.span[0] // 2] + [spec.lo[a] + spec.span[a] for a in (1, 2)]
    span = n * 0.001
    preds = {"bounds": (ccols, pkg.Predicate.bounds(lo, hi), 12),
             "bounds_class": (ccols, pkg.Predicate.bounds_class(lo, hi, 3), 13),
             "bounds_time": (tcols, pkg.Predicate.bounds_time(lo, hi, 0.25 * span, 0.75 * span), 20)}
    for name, (cols, pred, bpp) in preds.items():
        cc = ctx.count_collector()
        med, best = timed(lambda: ctx.scan_dev(cols, pred, cc, stream), 20)
        out[f"{name}_count_ms"] = med
        out[f"{name}_count_best_ms"] = best
        out[f"{name}_count_TBps_{bpp}B_per_point"] = n * bpp / (med * 1e-3) / 1e12
        out[f"{name}_count_fraction_of_8TBps"] = out[f"{name}_count_TBps_{bpp}B_per_point"] / 8.0
        cc.free()
    recs = {"bounds": (ccols, pkg.Predicate.bounds(lo, hi)),
            "bounds_class": (ccols, pkg.Predicate.bounds_class(lo, hi, 3)),
            "bounds_time": (tcols, pkg.Predicate.bounds_time(lo, hi, 0.37 * span, 0.47 * span))}
    hdr_min = [spec.lo[a] * spec.scale[a] + spec.offset[a] for a in range(3)]
    hdr_max = [(spec.lo[a] + spec.span[a]) * spec.scale[a] + spec.offset[a] for a in range(3)]
    for name, (cols, pred) in recs.items():
        gb = ctx.buffer_collector()
        def rec():
            gb.reset()
            ctx.scan_dev(cols, pred, gb, stream)
        med, best = timed(rec, 6)
        out[f"{name}_records_ms"] = med
        out[f"{name}_records_points"] = gb.point_count()
        gb.free()
        gg = ctx.grid_collector(hdr_min, hdr_max, 100.0)
        def dens():
            gg.reset()
            ctx.scan_dev(cols, pred, gg, stream)
            gg.point_count()  # the fold: the grid's result
        med, best = timed(dens, 4)
        out[f"{name}_density_100m_ms"] = med
        out[f"{name}_density_cells"] = gg.point_count()
        gg.free()
print(json.dumps(out))

if CLI:
    q = os.path.join(ROOT, "adhoc-queries-pointclouds_amd", "host", "query")
    env = dict(os.environ, PCQ_TIMING="1")
    box = sys.argv[sys.argv.index("--box") + 1] if "--box" in sys.argv else "-1e12;-1e12;-1e12;1e12;1e12;1e12"
    sidecar = os.path.join(CLI, "..", "combined_rate_stats.json")
    for label, extra in (("bounds", []), ("bounds_class", ["--combine", "--class", "2"]), ("bounds_time", ["--combine", "--time", "-1e300;1e300"])):
        per_file = []
        for rep in range(5):
            r = subprocess.run([q, "-i", CLI, "--bounds", box, "--optimized", "--stats-json", sidecar] + extra, capture_output=True, text=True,
                               env=env, timeout=600)
            print(f"--- cli {label} run {rep} rc={r.returncode}")
            print(r.stdout.strip())
            print("\n".join(l for l in r.stderr.splitlines() if "[pcq]" in l))
            per_file.append(json.load(open(sidecar))["per_file"][0]["search_ms"])
        print(json.dumps({"cli": label, "per_file_search_ms": per_file, "median_ms": sorted(per_file)[len(per_file) // 2]}))
