"""Developer tool: rates of the GPS time-range search (PCQ_PRED_TIME).

Over one resident format-3 LAST time block of n points (default 163 M) with gps = i * 0.001 and the synthetic positions of
tools/index_rate.py:
  * count: K3 over the packed f64 column, timed with device events after warm-up, reported against 8 B/point (algorithmic);
  * records: buffer collector at about 1 % and 10 % of the points kept (one contiguous time window each);
  * density: grid collector with 100 m cells over the file's box, 10 % kept.
--cli DIR: the `query --time` path per file with PCQ_TIMING=1 (the first run warms the page cache).
Nothing here builds or consults a chunk index."""
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
    gps = torch.arange(n, dtype=torch.float64, device=dev) * 0.001
    torch.cuda.synchronize()
    cols = binding.make_columns(xyz=raw.data_ptr(), cls=gps.data_ptr(), n=n, cls_stride=8, scale=list(spec.scale), offset=list(spec.offset))
    span = n * 0.001
    cc = ctx.count_collector()
    pred = pkg.Predicate.time_range(0.25 * span, 0.75 * span)
    med, best = timed(lambda: ctx.scan_dev(cols, pred, cc, stream), 20)
    out["count_ms"] = med
    out["count_best_ms"] = best
    out["count_TBps_8B_per_point"] = n * 8 / (med * 1e-3) / 1e12
    out["count_fraction_of_8TBps"] = out["count_TBps_8B_per_point"] / 8.0
    for frac in (0.01, 0.10):
        p = pkg.Predicate.time_range(0.37 * span, (0.37 + frac) * span)
        gb = ctx.buffer_collector()
        def rec():
            gb.reset()
            ctx.scan_dev(cols, p, gb, stream)
        med, best = timed(rec, 10)
        out[f"records_{int(frac * 100)}pct_ms"] = med
        out[f"records_{int(frac * 100)}pct_points"] = gb.point_count()
        gb.free()
    hdr_min = [spec.lo[a] * spec.scale[a] + spec.offset[a] for a in range(3)]
    hdr_max = [(spec.lo[a] + spec.span[a]) * spec.scale[a] + spec.offset[a] for a in range(3)]
    p = pkg.Predicate.time_range(0.37 * span, 0.47 * span)
    gg = ctx.grid_collector(hdr_min, hdr_max, 100.0)
    def dens():
        gg.reset()
        ctx.scan_dev(cols, p, gg, stream)
        gg.point_count()  # the fold: the grid's result
    med, best = timed(dens, 6)
    out["density_100m_10pct_ms"] = med
    out["density_cells"] = gg.point_count()
    gg.free()
print(json.dumps(out))

if CLI:
    q = os.path.join(ROOT, "adhoc-queries-pointclouds_amd", "host", "query")
    env = dict(os.environ, PCQ_TIMING="1")
    for rep in range(3):
        r = subprocess.run([q, "-i", CLI, "--time", "1000;2000", "--optimized"], capture_output=True, text=True, env=env, timeout=600)
        print(f"--- cli run {rep} rc={r.returncode}")
        print(r.stdout.strip())
        print("\n".join(l for l in r.stderr.splitlines() if "[pcq]" in l))
