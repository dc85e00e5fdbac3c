"""Developer tool: box AND class (PCQ_PRED_BOUNDS_CLASS) on resident data — what the batched launch and the chunk index buy.

(a) FILES resident synthetic files of N points each (positions of synth_ca13, class = i mod 7, class blocks at byte offset
    f mod 4): pcq_scan_dev_count_batch_combined over all of them against the only way to get that answer without it, a loop
    of pcq_scan_dev with PCQ_PRED_BOUNDS_CLASS per file into one device counter; both timed with device events around the
    whole query, alternated, after warm-up; per point and against the 8 TB/s peak on 13 B/point.
(b) one file of N points in the generator's random order and in a coherent order (x slabs, y inside a slab, the order of
    tools/index_rate.py): count and records through pcq_scan_dev_indexed_combined against pcq_scan_dev, x slabs keeping
    about 0.1 %, 1 % and 10 % of the chunks, class 3 of 7; counts and records compared, index statistics printed.
usage: resident_combined_rate.py [N [FILES [REPS]]]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 163_000_000
files = int(sys.argv[2]) if len(sys.argv) > 2 else 16
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
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


with pkg.Context(0) as ctx:
    spec = specs.synth_ca13(points_per_file=n)[5]
    sc = dict(scale=list(spec.scale), offset=list(spec.offset))
    lo = [spec.lo[a] for a in range(3)]
    hi = [spec.lo[0] + spec.span[0] // 2] + [spec.lo[a] + spec.span[a] for a in (1, 2)]
    idx = torch.arange(n + 16, dtype=torch.int64, device=dev)
    cls7 = (idx % 7).to(torch.uint8)
    del idx

    # ---- (a) batched against the per-file loop --------------------------------------------------------------------
    keep, cols = [], []
    for f in range(files):
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), None, stream)
        c = cls7.clone()
        keep += [raw, c]
        cols.append(binding.make_columns(xyz=raw.data_ptr(), cls=c.data_ptr() + f % 4, n=n, **sc))
    torch.cuda.synchronize()
    preds = [pkg.Predicate.bounds_class(lo, hi, 3)] * files
    counter = torch.zeros(2, dtype=torch.int64, device=dev)
    cc = ctx.count_collector(device_counter=counter.data_ptr())
    got = {}

    def batched():
        counter.zero_()
        ctx.scan_dev_count_batch_combined(cols, preds, counter.data_ptr(), stream)

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
        v["TBps_13B_per_point"] = files * n * 13 / (v["median_ms"] * 1e-3) / 1e12
        v["fraction_of_8TBps"] = v["TBps_13B_per_point"] / 8.0
    print("(a)", json.dumps({"files": files, "points_per_file": n, "matches": got["batched"], **res}), flush=True)
    cc.free()
    raw0 = keep[0]
    del keep, cols
    torch.cuda.empty_cache()

    # ---- (b) through the chunk index against the plain scan -------------------------------------------------------
    pts = raw0.view(n, 3)
    cls = cls7[:n].contiguous()
    key = ((pts[:, 0].long() - int(spec.lo[0])) * 2048 // int(spec.span[0])) * (1 << 32) + (pts[:, 1].long() - int(spec.lo[1]))
    order = torch.argsort(key)
    coh, coh_cls = pts[order].contiguous(), cls[order].contiguous()
    del key, order
    torch.cuda.synchronize()
    for label, t, c in (("random_order", pts, cls), ("coherent_order", coh, coh_cls)):
        cols1 = binding.make_columns(xyz=t.data_ptr(), cls=c.data_ptr(), n=n, **sc)
        ix = ctx.index_new()
        for frac in (0.001, 0.01, 0.1):
            x0 = int(spec.lo[0] + spec.span[0] * 0.37)
            pred = pkg.Predicate.bounds_class([x0, -2 ** 31, -2 ** 31], [x0 + int(spec.span[0] * frac), 2 ** 31 - 1, 2 ** 31 - 1], 3)
            out = {}
            for kind in ("count", "records"):
                mk = ctx.count_collector if kind == "count" else ctx.buffer_collector
                g = {False: mk(), True: mk()}

                def run(indexed):
                    g[indexed].reset()
                    if indexed: ctx.scan_dev_indexed_combined(cols1, pred, ix, g[indexed], stream)
                    else: ctx.scan_dev(cols1, pred, g[indexed], stream)

                r = alternate({"plain": lambda: run(False), "indexed": lambda: run(True)}, max(6, reps // 2))
                assert g[False].point_count() == g[True].point_count(), (label, frac, kind)
                if kind == "records":
                    assert g[False].points().tobytes() == g[True].points().tobytes(), (label, frac)
                st = ctx.index_stats(ix)
                out[kind] = {"matches": g[True].point_count(), "plain": r["plain"], "indexed": r["indexed"],
                             "speedup": r["plain"]["median_ms"] / r["indexed"]["median_ms"],
                             "chunks": st["chunks"], "skipped": st["skipped"], "whole": st["whole"], "scanned": st["scanned"]}
                for x in g.values(): x.free()
            print("(b)", label, f"x{frac}", json.dumps(out), flush=True)
        ctx.index_free(ix)
