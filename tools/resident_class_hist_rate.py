"""Developer tool: the class histogram of a box on resident data — one pass that bins the class byte of every point inside the
box, against the only other way to the same answer: one box AND class pass per class present.

FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13) with class bytes drawn
(a) from the synth-doc pmf (synth_specs.synth_doc: six classes, 45 % of the points in class 2), and
(b) uniformly over 32 values,
and the ca13_XL box.  Per distribution three routes, each timed with device events around the whole of it, alternated, REPS rounds
after 3 warm-up rounds; median, minimum and maximum, TB/s on 13 B/point:
  hist        ONE pcq_scan_dev_class_hist_batch;
  combined    ONE pcq_scan_dev_count_batch_combined (class 2): the floor — the same bytes, one compare instead of a bin;
  per_class   one pcq_scan_dev_count_batch_combined per class present (6 or 32 launches): what a caller did before.
The histogram is compared with the per-class counts.  break_even_classes = hist / combined: from how many classes on the one
pass pays.  Rule: hist's slowest round is below per_class's fastest round on (a).
(c) with PCQ_LAB=1 (libpcq_lab.so accepts the options "class_hist_waves_per_cu" and "class_hist_copies"): the one pass on (a) and
    (b) at 3 .. 16 workgroups per CU (3, 4, 5, 6, 8, 12, 16) and 1 / 4 / 8 / 16 copies of the LDS histogram per wave.
The last line restates the checks.
usage: resident_class_hist_rate.py [N [FILES [REPS]]]"""
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
lab = os.environ.get("PCQ_LAB") == "1"


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
    return passes * files * n * 13 / (ms * 1e-3) / 1e12


checks = {}
with pkg.Context(0) as ctx:
    tiles = specs.synth_ca13(points_per_file=n, files=files)
    doc = specs.synth_doc(points_per_file=n, files=1)[0]
    bmin, bmax = specs.box("ca13_XL")
    keep, cols = [], {"a": [], "b": []}
    gen = torch.Generator(device=dev); gen.manual_seed(32)
    for spec in tiles:
        spec.n_classes = doc.n_classes  # the positions of ca13, the classes of synth-doc
        for j in range(8):
            spec.cls_val[j], spec.cls_cum16[j] = doc.cls_val[j], doc.cls_cum16[j]
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        ca = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), ca.data_ptr(), stream)
        cb = torch.randint(0, 32, (n + 16,), dtype=torch.uint8, device=dev, generator=gen)
        keep += [raw, ca, cb]
        for name, c in (("a", ca), ("b", cb)):
            cols[name].append(binding.make_columns(xyz=raw.data_ptr(), cls=c.data_ptr(), n=n, scale=list(spec.scale), offset=list(spec.offset)))
    torch.cuda.synchronize()
    local = [pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) for s in tiles]
    boxes = [pkg.Predicate.bounds(*b) for b in local]
    hist = torch.zeros(256, dtype=torch.int64, device=dev)
    counter = torch.zeros(256, dtype=torch.int64, device=dev)

    for name, what in (("a", "synth-doc pmf, 6 classes"), ("b", "uniform over 32 classes")):
        c = cols[name]

        def one_hist():
            hist.zero_()
            ctx.scan_dev_class_hist_batch(c, boxes, hist.data_ptr(), stream)

        one_hist()
        torch.cuda.synchronize()
        h = hist.tolist()
        present = [k for k in range(256) if h[k]]
        by_class = {k: [pkg.Predicate.bounds_class(*b, k) for b in local] for k in present}

        def combined():
            counter.zero_()
            ctx.scan_dev_count_batch_combined(c, by_class[2], counter.data_ptr(), stream)

        def per_class():
            counter.zero_()
            for k in present:
                ctx.scan_dev_count_batch_combined(c, by_class[k], counter.data_ptr() + 8 * k, stream)

        per_class()
        torch.cuda.synchronize()
        assert counter.tolist() == h and len(present) == (6 if name == "a" else 32), (present, h, counter.tolist())
        res = alternate({"hist": one_hist, "combined": combined, "per_class": per_class}, reps)
        res["hist"]["TBps_13B_per_point"] = tbps(1, res["hist"]["median_ms"])
        res["combined"]["TBps_13B_per_point"] = tbps(1, res["combined"]["median_ms"])
        res["per_class"]["TBps_13B_per_point"] = tbps(len(present), res["per_class"]["median_ms"])
        speedup = res["per_class"]["median_ms"] / res["hist"]["median_ms"]
        checks[f"{name}_hist_faster_than_per_class_beyond_spread"] = res["hist"]["max_ms"] < res["per_class"]["min_ms"]
        checks[f"{name}_speedup"] = speedup
        checks[f"{name}_break_even_classes"] = res["hist"]["median_ms"] / res["combined"]["median_ms"]
        print(f"({name})", json.dumps({"classes": what, "files": files, "points_per_file": n, "present": len(present), "in_box": sum(h),
                                       "largest_bin_share": max(h) / max(1, sum(h)), "speedup": speedup,
                                       "break_even_classes": checks[f"{name}_break_even_classes"], **res}), flush=True)
    if lab:  # ---- (c) the one pass at other grids and with other numbers of copies ------------------------------------------
        for copies in (1, 4, 8, 16):
            ctx.set_option("class_hist_copies", copies)
            out = {"a": {}, "b": {}}
            for w in (3, 4, 5, 6, 8, 12, 16):
                ctx.set_option("class_hist_waves_per_cu", w)
                r = alternate({k: (lambda k=k: ctx.scan_dev_class_hist_batch(cols[k], boxes, hist.data_ptr(), stream)) for k in ("a", "b")},
                              max(3, reps // 2))
                for k in ("a", "b"):
                    r[k]["TBps_13B_per_point"] = tbps(1, r[k]["median_ms"])
                    out[k][w] = r[k]
            print("(c)", json.dumps({"copies": copies, "by_waves_per_cu": out}), flush=True)
        ctx.set_option("class_hist_copies", 0)
        ctx.set_option("class_hist_waves_per_cu", 0)
    del keep, cols
print("checks", json.dumps(checks), flush=True)
