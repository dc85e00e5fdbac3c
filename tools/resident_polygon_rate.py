"""Developer tool: box AND polygon on resident data — one pass that tests every point inside the box against the edges of an outline,
against the plain box count of the outline's bounding box on the same bytes (the read floor this pass is measured against).

FILES resident synthetic files of N points each (the 4 x 4 tiles of synth_ca13, generator order).  Outlines, all in the files' one
lattice: regular polygons of 4, 16, 64 and 256 vertices on the ellipse inscribed in the ca13_XL box, so most points pass the box and
every one of them meets every edge; and "thin", a diagonal quadrilateral whose bounding box is 1 / 32 of the box on x and on y, so
most tiles hold no point of its box and are skipped.  The z range is the box's.  Per outline the two routes are timed with device
events around the whole of each, alternated in one process, REPS rounds after 2 warm-up rounds; median, minimum and maximum:
  polygon     ONE pcq_scan_dev_count_batch_polygon with the outline's bounding box as the predicate;
  count       ONE pcq_scan_dev_count_batch of that bounding box: the floor — the same bytes, a popcount instead of the edge loop.
Checked: every polygon count is at most its box count, the 4-gon of a rectangle equals the count of the half-open box, and the count
of an outline does not depend on the grid.
With PCQ_LAB=1 (libpcq_lab.so accepts the option "polygon_waves_per_cu") also the one pass at 2 .. 16 workgroups per CU.
The last line restates the checks.
usage: resident_polygon_rate.py [N [FILES [REPS]]]"""
import importlib, json, math, os, sys
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
WAVES = (2, 3, 4, 5, 6, 8, 12, 16)


def spread(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "reps": len(v)}


def alternate(fns, reps, warm=2):
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


checks = {}
with pkg.Context(0) as ctx:
    tiles = specs.synth_ca13(points_per_file=n, files=files)
    bmin, bmax = specs.box("ca13_XL")
    keep, cols = [], []
    for spec in tiles:
        raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
        cls = torch.empty(n + 16, dtype=torch.uint8, device=dev)
        ctx.synth_fill(spec, 0, n, raw.data_ptr(), cls.data_ptr(), stream)
        torch.cuda.synchronize()
        del cls
        keep.append(raw)
        assert raw.data_ptr() % 16 == 0
        cols.append(binding.make_columns(xyz=raw.data_ptr(), n=n, scale=list(spec.scale), offset=list(spec.offset)))
    # every tile has the scale and offset of the first: one local box, one lattice, one outline
    lmin, lmax = pkg.box_to_local(bmin, bmax, list(tiles[0].scale), list(tiles[0].offset))
    assert all(pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) == (lmin, lmax) for s in tiles)
    total = torch.zeros(8, dtype=torch.int64, device=dev)
    points = files * n
    cx, cy = (lmin[0] + lmax[0]) // 2, (lmin[1] + lmax[1]) // 2
    rx, ry = (lmax[0] - lmin[0]) // 2, (lmax[1] - lmin[1]) // 2
    outlines = {f"regular_{m}": [(cx + int(rx * math.cos(0.1 + 2 * math.pi * i / m)), cy + int(ry * math.sin(0.1 + 2 * math.pi * i / m))) for i in range(m)]
                for m in (4, 16, 64, 256)}
    w, h = (lmax[0] - lmin[0]) // 32, (lmax[1] - lmin[1]) // 32
    outlines["thin"] = [(cx, cy), (cx + w // 8, cy), (cx + w, cy + h), (cx + w - w // 8, cy + h)]
    rect = [(cx - rx // 2, cy - ry // 2), (cx + rx // 2, cy - ry // 2), (cx + rx // 2, cy + ry // 2), (cx - rx // 2, cy + ry // 2)]

    def polygon_count(verts, lo, hi):
        total.zero_()
        ctx.scan_dev_count_batch_polygon(cols, [pkg.Predicate.bounds(lo, hi)] * files, [verts] * files, total.data_ptr(), stream)

    def box_count(lo, hi):
        total.zero_()
        ctx.scan_dev_count_batch(cols, [pkg.Predicate.bounds(lo, hi)] * files, total.data_ptr(), stream)

    def bbox(verts):
        xs, ys = [v[0] for v in verts], [v[1] for v in verts]
        return [min(xs), min(ys), lmin[2]], [max(xs), max(ys), lmax[2]]

    lo, hi = bbox(rect)
    polygon_count(rect, lo, hi); torch.cuda.synchronize(); got = int(total[0])
    box_count(lo, [hi[0] - 1, hi[1] - 1, hi[2]]); torch.cuda.synchronize()
    checks["rectangle_is_the_half_open_box"] = got == int(total[0]) and got > 0

    for name, verts in outlines.items():
        lo, hi = bbox(verts)
        polygon = lambda: polygon_count(verts, lo, hi)
        count = lambda: box_count(lo, hi)
        polygon(); torch.cuda.synchronize(); inside = int(total[0])
        count(); torch.cuda.synchronize(); in_box = int(total[0])
        checks[f"{name}_at_most_its_box"] = 0 < inside <= in_box
        r = reps if len(verts) <= 64 else max(3, reps // 2)
        res = alternate({"polygon": polygon, "count": count}, r)
        line = {"outline": name, "vertices": len(verts), "files": files, "points_per_file": n, "inside": inside, "in_box": in_box,
                "polygon_over_count": res["polygon"]["median_ms"] / res["count"]["median_ms"],
                "count_TBps_12B_per_point": points * 12 / (res["count"]["median_ms"] * 1e-3) / 1e12,
                "ns_per_point_and_edge_in_box": res["polygon"]["median_ms"] * 1e6 / (max(in_box, 1) * len(verts))}
        print("(rate)", json.dumps({**line, **res}), flush=True)
        if lab:  # ---- the one pass at other grids ------------------------------------------------------------------------------
            sweep = {}
            for wv in WAVES:
                ctx.set_option("polygon_waves_per_cu", wv)
                s = alternate({"polygon": polygon}, max(3, r // 2), warm=1)["polygon"]
                torch.cuda.synchronize()
                checks[f"{name}_w{wv}_same_count"] = int(total[0]) == inside
                sweep[f"w{wv}"] = [round(s["median_ms"], 3), round(s["min_ms"], 3), round(s["max_ms"], 3)]
            ctx.set_option("polygon_waves_per_cu", 0)
            print("(sweep)", json.dumps({"outline": name, "vertices": len(verts), "median_min_max_ms": sweep}), flush=True)
    del keep, cols
print("checks", json.dumps(checks), flush=True)
print("all checks hold" if all(checks.values()) else "A CHECK FAILED", flush=True)
