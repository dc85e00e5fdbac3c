"""Developer tool: the pipelined batched scans of TWO builds of libpcq.so against each other — another build (the parent commit's, as
a rule) and this tree's — for a change that is meant to leave their speed as it is.  Both libraries are loaded into ONE process (two
contexts) and alternated launch by launch: other, this, other, this, ...; device events around each call; ROUNDS timed rounds after 3
warm-up rounds.  The corpus is the rate tools': FILES resident synth_ca13 files x N points (generator order g; for the rasters
scan-strip order s as well; classes of synth-doc; f64 times in acquisition order), the ca13_XL box with z unbounded, so that every
point passes.  The rasters at 8 x 8 cells and at each entry's *_CELLS_MAX; the calls are those of tools/resident_*_rate.py.  Per
configuration one JSON line with both series, the medians, the other build's spread (max - min over its rounds), whether this tree's
median is at most the other's median + that spread ("inside") and whether both builds wrote the same words.  The last line lists
what is not inside.  profiles/raster_frame_rate.log is a table made of such lines.
usage: resident_ab_rate.py OTHER_LIBPCQ_SO [N [FILES [ROUNDS [ONLY,ONLY...]]]]   (ONLY: substrings of "kernel config" to keep)"""
import importlib, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")
specs = importlib.import_module("adhoc-queries-pointclouds_amd.synth_specs")

n = int(sys.argv[2]) if len(sys.argv) > 2 else 163_000_000
files = int(sys.argv[3]) if len(sys.argv) > 3 else 16
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 9
WARM = 3
PARENT = os.path.abspath(sys.argv[1])
dev = torch.device("cuda:0")
ts = torch.cuda.Stream(); torch.cuda.set_stream(ts); stream = ts.cuda_stream
I32_MIN, I32_MAX = -2**31, 2**31 - 1
BUT_7_18 = tuple(c for c in range(256) if c not in (7, 18))


def doc_classes(spec, points):
    doc = specs.synth_doc(points_per_file=points, files=1)[0]
    spec.n_classes = doc.n_classes
    for j in range(8):
        spec.cls_val[j], spec.cls_cum16[j] = doc.cls_val[j], doc.cls_cum16[j]
    return spec


this = binding.Context(0)
saved, path_fn = binding._lib, binding.lib_path
binding._lib, binding.lib_path = None, (lambda: PARENT)
parent = binding.Context(0)
binding._lib, binding.lib_path = saved, path_fn
assert parent.lib is not this.lib and parent.lib._name == PARENT, (parent.lib._name, this.lib._name)
CTX = {"parent": parent, "this": this}
ONLY = list(filter(None, (sys.argv[5] if len(sys.argv) > 5 else "").split(",")))
print("builds:", list(CTX), "only:", ONLY, flush=True)

tiles = [doc_classes(s, n) for s in specs.synth_ca13(points_per_file=n, files=files)]
bmin, bmax = specs.box("ca13_XL")
keep = []
cols = {"g": [], "s": [], "t": []}  # g, s: positions + class bytes; t: generator order + f64 times
for f, spec in enumerate(tiles):
    raw = torch.empty(n * 3, dtype=torch.int32, device=dev)
    cb = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    this.synth_fill(spec, 0, n, raw.data_ptr(), cb.data_ptr() + 3, stream)
    torch.cuda.synchronize()
    t = raw.view(n, 3)
    width, zwidth = int(10.0 / spec.scale[1]), int(10.0 / spec.scale[2])
    key = ((t[:, 1].long() // width) * 4096 + (t[:, 2].long() // zwidth + 2048)) * (1 << 32) + (t[:, 0].long() + (1 << 31))
    order = torch.argsort(key)
    del key
    strips = t[order].contiguous().view(-1)
    scb = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    scb[3:3 + n] = cb[3:3 + n][order]
    del order
    ta = torch.arange(f * n, (f + 1) * n, dtype=torch.float64, device=dev)
    keep += [raw, cb, strips, scb, ta]
    mk = lambda pos, cl, stride=1: binding.make_columns(xyz=pos.data_ptr(), cls=cl, n=n, cls_stride=stride, scale=list(spec.scale),
                                                        offset=list(spec.offset))
    cols["g"].append(mk(raw, cb.data_ptr() + 3))
    cols["s"].append(mk(strips, scb.data_ptr() + 3))
    cols["t"].append(mk(raw, ta.data_ptr(), 8))
torch.cuda.synchronize()
print("corpus: %d files x %d points, %.1f GB of positions per order" % (files, n, files * n * 12 / 1e9), flush=True)
lmin, lmax = pkg.box_to_local(bmin, bmax, list(tiles[0].scale), list(tiles[0].offset))
assert all(pkg.box_to_local(bmin, bmax, list(s.scale), list(s.offset)) == (lmin, lmax) for s in tiles)
points = files * n

W = 8192
i64 = [torch.zeros(4 * W, dtype=torch.int64, device=dev) for _ in range(2)]   # [0]: the run's words, [1]: the parent's, kept
i32 = [torch.zeros(2 * W, dtype=torch.int32, device=dev) for _ in range(2)]


def raster_args(nx, ny):
    cw = [-(-(lmax[a] - lmin[a] + 1) // d) for a, d in ((0, nx), (1, ny))]
    lo, hi = [lmin[0], lmin[1], -2**40], [lmin[0] + nx * cw[0] - 1, lmin[1] + ny * cw[1] - 1, 2**40]
    return [pkg.Predicate.bounds(lo, hi)] * files, [cw] * files


FULL = ([-2**40] * 3, [2**40] * 3)
results, failed = [], []


def ab(name, config, call, words):
    """call(ctx) presets the words and enqueues the entry on ctx; words(): the result as one tensor (compared between the builds)"""
    if ONLY and not any(o in name + " " + config for o in ONLY):
        return
    times = {k: [] for k in CTX}
    got = {}
    for it in range(ROUNDS + WARM):
        for who in CTX:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(CTX[who])
            e1.record(); e1.synchronize()
            if it >= WARM:
                times[who].append(e0.elapsed_time(e1))
            if it == 0:
                got[who] = words().clone()
    same = bool(torch.equal(got["parent"], got["this"]))
    p, t = sorted(times["parent"]), sorted(times["this"])
    pm, tm, spread = p[len(p) // 2], t[len(t) // 2], p[-1] - p[0]
    ok = tm <= pm + spread
    line = {"kernel": name, "config": config, "parent_ms": [round(x, 4) for x in times["parent"]], "this_ms": [round(x, 4) for x in times["this"]],
            "parent_median": round(pm, 4), "this_median": round(tm, 4), "parent_spread": round(spread, 4),
            "this_minus_parent_pct": round(100 * (tm - pm) / pm, 3), "inside": ok, "same_words": same, "sum": int(got["this"].long().sum())}
    results.append(line)
    if not ok or not same:
        failed.append((name, config))
    print(json.dumps(line), flush=True)


def rasters(name, sizes, orders, fn):
    for nx, ny in sizes:
        preds, cells = raster_args(nx, ny)
        for o in orders:
            call, words = fn(cols[o], preds, cells, nx, ny)
            ab(name, "%dx%d_%s" % (nx, ny, o), call, words)


def f_raster(c, preds, cells, nx, ny):
    def call(ctx):
        i64[0].zero_()
        ctx.scan_dev_raster_batch(c, preds, cells, nx, ny, i64[0].data_ptr(), stream)
    return call, lambda: i64[0][:nx * ny]


def f_zrange(c, preds, cells, nx, ny):
    def call(ctx):
        i32[0].fill_(I32_MAX); i32[1].fill_(I32_MIN)
        ctx.scan_dev_zrange_raster_batch(c, preds, cells, nx, ny, i32[0].data_ptr(), i32[1].data_ptr(), stream)
    return call, lambda: torch.cat([i32[0][:nx * ny], i32[1][:nx * ny]])


def f_zsum(c, preds, cells, nx, ny):
    def call(ctx):
        i64[0].zero_()
        ctx.scan_dev_zsum_raster_batch(c, preds, cells, nx, ny, i64[0].data_ptr(), i64[0].data_ptr() + 8 * W, stream)
    return call, lambda: torch.cat([i64[0][:nx * ny], i64[0][W:W + nx * ny]])


def f_zmoments(c, preds, cells, nx, ny):
    def call(ctx):
        i64[0].zero_()
        ctx.scan_dev_zmoments_raster_batch(c, preds, cells, nx, ny, *[i64[0].data_ptr() + 8 * W * k for k in range(4)], stream)
    return call, lambda: torch.cat([i64[0][W * k:W * k + nx * ny] for k in range(4)])


def f_zsum_classes(c, preds, cells, nx, ny):
    def call(ctx):
        i64[0].zero_()
        ctx.scan_dev_zsum_raster_batch_classes(c, preds, cells, nx, ny, (2,), i64[0].data_ptr(), i64[0].data_ptr() + 8 * W, stream)
    return call, lambda: torch.cat([i64[0][:nx * ny], i64[0][W:W + nx * ny]])


def f_zrange_classes(c, preds, cells, nx, ny):
    def call(ctx):
        i32[0].fill_(I32_MAX); i32[1].fill_(I32_MIN)
        ctx.scan_dev_zrange_raster_batch_classes(c, preds, cells, nx, ny, (2,), BUT_7_18, i32[0].data_ptr(), i32[1].data_ptr(), stream)
    return call, lambda: torch.cat([i32[0][:nx * ny], i32[1][:nx * ny]])


rasters("k_bounds_raster_pipe", ((8, 8), (128, 64)), "gs", f_raster)
rasters("k_bounds_zrange_pipe", ((8, 8), (64, 64)), "gs", f_zrange)
rasters("k_bounds_zsum_pipe", ((8, 8), (64, 32)), "gs", f_zsum)
rasters("k_bounds_zmoments_pipe", ((8, 8), (32, 32)), "gs", f_zmoments)
rasters("k_bounds_zsum_classes_pipe", ((8, 8), (64, 32)), "gs", f_zsum_classes)
rasters("k_bounds_zrange_classes_pipe", ((8, 8), (64, 64)), "gs", f_zrange_classes)

boxes = [pkg.Predicate.bounds(*FULL)] * files


def call_class_hist(ctx):
    i64[0].zero_()
    ctx.scan_dev_class_hist_batch(cols["g"], boxes, i64[0].data_ptr(), stream)


ab("k_bounds_class_hist_pipe", "all_points", call_class_hist, lambda: i64[0][:256])

for nbins in (8, 1024):
    edges = np.linspace(0.0, float(files) * n, nbins + 1)

    def call_time_hist(ctx, edges=edges):
        i64[0].zero_()
        ctx.scan_dev_time_hist_batch(cols["t"], boxes, edges, i64[0].data_ptr(), stream)

    ab("k_bounds_time_hist_pipe", "%d_bins_ordered" % nbins, call_time_hist, lambda nbins=nbins: i64[0][:nbins])

cx, cy = (lmin[0] + lmax[0]) // 2, (lmin[1] + lmax[1]) // 2
rx, ry = (lmax[0] - lmin[0]) // 2, (lmax[1] - lmin[1]) // 2
for m in (4, 64):
    verts = [(cx + int(rx * math.cos(0.1 + 2 * math.pi * i / m)), cy + int(ry * math.sin(0.1 + 2 * math.pi * i / m))) for i in range(m)]
    xs, ys = [v[0] for v in verts], [v[1] for v in verts]
    pp = [pkg.Predicate.bounds([min(xs), min(ys), -2**40], [max(xs), max(ys), 2**40])] * files

    def call_polygon(ctx, verts=verts, pp=pp):
        i64[0].zero_()
        ctx.scan_dev_count_batch_polygon(cols["g"], pp, [verts] * files, i64[0].data_ptr(), stream)

    ab("k_bounds_polygon_pipe", "regular_%d" % m, call_polygon, lambda: i64[0][:1])


def call_count(ctx):
    i64[0].zero_()
    ctx.scan_dev_count_batch(cols["g"], boxes, i64[0].data_ptr(), stream)


ab("k_bounds_count_batch_pipe<2>", "all_points", call_count, lambda: i64[0][:1])
combined = [pkg.Predicate.bounds_class(*FULL, 2)] * files


def call_combined(ctx):
    i64[0].zero_()
    ctx.scan_dev_count_batch_combined(cols["g"], combined, i64[0].data_ptr(), stream)


ab("k_bounds_count_batch_pipe<2, ClassBytes>", "class_2", call_combined, lambda: i64[0][:1])
timed = [pkg.Predicate.bounds_time(*FULL, 0.0, float(files) * n / 2)] * files


def call_bounds_time(ctx):
    i64[0].zero_()
    ctx.scan_dev_count_batch_bounds_time(cols["t"], timed, i64[0].data_ptr(), stream)


ab("k_bounds_count_batch_pipe<2, GpsTimes>", "first_half", call_bounds_time, lambda: i64[0][:1])

print("NOT INSIDE, OR OTHER WORDS:", failed if failed else "none", flush=True)
for c_ in CTX.values():
    c_.close()
