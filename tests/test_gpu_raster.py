"""pcq_scan_dev_raster_batch: the density raster of a box over many resident segments in one pass, every cell against numpy.

Segments of n = 0, 1, 511, 512, 513, 1535, 4133 points, the sizes of test_gpu_class_hist.py (a step of the pipeline is 512 points),
positions pieces 16-byte aligned in one buffer.  Every segment has its own origin, its own box and its own cell widths; x and y
are drawn independently, so a y taken from the wrong lane or load lands in another cell.  Every case uploads the positions it
needs.  The counts are ADDED: every call starts from distinct non-zero device words, PCQ_RASTER_CELLS_MAX of them and 64 more,
and the test looks at the difference: numpy's np.add.at on ((y - lo_y) // cw_y, (x - lo_x) // cw_x) of the points inside the box
for the raster's words, nothing for the words behind them.
"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _pipeline_plan as pp  # noqa: E402

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("adhoc-queries-pointclouds_amd")
binding = importlib.import_module("adhoc-queries-pointclouds_amd.binding")

NS = (0, 1, 511, 512, 513, 1535, 4133)
PCQ_ERR_ARG = pkg.PCQ_ERR_ARG
I32_MIN, I32_MAX = -2**31, 2**31 - 1
CELLS_MAX = 8192
WORDS = CELLS_MAX + 64
PRESET = np.asarray([1000 + 7 * c for c in range(WORDS)], dtype=np.uint64)
EMPTY = ([5, 5, 5], [4, 4, 4])


def origin(k):
    return 1000 * k - 300, 77 - 500 * k


def box_of(k, nx, ny, cw):
    """Segment k's box: nx x ny full cells from its origin, and a slab of z"""
    ox, oy = origin(k)
    return [ox, oy, 2 * k], [ox + nx * cw[0] - 1, oy + ny * cw[1] - 1, 99 - k]


def draw(rng, nx, ny, cws, margin=2):
    """Positions of every segment: x and y independent over the segment's raster and `margin` lattice steps around it, z in 0..99"""
    out = []
    for k, n in enumerate(NS):
        ox, oy = origin(k)
        out.append(np.stack([ox + rng.integers(-margin, nx * cws[k][0] + margin, n), oy + rng.integers(-margin, ny * cws[k][1] + margin, n),
                             rng.integers(0, 100, n)], axis=1).astype(np.int32))
    return out


class Dev:
    def __init__(self, ctx):
        self.ctx = ctx
        self.poff, self.psize = pp.carve(NS, [0] * len(NS), 12)
        self.blocks = [ctx.alloc(self.psize + 64), ctx.alloc(8 * WORDS)]
        self.d_pos, self.d_ras = self.blocks
        assert all(p % 16 == 0 for p in self.blocks) and all(o % 16 == 0 for o in self.poff)
        self.cols = [binding.make_columns(xyz=self.d_pos + p, n=n) for p, n in zip(self.poff, NS)]
        self.xyz = None

    def upload(self, xyz):
        assert [len(a) for a in xyz] == list(NS)
        img = np.zeros(self.psize, dtype=np.uint8)
        for o, a in zip(self.poff, xyz):
            img[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.ctx.to_device(self.d_pos, img)
        self.xyz = xyz

    def want(self, boxes, cws, nx, ny, segments=None):
        w = np.zeros((ny, nx), dtype=np.int64)
        for k, (lo, hi), cw in zip(range(len(NS)) if segments is None else segments, boxes, cws):
            sel = pp.in_box(self.xyz[k], lo, hi)
            p = self.xyz[k][sel].astype(np.int64)
            np.add.at(w, ((p[:, 1] - int(lo[1])) // int(cw[1]), (p[:, 0] - int(lo[0])) // int(cw[0])), 1)
        return w

    def words(self):
        out = np.zeros(WORDS, dtype=np.uint64)
        self.ctx.to_host(out, self.d_ras)  # (waits for the context's stream)
        return out

    def launch(self, boxes, cws, nx, ny, segments=None, cols=None, preds=None, d_raster=None):
        if cols is None:
            cols = self.cols if segments is None else [self.cols[k] for k in segments]
        if preds is None:
            preds = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
        self.ctx.scan_dev_raster_batch(cols, preds, cws, nx, ny, self.d_ras if d_raster is None else d_raster)

    def added(self, boxes, cws, nx, ny, segments=None):
        """One call from the preset words: what it ADDED to the raster's words; the words behind them stay as preset"""
        self.ctx.to_device(self.d_ras, PRESET)
        self.launch(boxes, cws, nx, ny, segments)
        got = self.words().astype(np.int64) - PRESET.astype(np.int64)
        assert not got[nx * ny:].any(), np.flatnonzero(got[nx * ny:])[:8] + nx * ny
        return got[:nx * ny].reshape(ny, nx)

    def check(self, boxes, cws, nx, ny, segments=None):
        got, want = self.added(boxes, cws, nx, ny, segments), self.want(boxes, cws, nx, ny, segments)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in bad[:12]]
        return want

    def free(self):
        for p in self.blocks:
            self.ctx.free(p)


@pytest.fixture(scope="module")
def dev(gpu_ctx):
    d = Dev(gpu_ctx)
    yield d
    d.free()


def test_widths_one_over_the_full_raster(dev):
    """64 x 128 cells of one lattice value each: all PCQ_RASTER_CELLS_MAX cells, x in [0, 64) and y in [0, 128) from the origin"""
    nx, ny = 64, 128
    cws = [(1, 1)] * len(NS)
    dev.upload(draw(np.random.default_rng(31), nx, ny, cws, margin=0))
    boxes = [box_of(k, nx, ny, (1, 1)) for k in range(len(NS))]
    want = dev.check(boxes, cws, nx, ny)
    assert 0 < want.sum() < sum(NS) and (want > 0).sum() > 4000
    # every point, through the z range as well
    full = [([lo[0], lo[1], -2**40], [hi[0], hi[1], 2**40]) for lo, hi in boxes]
    assert dev.check(full, cws, nx, ny).sum() == sum(NS)


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (37, 1), (3, 5)])
def test_small_dimensions(dev, nx, ny):
    cws = [(2 + k, 9 - k) for k in range(len(NS))]
    dev.upload(draw(np.random.default_rng(32 + nx + 100 * ny), nx, ny, cws))
    want = dev.check([box_of(k, nx, ny, cws[k]) for k in range(len(NS))], cws, nx, ny)
    assert 0 < want.sum() < sum(NS) and want.min() > 0


def test_hard_widths(dev):
    """Widths 3, 7 and 641 with points planted at q cw - 1, q cw and q cw + 1 from the origin, on both axes"""
    nx, ny = 12, 9
    hard = (3, 7, 641)
    cws = [(hard[k % 3], hard[(k + 1) % 3]) for k in range(len(NS))]
    rng = np.random.default_rng(33)
    xyz = draw(rng, nx, ny, cws)
    for k, n in enumerate(NS):
        ox, oy = origin(k)
        for a, (o, dim) in enumerate(((ox, nx), (oy, ny))):
            edge = (o + np.repeat(np.arange(dim + 1), 3) * cws[k][a] + np.tile([-1, 0, 1], dim + 1)).astype(np.int32)
            at = rng.permutation(n)[:len(edge)]
            xyz[k][at, a] = edge[:len(at)]
    dev.upload(xyz)
    want = dev.check([box_of(k, nx, ny, cws[k]) for k in range(len(NS))], cws, nx, ny)
    assert 0 < want.sum() < sum(NS) and want.min() > 0


def test_the_whole_i32_range_on_x(dev):
    """A box over the whole i32 range on x, 256 cells of 2^24: INT32_MIN lies in cell 0 and INT32_MAX in cell 255, planted inside a
    whole step and among leftover points"""
    nx, ny, cw = 256, 2, (2**24, 50)
    rng = np.random.default_rng(34)
    xyz = [np.stack([rng.integers(I32_MIN, I32_MAX + 1, n), rng.integers(-3, 103, n), rng.integers(0, 100, n)], axis=1).astype(np.int32)
           for n in NS]
    xyz[6][100, :2] = I32_MIN, 10   # inside a whole step
    xyz[4][512, :2] = I32_MIN, 60   # the one leftover point of a segment of 513
    xyz[6][3000, :2] = I32_MAX, 60  # inside a whole step
    xyz[5][1530, :2] = I32_MAX, 10  # among the 511 leftover points
    dev.upload(xyz)
    boxes = [([I32_MIN, 0, -1], [I32_MAX + (2**35 if k % 2 else 0), 99, 100]) for k in range(len(NS))]  # (lmax may be anywhere)
    want = dev.check(boxes, [cw] * len(NS), nx, ny)
    assert 0 < want.sum() < sum(NS) and want[:, 0].min() > 0 and want[:, 255].min() > 0
    for k, i in ((6, 100), (4, 512), (6, 3000), (5, 1530)):
        one = np.zeros_like(xyz[k])
        one[:, 1] = -50  # outside the box on y
        one[i] = xyz[k][i]
        alone = [a if j == k else np.full_like(a, -50) for j, a in enumerate(xyz)]
        alone[k] = one
        dev.upload(alone)
        w = dev.check(boxes, [cw] * len(NS), nx, ny)
        assert w.sum() == 1 and w[int(xyz[k][i, 1]) // 50, 0 if xyz[k][i, 0] == I32_MIN else 255] == 1
    dev.upload(xyz)


def test_seam_points(dev):
    """Points 84, 85 and 86 of a tile of 256: 84 starts at dword 252 (lane 63 of load 0, j = 0), 85 at dword 255 (its j = 3: x in
    load 0, y in lane 0 of load 1), 86 at dword 258 (lane 0 of load 1, j = 2).  In the first tile, the second tile of the first step
    and both tiles of a later step they carry distinct known cells; every other point lies outside the box."""
    k, nx, ny, cw = 6, 5, 4, (7, 3)
    ox, oy = origin(k)
    xyz = [np.full((n, 3), -10**6, dtype=np.int32) for n in NS]
    where = [base + i for base in (0, 256, 3 * 512, 3 * 512 + 256) for i in (84, 85, 86)]
    for i, p in enumerate(where):
        xyz[k][p] = ox + (i % nx) * cw[0] + 1 + i % 3, oy + (i // nx) * cw[1] + i % 2, 50
    dev.upload(xyz)
    want = dev.check([box_of(k, nx, ny, cw)], [cw], nx, ny, [k])
    assert want.sum() == len(where) == 12 and want.max() == 1
    assert [int(c) for c in np.flatnonzero(want.reshape(-1))] == list(range(12))
    # the same with every segment in the launch
    cws = [cw] * len(NS)
    assert dev.check([box_of(j, nx, ny, cw) for j in range(len(NS))], cws, nx, ny).sum() == 12


def test_empty_and_out_of_range_boxes(dev):
    nx, ny = 6, 7
    n = len(NS)
    cws = [(4 + k, 5) for k in range(n)]
    dev.upload(draw(np.random.default_rng(35), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    all_of = dev.check(boxes, cws, nx, ny).sum()
    odd = [EMPTY if k % 2 else boxes[k] for k in range(n)]
    assert 0 < dev.check(odd, cws, nx, ny).sum() < all_of  # (the odd segments would have matched: they are not evaluated)
    far_z = [([lo[0], lo[1], 2**31], [hi[0], hi[1], 2**40]) for lo, hi in boxes]  # outside the i32 range on z
    assert dev.check([far_z[k] if k == 6 else boxes[k] for k in range(n)], cws, nx, ny).sum() == all_of - dev.want([boxes[6]], [cws[6]], nx, ny, [6]).sum()
    assert not dev.added([EMPTY] * n, cws, nx, ny).any()
    assert not dev.added(far_z, cws, nx, ny).any()
    assert not dev.added([], [], nx, ny, []).any()  # nsegments == 0


def test_a_second_launch_with_other_widths(dev):
    """The same segments and boxes' origins, other widths: the table's compare sees the widths"""
    nx, ny = 8, 8
    n = len(NS)
    a, b = [(6, 6)] * n, [(3, 12)] * n
    dev.upload(draw(np.random.default_rng(36), nx, ny, a))
    boxes = [box_of(k, nx, ny, (3, 6)) for k in range(n)]  # fits both: 8 x 3 and 8 x 6 lattice steps
    wa = dev.check(boxes, a, nx, ny)
    wb = dev.check(boxes, b, nx, ny)
    assert wa.sum() == wb.sum() > 0 and not np.array_equal(wa, wb)
    assert np.array_equal(dev.check(boxes, a, nx, ny), wa)
    # and the plain box count of the same segments in between
    total = np.zeros(1, dtype=np.uint64)
    dev.ctx.memset(dev.d_ras, 0, 8)
    dev.ctx.scan_dev_count_batch(dev.cols, [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes], dev.d_ras)
    dev.ctx.to_host(total, dev.d_ras)
    assert int(total[0]) == wa.sum()
    assert np.array_equal(dev.check(boxes, b, nx, ny), wb)


def test_refusals_leave_the_words_alone(dev):
    nx, ny = 6, 7
    n = len(NS)
    cws = [(4 + k, 5) for k in range(n)]
    dev.upload(draw(np.random.default_rng(37), nx, ny, cws))
    boxes = [box_of(k, nx, ny, cws[k]) for k in range(n)]
    dev.check(boxes, cws, nx, ny)
    good = [pkg.Predicate.bounds(lo, hi) for lo, hi in boxes]
    dev.ctx.to_device(dev.d_ras, PRESET)

    def refused(cols=dev.cols, preds=good, cells=cws, nx=nx, ny=ny, d_raster=None):
        with pytest.raises(binding.PcqError) as e:
            dev.launch(None, cells, nx, ny, cols=cols, preds=preds, d_raster=d_raster)
        assert e.value.code == PCQ_ERR_ARG, e.value
        assert np.array_equal(dev.words(), PRESET)

    def swapped(seq, k, v):
        out = list(seq)
        out[k] = v
        return out

    refused(d_raster=0)                                # a null argument
    refused(nx=0), refused(ny=0), refused(nx=91, ny=91), refused(nx=CELLS_MAX + 1, ny=1), refused(nx=2**31, ny=2**31)
    for bad in (pkg.Predicate.classification(2), pkg.Predicate.bounds_class(*boxes[3], 2)):  # any other predicate kind
        refused(preds=swapped(good, 3, bad))
    c = dev.cols[5]
    for bad in (binding.make_columns(xyz=c.xyz, n=100, xyz_stride=20), binding.make_columns(xyz=c.xyz + 4, n=c.n - 1),
                binding.make_columns(xyz=None, n=100)):                                      # any other layout
        refused(cols=swapped(dev.cols, 5, bad))
    refused(cells=swapped(cws, 4, (0, 5))), refused(cells=swapped(cws, 4, (8, 0)))           # a cell width of 0 in a non-empty segment
    lo, hi = boxes[2]
    for a in (0, 1):
        out = pkg.Predicate.bounds(swapped(lo, a, I32_MIN - 1), hi)                          # lmin outside the i32 range
        refused(preds=swapped(good, 2, out), cells=swapped(cws, 2, (2**30, 2**30)))
        reach = pkg.Predicate.bounds(lo, swapped(hi, a, hi[a] + 1))                          # one lattice step beyond the raster
        refused(preds=swapped(good, 2, reach))
        refused(preds=swapped(good, 2, pkg.Predicate.bounds(lo, swapped(hi, a, 2**40))))
    # a width of 0 in the segment without points is nothing to refuse, and the table stored before the refusals serves the next call
    dev.check(boxes, swapped(cws, 0, (0, 0)), nx, ny)
    dev.check(boxes, cws, nx, ny)
