"""The rule of pcq_scan_dev_count_batch_polygon (include/pcq.h) restated for the tests: even-odd over the edges (V_i, V_(i+1) mod m),
an edge A -> B crossing a point (X, Y) iff (A.y <= Y < B.y and d > 0) or (B.y <= Y < A.y and d < 0) with
d = (B.x - A.x) (Y - A.y) - (X - A.x) (B.y - A.y).  numpy int64 is exact inside the entry's exactness bound (every product below
2^62); inside_exact is the same in Python integers, for the few points of a test that sits at the bound."""
import numpy as np


def inside(x, y, verts):
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    par = np.zeros(x.shape, dtype=bool)
    m = len(verts)
    for i in range(m):
        ax, ay = int(verts[i][0]), int(verts[i][1])
        bx, by = int(verts[(i + 1) % m][0]), int(verts[(i + 1) % m][1])
        if ay == by:
            continue  # a horizontal edge never crosses
        d = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
        par ^= ((ay <= y) & (y < by) & (d > 0)) | ((by <= y) & (y < ay) & (d < 0))
    return par


def inside_exact(x, y, verts):
    x, y = int(x), int(y)
    par, m = False, len(verts)
    for i in range(m):
        ax, ay = int(verts[i][0]), int(verts[i][1])
        bx, by = int(verts[(i + 1) % m][0]), int(verts[(i + 1) % m][1])
        d = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
        par ^= (ay <= y < by and d > 0) or (by <= y < ay and d < 0)
    return par


def in_box(xyz, lo, hi):
    p = np.asarray(xyz, dtype=np.int64)
    sel = np.ones(len(p), dtype=bool)
    for a in range(3):
        sel &= (p[:, a] >= int(lo[a])) & (p[:, a] <= int(hi[a]))
    return sel


def counted(xyz, lo, hi, verts):
    """The points of xyz (int32 [n][3]) that pass the box lo .. hi AND lie inside the outline, as a mask"""
    p = np.asarray(xyz, dtype=np.int64)
    return in_box(p, lo, hi) & inside(p[:, 0], p[:, 1], verts)


def bbox(verts, zlo=-2**40, zhi=2**40):
    """The box of the outline's vertices, z wide open"""
    v = np.asarray(verts, dtype=np.int64)
    return [int(v[:, 0].min()), int(v[:, 1].min()), zlo], [int(v[:, 0].max()), int(v[:, 1].max()), zhi]
