// raster_cells.h — what the kernels that bin the points of a box into the cells of a 2-D raster over x and y share: the density
// raster (scan_raster.hip: a count per cell), the height raster (scan_zrange.hip: min and max z per cell) and the mean-height raster (scan_zsum.hip: count and z sum per cell).  The cursor kind of
// seg_seek (scan_tiles.h) that carries a segment's origin, cell widths and division magics through SGPRs, the cell of a point,
// the move of a value from the next lane, the gather of a load's points (slot_xy, for the polygon count of scan_polygon.hip), and
// — host side — the one fill of a DevRasterSegment with every refusal of the three entries.
#pragma once

#include "pcq_internal.h"
#include "raster_div.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// The raster's cursor kind for seg_seek (scan_tiles.h): no second column is loaded (PipeRegs<TILES>), the segment's constants
// take the place of one.
constexpr int COL_RASTER = 3;
template <>
struct BatchSeg<COL_RASTER> {
    typedef DevRasterSegment type;
};
template <>
struct SegCol<COL_RASTER> {
    int32_t lox, loy;      // the raster's origin: the box's lower corner, unrotated (uniform)
    uint32_t cwx, cwy;     // cell widths (uniform)
    uint32_t mx, my;       // their magics (uniform)
};
typedef SegCol<COL_RASTER> RasterCol;
// through SGPRs like the box (seg_seek says why)
__device__ __forceinline__ void segcol_seek(RasterCol &c, const DevRasterSegment &g, int) {
    int32_t lox = g.lo[0], loy = g.lo[1];
    uint32_t cwx = g.cw[0], cwy = g.cw[1], mx = g.magic[0], my = g.magic[1];
    asm volatile("" : "+s"(lox), "+s"(loy), "+s"(cwx), "+s"(cwy), "+s"(mx), "+s"(my));
    c.lox = lox, c.loy = loy, c.cwx = cwx, c.cwy = cwy, c.mx = mx, c.my = my;
}

__device__ __forceinline__ uint32_t cell_of(int x, int y, const RasterCol &c, uint32_t nx) {
    return raster_div((uint32_t)(y - c.loy), c.cwy, c.my) * nx + raster_div((uint32_t)(x - c.lox), c.cwx, c.mx);
}

// v of lane + 1; lane 63 gets `last`
__device__ __forceinline__ int next_lane(int v, int last) {
    return __builtin_amdgcn_update_dpp(last, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

// The x and y of the points that start in load k of a tile, each pair in the lane that holds the point's first dword (the polygon
// count, scan_polygon.hip; tile_raster of scan_raster.hip spells the same gather out: written through this helper its kernel came
// out of the compiler with other code — 72 compares for 24, fewer SGPR spills — and 5 % slower at 8192 cells): (xa, ya) of the point every lane starts among j = 0..2, at j0 = (3 - (k + l) % 3)
// % 3, both its own; (xb, yb) of the second point that starts at j = 3 where j0 == 0: x = v[k][3], y = the NEXT lane's v[k][0] — one
// cross-lane move per load; for lane 63 of load 0 it is lane 0's v[1][0] (v_readlane), point 85 of the tile, the only one whose x
// and y sit in different loads (lane 63 starts no second point in loads 1 and 2).  Where no second point starts (xb, yb) mean nothing.
__device__ __forceinline__ void slot_xy(const v4i (&v)[3], int k, int lane, int &xa, int &ya, int &xb, int &yb) {
    const bool j0_0 = (start_lanes(k) >> lane) & 1ull, j0_1 = (start_lanes(k + 1) >> lane) & 1ull;
    xa = j0_0 ? v[k][0] : (j0_1 ? v[k][1] : v[k][2]);
    ya = j0_0 ? v[k][1] : (j0_1 ? v[k][2] : v[k][3]);
    xb = v[k][3];
    yb = next_lane(v[k][0], k == 0 ? __builtin_amdgcn_readlane(v[1][0], 0) : 0);
}

// Segment i of a raster launch of nx x ny cells (dim) with cell widths cw, as k1_batch_launch's fill: the refusals that keep every
// passing point inside the raster — a width of 0 in a segment with points, an origin outside the i32 range, a box that reaches
// beyond the cells — then the box, the widths and their magics.  `prefix`: of a refusal's text.
inline int raster_segment_fill(const char *prefix, DevRasterSegment &g, const pcq_predicate &pred, const pcq_columns &col, const uint32_t (&cw)[2],
                               const uint32_t (&dim)[2], size_t i) {
    DevPred dp;
    const int prc = pcq_make_dev_pred(&pred, &dp);
    if (prc) return prc;
    for (int a = 0; a < 2; a++) {
        if (cw[a] == 0) {
            if (col.n) return pcq_fail(PCQ_ERR_ARG, "%s: cell width 0 on axis %d of segment %zu", prefix, a, i);
            continue;
        }
        if (dp.empty) continue;  // (matches nothing: not evaluated)
        const int64_t lmin = pred.lmin[a], lmax = pred.lmax[a] > INT32_MAX ? (int64_t)INT32_MAX : pred.lmax[a];
        if (lmin < INT32_MIN || lmin > INT32_MAX)
            return pcq_fail(PCQ_ERR_ARG, "%s: the raster's origin on axis %d of segment %zu is outside the i32 range", prefix, a, i);
        if ((uint64_t)(lmax - lmin) / cw[a] >= dim[a])
            return pcq_fail(PCQ_ERR_ARG, "%s: the box of segment %zu reaches beyond the raster's %u cells on axis %d", prefix, i, dim[a], a);
    }
    seg_box(g, dp);
    for (int a = 0; a < 2; a++) g.cw[a] = cw[a], g.magic[a] = raster_div_magic(cw[a]);
    return (int)PCQ_OK;
}

}  // namespace
