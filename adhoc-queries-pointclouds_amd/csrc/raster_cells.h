// raster_cells.h — what the kernels that bin the points of a box into the cells of a 2-D raster over x and y share: the density
// raster (scan_raster.hip: a count per cell), the height raster (scan_zrange.hip: min and max z per cell), the mean-height raster
// (scan_zsum.hip: count and z sum per cell), the height-spread raster (scan_zmoments.hip: count, z sum and z^2 sum per cell) and, with
// the class sets of raster_classes.h, the ground-only mean-height raster (scan_zsum_classes.hip) and the canopy-height raster
// (scan_zrange_classes.hip).  All six share the cursor, cell_of, next_lane and the host side; the three that add 64-bit words
// measured slower on a shared tile and leftover loop at their largest rasters and keep their own text of both (their files say by
// how much).  Device side: the cursor kind of pipe_scan / seg_seek (scan_tiles.h) that carries a segment's origin, cell
// widths and division magics through SGPRs, the cell of a point, the move of a value from the next lane, the gather of a load's points
// (slot_xy, for the polygon count of scan_polygon.hip), the two halves of a z-carrying tile that the height and the canopy-height
// rasters share (tile_slot_masks, tile_slot_cells), and the one-lane-per-point loop over a segment's leftovers (raster_leftovers: the
// density, height and canopy-height rasters).
// Host side: the workgroups per CU of a raster launch (raster_waves_per_cu) and the one fill of a DevRasterSegment with every refusal
// of the six entries (raster_segment_fill).
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
template <>
struct PipeCol<COL_RASTER> {
    static constexpr int value = COL_NONE;
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

// The six slots of a tile: per load k the point every lane starts among j = 0..2 (s012[k]) and the second point that starts at j = 3
// where j0 == 0 (s3[k]); bit l of a mask says that lane l's point of the slot passes the box.  False when no point of the tile does.
__device__ __forceinline__ bool tile_slot_masks(const v4i (&v)[3], const LaneBox &lb, uint64_t (&s012)[3], uint64_t (&s3)[3]) {
    uint64_t t[3][4];
    tile_start_masks(v, lb, t);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s012[k] = (t[k][0] & start_lanes(k)) | (t[k][1] & start_lanes(k + 1)) | (t[k][2] & start_lanes(k + 2));
        s3[k] = t[k][3] & start_lanes(k + 3);
    }
    return (s012[0] | s012[1] | s012[2] | s3[0] | s3[1] | s3[2]) != 0;
}
// The cell and the z of the six slots' points, each in the lane that holds the point's first dword: in load k lane l starts one point
// at j0 = (3 - (k + l) % 3) % 3, whose z is dword j0 + 2 of the lane — v[k][2] or v[k][3] for j0 = 0 or 1, the NEXT lane's v[k][0] for
// j0 = 2 — and where j0 == 0 a second one at j = 3: x = v[k][3], y and z = the next lane's v[k][0] and v[k][1].  Two cross-lane moves
// per load (DPP wave_shl:1); lane 63 takes what lies behind its load from lane 0 of the next one (v_readlane): in load 0 the second
// point's y and z (point 85 of the tile), in load 1 the first point's z (point 170), in load 2 nothing.  Straight-line code, so that
// the twelve divisions overlap.
__device__ __forceinline__ void tile_slot_cells(const v4i (&v)[3], const RasterCol &c, uint32_t nx, int lane, uint32_t (&ca)[3], int (&za)[3],
                                                uint32_t (&cb)[3], int (&zb)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const bool j0_0 = (start_lanes(k) >> lane) & 1ull, j0_1 = (start_lanes(k + 1) >> lane) & 1ull;
        // dwords 4 and 5 of the lane: the next lane's 0 and 1; behind lane 63, lane 0 of the next load (the tile ends with load 2)
        const int n0 = next_lane(v[k][0], k < 2 ? __builtin_amdgcn_readlane(v[k < 2 ? k + 1 : k][0], 0) : 0);
        const int n1 = next_lane(v[k][1], k < 2 ? __builtin_amdgcn_readlane(v[k < 2 ? k + 1 : k][1], 0) : 0);
        const int x = j0_0 ? v[k][0] : (j0_1 ? v[k][1] : v[k][2]);
        const int y = j0_0 ? v[k][1] : (j0_1 ? v[k][2] : v[k][3]);
        za[k] = j0_0 ? v[k][2] : (j0_1 ? v[k][3] : n0);
        ca[k] = cell_of(x, y, c, nx);
        cb[k] = cell_of(v[k][3], n0, c, nx);
        zb[k] = n1;
    }
}
// What a raster kernel asks of a point of the leftover loop beside the box.  Nothing: the box verdicts are the fold's masks.
// (scan_zrange_classes.hip has the hook of its two class sets.)
struct BoxOnly {
    template <typename Seg>
    __device__ __forceinline__ bool point(bool box, const Seg &, uint64_t) const { return box; }
    __device__ __forceinline__ uint64_t masks(bool in) const { return __ballot(in); }
};
// The fewer-than-a-step leftovers of the segments blockIdx.x, blockIdx.x + gridDim.x, ..., one lane per point, in whole waves (the
// fold's masks are the wave's): fold(hook.masks(verdict), cell, z, lane) once per 64 points.
template <int TILES, typename Seg, typename Hook, typename Fold>
__device__ __forceinline__ void raster_leftovers(const Seg *__restrict__ segs, int nseg, uint32_t nx, int lane, const Hook &hook, const Fold &fold) {
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {
        const Seg &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const RasterCol c = {g.lo[0], g.lo[1], g.cw[0], g.cw[1], g.magic[0], g.magic[1]};
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {
            decltype(hook.point(false, g, p)) in{};
            int x = 0, y = 0, z = 0;
            if (p < n) {
                const int *q = q0 + 3 * p;
                x = q[0], y = q[1], z = q[2];
                in = hook.point(((uint32_t)(x - g.lo[0]) <= g.width[0]) & ((uint32_t)(y - g.lo[1]) <= g.width[1]) & ((uint32_t)(z - g.lo[2]) <= g.width[2]),
                                g, p);
            }
            fold(hook.masks(in), cell_of(x, y, c, nx), z, lane);
        }
    }
}

// Workgroups (of one wave) per CU of a raster launch: the smaller of the kernel's constant and what a CU's LDS holds at the launch's
// raster size, rounded down to a multiple of four from four on, so that no SIMD of a CU carries a wave more than another.  The lab
// library's sweeps (lab_override, 0: none) are taken as given up to the LDS limit: a sweep sees 5 and 6 as they are.  The constants
// and what was measured for them stand in the kernels' files.
constexpr uint32_t RASTER_LDS_PER_CU = 160 * 1024;
inline int raster_waves_per_cu(int default_waves, size_t lds_bytes, int lab_override) {
    int waves = lab_override ? lab_override : default_waves;
    const int by_lds = (int)(RASTER_LDS_PER_CU / lds_bytes);  // (>= 4: every entry's *_CELLS_MAX)
    if (waves > by_lds) waves = by_lds;
    if (!lab_override && waves > 4) waves &= ~3;
    return waves;
}

// Segment i of a raster launch of nx x ny cells with cell widths cw[0], cw[1], as k1_batch_launch's fill: the refusals that keep every
// passing point inside the raster — a width of 0 in a segment with points, an origin outside the i32 range, a box that reaches
// beyond the cells — then the box, the widths and their magics.  `prefix`: of a refusal's text.
inline int raster_segment_fill(const char *prefix, DevRasterSegment &g, const pcq_predicate &pred, const pcq_columns &col, const uint32_t *cw,
                               uint32_t nx, uint32_t ny, size_t i) {
    const uint32_t dim[2] = {nx, ny};
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
