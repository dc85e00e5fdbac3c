// scan_polygon.hip — box AND polygon, count only: "how many points of this box lie inside this outline?" asked of many resident
// LAST files in ONE pass (pcq_scan_dev_count_batch_polygon).
//
// k_bounds_polygon_pipe<TILES> keeps the frame of the density raster (scan_raster.hip: k_bounds_raster_pipe) — one wave per
// workgroup, TILES tiles per step, two register sets, 2 x 3 loads per set behind the counted s_waitcnt, steps numbered across
// segments, the cursor refreshed through SGPRs at a seek (seg_seek<TILES, COL_POLYGON>: the place and the number of the segment's
// edges travel like the box), the clamped tail prefetch, the one-lane-per-point leftover loop — and, instead of dividing the x and
// y of every passing point into a cell, tests them against the edges of the segment's outline:
//
//   values     slot_xy (raster_cells.h) brings the x and y of a tile's points into one lane each: six slots per tile, per load the
//              64 first points and the up to 22 second ones.  A tile none of whose points passes the box is skipped before that;
//   edges      the outline of a segment travels behind the segment table (the K1Batch trailer) as DevPolygonEdge records: every
//              edge A -> B of the rule with its lower end first, horizontal edges left out (they never cross).  Swapping the ends
//              negates d exactly — (A - B) x (P - B) = -((B - A) x (P - A)) in integers — so "A.y <= Y < B.y and d > 0, or B.y <= Y
//              < A.y and d < 0" becomes one test per edge: lo.y <= Y < hi.y and d > 0.  The edges are wave-uniform: the kernel reads
//              them through the constant address space, 16 bytes per SCALAR load (s_load_dwordx4, counted by lgkmcnt).  No vector load is issued between the two counted waits of a step, so nothing drains the
//              prefetched register set (seg_seek, scan_tiles.h, has the history);
//   the test   per edge and slot, with ex = hi.x - lo.x and h = hi.y - lo.y uniform (SALU): py = Y - lo.y, npx = lo.x - X, the
//              range test py < h as ONE unsigned compare, d = ex * py + npx * h as two 32 x 32 -> 64-bit multiply-adds
//              (v_mad_i64_i32), the sign of d as a 64-bit compare; the lanes that cross flip their bit of the slot's parity mask,
//              which lives in an SGPR pair.  Exact by the entry's bound: for a point that passes the box every difference fits 32
//              signed bits, every product is below 2^62 and d fits an i64.  What a lane that fails the box, or holds no point,
//              computes may wrap (unsigned arithmetic: no undefined behaviour) and is masked off by the box verdict;
//   the count  popcount of (passes the box AND parity odd) per slot, added to the wave's total; one partial word per workgroup,
//              folded into *device_total by k_finish_counts (pcq_launch_finish_counts, one slice).
//
// DESIGN.md §4 "Inside an outline" has the rule, the bound, the ISA facts and the measurements.
#include <vector>

#include "pcq_internal.h"
#include "raster_cells.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU.  The pass is bound by instruction issue once most points pass the box: per edge and tile it
// issues 36 vector instructions, 12 of them quarter-rate 64-bit multiply-adds, and more resident waves keep the SIMDs issuing across
// the scalar load of the next edge.  16 files x 163 M points, the ca13_XL box, regular outlines of 4 / 16 / 64 / 256 vertices inscribed
// in it (every point of the box meets every edge) and a thin quadrilateral whose box holds a thousandth of the points, ms by
// workgroups per CU: 2: 21.5 / 54.5 / 184 / 707 and 6.61, 3: 14.3 / 36.4 / 122 / 458 and 4.81, 4: 10.8 / 28.4 / 101 / 397 and 4.66,
// 5: 11.0 / 28.0 / 94.7 / 366 and 4.73, 6: 9.2 / 23.6 / 79.3 / 302 and 4.60, 8: 6.9 / 17.6 / 59.9 / 230 and 4.68, 12: 6.3 / 15.4 /
// 53.4 / 209 and 4.57, 16: 6.0 / 14.3 / 50.3 / 196 and 4.67 (profiles/polygon_rate_sweep.log, option polygon_waves_per_cu of the lab
// library).  16 is what a CU holds (98 VGPRs: four waves per SIMD) and the best wherever the edge loop runs; where nearly every tile
// is skipped the pass is a read and the grid matters little from 3 on.  The plain box count of the same boxes takes 4.4 - 4.8 ms.
constexpr int POLYGON_WAVES_PER_CU = 16;

// The polygon count's cursor kind for seg_seek (scan_tiles.h): no second column is loaded (PipeRegs<TILES>), the place of the
// segment's edges takes the place of one.
constexpr int COL_POLYGON = 4;
template <>
struct BatchSeg<COL_POLYGON> {
    typedef DevPolygonSegment type;
};
template <>
struct SegCol<COL_POLYGON> {
    uint32_t edge_begin, nedges;  // (uniform)
};
template <>
struct PipeCol<COL_POLYGON> {
    static constexpr int value = COL_NONE;
};
// through SGPRs like the box (seg_seek says why)
__device__ __forceinline__ void segcol_seek(SegCol<COL_POLYGON> &c, const DevPolygonSegment &g, int) {
    uint32_t eb = g.edge_begin, ne = g.nedges;
    asm volatile("" : "+s"(eb), "+s"(ne));
    c.edge_begin = eb, c.nedges = ne;
}

// An edge as the kernel reads it: the four words of a DevPolygonEdge through the constant address space, where a wave-uniform
// read is a scalar load.
typedef const __attribute__((address_space(4))) v4i *EdgePtr;
__device__ __forceinline__ EdgePtr edges_at(const DevPolygonEdge *edges, uint32_t edge_begin) {
    return (EdgePtr)(uintptr_t)(edges + edge_begin);
}

// Even-odd over `ne` edges from `e` for N slots side by side: bit l of in[i] says that the point (x[i], y[i]) of lane l is inside.
// The two verdicts of an edge are two compares into SGPR pairs, ANDed and XORed there: no lane keeps a parity of its own.
template <int N>
__device__ __forceinline__ void inside_masks(EdgePtr e, uint32_t ne, const int (&x)[N], const int (&y)[N], uint64_t (&in)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) in[i] = 0;
    for (uint32_t k = 0; k < ne; k++) {
        const v4i E = e[k];
        const uint32_t ax = (uint32_t)E[0], ay = (uint32_t)E[1];
        const int ex = (int)((uint32_t)E[2] - ax);
        const uint32_t h = (uint32_t)E[3] - ay;  // (1 .. 2^31 - 1)
#pragma unroll
        for (int i = 0; i < N; i++) {
            const uint32_t py = (uint32_t)y[i] - ay;
            const int npx = (int)(ax - (uint32_t)x[i]);
            const int64_t d = (int64_t)((uint64_t)((int64_t)ex * (int64_t)(int)py) + (uint64_t)((int64_t)npx * (int64_t)(int)h));
            in[i] ^= __ballot(py < h) & __ballot(d > 0);
        }
    }
}

// One tile in registers: its points that pass the box and lie inside the outline.  A tile none of whose points passes is skipped.
__device__ __forceinline__ uint32_t tile_polygon(const v4i (&v)[3], const LaneBox &lb, EdgePtr e, uint32_t ne, int lane) {
    uint64_t t[3][4], pass[6], in[6];
    tile_start_masks(v, lb, t);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        pass[2 * k] = (t[k][0] & start_lanes(k)) | (t[k][1] & start_lanes(k + 1)) | (t[k][2] & start_lanes(k + 2));
        pass[2 * k + 1] = t[k][3] & start_lanes(k + 3);
    }
    if ((pass[0] | pass[1] | pass[2] | pass[3] | pass[4] | pass[5]) == 0) return 0;
    int x[6], y[6];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        slot_xy(v, k, lane, x[2 * k], y[2 * k], x[2 * k + 1], y[2 * k + 1]);
    }
    inside_masks<6>(e, ne, x, y, in);
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) cnt += (uint32_t)__popcll(pass[i] & in[i]);
    return cnt;
}

template <int TILES>
__device__ __forceinline__ uint64_t polygon_eval(const PipeRegs<TILES> &P, const SegCursor<COL_POLYGON> &c, const DevPolygonEdge *edges, int lane) {
    const EdgePtr e = edges_at(edges, c.col.edge_begin);
    uint64_t cnt = 0;
#pragma unroll
    for (int t = 0; t < TILES; t++) cnt += tile_polygon(P.r[t], c.lb, e, c.col.nedges, lane);
    return cnt;
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_polygon_pipe(const DevPolygonSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                           const DevPolygonEdge *__restrict__ edges, uint64_t *__restrict__ partials) {
    constexpr int COL = COL_POLYGON;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    const int lane = threadIdx.x;
    uint64_t total = 0;
    pipe_scan<TILES, COL>(segs, nseg, total_steps, lane, [&](const PipeRegs<TILES> &P, const SegCursor<COL> &c, const Col2<COL_NONE> &) {
        total += polygon_eval<TILES>(P, c, edges, lane);
    });
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevPolygonSegment &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const EdgePtr e = edges_at(edges, g.edge_begin);
        const uint32_t ne = g.nedges;
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {  // (whole waves: the masks are the wave's)
            bool pass = false;
            int x[1] = {0}, y[1] = {0};
            if (p < n) {
                const int *q = q0 + 3 * p;
                x[0] = q[0], y[0] = q[1];
                pass = ((uint32_t)(x[0] - g.lo[0]) <= g.width[0]) & ((uint32_t)(y[0] - g.lo[1]) <= g.width[1]) & ((uint32_t)(q[2] - g.lo[2]) <= g.width[2]);
            }
            const uint64_t m = __ballot(pass);
            if (m == 0) continue;
            uint64_t in[1];
            inside_masks<1>(e, ne, x, y, in);
            total += (uint64_t)__popcll(m & in[0]);
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

// The hull of the box's range (clamped to i32: dp) and the vertices' range on axis a spans at most 2^31 - 1.
bool hull_exact(const DevPred &dp, const int32_t *verts, size_t nverts, int a) {
    int64_t lo = dp.lo[a], hi = (int64_t)dp.lo[a] + (int64_t)dp.width[a];
    for (size_t j = 0; j < nverts; j++) {
        const int64_t v = verts[2 * j + a];
        if (v < lo) lo = v;
        if (v > hi) hi = v;
    }
    return hi - lo <= (int64_t)INT32_MAX;
}

}  // namespace

extern "C" int pcq_scan_dev_count_batch_polygon(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const int32_t *verts_xy,
                                                size_t nsegments, size_t nverts, uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !cols || !preds || !verts_xy || !device_total) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_count_batch_polygon: null argument");
    if (nverts < 3 || nverts > PCQ_POLYGON_VERTS_MAX)
        return pcq_fail(PCQ_ERR_ARG, "count_batch_polygon: %zu vertices (3 .. %d)", nverts, PCQ_POLYGON_VERTS_MAX);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int waves = POLYGON_WAVES_PER_CU;
#ifdef PCQ_LAB  // (tools/resident_polygon_rate.py sweeps it)
    if (ctx->polygon_waves_per_cu) waves = ctx->polygon_waves_per_cu;
#endif
    // The trailer: the edges of segment 0, 1, ... one after the other, zeros behind them.  One size whatever the outlines hold, so that
    // the K1Batch can name it before the segments are filled.
    std::vector<DevPolygonEdge> edges(nsegments * nverts, DevPolygonEdge{0, 0, 0, 0});
    uint32_t nedges = 0;
    const K1Batch b = {"count_batch_polygon", PCQ_SEGMENTS_POLYGON, waves, 1, 1, /*null_refused=*/true,
                       edges.data(), edges.size() * sizeof(DevPolygonEdge)};
    return k1_batch_launch<DevPolygonSegment>(
        ctx, b, cols, nsegments, device_total, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevPolygonSegment &g, size_t i) {
            DevPred dp;
            const int prc = pcq_make_dev_pred(&preds[i], &dp);
            if (prc) return prc;
            seg_box(g, dp);
            g.edge_begin = nedges;
            if (dp.empty) return (int)PCQ_OK;  // (matches nothing: not evaluated, its vertices not examined)
            const int32_t *v = verts_xy + 2 * nverts * i;
            for (int a = 0; a < 2; a++)
                if (!hull_exact(dp, v, nverts, a))
                    return pcq_fail(PCQ_ERR_ARG, "count_batch_polygon: the box and the outline of segment %zu span more than 2^31 - 1 on axis %d", i, a);
            for (size_t j = 0; j < nverts; j++) {
                const int32_t *p = v + 2 * j, *q = v + 2 * ((j + 1) % nverts);
                if (p[1] == q[1]) continue;  // (a horizontal edge never crosses)
                edges[nedges++] = p[1] < q[1] ? DevPolygonEdge{p[0], p[1], q[0], q[1]} : DevPolygonEdge{q[0], q[1], p[0], p[1]};
            }
            g.nedges = nedges - g.edge_begin;
            return (int)PCQ_OK;
        },
        [&](unsigned g, uint64_t steps) {
            const uint8_t *behind = reinterpret_cast<const uint8_t *>(ctx->d_segments) + nsegments * sizeof(DevPolygonSegment);
            hipLaunchKernelGGL((k_bounds_polygon_pipe<K1_TILES>), dim3(g), dim3(64), 0, s,
                               reinterpret_cast<const DevPolygonSegment *>(ctx->d_segments), (int)nsegments, steps,
                               reinterpret_cast<const DevPolygonEdge *>(behind), ctx->d_partials);
            return (int)PCQ_OK;
        });
}
