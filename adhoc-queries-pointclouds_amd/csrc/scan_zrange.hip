// scan_zrange.hip — the height raster of a box: "how high is this box, cell by cell?" asked of many resident LAST files in ONE pass
// (pcq_scan_dev_zrange_raster_batch): the lowest and the highest z of the points of every cell of a 2-D raster over x and y.
//
// k_bounds_zrange_pipe<TILES> is the density raster's kernel (scan_raster.hip: k_bounds_raster_pipe<TILES, false>) up to the LDS
// operation — one wave per workgroup, TILES tiles per step, two register sets, 2 x 3 loads per set behind the counted s_waitcnt, the
// cursor SegCursor<COL_RASTER> over the same DevRasterSegment table, the clamped tail prefetch, skipped empty segments and skipped
// tiles without a passing point, the cell by two exact divisions (raster_cells.h, raster_div.h) — and brings the z of every passing
// point to the lane that holds its cell as well:
//
//   values     in load k lane l starts one point among j = 0..2, at j0 = (3 - (k + l) % 3) % 3; its z is dword j0 + 2 of the lane:
//              v[k][2] or v[k][3] for j0 = 0 or 1, the NEXT lane's v[k][0] for j0 = 2.  Where j0 == 0 a second point starts at
//              j = 3: x = v[k][3], y and z = the next lane's v[k][0] and v[k][1].  So two cross-lane moves per load (DPP
//              wave_shl:1), and lane 63 — (k + 63) % 3 == k % 3 — takes what lies behind its load from lane 0 of the next one
//              (v_readlane): in load 0 (j0 == 0) the second point's y = v[1][0] and z = v[1][1], point 85 of the tile; in load 1
//              (j0 == 2) the first point's z = v[2][0], point 170; in load 2 (j0 == 1) all its own.  The verdicts are the density
//              raster's: bit l of s012 for the first point, of t3 & start_lanes(k + 3) for the second; they include the z test, so
//              a point that fails only on z — by construction the most extreme z around — contributes nothing;
//   raster     2 x nx * ny i32 words of DYNAMIC shared memory, private to the wave: the minima, set to INT32_MAX, then the maxima,
//              set to INT32_MIN.  Every passing lane does one ds_min_i32 and one ds_max_i32 on its cell (atomicMin / atomicMax on
//              int with the result unused).  No wave-level shortcut: for the add it was measured and lost (scan_raster.hip,
//              RASTER_WAVE_ADD).
//
// At exit the wave writes one u64 per cell to partials[cell * gridDim.x + blockIdx.x], max in the high word and min in the low
// one; k_finish_zrange (scan_count_multi.hip) folds slice `cell` into device_zmin[cell] and device_zmax[cell] with a signed
// min / max.  Nothing can overflow: the words are values of the data.
#include "pcq_internal.h"
#include "raster_cells.h"
#include "raster_div.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU: the density raster's rule with twice the LDS per cell — the smaller of this constant and what a
// CU's LDS holds at the launch's raster size (ZRANGE_LDS_PER_CU / (8 nx ny): 5 at PCQ_ZRANGE_CELLS_MAX, 20 at 32 x 32), rounded down
// to a multiple of four from four on, so that no SIMD of a CU carries a wave more than another.  Measured (16 files x 163 M points,
// every point inside the box, generator order, ms by workgroups per CU): 8 x 8 cells: 2: 15.1, 4: 7.3, 8: 6.3, 16: 6.2; 4096 cells:
// 3: 10.1 - 12.3, 4: 9.3, 5 (the LDS limit): 13.4.  In scan-strip order all 64 lanes of a slot meet one LDS word and the pass takes
// 14 - 17 ms whatever the grid.  DESIGN.md §4 "How high is this box" has the sweep (profiles/zrange_raster_rate_sweep.log, option
// zrange_waves_per_cu of the lab library, which takes the value as given up to the LDS limit).
constexpr int ZRANGE_WAVES_PER_CU = 16;
constexpr uint32_t ZRANGE_LDS_PER_CU = 160 * 1024;

// One slot: the z of the lanes in `pass` (uniform) into the two words of their cells.
__device__ __forceinline__ void zrange_fold(int *zmin, int *zmax, uint64_t pass, uint32_t cell, int z, int lane) {
    if ((pass >> lane) & 1ull) {
        atomicMin(&zmin[cell], z);  // (results unused: ds_min_i32 / ds_max_i32, exec-masked)
        atomicMax(&zmax[cell], z);
    }
}

// One tile in registers: the z of every passing point into its cell's words.  A tile none of whose points passes is skipped;
// otherwise the six slots are straight-line code, so that their divisions overlap.
__device__ __forceinline__ void tile_zrange(const v4i (&v)[3], const LaneBox &lb, const RasterCol &c, uint32_t nx, int *zmin, int *zmax, int lane) {
    uint64_t t[3][4], s012[3], s3[3];
    tile_start_masks(v, lb, t);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s012[k] = (t[k][0] & start_lanes(k)) | (t[k][1] & start_lanes(k + 1)) | (t[k][2] & start_lanes(k + 2));
        s3[k] = t[k][3] & start_lanes(k + 3);
    }
    if ((s012[0] | s012[1] | s012[2] | s3[0] | s3[1] | s3[2]) == 0) return;
    uint32_t ca[3], cb[3];
    int za[3], zb[3];
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
#pragma unroll
    for (int k = 0; k < 3; k++) {
        zrange_fold(zmin, zmax, s012[k], ca[k], za[k], lane);
        zrange_fold(zmin, zmax, s3[k], cb[k], zb[k], lane);
    }
}

template <int TILES>
__device__ __forceinline__ void zrange_eval(const PipeRegs<TILES> &P, const SegCursor<COL_RASTER> &c, uint32_t nx, int *zmin, int *zmax, int lane) {
#pragma unroll
    for (int t = 0; t < TILES; t++) tile_zrange(P.r[t], c.lb, c.col, nx, zmin, zmax, lane);
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_zrange_pipe(const DevRasterSegment *__restrict__ segs, int nseg, uint64_t total_steps, uint32_t nx,
                                                          uint32_t cells, uint64_t *__restrict__ partials) {
    constexpr int COL = COL_RASTER;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    constexpr int LOADS = PipeRegs<TILES>::LOADS;  // per register set
    extern __shared__ int zwords[];                // 2 x `cells` words: the launch's dynamic shared memory
    int *const zmin = zwords, *const zmax = zwords + cells;
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    for (uint32_t i = lane; i < cells; i += 64) zmin[i] = INT32_MAX, zmax[i] = INT32_MIN;
    __syncthreads();
    if (blockIdx.x < total_steps) {
        PipeRegs<TILES> A, B;
        SegCursor<COL> ca = {0, 0, 0, nullptr, {}, true, {}}, cb;
        uint64_t u = blockIdx.x;
        seg_seek<TILES, COL>(ca, segs, nseg, u, lane);
        pipe_load<TILES>(A, ca.base, u - ca.begin, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) seg_seek<TILES, COL>(cb, segs, nseg, u1, lane);
            pipe_load<TILES>(B, cb.base, (u1 < total_steps ? u1 : u) - cb.begin, lane);  // clamped at the tail: an L2 hit
            pipe_wait<LOADS>(A);
            if (!ca.empty) zrange_eval<TILES>(A, ca, nx, zmin, zmax, lane);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES, COL>(ca, segs, nseg, u2, lane);
            pipe_load<TILES>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane);
            pipe_wait<LOADS>(B);
            if (!cb.empty) zrange_eval<TILES>(B, cb, nx, zmin, zmax, lane);
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<0>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<0>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevRasterSegment &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const RasterCol c = {g.lo[0], g.lo[1], g.cw[0], g.cw[1], g.magic[0], g.magic[1]};
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {  // (whole waves: the slot's masks are the wave's)
            bool pass = false;
            int x = 0, y = 0, z = 0;
            if (p < n) {
                const int *q = q0 + 3 * p;
                x = q[0], y = q[1], z = q[2];
                pass = ((uint32_t)(x - g.lo[0]) <= g.width[0]) & ((uint32_t)(y - g.lo[1]) <= g.width[1]) & ((uint32_t)(z - g.lo[2]) <= g.width[2]);
            }
            zrange_fold(zmin, zmax, __ballot(pass), cell_of(x, y, c, nx), z, lane);
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < cells; i += 64)
        partials[(uint64_t)i * gridDim.x + blockIdx.x] = ((uint64_t)(uint32_t)zmax[i] << 32) | (uint64_t)(uint32_t)zmin[i];
}

}  // namespace

extern "C" int pcq_scan_dev_zrange_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                                size_t nsegments, uint32_t nx, uint32_t ny, int32_t *device_zmin, int32_t *device_zmax, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || (!cell_xy && nsegments) || !device_zmin || !device_zmax)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_zrange_raster_batch: null argument");
    if (nx == 0 || ny == 0 || (uint64_t)nx * ny > PCQ_ZRANGE_CELLS_MAX)
        return pcq_fail(PCQ_ERR_ARG, "zrange_raster_batch: %u x %u cells (1 .. %d in all)", nx, ny, PCQ_ZRANGE_CELLS_MAX);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t cells = nx * ny;
    const size_t lds = 2 * cells * sizeof(int);
    int waves = ZRANGE_WAVES_PER_CU;
    bool whole_simds = true;
#ifdef PCQ_LAB  // (tools/resident_zrange_rate.py sweeps it; the sweep sees 5 and 6 as they are)
    if (ctx->zrange_waves_per_cu) waves = ctx->zrange_waves_per_cu, whole_simds = false;
#endif
    const int by_lds = (int)(ZRANGE_LDS_PER_CU / lds);  // (>= 5: cells <= PCQ_ZRANGE_CELLS_MAX)
    if (waves > by_lds) waves = by_lds;
    if (whole_simds && waves > 4) waves &= ~3;
    // (the density raster's table under its kind: the two kernels read it alike)
    const K1Batch b = {"zrange_raster_batch", PCQ_SEGMENTS_RASTER, waves, (int)cells, (int)cells, /*null_refused=*/true};
    return k1_batch_launch<DevRasterSegment>(
        ctx, b, cols, nsegments, s,
        [&](size_t i) {
            return preds[i].kind != PCQ_PRED_BOUNDS
                       ? pcq_fail(PCQ_ERR_ARG, "zrange_raster_batch: predicate kind %d of segment %zu (PCQ_PRED_BOUNDS only)", preds[i].kind, i)
                       : (int)PCQ_OK;
        },
        [&](DevRasterSegment &g, size_t i) {
            const uint32_t cw[2] = {cell_xy[2 * i], cell_xy[2 * i + 1]};
            const uint32_t dim[2] = {nx, ny};
            return raster_segment_fill("zrange_raster_batch", g, preds[i], cols[i], cw, dim, i);
        },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL((k_bounds_zrange_pipe<K1_TILES>), dim3(g), dim3(64), lds, s, reinterpret_cast<const DevRasterSegment *>(ctx->d_segments),
                               (int)nsegments, steps, nx, cells, ctx->d_partials);
            return (int)PCQ_OK;
        },
        [&](int g) { return pcq_launch_finish_zrange(ctx, (int)cells, g, device_zmin, device_zmax, s); });
}
