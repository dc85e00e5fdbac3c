// scan_zrange.hip — the height raster of a box: "how high is this box, cell by cell?" asked of many resident LAST files in ONE pass
// (pcq_scan_dev_zrange_raster_batch): the lowest and the highest z of the points of every cell of a 2-D raster over x and y.
//
// k_bounds_zrange_pipe<TILES> runs the software pipeline of the batched scans over the DevRasterSegment table (pipe_scan of
// scan_tiles.h: one wave per workgroup, TILES tiles per step, two register sets, 2 x 3 loads per set behind the counted s_waitcnt, the
// clamped tail prefetch, skipped empty segments) and the rasters' one-lane-per-point leftover loop (raster_leftovers of raster_cells.h).
// Its tile brings the cell and the z of every passing point to one lane through tile_slot_masks and tile_slot_cells (raster_cells.h,
// shared with the canopy-height raster; tile_slot_cells says which dword is whose).  The verdicts are the
// density raster's; they include the z test, so a point that fails only on z — by construction the most extreme z around —
// contributes nothing.  This file's own:
//
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
// CU's LDS holds at the launch's raster size (RASTER_LDS_PER_CU / (8 nx ny): 5 at PCQ_ZRANGE_CELLS_MAX, 20 at 32 x 32), rounded down
// to a multiple of four from four on (raster_waves_per_cu).  Measured (16 files x 163 M points,
// every point inside the box, generator order, ms by workgroups per CU): 8 x 8 cells: 2: 15.1, 4: 7.3, 8: 6.3, 16: 6.2; 4096 cells:
// 3: 10.1 - 12.3, 4: 9.3, 5 (the LDS limit): 13.4.  In scan-strip order all 64 lanes of a slot meet one LDS word and the pass takes
// 14 - 17 ms whatever the grid.  DESIGN.md §4 "How high is this box" has the sweep (profiles/zrange_raster_rate_sweep.log, option
// zrange_waves_per_cu of the lab library, which takes the value as given up to the LDS limit).
constexpr int ZRANGE_WAVES_PER_CU = 16;
// (the rasters' one LDS limit, RASTER_LDS_PER_CU of raster_cells.h, under the name the launch-plan test restates for this kernel)
constexpr uint32_t ZRANGE_LDS_PER_CU = 160 * 1024;
static_assert(ZRANGE_LDS_PER_CU == RASTER_LDS_PER_CU, "one LDS limit for every raster kernel");

// One slot: the z of the lanes in `pass` (uniform) into the two words of their cells.
struct zrange_fold {
    int *zmin, *zmax;
    __device__ __forceinline__ void operator()(uint64_t pass, uint32_t cell, int z, int lane) const {
        if ((pass >> lane) & 1ull) {
            atomicMin(&zmin[cell], z);  // (results unused: ds_min_i32 / ds_max_i32, exec-masked)
            atomicMax(&zmax[cell], z);
        }
    }
};

// One tile in registers: the z of every passing point into its cell's words.  A tile none of whose points passes is skipped;
// otherwise the six slots are straight-line code, so that their divisions overlap.
__device__ __forceinline__ void tile_zrange(const v4i (&v)[3], const LaneBox &lb, const RasterCol &c, uint32_t nx, const zrange_fold &fold, int lane) {
    uint64_t s012[3], s3[3];
    if (!tile_slot_masks(v, lb, s012, s3)) return;
    uint32_t ca[3], cb[3];
    int za[3], zb[3];
    tile_slot_cells(v, c, nx, lane, ca, za, cb, zb);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        fold(s012[k], ca[k], za[k], lane);
        fold(s3[k], cb[k], zb[k], lane);
    }
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_zrange_pipe(const DevRasterSegment *__restrict__ segs, int nseg, uint64_t total_steps, uint32_t nx,
                                                          uint32_t cells, uint64_t *__restrict__ partials) {
    extern __shared__ int zwords[];  // 2 x `cells` words: the launch's dynamic shared memory
    const zrange_fold fold = {zwords, zwords + cells};
    const int lane = threadIdx.x;
    for (uint32_t i = lane; i < cells; i += 64) fold.zmin[i] = INT32_MAX, fold.zmax[i] = INT32_MIN;
    __syncthreads();
    pipe_scan<TILES, COL_RASTER>(segs, nseg, total_steps, lane, [&](const PipeRegs<TILES> &P, const SegCursor<COL_RASTER> &c, const Col2<COL_NONE> &) {
#pragma unroll
        for (int t = 0; t < TILES; t++) tile_zrange(P.r[t], c.lb, c.col, nx, fold, lane);
    });
    raster_leftovers<TILES>(segs, nseg, nx, lane, BoxOnly{}, fold);
    __syncthreads();
    for (uint32_t i = lane; i < cells; i += 64)
        partials[(uint64_t)i * gridDim.x + blockIdx.x] = ((uint64_t)(uint32_t)fold.zmax[i] << 32) | (uint64_t)(uint32_t)fold.zmin[i];
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
    int lab_waves = 0;
#ifdef PCQ_LAB  // (tools/resident_zrange_rate.py sweeps it)
    lab_waves = ctx->zrange_waves_per_cu;
#endif
    const int waves = raster_waves_per_cu(ZRANGE_WAVES_PER_CU, lds, lab_waves);
    // (the density raster's table under its kind: the two kernels read it alike)
    const K1Batch b = {"zrange_raster_batch", PCQ_SEGMENTS_RASTER, waves, (int)cells, (int)cells, /*null_refused=*/true};
    return k1_batch_launch<DevRasterSegment>(
        ctx, b, cols, nsegments, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevRasterSegment &g, size_t i) { return raster_segment_fill(b.prefix, g, preds[i], cols[i], cell_xy + 2 * i, nx, ny, i); },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL((k_bounds_zrange_pipe<K1_TILES>), dim3(g), dim3(64), lds, s, reinterpret_cast<const DevRasterSegment *>(ctx->d_segments),
                               (int)nsegments, steps, nx, cells, ctx->d_partials);
            return (int)PCQ_OK;
        },
        [&](int g) { return pcq_launch_finish_zrange(ctx, (int)cells, g, device_zmin, device_zmax, s); });
}
