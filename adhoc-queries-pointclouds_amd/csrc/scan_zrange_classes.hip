// scan_zrange_classes.hip — the canopy-height raster of a box: "how high above the ground is this box, cell by cell?" asked of many
// resident LAST files in ONE pass (pcq_scan_dev_zrange_raster_batch_classes): per cell of a 2-D raster over x and y the lowest z of
// the points whose class byte is in a LOW set of the 256 classes and the highest z of the points whose class byte is in a HIGH set.
// Ground {2} and surface "everything but 7 and 18" give the canopy-height (or building-height) model; both sets equal give the
// class-filtered height raster; both sets full give the unfiltered height raster word for word.
//
// k_bounds_zrange_classes_pipe<TILES> is the height raster's kernel (scan_zrange.hip: k_bounds_zrange_pipe<TILES>) with the class bytes
// as a second column: pipe_scan (scan_tiles.h) with the cursor SegCursor<COL_RASTER_U8> over a DevRasterClassSegment table — the
// class-filtered mean-height raster's table under that entry's kind: the two kernels read every field alike, so a table uploaded by
// one entry serves the other — 2 x (3 + 2) loads per set behind the counted s_waitcnt, the two halves of that kernel's tile
// (tile_slot_masks, tile_slot_cells: raster_cells.h), the rasters' leftover loop (raster_leftovers), the exit into `partials` (max in
// the high word, min in the low one).  This file's own:
//
//   class sets    two ClassSet by value among the kernel's arguments, sixteen dwords (raster_classes.h says why not in the segment
//                 table), spread at entry into ONE table of 256 bytes in front of the raster's words in the wave's LDS: bit 0 of byte
//                 c says that c is in the low set, bit 1 that it is in the high set.  A class byte costs one ds_read_u8 for both.
//   verdicts      class_slot_masks2 (raster_classes.h) gives, per tile, twelve wave masks: low and high for the six
//                 slots, from six ds_bpermute of one word that carries both bits per byte.  A tile none of whose points passes the BOX
//                 is skipped before the transport, and again before the divisions when no passing point is in either set.
//   fold          a lane whose point passes the box and the low mask does one ds_min_i32 on zmin[cell], one whose point passes the box
//                 and the high mask one ds_max_i32 on zmax[cell]; a point in both sets does both, a point in neither nothing.
//   leftovers     the one-lane-per-point loop reads cls[p] and tests it with the same class_in_sets (the hook TwoSets).
//   finish        k_finish_zrange_classes below, not pcq_launch_finish_zrange: the two halves of a cell's word are folded each on its
//                 own (that finish skips a cell whose minimum lies above its maximum, which two sets make an ordinary case).
#include "pcq_internal.h"
#include "raster_cells.h"
#include "raster_classes.h"
#include "raster_div.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU: the height raster's rule (scan_zrange.hip: ZRANGE_WAVES_PER_CU) — the smaller of this constant and
// what a CU's LDS holds at the launch's raster size (RASTER_LDS_PER_CU / (256 + 8 nx ny): 4 at PCQ_ZRANGE_CLASSES_CELLS_MAX),
// rounded down to a multiple of four from four on (raster_waves_per_cu).  16 is the sweep's winner (profiles/zrange_classes_rate_sweep.log, option
// zrange_classes_waves_per_cu of the lab library, which takes the value as given up to the LDS limit; 16 files x 163 M points, 45 % of
// class 2, every point inside the box, generator order, ms for ground {2} and surface all but {7, 18} / both sets {2} / both sets full
// by workgroups per CU): 8 x 8 cells: 3: 14.7 / 14.6 / 14.8, 4: 10.8 / 10.7 / 11.0, 6: 9.1 / 9.0 / 9.6, 8: 7.0 / 6.8 / 8.0, 12: 6.6 /
// 6.3 / 7.7, 16: 6.4 / 6.2 / 7.5; 4096 cells: 3: 14.6 / 14.6 - 18.1 / 14.7, 4 (the LDS limit): 13.6 / 13.6 / 13.7.  DESIGN.md §4 "How
// high above the ground is this box" has the rates beside the unfiltered raster's.
constexpr int ZRANGE_CLASSES_WAVES_PER_CU = 16;

// A slot's two masks, and what the leftover loop (raster_leftovers) asks of a point beside the box: its class against both sets.
struct LowHigh {
    uint64_t low, high;
};
struct TwoSets {
    const uint32_t *table;  // class_table_fill2
    __device__ __forceinline__ uint32_t point(bool box, const DevRasterClassSegment &g, uint64_t p) const {
        return box ? class_in_sets(table, g.cls[p]) : 0u;
    }
    __device__ __forceinline__ LowHigh masks(uint32_t in) const { return {__ballot((in & CLASS_LOW) != 0), __ballot((in & CLASS_HIGH) != 0)}; }
};

// One slot: the z of the lanes in `low` into the minimum of their cells, of the lanes in `high` into the maximum (both uniform).
struct zrange_classes_fold {
    int *zmin, *zmax;
    __device__ __forceinline__ void operator()(const LowHigh &m, uint32_t cell, int z, int lane) const {
        if ((m.low >> lane) & 1ull) atomicMin(&zmin[cell], z);  // (results unused: ds_min_i32 / ds_max_i32, exec-masked)
        if ((m.high >> lane) & 1ull) atomicMax(&zmax[cell], z);
    }
};

// One tile in registers: the z of every point that passes the box into its cell's minimum when its class is in the low set and into
// its cell's maximum when its class is in the high set.  A tile none of whose points passes the BOX is skipped before the transport of
// the class verdicts, and again in front of the divisions when no passing point is in either set.
__device__ __forceinline__ void tile_zrange_classes(const v4i (&v)[3], const Col2Regs<COL_U8> &cr, const LaneBox &lb, const RasterClassCol &c,
                                                    const Col2<COL_U8> &lanes, const uint32_t *table, uint32_t nx,
                                                    const zrange_classes_fold &fold, int lane) {
    uint64_t s012[3], s3[3];
    if (!tile_slot_masks(v, lb, s012, s3)) return;
    uint64_t la[3], lb3[3], ha[3], hb3[3];
    class_slot_masks2(cr, c.shift, lanes, table, la, lb3, ha, hb3);
    LowHigh ma[3], mb[3];
#pragma unroll
    for (int k = 0; k < 3; k++) ma[k] = {la[k] & s012[k], ha[k] & s012[k]}, mb[k] = {lb3[k] & s3[k], hb3[k] & s3[k]};
    if ((ma[0].low | ma[1].low | ma[2].low | mb[0].low | mb[1].low | mb[2].low | ma[0].high | ma[1].high | ma[2].high | mb[0].high |
         mb[1].high | mb[2].high) == 0)
        return;
    uint32_t ca[3], cb[3];
    int za[3], zb[3];
    tile_slot_cells(v, c.r, nx, lane, ca, za, cb, zb);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        fold(ma[k], ca[k], za[k], lane);
        fold(mb[k], cb[k], zb[k], lane);
    }
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_zrange_classes_pipe(const DevRasterClassSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                                  uint32_t nx, uint32_t cells, ClassSet low, ClassSet high,
                                                                  uint64_t *__restrict__ partials) {
    extern __shared__ int zrange_classes_words[];  // the class table, then 2 x `cells` words: the launch's dynamic shared memory
    uint32_t *const table = reinterpret_cast<uint32_t *>(zrange_classes_words);
    int *const zmin = zrange_classes_words + CLASS_TABLE_BYTES / 4, *const zmax = zmin + cells;
    const zrange_classes_fold fold = {zmin, zmax};
    const TwoSets hook = {table};
    const int lane = threadIdx.x;
    class_table_fill2(table, low, high, lane);
    for (uint32_t i = lane; i < cells; i += 64) zmin[i] = INT32_MAX, zmax[i] = INT32_MIN;
    __syncthreads();
    pipe_scan<TILES, COL_RASTER_U8>(
        segs, nseg, total_steps, lane, [&](const PipeRegs<TILES, COL_U8> &P, const SegCursor<COL_RASTER_U8> &c, const Col2<COL_U8> &lanes) {
#pragma unroll
            for (int t = 0; t < TILES; t++) tile_zrange_classes(P.r[t], P.c[t], c.lb, c.col, lanes, table, nx, fold, lane);
        });
    raster_leftovers<TILES>(segs, nseg, nx, lane, hook, fold);
    __syncthreads();
    for (uint32_t i = lane; i < cells; i += 64)
        partials[(uint64_t)i * gridDim.x + blockIdx.x] = ((uint64_t)(uint32_t)zmax[i] << 32) | (uint64_t)(uint32_t)zmin[i];
}

// The finish: block `cell` folds slice `cell` of the per-workgroup partials and then the caller's two words, as k_finish_zrange
// (scan_count_multi.hip) does — but each word on its own.  That kernel folds a cell only where the minimum is at most the maximum,
// its test for "some point": right for one population, wrong for two, where a cell may hold surface points and no ground, or a
// ground above every surface point.  Here a half that stayed at its sentinel folds nothing and the other half is folded all the same.
constexpr int FINISH_BLOCK = 256;
__global__ __launch_bounds__(FINISH_BLOCK) void k_finish_zrange_classes(const uint64_t *__restrict__ partials, int nblocks,
                                                                       int32_t *__restrict__ d_zmin, int32_t *__restrict__ d_zmax) {
    __shared__ int32_t smin[FINISH_BLOCK], smax[FINISH_BLOCK];
    const uint64_t *slice = partials + (uint64_t)blockIdx.x * (uint64_t)nblocks;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    for (int i = threadIdx.x; i < nblocks; i += FINISH_BLOCK) {
        const uint64_t w = slice[i];
        const int32_t lo = (int32_t)(uint32_t)w, hi = (int32_t)(uint32_t)(w >> 32);
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
    }
    smin[threadIdx.x] = mn, smax[threadIdx.x] = mx;
    __syncthreads();
    for (int off = FINISH_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const int32_t a = smin[threadIdx.x + off], b = smax[threadIdx.x + off];
            if (a < smin[threadIdx.x]) smin[threadIdx.x] = a;
            if (b > smax[threadIdx.x]) smax[threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (smin[0] != INT32_MAX) atomicMin(d_zmin + blockIdx.x, smin[0]);  // (INT32_MAX folds nothing into a minimum)
        if (smax[0] != INT32_MIN) atomicMax(d_zmax + blockIdx.x, smax[0]);
    }
}

}  // namespace

extern "C" int pcq_scan_dev_zrange_raster_batch_classes(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                                        size_t nsegments, uint32_t nx, uint32_t ny, const uint32_t low_set[8],
                                                        const uint32_t high_set[8], int32_t *device_zmin, int32_t *device_zmax, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || (!cell_xy && nsegments) || !low_set || !high_set || !device_zmin || !device_zmax)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_zrange_raster_batch_classes: null argument");
    if (nx == 0 || ny == 0 || (uint64_t)nx * ny > PCQ_ZRANGE_CLASSES_CELLS_MAX)
        return pcq_fail(PCQ_ERR_ARG, "zrange_raster_batch_classes: %u x %u cells (1 .. %d in all)", nx, ny, PCQ_ZRANGE_CLASSES_CELLS_MAX);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t cells = nx * ny;
    const size_t lds = CLASS_TABLE_BYTES + 2 * cells * sizeof(int);
    int lab_waves = 0;
#ifdef PCQ_LAB  // (tools/resident_zrange_classes_rate.py sweeps it)
    lab_waves = ctx->zrange_classes_waves_per_cu;
#endif
    const int waves = raster_waves_per_cu(ZRANGE_CLASSES_WAVES_PER_CU, lds, lab_waves);
    ClassSet low, high;
    uint32_t any = 0;
    for (int w = 0; w < 8; w++) any |= (low.w[w] = low_set[w]) | (high.w[w] = high_set[w]);
    // (the class-filtered mean-height raster's table under its kind: the two kernels read it alike)
    K1Batch b = {"zrange_raster_batch_classes", PCQ_SEGMENTS_RASTER_CLASSES, waves, (int)cells, (int)cells, /*null_refused=*/true};
    b.checks_only = !any;  // both sets empty: every check of the table, then no upload, no launch, the words as they were
    return k1_batch_launch<DevRasterClassSegment>(
        ctx, b, cols, nsegments, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevRasterClassSegment &g, size_t i) { return raster_segment_fill(b.prefix, g, preds[i], cols[i], cell_xy + 2 * i, nx, ny, i); },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL((k_bounds_zrange_classes_pipe<K1_TILES>), dim3(g), dim3(64), lds, s,
                               reinterpret_cast<const DevRasterClassSegment *>(ctx->d_segments), (int)nsegments, steps, nx, cells, low, high,
                               ctx->d_partials);
            return (int)PCQ_OK;
        },
        [&](int g) {
            hipLaunchKernelGGL(k_finish_zrange_classes, dim3(cells), dim3(FINISH_BLOCK), 0, s, ctx->d_partials, g, device_zmin, device_zmax);
            PCQ_HIP(hipGetLastError());
            return (int)PCQ_OK;
        });
}
