// scan_zsum_classes.hip — the mean-height raster of the GROUND of a box: "how high are the points of these classes in this box on
// average, cell by cell?" asked of many resident LAST files in ONE pass (pcq_scan_dev_zsum_raster_batch_classes): the number of points
// of every cell of a 2-D raster over x and y whose class byte is in a set of the 256 classes, and the sum of their z.  A terrain
// model is the set {2}, or {2, 9}; a surface model everything but noise.  The count array is the class-filtered density raster.
//
// k_bounds_zsum_classes_pipe<TILES> is the mean-height raster's kernel (scan_zsum.hip: k_bounds_zsum_pipe<TILES>) with the class bytes
// as a second column — one wave per workgroup, TILES tiles per step, two register sets, 2 x (3 + 2) loads per set behind the counted
// s_waitcnt (PipeRegs<TILES, COL_U8>: the registers and loads of the box AND class count), the cursor SegCursor<COL_RASTER_U8> over a
// DevRasterClassSegment table, the clamped tail prefetch, skipped empty segments and skipped tiles without a passing point, the cell
// by two exact divisions (raster_cells.h, raster_div.h), the six straight-line slots, two ds_add_u64 per passing point into 2 x cells
// words of dynamic LDS (behind the 256 bytes of the class table), the exit into `partials` and pcq_launch_finish_zsum.  What differs:
//
//   class set     eight dwords among the kernel's arguments (raster_classes.h says why not in the segment table), spread at entry into
//                 a table of 256 bytes in front of the raster's words in the wave's LDS: the test of a class byte is one ds_read_u8.
//   verdicts      class_slot_masks (raster_classes.h) gives, per tile, the six wave masks "the point this lane starts in this slot is of
//                 a class in the set"; they are ANDed into s012[k] / s3[k] before the "no passing point" skip, so a tile none of whose
//                 points is ground costs no division and no LDS add.  A tile none of whose points passes the BOX is skipped before
//                 the transport.
//   leftovers     the one-lane-per-point loop reads cls[p] and tests it with the same class_in_set.
//
// The slots of tile_zsum_classes are tile_zsum's (scan_zsum.hip), spelt out again: that file's kernel is to come out of the compiler
// as it was (profiles/zsum_classes_asm_compare.log).
// This kernel keeps its own text of the pipeline loop, the tile and the leftover loop.  On pipe_scan (scan_tiles.h), a tile shared
// with the height raster and raster_leftovers (raster_cells.h) it compiled to a kernel structurally equal to this one (equal VGPRs, occupancy,
// waits, loads, LDS operations and compares) that ran 1.2 % and 1.0 % slower (9.747 against 9.634 ms, 10.602 against 10.497; spreads 0.025, 0.030) at the largest raster, where
// the LDS leaves one wave per SIMD, and inside the parent's spread at 8 x 8 cells (profiles/raster_frame_rate.log): outside the rule
// of that change, so the copy stays.
#include "pcq_internal.h"
#include "raster_cells.h"
#include "raster_classes.h"
#include "raster_div.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU: the mean-height raster's rule (scan_zsum.hip: ZSUM_WAVES_PER_CU) — the smaller of this constant and
// what a CU's LDS holds at the launch's raster size (RASTER_LDS_PER_CU / (256 + 16 nx ny): 4 at PCQ_ZSUM_CELLS_MAX), rounded
// down to a multiple of four from four on.  16 is the sweep's winner (profiles/zsum_classes_rate_sweep.log, option
// zsum_classes_waves_per_cu of the lab library, which takes the value as given up to the LDS limit; 16 files x 163 M points, 45 % of
// class 2, every point inside the box, generator order, ms for the set {2} / all 256 classes by workgroups per CU): 8 x 8 cells: 3:
// 13.3 / 13.6, 4: 9.7 / 10.3, 6: 8.0 / 9.2, 8: 6.4 / 8.1, 12: 5.9 / 8.1, 16: 5.9 / 8.0; 2048 cells: 3: 13.2 / 13.2, 4 (the LDS limit):
// 9.6 / 9.6.  DESIGN.md §4 "How high is the ground in this box" has the rates beside the unfiltered raster's.
constexpr int ZSUM_CLASSES_WAVES_PER_CU = 16;

// One slot: a point and its z from the lanes in `pass` (uniform) into the two words of their cells.
__device__ __forceinline__ void zsum_classes_fold(unsigned long long *cnt, unsigned long long *sum, uint64_t pass, uint32_t cell, int z, int lane) {
    if ((pass >> lane) & 1ull) {
        atomicAdd(&cnt[cell], 1ull);  // (results unused: ds_add_u64, exec-masked)
        atomicAdd(&sum[cell], (unsigned long long)(long long)z);
    }
}

// One tile in registers: every point that passes the box and whose class is in the set into its cell's words.
__device__ __forceinline__ void tile_zsum_classes(const v4i (&v)[3], const Col2Regs<COL_U8> &cr, const LaneBox &lb, const RasterClassCol &c,
                                                  const Col2<COL_U8> &lanes, const uint32_t *table, uint32_t nx, unsigned long long *cnt,
                                                  unsigned long long *sum, int lane) {
    uint64_t t[3][4], s012[3], s3[3];
    tile_start_masks(v, lb, t);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s012[k] = (t[k][0] & start_lanes(k)) | (t[k][1] & start_lanes(k + 1)) | (t[k][2] & start_lanes(k + 2));
        s3[k] = t[k][3] & start_lanes(k + 3);
    }
    if ((s012[0] | s012[1] | s012[2] | s3[0] | s3[1] | s3[2]) == 0) return;
    uint64_t va[3], vb[3];
    class_slot_masks(cr, c.shift, lanes, table, va, vb);
#pragma unroll
    for (int k = 0; k < 3; k++) s012[k] &= va[k], s3[k] &= vb[k];
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
        ca[k] = cell_of(x, y, c.r, nx);
        cb[k] = cell_of(v[k][3], n0, c.r, nx);
        zb[k] = n1;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        zsum_classes_fold(cnt, sum, s012[k], ca[k], za[k], lane);
        zsum_classes_fold(cnt, sum, s3[k], cb[k], zb[k], lane);
    }
}

template <int TILES>
__device__ __forceinline__ void zsum_classes_eval(const PipeRegs<TILES, COL_U8> &P, const SegCursor<COL_RASTER_U8> &c, const Col2<COL_U8> &lanes,
                                                  const uint32_t *table, uint32_t nx, unsigned long long *cnt, unsigned long long *sum, int lane) {
#pragma unroll
    for (int t = 0; t < TILES; t++) tile_zsum_classes(P.r[t], P.c[t], c.lb, c.col, lanes, table, nx, cnt, sum, lane);
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_zsum_classes_pipe(const DevRasterClassSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                                uint32_t nx, uint32_t cells, ClassSet set, uint64_t *__restrict__ partials) {
    constexpr int COL = COL_RASTER_U8;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    constexpr int LOADS = PipeRegs<TILES, COL_U8>::LOADS;  // per register set
    extern __shared__ unsigned long long zsum_classes_words[];  // the class table, then 2 x `cells` words: the launch's dynamic shared memory
    uint32_t *const table = reinterpret_cast<uint32_t *>(zsum_classes_words);
    unsigned long long *const cnt = zsum_classes_words + CLASS_TABLE_BYTES / 8, *const sum = cnt + cells;
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    class_table_fill(table, set, lane);
    for (uint32_t i = lane; i < 2 * cells; i += 64) cnt[i] = 0;
    __syncthreads();
    if (blockIdx.x < total_steps) {
        Col2<COL_U8> lanes{};
        lanes.off_lo = 4 * lane;
        col2_lanes<COL_U8>(lanes, lane);
        PipeRegs<TILES, COL_U8> A, B;
        SegCursor<COL> ca = {0, 0, 0, nullptr, {}, true, {}}, cb;
        uint64_t u = blockIdx.x;
        seg_seek<TILES, COL>(ca, segs, nseg, u, lane);
        pipe_load<TILES, COL_U8>(A, ca.base, u - ca.begin, lane, col2_of(lanes, ca.col));
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) seg_seek<TILES, COL>(cb, segs, nseg, u1, lane);
            pipe_load<TILES, COL_U8>(B, cb.base, (u1 < total_steps ? u1 : u) - cb.begin, lane, col2_of(lanes, cb.col));  // clamped at the tail: an L2 hit
            pipe_wait<LOADS>(A);
            if (!ca.empty) zsum_classes_eval<TILES>(A, ca, lanes, table, nx, cnt, sum, lane);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES, COL>(ca, segs, nseg, u2, lane);
            pipe_load<TILES, COL_U8>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane, col2_of(lanes, ca.col));
            pipe_wait<LOADS>(B);
            if (!cb.empty) zsum_classes_eval<TILES>(B, cb, lanes, table, nx, cnt, sum, lane);
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<0>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<0>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevRasterClassSegment &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const uint8_t *cls = g.cls;
        const RasterCol c = {g.lo[0], g.lo[1], g.cw[0], g.cw[1], g.magic[0], g.magic[1]};
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {  // (whole waves: the slot's masks are the wave's)
            bool pass = false;
            int x = 0, y = 0, z = 0;
            if (p < n) {
                const int *q = q0 + 3 * p;
                x = q[0], y = q[1], z = q[2];
                pass = ((uint32_t)(x - g.lo[0]) <= g.width[0]) & ((uint32_t)(y - g.lo[1]) <= g.width[1]) & ((uint32_t)(z - g.lo[2]) <= g.width[2]) &
                       (class_in_set(table, cls[p]) != 0);
            }
            zsum_classes_fold(cnt, sum, __ballot(pass), cell_of(x, y, c, nx), z, lane);
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < 2 * cells; i += 64) partials[(uint64_t)i * gridDim.x + blockIdx.x] = cnt[i];
}

}  // namespace

extern "C" int pcq_scan_dev_zsum_raster_batch_classes(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                                      size_t nsegments, uint32_t nx, uint32_t ny, const uint32_t class_set[8],
                                                      uint64_t *device_count, int64_t *device_zsum, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || (!cell_xy && nsegments) || !class_set || !device_count || !device_zsum)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_zsum_raster_batch_classes: null argument");
    if (nx == 0 || ny == 0 || (uint64_t)nx * ny > PCQ_ZSUM_CELLS_MAX)
        return pcq_fail(PCQ_ERR_ARG, "zsum_raster_batch_classes: %u x %u cells (1 .. %d in all)", nx, ny, PCQ_ZSUM_CELLS_MAX);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t cells = nx * ny;
    const size_t lds = CLASS_TABLE_BYTES + 2 * cells * sizeof(uint64_t);
    int lab_waves = 0;
#ifdef PCQ_LAB  // (tools/resident_zsum_classes_rate.py sweeps it)
    lab_waves = ctx->zsum_classes_waves_per_cu;
#endif
    const int waves = raster_waves_per_cu(ZSUM_CLASSES_WAVES_PER_CU, lds, lab_waves);
    ClassSet set;
    uint32_t any = 0;
    for (int w = 0; w < 8; w++) any |= (set.w[w] = class_set[w]);
    K1Batch b = {"zsum_raster_batch_classes", PCQ_SEGMENTS_RASTER_CLASSES, waves, 2 * (int)cells, 2 * (int)cells, /*null_refused=*/true};
    b.checks_only = !any;  // the empty set: every check of the table, then no upload, no launch, the words as they were
    return k1_batch_launch<DevRasterClassSegment>(
        ctx, b, cols, nsegments, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevRasterClassSegment &g, size_t i) { return raster_segment_fill(b.prefix, g, preds[i], cols[i], cell_xy + 2 * i, nx, ny, i); },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL((k_bounds_zsum_classes_pipe<K1_TILES>), dim3(g), dim3(64), lds, s,
                               reinterpret_cast<const DevRasterClassSegment *>(ctx->d_segments), (int)nsegments, steps, nx, cells, set, ctx->d_partials);
            return (int)PCQ_OK;
        },
        [&](int g) { return pcq_launch_finish_zsum(ctx, (int)cells, g, device_count, device_zsum, s); });
}
