// scan_zmoments.hip — the height-spread raster of a box: "how rough is this box, cell by cell?" asked of many resident LAST files in
// ONE pass (pcq_scan_dev_zmoments_raster_batch): the number of points of every cell of a 2-D raster over x and y, the sum of their z
// and the sum of their z squared, the words a mean and a standard deviation rest on.
//
// k_bounds_zmoments_pipe<TILES> is the mean-height raster's kernel (scan_zsum.hip: k_bounds_zsum_pipe<TILES>) up to the LDS operation
// — one wave per workgroup, TILES tiles per step, two register sets, 2 x 3 loads per set behind the counted s_waitcnt, the cursor
// SegCursor<COL_RASTER> over the same DevRasterSegment table, the clamped tail prefetch, skipped empty segments and skipped tiles
// without a passing point, the cell by two exact divisions (raster_cells.h, raster_div.h), the z of every passing point brought to
// the lane that holds its cell (next_lane, v_readlane behind lane 63: see scan_zrange.hip for which dword is whose), the six
// straight-line slots and the one-lane-per-point leftover loop over whole waves.  What differs:
//
//   raster     4 x nx * ny u64 words of DYNAMIC shared memory, private to the wave: the counts, the sums, the sums of z^2 mod 2^32,
//              then the sums of z^2 >> 32, all zero at entry.  z is an i32, so z^2 <= 2^62 is formed in 64 bits and its two dwords
//              go into a u64 word each: neither word can wrap while a launch reads fewer than 2^32 points, and sum z^2 = hi * 2^32 +
//              lo exactly.  Every passing lane does four 64-bit LDS adds on its cell, 1, (uint64_t)(int64_t)z and the two dwords,
//              results unused (ds_add_u64, exec-masked: profiles/zmoments_asm_compare.log has the disassembly's count of them and
//              that no compare-and-swap loop stands in: 100 of them, 84 VGPRs, no scratch).  No carry from the low word into the
//              high one is propagated in the kernel: that would need the low add's result back.
//
// At exit the wave writes four u64 per cell to partials[slice * gridDim.x + blockIdx.x]: slice `cell` the count, `cells + cell` the
// sum, `2 cells + cell` the low and `3 cells + cell` the high word; pcq_launch_finish_zmoments (scan_count_multi.hip: k_finish_counts
// per array) adds each quarter into its array, modulo 2^64.
// This kernel keeps its own text of the pipeline loop, the tile and the leftover loop.  On pipe_scan (scan_tiles.h), a tile shared
// with the height raster and raster_leftovers (raster_cells.h) it compiled to a kernel structurally equal to this one (equal VGPRs, occupancy,
// waits, loads, LDS operations and compares) that ran 0.76 % slower (9.530 against 9.458 ms, the parent's spread 0.030) at the largest raster, where
// the LDS leaves one wave per SIMD, and inside the parent's spread at 8 x 8 cells (profiles/raster_frame_rate.log): outside the rule
// of that change, so the copy stays.
#include "pcq_internal.h"
#include "raster_cells.h"
#include "raster_div.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU: the mean-height raster's rule with twice its LDS per cell — the smaller of this constant and what
// a CU's LDS holds at the launch's raster size (RASTER_LDS_PER_CU / (32 nx ny): 5 at PCQ_ZMOMENTS_CELLS_MAX, 80 at 8 x 8), rounded
// down to a multiple of four from four on, so that no SIMD of a CU carries a wave more than another.  Measured (16 files x 163 M
// points, every point inside the box, generator order, ms by workgroups per CU): 8 x 8 cells: 4: 13.8, 8: 13.7, 12: 13.7, 16: 13.6;
// 1024 cells: 4: 9.5, 5 (the LDS limit): 16.7.  The pass follows its LDS adds, four per point: 1.94 times the mean-height pass at
// 8 x 8, and 32.5 - 33.4 ms in scan-strip order, where all 64 lanes of a slot meet one word.  DESIGN.md §4 "How rough is this box"
// has the sweep (profiles/zmoments_rate_sweep.log, option zmoments_waves_per_cu of the lab library, which takes the value
// as given up to the LDS limit).
constexpr int ZMOMENTS_WAVES_PER_CU = 16;

// The four arrays of a wave's raster in its shared memory.
struct MomentWords {
    unsigned long long *cnt, *sum, *lo, *hi;
};

// One slot: a point and its z from the lanes in `pass` (uniform) into the four words of their cells.
__device__ __forceinline__ void zmoments_fold(const MomentWords &w, uint64_t pass, uint32_t cell, int z, int lane) {
    if ((pass >> lane) & 1ull) {
        const unsigned long long sq = (unsigned long long)((long long)z * (long long)z);  // (<= 2^62: INT32_MIN squared)
        atomicAdd(&w.cnt[cell], 1ull);  // (results unused: ds_add_u64, exec-masked)
        atomicAdd(&w.sum[cell], (unsigned long long)(long long)z);
        atomicAdd(&w.lo[cell], sq & 0xffffffffull);
        atomicAdd(&w.hi[cell], sq >> 32);
    }
}

// One tile in registers: every passing point into its cell's words.  A tile none of whose points passes is skipped; otherwise the
// six slots are straight-line code, so that their divisions overlap.
__device__ __forceinline__ void tile_zmoments(const v4i (&v)[3], const LaneBox &lb, const RasterCol &c, uint32_t nx, const MomentWords &w,
                                              int lane) {
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
        zmoments_fold(w, s012[k], ca[k], za[k], lane);
        zmoments_fold(w, s3[k], cb[k], zb[k], lane);
    }
}

template <int TILES>
__device__ __forceinline__ void zmoments_eval(const PipeRegs<TILES> &P, const SegCursor<COL_RASTER> &c, uint32_t nx, const MomentWords &w,
                                              int lane) {
#pragma unroll
    for (int t = 0; t < TILES; t++) tile_zmoments(P.r[t], c.lb, c.col, nx, w, lane);
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_zmoments_pipe(const DevRasterSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                            uint32_t nx, uint32_t cells, uint64_t *__restrict__ partials) {
    constexpr int COL = COL_RASTER;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    constexpr int LOADS = PipeRegs<TILES>::LOADS;           // per register set
    extern __shared__ unsigned long long zmoments_words[];  // 4 x `cells` words: the launch's dynamic shared memory
    const MomentWords w = {zmoments_words, zmoments_words + cells, zmoments_words + 2 * cells, zmoments_words + 3 * cells};
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    for (uint32_t i = lane; i < 4 * cells; i += 64) zmoments_words[i] = 0;
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
            if (!ca.empty) zmoments_eval<TILES>(A, ca, nx, w, lane);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES, COL>(ca, segs, nseg, u2, lane);
            pipe_load<TILES>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane);
            pipe_wait<LOADS>(B);
            if (!cb.empty) zmoments_eval<TILES>(B, cb, nx, w, lane);
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
            zmoments_fold(w, __ballot(pass), cell_of(x, y, c, nx), z, lane);
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < 4 * cells; i += 64) partials[(uint64_t)i * gridDim.x + blockIdx.x] = zmoments_words[i];
}

}  // namespace

extern "C" int pcq_scan_dev_zmoments_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                                  size_t nsegments, uint32_t nx, uint32_t ny, uint64_t *device_count, int64_t *device_zsum,
                                                  uint64_t *device_zsq_lo, uint64_t *device_zsq_hi, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || (!cell_xy && nsegments) || !device_count || !device_zsum || !device_zsq_lo ||
        !device_zsq_hi)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_zmoments_raster_batch: null argument");
    if (nx == 0 || ny == 0 || (uint64_t)nx * ny > PCQ_ZMOMENTS_CELLS_MAX)
        return pcq_fail(PCQ_ERR_ARG, "zmoments_raster_batch: %u x %u cells (1 .. %d in all)", nx, ny, PCQ_ZMOMENTS_CELLS_MAX);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t cells = nx * ny;
    const size_t lds = 4 * cells * sizeof(uint64_t);
    int lab_waves = 0;
#ifdef PCQ_LAB  // (tools/resident_zmoments_rate.py sweeps it)
    lab_waves = ctx->zmoments_waves_per_cu;
#endif
    const int waves = raster_waves_per_cu(ZMOMENTS_WAVES_PER_CU, lds, lab_waves);
    // (the density raster's table under its kind: the four kernels read it alike)
    const K1Batch b = {"zmoments_raster_batch", PCQ_SEGMENTS_RASTER, waves, 4 * (int)cells, 4 * (int)cells, /*null_refused=*/true};
    return k1_batch_launch<DevRasterSegment>(
        ctx, b, cols, nsegments, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevRasterSegment &g, size_t i) { return raster_segment_fill(b.prefix, g, preds[i], cols[i], cell_xy + 2 * i, nx, ny, i); },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL((k_bounds_zmoments_pipe<K1_TILES>), dim3(g), dim3(64), lds, s,
                               reinterpret_cast<const DevRasterSegment *>(ctx->d_segments), (int)nsegments, steps, nx, cells, ctx->d_partials);
            return (int)PCQ_OK;
        },
        [&](int g) { return pcq_launch_finish_zmoments(ctx, (int)cells, g, device_count, device_zsum, device_zsq_lo, device_zsq_hi, s); });
}
