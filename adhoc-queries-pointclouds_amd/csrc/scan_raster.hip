// scan_raster.hip — the density raster of a box: "where in this box are the points?" asked of many resident LAST files in ONE
// pass (pcq_scan_dev_raster_batch).
//
// The box count (scan_tiles.h: k_bounds_count_batch_pipe<2>) answers one cell per read of the 12 B/point, the multi-box count
// eight.  k_bounds_raster_pipe<TILES, WAVE> runs the box count's software pipeline (pipe_scan of scan_tiles.h: one wave per workgroup,
// TILES tiles per step, two register sets, 2 x 3 loads per set behind the counted s_waitcnt, steps numbered across segments, the
// cursor refreshed through SGPRs at a seek — COL_RASTER: the origin, the cell widths and their magics travel like the box — the
// clamped tail prefetch) and the rasters' leftover loop (raster_leftovers of raster_cells.h), and, instead of popcounting the start
// bits, brings the x and y of every passing point into one lane, divides both by the segment's cell widths and adds 1 to the cell's
// word of a raster in LDS.  The tile is this file's own (tile_raster: one value moves across lanes, not the two of the z-carrying tiles, and
// raster_cells.h has what a helper did to it):
//
//   values     in load k lane l starts one point among j = 0..2, at j0 = (3 - (k + l) % 3) % 3: x = v[k][j0], y = v[k][j0 + 1],
//              both its own; the verdict is bit l of s012 (tile_count_regs).  Where j0 == 0 a second point starts at j = 3: x =
//              v[k][3], y = the NEXT lane's v[k][0] — one cross-lane move per load (DPP wave_shl:1); for lane 63 of load 0
//              it is lane 0's v[1][0] (v_readlane), point 85 of the tile, the only one whose x and y sit in different loads
//              (lane 63 starts no second point in loads 1 and 2).  Its verdict is bit l of t3 & start_lanes(k + 3);
//   division   cx = (x - lo_x) / cw_x, cy = (y - lo_y) / cw_y, exact u32 floor divisions by multiply-high and one fix-up
//              (raster_div.h).  A passing point has x >= lo_x, so the u32 difference is the true one, and the entry's checks bound
//              its quotient by nx (ny): the cell cy * nx + cx lies inside the raster.  What a point that fails the box computes
//              is never used as an address;
//   raster     nx * ny u32 words of DYNAMIC shared memory, private to the wave (a small raster does not cost occupancy), zeroed
//              at start; a tile none of whose points passes is skipped before its divisions, and the six slots of a tile (per
//              load the 64 first points and the up to 22 second ones) are straight-line code.  Scanner order is spatially
//              coherent, so the passing lanes of a slot usually share a cell.  Two forms of the add: every passing lane adds 1
//              (ds_add_u32), or — WAVE — when all passing lanes of a slot share a cell ONE lane adds their popcount (one
//              v_readlane, one compare, no branch).  RASTER_WAVE_ADD below has the measurement and what ships.
//
// At exit the wave writes its words as u64 to partials[cell * gridDim.x + blockIdx.x]; k_finish_counts (scan_count_multi.hip)
// folds slice `cell` into device_raster[cell].
//
// A u32 word cannot overflow.  The grid g is min(CUs x workgroups per CU, steps + segments) and the steps are dealt round robin,
// so a wave bins at most ceil(steps / g) steps of 512 points and the leftovers (< 512 points each) of ceil(segments / g) segments:
// less than (points + 512 x segments) / g + 1024, and a word grows by points binned whether they arrive one by one or as a
// popcount.  With the smallest full grid (one workgroup per CU: 256 on the MI355X) that reaches 2^32 only above 10^12 points, or
// segments x 512, in all, and HBM (288 GB) holds 2.4 x 10^10 points at 12 B/point; with the grid capped at steps + segments every
// wave has one step and one segment's leftovers at most.
#include "pcq_internal.h"
#include "raster_cells.h"
#include "raster_div.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU: the smaller of this constant and what a CU's LDS holds at the launch's raster size
// (RASTER_LDS_PER_CU / (4 nx ny): 5 at PCQ_RASTER_CELLS_MAX, 40 at 32 x 32), rounded down to a multiple of four from four on
// (raster_waves_per_cu of raster_cells.h): the
// steps are dealt out evenly, the pass waits for instruction latency rather than for HBM, and a fifth wave makes one SIMD of a CU
// carry two (5 per CU is slower than 4, 10 slower than 8).  DESIGN.md §4 "Where in this box are the points" has the sweep
// (profiles/raster_rate_sweep.log, option raster_waves_per_cu of the lab library).
constexpr int RASTER_WAVES_PER_CU = 16;
// The form of the LDS add that ships: the wave-level shortcut (true) or the plain per-lane ds_add_u32 (false).  Measured (16 files x
// 163 M points, every point inside the box, the best grid of each, ms, generator order / scan-strip order): 8 x 8 cells: plain 5.2 /
// 8.4, shortcut 5.7 / 5.7; 64 x 64: plain 6.6 / 8.8, shortcut 8.5 / 8.7; 128 x 64: plain 9.3 / 9.3, shortcut 13.2 / 13.2.  The
// shortcut pays only where all 64 lanes hit one of very few cells AND many waves hide its scalar chain (v_readlane, ballot, two
// selects per slot); at the one or two waves per SIMD that a large raster's LDS allows it costs more than the same-address adds it
// saves.  So the plain add ships; the shortcut is instantiated in libpcq_lab.so only (option raster_add), for the comparison in
// profiles/raster_rate_sweep.log.
constexpr bool RASTER_WAVE_ADD = false;

// One slot: the points of the lanes in `pass` (uniform) into their cells, without a branch.  WAVE: when every passing lane has the
// cell of the first one, that lane alone adds their number; a slot without a passing lane has no first lane and adds nothing.
// (A function, adapted by a lambda where raster_leftovers wants a fold: as a functor that holds `ras`, like the z folds, the kernel came out of the
// compiler with 79 VGPRs for 80 and 1407 instructions for 1427 in the pipeline, which tools/count_kernels_asm_compare.py does not
// pass as the same kernel.)
template <bool WAVE>
__device__ __forceinline__ void raster_add(uint32_t *ras, uint64_t pass, uint32_t cell, int lane) {
    bool add = (pass >> lane) & 1ull;
    uint32_t by = 1u;
    if constexpr (WAVE) {
        const int first = __ffsll((unsigned long long)pass) - 1;  // (-1: no lane; v_readlane then reads lane 63, whose cell nobody uses)
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cell, first & 63);
        const bool same = (pass & ~__ballot(cell == c0)) == 0;  // (uniform)
        add = same ? lane == first : add;
        by = same ? (uint32_t)__popcll(pass) : 1u;
    }
    if (add) atomicAdd(&ras[cell], by);  // (result unused: ds_add_u32, exec-masked)
}

// One tile in registers: every passing point into the raster.  A tile none of whose points passes is skipped; otherwise the six
// slots are straight-line code, so that their divisions overlap.
template <bool WAVE>
__device__ __forceinline__ void tile_raster(const v4i (&v)[3], const LaneBox &lb, const RasterCol &c, uint32_t nx, uint32_t *ras, int lane) {
    uint64_t t[3][4], s012[3], s3[3];
    tile_start_masks(v, lb, t);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s012[k] = (t[k][0] & start_lanes(k)) | (t[k][1] & start_lanes(k + 1)) | (t[k][2] & start_lanes(k + 2));
        s3[k] = t[k][3] & start_lanes(k + 3);
    }
    if ((s012[0] | s012[1] | s012[2] | s3[0] | s3[1] | s3[2]) == 0) return;
    uint32_t ca[3], cb[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const bool j0_0 = (start_lanes(k) >> lane) & 1ull, j0_1 = (start_lanes(k + 1) >> lane) & 1ull;
        const int x = j0_0 ? v[k][0] : (j0_1 ? v[k][1] : v[k][2]);
        const int y = j0_0 ? v[k][1] : (j0_1 ? v[k][2] : v[k][3]);
        ca[k] = cell_of(x, y, c, nx);
        cb[k] = cell_of(v[k][3], next_lane(v[k][0], k == 0 ? __builtin_amdgcn_readlane(v[1][0], 0) : 0), c, nx);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        raster_add<WAVE>(ras, s012[k], ca[k], lane);
        raster_add<WAVE>(ras, s3[k], cb[k], lane);
    }
}

template <int TILES, bool WAVE>
__global__ __launch_bounds__(64) void k_bounds_raster_pipe(const DevRasterSegment *__restrict__ segs, int nseg, uint64_t total_steps, uint32_t nx,
                                                          uint32_t cells, uint64_t *__restrict__ partials) {
    constexpr int COL = COL_RASTER;
    extern __shared__ uint32_t ras[];  // `cells` words: the launch's dynamic shared memory
    const int lane = threadIdx.x;
    for (uint32_t i = lane; i < cells; i += 64) ras[i] = 0;
    __syncthreads();
    pipe_scan<TILES, COL>(segs, nseg, total_steps, lane, [&](const PipeRegs<TILES> &P, const SegCursor<COL> &c, const Col2<COL_NONE> &) {
#pragma unroll
        for (int t = 0; t < TILES; t++) tile_raster<WAVE>(P.r[t], c.lb, c.col, nx, ras, lane);
    });
    raster_leftovers<TILES>(segs, nseg, nx, lane, BoxOnly{}, [&](uint64_t pass, uint32_t cell, int, int l) { raster_add<WAVE>(ras, pass, cell, l); });
    __syncthreads();
    for (uint32_t i = lane; i < cells; i += 64) partials[(uint64_t)i * gridDim.x + blockIdx.x] = ras[i];
}

template <bool WAVE>
void launch_raster(pcq_ctx *ctx, unsigned g, int nsegments, uint64_t steps, uint32_t nx, uint32_t cells, hipStream_t s) {
    hipLaunchKernelGGL((k_bounds_raster_pipe<K1_TILES, WAVE>), dim3(g), dim3(64), cells * sizeof(uint32_t), s,
                       reinterpret_cast<const DevRasterSegment *>(ctx->d_segments), nsegments, steps, nx, cells, ctx->d_partials);
}

}  // namespace

extern "C" int pcq_scan_dev_raster_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, const uint32_t *cell_xy,
                                         size_t nsegments, uint32_t nx, uint32_t ny, uint64_t *device_raster, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || (!cell_xy && nsegments) || !device_raster)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_raster_batch: null argument");
    if (nx == 0 || ny == 0 || (uint64_t)nx * ny > PCQ_RASTER_CELLS_MAX)
        return pcq_fail(PCQ_ERR_ARG, "raster_batch: %u x %u cells (1 .. %d in all)", nx, ny, PCQ_RASTER_CELLS_MAX);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const uint32_t cells = nx * ny;
    int lab_waves = 0;
#ifdef PCQ_LAB  // (tools/resident_raster_rate.py sweeps both)
    lab_waves = ctx->raster_waves_per_cu;
    const bool other_add = ctx->raster_add && (ctx->raster_add == 2) != RASTER_WAVE_ADD;
#endif
    const int waves = raster_waves_per_cu(RASTER_WAVES_PER_CU, cells * sizeof(uint32_t), lab_waves);
    const K1Batch b = {"raster_batch", PCQ_SEGMENTS_RASTER, waves, (int)cells, (int)cells, /*null_refused=*/true};
    return k1_batch_launch<DevRasterSegment>(
        ctx, b, cols, nsegments, device_raster, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevRasterSegment &g, size_t i) { return raster_segment_fill(b.prefix, g, preds[i], cols[i], cell_xy + 2 * i, nx, ny, i); },
        [&](unsigned g, uint64_t steps) {
#ifdef PCQ_LAB
            if (other_add) launch_raster<!RASTER_WAVE_ADD>(ctx, g, (int)nsegments, steps, nx, cells, s);
            else
#endif
                launch_raster<RASTER_WAVE_ADD>(ctx, g, (int)nsegments, steps, nx, cells, s);
            return (int)PCQ_OK;
        });
}
