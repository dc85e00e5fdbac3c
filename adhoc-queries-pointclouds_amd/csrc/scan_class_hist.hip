// scan_class_hist.hip — the class histogram of a box: "what is in this box, by class?" asked of many resident LAST files in
// ONE pass (pcq_scan_dev_class_hist_batch).
//
// The box AND class count (scan_tiles.h: k_bounds_count_batch_pipe<2, ClassBytes>) compares every point's class byte with one
// value, so a per-class breakdown costs one read of the same 13 B/point per class, and the caller has to know the classes.
// k_bounds_class_hist_pipe<TILES, R> keeps the shape of that kernel — one wave per workgroup, TILES tiles per step, two register
// sets, 2 x (3 + 2) loads per set behind the counted s_waitcnt, steps numbered across segments, the cursor refreshed through
// SGPRs at a seek (seg_seek<TILES, COL_U8>; the segment's `pat` is not used), the clamped tail prefetch — and, instead of
// popcounting, brings the box verdict of every point to the lane that holds its class byte and bins the byte:
//
//   class bytes   after v_alignbit lane l holds the bytes of points 4l .. 4l + 3 of the tile (Col2Regs<COL_U8>);
//   verdicts      tile_start_masks gives t[k][j]: bit `lane` is the verdict of the point that starts at dword (k, lane, j).
//                 Point p = 4l + i starts at dword d = 12l + 3i: k = d >> 8, source lane (d >> 2) & 63, j = d & 3 = (0, 3, 2, 1)[i].
//                 So j is fixed per i, k is a per-lane select among three SGPR pairs, and the bit comes out with one 64-bit
//                 shift by a per-lane amount;
//   bins          a histogram of 256 u32 bins in LDS, private to the wave: one ds_add_u32 per point that passes (R interleaved
//                 copies of it were tried against same-bin contention and bought nothing: CLASS_HIST_COPIES below).
//
// At exit the wave writes its 256 bins as u64 to partials[c * gridDim.x + blockIdx.x]; k_finish_counts (scan_count_multi.hip)
// folds slice c into device_hist[c].
//
// A u32 bin cannot overflow.  The grid g is min(CUs x CLASS_HIST_WAVES_PER_CU, steps + segments) and the steps are dealt round
// robin, so a wave bins at most ceil(steps / g) steps of 512 points and the leftovers (< 512 points each) of ceil(segments / g)
// segments: less than (points + 512 x segments) / g + 1024.  With the full grid (4 x 256 CUs = 1024 workgroups on the MI355X) that
// reaches 2^32 only above 4 x 10^12 points, or segments x 512, in all, and HBM (288 GB) holds 2 x 10^10 points at 13 B/point;
// with the grid capped at steps + segments every wave has one step and one segment's leftovers at most.
#include "pcq_internal.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU.  The kernel does more per tile than K1 (MULTI_WAVES_PER_CU in scan_count_multi.hip has that case), but it stays
// bound by HBM: 16 files x 163 M points, every point inside the box, synth-doc classes, by workgroups per CU: 3: 5.41 ms, 4: 4.95,
// 5: 5.34, 6: 5.28, 8: 5.30, 12: 5.26, 16: 5.41 (profiles/class_hist_rate_sweep.log; 32 uniform classes alike).  4 is one wave on
// each SIMD of a CU; the box AND class count with K1's 3 takes 5.16 ms on the same data.
constexpr int CLASS_HIST_WAVES_PER_CU = 4;
// Copies of the histogram per wave (copy lane & (R - 1) of bin c at word c * R + copy), against lanes of a wave adding to one
// bin at the same time: 45 % of synth-doc's points are class 2.  Measured, it buys nothing: with 1, 4 and 8 copies every grid
// of the sweep above takes the same time within 0.15 ms on the skewed classes and on the uniform ones, and 16 copies lose 0.4 ms
// from 12 workgroups per CU on (16 KB of LDS per wave: 12 no longer fit a CU's 160 KB).  The same-bin adds of a wave are not what the pass waits for, so the
// plain per-lane add ships; the other values are instantiated in libpcq_lab.so only, for the sweep.
constexpr int CLASS_HIST_COPIES = 1;

// What a lane needs to find the verdicts of its four points (computed once).
struct HistLanes {
    uint32_t src[4];  // the lane whose bit of t[k][j] is the verdict of point 4 lane + i
    bool k1[4], k2[4];  // that point starts in load 1 / load 2 of the tile (else load 0)
};
__device__ __forceinline__ HistLanes hist_lanes(int lane) {
    HistLanes h;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t d = 12u * (uint32_t)lane + 3u * (uint32_t)i;  // first dword of point 4 lane + i
        h.src[i] = (d >> 2) & 63u;
        h.k1[i] = (d >> 8) == 1u;
        h.k2[i] = (d >> 8) == 2u;
    }
    return h;
}

template <int R>
__device__ __forceinline__ void hist_add(uint32_t *hist, uint32_t cls, int lane) {
    atomicAdd(&hist[cls * R + ((uint32_t)lane & (uint32_t)(R - 1))], 1u);  // (result unused: ds_add_u32)
}

// One tile in registers: the four (verdict, class byte) pairs of every lane into the histogram.
template <int R>
__device__ __forceinline__ void tile_hist(const v4i (&v)[3], const Col2Regs<COL_U8> &cr, const LaneBox &lb, uint32_t shift, const HistLanes &hl,
                                          uint32_t *hist, int lane) {
    uint64_t t[3][4];
    tile_start_masks(v, lb, t);
    const uint32_t bytes = __builtin_amdgcn_alignbit((uint32_t)cr.hi, (uint32_t)cr.lo, shift);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        constexpr int J[4] = {0, 3, 2, 1};
        const int j = J[i];
        const uint64_t m = hl.k2[i] ? t[2][j] : (hl.k1[i] ? t[1][j] : t[0][j]);
        if ((m >> hl.src[i]) & 1ull) hist_add<R>(hist, (bytes >> (8 * i)) & 0xffu, lane);
    }
}

template <int TILES, int R>
__device__ __forceinline__ void hist_eval(const PipeRegs<TILES, COL_U8> &P, const SegCursor<COL_U8> &c, const HistLanes &hl, uint32_t *hist,
                                          int lane) {
#pragma unroll
    for (int t = 0; t < TILES; t++) tile_hist<R>(P.r[t], P.c[t], c.lb, c.col.shift, hl, hist, lane);
}

template <int TILES, int R>
__global__ __launch_bounds__(64) void k_bounds_class_hist_pipe(const DevCombinedSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                              uint64_t *__restrict__ partials) {
    static_assert(R >= 1 && R <= 16 && (R & (R - 1)) == 0, "copies of the histogram: a power of two");
    constexpr int COL = COL_U8;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    __shared__ uint32_t hist[PCQ_CLASS_BINS * R];
    const int lane = threadIdx.x;
    for (int i = lane; i < PCQ_CLASS_BINS * R; i += 64) hist[i] = 0;
    __syncthreads();
    const HistLanes hl = hist_lanes(lane);
    pipe_scan<TILES, COL>(segs, nseg, total_steps, lane, [&](const PipeRegs<TILES, COL> &P, const SegCursor<COL> &c, const Col2<COL> &) {
        hist_eval<TILES, R>(P, c, hl, hist, lane);
    });
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevCombinedSegment &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < n; p += 64) {
            const int *q = q0 + 3 * p;
            const bool pass = ((uint32_t)(q[0] - g.lo[0]) <= g.width[0]) & ((uint32_t)(q[1] - g.lo[1]) <= g.width[1]) &
                              ((uint32_t)(q[2] - g.lo[2]) <= g.width[2]);
            if (pass) hist_add<R>(hist, g.cls[p], lane);
        }
    }
    __syncthreads();
    for (int c = lane; c < PCQ_CLASS_BINS; c += 64) {
        uint64_t sum = 0;
#pragma unroll
        for (int r = 0; r < R; r++) sum += hist[c * R + r];
        partials[(uint64_t)c * gridDim.x + blockIdx.x] = sum;
    }
}

template <int R>
void launch_hist(pcq_ctx *ctx, unsigned g, int nsegments, uint64_t steps, hipStream_t s) {
    hipLaunchKernelGGL((k_bounds_class_hist_pipe<K1_TILES, R>), dim3(g), dim3(64), 0, s,
                       reinterpret_cast<const DevCombinedSegment *>(ctx->d_segments), nsegments, steps, ctx->d_partials);
}

}  // namespace

extern "C" int pcq_scan_dev_class_hist_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                             uint64_t *device_hist, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_hist)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_class_hist_batch: null argument");
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int waves = CLASS_HIST_WAVES_PER_CU;
#ifdef PCQ_LAB  // (tools/resident_class_hist_rate.py sweeps both)
    if (ctx->class_hist_waves_per_cu) waves = ctx->class_hist_waves_per_cu;
    const int copies = ctx->class_hist_copies ? ctx->class_hist_copies : CLASS_HIST_COPIES;
#endif
    const K1Batch b = {"class_hist_batch", PCQ_SEGMENTS_CLASS_HIST, waves, PCQ_CLASS_BINS, PCQ_CLASS_BINS, /*null_refused=*/true};
    return k1_batch_launch<DevCombinedSegment>(
        ctx, b, cols, nsegments, device_hist, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevCombinedSegment &g, size_t i) {
            if (cols[i].cls_stride != 1 || (!cols[i].cls && cols[i].n))
                return pcq_fail(PCQ_ERR_ARG, "class_hist_batch: LAST classification blocks only (stride 1), segment %zu", i);
            DevPred dp;
            const int prc = pcq_make_dev_pred(&preds[i], &dp);
            if (prc) return prc;
            g.cls = (const uint8_t *)cols[i].cls;
            seg_box(g, dp);
            return (int)PCQ_OK;
        },
        [&](unsigned g, uint64_t steps) {
#ifdef PCQ_LAB
            switch (copies) {
            case 1: launch_hist<1>(ctx, g, (int)nsegments, steps, s); break;
            case 2: launch_hist<2>(ctx, g, (int)nsegments, steps, s); break;
            case 4: launch_hist<4>(ctx, g, (int)nsegments, steps, s); break;
            case 8: launch_hist<8>(ctx, g, (int)nsegments, steps, s); break;
            case 16: launch_hist<16>(ctx, g, (int)nsegments, steps, s); break;
            default: return pcq_fail(PCQ_ERR_ARG, "class_hist_batch: option class_hist_copies %d (1, 2, 4, 8 or 16)", copies);
            }
#else
            launch_hist<CLASS_HIST_COPIES>(ctx, g, (int)nsegments, steps, s);
#endif
            return (int)PCQ_OK;
        });
}
