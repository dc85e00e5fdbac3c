// scan_time_hist.hip — the time histogram of a box: "when was this box scanned?" asked of many resident LAST files in ONE pass
// (pcq_scan_dev_time_hist_batch).
//
// The box AND time count (scan_tiles.h: k_bounds_count_batch_pipe<2, GpsTimes>) tests every point's GPS time against one range,
// so a points-per-time-slice breakdown costs one read of the same 20 B/point per slice.  k_bounds_time_hist_pipe<TILES> keeps the
// shape of that kernel — one wave per workgroup, TILES tiles per step, two register sets, 2 x (3 + 2) loads per set behind the
// counted s_waitcnt, steps numbered across segments, the cursor refreshed through SGPRs at a seek (seg_seek<TILES, COL_F64>; the
// segment's t0 / t1 are not used), the clamped tail prefetch — and, instead of popcounting, finds the bin of every time and
// brings the box verdict of its point to the lane that holds the time:
//
//   edges         the caller's nbins + 1 edges e[0] <= ... <= e[nbins] are the same for every segment: they travel behind the
//                 segment table (TimeHistTrailer; the table's upload is skipped only when ALL its bytes equal the ones in
//                 HBM, the edges among them) and are copied into LDS at kernel start.  e[0] and e[nbins] stay in SGPRs; the
//                 interior edges e[1 .. nbins) fill slots 0 .. nbins - 2 of a table of P = 2^L >= nbins slots, +inf behind them.
//   bins          bin b is [e[b], e[b + 1]) under IEEE compares (t_in, scan_tiles.h).  A time t has a bin when e[0] <= t and
//                 t < e[nbins]; then #{i : e[i] <= t} - 1 = #{i in 1 .. nbins - 1 : e[i] <= t}, which a branch-free upper-bound
//                 search over the LDS table finds in L wave-uniform steps (slot P - 1 is never read).  Only compares decide:
//                 NaN fails e[0] <= t; t = +inf fails t < e[nbins] whatever the padding made of its search; an edge equal to
//                 its neighbour is passed by the same compare as the neighbour, so a bin with equal edges stays empty; -0.0 and
//                 0.0 compare equal.  The eight searches of a step (four times per lane and tile) run side by side, so eight
//                 ds_read_b64 are in flight per level;
//   verdicts      after the loads lane l holds the times of points 2l, 2l + 1, 128 + 2l, 129 + 2l of the tile
//                 (Col2Regs<COL_F64>); tile_start_masks gives t[k][j]: bit `lane` is the verdict of the point that starts at
//                 dword (k, lane, j).  Point p starts at dword d = 3p: k = d >> 8, source lane (d >> 2) & 63, j = d & 3.  For
//                 slot i of a lane (p = 2l + i, then 128 + 2l + i - 2) k is one of two values (0 / 1 for the first two slots,
//                 1 / 2 for the others) and j one of two (0 / 2 on even / odd lanes for the even points, 3 / 1 for the odd
//                 ones): a select chain of three 64-bit selects per slot among four of the twelve masks, then one 64-bit shift
//                 by a per-lane amount.  (The alternatives — the twelve masks through LDS with a per-lane 64-bit read, and the
//                 bin brought to the start lane with ds_bpermute — are in DESIGN.md §4.);
//   histogram     PCQ_TIME_BINS_MAX u32 bins in LDS, private to the wave: one ds_add_u32 per passing point that has a bin.
//
// At exit the wave writes bins 0 .. nbins - 1 as u64 to partials[b * gridDim.x + blockIdx.x]; k_finish_counts
// (scan_count_multi.hip) folds slice b into device_hist[b].
//
// A u32 bin cannot overflow.  The grid g is min(CUs x TIME_HIST_WAVES_PER_CU, steps + segments) and the steps are dealt round
// robin, so a wave bins at most ceil(steps / g) steps of 512 points and the leftovers (< 512 points each) of ceil(segments / g)
// segments: less than (points + 512 x segments) / g + 1024.  With the full grid (12 x 256 CUs = 3072 workgroups on the MI355X) that
// reaches 2^32 only above 10^13 points, or segments x 512, in all, and HBM (288 GB) holds 1.5 x 10^10 points at 20 B/point;
// with the grid capped at steps + segments every wave has one step and one segment's leftovers at most.
//
// LDS per wave: 8 KB of edges + 4 KB of bins = 12 KB, so 13 workgroups fit a CU's 160 KB: PCQ_TIME_BINS_MAX = 1024 does not
// limit residency below what the registers allow (12).
#include <cmath>
#include <cstring>
#include <vector>

#include "pcq_internal.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU.  Unlike the class histogram this kernel is not bound by HBM: per point it makes up to ten
// dependent LDS reads and one LDS add, and more waves hide them.  16 files x 163 M points, every point inside the box, by workgroups
// per CU, 8 bins / 1024 bins with acquisition-ordered times / 1024 bins with shuffled times: 3: 12.0 / 17.9 / 16.0 ms, 4: 11.4 /
// 15.9 / 11.4, 5: 12.0 / 16.0 / 11.4, 6: 10.6 / 14.2 / 10.0, 8: 10.0 / 12.4 / 8.8, 10: 9.8 / 12.2 / 9.5, 12: 9.6 / 11.5 / 9.0,
// 16: 9.5 / 11.6 / 9.1 (profiles/time_hist_rate_sweep.log).  12 is what a CU holds (134 VGPRs: three waves per SIMD; 12 KB of LDS
// each: thirteen per CU), so 16 is 12 resident and a second round; one box AND time pass with K1's 3 takes 7.8 ms on the same data.
constexpr int TIME_HIST_WAVES_PER_CU = 12;

// What travels behind the segment table: nbins in front of the edges, so that two tables of one launch shape (segments, kind)
// that differ in nbins differ inside the bytes both uploaded.
struct TimeHistTrailer {
    uint64_t nbins;
    // double e[nbins + 1] follows
};

// What a lane needs to find the verdicts of its four points (computed once).
struct TimeLanes {
    uint32_t src[4];  // the lane whose bit of t[k][j] is the verdict of the point in slot i
    bool khi[4];      // that point starts in the later of the slot's two loads
    bool odd;         // j is the second of the slot's two values
};
// slot i: the earlier load, and j on even / odd lanes
__device__ constexpr int SLOT_K[4] = {0, 0, 1, 1};
__device__ constexpr int SLOT_JE[4] = {0, 3, 0, 3};
__device__ constexpr int SLOT_JO[4] = {2, 1, 2, 1};
__device__ __forceinline__ TimeLanes time_lanes(int lane) {
    TimeLanes h;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t p = (i < 2 ? 0u : 128u) + 2u * (uint32_t)lane + (uint32_t)(i & 1);
        const uint32_t d = 3u * p;  // first dword of the point
        h.src[i] = (d >> 2) & 63u;
        h.khi[i] = (d >> 8) == (uint32_t)SLOT_K[i] + 1u;
    }
    h.odd = (lane & 1) != 0;  // d & 3 = (6 lane + 3 (i & 1)) & 3
    return h;
}

// The launch's edges as a wave sees them.
struct EdgeTable {
    const double *tab;  // LDS: the interior edges, +inf behind them
    uint32_t half;      // P / 2: the first step of the search (0: one bin, no search)
    double e0, eN;      // the first and the last edge (uniform)
};

// The bins of N times side by side: pos[i] = #{interior edges <= t[i]}.
template <int N>
__device__ __forceinline__ void time_bins(const EdgeTable &E, const double (&t)[N], uint32_t (&pos)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) pos[i] = 0;
    for (uint32_t step = E.half; step; step >>= 1) {
        double e[N];  // (all N reads issued before the first compare: the searches are independent)
#pragma unroll
        for (int i = 0; i < N; i++) e[i] = E.tab[pos[i] + step - 1];
#pragma unroll
        for (int i = 0; i < N; i++) pos[i] += e[i] <= t[i] ? step : 0u;
    }
}
__device__ __forceinline__ bool has_bin(const EdgeTable &E, double t) { return (t >= E.e0) & (t < E.eN); }  // (NaN: no bin)

// One step in registers: the 4 x TILES (verdict, time) pairs of every lane into the histogram.
template <int TILES>
__device__ __forceinline__ void hist_eval(const PipeRegs<TILES, COL_F64> &P, const LaneBox &lb, const TimeLanes &hl, const EdgeTable &E,
                                          uint32_t *hist) {
    double tm[4 * TILES];
    uint32_t pos[4 * TILES];
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        const Col2Regs<COL_F64> &c = P.c[t];
        tm[4 * t + 0] = time_of(c.a[0], c.a[1]);
        tm[4 * t + 1] = time_of(c.a[2], c.a[3]);
        tm[4 * t + 2] = time_of(c.b[0], c.b[1]);
        tm[4 * t + 3] = time_of(c.b[2], c.b[3]);
    }
    time_bins<4 * TILES>(E, tm, pos);
#pragma unroll
    for (int t = 0; t < TILES; t++) {
        uint64_t m[3][4];
        tile_start_masks(P.r[t], lb, m);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = SLOT_K[i], je = SLOT_JE[i], jo = SLOT_JO[i];
            const uint64_t lo = hl.odd ? m[k][jo] : m[k][je], hi = hl.odd ? m[k + 1][jo] : m[k + 1][je];
            const uint64_t v = hl.khi[i] ? hi : lo;
            if (((v >> hl.src[i]) & 1ull) && has_bin(E, tm[4 * t + i])) atomicAdd(&hist[pos[4 * t + i]], 1u);  // (result unused: ds_add_u32)
        }
    }
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_time_hist_pipe(const DevBoundsTimeSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                             const double *__restrict__ edges, int nbins, uint32_t half,
                                                             uint64_t *__restrict__ partials) {
    constexpr int COL = COL_F64;
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    __shared__ double tab[PCQ_TIME_BINS_MAX];
    __shared__ uint32_t hist[PCQ_TIME_BINS_MAX];
    const int lane = threadIdx.x;
    const uint32_t slots = half ? 2 * half : 1;  // P (<= PCQ_TIME_BINS_MAX: the entry has checked nbins)
    for (uint32_t i = lane; i < slots; i += 64) {
        tab[i] = i + 1 < (uint32_t)nbins ? edges[i + 1] : __longlong_as_double(0x7ff0000000000000ll);
        hist[i] = 0;
    }
    const EdgeTable E = {tab, half, edges[0], edges[nbins]};
    __syncthreads();
    const TimeLanes hl = time_lanes(lane);
    pipe_scan<TILES, COL>(segs, nseg, total_steps, lane, [&](const PipeRegs<TILES, COL> &P, const SegCursor<COL> &c, const Col2<COL> &) {
        hist_eval<TILES>(P, c.lb, hl, E, hist);
    });
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevBoundsTimeSegment &g = segs[i];
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const double *tq = reinterpret_cast<const double *>(g.times);
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {  // (whole waves: the search's steps are uniform)
            bool pass = false;
            double tm[1] = {0.0};
            if (p < n) {
                const int *q = q0 + 3 * p;
                pass = ((uint32_t)(q[0] - g.lo[0]) <= g.width[0]) & ((uint32_t)(q[1] - g.lo[1]) <= g.width[1]) &
                       ((uint32_t)(q[2] - g.lo[2]) <= g.width[2]);
                tm[0] = tq[p];
            }
            uint32_t pos[1];
            time_bins<1>(E, tm, pos);
            if (pass && has_bin(E, tm[0])) atomicAdd(&hist[pos[0]], 1u);
        }
    }
    __syncthreads();
    for (int b = lane; b < nbins; b += 64) partials[(uint64_t)b * gridDim.x + blockIdx.x] = hist[b];
}

}  // namespace

extern "C" int pcq_scan_dev_time_hist_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                            const double *edges, size_t nbins, uint64_t *device_hist, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !edges || !device_hist)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_time_hist_batch: null argument");
    if (nbins == 0 || nbins > PCQ_TIME_BINS_MAX) return pcq_fail(PCQ_ERR_ARG, "time_hist_batch: %zu bins (1 .. %d)", nbins, PCQ_TIME_BINS_MAX);
    for (size_t i = 0; i <= nbins; i++) {
        if (std::isnan(edges[i])) return pcq_fail(PCQ_ERR_ARG, "time_hist_batch: edge %zu is NaN", i);
        if (i && edges[i - 1] > edges[i]) return pcq_fail(PCQ_ERR_ARG, "time_hist_batch: edge %zu is below edge %zu", i, i - 1);
    }
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int waves = TIME_HIST_WAVES_PER_CU;
#ifdef PCQ_LAB  // (tools/resident_time_hist_rate.py sweeps it)
    if (ctx->time_hist_waves_per_cu) waves = ctx->time_hist_waves_per_cu;
#endif
    std::vector<uint64_t> trailer(1 + nbins + 1);  // TimeHistTrailer, then the edges
    trailer[0] = (uint64_t)nbins;
    memcpy(&trailer[1], edges, (nbins + 1) * sizeof(double));
    uint32_t slots = 1;
    while (slots < nbins) slots <<= 1;
    const K1Batch b = {"time_hist_batch", PCQ_SEGMENTS_TIME_HIST, waves, (int)nbins, (int)nbins, /*null_refused=*/true,
                       trailer.data(), trailer.size() * sizeof(uint64_t)};
    return k1_batch_launch<DevBoundsTimeSegment>(
        ctx, b, cols, nsegments, device_hist, s, [&](size_t i) { return admit_bounds_only(b.prefix, preds[i], i); },
        [&](DevBoundsTimeSegment &g, size_t i) {
            if (cols[i].cls_stride != 8 || ((uintptr_t)cols[i].cls & 7) != 0 || (!cols[i].cls && cols[i].n))
                return pcq_fail(PCQ_ERR_ARG, "time_hist_batch: LAST time blocks only (stride 8, 8-byte aligned), segment %zu", i);
            DevPred dp;
            const int prc = pcq_make_dev_pred(&preds[i], &dp);
            if (prc) return prc;
            g.times = (const uint8_t *)cols[i].cls;
            seg_box(g, dp);  // (t0, t1 stay zero: the edges are the launch's, not the segment's)
            return (int)PCQ_OK;
        },
        [&](unsigned g, uint64_t steps) {
            const uint8_t *behind = reinterpret_cast<const uint8_t *>(ctx->d_segments) + nsegments * sizeof(DevBoundsTimeSegment);
            const DevBoundsTimeSegment *segs = reinterpret_cast<const DevBoundsTimeSegment *>(ctx->d_segments);
            const double *e = reinterpret_cast<const double *>(behind + sizeof(TimeHistTrailer));
            hipLaunchKernelGGL((k_bounds_time_hist_pipe<K1_TILES>), dim3(g), dim3(64), 0, s, segs, (int)nsegments, steps, e, (int)nbins,
                               slots / 2, ctx->d_partials);
            return (int)PCQ_OK;
        });
}
