// scan_count_multi.hip — the multi-box batched count: up to PCQ_MULTI_BOX_MAX boxes asked of many resident LAST positions
// blocks in ONE pass (pcq_scan_dev_count_batch_multi).
//
// The batched K1 (scan_tiles.h: k_bounds_count_batch_pipe) runs at the HBM rate and hides its per-tile work — 12 subtract /
// compare pairs and the SGPR mask algebra of tile_count_regs per 256 points — behind the wait for the next tiles.  A caller
// with Q boxes pays Q full reads of the same data.  k_bounds_count_multi_pipe<TILES, NQ> keeps the shape of that kernel (one
// wave per workgroup, TILES tiles per step, two register sets, counted s_waitcnt, steps numbered across segments, the clamped
// tail prefetch) and evaluates NQ boxes on every tile while it is in registers: Q reads become one.
//
// Per cursor (one per register set) the NQ rotated boxes of its segment and the segment's `live` mask; everything of a segment
// passes through SGPRs at a seek (seg_seek in scan_tiles.h has the reason).  A box whose live bit is clear — not asked of the
// segment, or empty — is skipped by a wave-uniform branch.  The wave's NQ totals go to partials[q * gridDim.x + blockIdx.x];
// k_finish_counts folds slice q into device_totals[q].
#include "pcq_internal.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// Workgroups (of one wave) per CU.  With NQ boxes per tile the kernel is bound by instruction issue, not by HBM, and K1's 3 per CU
// leave a SIMD's issue slots idle while its one wave waits: 16 files x 163 M points, NQ = 8, by workgroups per CU: 3: 24.9 ms, 4: 19.2,
// 6: 17.4, 8: 13.2, 12: 11.65, 16: 11.6, 24: 10.9 (profiles/multi_box_rate_sweep.log; NQ = 2 and 4 alike).  12 is what the 151 VGPRs of
// NQ = 8 allow to be resident at once (3 waves per SIMD); beyond it workgroups queue, for 6 % more at twice the grid.
constexpr int MULTI_WAVES_PER_CU = 12;

template <int NQ>
struct MultiCursor {
    int s;
    uint64_t begin, end;
    const v4i *base;
    uint32_t live;  // (uniform)
    LaneBox lb[NQ];
};

template <int TILES, int NQ>
__device__ __forceinline__ void multi_seek(MultiCursor<NQ> &c, const DevMultiSegment *__restrict__ segs, int nseg, uint64_t u, int lane) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= segs[c.s + 1].tile_begin) c.s++;
    const DevMultiSegment &g = segs[c.s];
    c.begin = g.tile_begin;
    c.end = c.begin + g.n / ((uint64_t)TILES * TILE_POINTS);
    c.base = reinterpret_cast<const v4i *>(g.xyz);
    uint32_t live = g.live;
    asm volatile("" : "+s"(live));
    c.live = live;
    // every box of the segment through SGPRs, as seg_seek does for its one box: a vector load here would be followed by an
    // s_waitcnt vmcnt(0) that drains the prefetched register set
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        int32_t lo[3];
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = g.lo[q][k];
            w[k] = g.width[q][k];
            asm volatile("" : "+s"(lo[k]), "+s"(w[k]));
        }
        c.lb[q] = rotate_box(lo, w, lane);
    }
}

template <int TILES, int NQ>
__device__ __forceinline__ void multi_eval(const PipeRegs<TILES> &R, const MultiCursor<NQ> &c, uint64_t (&total)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        if (!((c.live >> q) & 1u)) continue;  // wave-uniform
#pragma unroll
        for (int t = 0; t < TILES; t++) total[q] += tile_count_regs(R.r[t], c.lb[q]);
    }
}

template <int TILES, int NQ>
__global__ __launch_bounds__(64) void k_bounds_count_multi_pipe(const DevMultiSegment *__restrict__ segs, int nseg, uint64_t total_steps,
                                                               uint64_t *__restrict__ partials) {
    static_assert(NQ >= 2 && NQ <= PCQ_MULTI_BOX_MAX, "boxes per pass");
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    constexpr int LOADS = PipeRegs<TILES>::LOADS;  // per register set
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    uint64_t total[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) total[q] = 0;
    if (blockIdx.x < total_steps) {
        PipeRegs<TILES> A, B;
        MultiCursor<NQ> ca, cb;
        ca.s = 0, ca.begin = 0, ca.end = 0, ca.base = nullptr, ca.live = 0;
#pragma unroll
        for (int q = 0; q < NQ; q++) ca.lb[q] = LaneBox{};
        uint64_t u = blockIdx.x;
        multi_seek<TILES, NQ>(ca, segs, nseg, u, lane);
        pipe_load<TILES>(A, ca.base, u - ca.begin, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) multi_seek<TILES, NQ>(cb, segs, nseg, u1, lane);
            pipe_load<TILES>(B, cb.base, (u1 < total_steps ? u1 : u) - cb.begin, lane);  // clamped at the tail: an L2 hit
            pipe_wait<LOADS>(A);
            multi_eval<TILES, NQ>(A, ca, total);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) multi_seek<TILES, NQ>(ca, segs, nseg, u2, lane);
            pipe_load<TILES>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane);
            pipe_wait<LOADS>(B);
            multi_eval<TILES, NQ>(B, cb, total);
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<0>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<0>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point, every live box
        const DevMultiSegment &g = segs[i];
        const uint32_t live = g.live;
        if (!live) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {
            int x = 0, y = 0, z = 0;
            if (p < n) {
                const int *pt = q0 + 3 * p;
                x = pt[0], y = pt[1], z = pt[2];
            }
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                if (!((live >> q) & 1u)) continue;
                const bool pass = (p < n) & ((uint32_t)(x - g.lo[q][0]) <= g.width[q][0]) & ((uint32_t)(y - g.lo[q][1]) <= g.width[q][1]) &
                                  ((uint32_t)(z - g.lo[q][2]) <= g.width[q][2]);
                total[q] += (uint64_t)__popcll(__ballot(pass));
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NQ; q++) partials[(uint64_t)q * gridDim.x + blockIdx.x] = total[q];
    }
}

// THE finish reduction of every count kernel (pcq_launch_finish_counts): block q folds slice q of the per-workgroup partial
// counts (nblocks words), += into d_counts[q].  One slice for the one-count kernels, a slice per box or class here and in
// scan_class_hist.hip.
__global__ __launch_bounds__(BLOCK) void k_finish_counts(const uint64_t *__restrict__ partials, int nblocks, uint64_t *__restrict__ d_counts) {
    __shared__ uint64_t s[BLOCK];
    const uint64_t *slice = partials + (uint64_t)blockIdx.x * (uint64_t)nblocks;
    uint64_t t = 0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) t += slice[i];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)(d_counts + blockIdx.x), (unsigned long long)s[0]);
}

// The finish of the height raster (scan_zrange.hip, pcq_launch_finish_zrange): block `cell` folds slice `cell` of the per-workgroup
// partials — max z in the high word, min z in the low word, both signed; a workgroup that met no point of the cell wrote INT32_MIN
// and INT32_MAX — and folds the two into d_zmin[cell] and d_zmax[cell] (vector atomics on global memory: callers on several streams
// may fold into the same words).  A cell no workgroup reached touches neither word.
__global__ __launch_bounds__(BLOCK) void k_finish_zrange(const uint64_t *__restrict__ partials, int nblocks, int32_t *__restrict__ d_zmin,
                                                        int32_t *__restrict__ d_zmax) {
    __shared__ int32_t smin[BLOCK], smax[BLOCK];
    const uint64_t *slice = partials + (uint64_t)blockIdx.x * (uint64_t)nblocks;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) {
        const uint64_t w = slice[i];
        const int32_t lo = (int32_t)(uint32_t)w, hi = (int32_t)(uint32_t)(w >> 32);
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
    }
    smin[threadIdx.x] = mn, smax[threadIdx.x] = mx;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const int32_t a = smin[threadIdx.x + off], b = smax[threadIdx.x + off];
            if (a < smin[threadIdx.x]) smin[threadIdx.x] = a;
            if (b > smax[threadIdx.x]) smax[threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && smin[0] <= smax[0]) {
        atomicMin(d_zmin + blockIdx.x, smin[0]);
        atomicMax(d_zmax + blockIdx.x, smax[0]);
    }
}

template <int NQ>
void launch_multi(pcq_ctx *ctx, unsigned g, int nsegments, uint64_t steps, hipStream_t s) {
    hipLaunchKernelGGL((k_bounds_count_multi_pipe<K1_TILES, NQ>), dim3(g), dim3(64), 0, s,
                       reinterpret_cast<const DevMultiSegment *>(ctx->d_segments), nsegments, steps, ctx->d_partials);
}

}  // namespace

extern "C" int pcq_scan_dev_count_batch_multi(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                              size_t nqueries, uint64_t *device_totals, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_totals)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_count_batch_multi: null argument");
    if (nqueries == 0 || nqueries > PCQ_MULTI_BOX_MAX)
        return pcq_fail(PCQ_ERR_ARG, "count_batch_multi: %zu queries (1 .. %d)", nqueries, PCQ_MULTI_BOX_MAX);
    if (nsegments == 0) return PCQ_OK;
    for (size_t i = 0; i < nsegments * nqueries; i++)
        if (preds[i].kind != PCQ_PRED_BOUNDS)
            return pcq_fail(PCQ_ERR_ARG, "count_batch_multi: predicate kind %d of segment %zu, query %zu (PCQ_PRED_BOUNDS only)", preds[i].kind,
                            i / nqueries, i % nqueries);
    if (nqueries == 1) {  // one box: the batched K1 (it checks stride and alignment itself)
        for (size_t i = 0; i < nsegments; i++)
            if (!cols[i].xyz && cols[i].n) return pcq_fail(PCQ_ERR_ARG, "count_batch_multi: positions block %zu is null", i);
        return pcq_scan_dev_count_batch(ctx, cols, preds, nsegments, device_totals, stream);
    }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const int nq = nqueries <= 2 ? 2 : (nqueries <= 4 ? 4 : 8);  // the instantiation: slots from nqueries on are dead
    int waves = MULTI_WAVES_PER_CU;
#ifdef PCQ_LAB  // (tools/resident_multi_rate.py sweeps it)
    if (ctx->multi_waves_per_cu) waves = ctx->multi_waves_per_cu;
#endif
    const K1Batch b = {"count_batch_multi", PCQ_SEGMENTS_MULTI, waves, nq, (int)nqueries, /*null_refused=*/true};
    return k1_batch_launch<DevMultiSegment>(
        ctx, b, cols, nsegments, device_totals, s, [](size_t) { return (int)PCQ_OK; },
        [&](DevMultiSegment &g, size_t i) {
            for (size_t q = 0; q < nqueries; q++) {
                DevPred dp;
                const int rc = pcq_make_dev_pred(&preds[i * nqueries + q], &dp);
                if (rc) return rc;
                if (dp.empty) continue;  // the slot stays zero and its live bit clear
                g.live |= 1u << q;
                for (int a = 0; a < 3; a++) g.lo[q][a] = dp.lo[a], g.width[q][a] = dp.width[a];
            }
            return (int)PCQ_OK;
        },
        [&](unsigned g, uint64_t steps) {
            if (nq == 2) launch_multi<2>(ctx, g, (int)nsegments, steps, s);
            else if (nq == 4) launch_multi<4>(ctx, g, (int)nsegments, steps, s);
            else launch_multi<8>(ctx, g, (int)nsegments, steps, s);
            return (int)PCQ_OK;
        });
}

int pcq_launch_finish_counts(pcq_ctx *ctx, int nslices, int nblocks, uint64_t *d_counts, hipStream_t s) {
    hipLaunchKernelGGL(k_finish_counts, dim3((unsigned)nslices), dim3(BLOCK), 0, s, ctx->d_partials, nblocks, d_counts);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}

// The finish of the mean-height raster (scan_zsum.hip): k_finish_counts twice, over the count slices into d_count and over the sum
// slices behind them into d_zsum — the sums are two's complement words, so the unsigned add modulo 2^64 is the signed one.
int pcq_launch_finish_zsum(pcq_ctx *ctx, int ncells, int nblocks, uint64_t *d_count, int64_t *d_zsum, hipStream_t s) {
    const uint64_t *sums = ctx->d_partials + (uint64_t)ncells * (uint64_t)nblocks;
    hipLaunchKernelGGL(k_finish_counts, dim3((unsigned)ncells), dim3(BLOCK), 0, s, ctx->d_partials, nblocks, d_count);
    hipLaunchKernelGGL(k_finish_counts, dim3((unsigned)ncells), dim3(BLOCK), 0, s, sums, nblocks, reinterpret_cast<uint64_t *>(d_zsum));
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}

// The finish of the height-spread raster (scan_zmoments.hip): k_finish_counts once per array, over the four quarters of the partials
// in the kernel's order — counts, sums, the low and the high words of the squares — each += into its array modulo 2^64.
int pcq_launch_finish_zmoments(pcq_ctx *ctx, int ncells, int nblocks, uint64_t *d_count, int64_t *d_zsum, uint64_t *d_zsq_lo, uint64_t *d_zsq_hi,
                               hipStream_t s) {
    const uint64_t quarter = (uint64_t)ncells * (uint64_t)nblocks;
    uint64_t *const out[4] = {d_count, reinterpret_cast<uint64_t *>(d_zsum), d_zsq_lo, d_zsq_hi};
    for (int a = 0; a < 4; a++)
        hipLaunchKernelGGL(k_finish_counts, dim3((unsigned)ncells), dim3(BLOCK), 0, s, ctx->d_partials + a * quarter, nblocks, out[a]);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}

int pcq_launch_finish_zrange(pcq_ctx *ctx, int ncells, int nblocks, int32_t *d_zmin, int32_t *d_zmax, hipStream_t s) {
    hipLaunchKernelGGL(k_finish_zrange, dim3((unsigned)ncells), dim3(BLOCK), 0, s, ctx->d_partials, nblocks, d_zmin, d_zmax);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}
