// scan_count_bounds_time.hip — the batched count of PCQ_PRED_BOUNDS_TIME: box AND GPS time range over many resident LAST files
// in one launch.
//
// k_bounds_class_count_batch_pipe (scan_count_combined.hip) with K1's other compile-time second column, COL_F64
// (scan_tiles.h): one wave per workgroup, two tiles per step, two register sets; a tile's two 16-byte time loads per lane
// (points 2l, 2l + 1 and 128 + 2l, 129 + 2l) ride behind its three position loads in the same counted s_waitcnt pipeline
// (TILES * (3 + 2) loads per register set), and the verdicts reach the lanes that hold a point's first dword through
// ds_bpermute, as in k_bounds_count_w1_pipe<2, Times>.  20 B per point.
// What changes with the segment: the box, the time block's base and the range [t0, t1) — all through SGPRs; the addr_* /
// bit_* lane constants are computed once.  The segments are DevBoundsTimeSegment, at their own pitch in the context's segment
// table (d_segments / h_segments).
#include <vector>

#include "pcq_internal.h"
#include "scan_tiles.h"

namespace {

// Steps are numbered across all segments; each of the two register sets remembers the segment its step came from.
struct SegCursorT {
    int s;
    uint64_t begin, end;
    const v4i *base;
    LaneBox lb;
    bool empty;
    const uint8_t *tbase;  // the segment's times (uniform)
    double t0, t1;         // its range (uniform)
};
__device__ __forceinline__ const DevBoundsTimeSegment &tseg(const DevSegment *raw, int i) {
    return reinterpret_cast<const DevBoundsTimeSegment *>(raw)[i];
}
template <int TILES>
__device__ __forceinline__ void seg_seek(SegCursorT &c, const DevSegment *__restrict__ raw, int nseg, uint64_t u, int lane) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= tseg(raw, c.s + 1).tile_begin) c.s++;
    const DevBoundsTimeSegment &g = tseg(raw, c.s);
    c.begin = g.tile_begin;
    c.end = c.begin + g.n / ((uint64_t)TILES * TILE_POINTS);
    c.base = reinterpret_cast<const v4i *>(g.xyz);
    c.empty = g.empty != 0;
    // the segment's box, time block and range through SGPRs (scan_count.hip seg_seek: a vector load here would bring a
    // vmcnt(0) that drains the prefetched tiles).  The skip loop above is not covered: from its second iteration on the compiler
    // reads tile_begin with a vector load and waits for it, so a workgroup that jumps over more than one segment drains both
    // register sets once — as in k_bounds_class_count_batch_pipe, whose seek this is
    int32_t lo[3];
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = g.lo[k];
        w[k] = g.width[k];
        asm volatile("" : "+s"(lo[k]), "+s"(w[k]));
    }
    c.lb = rotate_box(lo, w, lane);
    uint64_t times = (uint64_t)(uintptr_t)g.times;
    uint64_t b0 = (uint64_t)__double_as_longlong(g.t0), b1 = (uint64_t)__double_as_longlong(g.t1);
    asm volatile("" : "+s"(times), "+s"(b0), "+s"(b1));
    c.tbase = reinterpret_cast<const uint8_t *>((uintptr_t)times);
    c.t0 = __longlong_as_double((long long)b0);
    c.t1 = __longlong_as_double((long long)b1);
}
// the lane constants with the cursor's segment
__device__ __forceinline__ Col2<COL_F64> col2_of(Col2<COL_F64> lanes, const SegCursorT &c) {
    lanes.base = c.tbase;
    lanes.t0 = c.t0;
    lanes.t1 = c.t1;
    return lanes;
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_time_count_batch_pipe(const DevSegment *__restrict__ raw, int nseg, uint64_t total_steps,
                                                                    uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    constexpr int LOADS = TILES * (3 + col2_loads(COL_F64));  // per register set
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    uint64_t total = 0;
    if (blockIdx.x < total_steps) {
        Col2<COL_F64> lanes;
        lanes.base = nullptr;
        lanes.t0 = lanes.t1 = 0.0;
        col2_lanes<COL_F64>(lanes, lane);
        PipeRegs<TILES, COL_F64> A, B;
        SegCursorT ca = {0, 0, 0, nullptr, {}, true, nullptr, 0.0, 0.0}, cb;
        uint64_t u = blockIdx.x;
        seg_seek<TILES>(ca, raw, nseg, u, lane);
        pipe_load<TILES, COL_F64>(A, ca.base, u - ca.begin, lane, col2_of(lanes, ca));
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) seg_seek<TILES>(cb, raw, nseg, u1, lane);
            pipe_load<TILES, COL_F64>(B, cb.base, (u1 < total_steps ? u1 : u) - cb.begin, lane, col2_of(lanes, cb));  // clamped at the tail: an L2 hit
            pipe_wait<TILES, LOADS, COL_F64>(A);
            if (!ca.empty) total += pipe_eval<TILES, COL_F64>(A, ca.lb, col2_of(lanes, ca));
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES>(ca, raw, nseg, u2, lane);
            pipe_load<TILES, COL_F64>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane, col2_of(lanes, ca));
            pipe_wait<TILES, LOADS, COL_F64>(B);
            if (!cb.empty) total += pipe_eval<TILES, COL_F64>(B, cb.lb, col2_of(lanes, cb));
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<TILES, 0, COL_F64>(A);
        pipe_wait<TILES, 0, COL_F64>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevBoundsTimeSegment &g = tseg(raw, i);
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const double *tq = reinterpret_cast<const double *>(g.times);
        const double t0 = g.t0, t1 = g.t1;
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {
            bool pass = false;
            if (p < n) {
                const int *q = q0 + 3 * p;
                const double t = tq[p];
                pass = ((uint32_t)(q[0] - g.lo[0]) <= g.width[0]) & ((uint32_t)(q[1] - g.lo[1]) <= g.width[1]) &
                       ((uint32_t)(q[2] - g.lo[2]) <= g.width[2]) & (t >= t0) & (t < t1);
            }
            total += (uint64_t)__popcll(__ballot(pass));
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(BLOCK) void k_finish_count_bounds_time(const uint64_t *__restrict__ partials, int nblocks, uint64_t *__restrict__ d_count) {
    __shared__ uint64_t s[BLOCK];
    uint64_t t = 0;
    for (int i = threadIdx.x; i < nblocks; i += BLOCK) t += partials[i];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd((unsigned long long *)d_count, (unsigned long long)s[0]);
}

}  // namespace

extern "C" int pcq_scan_dev_count_batch_bounds_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                                    uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_total)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_count_batch_bounds_time: null argument");
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // the table first: nothing is touched when a segment is refused
    std::vector<DevBoundsTimeSegment> table(nsegments);
    memset(table.data(), 0, nsegments * sizeof(DevBoundsTimeSegment));
    uint64_t steps = 0;
    for (size_t i = 0; i < nsegments; i++) {
        if (preds[i].kind != PCQ_PRED_BOUNDS_TIME)
            return pcq_fail(PCQ_ERR_ARG, "count_batch_bounds_time: predicate kind %d of segment %zu (PCQ_PRED_BOUNDS_TIME only)", preds[i].kind, i);
        if (cols[i].xyz_stride != 12) return pcq_fail(PCQ_ERR_ARG, "count_batch_bounds_time: LAST positions blocks only (stride 12)");
        if (((uintptr_t)cols[i].xyz & 15) != 0 || (!cols[i].xyz && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "count_batch_bounds_time: positions block %zu not 16-byte aligned", i);
        if (cols[i].cls_stride != 8 || ((uintptr_t)cols[i].cls & 7) != 0 || (!cols[i].cls && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "count_batch_bounds_time: LAST time blocks only (stride 8, 8-byte aligned), segment %zu", i);
        DevPred dp;
        const int rc = pcq_make_dev_pred(&preds[i], &dp);
        if (rc) return rc;
        DevBoundsTimeSegment &g = table[i];
        g.xyz = reinterpret_cast<const int4 *>(cols[i].xyz);
        g.times = (const uint8_t *)cols[i].cls;
        g.n = cols[i].n;
        g.tile_begin = steps;
        for (int a = 0; a < 3; a++) g.lo[a] = dp.lo[a], g.width[a] = dp.width[a];
        g.empty = dp.empty;
        g.t0 = dp.wmin[0];
        g.t1 = dp.wmax[0];
        steps += cols[i].n / ((uint64_t)K1_TILES * TILE_POINTS);
    }
    int rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const size_t bytes = nsegments * sizeof(DevBoundsTimeSegment);
    rc = pcq_ensure_segment_table(ctx, bytes);
    if (rc) return rc;
    // uploaded only when it differs from the table in HBM.  The byte compare alone decides that today: a table of another kind
    // has another layout, so its bytes differ; the kind in the key only keeps this true should two kinds ever share a layout
    if (ctx->segments_uploaded != nsegments || ctx->segments_kind != PCQ_PRED_BOUNDS_TIME || memcmp(ctx->h_segments, table.data(), bytes) != 0) {
        PCQ_HIP(hipStreamSynchronize(s));  // the previous upload from the pinned table must have been consumed
        memcpy(ctx->h_segments, table.data(), bytes);
        PCQ_HIP(hipMemcpyAsync(ctx->d_segments, ctx->h_segments, bytes, hipMemcpyHostToDevice, s));
        ctx->segments_uploaded = nsegments;
        ctx->segments_kind = PCQ_PRED_BOUNDS_TIME;
    }
    uint64_t g = (uint64_t)ctx->num_cus * K1_WAVES_PER_CU;
    if (g > steps + nsegments) g = steps + nsegments;
    rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bounds_time_count_batch_pipe<K1_TILES>, dim3((unsigned)g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps,
                       ctx->d_partials);
    hipLaunchKernelGGL(k_finish_count_bounds_time, dim3(1), dim3(BLOCK), 0, s, ctx->d_partials, (int)g, device_total);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}
