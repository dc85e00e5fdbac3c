// scan_count_combined.hip — the batched count of PCQ_PRED_BOUNDS_CLASS: box AND class over many resident LAST files in one launch.
//
// k_bounds_count_batch_pipe (scan_count.hip) with K1's compile-time second column COL_U8 (scan_tiles.h): one wave per
// workgroup, two tiles per step, two register sets; a tile's two class dwords per lane ride behind its three position loads
// in the same counted s_waitcnt pipeline (TILES * (3 + 2) loads per register set), and the verdicts reach the lanes that
// hold a point's first dword through ds_bpermute, as in k_bounds_count_w1_pipe<2, ClassBytes>.  13 B per point.
// New here is what changes with the segment: besides the box, the half of Col2<COL_U8> that depends on the class block's
// address and the class byte (base, shift, pat, lane 63's off_hi); the addr_* / bit_* lane constants are computed once.
// The segments are DevCombinedSegment, at their own pitch in the context's segment table (d_segments / h_segments).
#include <vector>

#include "pcq_internal.h"
#include "scan_tiles.h"

namespace {

// Steps are numbered across all segments; each of the two register sets remembers the segment its step came from.
struct SegCursor2 {
    int s;
    uint64_t begin, end;
    const v4i *base;
    LaneBox lb;
    bool empty;
    const uint8_t *cbase;  // the class bytes, rounded down to a dword (uniform)
    uint32_t shift, pat;   // 8 x the misalignment; the class byte in every byte (uniform)
    uint32_t off_hi;       // this lane's second dword of a tile (lane 63 of an aligned block: its first)
};
__device__ __forceinline__ const DevCombinedSegment &xseg(const DevSegment *raw, int i) {
    return reinterpret_cast<const DevCombinedSegment *>(raw)[i];
}
template <int TILES>
__device__ __forceinline__ void seg_seek(SegCursor2 &c, const DevSegment *__restrict__ raw, int nseg, uint64_t u, int lane) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= xseg(raw, c.s + 1).tile_begin) c.s++;
    const DevCombinedSegment &g = xseg(raw, c.s);
    c.begin = g.tile_begin;
    c.end = c.begin + g.n / ((uint64_t)TILES * TILE_POINTS);
    c.base = reinterpret_cast<const v4i *>(g.xyz);
    c.empty = g.empty != 0;
    // everything of the segment through SGPRs (scan_count.hip seg_seek: a vector load here would bring a vmcnt(0) that
    // drains the prefetched tiles)
    int32_t lo[3];
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = g.lo[k];
        w[k] = g.width[k];
        asm volatile("" : "+s"(lo[k]), "+s"(w[k]));
    }
    c.lb = rotate_box(lo, w, lane);
    uint64_t cls = (uint64_t)(uintptr_t)g.cls;
    uint32_t pat = g.pat;
    asm volatile("" : "+s"(cls), "+s"(pat));
    const uint32_t mis = (uint32_t)cls & 3u;
    c.cbase = reinterpret_cast<const uint8_t *>((uintptr_t)(cls - mis));
    c.shift = 8 * mis;
    c.pat = pat;
    c.off_hi = lane == 63 && mis == 0 ? 4 * lane : 4 * lane + 4;  // (col2_setup: nothing of the tile lies behind an aligned block's dword 63)
}
// the lane constants with the cursor's segment
__device__ __forceinline__ Col2<COL_U8> col2_of(Col2<COL_U8> lanes, const SegCursor2 &c) {
    lanes.base = c.cbase;
    lanes.off_hi = c.off_hi;
    lanes.shift = c.shift;
    lanes.pat = c.pat;
    return lanes;
}

template <int TILES>
__global__ __launch_bounds__(64) void k_bounds_class_count_batch_pipe(const DevSegment *__restrict__ raw, int nseg, uint64_t total_steps,
                                                                     uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_POINTS = (uint64_t)TILES * TILE_POINTS;
    constexpr int LOADS = TILES * (3 + col2_loads(COL_U8));  // per register set
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    uint64_t total = 0;
    if (blockIdx.x < total_steps) {
        Col2<COL_U8> lanes;
        lanes.base = nullptr;
        lanes.off_lo = 4 * lane, lanes.off_hi = 0, lanes.shift = 0, lanes.pat = 0;
        col2_lanes<COL_U8>(lanes, lane);
        PipeRegs<TILES, COL_U8> A, B;
        SegCursor2 ca = {0, 0, 0, nullptr, {}, true, nullptr, 0, 0, 0}, cb;
        uint64_t u = blockIdx.x;
        seg_seek<TILES>(ca, raw, nseg, u, lane);
        pipe_load<TILES, COL_U8>(A, ca.base, u - ca.begin, lane, col2_of(lanes, ca));
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) seg_seek<TILES>(cb, raw, nseg, u1, lane);
            pipe_load<TILES, COL_U8>(B, cb.base, (u1 < total_steps ? u1 : u) - cb.begin, lane, col2_of(lanes, cb));  // clamped at the tail: an L2 hit
            pipe_wait<TILES, LOADS, COL_U8>(A);
            if (!ca.empty) total += pipe_eval<TILES, COL_U8>(A, ca.lb, col2_of(lanes, ca));
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) seg_seek<TILES>(ca, raw, nseg, u2, lane);
            pipe_load<TILES, COL_U8>(A, ca.base, (u2 < total_steps ? u2 : u1) - ca.begin, lane, col2_of(lanes, ca));
            pipe_wait<TILES, LOADS, COL_U8>(B);
            if (!cb.empty) total += pipe_eval<TILES, COL_U8>(B, cb.lb, col2_of(lanes, cb));
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<TILES, 0, COL_U8>(A);
        pipe_wait<TILES, 0, COL_U8>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {  // fewer-than-a-step leftovers of segment i, one lane per point
        const DevCombinedSegment &g = xseg(raw, i);
        if (g.empty) continue;
        const uint64_t n = g.n;
        const int *q0 = reinterpret_cast<const int *>(g.xyz);
        const uint8_t c8 = (uint8_t)(g.pat & 0xffu);
        for (uint64_t p = (n / STEP_POINTS) * STEP_POINTS + lane; p < ((n + 63) & ~63ull); p += 64) {
            bool pass = false;
            if (p < n) {
                const int *q = q0 + 3 * p;
                pass = ((uint32_t)(q[0] - g.lo[0]) <= g.width[0]) & ((uint32_t)(q[1] - g.lo[1]) <= g.width[1]) &
                       ((uint32_t)(q[2] - g.lo[2]) <= g.width[2]) & (g.cls[p] == c8);
            }
            total += (uint64_t)__popcll(__ballot(pass));
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(BLOCK) void k_finish_count_combined(const uint64_t *__restrict__ partials, int nblocks, uint64_t *__restrict__ d_count) {
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

extern "C" int pcq_scan_dev_count_batch_combined(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                                 uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_total)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_count_batch_combined: null argument");
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // the table first: nothing is touched when a segment is refused
    std::vector<DevCombinedSegment> table(nsegments);
    memset(table.data(), 0, nsegments * sizeof(DevCombinedSegment));
    uint64_t steps = 0;
    for (size_t i = 0; i < nsegments; i++) {
        if (preds[i].kind != PCQ_PRED_BOUNDS_CLASS)
            return pcq_fail(PCQ_ERR_ARG, "count_batch_combined: predicate kind %d of segment %zu (PCQ_PRED_BOUNDS_CLASS only)", preds[i].kind, i);
        if (cols[i].xyz_stride != 12) return pcq_fail(PCQ_ERR_ARG, "count_batch_combined: LAST positions blocks only (stride 12)");
        if (((uintptr_t)cols[i].xyz & 15) != 0 || (!cols[i].xyz && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "count_batch_combined: positions block %zu not 16-byte aligned", i);
        if (cols[i].cls_stride != 1 || (!cols[i].cls && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "count_batch_combined: LAST classification blocks only (stride 1)");
        DevPred dp;
        const int rc = pcq_make_dev_pred(&preds[i], &dp);
        if (rc) return rc;
        DevCombinedSegment &g = table[i];
        g.xyz = reinterpret_cast<const int4 *>(cols[i].xyz);
        g.cls = (const uint8_t *)cols[i].cls;
        g.n = cols[i].n;
        g.tile_begin = steps;
        for (int a = 0; a < 3; a++) g.lo[a] = dp.lo[a], g.width[a] = dp.width[a];
        g.empty = dp.empty;
        g.pat = 0x01010101u * (dp.cls & 0xffu);
        steps += cols[i].n / ((uint64_t)K1_TILES * TILE_POINTS);
    }
    int rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    const size_t bytes = nsegments * sizeof(DevCombinedSegment);
    rc = pcq_ensure_segment_table(ctx, bytes);
    if (rc) return rc;
    // uploaded only when it differs from the table in HBM: the kind tells a combined table from a bounds or class table of
    // as many segments
    if (ctx->segments_uploaded != nsegments || ctx->segments_kind != PCQ_PRED_BOUNDS_CLASS || memcmp(ctx->h_segments, table.data(), bytes) != 0) {
        PCQ_HIP(hipStreamSynchronize(s));  // the previous upload from the pinned table must have been consumed
        memcpy(ctx->h_segments, table.data(), bytes);
        PCQ_HIP(hipMemcpyAsync(ctx->d_segments, ctx->h_segments, bytes, hipMemcpyHostToDevice, s));
        ctx->segments_uploaded = nsegments;
        ctx->segments_kind = PCQ_PRED_BOUNDS_CLASS;
    }
    uint64_t g = (uint64_t)ctx->num_cus * K1_WAVES_PER_CU;
    if (g > steps + nsegments) g = steps + nsegments;
    rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bounds_class_count_batch_pipe<K1_TILES>, dim3((unsigned)g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps,
                       ctx->d_partials);
    hipLaunchKernelGGL(k_finish_count_combined, dim3(1), dim3(BLOCK), 0, s, ctx->d_partials, (int)g, device_total);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}
