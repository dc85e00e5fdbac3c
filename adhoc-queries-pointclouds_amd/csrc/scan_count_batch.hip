// scan_count_batch.hip — the batched counts of the combined kinds over many resident LAST files in one launch:
// PCQ_PRED_BOUNDS_CLASS (box AND class, 13 B per point) and PCQ_PRED_BOUNDS_TIME (box AND GPS time range, 20 B per point).
//
// The kernel is k_bounds_count_batch_pipe<K1_TILES, ClassBytes / GpsTimes> (scan_tiles.h), the batched K1 with a compile-time
// second column; the plain box kind is the same template without one, launched by pcq_scan_dev_count_batch (scan_count.hip).
// One host routine serves both kinds here; per kind only the checks of the second column and the column's fields of a segment
// differ (DevCombinedSegment / DevBoundsTimeSegment, each at its own pitch in the context's segment table).
#include <vector>

#include "pcq_internal.h"
#include "scan_tiles.h"

namespace {

template <typename Col>
struct BatchKind {};
template <>
struct BatchKind<ClassBytes> {
    static constexpr int pred = PCQ_PRED_BOUNDS_CLASS;
    static constexpr const char *entry = "pcq_scan_dev_count_batch_combined", *prefix = "count_batch_combined", *pred_name = "PCQ_PRED_BOUNDS_CLASS";
};
template <>
struct BatchKind<GpsTimes> {
    static constexpr int pred = PCQ_PRED_BOUNDS_TIME;
    static constexpr const char *entry = "pcq_scan_dev_count_batch_bounds_time", *prefix = "count_batch_bounds_time", *pred_name = "PCQ_PRED_BOUNDS_TIME";
};

// the second column of segment i: refused, or into the segment
int seg_column(DevCombinedSegment &g, const pcq_columns &c, size_t) {
    if (c.cls_stride != 1 || (!c.cls && c.n)) return pcq_fail(PCQ_ERR_ARG, "count_batch_combined: LAST classification blocks only (stride 1)");
    g.cls = (const uint8_t *)c.cls;
    return PCQ_OK;
}
int seg_column(DevBoundsTimeSegment &g, const pcq_columns &c, size_t i) {
    if (c.cls_stride != 8 || ((uintptr_t)c.cls & 7) != 0 || (!c.cls && c.n))
        return pcq_fail(PCQ_ERR_ARG, "count_batch_bounds_time: LAST time blocks only (stride 8, 8-byte aligned), segment %zu", i);
    g.times = (const uint8_t *)c.cls;
    return PCQ_OK;
}
void seg_pred(DevCombinedSegment &g, const DevPred &dp) { g.pat = 0x01010101u * (dp.cls & 0xffu); }
void seg_pred(DevBoundsTimeSegment &g, const DevPred &dp) { g.t0 = dp.wmin[0], g.t1 = dp.wmax[0]; }

template <typename Col>
int count_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments, uint64_t *device_total, void *stream) {
    typedef BatchKind<Col> K;
    typedef typename BatchSeg<ColOf<Col>::value>::type Seg;
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_total) return pcq_fail(PCQ_ERR_ARG, "%s: null argument", K::entry);
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // the table first: nothing is touched when a segment is refused
    std::vector<Seg> table(nsegments);
    memset(table.data(), 0, nsegments * sizeof(Seg));
    uint64_t steps = 0;
    for (size_t i = 0; i < nsegments; i++) {
        if (preds[i].kind != K::pred)
            return pcq_fail(PCQ_ERR_ARG, "%s: predicate kind %d of segment %zu (%s only)", K::prefix, preds[i].kind, i, K::pred_name);
        if (cols[i].xyz_stride != 12) return pcq_fail(PCQ_ERR_ARG, "%s: LAST positions blocks only (stride 12)", K::prefix);
        if (((uintptr_t)cols[i].xyz & 15) != 0 || (!cols[i].xyz && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "%s: positions block %zu not 16-byte aligned", K::prefix, i);
        Seg &g = table[i];
        int rc = seg_column(g, cols[i], i);
        if (rc) return rc;
        DevPred dp;
        rc = pcq_make_dev_pred(&preds[i], &dp);
        if (rc) return rc;
        g.xyz = reinterpret_cast<const int4 *>(cols[i].xyz);
        g.n = cols[i].n;
        g.tile_begin = steps;
        for (int a = 0; a < 3; a++) g.lo[a] = dp.lo[a], g.width[a] = dp.width[a];
        g.empty = dp.empty;
        seg_pred(g, dp);
        steps += cols[i].n / ((uint64_t)K1_TILES * TILE_POINTS);
    }
    int rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    rc = pcq_upload_segment_table(ctx, K::pred, nsegments, table.data(), nsegments * sizeof(Seg), s);
    if (rc) return rc;
    uint64_t g = (uint64_t)ctx->num_cus * K1_WAVES_PER_CU;
    if (g > steps + nsegments) g = steps + nsegments;
    rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL((k_bounds_count_batch_pipe<K1_TILES, Col>), dim3((unsigned)g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps,
                       ctx->d_partials);
    hipLaunchKernelGGL(k_finish_count, dim3(1), dim3(BLOCK), 0, s, ctx->d_partials, (int)g, device_total);
    PCQ_HIP(hipGetLastError());
    return PCQ_OK;
}

}  // namespace

extern "C" int pcq_scan_dev_count_batch_combined(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                                 uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    return count_batch<ClassBytes>(ctx, cols, preds, nsegments, device_total, stream);
}

extern "C" int pcq_scan_dev_count_batch_bounds_time(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments,
                                                    uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    return count_batch<GpsTimes>(ctx, cols, preds, nsegments, device_total, stream);
}
