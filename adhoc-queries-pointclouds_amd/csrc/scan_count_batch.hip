// scan_count_batch.hip — the batched counts of the combined kinds over many resident LAST files in one launch:
// PCQ_PRED_BOUNDS_CLASS (box AND class, 13 B per point) and PCQ_PRED_BOUNDS_TIME (box AND GPS time range, 20 B per point).
//
// The kernel is k_bounds_count_batch_pipe<K1_TILES, ClassBytes / GpsTimes> (scan_tiles.h), the batched K1 with a compile-time
// second column; the plain box kind is the same template without one, launched by pcq_scan_dev_count_batch (scan_count.hip).
// k1_batch_launch (scan_batch_host.h) is the host side; per kind only the checks of the second column and the column's fields of a
// segment differ (DevCombinedSegment / DevBoundsTimeSegment, each at its own pitch in the context's segment table).
#include "pcq_internal.h"
#include "scan_batch_host.h"
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
    const K1Batch b = {K::prefix, K::pred, K1_WAVES_PER_CU, 1, 1, /*null_refused=*/true};
    return k1_batch_launch<Seg>(
        ctx, b, cols, nsegments, device_total, s,
        [&](size_t i) {
            return preds[i].kind != K::pred
                       ? pcq_fail(PCQ_ERR_ARG, "%s: predicate kind %d of segment %zu (%s only)", K::prefix, preds[i].kind, i, K::pred_name)
                       : (int)PCQ_OK;
        },
        [&](Seg &g, size_t i) {
            int rc = seg_column(g, cols[i], i);
            if (rc) return rc;
            DevPred dp;
            rc = pcq_make_dev_pred(&preds[i], &dp);
            if (rc) return rc;
            seg_box(g, dp);
            seg_pred(g, dp);
            return (int)PCQ_OK;
        },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL((k_bounds_count_batch_pipe<K1_TILES, Col>), dim3(g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps,
                               ctx->d_partials);
            return (int)PCQ_OK;
        });
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
