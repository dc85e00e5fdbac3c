// scan_batch_host.h — the host side of the K1-family batched launches (scan_count.hip, scan_count_batch.hip, scan_count_multi.hip,
// scan_class_hist.hip, scan_time_hist.hip, scan_raster.hip, scan_zrange.hip, scan_zsum.hip, scan_zsum_classes.hip, scan_zrange_classes.hip, scan_zmoments.hip, scan_polygon.hip): host code only; the kernels and their constants are in scan_tiles.h.
#pragma once

#include <vector>

#include "scan_tiles.h"

namespace {

// The host side of a K1-family batched launch (the box, box AND class and box AND time counts, the multi-box count, the class
// histogram): a table of Seg, one per positions block, steps numbered across the segments; then the scratch stream, the table's
// upload under the entry's kind, min(CUs x waves, steps + segments) workgroups of one wave, their partials, the kernel and
// the finish.  The table first: nothing is touched when a segment is refused.  Per segment, in this order: admit(i) (the
// entry's refusals that come before those of the positions), the positions' refusals, fill(seg, i) (the entry's columns and
// predicates, or their refusal); xyz, n and tile_begin are filled here.  launch(workgroups, steps) enqueues the kernel, or refuses.
// A trailer (the time histogram's edges, the polygon count's outlines) travels behind the table in the same upload, under the same compare of all bytes.
// finish(workgroups) enqueues the fold of the partials into the caller's words: pcq_launch_finish_counts (`folded` slices added into
// d_out) for every count; the height, mean-height and height-spread rasters bring their own (pcq_launch_finish_zrange, _zsum, _zmoments).
struct K1Batch {
    const char *prefix;  // of a refusal's text
    int table_kind;      // the key of the table in HBM (pcq_upload_segment_table)
    int waves_per_cu;
    int slices;          // words of the partials per workgroup
    int folded;          // the first `folded` slices are added into d_out[0 .. folded)
    bool null_refused;   // positions that are null with n > 0 are refused (the plain box kind never has)
    const void *trailer = nullptr;  // launch-level data behind the table in HBM (8-byte aligned there: every Seg is)
    size_t trailer_bytes = 0;
    bool checks_only = false;       // every refusal of the table, then PCQ_OK: no upload, no launch, no finish (the class-filtered mean-height raster's empty set)
};
template <typename Seg, typename DP>
void seg_box(Seg &g, const DP &dp) {
    for (int a = 0; a < 3; a++) g.lo[a] = dp.lo[a], g.width[a] = dp.width[a];
    g.empty = dp.empty;
}
// admit(i) of the entries that take a box and nothing else
inline int admit_bounds_only(const char *prefix, const pcq_predicate &pred, size_t i) {
    return pred.kind != PCQ_PRED_BOUNDS ? pcq_fail(PCQ_ERR_ARG, "%s: predicate kind %d of segment %zu (PCQ_PRED_BOUNDS only)", prefix, pred.kind, i)
                                        : (int)PCQ_OK;
}
template <typename Seg, typename Admit, typename Fill, typename Launch, typename Finish>
int k1_batch_launch(pcq_ctx *ctx, const K1Batch &b, const pcq_columns *cols, size_t nsegments, hipStream_t s, Admit admit, Fill fill, Launch launch,
                    Finish finish) {
    std::vector<Seg> table(nsegments);
    memset(table.data(), 0, nsegments * sizeof(Seg));
    uint64_t steps = 0;
    for (size_t i = 0; i < nsegments; i++) {
        int rc = admit(i);
        if (rc) return rc;
        if (cols[i].xyz_stride != 12) return pcq_fail(PCQ_ERR_ARG, "%s: LAST positions blocks only (stride 12)", b.prefix);
        if (((uintptr_t)cols[i].xyz & 15) != 0 || (b.null_refused && !cols[i].xyz && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "%s: positions block %zu not 16-byte aligned", b.prefix, i);
        Seg &g = table[i];
        rc = fill(g, i);
        if (rc) return rc;
        g.xyz = reinterpret_cast<const int4 *>(cols[i].xyz);
        g.n = cols[i].n;
        g.tile_begin = steps;
        steps += cols[i].n / ((uint64_t)K1_TILES * TILE_POINTS);
    }
    if (b.checks_only) return PCQ_OK;
    int rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    if (b.trailer_bytes) {
        std::vector<uint8_t> both(nsegments * sizeof(Seg) + b.trailer_bytes);
        memcpy(both.data(), table.data(), nsegments * sizeof(Seg));
        memcpy(both.data() + nsegments * sizeof(Seg), b.trailer, b.trailer_bytes);
        rc = pcq_upload_segment_table(ctx, b.table_kind, nsegments, both.data(), both.size(), s);
    } else {
        rc = pcq_upload_segment_table(ctx, b.table_kind, nsegments, table.data(), nsegments * sizeof(Seg), s);
    }
    if (rc) return rc;
    uint64_t g = (uint64_t)ctx->num_cus * (uint64_t)b.waves_per_cu;
    if (g > steps + nsegments) g = steps + nsegments;
    rc = pcq_ensure_partials(ctx, (size_t)g * (size_t)b.slices);
    if (rc) return rc;
    rc = launch((unsigned)g, steps);
    if (rc) return rc;
    return finish((int)g);
}
template <typename Seg, typename Admit, typename Fill, typename Launch>
int k1_batch_launch(pcq_ctx *ctx, const K1Batch &b, const pcq_columns *cols, size_t nsegments, uint64_t *d_out, hipStream_t s, Admit admit,
                    Fill fill, Launch launch) {
    return k1_batch_launch<Seg>(ctx, b, cols, nsegments, s, admit, fill, launch,
                                [&](int g) { return pcq_launch_finish_counts(ctx, b.folded, g, d_out, s); });
}

}  // namespace
