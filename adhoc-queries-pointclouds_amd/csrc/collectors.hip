// collectors.hip — the device-resident collectors of include/pcq.h (count, buffer, grid: construction, accessors, reset) and
// the scan over device-resident columns that feeds them.
#include "pcq_internal.h"

#include <cmath>
#include <new>

// ---------------------------------------------------------------------------------------------
// collectors
// ---------------------------------------------------------------------------------------------
static int new_collector(pcq_ctx *ctx, int kind, pcq_collector **out) {
    if (!ctx || !out) return pcq_fail(PCQ_ERR_ARG, "collector: null argument");
    *out = nullptr;
    PCQ_HIP(hipSetDevice(ctx->device));  // the collector's memory belongs to the context's device, whatever the thread used before
    pcq_collector *c = new (std::nothrow) pcq_collector();
    if (!c) return pcq_fail(PCQ_ERR_NOMEM, "collector: out of memory");
    c->kind = kind;
    c->ctx = ctx;
    *out = c;
    return PCQ_OK;
}

int pcq_collector_wait_last(const pcq_collector *c, hipStream_t s) {
    if (c->last_stream && c->last_stream != s) PCQ_HIP(hipStreamSynchronize(c->last_stream));
    return PCQ_OK;
}

// The number of points a count or buffer collector holds now, read on stream `s` (one synchronisation).
static int read_count(pcq_collector *c, hipStream_t s, uint64_t *out) {
    pcq_ctx *ctx = c->ctx;
    PCQ_HIP(hipMemcpyAsync(ctx->h_scalars, c->d_count + c->count_slot, 8, hipMemcpyDeviceToHost, s));
    PCQ_HIP(hipStreamSynchronize(s));
    *out = ctx->h_scalars[0];
    if (c->kind == COLL_BUFFER) c->n_upper = *out;
    return PCQ_OK;
}

// A count or buffer collector with its own counter: the point count (two words, see pcq_internal.h), zeroed.
static int new_counted(pcq_ctx *ctx, int kind, const char *what, pcq_collector **out) {
    int rc = new_collector(ctx, kind, out);
    if (rc) return rc;
    pcq_collector *c = *out;
    hipError_t e = hipMalloc((void **)&c->d_count, 16);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_count, 0, 16, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // scans may be enqueued on a caller's stream
    if (e != hipSuccess) {
        delete c;
        *out = nullptr;
        return pcq_fail(PCQ_ERR_HIP, "%s collector: %s", what, hipGetErrorString(e));
    }
    c->owns_count = true;
    return PCQ_OK;
}

extern "C" int pcq_collector_new_count(pcq_ctx *ctx, pcq_collector **out) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    return new_counted(ctx, COLL_COUNT, "count", out);
}

extern "C" int pcq_collector_new_count_at(pcq_ctx *ctx, uint64_t *device_counter, pcq_collector **out) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!device_counter) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_new_count_at: null counter");
    int rc = new_collector(ctx, COLL_COUNT, out);
    if (rc) return rc;
    (*out)->d_count = device_counter;
    (*out)->owns_count = false;
    return PCQ_OK;
}

extern "C" int pcq_collector_new_buffer(pcq_ctx *ctx, pcq_collector **out) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    return new_counted(ctx, COLL_BUFFER, "buffer", out);
}

static uint64_t rust_f64_as_u64(double v) {  // Rust `f64 as u64`: truncate toward zero, saturate, NaN -> 0
    if (!(v > 0.0)) return 0;
    if (v >= 18446744073709551616.0) return UINT64_MAX;
    return (uint64_t)v;
}

// SparseGrid::new — grid_sampling.rs:18-47
extern "C" int pcq_collector_new_grid(pcq_ctx *ctx, const double bmin[3], const double bmax[3], double cell_size,
                                      pcq_collector **out) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!bmin || !bmax) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_new_grid: null bounds");
    if (!ctx || !out) return pcq_fail(PCQ_ERR_ARG, "collector: null argument");
    *out = nullptr;
    uint64_t dims[3], bits[3], bitsum = 0;
    for (int a = 0; a < 3; a++) {
        const double extent = bmax[a] - bmin[a];          // :19-23
        const double ncells = std::ceil(extent / cell_size);  // :24-28
        bits[a] = rust_f64_as_u64(std::ceil(std::log2(ncells)));  // :29-31
        dims[a] = rust_f64_as_u64(ncells);                // :39-43
        bitsum += bits[a];
    }
    if (bitsum > 64)  // :32-34
        return pcq_fail(PCQ_ERR_GRID, "Too many cells ({}*{}*{}) in SparseGrid! The number of cells exceeds the capacity of a u64 index!");
    if (bitsum == 64)  // all-ones is a legal key then, which this table reserves as "empty"
        return pcq_fail(PCQ_ERR_UNSUPPORTED, "SparseGrid with exactly 64 key bits is not supported by the device hash table");
    if (!std::isfinite(cell_size) || !std::isfinite(bmin[0]) || !std::isfinite(bmin[1]) || !std::isfinite(bmin[2]) ||
        !std::isfinite(bmax[0]) || !std::isfinite(bmax[1]) || !std::isfinite(bmax[2]))
        return pcq_fail(PCQ_ERR_UNSUPPORTED, "SparseGrid with non-finite bounds or cell size is not supported");
    int rc = new_collector(ctx, COLL_GRID, out);
    if (rc) return rc;
    pcq_collector *c = *out;
    c->cell_size = cell_size;
    DevGrid &g = c->grid;
    for (int a = 0; a < 3; a++) {
        c->bmin[a] = g.bmin[a] = bmin[a];
        c->bmax[a] = g.bmax[a] = bmax[a];
        c->bits[a] = bits[a];
        c->dims[a] = dims[a];
        g.dims_f[a] = (double)dims[a];
        g.inv_extent[a] = 1.0 / (bmax[a] - bmin[a]);
        g.qk[a] = g.dims_f[a] / (bmax[a] - bmin[a]);
        g.qmax[a] = g.dims_f[a] + 2.0 < 0x1p31 ? g.dims_f[a] + 2.0 : 0x1p31;  // every point inside the bounds is below dims + 1
        g.guard[a] = g.qmax[a] * 0x1p-50;
        g.mask[a] = (1ull << (bits[a] & 63)) - 1;  // Rust release `1u64 << n` masks n to 6 bits
    }
    g.cell_size = cell_size;
    g.shift[0] = 0;
    g.shift[1] = (uint32_t)(bits[0] & 63);
    g.shift[2] = (uint32_t)((bits[0] + bits[1]) & 63);
    g.keys_wide = bitsum > 32 ? 1u : 0u;
    return PCQ_OK;
}

extern "C" int pcq_collector_free(pcq_collector *c) {
    PCQ_ON_DEVICE_OF_COLLECTOR(c);
    if (!c) return PCQ_OK;
    if (c->ctx) {
        (void)hipSetDevice(c->ctx->device);
        (void)hipStreamSynchronize(c->ctx->stream);
        (void)pcq_collector_wait_last(c, c->ctx->stream);  // scans enqueued on a caller's stream
    }
    if (c->owns_count && c->d_count) (void)hipFree(c->d_count);
    if (c->d_points && c->ctx) pcq_pool_free(c->ctx, c->d_points);
    if (c->kind == COLL_GRID) pcq_grid_release(c);
    delete c;
    return PCQ_OK;
}

extern "C" int pcq_collector_reset(pcq_collector *c) {
    PCQ_ON_DEVICE_OF_COLLECTOR(c);
    if (!c) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_reset: null collector");
    hipStream_t s = c->ctx->stream;
    c->next_index = 0;
    // scans enqueued on a caller's stream may still be reading and moving the counters
    int rc = pcq_collector_wait_last(c, s);
    if (rc) return rc;
    // The counters are zeroed on the context's stream and the stream is drained: the next scan may arrive on a caller's
    // stream that the context's scratch was last used on (pcq_scratch_stream then waits for nothing), and nothing else
    // would order the zeroing in front of that scan's read of the counter.
    if (c->kind != COLL_GRID) PCQ_HIP(hipMemsetAsync(c->d_count, 0, c->kind == COLL_COUNT ? 8 : 16, s));
    PCQ_HIP(hipStreamSynchronize(s));
    if (c->kind == COLL_BUFFER) {
        c->n_upper = 0;
        c->count_slot = 0;
    }
    if (c->kind == COLL_GRID) pcq_grid_release(c);
    return PCQ_OK;
}

extern "C" int pcq_collector_has_points(const pcq_collector *c) { return c && c->kind != COLL_COUNT; }

extern "C" int pcq_collector_flush(pcq_collector *c) {
    PCQ_ON_DEVICE_OF_COLLECTOR(c);
    if (!c) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_flush: null collector");
    int rc = pcq_collector_wait_last(c, c->ctx->stream);
    if (rc) return rc;
    if (c->kind == COLL_GRID) return pcq_grid_flush(c);  // (synchronises)
    PCQ_HIP(hipStreamSynchronize(c->ctx->stream));
    return PCQ_OK;
}

extern "C" int pcq_collector_point_count(pcq_collector *c, uint64_t *out) {
    PCQ_ON_DEVICE_OF_COLLECTOR(c);
    if (!c || !out) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_point_count: null argument");
    int rc = pcq_collector_wait_last(c, c->ctx->stream);
    if (rc) return rc;
    if (c->kind == COLL_GRID) return pcq_grid_drain(c, nullptr, nullptr, 0, out);
    return read_count(c, c->ctx->stream, out);
}

extern "C" int pcq_collector_points(pcq_collector *c, pcq_point *out, uint64_t cap, uint64_t *out_n) {
    PCQ_ON_DEVICE_OF_COLLECTOR(c);
    if (!c || !out_n) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_points: null argument");
    *out_n = 0;
    if (c->kind == COLL_COUNT) return PCQ_OK;  // points() is None (collect_points.rs:87-93)
    int rc = pcq_collector_wait_last(c, c->ctx->stream);
    if (rc) return rc;
    if (c->kind == COLL_GRID) return pcq_grid_drain(c, out, nullptr, cap, out_n);
    uint64_t n_points = 0;
    rc = read_count(c, c->ctx->stream, &n_points);
    if (rc) return rc;
    *out_n = n_points;
    if (!out || n_points == 0) return PCQ_OK;
    if (cap < n_points)
        return pcq_fail(PCQ_ERR_CAPACITY, "buffer collector holds %llu points, capacity %llu",
                        (unsigned long long)n_points, (unsigned long long)cap);
    PCQ_HIP(hipMemcpy(out, c->d_points, n_points * 31, hipMemcpyDeviceToHost));
    return PCQ_OK;
}

extern "C" int pcq_collector_grid_cells(pcq_collector *c, uint64_t *out, uint64_t cap, uint64_t *out_n) {
    PCQ_ON_DEVICE_OF_COLLECTOR(c);
    if (!c || !out_n) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_grid_cells: null argument");
    if (c->kind != COLL_GRID) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_grid_cells: not a grid collector");
    return pcq_grid_drain(c, nullptr, out, cap, out_n);
}

extern "C" int pcq_collector_grid_params(const pcq_collector *c, uint64_t dims[3], uint64_t bits[3]) {
    if (!c || c->kind != COLL_GRID || !dims || !bits) return pcq_fail(PCQ_ERR_ARG, "pcq_collector_grid_params: not a grid collector");
    for (int a = 0; a < 3; a++) dims[a] = c->dims[a], bits[a] = c->bits[a];
    return PCQ_OK;
}

// ---------------------------------------------------------------------------------------------
// scan over device-resident columns
// ---------------------------------------------------------------------------------------------
int pcq_validate_scan(const pcq_columns *cols, const pcq_predicate *pred, const pcq_collector *c) {
    if (!cols || !pred || !c) return pcq_fail(PCQ_ERR_ARG, "scan: null argument");
    if (pred->kind != PCQ_PRED_BOUNDS && pred->kind != PCQ_PRED_CLASS && pred->kind != PCQ_PRED_BOUNDS_F64 && pred->kind != PCQ_PRED_TIME &&
        !pred_is_combined(pred->kind))
        return pcq_fail(PCQ_ERR_ARG, "scan: bad predicate kind %d", pred->kind);
    if (cols->n == 0) return PCQ_OK;
    // index arithmetic (n * stride, first_index + n) must stay far from 2^64: a LAS record length is a u16
    // and 2^40 points is ~3 orders of magnitude beyond the largest dataset of the reference
    if (cols->n > (1ull << 40) || cols->first_index > (1ull << 62))
        return pcq_fail(PCQ_ERR_ARG, "scan: %llu points (first index %llu) is out of range", (unsigned long long)cols->n,
                        (unsigned long long)cols->first_index);
    if (cols->xyz_stride > 65535 || cols->cls_stride > 65535 || cols->rgb_stride > 65535)
        return pcq_fail(PCQ_ERR_ARG, "scan: column stride above 65535");
    const ScanNeeds need = scan_needs(pred->kind, c->kind);  // (stage_plan.h: the host scans move exactly these columns)
    if (need.xyz && (!cols->xyz || cols->xyz_stride < 12)) return pcq_fail(PCQ_ERR_ARG, "scan: positions column missing or stride < 12");
    if (need.cls && (!cols->cls || cols->cls_stride < need.cls_w))
        return pcq_fail(PCQ_ERR_ARG, need.cls_w == 8 ? "scan: time column missing or stride < 8" : "scan: classification column missing");
    // (a time record has no colour: rgb is ignored then; otherwise a colour column is checked even where it is not read)
    if (!pred_tests_time(pred->kind) && cols->rgb && cols->rgb_stride < 6) return pcq_fail(PCQ_ERR_ARG, "scan: colour stride < 6");
    return PCQ_OK;
}

static DevCols to_dev_cols(const pcq_columns *cols) {
    DevCols d;
    d.xyz = (const uint8_t *)cols->xyz;
    d.cls = (const uint8_t *)cols->cls;
    d.rgb = (const uint8_t *)cols->rgb;
    d.xyz_stride = cols->xyz_stride;
    d.cls_stride = cols->cls_stride;
    d.rgb_stride = cols->rgb_stride;
    d.n = cols->n;
    d.first_index = cols->first_index;
    for (int a = 0; a < 3; a++) d.scale[a] = cols->scale[a], d.offset[a] = cols->offset[a];
    return d;
}

// Count of matches into *d_count (+=), choosing the fast kernels where the layout allows.
static int count_into(pcq_ctx *ctx, const DevCols &dc, const DevPred &dp, uint64_t *d_count, hipStream_t s) {
    if (dc.n == 0) return PCQ_OK;
    if (pred_has_box(dp.kind)) {  // BOUNDS, and the combined kinds: K1 (with a second column) over LAST blocks
        if (dp.empty) return PCQ_OK;
        // the combined kinds' second column: packed class bytes (any alignment) or packed, 8-byte aligned times
        const uint64_t w = dp.kind == PCQ_PRED_BOUNDS_TIME ? 8 : 1;
        const bool col_ok = dp.kind == PCQ_PRED_BOUNDS || (dc.cls_stride == w && ((uintptr_t)dc.cls & (w - 1)) == 0);
        if (dc.xyz_stride == 12 && ((uintptr_t)dc.xyz & 3) == 0 && col_ok) {
            // peel the (at most 3) points in front of the first 16-byte aligned point boundary
            uint64_t head = ((uintptr_t)dc.xyz & 15) / 4;  // 12*head == -addr (mod 16)
            if (head > dc.n) head = dc.n;
            if (head) {
                DevCols h = dc;
                h.n = head;
                int rc = pcq_launch_generic_count(ctx, h, dp, d_count, s);
                if (rc) return rc;
            }
            if (dp.kind == PCQ_PRED_BOUNDS) return pcq_launch_bounds_count_xyz12(ctx, dc.xyz + 12 * head, dc.n - head, dp, d_count, s);
            return pcq_launch_bounds_count_xyz12_col(ctx, dc.xyz + 12 * head, dc.cls + w * head, dc.n - head, dp, d_count, s);
        }
        return pcq_launch_generic_count(ctx, dc, dp, d_count, s);
    }
    if (dp.kind == PCQ_PRED_BOUNDS_F64) return pcq_launch_generic_count(ctx, dc, dp, d_count, s);
    if (dp.kind == PCQ_PRED_TIME) {  // K3 over a packed, 8-byte aligned column; LAS records and unaligned blocks: the strided kernel
        if (dc.cls_stride == 8 && ((uintptr_t)dc.cls & 7) == 0) return pcq_launch_time_count_f64(ctx, dc.cls, dc.n, dp, d_count, s);
        return pcq_launch_generic_count(ctx, dc, dp, d_count, s);
    }
    if (dc.cls_stride == 1) return pcq_launch_class_count_u8(ctx, dc.cls, dc.n, (uint8_t)dp.cls, d_count, s);
    return pcq_launch_generic_count(ctx, dc, dp, d_count, s);
}

// Room for `incoming` more points.  The host knows only an upper bound of the points held (every scanned point may have
// matched); while that bound fits the buffer nothing is asked of the device.  When it does not, the true count is read
// (one synchronisation), and the buffer grows only if the truth needs it.
static int buffer_reserve(pcq_collector *c, uint64_t incoming, hipStream_t s) {
    if (c->n_upper + incoming <= c->cap_points) return PCQ_OK;
    pcq_ctx *ctx = c->ctx;
    uint64_t have = 0;
    int rc = pcq_collector_wait_last(c, s);
    if (!rc) rc = read_count(c, s, &have);
    if (rc) return rc;
    if (have + incoming <= c->cap_points) return PCQ_OK;
    uint64_t cap = 2 * c->cap_points;  // geometric growth, but never beyond what is asked for when that is more
    if (cap < have + incoming) cap = have + incoming;
    if (cap < 4096) cap = 4096;
    void *nb = nullptr;
    rc = pcq_pool_alloc(ctx, cap * 31 + 16, &nb);
    if (rc) return rc;
    if (have) PCQ_HIP(hipMemcpyAsync(nb, c->d_points, have * 31, hipMemcpyDeviceToDevice, s));
    PCQ_HIP(hipStreamSynchronize(s));
    pcq_pool_free(ctx, c->d_points);
    c->d_points = (uint8_t *)nb;
    c->cap_points = cap;
    return PCQ_OK;
}

// The per-context scratch (partial counts, tile offsets, the grid's count table, the segment table) is shared by all
// scans of the context and ordered only by the stream they run on: when a scan arrives on a different stream than the
// previous one, the previous stream is drained first (one stream in flight per context).
int pcq_scratch_stream(pcq_ctx *ctx, hipStream_t s) {
    if (ctx->scratch_stream && ctx->scratch_stream != s) PCQ_HIP(hipStreamSynchronize(ctx->scratch_stream));
    ctx->scratch_stream = s;
    return PCQ_OK;
}

int pcq_scan_dev_impl(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c, hipStream_t s, const EmitIndex *ix) {
    int rc = pcq_validate_scan(cols, pred, c);
    if (rc) return rc;
    if (cols->n == 0) return PCQ_OK;
    rc = pcq_scratch_stream(ctx, s);
    if (rc) return rc;
    DevPred dp;
    rc = pcq_make_dev_pred(pred, &dp);
    if (rc) return rc;
    DevCols dc = to_dev_cols(cols);
    if (pred_tests_time(dp.kind)) dc.rgb = nullptr, dc.rgb_stride = 0;  // a time record's colour is (0,0,0) (las.rs:345-355)
    c->last_stream = s;
    switch (c->kind) {
    case COLL_COUNT:
        return count_into(ctx, dc, dp, c->d_count, s);
    case COLL_BUFFER: {
        if (pred_has_box(dp.kind) && dp.empty) return PCQ_OK;
        rc = buffer_reserve(c, dc.n, s);
        if (rc) return rc;
        rc = pcq_launch_emit_points(ctx, dc, dp, c->d_points, c->d_count + c->count_slot, c->d_count + (c->count_slot ^ 1), s, ix);  // asynchronous: one pass, no count first
        if (rc) return rc;
        c->count_slot ^= 1;
        c->n_upper += dc.n;
        return PCQ_OK;
    }
    case COLL_GRID: {
        if (pred_has_box(dp.kind) && dp.empty) return PCQ_OK;
        return pcq_grid_scan(ctx, c, dc, dp, s);  // asynchronous: the matches are partitioned now and folded when a result is asked for
    }
    }
    return pcq_fail(PCQ_ERR_ARG, "scan: unknown collector kind");
}

extern "C" int pcq_scan_dev(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev: null context");
    return pcq_scan_dev_impl(ctx, cols, pred, c, stream ? (hipStream_t)stream : ctx->stream);
}
