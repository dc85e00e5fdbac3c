// scan_count.hip — the count-only fast paths of the predicate scan (kernels K1 and K2).
//
// K1 bounds_count restates the loop of search_last_file_by_bounds_optimized
//    (query/src/search/last.rs:117-135) feeding a CountCollector (collect_points.rs:83-85):
//    count of points with lmin <= (x,y,z) <= lmax over the LAST positions block, N x {i32 x,y,z}.
// K2 class_count restates search_last_file_by_classification_optimized (last.rs:253-262):
//    count of classification bytes equal to `cls` over the LAST classification block, N x u8.
//
// Both are pure HBM streaming reads (12 B/point, 1 B/point): no MFMA, no reuse.  Design for gfx950:
//  * every global load is a fully coalesced 16 B/lane access (1 KiB per wave-instruction),
//    issued non-temporal (the stream is read once);
//  * a 12-byte point is not a power of two, so a wave owns a 768-dword tile (= 256 whole points,
//    3 KiB) loaded by three dwordx4 instructions; instead of transposing through LDS, each dword is
//    range-tested against the bound of ITS component ((k + lane + j) mod 3, rotated per lane once)
//    and the 64-bit compare masks (wave64: v_cmp writes an SGPR pair) are combined with scalar
//    shifts/ANDs into "three consecutive dwords pass" bits, popcounted with s_bcnt1 — the VALU sees
//    two instructions per dword, everything else runs on the scalar unit;
//  * ONE-WAVE workgroups, three (class: four) per CU, persistent, software-pipelined by hand: the loads
//    of the next step are in flight (inline-asm global_load_dwordx4 nt + counted s_waitcnt) while the
//    current step is evaluated; per-workgroup partial counts are written with plain stores and folded by
//    a 1-block finishing kernel, so no same-address atomic storm at the tail.
// K1 also counts the combined kinds over LAST blocks (PCQ_PRED_BOUNDS_CLASS / _TIME): the same kernel with a compile-time
//    second column (COL_U8: the class block, COL_F64: the time block), whose loads ride in the same software pipeline.  Each
//    tile's 256 class bytes (one dword per lane) or 256 times (two dwordx4 per lane) are tested per lane into a verdict word;
//    one ds_bpermute per (load, start phase) brings each point's verdict to the lane that holds its first dword, where it is
//    ANDed into the mask algebra before the popcount.  13 / 20 B per point.
// The loop of the software pipeline is written out in the kernels of this file, in the multi-box count and in three rasters: a
//    shared driver with every kernel as a stage object compiled to the same vector code, but its other scalar code measured slower
//    than this form in alternated runs ("The software pipeline").  Nine kernels that walk a segment table with seg_seek
//    share pipe_scan (scan_tiles.h), which takes only the eval as a callable, came out of the compiler structurally as the loops it
//    replaced and measured as fast ("One pipeline driver for the batched scans"); three rasters did not and keep their
//    loops.  The register sets, their loads and their counted waits are shared (scan_tiles.h: PipeRegs, VecRegs).
// The batched K1 (k_bounds_count_batch_pipe<TILES, Col...>, on pipe_scan) and the host side of its launch
//    (k1_batch_launch, scan_batch_host.h) live in headers: pcq_scan_dev_count_batch below launches the box kind, scan_count_batch.hip the two
//    kinds with a second column.  The batched K2 and the per-file kernels are here; the finish reduction of every count is
//    pcq_launch_finish_counts (scan_count_multi.hip).
// The kernel shapes these replaced (256-thread blocks, unpipelined one-wave forms, other tile counts) live
// in csrc/lab/scan_count_lab.hip and are built only into libpcq_lab.so for the sweeps in tools/.
#include <vector>

#include "pcq_internal.h"
#include "scan_batch_host.h"
#include "scan_tiles.h"

namespace {

// the second column's address out of K1's last argument (scan_tiles.h: ClassBytes, GpsTimes), none: null
__device__ __forceinline__ const uint8_t *col_ptr() { return nullptr; }
template <typename C>
__device__ __forceinline__ const uint8_t *col_ptr(C c) { return c.p; }

template <int TILES, typename... Col>
__global__ __launch_bounds__(64) void k_bounds_count_w1_pipe(const v4i *__restrict__ base, uint64_t n, DevPred pred,
                                                             uint64_t *__restrict__ partials, Col... col) {
    constexpr int COL = ColOf<Col...>::value;
    static_assert(sizeof...(Col) <= 1, "one second column at most");
    const int lane = threadIdx.x;
    const uint64_t tiles = n / TILE_POINTS, steps = tiles / TILES, stride = gridDim.x;
    const LaneBox lb = rotate_box(pred.lo, pred.width, lane);
    const Col2<COL> c2 = col2_setup(col_ptr(col...), pred, lane, IntC<COL>{});
    constexpr int LOADS = TILES * (3 + col2_loads(COL));  // per register set
    uint64_t total = 0;
    if (blockIdx.x < steps) {
        PipeRegs<TILES, COL> A, B;
        uint64_t g = blockIdx.x;
        pipe_load<TILES, COL>(A, base, g, lane, c2);
        for (;;) {
            const uint64_t g1 = g + stride;
            pipe_load<TILES, COL>(B, base, g1 < steps ? g1 : g, lane, c2);  // clamped at the tail: a re-read that hits L2
            pipe_wait<LOADS>(A);                                 // A has landed, B's loads stay in flight
            total += pipe_eval<TILES, COL>(A, lb, c2);
            if (g1 >= steps) break;
            const uint64_t g2 = g1 + stride;
            pipe_load<TILES, COL>(A, base, g2 < steps ? g2 : g1, lane, c2);
            pipe_wait<LOADS>(B);
            total += pipe_eval<TILES, COL>(B, lb, c2);
            if (g2 >= steps) break;
            g = g2;
        }
        pipe_wait<0>(A);  // the clamped tail prefetch is still in flight: land it before the registers die
        pipe_wait<0>(B);
    }
    if (blockIdx.x == 0) {
        for (uint64_t t = steps * TILES; t < tiles; t++) {
            if constexpr (COL == COL_NONE) {
                total += tile_count_masks(base + t * 192, lane, lb);
            } else {
                const v4i *tile = base + t * 192;
                const v4i v[3] = {tile[lane], tile[64 + lane], tile[128 + lane]};
                Col2Regs<COL> r;
                col2_load_plain(r, c2, t);
                total += tile_count_regs<COL>(v, lb, c2, verdict_word(r, c2));
            }
        }
        for (int k = 0; k < 4; k++) {
            const uint64_t p = tiles * TILE_POINTS + (uint64_t)(64 * k + lane);
            bool pass = false;
            if (p < n) {
                const int *q = reinterpret_cast<const int *>(base) + 3 * p;
                pass = ((uint32_t)(q[0] - pred.lo[0]) <= pred.width[0]) & ((uint32_t)(q[1] - pred.lo[1]) <= pred.width[1]) &
                       ((uint32_t)(q[2] - pred.lo[2]) <= pred.width[2]);
                if constexpr (COL != COL_NONE) pass = pass && col2_point(c2, p);
            }
            total += (uint64_t)__popcll(__ballot(pass));
        }
    }
    if (lane == 0) partials[blockIdx.x] = total;
}

// The class segments live in the same device table as the bounds segments, at DevSegment pitch.
__device__ __forceinline__ const DevClassSegment &cseg(const DevSegment *raw, int i) {
    return *reinterpret_cast<const DevClassSegment *>(raw + i);
}

// Batched K2, one wave per workgroup, LOADS 1 KiB loads per step (VecRegs), software-pipelined like k_bounds_count_batch_pipe.
template <int LOADS>
__device__ __forceinline__ uint32_t class_eval(const VecRegs<LOADS> &R, uint32_t pat) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < LOADS; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) c += __popc(zero_bytes((uint32_t)R.r[k][j] ^ pat));
    return c;
}
struct ClassCursor {
    int s;
    uint64_t begin, end;
    const v4i *body;
    uint32_t pat;
};
template <int LOADS>
__device__ __forceinline__ void class_seek(ClassCursor &c, const DevSegment *__restrict__ raw, int nseg, uint64_t u) {
    if (u < c.end) return;
    while (c.s + 1 < nseg && u >= cseg(raw, c.s + 1).tile_begin) c.s++;
    c.begin = cseg(raw, c.s).tile_begin;
    c.end = c.begin + cseg(raw, c.s).nvec / (64ull * LOADS);
    c.body = reinterpret_cast<const v4i *>(cseg(raw, c.s).cls + cseg(raw, c.s).head);
    c.pat = cseg(raw, c.s).pat;
}

template <int LOADS>
__global__ __launch_bounds__(64) void k_class_count_batch_pipe(const DevSegment *__restrict__ raw, int nseg, uint64_t total_steps,
                                                              uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_VEC = 64 * LOADS;
    const int lane = threadIdx.x;
    const uint64_t stride = gridDim.x;
    uint32_t cnt = 0;
    if (blockIdx.x < total_steps) {
        VecRegs<LOADS> A, B;
        ClassCursor ca = {0, 0, 0, nullptr, 0}, cb;
        uint64_t u = blockIdx.x;
        class_seek<LOADS>(ca, raw, nseg, u);
        vec_load(A, ca.body + (u - ca.begin) * STEP_VEC, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            cb = ca;
            if (u1 < total_steps) class_seek<LOADS>(cb, raw, nseg, u1);
            vec_load(B, cb.body + ((u1 < total_steps ? u1 : u) - cb.begin) * STEP_VEC, lane);
            pipe_wait<LOADS>(A);
            cnt += class_eval<LOADS>(A, ca.pat);
            if (u1 >= total_steps) break;
            const uint64_t u2 = u1 + stride;
            ca = cb;
            if (u2 < total_steps) class_seek<LOADS>(ca, raw, nseg, u2);
            vec_load(A, ca.body + ((u2 < total_steps ? u2 : u1) - ca.begin) * STEP_VEC, lane);
            pipe_wait<LOADS>(B);
            cnt += class_eval<LOADS>(B, cb.pat);
            if (u2 >= total_steps) break;
            u = u2;
        }
        pipe_wait<0>(A);
        pipe_wait<0>(B);
    }
    for (int i = blockIdx.x; i < nseg; i += gridDim.x) {
        const DevClassSegment g = cseg(raw, i);
        const uint8_t c8 = (uint8_t)(g.pat & 0xff);
        const v4i *bd = reinterpret_cast<const v4i *>(g.cls + g.head);
        for (uint64_t v = (g.nvec / STEP_VEC) * STEP_VEC + lane; v < g.nvec; v += 64) {
            const v4i a = bd[v];
#pragma unroll
            for (int j = 0; j < 4; j++) cnt += __popc(zero_bytes((uint32_t)a[j] ^ g.pat));
        }
        if (lane < 16) {
            const uint64_t p = lane;
            if (p < g.head && g.cls[p] == c8) cnt++;
        } else if (lane < 32) {
            const uint64_t p = g.head + 16 * g.nvec + (lane - 16);
            if (p < g.n && g.cls[p] == c8) cnt++;
        }
    }
    uint64_t w = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) w += __shfl_down((unsigned long long)w, off, 64);
    if (lane == 0) partials[blockIdx.x] = w;
}

// Per-file K2 in the same shape: one wave per workgroup, LOADS KiB per step, software-pipelined.
template <int LOADS>
__global__ __launch_bounds__(64) void k_class_count_pipe(const uint8_t *__restrict__ cls, uint64_t n, uint32_t pat, uint64_t head,
                                                        uint64_t nvec, uint64_t *__restrict__ partials) {
    constexpr uint64_t STEP_VEC = 64 * LOADS;
    const int lane = threadIdx.x;
    const v4i *body = reinterpret_cast<const v4i *>(cls + head);
    const uint64_t steps = nvec / STEP_VEC, stride = gridDim.x;
    uint32_t cnt = 0;
    if (blockIdx.x < steps) {
        VecRegs<LOADS> A, B;
        uint64_t u = blockIdx.x;
        vec_load(A, body + u * STEP_VEC, lane);
        for (;;) {
            const uint64_t u1 = u + stride;
            vec_load(B, body + (u1 < steps ? u1 : u) * STEP_VEC, lane);
            pipe_wait<LOADS>(A);
            cnt += class_eval<LOADS>(A, pat);
            if (u1 >= steps) break;
            const uint64_t u2 = u1 + stride;
            vec_load(A, body + (u2 < steps ? u2 : u1) * STEP_VEC, lane);
            pipe_wait<LOADS>(B);
            cnt += class_eval<LOADS>(B, pat);
            if (u2 >= steps) break;
            u = u2;
        }
        pipe_wait<0>(A);
        pipe_wait<0>(B);
    }
    if (blockIdx.x == 0) {
        const uint8_t c8 = (uint8_t)(pat & 0xff);
        for (uint64_t v = steps * STEP_VEC + lane; v < nvec; v += 64) {  // fewer than a step of leftover vectors
            const v4i a = body[v];
#pragma unroll
            for (int j = 0; j < 4; j++) cnt += __popc(zero_bytes((uint32_t)a[j] ^ pat));
        }
        if (lane < 16) {  // head: [0, head)   tail: [head + 16*nvec, n)   (each < 16 bytes)
            const uint64_t p = lane;
            if (p < head && cls[p] == c8) cnt++;
        } else if (lane < 32) {
            const uint64_t p = head + 16 * nvec + (lane - 16);
            if (p < n && cls[p] == c8) cnt++;
        }
    }
    uint64_t w = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) w += __shfl_down((unsigned long long)w, off, 64);
    if (lane == 0) partials[blockIdx.x] = w;
}

}  // namespace

template <typename... Col>
static int launch_k1(pcq_ctx *ctx, const void *d_xyz, uint64_t n, const DevPred &pred, uint64_t *d_count, hipStream_t s, Col... col) {
    if (n == 0 || pred.empty) return PCQ_OK;
    if (((uintptr_t)d_xyz & 15) != 0) return pcq_fail(PCQ_ERR_ARG, "bounds_count_xyz12: positions block must be 16-byte aligned");
    const uint64_t units = n / ((uint64_t)K1_TILES * TILE_POINTS) + 1;
    uint64_t g = (uint64_t)ctx->num_cus * K1_WAVES_PER_CU;
    if (g > units) g = units;
    int rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL((k_bounds_count_w1_pipe<K1_TILES, Col...>), dim3((unsigned)g), dim3(64), 0, s, reinterpret_cast<const v4i *>(d_xyz), n, pred,
                       ctx->d_partials, col...);
    return pcq_launch_finish_counts(ctx, 1, (int)g, d_count, s);
}

int pcq_launch_bounds_count_xyz12(pcq_ctx *ctx, const void *d_xyz, uint64_t n, const DevPred &pred,
                                  uint64_t *d_count, hipStream_t s) {
    return launch_k1(ctx, d_xyz, n, pred, d_count, s);
}

int pcq_launch_bounds_count_xyz12_col(pcq_ctx *ctx, const void *d_xyz, const void *d_col, uint64_t n, const DevPred &pred, uint64_t *d_count,
                                      hipStream_t s) {
    if (pred.kind == PCQ_PRED_BOUNDS_CLASS) return launch_k1(ctx, d_xyz, n, pred, d_count, s, ClassBytes{(const uint8_t *)d_col});
    if (pred.kind != PCQ_PRED_BOUNDS_TIME) return pcq_fail(PCQ_ERR_ARG, "bounds_count_xyz12_col: predicate kind %d", pred.kind);
    if (((uintptr_t)d_col & 7) != 0) return pcq_fail(PCQ_ERR_ARG, "bounds_count_xyz12_col: time block must be 8-byte aligned");
    return launch_k1(ctx, d_xyz, n, pred, d_count, s, GpsTimes{(const uint8_t *)d_col});
}

int pcq_launch_class_count_u8(pcq_ctx *ctx, const void *d_cls, uint64_t n, uint8_t cls, uint64_t *d_count,
                              hipStream_t s) {
    if (n == 0) return PCQ_OK;
    uint64_t head = (uint64_t)((16 - ((uintptr_t)d_cls & 15)) & 15);
    if (head > n) head = n;
    const uint64_t nvec = (n - head) / 16;
    const uint32_t pat = 0x01010101u * (uint32_t)cls;
    uint64_t g = (uint64_t)ctx->num_cus * K2_WAVES_PER_CU;
    const uint64_t steps = nvec / (64 * K2_LOADS) + 1;
    if (g > steps) g = steps;
    int rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_class_count_pipe<K2_LOADS>, dim3((unsigned)g), dim3(64), 0, s, reinterpret_cast<const uint8_t *>(d_cls), n, pat, head,
                       nvec, ctx->d_partials);
    return pcq_launch_finish_counts(ctx, 1, (int)g, d_count, s);
}

// The batched K2: one DevClassSegment per classification block (at DevSegment pitch), steps numbered across them.
static int class_count_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds, size_t nsegments, uint64_t *device_total,
                             hipStream_t s) {
    static_assert(sizeof(DevClassSegment) <= sizeof(DevSegment), "the two segment tables share one buffer");
    std::vector<DevSegment> table(nsegments);
    memset(table.data(), 0, nsegments * sizeof(DevSegment));
    uint64_t steps = 0;
    for (size_t i = 0; i < nsegments; i++) {
        if (preds[i].kind != PCQ_PRED_CLASS) return pcq_fail(PCQ_ERR_ARG, "count_batch: mixed predicate kinds");
        if (cols[i].cls_stride != 1 || (!cols[i].cls && cols[i].n))
            return pcq_fail(PCQ_ERR_ARG, "count_batch: LAST classification blocks only (stride 1)");
        DevClassSegment g;
        memset(&g, 0, sizeof g);
        g.cls = (const uint8_t *)cols[i].cls;
        g.n = cols[i].n;
        g.head = (uint64_t)((16 - ((uintptr_t)g.cls & 15)) & 15);
        if (g.head > g.n) g.head = g.n;
        g.nvec = (g.n - g.head) / 16;
        g.tile_begin = steps;
        g.pat = 0x01010101u * (uint32_t)preds[i].cls;
        memcpy(&table[i], &g, sizeof g);
        steps += g.nvec / (64 * (uint64_t)K2_LOADS);
    }
    // (pcq_upload_segment_table: the table travels only when it differs from the one already in HBM)
    int rc = pcq_upload_segment_table(ctx, PCQ_PRED_CLASS, nsegments, table.data(), nsegments * sizeof(DevSegment), s);
    if (rc) return rc;
    uint64_t g = (uint64_t)ctx->num_cus * K2_WAVES_PER_CU;
    if (g > steps + nsegments) g = steps + nsegments;
    rc = pcq_ensure_partials(ctx, (size_t)g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_class_count_batch_pipe<K2_LOADS>, dim3((unsigned)g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps, ctx->d_partials);
    return pcq_launch_finish_counts(ctx, 1, (int)g, device_total, s);
}

extern "C" int pcq_scan_dev_count_batch(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *preds,
                                        size_t nsegments, uint64_t *device_total, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!cols && nsegments) || (!preds && nsegments) || !device_total)
        return pcq_fail(PCQ_ERR_ARG, "pcq_scan_dev_count_batch: null argument");
    if (nsegments == 0) return PCQ_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    {  // (this entry has always taken the scratch stream before it builds its table: k1_batch_launch's own call then finds it taken)
        const int src = pcq_scratch_stream(ctx, s);
        if (src) return src;
    }
    const int kind = preds[0].kind;
    if (kind == PCQ_PRED_CLASS) return class_count_batch(ctx, cols, preds, nsegments, device_total, s);
    if (kind != PCQ_PRED_BOUNDS) return pcq_fail(PCQ_ERR_ARG, "count_batch: bad predicate kind %d", kind);
    const K1Batch b = {"count_batch", PCQ_PRED_BOUNDS, K1_WAVES_PER_CU, 1, 1, /*null_refused=*/false};
    return k1_batch_launch<DevSegment>(
        ctx, b, cols, nsegments, device_total, s,
        [&](size_t i) { return preds[i].kind != kind ? pcq_fail(PCQ_ERR_ARG, "count_batch: mixed predicate kinds") : (int)PCQ_OK; },
        [&](DevSegment &g, size_t i) {
            DevPred dp;
            const int rc = pcq_make_dev_pred(&preds[i], &dp);
            if (!rc) seg_box(g, dp);
            return rc;
        },
        [&](unsigned g, uint64_t steps) {
            hipLaunchKernelGGL(k_bounds_count_batch_pipe<K1_TILES>, dim3(g), dim3(64), 0, s, ctx->d_segments, (int)nsegments, steps, ctx->d_partials);
            return (int)PCQ_OK;
        });
}
