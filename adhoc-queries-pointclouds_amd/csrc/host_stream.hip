// host_stream.hip — scans over host-resident columns and files: the pinned staging ring (StageRing, pcq_internal.h) and the
// pipeline that moves a scan through it chunk by chunk, hipMemcpyAsync overlapped with the kernels.  The layout of a scan in
// the ring is worked out by stage_plan.h.
#include "pcq_internal.h"

#include <chrono>
#include <cstdlib>

static bool pcq_timing() {
    static const bool timing = getenv("PCQ_TIMING") && getenv("PCQ_TIMING")[0] == '1';
    return timing;
}

// ---------------------------------------------------------------------------------------------
// the staging ring
// ---------------------------------------------------------------------------------------------
int StageRing::init(pcq_ctx *ctx) {
    ctx_ = ctx;
    for (int i = 0; i < 2; i++) {
        PCQ_HIP(hipEventCreateWithFlags(&copied_[i], hipEventDisableTiming));
        PCQ_HIP(hipEventCreateWithFlags(&consumed_[i], hipEventDisableTiming));
    }
    return PCQ_OK;
}

void StageRing::join_prepare() {
    if (prepare_.joinable()) prepare_.join();
}
void StageRing::wait_copy_path() {
    if (copy_warm_.joinable()) copy_warm_.join();
}

int StageRing::drain() {
    const hipError_t e1 = ctx_->stream ? hipStreamSynchronize(ctx_->stream) : hipSuccess;
    const hipError_t e2 = ctx_->copy_stream ? hipStreamSynchronize(ctx_->copy_stream) : hipSuccess;
    set_idle();
    PCQ_HIP(e1);
    PCQ_HIP(e2);
    return PCQ_OK;
}

void StageRing::free_pairs() {
    for (int i = 0; i < 2; i++) {
        if (h_[i]) (void)hipHostFree(h_[i]);
        if (d_[i]) (void)hipFree(d_[i]);
        h_[i] = d_[i] = nullptr;
    }
    bytes_ = 0;
}

void StageRing::drop() {
    join_prepare();
    delete pool_;  // helpers are re-created with or without the affinity
    pool_ = nullptr;
    if (bytes_) {  // and the staging buffers re-allocated on the next scan
        (void)drain();
        free_pairs();
    }
}

void StageRing::destroy() {
    if (!ctx_) return;
    join_prepare();
    wait_copy_path();
    (void)drain();
    drop();
    if (copy_warm_h_) (void)hipHostFree(copy_warm_h_);
    if (copy_warm_d_) (void)hipFree(copy_warm_d_);
    for (int i = 0; i < 2; i++) {
        if (copied_[i]) (void)hipEventDestroy(copied_[i]);
        if (consumed_[i]) (void)hipEventDestroy(consumed_[i]);
    }
}

// `upto` = how many of the pairs the caller needs NOW: a scan asks for the first pair, issues its first chunk, and only then
// for the second — pinning 24 MB is 5 ms (profiles/r03_hip_startup.log: 11 ms for the ring), and the second pair's 5 ms then
// run under the first chunk's transfer instead of in front of it (the first file of a process cost 15-24 ms where the others
// cost 1: profiles/r03_cli_e2e.log).
int StageRing::ensure(size_t bytes, int upto) {
    join_prepare();
    return ensure_now(bytes, upto);
}
int StageRing::ensure_now(size_t bytes, int upto) {
    pcq_ctx *ctx = ctx_;
    if (bytes_ < bytes) {
        if (h_[0] || h_[1]) {  // too small: drop what there is
            int rc = drain();
            if (rc) return rc;
            free_pairs();
        }
        bytes_ = bytes;  // (the size the pairs are allocated with from here on)
    }
    bool need = false;
    for (int i = 0; i < upto; i++) need |= !h_[i];
    if (!need) return PCQ_OK;
    const auto t0 = std::chrono::steady_clock::now();
    // pinned pages are allocated where the allocating thread runs (default "local" policy): run on the GPU's node for it
    cpu_set_t saved;
    const bool rebind = ctx->numa_local && ctx->numa_node >= 0 && sched_getaffinity(0, sizeof saved, &saved) == 0 &&
                        sched_setaffinity(0, sizeof ctx->node_cpus, &ctx->node_cpus) == 0;
    hipError_t e = hipSuccess;
    for (int i = 0; i < upto && e == hipSuccess; i++) {
        if (h_[i]) continue;
        uint8_t *h = nullptr, *d = nullptr;
        e = hipHostMalloc((void **)&h, bytes_, hipHostMallocDefault);  // (pinned = resident: the pages exist when this returns)
        if (e == hipSuccess && (e = hipMalloc((void **)&d, bytes_)) != hipSuccess) (void)hipHostFree(h);  // no half pair
        if (e == hipSuccess) h_[i] = h, d_[i] = d;
    }
    if (rebind) (void)sched_setaffinity(0, sizeof saved, &saved);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return pcq_fail(PCQ_ERR_HIP, "staging allocation failed: %s", hipGetErrorString(e));
    }
    if (pcq_timing())
        fprintf(stderr, "[pcq] staging pair(s) up to %d of %zu MB pinned + device in %.1f ms\n", upto, bytes_ >> 20,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return PCQ_OK;
}

// The copy is split over the context's helper threads (copy_pool.h).
void StageRing::ensure_pool_now() {
    pcq_ctx *ctx = ctx_;
    if (!pool_ || pool_->helpers() != ctx->copy_threads - 1) {
        delete pool_;
        pool_ = new CopyPool(ctx->copy_threads - 1, ctx->numa_local && ctx->numa_node >= 0 ? &ctx->node_cpus : nullptr);
    }
}

void StageRing::prepare() {
    if (prepare_.joinable() || h_[0]) return;  // under way, or nothing left to prepare
    prepare_ = std::thread([this] {
        (void)hipSetDevice(ctx_->device);
        // (what a scan of positions + classes asks for: scan_host_impl.  BOTH pairs: with only the first one pinned here the scan pins
        // the second on a thread of its own while a third sets the copy path up, and its first launch waits for the two of them inside
        // the runtime — first file 14 -> 17.7 ms, profiles/r04_cli_first_file.log)
        (void)ensure_now((size_t)ctx_->chunk_points * 12 + 4096, 2);
        ensure_pool_now();
    });
}

// The first LARGE host-to-device copy of a process takes 8 ms inside the call (the runtime sets its copy path up; the later
// ones take microseconds; a copy of 8 bytes does not do it: profiles/r04_cli_first_file.log).  copy_path_ready() spends them
// on a thread of its own — one pinned megabyte through hipMemcpyAsync on the copy stream — while the context's first scan
// reads its chunks in place; whoever uses the copy stream next joins it first.
bool StageRing::copy_path_ready() {
    if (copy_warm_state_.load() == 2) return true;
    int expected = 0;
    if (!copy_warm_state_.compare_exchange_strong(expected, 1)) return false;
    copy_warm_ = std::thread([this] {
        pcq_ctx *ctx = ctx_;
        (void)hipSetDevice(ctx->device);
        const size_t bytes = 1u << 20;
        if (hipHostMalloc(&copy_warm_h_, bytes, hipHostMallocDefault) == hipSuccess && hipMalloc(&copy_warm_d_, bytes) == hipSuccess &&
            hipMemcpyAsync(copy_warm_d_, copy_warm_h_, bytes, hipMemcpyHostToDevice, ctx->copy_stream) == hipSuccess)
            (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipGetLastError();
        copy_warm_state_.store(2);
    });
    return false;
}

// Copies `bytes` from the host source into pinned memory: memcpy from caller memory, or — when the
// columns are given as offsets into an open file (pcq_scan_fd) — pread straight from the page cache
// (no mmap page-table work: measured ~2x the rate of memcpy from a freshly mmapped file).
int StageRing::fetch(int fd, uint8_t *dst, const uint8_t *src, size_t bytes) {
    join_prepare();
    ensure_pool_now();
    const int r = pool_->run(fd, dst, src, bytes);
    if (r < 0) return pcq_fail(PCQ_ERR_IO, "pread failed: %s", strerror(-r));
    if (r > 0) return pcq_fail(PCQ_ERR_EOF, "failed to fill whole buffer");
    return PCQ_OK;
}

int StageRing::copy_out(int b, void *d_dst, size_t bytes) {
    PCQ_HIP(hipMemcpyAsync(d_dst, h_[b], bytes, hipMemcpyHostToDevice, ctx_->copy_stream));
    PCQ_HIP(hipEventRecord(copied_[b], ctx_->copy_stream));
    return PCQ_OK;
}
int StageRing::wait_copied(int b, hipStream_t s) {
    PCQ_HIP(hipStreamWaitEvent(s, copied_[b], 0));
    return PCQ_OK;
}
int StageRing::host_wait_copied(int b) {
    PCQ_HIP(hipEventSynchronize(copied_[b]));
    return PCQ_OK;
}
int StageRing::wait_free(int b) {
    if (busy_[b]) {
        PCQ_HIP(hipEventSynchronize(consumed_[b]));
        busy_[b] = false;
    }
    return PCQ_OK;
}
int StageRing::mark_busy(int b, hipStream_t s) {
    PCQ_HIP(hipEventRecord(consumed_[b], s));
    busy_[b] = true;
    return PCQ_OK;
}

extern "C" int pcq_prepare_host_scans(pcq_ctx *ctx) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_prepare_host_scans: null context");
    ctx->ring.prepare();
    return PCQ_OK;
}

// ---------------------------------------------------------------------------------------------
// a file range into device memory
// ---------------------------------------------------------------------------------------------
int pcq_stream_fd_to_device(pcq_ctx *ctx, int fd, uint64_t offset, uint64_t bytes, uint8_t *d_dst) {
    StageRing &ring = ctx->ring;
    const size_t chunk = 32u << 20;
    int rc = ring.ensure((bytes < chunk ? (size_t)bytes : chunk) + 64);
    if (rc) return rc;
    ring.wait_copy_path();
    if (ring.busy()) {  // a nowait scan may still be reading the staging buffers
        PCQ_HIP(hipStreamSynchronize(ctx->stream));
        ring.set_idle();
    }
    const uint64_t nchunks = (bytes + chunk - 1) / chunk;
    for (uint64_t k = 0; k < nchunks && !rc; k++) {
        const int b = (int)(k & 1);
        const uint64_t at = k * chunk, len = bytes - at < chunk ? bytes - at : chunk;
        if (k >= 2) rc = ring.host_wait_copied(b);  // staging buffer b has been copied out
        if (!rc) rc = ring.fetch(fd, ring.host(b), (const uint8_t *)(uintptr_t)(offset + at), (size_t)len);
        if (!rc) rc = ring.copy_out(b, d_dst + at, (size_t)len);
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->copy_stream);  // (what was queued reads the staging buffers)
        return rc;
    }
    PCQ_HIP(hipStreamSynchronize(ctx->copy_stream));
    return PCQ_OK;
}

extern "C" int pcq_read_fd_to_device(pcq_ctx *ctx, int fd, uint64_t file_offset, uint64_t bytes, void *d_dst) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || fd < 0 || (!d_dst && bytes)) return pcq_fail(PCQ_ERR_ARG, "pcq_read_fd_to_device: bad argument");
    if (bytes == 0) return PCQ_OK;
    return pcq_stream_fd_to_device(ctx, fd, file_offset, bytes, (uint8_t *)d_dst);
}

// ---------------------------------------------------------------------------------------------
// scan over host-resident columns: pinned double buffers + hipMemcpyAsync overlapped with kernels
// ---------------------------------------------------------------------------------------------
static int scan_host_impl(pcq_ctx *ctx, int fd, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c, bool wait) {
    if (!ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_host: null context");
    int rc = pcq_validate_scan(cols, pred, c);
    if (rc) return rc;
    if (cols->n == 0) return PCQ_OK;
    PCQ_HIP(hipSetDevice(ctx->device));

    const StagePlan pl = stage_plan(*cols, pred->kind, c->kind, ctx->chunk_points);
    if (!pl.ok) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_host: columns must be packed blocks (LAST) or one interleaved record (LAS)");
    const uint64_t chunk = pl.chunk;
    const uint8_t *hx = (const uint8_t *)cols->xyz, *hc = (const uint8_t *)cols->cls, *hr = (const uint8_t *)cols->rgb;
    const uint8_t *aos_base = (const uint8_t *)pl.aos_base;
    StageRing &ring = ctx->ring;

    const bool first_scan = pcq_timing() && !ctx->scanned_before;
    ctx->scanned_before = true;
    const auto t_scan = std::chrono::steady_clock::now();
    auto stamp = [&](const char *what) {
        if (first_scan) fprintf(stderr, "[pcq] first scan of the context: %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_scan).count());
    };
    rc = ring.ensure(pl.stage_need, 1);  // (the second pair: behind the first chunk, below)
    if (rc) return rc;
    stamp("first staging pair ready");

    hipStream_t s = ctx->stream;
    const uint64_t nchunks = (cols->n + chunk - 1) / chunk;

    // A scan that reads every byte ONCE — count and grid collectors — reads the pinned ring in place: the kernels stream host
    // memory over PCIe at the rate the copy engine moves it (59 against 54.5 GB/s for a count, 56.5 against 50.1 for a grid
    // scan: profiles/r04_zero_copy.log), the chunk is not written to and read from HBM in between, and the process never sets
    // up its copy path (8 ms inside the first large hipMemcpyAsync: profiles/r04_cli_first_file.log) — but on a stream of files the
    // copy engine is a tenth faster (median file of 240 MB: 5.5 against 6.6 ms).  So, by default (host_in_place 2), the scans of
    // a context read in place WHILE a thread sets the copy path up, and copy from then on.  The buffer collector reads the
    // positions twice (count pass, emit pass): it always keeps the device twin.
    bool in_place = false;
    if (c->kind != COLL_BUFFER && ctx->host_in_place == 1) in_place = true;
    // (the NEXT scan copies: 5.5 ms per 240 MB file against 6.6 in place, once the copy path exists)
    if (c->kind != COLL_BUFFER && ctx->host_in_place == 2 && !ring.copy_path_ready()) in_place = true;
    if (!in_place) ring.wait_copy_path();  // (nobody else is on the copy stream)
    auto stage = [&](uint64_t k) -> int {
        const int b = (int)(k & 1);
        const uint64_t first = k * chunk;
        const uint64_t cnt = cols->n - first < chunk ? cols->n - first : chunk;
        // the kernels of the chunk that used staging pair b last (this call's or an earlier nowait call's) are done with it
        int frc = ring.wait_free(b);
        if (frc) return frc;
        uint8_t *h = ring.host(b);
        const size_t bytes = pl.bytes(cnt);
        if (pl.aos) {
            frc = ring.fetch(fd, h, aos_base + first * pl.stride, bytes);
        } else {
            if (pl.need_xyz) frc = ring.fetch(fd, h + pl.off_xyz, hx + first * 12, (size_t)cnt * 12);
            if (!frc && pl.need_cls) frc = ring.fetch(fd, h + pl.off_cls, hc + first * pl.w, (size_t)cnt * pl.w);
            if (!frc && pl.need_rgb) frc = ring.fetch(fd, h + pl.off_rgb, hr + first * 6, (size_t)cnt * 6);
        }
        if (frc) return frc;
        if (k == 0) stamp("first chunk read into the staging buffer");
        if (in_place) return PCQ_OK;  // (the kernels read it where it is)
        frc = ring.copy_out(b, ring.dev(b), bytes);
        if (frc) return frc;
        if (k == 0) stamp("first transfer issued");
        return PCQ_OK;
    };

    // every error exit below goes through fail(): queued copies and kernels drain before the staging buffers (or the caller's
    // memory) can be touched again, and no staging pair stays marked busy
    auto fail = [&](int code) {
        (void)ring.drain();
        return code;
    };
    // The second pair is pinned by a thread of this call WHILE the first chunk is read into the first pair (4 ms each, the
    // first scan of a context only; joined before anything else happens).
    int rc2 = PCQ_OK;
    std::thread second_pair;
    if (nchunks > 1 && !ring.host(1))
        second_pair = std::thread([&] {
            (void)hipSetDevice(ctx->device);
            rc2 = ring.ensure(pl.stage_need, 2);
        });
    rc = stage(0);
    if (second_pair.joinable()) second_pair.join();
    if (rc) return fail(rc);
    if (rc2) return fail(pcq_fail(PCQ_ERR_HIP, "staging allocation failed (second pair)"));
    stamp("first chunk read and its transfer issued, second staging pair ready");
    if (nchunks > 1) {
        rc = ring.ensure(pl.stage_need, 2);  // (no-op unless the pair above was not asked for)
        if (rc) return fail(rc);
    }
    for (uint64_t k = 0; k < nchunks; k++) {
        const int b = (int)(k & 1);
        const uint64_t first = k * chunk;
        const uint64_t cnt = cols->n - first < chunk ? cols->n - first : chunk;
        if (!in_place && (rc = ring.wait_copied(b, s))) return fail(rc);
        pcq_columns dcols = *cols;
        const uint8_t *d = in_place ? ring.host(b) : ring.dev(b);
        if (pl.aos) {
            dcols.xyz = pl.need_xyz ? d + (hx - aos_base) : nullptr;
            dcols.cls = pl.need_cls ? d + (hc - aos_base) : nullptr;
            dcols.rgb = pl.need_rgb ? d + (hr - aos_base) : nullptr;
        } else {
            dcols.xyz = pl.need_xyz ? d + pl.off_xyz : nullptr;
            dcols.cls = pl.need_cls ? d + pl.off_cls : nullptr;
            dcols.rgb = pl.need_rgb ? d + pl.off_rgb : nullptr;
        }
        dcols.n = cnt;
        dcols.first_index = cols->first_index + first;
        rc = pcq_scan_dev_impl(ctx, &dcols, pred, c, s);
        if (!rc) rc = ring.mark_busy(b, s);
        if (rc) return fail(rc);
        if (k == 0) stamp("first chunk's kernels launched");
        if (k + 1 < nchunks) {  // the next chunk is read while this one's kernels run (in place: while they read this one over PCIe)
            rc = stage(k + 1);
            if (rc) return fail(rc);
        }
    }
    if (wait) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(pcq_fail(PCQ_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e)));
        ring.set_idle();
    }
    stamp(wait ? "last chunk done" : "last chunk's kernels launched (not waited for)");
    return PCQ_OK;
}

extern "C" int pcq_scan_host(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    return scan_host_impl(ctx, -1, cols, pred, c, true);
}

extern "C" int pcq_scan_host_nowait(pcq_ctx *ctx, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    return scan_host_impl(ctx, -1, cols, pred, c, false);
}

extern "C" int pcq_scan_fd(pcq_ctx *ctx, int fd, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (fd < 0) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_fd: bad file descriptor");
    return scan_host_impl(ctx, fd, cols, pred, c, true);
}

extern "C" int pcq_scan_fd_nowait(pcq_ctx *ctx, int fd, const pcq_columns *cols, const pcq_predicate *pred, pcq_collector *c) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (fd < 0) return pcq_fail(PCQ_ERR_ARG, "pcq_scan_fd_nowait: bad file descriptor");
    return scan_host_impl(ctx, fd, cols, pred, c, false);
}
