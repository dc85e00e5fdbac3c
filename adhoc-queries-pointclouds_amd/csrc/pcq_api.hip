// pcq_api.hip — the C ABI of include/pcq.h: context, device-memory pool, options, memory helpers and the host-side math of
// the boundary.  The collectors and the scan over device columns are in collectors.hip, the host / file scans in host_stream.hip.
//
// Everything here is plumbing around the kernels of scan_count.hip / scan_generic.hip / grid_*.hip.
// There is deliberately no CPU implementation of any scan in this library: if no HIP device is
// usable, pcq_init fails and nothing else can be called.
#include "pcq_internal.h"

#include <unistd.h>

#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <new>

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[1024];

int pcq_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *pcq_last_error(void) { return g_err; }
// a few 64-bit words from device memory into pinned host memory (pcq_copy_to_host)
__global__ void k_words_to_host(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst_pinned, uint32_t n) {
    if (threadIdx.x < n) dst_pinned[threadIdx.x] = src[threadIdx.x];
}

extern "C" int pcq_abi_version(void) { return PCQ_ABI_VERSION; }
static void options_from_env(pcq_ctx *ctx);

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// Which NUMA node is the GPU attached to, and which CPUs belong to it (Linux sysfs; silently unknown elsewhere).
// DMA out of pinned host memory on the GPU's own socket runs at the PCIe rate; across the socket
// interconnect it was measured at about two thirds of it (profiles/r01_file_path_rate.log).
static void detect_numa_node(pcq_ctx *ctx) {
    CPU_ZERO(&ctx->node_cpus);
    ctx->numa_node = -1;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, ctx->device) != hipSuccess) return;
    for (char *p = bus; *p; p++) *p = (char)tolower((unsigned char)*p);
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    if (node < 0) return;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return;
    char list[1024] = {0};
    if (fgets(list, sizeof list, f)) {
        for (char *tok = strtok(list, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
            int a = 0, b = 0;
            const int k = sscanf(tok, "%d-%d", &a, &b);
            if (k == 1) b = a;
            if (k >= 1)
                for (int c = a; c <= b && c < CPU_SETSIZE; c++) CPU_SET(c, &ctx->node_cpus);
        }
    }
    fclose(f);
    if (CPU_COUNT(&ctx->node_cpus) > 0) ctx->numa_node = node;
}

extern "C" int pcq_init(int device, pcq_ctx **out_ctx) {
    if (!out_ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_init: out_ctx is null");
    *out_ctx = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return pcq_fail(PCQ_ERR_HIP, "pcq_init: no HIP device available (%s); this library has no CPU path",
                        e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= ndev) return pcq_fail(PCQ_ERR_ARG, "pcq_init: device %d out of range [0,%d)", device, ndev);
    PCQ_HIP(hipSetDevice(device));
    pcq_ctx *ctx = new (std::nothrow) pcq_ctx();
    if (!ctx) return pcq_fail(PCQ_ERR_NOMEM, "pcq_init: out of memory");
    ctx->device = device;
    e = hipGetDeviceProperties(&ctx->prop, device);
    if (e != hipSuccess) {
        delete ctx;
        return pcq_fail(PCQ_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    }
    ctx->num_cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
    detect_numa_node(ctx);
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess) {
        pcq_shutdown(ctx);
        return pcq_fail(PCQ_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    int rc = ctx->ring.init(ctx);
    if (rc) {
        pcq_shutdown(ctx);
        return rc;
    }
    if ((e = hipMalloc((void **)&ctx->d_scalars, 64 * sizeof(uint64_t))) != hipSuccess ||
        (e = hipHostMalloc((void **)&ctx->h_scalars, 64 * sizeof(uint64_t), hipHostMallocDefault)) != hipSuccess) {
        pcq_shutdown(ctx);
        return pcq_fail(PCQ_ERR_HIP, "scratch allocation: %s", hipGetErrorString(e));
    }
    rc = pcq_ensure_partials(ctx, (size_t)ctx->num_cus * 16);
    if (rc) {
        pcq_shutdown(ctx);
        return rc;
    }
    {  // (not more copy threads than this GPU's share of the host's hardware threads)
        const unsigned hw = std::thread::hardware_concurrency();
        const int share = hw ? (int)(hw / (unsigned)ndev) : ctx->copy_threads;
        if (ctx->copy_threads > share) ctx->copy_threads = share < 2 ? 2 : share;
    }
    options_from_env(ctx);  // tuning / test knobs (same meaning as pcq_set_option)
    *out_ctx = ctx;
    return PCQ_OK;
}

extern "C" int pcq_shutdown(pcq_ctx *ctx) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx) return PCQ_OK;
    (void)hipSetDevice(ctx->device);
    ctx->ring.destroy();  // (joins its threads and drains both streams first)
    pcq_pool_clear(ctx);
    if (ctx->d_partials) (void)hipFree(ctx->d_partials);
    if (ctx->d_scalars) (void)hipFree(ctx->d_scalars);
    if (ctx->h_scalars) (void)hipHostFree(ctx->h_scalars);
    if (ctx->d_segments) (void)hipFree(ctx->d_segments);
    if (ctx->h_segments) (void)hipHostFree(ctx->h_segments);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    delete ctx;
    return PCQ_OK;
}

// ---------------------------------------------------------------------------------------------
// device-memory pool
// ---------------------------------------------------------------------------------------------
int pcq_pool_alloc(pcq_ctx *ctx, size_t bytes, void **out) {
    *out = nullptr;
    if (bytes == 0) bytes = 256;
    PoolBlock *best = nullptr;  // the smallest free block that is large enough, and not wastefully larger
    for (PoolBlock &b : ctx->pool)
        if (!b.used && b.bytes >= bytes && (b.bytes <= 2 * bytes + (64u << 20)) && (!best || b.bytes < best->bytes)) best = &b;
    if (best) {
        best->used = true;
        *out = best->p;
        return PCQ_OK;
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {  // give the free blocks back and try once more
        (void)hipGetLastError();
        for (size_t i = 0; i < ctx->pool.size();) {
            if (!ctx->pool[i].used) {
                (void)hipFree(ctx->pool[i].p);
                ctx->pool.erase(ctx->pool.begin() + (long)i);
            } else {
                i++;
            }
        }
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return pcq_fail(PCQ_ERR_NOMEM, "device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    ctx->pool.push_back(PoolBlock{p, bytes, true});
    if (bytes >= (64u << 20)) {
        static const bool timing = getenv("PCQ_TIMING") && getenv("PCQ_TIMING")[0] == '1';
        if (timing) fprintf(stderr, "pcq: pool block %p (%zu MiB, address mod 2 MiB = %zu KiB)\n", p, bytes >> 20, ((size_t)p & ((2u << 20) - 1)) >> 10);
    }
    *out = p;
    return PCQ_OK;
}

void pcq_pool_free(pcq_ctx *ctx, void *p) {
    if (!p) return;
    uint64_t free_bytes = 0;
    for (PoolBlock &b : ctx->pool) {
        if (b.p == p) b.used = false;
        if (!b.used) free_bytes += b.bytes;
    }
    while (free_bytes > ctx->pool_limit) {  // keep the pool bounded: drop the largest free block
        size_t big = ctx->pool.size();
        for (size_t i = 0; i < ctx->pool.size(); i++)
            if (!ctx->pool[i].used && (big == ctx->pool.size() || ctx->pool[i].bytes > ctx->pool[big].bytes)) big = i;
        if (big == ctx->pool.size()) break;
        free_bytes -= ctx->pool[big].bytes;
        (void)hipFree(ctx->pool[big].p);
        ctx->pool.erase(ctx->pool.begin() + (long)big);
    }
}

void pcq_pool_clear(pcq_ctx *ctx) {
    for (PoolBlock &b : ctx->pool) (void)hipFree(b.p);
    ctx->pool.clear();
}

int pcq_ensure_partials(pcq_ctx *ctx, size_t n) {
    if (n <= ctx->partials_cap) return PCQ_OK;
    if (ctx->scratch_cap_words > 0 && n > (size_t)ctx->scratch_cap_words)  // (tests: an allocation that fails, before anything is freed)
        return pcq_fail(PCQ_ERR_NOMEM, "scratch of %zu words is above the test cap of %lld", n, (long long)ctx->scratch_cap_words);
    // The old buffer may still be referenced by kernels enqueued on the context's or a caller's stream.
    if (ctx->d_partials) {
        PCQ_HIP(hipDeviceSynchronize());
        PCQ_HIP(hipFree(ctx->d_partials));
        ctx->d_partials = nullptr;
        ctx->partials_cap = 0;
    }
    size_t cap = 4096;
    while (cap < n && cap < ((size_t)1 << 22)) cap <<= 1;
    if (cap < n) cap = (n + (((size_t)1 << 22) - 1)) & ~(((size_t)1 << 22) - 1);  // beyond 32 MB: whole 32 MB steps, not the next power of two
    PCQ_HIP(hipMalloc((void **)&ctx->d_partials, cap * sizeof(uint64_t)));
    ctx->partials_cap = cap;
    return PCQ_OK;
}

// The segment tables of the batched count kernels (DevSegment: box, DevClassSegment: class at DevSegment pitch,
// DevCombinedSegment: box AND class, DevBoundsTimeSegment: box AND time, or the time histogram's with its edges behind the
// table, DevRasterSegment: the density raster) share one pinned buffer and its device twin, sized in bytes.
int pcq_ensure_segment_table(pcq_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->segments_cap) return PCQ_OK;
    if (ctx->d_segments) (void)hipFree(ctx->d_segments);
    if (ctx->h_segments) (void)hipHostFree(ctx->h_segments);
    ctx->d_segments = nullptr;
    ctx->h_segments = nullptr;
    ctx->segments_cap = 0;
    ctx->segments_uploaded = 0;
    const size_t cap = bytes < 64 * sizeof(DevCombinedSegment) ? 64 * sizeof(DevCombinedSegment) : bytes;
    PCQ_HIP(hipMalloc((void **)&ctx->d_segments, cap));
    PCQ_HIP(hipHostMalloc((void **)&ctx->h_segments, cap, hipHostMallocDefault));
    ctx->segments_cap = cap;
    return PCQ_OK;
}

// A batched count's table into d_segments, on stream s.  It travels only when it differs from the table already in HBM: a
// repeated query re-launches without touching the pinned buffer, so no host-side wait.  The byte compare alone decides that
// today: a table of another kind has another layout, so its bytes differ; the kind in the key only keeps this true should
// two kinds ever share a layout.
int pcq_upload_segment_table(pcq_ctx *ctx, int kind, size_t nsegments, const void *table, size_t bytes, hipStream_t s) {
    const int rc = pcq_ensure_segment_table(ctx, bytes);
    if (rc) return rc;
    if (ctx->segments_uploaded == nsegments && ctx->segments_kind == kind && memcmp(ctx->h_segments, table, bytes) == 0) return PCQ_OK;
    PCQ_HIP(hipStreamSynchronize(s));  // the previous upload from the pinned table must have been consumed
    memcpy(ctx->h_segments, table, bytes);
    PCQ_HIP(hipMemcpyAsync(ctx->d_segments, ctx->h_segments, bytes, hipMemcpyHostToDevice, s));
    ctx->segments_uploaded = nsegments;
    ctx->segments_kind = kind;
    return PCQ_OK;
}

extern "C" int pcq_get_device_info(pcq_ctx *ctx, pcq_device_info *out) {
    if (!ctx || !out) return pcq_fail(PCQ_ERR_ARG, "pcq_get_device_info: null argument");
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", ctx->prop.name);
    snprintf(out->gcn_arch, sizeof out->gcn_arch, "%s", ctx->prop.gcnArchName);
    out->compute_units = ctx->prop.multiProcessorCount;
    out->wavefront_size = ctx->prop.warpSize;
    out->hbm_bytes = (uint64_t)ctx->prop.totalGlobalMem;
    out->lds_bytes_per_block = (uint64_t)ctx->prop.sharedMemPerBlock;
    out->clock_khz = ctx->prop.clockRate;
    return PCQ_OK;
}

extern "C" void *pcq_ctx_stream(pcq_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int pcq_ctx_synchronize(pcq_ctx *ctx) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_ctx_synchronize: null context");
    return ctx->ring.drain();
}

extern "C" int pcq_bind_thread_near_device(pcq_ctx *ctx) {
    if (!ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_bind_thread_near_device: null context");
    if (ctx->numa_local && ctx->numa_node >= 0) (void)sched_setaffinity(0, sizeof ctx->node_cpus, &ctx->node_cpus);
    return PCQ_OK;
}

// ---------------------------------------------------------------------------------------------
// options (pcq.h: pcq_set_option / pcq_get_option; pcq_init reads the ones marked OPT_ENV from PCQ_<NAME>)
// ---------------------------------------------------------------------------------------------
enum : unsigned {
    OPT_SET = 1,   // settable; without it: a diagnostic, read only
    OPT_BOOL = 2,  // stored as value != 0
    OPT_ENV = 4,   // pcq_init takes it from the environment variable PCQ_<NAME IN CAPITALS>; a value outside the range is ignored
};
struct Option {
    const char *name;
    int pcq_ctx::*i32 = nullptr;  // where it lives in pcq_ctx: one of the three
    int64_t pcq_ctx::*i64 = nullptr;
    uint64_t pcq_ctx::*u64 = nullptr;
    int64_t min = 0, max = 0;
    unsigned flags = 0;
    constexpr Option(const char *n, int pcq_ctx::*p, int64_t lo, int64_t hi, unsigned f) : name(n), i32(p), min(lo), max(hi), flags(f) {}
    constexpr Option(const char *n, int64_t pcq_ctx::*p, int64_t lo, int64_t hi, unsigned f) : name(n), i64(p), min(lo), max(hi), flags(f) {}
    constexpr Option(const char *n, uint64_t pcq_ctx::*p, int64_t lo, int64_t hi, unsigned f) : name(n), u64(p), min(lo), max(hi), flags(f) {}
    int64_t get(const pcq_ctx *c) const { return i32 ? c->*i32 : i64 ? c->*i64 : (int64_t)(c->*u64); }
    void set(pcq_ctx *c, int64_t v) const {
        if (flags & OPT_BOOL) v = v != 0;
        if (i32) c->*i32 = (int)v;
        else if (i64) c->*i64 = v;
        else c->*u64 = (uint64_t)v;
    }
    bool accepts(int64_t v) const { return (flags & OPT_BOOL) || (v >= min && v <= max); }
};
#define DIAG(field) Option(#field, &pcq_ctx::field, 0, 0, 0)
static const Option k_options[] = {
    {"blocks_per_cu", &pcq_ctx::grid_blocks_per_cu, 1, 32, OPT_SET},  // (the lab build: batch_blocks_per_cu with it, below)
    {"chunk_points", &pcq_ctx::chunk_points, 4, INT64_MAX, OPT_SET | OPT_ENV},
    {"copy_threads", &pcq_ctx::copy_threads, 1, 64, OPT_SET | OPT_ENV},
    {"numa_local", &pcq_ctx::numa_local, 0, 1, OPT_SET | OPT_BOOL | OPT_ENV},  // (drops the staging ring, below)
    {"host_in_place", &pcq_ctx::host_in_place, 0, 2, OPT_SET | OPT_ENV},  // 0 never, 1 always, 2 until the copy path is set up
    {"allreduce_single_rank", &pcq_ctx::allreduce_single_rank, 0, 1, OPT_SET | OPT_BOOL},
    {"allreduce_fail", &pcq_ctx::allreduce_fail, 0, 3, OPT_SET},
    // (points scanned into a grid collector before it folds; a fold's tuple counts and offsets are 32-bit, grid_host.hip clamps to that)
    {"grid_pending_budget", &pcq_ctx::grid_pending_budget, 0, (int64_t)1 << 40, OPT_SET},
    {"grid_agg", &pcq_ctx::grid_agg, 0, 2, OPT_SET},  // 0 adaptive, 1 always, 2 never
    {"grid_f2", &pcq_ctx::grid_f2, 0, 4096, OPT_SET},
    {"grid_stream", &pcq_ctx::grid_stream, 0, 1, OPT_SET},
    {"grid_tuple16", &pcq_ctx::grid_tuple16, 0, 2, OPT_SET},
    {"grid_block_pad", &pcq_ctx::grid_block_pad, 0, 65536, OPT_SET},
    {"grid_p0_blocks", &pcq_ctx::grid_p0_blocks, 0, 65536, OPT_SET},  // (lowers pass 0's workgroup count only: grid_host.hip)
    {"emit_park_max", &pcq_ctx::emit_park_max, 0, 256, OPT_SET},
    {"emit_sparse_max", &pcq_ctx::emit_sparse_max, 0, 2048, OPT_SET},
    {"scratch_cap_words", &pcq_ctx::scratch_cap_words, 0, INT64_MAX, OPT_SET},
    DIAG(numa_node), DIAG(grid_folds), DIAG(grid_level2), DIAG(grid_refolds), DIAG(grid_level2_exact), DIAG(grid_last_f2),
    DIAG(grid_compactions), DIAG(grid_deferred), DIAG(grid_dense_deferred), DIAG(grid_last_tuples), DIAG(grid_last_tuple_bytes), DIAG(emit_park_fallbacks),
#ifdef PCQ_LAB
    {"k1_variant", &pcq_ctx::k1_variant, 0, 14, OPT_SET | OPT_ENV},
    {"k1_waves_per_cu", &pcq_ctx::k1_waves_per_cu, 1, 32, OPT_SET | OPT_ENV},
    {"k1_grid", &pcq_ctx::k1_grid, 0, 1 << 20, OPT_SET},
    {"batch_variant", &pcq_ctx::batch_variant, 0, 3, OPT_SET | OPT_ENV},
    {"batch_waves_per_cu", &pcq_ctx::batch_waves_per_cu, 1, 32, OPT_SET | OPT_ENV},
    {"class_batch_loads", &pcq_ctx::class_batch_loads, 0, 12, OPT_SET},  // (only 0, 4, 6, 8 and 12, below)
    {"class_batch_pipe", &pcq_ctx::class_batch_pipe, 0, 1, OPT_SET | OPT_BOOL},
    {"class_batch_waves_per_cu", &pcq_ctx::class_batch_waves_per_cu, 1, 32, OPT_SET},
    {"multi_waves_per_cu", &pcq_ctx::multi_waves_per_cu, 0, 32, OPT_SET},
    {"class_hist_waves_per_cu", &pcq_ctx::class_hist_waves_per_cu, 0, 32, OPT_SET},
    {"time_hist_waves_per_cu", &pcq_ctx::time_hist_waves_per_cu, 0, 32, OPT_SET},
    {"raster_waves_per_cu", &pcq_ctx::raster_waves_per_cu, 0, 32, OPT_SET},
    {"zrange_waves_per_cu", &pcq_ctx::zrange_waves_per_cu, 0, 32, OPT_SET},
    {"zsum_waves_per_cu", &pcq_ctx::zsum_waves_per_cu, 0, 32, OPT_SET},
    {"zsum_classes_waves_per_cu", &pcq_ctx::zsum_classes_waves_per_cu, 0, 32, OPT_SET},
    {"zmoments_waves_per_cu", &pcq_ctx::zmoments_waves_per_cu, 0, 32, OPT_SET},
    {"zrange_classes_waves_per_cu", &pcq_ctx::zrange_classes_waves_per_cu, 0, 32, OPT_SET},
    {"polygon_waves_per_cu", &pcq_ctx::polygon_waves_per_cu, 0, 32, OPT_SET},
    {"raster_add", &pcq_ctx::raster_add, 0, 2, OPT_SET},  // 0 the product's, 1 per lane, 2 wave-level (scan_raster.hip)
    {"class_hist_copies", &pcq_ctx::class_hist_copies, 0, 16, OPT_SET},  // (only 0, 1, 2, 4, 8 and 16: scan_class_hist.hip)
#endif
};
#undef DIAG

static const Option *find_option(const char *key) {
    for (const Option &o : k_options)
        if (!strcmp(key, o.name)) return &o;
    return nullptr;
}

static void options_from_env(pcq_ctx *ctx) {
    for (const Option &o : k_options) {
        if (!(o.flags & OPT_ENV)) continue;
        char var[64] = "PCQ_";
        for (size_t i = 0; o.name[i] && i + 5 < sizeof var; i++) var[4 + i] = (char)toupper((unsigned char)o.name[i]);
        const char *e = getenv(var);
        if (!e) continue;
        const long long v = atoll(e);
        if (o.accepts(v)) o.set(ctx, v);
    }
}

extern "C" int pcq_set_option(pcq_ctx *ctx, const char *key, int64_t value) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !key) return pcq_fail(PCQ_ERR_ARG, "pcq_set_option: null argument");
    const Option *o = find_option(key);
    if (!o) return pcq_fail(PCQ_ERR_ARG, "unknown option '%s'", key);
    if (!(o->flags & OPT_SET)) return pcq_fail(PCQ_ERR_ARG, "option '%s' is read-only", key);
    if (!o->accepts(value)) return pcq_fail(PCQ_ERR_ARG, "%s must be %lld..%lld", key, (long long)o->min, (long long)o->max);
#ifdef PCQ_LAB
    if (o->i32 == &pcq_ctx::class_batch_loads && value != 0 && value != 4 && value != 6 && value != 8 && value != 12)
        return pcq_fail(PCQ_ERR_ARG, "class_batch_loads must be 0, 4, 6, 8 or 12");
    if (o->i32 == &pcq_ctx::grid_blocks_per_cu) ctx->batch_blocks_per_cu = (int)value;
#endif
    // the thread of pcq_prepare_host_scans reads these three: it is joined before they change
    const bool numa = o->i32 == &pcq_ctx::numa_local;
    if (numa || o->i32 == &pcq_ctx::copy_threads || o->u64 == &pcq_ctx::chunk_points) ctx->ring.join_prepare();
    o->set(ctx, value);
    if (numa) ctx->ring.drop();  // the copy helpers and the pinned buffers are re-created with or without the affinity by the next scan
    return PCQ_OK;
}

extern "C" int pcq_get_option(pcq_ctx *ctx, const char *key, int64_t *value) {
    if (!ctx || !key || !value) return pcq_fail(PCQ_ERR_ARG, "pcq_get_option: null argument");
    const Option *o = find_option(key);
    if (!o) return pcq_fail(PCQ_ERR_ARG, "unknown option '%s'", key);
    *value = o->get(ctx);
    return PCQ_OK;
}

// ---------------------------------------------------------------------------------------------
// device memory helpers
// ---------------------------------------------------------------------------------------------
extern "C" int pcq_device_alloc(pcq_ctx *ctx, uint64_t bytes, void **out) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || !out) return pcq_fail(PCQ_ERR_ARG, "pcq_device_alloc: null argument");
    *out = nullptr;
    PCQ_HIP(hipSetDevice(ctx->device));
    PCQ_HIP(hipMalloc(out, bytes ? bytes : 16));
    return PCQ_OK;
}
extern "C" int pcq_device_free(pcq_ctx *ctx, void *p) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx) return pcq_fail(PCQ_ERR_ARG, "pcq_device_free: null context");
    if (p) PCQ_HIP(hipFree(p));
    return PCQ_OK;
}
extern "C" int pcq_copy_to_device(pcq_ctx *ctx, void *dst, const void *src, uint64_t bytes) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!dst && bytes) || (!src && bytes)) return pcq_fail(PCQ_ERR_ARG, "pcq_copy_to_device: null argument");
    if (bytes) PCQ_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return PCQ_OK;
}
extern "C" int pcq_copy_to_host(pcq_ctx *ctx, void *dst, const void *src, uint64_t bytes) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!dst && bytes) || (!src && bytes)) return pcq_fail(PCQ_ERR_ARG, "pcq_copy_to_host: null argument");
    if (bytes) {
        if (bytes <= 64 * sizeof(uint64_t) && bytes % 8 == 0 && ((uintptr_t)src & 7) == 0) {
            // A few words (a count): a kernel stores them into the context's pinned, device-visible scratch.  The first
            // device-to-host hipMemcpy of a process sets up the runtime's copy-engine path — 8 ms in the CLI, where this
            // read is the only one (profiles/r03_cli_e2e.log).
            hipLaunchKernelGGL(k_words_to_host, dim3(1), dim3(64), 0, ctx->stream, (const uint64_t *)src, ctx->h_scalars, (uint32_t)(bytes / 8));
            PCQ_HIP(hipGetLastError());
            PCQ_HIP(hipStreamSynchronize(ctx->stream));
            memcpy(dst, ctx->h_scalars, bytes);
            return PCQ_OK;
        }
        PCQ_HIP(hipStreamSynchronize(ctx->stream));
        PCQ_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    }
    return PCQ_OK;
}
extern "C" int pcq_device_memset(pcq_ctx *ctx, void *dst, int value, uint64_t bytes, void *stream) {
    PCQ_ON_DEVICE_OF_CTX(ctx);
    if (!ctx || (!dst && bytes)) return pcq_fail(PCQ_ERR_ARG, "pcq_device_memset: null argument");
    if (bytes) PCQ_HIP(hipMemsetAsync(dst, value, bytes, stream ? (hipStream_t)stream : ctx->stream));
    return PCQ_OK;
}

// ---------------------------------------------------------------------------------------------
// host-side math of the boundary
// ---------------------------------------------------------------------------------------------

// Rust `f64 as i64`: truncate toward zero, saturate, NaN -> 0.
static int64_t rust_f64_as_i64(double v) {
    if (std::isnan(v)) return 0;
    if (v >= 9223372036854775808.0) return INT64_MAX;
    if (v <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)v;
}

// last.rs:98-109 / las.rs:88-99
extern "C" int pcq_box_to_local(const double bmin[3], const double bmax[3], const double scale[3],
                                const double offset[3], int64_t lmin[3], int64_t lmax[3]) {
    if (!bmin || !bmax || !scale || !offset || !lmin || !lmax) return pcq_fail(PCQ_ERR_ARG, "pcq_box_to_local: null argument");
    for (int a = 0; a < 3; a++) {
        lmin[a] = rust_f64_as_i64((bmin[a] - offset[a]) / scale[0]);  // sic: x scale on every axis (last.rs:100-102)
        lmax[a] = rust_f64_as_i64((bmax[a] - offset[a]) / scale[a]);
    }
    for (int a = 0; a < 3; a++)
        if (lmin[a] > lmax[a])
            return pcq_fail(PCQ_ERR_PANIC, "AABB::from_min_max: Minimum position must be <= maximum position!");
    return PCQ_OK;
}

int pcq_make_dev_pred(const pcq_predicate *p, DevPred *out) {
    memset(out, 0, sizeof *out);
    out->kind = p->kind;
    if (p->kind == PCQ_PRED_CLASS) {
        out->cls = p->cls;
        return PCQ_OK;
    }
    if (p->kind == PCQ_PRED_BOUNDS_F64) {
        for (int a = 0; a < 3; a++) out->wmin[a] = p->wmin[a], out->wmax[a] = p->wmax[a];
        return PCQ_OK;
    }
    if (pred_tests_time(p->kind)) {  // [start, end): an empty or NaN range is legal and matches nothing
        out->wmin[0] = p->wmin[0];
        out->wmax[0] = p->wmax[0];
        if (p->kind == PCQ_PRED_TIME) return PCQ_OK;
    }
    if (p->kind == PCQ_PRED_BOUNDS_CLASS) out->cls = p->cls;  // (and the box below)
    if (!pred_has_box(p->kind)) return pcq_fail(PCQ_ERR_ARG, "unknown predicate kind %d", p->kind);
    for (int a = 0; a < 3; a++) {
        const int64_t lo = p->lmin[a] < INT32_MIN ? (int64_t)INT32_MIN : p->lmin[a];
        const int64_t hi = p->lmax[a] > INT32_MAX ? (int64_t)INT32_MAX : p->lmax[a];
        if (lo > hi) {  // covers lmin > lmax as well as boxes outside the i32 value range
            out->empty = 1;
            out->lo[a] = 0;
            out->width[a] = 0;
        } else {
            out->lo[a] = (int32_t)lo;
            out->width[a] = (uint32_t)(hi - lo);
        }
    }
    return PCQ_OK;
}
