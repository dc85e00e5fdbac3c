// search.cpp — collectors, the plan of the optimized per-file searches and the Searcher dispatch.
//
// plan_file does on the host exactly what the reference does before its per-point loop
// (open + mmap, header parse, block offsets, file-level early-out, query box -> local integer box)
// and then hands the column blocks to libpcq.so, which replaces the loop and the collector pushes.
#include "pcq_host.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <initializer_list>

namespace pcq {

// ---- collectors (collect_points.rs) ---------------------------------------------------------------
ResultCollector::~ResultCollector() {
    if (handle_) pcq_collector_free(handle_);
}
std::optional<std::vector<Point>> ResultCollector::points() { return std::nullopt; }  // collect_points.rs:87-89
const std::vector<Point> *ResultCollector::points_ref() { return nullptr; }           // :91-93
Status ResultCollector::point_count(size_t *out) {
    uint64_t n = 0;
    const int rc = pcq_collector_point_count(handle_, &n);
    if (rc) return Status::FromLib(rc);
    *out = (size_t)n;
    return Status::Ok();
}
Status ResultCollector::fetch() {
    if (cached_) return Status::Ok();
    uint64_t n = 0;
    int rc = pcq_collector_points(handle_, nullptr, 0, &n);
    if (rc) return Status::FromLib(rc);
    cache_.resize((size_t)n);
    if (n) {
        rc = pcq_collector_points(handle_, cache_.data(), n, &n);
        if (rc) return Status::FromLib(rc);
    }
    cached_ = true;
    return Status::Ok();
}

Status CountCollector::create(pcq_ctx *ctx, std::unique_ptr<ResultCollector> *out, uint64_t *device_counter) {
    auto c = std::make_unique<CountCollector>();
    c->ctx_ = ctx;
    const int rc = device_counter ? pcq_collector_new_count_at(ctx, device_counter, &c->handle_) : pcq_collector_new_count(ctx, &c->handle_);
    if (rc) return Status::FromLib(rc);
    *out = std::move(c);
    return Status::Ok();
}
Status BufferCollector::create(pcq_ctx *ctx, std::unique_ptr<ResultCollector> *out) {
    auto c = std::make_unique<BufferCollector>();
    c->ctx_ = ctx;
    const int rc = pcq_collector_new_buffer(ctx, &c->handle_);
    if (rc) return Status::FromLib(rc);
    *out = std::move(c);
    return Status::Ok();
}
std::optional<std::vector<Point>> BufferCollector::points() {  // :33-35
    if (!fetch().ok()) return std::vector<Point>{};
    return cache_;
}
const std::vector<Point> *BufferCollector::points_ref() {  // :37-39
    if (!fetch().ok()) return nullptr;
    return &cache_;
}
Status GridSampledCollector::create(pcq_ctx *ctx, const AABB &bounds, double cell_size, std::unique_ptr<ResultCollector> *out) {
    auto c = std::make_unique<GridSampledCollector>();
    c->ctx_ = ctx;
    const int rc = pcq_collector_new_grid(ctx, bounds.min, bounds.max, cell_size, &c->handle_);
    if (rc) return Status::FromLib(rc);
    *out = std::move(c);
    return Status::Ok();
}
std::optional<std::vector<Point>> GridSampledCollector::points() {  // :116-118
    if (!fetch().ok()) return std::vector<Point>{};
    return cache_;
}

// The column blocks were located in the mapped file (header parse, offsets: exactly as the reference does); the
// bytes themselves are streamed by the library with pread, so a plan carries FILE OFFSETS instead of addresses inside a
// mapping — and nothing else of the file: the mapping and the descriptor of the prologue are gone when the plan is
// returned, and the file is opened again here, for the duration of its scan.  (run_search_parallel plans every file before
// the first worker starts; a plan that kept its file open put a query over a thousand files past RLIMIT_NOFILE, where the
// reference — which opens inside the rayon task — has at most one file per thread open.)
Status execute_plan(FilePlan &plan, ResultCollector &rc) {
    if (!plan.status.ok() || !plan.needs_gpu) return plan.status;
    pcq_columns cols = plan.cols;
    cols.first_index = rc.next_index;
    const int fd = ::open(plan.path.c_str(), O_RDONLY);
    if (fd < 0) return Status::Err(PCQ_ERR_IO, plan.path + ": " + strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || (uint64_t)st.st_size < plan.file_size) {  // (truncated between the prologue and the scan)
        ::close(fd);
        return Status::Err(PCQ_ERR_EOF, "failed to fill whole buffer");
    }
    // The reference opens a file once, inside its task (last.rs:51); here the header was read by the prologue and the path
    // is opened again.  Another file under the same name — replaced, or rewritten in place — must not be scanned with the
    // first one's offsets, scale and point count.
    if ((uint64_t)st.st_dev != plan.file_dev || (uint64_t)st.st_ino != plan.file_ino || (uint64_t)st.st_size != plan.file_size ||
        (int64_t)st.st_mtim.tv_sec * 1000000000ll + st.st_mtim.tv_nsec != plan.file_mtime_ns) {
        ::close(fd);
        return Status::Err(PCQ_ERR_IO, plan.path + ": the file changed while the query was running");
    }
    // (not waited for: the bytes have been read when this returns, the collector's accessors — or the driver's
    // synchronisation of the context before it merges — wait for the kernels; the next file's first read overlaps them)
    const int r = pcq_scan_fd_nowait(rc.context(), fd, &cols, &plan.pred, rc.handle());
    ::close(fd);
    rc.next_index += cols.n;
    return Status::FromLib(r);
}

// ---- where a file's columns lie: the one place that knows these numbers -----------------------------------------------
ColumnLayout column_layout(const LasHeader &h, FileLayout layout) {
    const uint8_t fmt = h.point_data_record_format;
    const uint64_t otp = h.offset_to_point_data, n = h.number_of_points;
    ColumnLayout l;
    l.record_length = layout == FileLayout::LAS ? h.point_data_record_length : 0;
    auto at = [&](uint64_t in_point, uint64_t size) {
        return layout == FileLayout::LAS ? FileColumn{true, otp + in_point, l.record_length, size} : FileColumn{true, otp + n * in_point, size, size};
    };
    l.xyz = at(0, 12);                                      // last.rs:114-121, las.rs:102-104
    l.cls = at(fmt <= 5 ? 15 : 16, 1);                      // last.rs:69-81
    l.rgb.stride = at(0, 6).stride;                         // (a plan names the colours' stride even where the format has none)
    if (fmt == 2) l.rgb = at(20, 6);                        // las.rs:38-45, last.rs:83-88: the reference knows the colours of
    if (fmt == 3 || fmt == 5) l.rgb = at(28, 6);            // formats 2, 3 and 5 only
    if (fmt != 0 && fmt != 2) l.time = at(fmt <= 5 ? 20 : 22, 8);  // las.rs:305-330
    return l;
}

namespace {
Status invalid_format(uint8_t fmt, const std::string &path) {
    return Status::Err(PCQ_ERR_FORMAT, "Invalid LAS format " + std::to_string(fmt) + " in file " + path);
}
Status eof() { return Status::Err(PCQ_ERR_EOF, "failed to fill whole buffer"); }

// A block [off, off + bytes) must lie inside the mapped file.  The reference's Cursor reads fail
// lazily with UnexpectedEof when a truncated byte is touched; here the blocks a scan may touch are
// validated up front ("deviations").
bool block_ok(const MappedFile &f, uint64_t off, uint64_t bytes) { return off <= f.size() && bytes <= f.size() - off; }

// Every column of `read` lies inside the file.  LAST: each block, n elements.  LAS: every record up to the last byte any of the
// columns needs, as one block from the first record.
bool columns_ok(const MappedFile &f, const LasHeader &h, FileLayout layout, std::initializer_list<FileColumn> read) {
    const uint64_t n = h.number_of_points, otp = h.offset_to_point_data;
    uint64_t last_needed = 0;
    for (const FileColumn &c : read) {
        if (!c.present) continue;
        if (layout == FileLayout::LAST && !block_ok(f, c.offset, n * c.size)) return false;
        last_needed = std::max(last_needed, c.offset - otp + c.size);
    }
    return layout == FileLayout::LAST || block_ok(f, otp, (n - 1) * h.point_data_record_length + last_needed);
}
}  // namespace

// What the host does for one file before the per-point loop: open + mmap, header, where the columns lie, the file-level early-out,
// the query box -> local integer box.  One body for the five kinds and both layouts; what differs between them is named first.
FilePlan plan_file(const std::string &path, FileLayout layout, const Query &q) {
    const bool las = layout == FileLayout::LAS;
    const bool plain_box = q.kind == PCQ_PRED_BOUNDS;
    const bool by_class = q.kind == PCQ_PRED_CLASS || q.kind == PCQ_PRED_BOUNDS_CLASS;
    const bool by_time = q.kind == PCQ_PRED_TIME || q.kind == PCQ_PRED_BOUNDS_TIME;
    const bool boxed = !(q.kind == PCQ_PRED_CLASS || q.kind == PCQ_PRED_TIME);
    const bool mask_format = !las && by_class;     // last.rs:220-223 `&= 0b1111`; no other search masks (last.rs:53-54, las.rs:59-60, :199-200, :302-303)
    const bool format_rereported = by_time;        // las.rs:324-329: the time search's own match arm names a format above 10
    const bool class_at_15 = las && plain_box;     // las.rs:121-124 seek(Current(3)): +15 whatever the format; las.rs:224-228 goes by format
    const bool prints_record_size = las && plain_box;  // las.rs:73, before the early-out; the combined kinds print none
    const bool box_first = plain_box;              // last.rs:92-109: early-out and box before a byte of a point is touched; the combined
                                                   // kinds run the attribute search's prologue, then these two
    const bool colours = !by_time;                 // las.rs:345-355 `..Default::default()`: a time record has no colour

    FilePlan plan;  // resolved on the host (no GPU work) until the last lines
    auto resolved = [&](Status st = Status::Ok()) {
        FilePlan p;
        p.status = std::move(st), p.las_record_size = plan.las_record_size;
        return p;
    };
    MappedFile file;
    Status st = file.open(path);  // last.rs:51
    if (!st.ok()) return resolved(st);
    LasHeader h;
    st = parse_las_header(file.data(), file.size(), mask_format, &h);
    if (!st.ok() && format_rereported && st.message.rfind("invalid point format number: ", 0) == 0) st = invalid_format(file.data()[104], path);  // (the format byte)
    if (!st.ok()) return resolved(st);
    if (prints_record_size) plan.las_record_size = h.point_data_record_length;
    ColumnLayout l = column_layout(h, layout);
    if (class_at_15) l.cls.offset = h.offset_to_point_data + 15;
    if (by_time && !l.time.present) return resolved(Status::Err(PCQ_ERR_FORMAT, "File " + path + " does not contain GPS times!"));  // las.rs:306-318
    const FileColumn attribute = by_time ? l.time : l.cls, rgb = colours ? l.rgb : FileColumn{};
    const uint64_t n = h.number_of_points;

    // the header-AABB early-out (last.rs:92-94: resolved from the header alone), then the box (:98-109) and its error
    pcq_predicate pred{};
    auto box = [&]() -> std::optional<FilePlan> {
        if (!h.bounds.intersects(q.box)) return resolved();
        const int rc = pcq_box_to_local(q.box.min, q.box.max, h.scale, h.offset, pred.lmin, pred.lmax);
        if (rc) return resolved(Status::FromLib(rc));
        return std::nullopt;
    };
    if (box_first)
        if (auto out = box()) return *out;
    if (n != 0 && !columns_ok(file, h, layout, {l.xyz, attribute, rgb})) return resolved(eof());
    if (boxed && !box_first)
        if (auto out = box()) return *out;
    if (n == 0) {  // (no points; no file-level early-out for the attributes: the header has no class or time bounds, las.rs:332)
        FilePlan p = resolved();
        if (!box_first) p.pred = pred;  // (a combined plan keeps the box it converted; nothing reads the predicate of a resolved plan)
        return p;
    }

    pred.kind = q.kind;
    if (by_class) pred.cls = q.cls;                               // last.rs:259-262 whole byte
    if (by_time) pred.wmin[0] = q.start, pred.wmax[0] = q.end;    // Range { start, end }: start <= t && t < end (las.rs:336)
    // The bytes are streamed by the library with pread, so the plan carries FILE OFFSETS as column "pointers" (a NULL column stays
    // NULL; offset 0 never is a column, the header lives there) and which file they hold for: execute_plan opens the path again.
    auto pointer = [](const FileColumn &c) { return c.present ? (const void *)(uintptr_t)c.offset : nullptr; };
    plan.needs_gpu = true;
    plan.path = path;
    plan.file_size = file.size();
    plan.file_dev = file.dev(), plan.file_ino = file.ino(), plan.file_mtime_ns = file.mtime_ns();
    plan.cols.xyz = pointer(l.xyz), plan.cols.xyz_stride = l.xyz.stride;
    plan.cols.cls = pointer(attribute), plan.cols.cls_stride = attribute.stride;  // (the predicate's column: class bytes or GPS times)
    plan.cols.rgb = pointer(rgb), plan.cols.rgb_stride = rgb.stride;
    plan.cols.n = n;
    for (int a = 0; a < 3; a++) plan.cols.scale[a] = h.scale[a], plan.cols.offset[a] = h.offset[a];  // last.rs:156-160
    plan.pred = pred;
    return plan;
}

// The host-only part of ResidentDataset::load for one LAST file.  with_times: first everything the LAST time search's prologue
// raises for this file, so a file fails here as it fails there (no GPS times, a format above 10, a block past the file's end).
Status resident_file_blocks(const std::string &path, bool with_points, bool with_times, MappedFile *file, ResidentBlocks *out) {
    *out = ResidentBlocks{};
    if (path.size() < 5 || path.compare(path.size() - 5, 5, ".last") != 0)
        return Status::Err(PCQ_ERR_EXTENSION, "resident datasets hold LAST files: " + path);
    if (with_times) {
        const FilePlan plan = plan_file(path, FileLayout::LAST, Query{PCQ_PRED_TIME, {}, 0, 0.0, 0.0});
        if (!plan.status.ok()) return plan.status;
    }
    Status st = file->open(path);
    if (!st.ok()) return st;
    st = parse_las_header(file->data(), file->size(), /*mask_format=*/false, &out->header);  // last.rs:53-54
    if (!st.ok()) return st;
    const ColumnLayout l = column_layout(out->header, FileLayout::LAST);
    if (!columns_ok(*file, out->header, FileLayout::LAST, {l.xyz, l.cls})) return eof();
    const bool colours = with_points && l.rgb.present;
    if (colours && !columns_ok(*file, out->header, FileLayout::LAST, {l.rgb})) return eof();
    out->xyz = l.xyz.offset, out->cls = l.cls.offset;
    out->rgb = colours ? l.rgb.offset : 0, out->time = with_times ? l.time.offset : 0;
    return Status::Ok();
}

// ---- searcher.rs ---------------------------------------------------------------------------------------------
namespace {
std::optional<std::string> extension_of(const std::string &path) {  // Path::extension().and_then(OsStr::to_str)
    const size_t slash = path.find_last_of('/');
    const std::string base = slash == std::string::npos ? path : path.substr(slash + 1);
    const size_t dot = base.find_last_of('.');
    if (dot == std::string::npos || dot == 0) return std::nullopt;
    return base.substr(dot + 1);
}
Status out_of_scope(const std::string &what, const std::string &path) {
    return Status::Err(PCQ_ERR_UNSUPPORTED, what + " is outside the MI355X hot path (SURVEY.md §2): " + path);
}
}  // namespace

// The host-only prologue of search_file for the formats whose prologue needs no GPU (LAS / LAST --optimized): everything
// the reference does before its per-point loop.  Other formats (and errors of the dispatch itself) are left to search_file.
std::optional<FilePlan> Searcher::plan_file(const std::string &path, SearchImplementation impl) const {
    const auto ext = extension_of(path);
    if (!ext || impl != SearchImplementation::Optimized) return std::nullopt;
    if (*ext == "las") return pcq::plan_file(path, FileLayout::LAS, query_);
    if (*ext == "last") return pcq::plan_file(path, FileLayout::LAST, query_);
    return std::nullopt;
}

Status Searcher::search_file(const std::string &path, SearchImplementation impl, ResultCollector &collector, SearchLog *log) const {  // searcher.rs:43-90, :104-151
    const auto ext = extension_of(path);
    if (!ext) return Status::Err(PCQ_ERR_EXTENSION, "Invalid extension on file " + path);
    if (*ext == "las" || *ext == "last") {
        if (impl == SearchImplementation::Regular) return out_of_scope("the Regular (non --optimized) search implementation", path);
        FilePlan plan = *plan_file(path, impl);
        if (log) log->las_record_size = plan.las_record_size;
        return execute_plan(plan, collector);
    }
    if (*ext == "lazer") {  // searcher.rs:83, :144, either implementation
        if (query_.kind == PCQ_PRED_BOUNDS) return search_lazer_file_by_bounds(path, query_.box, collector);
        if (query_.kind == PCQ_PRED_CLASS) return search_lazer_file_by_classification(path, query_.cls, collector);
        // the reference's LAZ / LAZER time searches are todo!() stubs (laz.rs:131-146, lazer.rs:115-122)
        return out_of_scope(query_.kind == PCQ_PRED_TIME ? "time search in .lazer files" : "combined search in .lazer files", path);
    }
    if (*ext == "laz") return out_of_scope("compressed format .laz", path);
    return Status::Err(PCQ_ERR_EXTENSION, "Unsupported file extension in file " + path);
}

}  // namespace pcq
