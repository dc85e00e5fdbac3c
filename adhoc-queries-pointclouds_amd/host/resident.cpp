// resident.cpp — a dataset kept in HBM and queried repeatedly: count queries as ONE batched launch per GPU.
//
// The reference answers every query by walking the files again (main.rs:146-183); with the blocks already resident in
// HBM the same answer is a single launch over all files of the GPU — per file the host prologue the reference runs
// before its loop (the header-AABB early-out last.rs:92-94, the f64 -> local integer box :98-109), then
// pcq_scan_dev_count_batch: one segment per surviving file, the total added into one device counter.  A per-file launch
// of the class kernel over one 163 MB block is launch-bound (5.0-5.7 TB/s, profiles/r01_k2_file_rate.log); the batched
// launch reaches the streaming rate (7.1 TB/s) because 15 of 16 launch tails disappear.
//
// Point and density queries (search_bounds / search_class) are the per-file searches of search.cpp over the resident blocks,
// file by file into one collector.  A count or buffer collector goes through each file's chunk index (pcq_scan_dev_indexed):
// its first query of a kind builds the index, later ones read only the chunks that straddle the box.  A grid collector goes
// through pcq_scan_dev; its pass 0 does not consult the index.
//
// Box AND class (count_bounds_class / search_bounds_class): both blocks of a file lie in HBM side by side, so the count is one
// pcq_scan_dev_count_batch_combined and the search goes through both parts of the file's index (pcq_scan_dev_indexed_combined).
//
// GPS time (search_time): a dataset loaded with its time blocks answers the LAST time search over them, count and buffer
// collectors through the time part of the file's index (pcq_scan_dev_indexed_time).
//
// Box AND time (count_bounds_time / search_bounds_time): the positions and time blocks of such a dataset side by side — the count is
// one pcq_scan_dev_count_batch_bounds_time, the search goes through the bounds and time parts of the file's index
// (pcq_scan_dev_indexed_bounds_time).
//
// The class histogram of a box (count_bounds_by_class): the per-class breakdown of count_bounds_class for all 256 classes from
// one pcq_scan_dev_class_hist_batch, instead of one combined count per class.
//
// The time histogram of a box (count_bounds_by_time): the per-slice breakdown of count_bounds_time for the bins between the
// caller's edges, one pcq_scan_dev_time_hist_batch per group of PCQ_TIME_BINS_MAX bins, instead of one box AND time count per bin.
//
// The density raster of a box (count_bounds_raster): the per-cell breakdown of count_bounds over a 2-D lattice of cells, one
// pcq_scan_dev_raster_batch per block of PCQ_RASTER_CELLS_MAX cells, instead of one box count per cell.
//
// The height raster of a box (bounds_zrange_raster): the lowest and the highest world z of the points of every cell of the same
// lattice, one pcq_scan_dev_zrange_raster_batch per group of files of one z lattice and block of PCQ_ZRANGE_CELLS_MAX cells, instead of
// a search into a buffer collector whose records the host would have to reduce.
//
// The mean-height raster of a box (bounds_zmean_raster): the count and the mean world z of the points of every cell of the same
// lattice, one pcq_scan_dev_zsum_raster_batch per batch of files of one z lattice (zsum_plan.h) and block of PCQ_ZSUM_CELLS_MAX
// cells, the batches' counts and sums merged on the host in world space.  Of the points of a set of classes
// (bounds_zmean_raster_classes): the same body with pcq_scan_dev_zsum_raster_batch_classes and the class blocks in the columns.
//
// The height-spread raster of a box (bounds_zstd_raster): count, mean and population standard deviation of the world z of the points
// of every cell, one pcq_scan_dev_zmoments_raster_batch per batch of the mean-height raster and block of PCQ_ZMOMENTS_CELLS_MAX
// cells, the batches' exact integer words merged on the host (zmoments_merge.h).
//
// Box AND polygon (count_polygon): the points inside a world outline, one pcq_scan_dev_count_batch_polygon over the surviving files
// with the outline rounded into each file's lattice (polygon_plan.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pcq_host.hpp"
#include "polygon_plan.h"
#include "zmoments_merge.h"
#include "zsum_plan.h"

namespace pcq {

ResidentDataset::~ResidentDataset() {
    for (auto &f : files_) {
        if (f.xyz) pcq_device_free(ctx_, f.xyz);
        if (f.cls) pcq_device_free(ctx_, f.cls);
        if (f.rgb) pcq_device_free(ctx_, f.rgb);
        if (f.time) pcq_device_free(ctx_, f.time);
        if (f.index) pcq_index_free(f.index);
    }
    if (counter_) pcq_device_free(ctx_, counter_);
}

// Loads the positions and classification blocks of every .last file into HBM; where they lie, and what fails before a byte is
// loaded, is resident_file_blocks (search.cpp).
// with_points: the colour block as well (last.rs:83-90), for the records of buffer and grid collectors.
// with_times: the GPS time block as well, where the LAST time search finds it.
Status ResidentDataset::load(pcq_ctx *ctx, const std::vector<std::string> &paths, std::unique_ptr<ResidentDataset> *out, bool with_points,
                             bool with_times) {
    auto ds = std::unique_ptr<ResidentDataset>(new ResidentDataset());
    ds->ctx_ = ctx;
    ds->with_points_ = with_points;
    ds->with_times_ = with_times;
    void *p = nullptr;
    Status st = Status::FromLib(pcq_device_alloc(ctx, 16, &p));
    if (!st.ok()) return st;
    ds->counter_ = (uint64_t *)p;
    for (const auto &path : paths) {
        MappedFile file;
        ResidentBlocks b;
        st = resident_file_blocks(path, with_points, with_times, &file, &b);
        if (!st.ok()) return st;
        ResidentFile rf;
        rf.header = b.header;
        const uint64_t n = rf.header.number_of_points, otp = b.xyz, cls_block = b.cls, col_block = b.rgb, time_block = b.time;
        const bool colours = b.rgb != 0;
        rf.path = path;
        if (n) {
            st = Status::FromLib(pcq_device_alloc(ctx, n * 12, &rf.xyz));
            if (st.ok()) st = Status::FromLib(pcq_device_alloc(ctx, n, &rf.cls));
            if (st.ok() && colours) st = Status::FromLib(pcq_device_alloc(ctx, n * 6, &rf.rgb));
            if (st.ok() && with_times) st = Status::FromLib(pcq_device_alloc(ctx, n * 8, &rf.time));
            if (st.ok() && with_times) st = Status::FromLib(pcq_read_fd_to_device(ctx, file.fd(), time_block, n * 8, rf.time));
            if (st.ok()) st = Status::FromLib(pcq_read_fd_to_device(ctx, file.fd(), otp, n * 12, rf.xyz));
            if (st.ok()) st = Status::FromLib(pcq_read_fd_to_device(ctx, file.fd(), cls_block, n, rf.cls));
            if (st.ok() && colours) st = Status::FromLib(pcq_read_fd_to_device(ctx, file.fd(), col_block, n * 6, rf.rgb));
        }
        ds->files_.push_back(rf);
        if (!st.ok()) return st;
        ds->points_ += n;
    }
    *out = std::move(ds);
    return Status::Ok();
}

static const char *const NO_COLOURS = "resident dataset loaded without its colour blocks: count collectors only (pcq_query_resident_load_points)";
static const char *const NO_TIMES = "resident dataset loaded without its GPS time blocks (pcq_query_resident_load_with, PCQ_RESIDENT_TIME)";

// A query's predicate but for its box: the class is the whole byte (last.rs:259-262), the times Range { start, end }: start <= t && t < end
// (las.rs:336).
static pcq_predicate predicate(int kind, uint8_t cls = 0, double start = 0.0, double end = 0.0) {
    pcq_predicate pred{};
    pred.kind = kind, pred.cls = cls, pred.wmin[0] = start, pred.wmax[0] = end;
    return pred;
}

// The prologue the reference runs per file before its loop, in its order: the header early-out (last.rs:92-94), the f64 -> local
// integer box (:98-109) with its error, then the skip of a file without points.  *scan: the file is to be scanned with pred's box.
static int box_prologue(const ResidentFile &f, const AABB &bounds, pcq_predicate *pred, bool *scan) {
    *scan = false;
    if (!f.header.bounds.intersects(bounds)) return PCQ_OK;
    const int rc = pcq_box_to_local(bounds.min, bounds.max, f.header.scale, f.header.offset, pred->lmin, pred->lmax);
    *scan = !rc && f.header.number_of_points != 0;
    return rc;
}

// The resident blocks of a file as a scan's columns: the positions, and the second column a predicate of `kind` tests (the class
// block; the time block for the kinds that test GPS times; none for a plain box).
static pcq_columns file_columns(const ResidentFile &f, int kind) {
    pcq_columns c{};
    c.xyz = f.xyz, c.xyz_stride = 12, c.n = f.header.number_of_points;  // last.rs:114-121
    if (kind == PCQ_PRED_CLASS || kind == PCQ_PRED_BOUNDS_CLASS) c.cls = f.cls, c.cls_stride = 1;  // :138-142
    if (kind == PCQ_PRED_TIME || kind == PCQ_PRED_BOUNDS_TIME) c.cls = f.time, c.cls_stride = 8;
    for (int a = 0; a < 3; a++) c.scale[a] = f.header.scale[a], c.offset[a] = f.header.offset[a];  // :156-160
    return c;
}

// The dataset's device counter, `words` words at least.  A call that failed has left launches on the context's stream that add
// into the old counter, so the stream is drained before that one is freed.
int ResidentDataset::ensure_counter(size_t words) {
    if (words <= counter_words_) return PCQ_OK;
    void *p = nullptr;
    int rc = pcq_device_alloc(ctx_, words * 8, &p);
    if (!rc) rc = pcq_ctx_synchronize(ctx_);
    if (rc) {
        if (p) pcq_device_free(ctx_, p);
        return rc;
    }
    pcq_device_free(ctx_, counter_);
    counter_ = (uint64_t *)p;
    counter_words_ = words;
    return PCQ_OK;
}

// `words` words of the counter zeroed, `launch` adding into them on the context's stream, then copied back (which waits for the
// stream).  `out` is written only when everything has succeeded.
template <typename Launch>
Status ResidentDataset::read_counts(size_t words, Launch launch, uint64_t *out) {
    uint64_t few[PCQ_CLASS_BINS];
    std::vector<uint64_t> many(words > PCQ_CLASS_BINS ? words : 0);  // (more boxes than classes: count_bounds_many; time bins)
    uint64_t *got = many.empty() ? few : many.data();
    int rc = ensure_counter(words);
    if (!rc) rc = pcq_device_memset(ctx_, counter_, 0, words * 8, nullptr);
    if (!rc) rc = launch();
    if (!rc) rc = pcq_copy_to_host(ctx_, got, counter_, words * 8);
    if (rc) return Status::FromLib(rc);
    memcpy(out, got, words * 8);
    return Status::Ok();
}

// The segments of one batched launch: the surviving files' columns, each with its predicate, and their points.
struct ResidentDataset::Segments {
    std::vector<pcq_columns> cols;
    std::vector<pcq_predicate> preds;
    uint64_t scanned = 0;
};

// The prologue for every file: a segment per surviving file, `pred` with the box in that file's integers, `col_kind` picking
// the second column.
Status ResidentDataset::box_segments(const AABB &bounds, pcq_predicate pred, int col_kind, Segments *seg) {
    for (const auto &f : files_) {
        bool go;
        const int brc = box_prologue(f, bounds, &pred, &go);
        if (brc) return Status::FromLib(brc);
        if (!go) continue;
        seg->cols.push_back(file_columns(f, col_kind));
        seg->preds.push_back(pred);
        seg->scanned += f.header.number_of_points;
    }
    return Status::Ok();
}

// ONE batched launch of `entry` over the segments, `words` words of counts into the dataset's counter and back.
Status ResidentDataset::run(BatchEntry entry, size_t words, const Segments &seg, uint64_t *out) {
    return read_counts(
        words, [&] { return seg.cols.empty() ? (int)PCQ_OK : entry(ctx_, seg.cols.data(), seg.preds.data(), seg.cols.size(), counter_, nullptr); }, out);
}

// The three box counts: per file the prologue the reference runs before its loop, then one batched launch over the surviving
// files.  `pred` brings the kind and what it tests besides the box (cls; [wmin[0], wmax[0])); the kind picks the entry and the
// second column (PCQ_PRED_BOUNDS_CLASS: the classification block, PCQ_PRED_BOUNDS_TIME: the time block).
Status ResidentDataset::count_box(const AABB &bounds, const pcq_predicate &pred, uint64_t *matches, uint64_t *points_scanned) {
    Segments seg;
    Status st = box_segments(bounds, pred, pred.kind, &seg);
    if (!st.ok()) return st;
    if (points_scanned) *points_scanned = seg.scanned;
    return run(pred.kind == PCQ_PRED_BOUNDS_CLASS  ? pcq_scan_dev_count_batch_combined
               : pred.kind == PCQ_PRED_BOUNDS_TIME ? pcq_scan_dev_count_batch_bounds_time
                                                   : pcq_scan_dev_count_batch,
               1, seg, matches);
}

// `--bounds` over the dataset, count only: BoundsSearcher + CountCollector + the sum of main.rs:164-180.
Status ResidentDataset::count_bounds(const AABB &bounds, uint64_t *matches, uint64_t *points_scanned) {
    return count_box(bounds, predicate(PCQ_PRED_BOUNDS), matches, points_scanned);
}

// Many boxes, one pass per group of PCQ_MULTI_BOX_MAX (pcq_scan_dev_count_batch_multi).  First the prologue of count_box for every
// box and file, boxes outermost: the first failure is that of the lowest box whose own call fails, found before anything is
// enqueued or written.  A file whose header misses box q carries an EMPTY predicate in slot q — also where its points would
// match in integer space: the early-out decides, as in the reference; a file no box of a group meets is no segment of that
// group's launch.  All launches go to the context's stream, the counts into a word per box of the dataset's counter; the host
// waits for the copy of the counts at the end, and once per group whose table differs from the one in HBM (pcq_upload_segment_table).
Status ResidentDataset::count_bounds_many(size_t nboxes, const double *bmin, const double *bmax, uint64_t *matches, uint64_t *points_scanned,
                                          uint64_t *points_read) {
    if (nboxes == 0) return Status::Ok();
    const size_t nfiles = files_.size();
    pcq_predicate none{};  // "not asked of this file"
    none.kind = PCQ_PRED_BOUNDS;
    for (int a = 0; a < 3; a++) none.lmin[a] = 1, none.lmax[a] = 0;
    std::vector<pcq_predicate> local(nboxes * nfiles, none);  // [box][file]
    std::vector<uint8_t> asked(nboxes * nfiles, 0);
    std::vector<uint64_t> scanned(nboxes, 0);
    Status st = Status::Ok();
    for (size_t q = 0; q < nboxes; q++) {
        AABB bounds;
        st = AABB::from_min_max(bmin + 3 * q, bmax + 3 * q, &bounds);
        if (!st.ok()) return st;
        for (size_t i = 0; i < nfiles; i++) {
            pcq_predicate pred = predicate(PCQ_PRED_BOUNDS);
            bool go;
            const int brc = box_prologue(files_[i], bounds, &pred, &go);
            if (brc) return Status::FromLib(brc);
            if (!go) continue;
            local[q * nfiles + i] = pred;
            asked[q * nfiles + i] = 1;
            scanned[q] += files_[i].header.number_of_points;
        }
    }
    uint64_t read = 0;
    // (the copy back waits for the context's stream; a group whose table differs from the one in HBM has waited once before its upload)
    st = read_counts(nboxes, [&] {
        std::vector<pcq_columns> cols;
        std::vector<pcq_predicate> preds;
        int rc = PCQ_OK;
        for (size_t q0 = 0; q0 < nboxes && !rc; q0 += PCQ_MULTI_BOX_MAX) {
            const size_t nq = nboxes - q0 < PCQ_MULTI_BOX_MAX ? nboxes - q0 : (size_t)PCQ_MULTI_BOX_MAX;
            cols.clear();
            preds.clear();
            for (size_t i = 0; i < nfiles; i++) {
                bool met = false;
                for (size_t q = q0; q < q0 + nq; q++) met |= asked[q * nfiles + i] != 0;
                if (!met) continue;
                cols.push_back(file_columns(files_[i], PCQ_PRED_BOUNDS));
                for (size_t q = q0; q < q0 + nq; q++) preds.push_back(local[q * nfiles + i]);
                read += files_[i].header.number_of_points;
            }
            if (!cols.empty()) rc = pcq_scan_dev_count_batch_multi(ctx_, cols.data(), preds.data(), cols.size(), nq, counter_ + q0, nullptr);
        }
        return rc;
    }, matches);
    if (!st.ok()) return st;
    if (points_scanned)
        for (size_t q = 0; q < nboxes; q++) points_scanned[q] = scanned[q];
    if (points_read) *points_read = read;
    return Status::Ok();
}

// What is in this box, by class: the prologue of count_box with a plain box predicate, then ONE pcq_scan_dev_class_hist_batch over
// the positions and class blocks of the surviving files into PCQ_CLASS_BINS words of the dataset's counter.  `hist` is written
// only when everything has succeeded.
Status ResidentDataset::count_bounds_by_class(const AABB &bounds, uint64_t *hist, uint64_t *points_scanned) {
    Segments seg;
    Status st = box_segments(bounds, predicate(PCQ_PRED_BOUNDS), PCQ_PRED_BOUNDS_CLASS, &seg);
    if (st.ok()) st = run(pcq_scan_dev_class_hist_batch, PCQ_CLASS_BINS, seg, hist);
    if (st.ok() && points_scanned) *points_scanned = seg.scanned;
    return st;
}

// When was this box scanned: the prologue of count_box with a plain box predicate, then the bins in their order in groups of
// PCQ_TIME_BINS_MAX, ONE pcq_scan_dev_time_hist_batch per group over the positions and time blocks of the surviving files: edges
// q0 .. q0 + nq, counter words from q0.  All launches go to the context's stream; the host waits for the copy of the counts at the
// end (and once per group for the upload of its edges: pcq_upload_segment_table).  The caller has checked the edges.  `hist` and
// `points_scanned` are written only when everything has succeeded.
Status ResidentDataset::count_bounds_by_time(const double bmin[3], const double bmax[3], const double *edges, size_t nbins, uint64_t *hist,
                                             uint64_t *points_scanned) {
    if (!with_times_) return Status::Err(PCQ_ERR_ARG, NO_TIMES);
    AABB bounds;
    Status st = AABB::from_min_max(bmin, bmax, &bounds);
    if (!st.ok()) return st;
    Segments seg;
    st = box_segments(bounds, predicate(PCQ_PRED_BOUNDS), PCQ_PRED_BOUNDS_TIME, &seg);
    if (!st.ok()) return st;
    st = read_counts(nbins, [&] {
        int rc = PCQ_OK;
        for (size_t q0 = 0; q0 < nbins && !rc && !seg.cols.empty(); q0 += PCQ_TIME_BINS_MAX) {
            const size_t nq = nbins - q0 < PCQ_TIME_BINS_MAX ? nbins - q0 : (size_t)PCQ_TIME_BINS_MAX;
            rc = pcq_scan_dev_time_hist_batch(ctx_, seg.cols.data(), seg.preds.data(), seg.cols.size(), edges + q0, nq, counter_ + q0, nullptr);
        }
        return rc;
    }, hist);
    if (st.ok() && points_scanned) *points_scanned = seg.scanned;
    return st;
}

// How many points lie inside this outline: the prologue of count_box with the world box of the outline, then per surviving file
// the outline in that file's lattice (polygon_plan.h: the rounded vertices and their box, or PCQ_ERR_UNSUPPORTED) with the z range of
// the converted box, then ONE pcq_scan_dev_count_batch_polygon over the positions of the surviving files.  `matches` and
// `points_scanned` are written only when everything has succeeded.
Status ResidentDataset::count_polygon(size_t nverts, const double *xy, double zmin, double zmax, uint64_t *matches, uint64_t *points_scanned) {
    double lo[2], hi[2];
    polygon_plan::world_box(nverts, xy, lo, hi);
    const double bmin[3] = {lo[0], lo[1], zmin}, bmax[3] = {hi[0], hi[1], zmax};
    AABB bounds;
    Status st = AABB::from_min_max(bmin, bmax, &bounds);
    if (!st.ok()) return st;
    Segments seg;
    std::vector<int32_t> verts;  // [segment][nverts][2]
    pcq_predicate pred = predicate(PCQ_PRED_BOUNDS);
    for (const auto &f : files_) {
        bool go;
        const int brc = box_prologue(f, bounds, &pred, &go);
        if (brc) return Status::FromLib(brc);
        if (!go) continue;
        polygon_plan::Outline o;
        const polygon_plan::Refusal why = polygon_plan::to_lattice(nverts, xy, f.header.scale, f.header.offset, &o);
        if (why) return Status::Err(PCQ_ERR_UNSUPPORTED, polygon_plan::refusal_text(why) + f.path);
        for (int a = 0; a < 2; a++) pred.lmin[a] = o.lo[a], pred.lmax[a] = o.hi[a];
        verts.insert(verts.end(), o.xy.begin(), o.xy.end());
        seg.cols.push_back(file_columns(f, PCQ_PRED_BOUNDS));
        seg.preds.push_back(pred);
        seg.scanned += f.header.number_of_points;
    }
    uint64_t got = 0;
    st = read_counts(1, [&] {
        return seg.cols.empty() ? (int)PCQ_OK
                                : pcq_scan_dev_count_batch_polygon(ctx_, seg.cols.data(), seg.preds.data(), verts.data(), seg.cols.size(), nverts, counter_, nullptr);
    }, &got);
    if (!st.ok()) return st;
    *matches = got;
    if (points_scanned) *points_scanned = seg.scanned;
    return Status::Ok();
}

// The prologue of the three rasters of a box (count_bounds_raster, bounds_zrange_raster, bounds_zmean_raster): the prologue of count_box with the world
// box of the whole raster, then per surviving file the cell as a whole number of that file's lattice steps (else
// PCQ_ERR_UNSUPPORTED) and the file's box cut to full cells: lmin .. lmin + n k - 1 on x and y.  cells: [segment][2], the cell in
// each segment's lattice steps.  z_lattice: a surviving file whose z scale is not finite or not above 0 is PCQ_ERR_UNSUPPORTED as
// well (the height raster's conversion to world z has to be monotone).
Status ResidentDataset::raster_segments(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny, bool z_lattice, int col_kind, Segments *seg,
                                        std::vector<uint32_t> *cells) {
    const double bmax[3] = {bmin[0] + (double)nx * cell_size, bmin[1] + (double)ny * cell_size, zmax};
    AABB bounds;
    Status st = AABB::from_min_max(bmin, bmax, &bounds);
    if (!st.ok()) return st;
    const uint64_t dim[2] = {nx, ny};
    pcq_predicate pred = predicate(PCQ_PRED_BOUNDS);
    for (const auto &f : files_) {
        bool go;
        const int brc = box_prologue(f, bounds, &pred, &go);
        if (brc) return Status::FromLib(brc);
        if (!go) continue;
        for (int a = 0; a < 2; a++) {
            const double cw = cell_size / f.header.scale[a], k = std::nearbyint(cw);
            if (!(k >= 1.0 && k <= 4294967295.0) || !(std::fabs(cw - k) <= 1e-9 * k))
                return Status::Err(PCQ_ERR_UNSUPPORTED, "raster: the cell size is not a whole number of lattice steps of " + f.path);
            if (pred.lmin[a] < INT32_MIN || pred.lmin[a] > INT32_MAX)
                return Status::Err(PCQ_ERR_UNSUPPORTED, "raster: the origin lies outside the lattice of " + f.path);
            cells->push_back((uint32_t)k);
            pred.lmax[a] = pred.lmin[a] + (int64_t)dim[a] * (int64_t)k - 1;
        }
        const double sz = f.header.scale[2];
        if (z_lattice && (!(sz > 0.0) || sz - sz != 0.0))
            return Status::Err(PCQ_ERR_UNSUPPORTED, "height raster: the z scale is not finite and above 0 in " + f.path);
        seg->cols.push_back(file_columns(f, col_kind));
        seg->preds.push_back(pred);
        seg->scanned += f.header.number_of_points;
    }
    return Status::Ok();
}

// A raster of nx x ny cells cut into the blocks of one launch each, at most `limit` cells: whole rows, or row pieces where a row
// alone is too long; row-major over the raster, block b's words following block b - 1's (`at`).
namespace {
struct RasterBlock {
    uint64_t x0, y0, w, h;
    size_t at;
};
std::vector<RasterBlock> raster_blocks(uint64_t nx, uint64_t ny, uint64_t limit) {
    const uint64_t bw = nx < limit ? nx : limit;
    const uint64_t bh = limit / bw < ny ? limit / bw : ny;
    std::vector<RasterBlock> out;
    size_t at = 0;
    for (uint64_t y0 = 0; y0 < ny; y0 += bh)
        for (uint64_t x0 = 0; x0 < nx; x0 += bw) {
            const RasterBlock b = {x0, y0, nx - x0 < bw ? nx - x0 : bw, ny - y0 < bh ? ny - y0 : bh, at};
            out.push_back(b);
            at += (size_t)(b.w * b.h);
        }
    return out;
}
// Segment i's predicate for a block: the integer sub-box of its file — empty where it starts beyond the i32 range.
pcq_predicate block_predicate(pcq_predicate p, const uint32_t *cell, const RasterBlock &b) {
    const uint64_t off[2] = {b.x0, b.y0}, ext[2] = {b.w, b.h};
    for (int a = 0; a < 2; a++) {
        const int64_t k = cell[a];
        p.lmin[a] += (int64_t)off[a] * k;
        p.lmax[a] = p.lmin[a] + (int64_t)ext[a] * k - 1;
        if (p.lmin[a] > INT32_MAX) p.lmin[0] = 1, p.lmax[0] = 0;  // no stored point can lie in this block: an empty predicate
    }
    if (p.lmin[0] > p.lmax[0]) p.lmin[1] = 1, p.lmax[1] = 0;
    return p;
}
// the words of the blocks, one after the other in `got`, into the row-major raster
template <typename T>
void scatter_blocks(const std::vector<RasterBlock> &blocks, const T *got, uint64_t nx, T *raster) {
    for (const RasterBlock &b : blocks)
        for (uint64_t y = 0; y < b.h; y++) memcpy(raster + (b.y0 + y) * nx + b.x0, got + b.at + (size_t)(y * b.w), (size_t)b.w * sizeof(T));
}
}  // namespace

// Where in this box are the points: raster_segments, then a raster of at most PCQ_RASTER_CELLS_MAX cells is ONE
// pcq_scan_dev_raster_batch; a larger one is cut into blocks (raster_blocks), each block the integer sub-box of every file and one
// launch into its own counter words.  All launches go to the context's stream; the counts are copied back once and scattered.
// `raster` and `points_scanned` are written only when everything has succeeded.
Status ResidentDataset::count_bounds_raster(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny, uint64_t *raster,
                                            uint64_t *points_scanned) {
    Segments seg;
    std::vector<uint32_t> cells;  // [segment][2]
    Status st = raster_segments(bmin, zmax, cell_size, nx, ny, /*z_lattice=*/false, PCQ_PRED_BOUNDS, &seg, &cells);
    if (!st.ok()) return st;
    const std::vector<RasterBlock> blocks = raster_blocks(nx, ny, PCQ_RASTER_CELLS_MAX);
    const size_t words = (size_t)(nx * ny);
    std::vector<uint64_t> got(words);
    st = read_counts(words, [&] {
        int rc = PCQ_OK;
        std::vector<pcq_predicate> preds(seg.preds.size());
        for (size_t b = 0; b < blocks.size() && !rc && !seg.cols.empty(); b++) {
            for (size_t i = 0; i < preds.size(); i++) preds[i] = block_predicate(seg.preds[i], &cells[2 * i], blocks[b]);
            rc = pcq_scan_dev_raster_batch(ctx_, seg.cols.data(), preds.data(), cells.data(), preds.size(), (uint32_t)blocks[b].w, (uint32_t)blocks[b].h,
                                           counter_ + blocks[b].at, nullptr);
        }
        return rc;
    }, got.data());
    if (!st.ok()) return st;
    scatter_blocks(blocks, got.data(), nx, raster);
    if (points_scanned) *points_scanned = seg.scanned;
    return Status::Ok();
}

// How high is this box, cell by cell: raster_segments (with the z lattice rule), then the surviving files in groups of one z
// lattice — bitwise-equal (scale[2], offset[2]), in the order of their first file: the integers of two lattices are not comparable.
// Per group the dataset's counter holds nx * ny i32 minima and behind them nx * ny i32 maxima, uploaded as INT32_MAX / INT32_MIN
// (pcq_device_memset is bytewise); per block of at most PCQ_ZRANGE_CELLS_MAX cells ONE pcq_scan_dev_zrange_raster_batch over the
// group's files on the context's stream; then one copy back.  The words become world values (Z as f64 * scale[2]) + offset[2], the
// reference's two-rounding rebuild (last.rs:156-160); that map is non-decreasing in Z for a scale above 0, so a cell's world minimum
// is the image of its integer minimum whatever the order of the points.  Groups are merged with < and > on f64; a cell no point
// reached is NaN in both arrays.  `zlo`, `zhi` and `points_scanned` are written only when everything has succeeded.
Status ResidentDataset::bounds_zrange_raster(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny, double *zlo, double *zhi,
                                             uint64_t *points_scanned) {
    Segments seg;
    std::vector<uint32_t> cells;  // [segment][2]
    Status st = raster_segments(bmin, zmax, cell_size, nx, ny, /*z_lattice=*/true, PCQ_PRED_BOUNDS, &seg, &cells);
    if (!st.ok()) return st;
    const std::vector<RasterBlock> blocks = raster_blocks(nx, ny, PCQ_ZRANGE_CELLS_MAX);
    const size_t words = (size_t)(nx * ny), nseg = seg.cols.size();
    const double nan = std::nan("");
    std::vector<double> lo(words, nan), hi(words, nan);
    std::vector<int32_t> preset(2 * words), got(2 * words), zmin(words), zmax_i(words);
    std::fill(preset.begin(), preset.begin() + words, INT32_MAX);
    std::fill(preset.begin() + words, preset.end(), INT32_MIN);
    std::vector<uint8_t> grouped(nseg, 0);
    for (size_t first = 0; first < nseg; first++) {
        if (grouped[first]) continue;
        const double scale = seg.cols[first].scale[2], offset = seg.cols[first].offset[2];
        Segments grp;
        std::vector<uint32_t> gcells;
        for (size_t i = first; i < nseg; i++) {
            if (grouped[i] || memcmp(&seg.cols[i].scale[2], &scale, 8) || memcmp(&seg.cols[i].offset[2], &offset, 8)) continue;
            grouped[i] = 1;
            grp.cols.push_back(seg.cols[i]);
            grp.preds.push_back(seg.preds[i]);
            gcells.push_back(cells[2 * i]), gcells.push_back(cells[2 * i + 1]);
        }
        int rc = ensure_counter(words);  // (2 x words i32)
        if (!rc) rc = pcq_ctx_synchronize(ctx_);  // (a call that failed may have left launches that write the counter)
        if (!rc) rc = pcq_copy_to_device(ctx_, counter_, preset.data(), 2 * words * sizeof(int32_t));
        int32_t *const d_zmin = reinterpret_cast<int32_t *>(counter_), *const d_zmax = d_zmin + words;
        std::vector<pcq_predicate> preds(grp.preds.size());
        for (size_t b = 0; b < blocks.size() && !rc; b++) {
            for (size_t i = 0; i < preds.size(); i++) preds[i] = block_predicate(grp.preds[i], &gcells[2 * i], blocks[b]);
            rc = pcq_scan_dev_zrange_raster_batch(ctx_, grp.cols.data(), preds.data(), gcells.data(), preds.size(), (uint32_t)blocks[b].w,
                                                  (uint32_t)blocks[b].h, d_zmin + blocks[b].at, d_zmax + blocks[b].at, nullptr);
        }
        if (!rc) rc = pcq_copy_to_host(ctx_, got.data(), counter_, 2 * words * sizeof(int32_t));
        if (rc) return Status::FromLib(rc);
        scatter_blocks(blocks, got.data(), nx, zmin.data());
        scatter_blocks(blocks, got.data() + words, nx, zmax_i.data());
        for (size_t c = 0; c < words; c++) {
            if (zmin[c] > zmax_i[c]) continue;  // (no point of this group)
            const double a = ((double)zmin[c] * scale) + offset, b = ((double)zmax_i[c] * scale) + offset;
            if (!(lo[c] <= a)) lo[c] = a;  // (NaN: nothing yet)
            if (!(hi[c] >= b)) hi[c] = b;
        }
    }
    memcpy(zlo, lo.data(), words * sizeof(double));
    memcpy(zhi, hi.data(), words * sizeof(double));
    if (points_scanned) *points_scanned = seg.scanned;
    return Status::Ok();
}

// How high above the ground is this box, cell by cell: the body of bounds_zrange_raster, spelt out beside it so that that entry
// compiles as it did — the same prologue (with the class blocks in the columns), groups, presets, blocks and copy back — with ONE
// pcq_scan_dev_zrange_raster_batch_classes per group and block of at most PCQ_ZRANGE_CLASSES_CELLS_MAX cells.  The two arrays are
// independent: a minimum that left INT32_MAX becomes a world value whatever the maximum holds, and the reverse, so a ground point
// stored at INT32_MAX and a surface point stored at INT32_MIN read as no point (include/pcq_query_canopy.h: the sentinel rule).
// height = zsurface - zground in f64, NaN where either is.  Both sets empty: the prologue's refusals, then NaN everywhere without a
// launch.  The outputs are written only when everything has succeeded.
Status ResidentDataset::bounds_canopy_raster(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny,
                                             const uint32_t ground_set[8], const uint32_t surface_set[8], double *zground, double *zsurface,
                                             double *height, uint64_t *points_scanned) {
    Segments seg;
    std::vector<uint32_t> cells;  // [segment][2]
    Status st = raster_segments(bmin, zmax, cell_size, nx, ny, /*z_lattice=*/true, PCQ_PRED_BOUNDS_CLASS, &seg, &cells);
    if (!st.ok()) return st;
    uint32_t any = 0;
    for (int w = 0; w < 8; w++) any |= ground_set[w] | surface_set[w];
    const std::vector<RasterBlock> blocks = raster_blocks(nx, ny, PCQ_ZRANGE_CLASSES_CELLS_MAX);
    const size_t words = (size_t)(nx * ny), nseg = seg.cols.size();
    const double nan = std::nan("");
    std::vector<double> lo(words, nan), hi(words, nan);
    std::vector<int32_t> preset(2 * words), got(2 * words), zmin(words), zmax_i(words);
    std::fill(preset.begin(), preset.begin() + words, INT32_MAX);
    std::fill(preset.begin() + words, preset.end(), INT32_MIN);
    std::vector<uint8_t> grouped(nseg, 0);
    for (size_t first = 0; first < nseg && any; first++) {
        if (grouped[first]) continue;
        const double scale = seg.cols[first].scale[2], offset = seg.cols[first].offset[2];
        Segments grp;
        std::vector<uint32_t> gcells;
        for (size_t i = first; i < nseg; i++) {
            if (grouped[i] || memcmp(&seg.cols[i].scale[2], &scale, 8) || memcmp(&seg.cols[i].offset[2], &offset, 8)) continue;
            grouped[i] = 1;
            grp.cols.push_back(seg.cols[i]);
            grp.preds.push_back(seg.preds[i]);
            gcells.push_back(cells[2 * i]), gcells.push_back(cells[2 * i + 1]);
        }
        int rc = ensure_counter(words);  // (2 x words i32)
        if (!rc) rc = pcq_ctx_synchronize(ctx_);  // (a call that failed may have left launches that write the counter)
        if (!rc) rc = pcq_copy_to_device(ctx_, counter_, preset.data(), 2 * words * sizeof(int32_t));
        int32_t *const d_zmin = reinterpret_cast<int32_t *>(counter_), *const d_zmax = d_zmin + words;
        std::vector<pcq_predicate> preds(grp.preds.size());
        for (size_t b = 0; b < blocks.size() && !rc; b++) {
            for (size_t i = 0; i < preds.size(); i++) preds[i] = block_predicate(grp.preds[i], &gcells[2 * i], blocks[b]);
            rc = pcq_scan_dev_zrange_raster_batch_classes(ctx_, grp.cols.data(), preds.data(), gcells.data(), preds.size(), (uint32_t)blocks[b].w,
                                                          (uint32_t)blocks[b].h, ground_set, surface_set, d_zmin + blocks[b].at,
                                                          d_zmax + blocks[b].at, nullptr);
        }
        if (!rc) rc = pcq_copy_to_host(ctx_, got.data(), counter_, 2 * words * sizeof(int32_t));
        if (rc) return Status::FromLib(rc);
        scatter_blocks(blocks, got.data(), nx, zmin.data());
        scatter_blocks(blocks, got.data() + words, nx, zmax_i.data());
        for (size_t c = 0; c < words; c++) {
            if (zmin[c] != INT32_MAX) {  // (the sentinel: no ground point of this group)
                const double a = ((double)zmin[c] * scale) + offset;
                if (!(lo[c] <= a)) lo[c] = a;  // (NaN: nothing yet)
            }
            if (zmax_i[c] != INT32_MIN) {
                const double b = ((double)zmax_i[c] * scale) + offset;
                if (!(hi[c] >= b)) hi[c] = b;
            }
        }
    }
    memcpy(zground, lo.data(), words * sizeof(double));
    memcpy(zsurface, hi.data(), words * sizeof(double));
    if (height)
        for (size_t c = 0; c < words; c++) height[c] = hi[c] - lo[c];  // (NaN where either is)
    if (points_scanned) *points_scanned = seg.scanned;
    return Status::Ok();
}

// How high is this box on average, cell by cell: raster_segments (with the z lattice rule), the surviving files in groups of one z
// lattice as for bounds_zrange_raster, and within a group the files, in load order, in batches of fewer than 2^32 points
// (zsum_plan.h), so that a batch's i64 sums cannot wrap.  Per batch the dataset's counter holds nx * ny u64 counts and behind them
// nx * ny i64 sums, zeroed; per block of at most PCQ_ZSUM_CELLS_MAX cells ONE pcq_scan_dev_zsum_raster_batch over the batch's files
// on the context's stream; then one copy back.  The merge, per cell and in batch order (groups in the order of their first file):
//
//     W += offset * (double)cnt + scale * (double)(int64_t)sum;   N += cnt;
//     count[c] = N;   zmean[c] = N ? W / (double)N : NaN
//
// every product rounded before the add: this file is compiled with -ffp-contract=off (host/Makefile), and the two products are
// named values below.  `count`, `zmean` and `points_scanned` are written only when everything has succeeded.
//
// class_set (null: every point) restricts cnt and sum to the points whose class byte is in the set: the columns then carry the class
// blocks and the launch is pcq_scan_dev_zsum_raster_batch_classes; everything else is the same code.  An empty set makes every
// refusal and no launch: cnt and sum are 0 in every batch.
Status ResidentDataset::bounds_zmean_raster(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny, uint64_t *count,
                                            double *zmean, uint64_t *points_scanned) {
    return zmean_raster(bmin, zmax, cell_size, nx, ny, nullptr, count, zmean, points_scanned);
}
Status ResidentDataset::bounds_zmean_raster_classes(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny,
                                                    const uint32_t class_set[8], uint64_t *count, double *zmean, uint64_t *points_scanned) {
    return zmean_raster(bmin, zmax, cell_size, nx, ny, class_set, count, zmean, points_scanned);
}
Status ResidentDataset::zmean_raster(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny, const uint32_t *class_set,
                                     uint64_t *count, double *zmean, uint64_t *points_scanned) {
    Segments seg;
    std::vector<uint32_t> cells;  // [segment][2]
    Status st = raster_segments(bmin, zmax, cell_size, nx, ny, /*z_lattice=*/true, class_set ? PCQ_PRED_BOUNDS_CLASS : PCQ_PRED_BOUNDS, &seg, &cells);
    if (!st.ok()) return st;
    bool none = class_set != nullptr;  // the empty set
    for (int w = 0; class_set && w < 8; w++) none = none && class_set[w] == 0;
    const std::vector<RasterBlock> blocks = raster_blocks(nx, ny, PCQ_ZSUM_CELLS_MAX);
    const size_t words = (size_t)(nx * ny), nseg = seg.cols.size();
    std::vector<double> W(words, 0.0);
    std::vector<uint64_t> N(words, 0), got(2 * words), cnt(words), sum(words);
    std::vector<uint8_t> grouped(nseg, 0);
    for (size_t first = 0; first < nseg; first++) {
        if (grouped[first]) continue;
        const double scale = seg.cols[first].scale[2], offset = seg.cols[first].offset[2];
        std::vector<size_t> members;  // of seg, in load order
        std::vector<uint64_t> points;
        for (size_t i = first; i < nseg; i++) {
            if (grouped[i] || memcmp(&seg.cols[i].scale[2], &scale, 8) || memcmp(&seg.cols[i].offset[2], &offset, 8)) continue;
            grouped[i] = 1;
            members.push_back(i);
            points.push_back(seg.cols[i].n);
        }
        std::vector<zsum_plan::Batch> batches;
        size_t refused = 0;
        if (!zsum_plan::cut(points, zsum_plan::POINTS_LIMIT, &batches, &refused)) {
            std::string path;  // (a file with points owns its positions block)
            for (const auto &f : files_)
                if (f.xyz == seg.cols[members[refused]].xyz) path = f.path;
            return Status::Err(PCQ_ERR_UNSUPPORTED, "mean-height raster: 2^32 points or more in " + path);
        }
        for (const zsum_plan::Batch &batch : batches) {
            if (none) break;  // (W and N stay 0)
            Segments grp;
            std::vector<uint32_t> gcells;
            for (size_t m = batch.begin; m < batch.end; m++) {
                const size_t i = members[m];
                grp.cols.push_back(seg.cols[i]);
                grp.preds.push_back(seg.preds[i]);
                gcells.push_back(cells[2 * i]), gcells.push_back(cells[2 * i + 1]);
            }
            st = read_counts(2 * words, [&] {
                int rc = PCQ_OK;
                int64_t *const d_sum = reinterpret_cast<int64_t *>(counter_ + words);
                std::vector<pcq_predicate> preds(grp.preds.size());
                for (size_t b = 0; b < blocks.size() && !rc; b++) {
                    for (size_t i = 0; i < preds.size(); i++) preds[i] = block_predicate(grp.preds[i], &gcells[2 * i], blocks[b]);
                    rc = class_set ? pcq_scan_dev_zsum_raster_batch_classes(ctx_, grp.cols.data(), preds.data(), gcells.data(), preds.size(),
                                                                            (uint32_t)blocks[b].w, (uint32_t)blocks[b].h, class_set,
                                                                            counter_ + blocks[b].at, d_sum + blocks[b].at, nullptr)
                                   : pcq_scan_dev_zsum_raster_batch(ctx_, grp.cols.data(), preds.data(), gcells.data(), preds.size(),
                                                                    (uint32_t)blocks[b].w, (uint32_t)blocks[b].h, counter_ + blocks[b].at,
                                                                    d_sum + blocks[b].at, nullptr);
                }
                return rc;
            }, got.data());
            if (!st.ok()) return st;
            scatter_blocks(blocks, got.data(), nx, cnt.data());
            scatter_blocks(blocks, got.data() + words, nx, sum.data());
            for (size_t c = 0; c < words; c++) {
                const double a = offset * (double)cnt[c], b = scale * (double)(int64_t)sum[c];
                W[c] += a + b;
                N[c] += cnt[c];
            }
        }
    }
    const double nan = std::nan("");
    for (size_t c = 0; c < words; c++) count[c] = N[c], zmean[c] = N[c] ? W[c] / (double)N[c] : nan;
    if (points_scanned) *points_scanned = seg.scanned;
    return Status::Ok();
}

// How rough is this box, cell by cell: the prologue, the groups of one z lattice and the batches of fewer than 2^32 points of
// zmean_raster (without a class set), so that neither a batch's i64 sums nor the two u64 halves of its sums of squares can wrap.  Per
// batch the dataset's counter holds four arrays of nx * ny words, zeroed — counts, sums, the low and the high halves of the sums of
// squares; per block of at most PCQ_ZMOMENTS_CELLS_MAX cells ONE pcq_scan_dev_zmoments_raster_batch over the batch's files on the
// context's stream; then one copy back.  The merge, per cell and in batch order, is zmoments_merge.h's, which states the formula.
// `count`, `zmean`, `zstd` and `points_scanned` are written only when everything has succeeded.
Status ResidentDataset::bounds_zstd_raster(const double bmin[3], double zmax, double cell_size, uint64_t nx, uint64_t ny, uint64_t *count,
                                           double *zmean, double *zstd, uint64_t *points_scanned) {
    Segments seg;
    std::vector<uint32_t> cells;  // [segment][2]
    Status st = raster_segments(bmin, zmax, cell_size, nx, ny, /*z_lattice=*/true, PCQ_PRED_BOUNDS, &seg, &cells);
    if (!st.ok()) return st;
    const std::vector<RasterBlock> blocks = raster_blocks(nx, ny, PCQ_ZMOMENTS_CELLS_MAX);
    const size_t words = (size_t)(nx * ny), nseg = seg.cols.size();
    std::vector<zmoments_merge::Cell> acc(words);
    std::vector<uint64_t> got(4 * words), part[4];
    for (auto &p : part) p.resize(words);
    std::vector<uint8_t> grouped(nseg, 0);
    for (size_t first = 0; first < nseg; first++) {
        if (grouped[first]) continue;
        const double scale = seg.cols[first].scale[2], offset = seg.cols[first].offset[2];
        std::vector<size_t> members;  // of seg, in load order
        std::vector<uint64_t> points;
        for (size_t i = first; i < nseg; i++) {
            if (grouped[i] || memcmp(&seg.cols[i].scale[2], &scale, 8) || memcmp(&seg.cols[i].offset[2], &offset, 8)) continue;
            grouped[i] = 1;
            members.push_back(i);
            points.push_back(seg.cols[i].n);
        }
        std::vector<zsum_plan::Batch> batches;
        size_t refused = 0;
        if (!zsum_plan::cut(points, zsum_plan::POINTS_LIMIT, &batches, &refused)) {
            std::string path;  // (a file with points owns its positions block)
            for (const auto &f : files_)
                if (f.xyz == seg.cols[members[refused]].xyz) path = f.path;
            return Status::Err(PCQ_ERR_UNSUPPORTED, "height-spread raster: 2^32 points or more in " + path);
        }
        for (const zsum_plan::Batch &batch : batches) {
            Segments grp;
            std::vector<uint32_t> gcells;
            for (size_t m = batch.begin; m < batch.end; m++) {
                const size_t i = members[m];
                grp.cols.push_back(seg.cols[i]);
                grp.preds.push_back(seg.preds[i]);
                gcells.push_back(cells[2 * i]), gcells.push_back(cells[2 * i + 1]);
            }
            st = read_counts(4 * words, [&] {
                int rc = PCQ_OK;
                std::vector<pcq_predicate> preds(grp.preds.size());
                for (size_t b = 0; b < blocks.size() && !rc; b++) {
                    for (size_t i = 0; i < preds.size(); i++) preds[i] = block_predicate(grp.preds[i], &gcells[2 * i], blocks[b]);
                    uint64_t *const at = counter_ + blocks[b].at;
                    rc = pcq_scan_dev_zmoments_raster_batch(ctx_, grp.cols.data(), preds.data(), gcells.data(), preds.size(), (uint32_t)blocks[b].w,
                                                            (uint32_t)blocks[b].h, at, reinterpret_cast<int64_t *>(at + words), at + 2 * words,
                                                            at + 3 * words, nullptr);
                }
                return rc;
            }, got.data());
            if (!st.ok()) return st;
            for (int a = 0; a < 4; a++) scatter_blocks(blocks, got.data() + a * words, nx, part[a].data());
            for (size_t c = 0; c < words; c++)
                zmoments_merge::add(acc[c], scale, offset, part[0][c], (int64_t)part[1][c], part[2][c], part[3][c]);
        }
    }
    for (size_t c = 0; c < words; c++) count[c] = acc[c].N, zmean[c] = zmoments_merge::zmean(acc[c]), zstd[c] = zmoments_merge::zstd(acc[c]);
    if (points_scanned) *points_scanned = seg.scanned;
    return Status::Ok();
}

// `--class` over the dataset, count only (last.rs:253-262: whole byte, no file-level early-out).
Status ResidentDataset::count_class(uint8_t cls, uint64_t *matches, uint64_t *points_scanned) {
    const pcq_predicate pred = predicate(PCQ_PRED_CLASS, cls);
    Segments seg;
    for (const auto &f : files_) {
        if (f.header.number_of_points == 0) continue;
        pcq_columns c{};
        c.cls = f.cls, c.cls_stride = 1, c.n = f.header.number_of_points;
        seg.cols.push_back(c);
        seg.preds.push_back(pred);
        seg.scanned += c.n;
    }
    if (points_scanned) *points_scanned = seg.scanned;
    return run(pcq_scan_dev_count_batch, 1, seg, matches);
}

// `--combine --bounds --class` over the dataset, count only (pcq_scan_dev_count_batch_combined over the positions and
// classification blocks).
Status ResidentDataset::count_bounds_class(const AABB &bounds, uint8_t cls, uint64_t *matches, uint64_t *points_scanned) {
    return count_box(bounds, predicate(PCQ_PRED_BOUNDS_CLASS, cls), matches, points_scanned);
}

// `--combine --bounds --time` over the dataset, count only (pcq_scan_dev_count_batch_bounds_time over the positions and time
// blocks).
Status ResidentDataset::count_bounds_time(const AABB &bounds, double start, double end, uint64_t *matches, uint64_t *points_scanned) {
    if (!with_times_) return Status::Err(PCQ_ERR_ARG, NO_TIMES);
    return count_box(bounds, predicate(PCQ_PRED_BOUNDS_TIME, 0, start, end), matches, points_scanned);
}

// One file of the search_* : execute_plan (search.cpp) with the resident blocks in place of the file.
Status ResidentDataset::scan(ResidentFile &f, const pcq_predicate &pred, ResultCollector &rc) {
    const uint64_t n = f.header.number_of_points;
    const bool time = pred.kind == PCQ_PRED_TIME || pred.kind == PCQ_PRED_BOUNDS_TIME;
    pcq_columns c = file_columns(f, time ? PCQ_PRED_TIME : PCQ_PRED_CLASS);  // the predicate's column, or the class of the records
    c.rgb = time ? nullptr : f.rgb, c.rgb_stride = 6;  // last.rs:145-153; a time record has no class and no colour
    c.first_index = rc.next_index;
    int r;
    if (dynamic_cast<GridSampledCollector *>(&rc)) {
        r = pcq_scan_dev(ctx_, &c, &pred, rc.handle(), nullptr);
    } else {
        if (!f.index) {
            r = pcq_index_new(ctx_, &f.index);
            if (r) return Status::FromLib(r);
        }
        r = pred.kind == PCQ_PRED_TIME           ? pcq_scan_dev_indexed_time(ctx_, &c, &pred, f.index, rc.handle(), nullptr)
            : pred.kind == PCQ_PRED_BOUNDS_TIME  ? pcq_scan_dev_indexed_bounds_time(ctx_, &c, &pred, f.index, rc.handle(), nullptr)
            : pred.kind == PCQ_PRED_BOUNDS_CLASS ? pcq_scan_dev_indexed_combined(ctx_, &c, &pred, f.index, rc.handle(), nullptr)
                                                 : pcq_scan_dev_indexed(ctx_, &c, &pred, f.index, rc.handle(), nullptr);
        if (!r) last_indices_.push_back(f.index);
    }
    rc.next_index += n;
    return Status::FromLib(r);
}

// Every file in load order through scan().  With `bounds`: the prologue of the box searches first, whose header early-out
// (last.rs:92-94) skips a file without moving the collector's file-order index, as the per-file search does.  Without: no
// file-level early-out (a header has no class and no time bounds).
Status ResidentDataset::search_files(const AABB *bounds, pcq_predicate pred, ResultCollector &rc) {
    last_indices_.clear();
    for (auto &f : files_) {
        bool go = f.header.number_of_points != 0;
        const int brc = bounds ? box_prologue(f, *bounds, &pred, &go) : (int)PCQ_OK;
        if (brc) return Status::FromLib(brc);
        if (!go) continue;
        Status st = scan(f, pred, rc);
        if (!st.ok()) return st;
    }
    return Status::Ok();
}

// search_last_file_by_bounds_optimized (last.rs:46-166) for every file.
Status ResidentDataset::search_bounds(const AABB &bounds, ResultCollector &rc) {
    if (!with_points_ && rc.has_points()) return Status::Err(PCQ_ERR_ARG, NO_COLOURS);
    return search_files(&bounds, predicate(PCQ_PRED_BOUNDS), rc);
}

// search_last_file_by_classification_optimized (last.rs:213-293) for every file.
Status ResidentDataset::search_class(uint8_t cls, ResultCollector &rc) {
    if (!with_points_ && rc.has_points()) return Status::Err(PCQ_ERR_ARG, NO_COLOURS);
    return search_files(nullptr, predicate(PCQ_PRED_CLASS, cls), rc);
}

// The combined search of search.cpp (DESIGN §8 "Combined searches") for every file: the prologue of search_bounds, then box
// AND class in one scan — through both parts of the file's chunk index for count and buffer collectors.
Status ResidentDataset::search_bounds_class(const AABB &bounds, uint8_t cls, ResultCollector &rc) {
    if (!with_points_ && rc.has_points()) return Status::Err(PCQ_ERR_ARG, NO_COLOURS);
    return search_files(&bounds, predicate(PCQ_PRED_BOUNDS_CLASS, cls), rc);
}

// search_last_file_by_time_range_optimized (search.cpp) for every file.  Any collector: a time record's colour is (0,0,0), so
// no colour block is needed.
Status ResidentDataset::search_time(double start, double end, ResultCollector &rc) {
    if (!with_times_) return Status::Err(PCQ_ERR_ARG, NO_TIMES);
    return search_files(nullptr, predicate(PCQ_PRED_TIME, 0, start, end), rc);
}

// The combined time search of search.cpp for every file: the prologue of search_bounds, then box AND time in one scan — through
// the bounds and time parts of the file's chunk index for count and buffer collectors.  Any collector: the records carry class 0
// and colour (0,0,0).
Status ResidentDataset::search_bounds_time(const AABB &bounds, double start, double end, ResultCollector &rc) {
    if (!with_times_) return Status::Err(PCQ_ERR_ARG, NO_TIMES);
    return search_files(&bounds, predicate(PCQ_PRED_BOUNDS_TIME, 0, start, end), rc);
}

Status ResidentDataset::last_stats(pcq_index_stats *out) {
    *out = pcq_index_stats{};
    for (pcq_index *ix : last_indices_) {
        pcq_index_stats st;
        const int r = pcq_index_get_stats(ix, &st);  // (waits for that file's scan)
        if (r) return Status::FromLib(r);
        out->chunks += st.chunks, out->skipped += st.skipped, out->whole += st.whole, out->scanned += st.scanned, out->built += st.built;
    }
    return Status::Ok();
}

}  // namespace pcq
