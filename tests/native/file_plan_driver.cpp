// What the host layer decides about a file before any GPU work, printed one line per case (no GPU call is made).
// Built with -fsanitize=address,undefined by tests/test_file_plans.py, which compares the output with tests/golden/file_plans.txt.
//
//   plans <jobs>       every line of <jobs> is "file tag kind x0 y0 z0 x1 y1 z1 class start end": Searcher::plan_file of the searcher
//                      of that predicate kind (0 bounds, 1 class, 3 time, 4 bounds and class, 5 bounds and time), --optimized
//   dispatch           Searcher::search_file of the five searchers on names that are resolved before a file is opened
//   resident <files>   resident_file_blocks under the four with_points / with_times combinations
//
// The first two modes use only Searcher::plan_file and Searcher::search_file, so that the same source also compiles against a
// tree from before plan_file was written once (with -DFILE_PLAN_DRIVER_NO_RESIDENT): that is how the golden file was recorded.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>

#include "pcq_host.hpp"

using namespace pcq;

static uint64_t bits(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}

static std::unique_ptr<Searcher> searcher_of(int kind, const AABB &box, uint8_t cls, double start, double end) {
    switch (kind) {
    case PCQ_PRED_BOUNDS: return std::make_unique<BoundsSearcher>(box);
    case PCQ_PRED_CLASS: return std::make_unique<ClassSearcher>(cls);
    case PCQ_PRED_TIME: return std::make_unique<TimeSearcher>(start, end);
    case PCQ_PRED_BOUNDS_CLASS: return std::make_unique<BoundsClassSearcher>(box, cls);
    case PCQ_PRED_BOUNDS_TIME: return std::make_unique<BoundsTimeSearcher>(box, start, end);
    }
    return nullptr;
}

static int plans(const char *jobs) {
    std::ifstream in(jobs);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string file, tag;
        int kind = -1, cls = 0;
        double mn[3], mx[3], start = 0, end = 0;
        ls >> file >> tag >> kind >> mn[0] >> mn[1] >> mn[2] >> mx[0] >> mx[1] >> mx[2] >> cls >> start >> end;
        const auto searcher = ls ? searcher_of(kind, AABB::from_min_max_unchecked(mn, mx), (uint8_t)cls, start, end) : nullptr;
        if (!searcher) {
            fprintf(stderr, "bad job: %s\n", line.c_str());
            return 2;
        }
        const std::optional<FilePlan> plan = searcher->plan_file(file, SearchImplementation::Optimized);
        if (!plan) {
            printf("%s %s no plan\n", file.c_str(), tag.c_str());
            continue;
        }
        const pcq_columns &c = plan->cols;
        const pcq_predicate &p = plan->pred;
        printf("%s %s rc=%d gpu=%d rec=%d xyz=%" PRIuPTR "/%" PRIu64 " cls=%" PRIuPTR "/%" PRIu64 " rgb=%" PRIuPTR "/%" PRIu64 " n=%" PRIu64, file.c_str(),
               tag.c_str(), plan->status.code, (int)plan->needs_gpu, plan->las_record_size, (uintptr_t)c.xyz, c.xyz_stride, (uintptr_t)c.cls, c.cls_stride,
               (uintptr_t)c.rgb, c.rgb_stride, c.n);
        printf(" s=%" PRIx64 ",%" PRIx64 ",%" PRIx64 " o=%" PRIx64 ",%" PRIx64 ",%" PRIx64, bits(c.scale[0]), bits(c.scale[1]), bits(c.scale[2]),
               bits(c.offset[0]), bits(c.offset[1]), bits(c.offset[2]));
        printf(" k=%d c=%d lo=%" PRId64 ",%" PRId64 ",%" PRId64 " hi=%" PRId64 ",%" PRId64 ",%" PRId64 " t=%" PRIx64 ",%" PRIx64 " msg=%s\n",
               (int)p.kind, (int)p.cls, p.lmin[0], p.lmin[1], p.lmin[2], p.lmax[0], p.lmax[1], p.lmax[2], bits(p.wmin[0]), bits(p.wmax[0]),
               plan->status.message.c_str());
    }
    return 0;
}

// a collector that is nothing: no call of the dispatch mode reaches it
struct NoCollector : ResultCollector {};

static int dispatch() {
    const double mn[3] = {0, 0, 0}, mx[3] = {1, 1, 1};
    const AABB box = AABB::from_min_max_unchecked(mn, mx);
    const char *const names[5] = {"bounds", "class", "time", "bounds+class", "bounds+time"};
    const int kinds[5] = {PCQ_PRED_BOUNDS, PCQ_PRED_CLASS, PCQ_PRED_TIME, PCQ_PRED_BOUNDS_CLASS, PCQ_PRED_BOUNDS_TIME};
    struct Case {
        const char *path;
        SearchImplementation impl;
        bool attribute_searchers_only;  // (the bounds and class searchers open a .lazer file)
    };
    const Case cases[] = {{"dir.d/noext", SearchImplementation::Optimized, false}, {"x.laz", SearchImplementation::Optimized, false},
                          {"x.xyz", SearchImplementation::Optimized, false},       {"x.las", SearchImplementation::Regular, false},
                          {"x.last", SearchImplementation::Regular, false},        {"x.lazer", SearchImplementation::Optimized, true}};
    NoCollector collector;
    for (const Case &c : cases)
        for (int k = 0; k < 5; k++) {
            if (c.attribute_searchers_only && k < 2) continue;
            const Status st = searcher_of(kinds[k], box, 2, 0.0, 1.0)->search_file(c.path, c.impl, collector);
            printf("%s %s %s rc=%d msg=%s\n", c.path, c.impl == SearchImplementation::Regular ? "regular" : "optimized", names[k], st.code, st.message.c_str());
        }
    return 0;
}

#ifndef FILE_PLAN_DRIVER_NO_RESIDENT
static int resident(int nfiles, char **files) {
    for (int i = 0; i < nfiles; i++)
        for (int combo = 0; combo < 4; combo++) {
            const bool with_points = combo & 1, with_times = combo & 2;
            MappedFile file;
            ResidentBlocks b;
            const Status st = resident_file_blocks(files[i], with_points, with_times, &file, &b);
            printf("%s points=%d times=%d rc=%d format=%d n=%" PRIu64 " xyz=%" PRIu64 " cls=%" PRIu64 " rgb=%" PRIu64 " time=%" PRIu64 " msg=%s\n", files[i],
                   (int)with_points, (int)with_times, st.code, (int)b.header.point_data_record_format, b.header.number_of_points, b.xyz, b.cls, b.rgb, b.time,
                   st.message.c_str());
        }
    return 0;
}
#endif

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "plans")) return plans(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "dispatch")) return dispatch();
#ifndef FILE_PLAN_DRIVER_NO_RESIDENT
    if (argc >= 2 && !strcmp(argv[1], "resident")) return resident(argc - 2, argv + 2);
#endif
    fprintf(stderr, "usage: %s plans <jobs> | dispatch | resident <files...>\n", argv[0]);
    return 2;
}
