// zsum_plan.h — the files of one z lattice cut into the launches of the mean-height raster (ResidentDataset::bounds_zmean_raster): a
// launch adds i32 heights into i64 words, which cannot wrap while it reads fewer than 2^32 points (pcq.h:
// pcq_scan_dev_zsum_raster_batch), so the files go, in their order, into batches whose point total stays BELOW a limit.  Pure host
// arithmetic without a HIP include and without the dataset type: tests/native/zsum_plan_driver.cpp compiles it with g++ alone and
// passes small limits.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace zsum_plan {

constexpr uint64_t POINTS_LIMIT = 1ull << 32;  // the product's limit: a batch holds fewer points than this

struct Batch {
    size_t begin, end;  // files [begin, end) of the list
    uint64_t points;    // their total: below the limit
};

// Greedy in list order: a file joins the open batch while the total stays below `limit`, else it opens the next one.  Every file
// lands in exactly one batch, batches are consecutive and none is empty (a file of no points joins like any other).  A file that
// alone holds `limit` points or more fits no batch: false, *refused its position, `out` left as it was.  (The running total is
// compared without being formed, so that no sum can overflow.)
inline bool cut(const std::vector<uint64_t> &points, uint64_t limit, std::vector<Batch> *out, size_t *refused) {
    std::vector<Batch> batches;
    for (size_t i = 0; i < points.size(); i++) {
        if (points[i] >= limit) {
            if (refused) *refused = i;
            return false;
        }
        if (batches.empty() || points[i] >= limit - batches.back().points) batches.push_back({i, i, 0});
        batches.back().end = i + 1;
        batches.back().points += points[i];
    }
    *out = std::move(batches);
    return true;
}

}  // namespace zsum_plan
