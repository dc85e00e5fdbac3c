// polygon_plan.h — a world outline in one file's integer lattice (ResidentDataset::count_polygon): the vertices rounded to the
// lattice, their bounding box, or the reason the file cannot be asked.  Pure host arithmetic without a HIP include and without the
// dataset type: tests/native/polygon_plan_driver.cpp compiles it with g++ alone.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace polygon_plan {

enum Refusal {
    PLAN_OK = 0,
    PLAN_SCALE,   // scale[0] or scale[1] is not finite or not above 0
    PLAN_VERTEX,  // a vertex lands outside the i32 range
    PLAN_SPAN,    // the outline spans more than 2^31 - 1 lattice steps on an axis
};
inline const char *refusal_text(Refusal r) {
    switch (r) {
    case PLAN_SCALE: return "polygon: the x or y scale is not finite and above 0 in ";
    case PLAN_VERTEX: return "polygon: a vertex of the outline lies outside the i32 lattice of ";
    case PLAN_SPAN: return "polygon: the outline spans more than 2^31 - 1 lattice steps of ";
    default: return "";
    }
}

struct Outline {
    std::vector<int32_t> xy;  // [nverts][2]: the vertices in the file's lattice
    int64_t lo[2], hi[2];     // their bounding box (inclusive): the predicate's x and y range
};

// The world bounding box of nverts finite vertices: (min x, min y) .. (max x, max y).
inline void world_box(size_t nverts, const double *xy, double lo[2], double hi[2]) {
    for (int a = 0; a < 2; a++) lo[a] = hi[a] = xy[a];
    for (size_t i = 1; i < nverts; i++)
        for (int a = 0; a < 2; a++) {
            const double v = xy[2 * i + a];
            if (v < lo[a]) lo[a] = v;
            if (v > hi[a]) hi[a] = v;
        }
}

// V = nearbyint((w - offset) / scale) per coordinate: two f64 operations in this order under the default rounding (ties to even).
// The box is that of the ROUNDED vertices, not the converted world box.  `out` is written only on PLAN_OK.
inline Refusal to_lattice(size_t nverts, const double *xy, const double scale[2], const double offset[2], Outline *out) {
    for (int a = 0; a < 2; a++)
        if (!(scale[a] > 0.0) || scale[a] - scale[a] != 0.0) return PLAN_SCALE;
    Outline o;
    o.xy.resize(2 * nverts);
    for (size_t i = 0; i < nverts; i++)
        for (int a = 0; a < 2; a++) {
            const double q = (xy[2 * i + a] - offset[a]) / scale[a];
            const double v = std::nearbyint(q);
            if (!(v >= -2147483648.0 && v <= 2147483647.0)) return PLAN_VERTEX;  // (NaN among them)
            const int32_t w = (int32_t)v;
            o.xy[2 * i + a] = w;
            if (i == 0 || w < o.lo[a]) o.lo[a] = w;
            if (i == 0 || w > o.hi[a]) o.hi[a] = w;
        }
    for (int a = 0; a < 2; a++)
        if (o.hi[a] - o.lo[a] > (int64_t)INT32_MAX) return PLAN_SPAN;
    *out = o;
    return PLAN_OK;
}

}  // namespace polygon_plan
