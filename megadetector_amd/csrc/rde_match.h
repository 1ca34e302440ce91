// Repeat-detection elimination: the arithmetic the device kernels (rde_kernels.cpp) and the host model (rde_host.cpp,
// mdjpeg_repeat_detections) share, so that both decide every pair of boxes with the same statements.
//
// The reference (postprocessing/repeat_detection_elimination/repeat_detections_core.py _find_matches_in_directory) asks
//     candidate.category == category (unless categoryAgnosticComparisons)  and  ct_utils.get_iou(bbox, candidate.bbox) >= iouThreshold
// in Python floats, i.e. IEEE doubles, one operation at a time.  get_iou is restated below operation for operation: no fused
// multiply-add (inter = p * q followed by (a1 + a2) - inter is exactly the shape a compiler contracts), no reciprocal, no
// inter >= t * union.  Both translation units are built with -ffp-contract=off; the pragmas below say the same to a compiler
// that honours them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RDE_HD __host__ __device__
#else
#define RDE_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

// a box as get_iou sees it after convert_xywh_to_xyxy, with what does not depend on the other box computed once
struct rde_pbox {
    double x1, y1, x2, y2;   // x, y, x + w, y + h
    double area;             // (x2 - x1) * (y2 - y1)
    int32_t group;           // location: boxes of different locations never match
    int32_t category;
    int32_t ok;              // 0: get_iou raises for this box ("Malformed bounding box"), the caller treats that as no match
    int32_t pad;
};

RDE_HD inline rde_pbox rde_prepare(double x, double y, double w, double h, int32_t group, int32_t category) {
    rde_pbox b;
    b.x1 = x;
    b.y1 = y;
    b.x2 = x + w;
    b.y2 = y + h;
    b.area = (b.x2 - b.x1) * (b.y2 - b.y1);
    b.group = group;
    b.category = category;
    b.ok = (b.x1 < b.x2) && (b.y1 < b.y2);      // the reference's asserts; a NaN fails them too
    b.pad = 0;
    return b;
}

// largest chunk (boxes resolved per step) either entry point takes: the device keeps chunk^2 / 8 bytes of match bits
#define RDE_MAX_CHUNK 16384
// largest n: rows are 32-bit on the device
#define RDE_MAX_BOXES (int64_t(1) << 30)

// the argument checks both entry points make; the text of what is wrong, or nullptr
template <class Box>
inline const char* rde_check_args(const Box* boxes, int64_t n, double iou_threshold, int32_t chunk, const uint8_t* is_candidate,
                                  const int32_t* n_instances, const int64_t* pairs, int64_t capacity, const int64_t* needed) {
    if (n < 0) return "n < 0";
    if (n > RDE_MAX_BOXES) return "more than 2^30 boxes";
    if (iou_threshold != iou_threshold) return "the IoU threshold is a NaN";
    if (chunk < 0 || chunk > RDE_MAX_CHUNK) return "chunk outside 0 .. 16384";
    if (capacity < 0 || (capacity > 0 && !pairs)) return "capacity < 0, or pairs is NULL with capacity > 0";
    if (!needed) return "needed is NULL";
    if (n > 0 && (!boxes || !is_candidate || !n_instances)) return "boxes, is_candidate or n_instances is NULL";
    for (int64_t i = 1; i < n; ++i)
        if (boxes[i].group < boxes[i - 1].group) return "group decreases along the boxes";
    return nullptr;
}

// Python's max(a, b) / min(a, b): the first argument unless the second is larger / smaller
RDE_HD inline double rde_pymax(double a, double b) { return b > a ? b : a; }
RDE_HD inline double rde_pymin(double a, double b) { return b < a ? b : a; }

// does detection `d` match candidate `c`?  (bb1 = the detection, bb2 = the candidate, as the reference passes them)
RDE_HD inline bool rde_match(const rde_pbox& d, const rde_pbox& c, double iou_threshold, int category_agnostic) {
    if (d.group != c.group) return false;
    if (d.category != c.category && !category_agnostic) return false;
    if (!d.ok || !c.ok) return false;
    const double x_left = rde_pymax(d.x1, c.x1);
    const double y_top = rde_pymax(d.y1, c.y1);
    const double x_right = rde_pymin(d.x2, c.x2);
    const double y_bottom = rde_pymin(d.y2, c.y2);
    if (x_right < x_left || y_bottom < y_top) return 0.0 >= iou_threshold;
    const double inter = (x_right - x_left) * (y_bottom - y_top);
    const double sum = d.area + c.area;
    const double uni = sum - inter;
    const double iou = inter / uni;
    // get_iou asserts 0 <= iou <= 1 and Python raises on a division by zero; the caller catches either as "no match".
    // Here 0 / 0 is a NaN and x / 0 an infinity, which fail these comparisons as well.
    if (!(iou >= 0.0) || !(iou <= 1.0)) return false;
    return iou >= iou_threshold;
}
