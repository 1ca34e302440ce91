// Change detection between two images: the arithmetic the device kernels (change_kernels.cpp) and the host model
// (change_host.cpp, mdjpeg_change_detect) share, so that both compute every pixel with the same statements.  All of it is
// integer arithmetic; the one floating-point step, Otsu's threshold, runs on the host in both legs (chg_otsu below).
//
// What the reference (detection/change_detection.py detect_motion, FRAME_DIFF) asks of OpenCV, and what stands here for it:
//
//   gray     cv2.cvtColor(BGR2GRAY): (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15.  The constants are OpenCV 4's 8-bit ones
//            as remembered (they sum to 32768); NOT VERIFIED AGAINST OPENCV, which is not available to this project.
//   region   ignore_rows = int(abs(f) * h); the top rows (f < 0) or the bottom rows (f > 0) are zeroed in the gray image before
//   of       the blur and in the thresholded mask after it, and leave the denominator of diff_percentage.  |f| <= 1.
//   interest
//   blur     cv2.GaussianBlur(gray, (k, k), 0), k odd: separable, 8.8 fixed-point weights that sum to exactly 256.
//            k = 1, 3, 5, 7: OpenCV's fixed tables [1], [1 2 1] / 4, [1 4 6 4 1] / 16, [1 3.5 7 9 7 3.5 1] / 32 (x 256: exact).
//            Larger k: g(i) = exp(-(i - c)^2 / (2 sigma^2)), c = (k - 1) / 2, sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8, in doubles;
//            THE RULE: every tap but the centre is floor(256 * g(i) / sum(g) + 0.5), the centre tap is 256 minus the sum of the
//            others.  OpenCV's own routine spreads the rounding error differently; it could not be read, so THESE COEFFICIENTS
//            ARE THE PROJECT'S, not OpenCV's.  First pass (along x): 16-bit sums of weight x pixel, no rounding (at most
//            255 * 256).  Second pass (along y): 32-bit sums of weight x first-pass value, then (v + 32768) >> 16.
//            Border: BORDER_REFLECT_101 (dcb|abcd|cba), the reflection repeated until the index is inside -- chg_reflect101
//            is the closed form of that repetition; an axis of length 1 gives index 0.
//   diff     |a - b|; 255 where > threshold, else 0.  OTSU: the threshold comes from chg_otsu over the 256-bin histogram of
//            the difference (all pixels, as cv2.threshold sees them).
//   dilate   per iteration the maximum over the k x k square with anchor k / 2: columns x - k / 2 .. x - k / 2 + k - 1, rows
//            likewise; pixels outside the image contribute nothing.  Because nothing comes in from outside, n iterations equal
//            ONE maximum over columns x - n * (k / 2) .. x + n * (k - 1 - k / 2): both legs may fuse iterations.
//   regions  the 8-connected components of the dilated mask.  A component's label is the smallest raster index (y * w + x) of
//            its pixels, its area its PIXEL COUNT, it is significant when area > min_area, its rectangle is
//            (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1); regions are listed by ascending label.  Both differ from OpenCV
//            on purpose: cv2.contourArea is a polygon's area (smaller by about half the border length), and the order of
//            cv2.findContours is not known to this project.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CHG_HD __host__ __device__
#else
#define CHG_HD
#endif

#define CHG_MAX_BLUR 127          /* blur_kernel_size: odd, 1 .. 127 */
#define CHG_MAX_DILATE 33         /* dilate_kernel_size: 1 .. 33 */
#define CHG_MAX_ITERATIONS 64     /* dilate_iterations: 0 .. 64 */
#define CHG_MAX_SIDE 32767        /* width and height: 1 .. 32767 */
#define CHG_MAX_PIXELS 0x7fff0000 /* width x height of one image */

struct ChgWeights {
    int32_t k;                    // taps
    uint16_t w[CHG_MAX_BLUR + 1]; // 8.8 fixed point, sum 256
};

// BORDER_REFLECT_101 for any i: period 2 (n - 1); n >= 1
CHG_HD inline int chg_reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

CHG_HD inline int chg_gray(int r, int g, int b) { return (r * 9798 + g * 19235 + b * 3735 + 16384) >> 15; }

// the kept rows [*y0, *y1) of an image of h rows; has_ignore 0: all of them
inline void chg_roi_rows(int has_ignore, double f, int h, int* y0, int* y1) {
    *y0 = 0;
    *y1 = h;
    if (!has_ignore) return;
    const int rows = (int)(fabs(f) * (double)h);
    if (f < 0) *y0 = rows;
    else if (f > 0) *y1 = h - rows;
}

// the weights of blur_kernel_size k (odd, 1 .. CHG_MAX_BLUR) by THE RULE above; returns 0 for another k
inline int chg_blur_weights(int k, ChgWeights* out) {
    if (k < 1 || k > CHG_MAX_BLUR || !(k & 1)) return 0;
    for (int i = 0; i <= CHG_MAX_BLUR; ++i) out->w[i] = 0;
    out->k = k;
    static const uint16_t t1[1] = {256}, t3[3] = {64, 128, 64}, t5[5] = {16, 64, 96, 64, 16}, t7[7] = {8, 28, 56, 72, 56, 28, 8};
    const uint16_t* fixed = k == 1 ? t1 : k == 3 ? t3 : k == 5 ? t5 : k == 7 ? t7 : nullptr;
    if (fixed) {
        for (int i = 0; i < k; ++i) out->w[i] = fixed[i];
        return 1;
    }
    const double sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8;
    const int c = (k - 1) / 2;
    double g[CHG_MAX_BLUR], sum = 0.0;
    for (int i = 0; i < k; ++i) {
        const double d = (double)(i - c);
        g[i] = exp(-(d * d) / (2.0 * sigma * sigma));
        sum += g[i];
    }
    int others = 0;
    for (int i = 0; i < k; ++i) {
        if (i == c) continue;
        out->w[i] = (uint16_t)floor(256.0 * g[i] / sum + 0.5);
        others += out->w[i];
    }
    out->w[c] = (uint16_t)(256 - others);
    return 1;
}

// Otsu's threshold of a 256-bin histogram, the published loop in the form of OpenCV's getThreshVal_Otsu_8u (doubles; the
// first maximum of the between-class variance wins).  An empty histogram gives 0.
inline int chg_otsu(const uint32_t hist[256]) {
    double total = 0.0;
    for (int i = 0; i < 256; ++i) total += (double)hist[i];
    if (total <= 0.0) return 0;
    const double scale = 1.0 / total;
    double mu = 0.0;
    for (int i = 0; i < 256; ++i) mu += (double)i * (double)hist[i];
    mu *= scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int max_val = 0;
    const double eps = 1.1920928955078125e-07;   // FLT_EPSILON
    for (int i = 0; i < 256; ++i) {
        const double p_i = (double)hist[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        if ((q1 < q2 ? q1 : q2) < eps || (q1 > q2 ? q1 : q2) > 1.0 - eps) continue;
        mu1 = (mu1 + (double)i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) {
            max_sigma = sigma;
            max_val = i;
        }
    }
    return max_val;
}

// the fused dilation window of n iterations with a k x k square: columns x - *lo .. x + *hi (rows likewise)
CHG_HD inline void chg_dilate_reach(int k, int n, int* lo, int* hi) {
    *lo = n * (k / 2);
    *hi = n * (k - 1 - k / 2);
}

// what both entry points refuse (mdjpeg_change_options of include/mdjpeg.h, passed field by field to stay free of that header)
inline int chg_options_ok(int blur_k, int threshold_type, int threshold, int dilate_k, int dilate_iterations, int min_area, int has_ignore,
                          double ignore_fraction, int region_cap) {
    if (blur_k < 1 || blur_k > CHG_MAX_BLUR || !(blur_k & 1)) return 0;
    if (threshold_type != 0 && threshold_type != 1) return 0;
    if (threshold < 0 || threshold > 255) return 0;
    if (dilate_k < 1 || dilate_k > CHG_MAX_DILATE || dilate_iterations < 0 || dilate_iterations > CHG_MAX_ITERATIONS) return 0;
    if (min_area < 0 || region_cap < 0 || region_cap > 65536) return 0;
    if (has_ignore && !(ignore_fraction >= -1.0 && ignore_fraction <= 1.0)) return 0;
    return 1;
}

// the argument checks both entry points share (the pointers are never dereferenced beyond the host arrays); 1 = fine
inline int chg_args_ok(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches, int n_images,
                       uint8_t* const* blurred, const uint8_t* blurred_ready, const int32_t* pairs, int n_pairs, const void* counts,
                       const void* hist, const void* thresholds, const void* n_regions, const void* regions, const void* overflow,
                       int region_cap) {
    if (!images || !widths || !heights || !pitches || !blurred || !blurred_ready || n_images < 1 || n_pairs < 0) return 0;
    if (n_pairs && (!pairs || !counts || !hist || !thresholds || !n_regions || !overflow || (region_cap && !regions))) return 0;
    for (int i = 0; i < n_images; ++i) {
        if (widths[i] < 1 || heights[i] < 1 || widths[i] > CHG_MAX_SIDE || heights[i] > CHG_MAX_SIDE) return 0;
        if ((long long)widths[i] * heights[i] > CHG_MAX_PIXELS) return 0;
        if (!blurred[i]) return 0;
        if (!blurred_ready[i] && (!images[i] || pitches[i] < (long long)widths[i] * 3 ||
                                  (long long)(heights[i] - 1) * pitches[i] + (long long)widths[i] * 3 > 0x7fff0000LL)) return 0;
    }
    for (int p = 0; p < n_pairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || b < 0 || a >= n_images || b >= n_images || widths[a] != widths[b] || heights[a] != heights[b]) return 0;
    }
    return 1;
}
