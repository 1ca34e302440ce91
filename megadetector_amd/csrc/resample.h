// Pillow's LANCZOS resize and the drawing of annotated previews, shared by the GPU kernels (preview_kernels.cpp) and their
// host models (mdjpeg_resample, mdjpeg_draw in jpeg_entropy.cpp): ONE computation of the coefficient tables, ONE weighted
// sum of a run of samples, ONE walk of a pixel through its image's drawing operations, compiled by both, so that the CPU
// suite and the host sanitizers exercise the very statements the lanes run (the arrangement of blur_box.h).
//
// What is computed (Pillow's Resample.c, Image.resize(size, LANCZOS) of an 8-bit RGB image): for each axis whose size
// changes, the horizontal one first, every output sample is a weighted sum of a run of input samples of its line:
//   scale      in / out;  filterscale = max(scale, 1);  support = 3 filterscale
//   run        center = (i + 0.5) scale;  first = max(int(center - support + 0.5), 0);
//              count = min(int(center + support + 0.5), in) - first
//   weights    lanczos3((x + first - center + 0.5) / filterscale) in double, divided by their sum, then to integers:
//              k = (int)(+-0.5 + w 2^22), the sign of w
//   one pass   out = clip8((2^21 + sum k p) >> 22) in 32-bit integers; the image between the two passes has 8 bits
// An axis whose size does not change is not resampled at all.
//
// Drawing (visualization_utils.render_detection_bounding_boxes as megadetector_amd/preview.py plans it): an image has an
// ordered list of operations, each a solid rectangle or the paste of a patch of pixels, both clipped to the image; where
// operations overlap the later one wins.  A pixel therefore takes the value of the LAST operation that covers it, which
// md_draw_pixel finds by walking the list backwards: the result does not depend on the order pixels are visited in.
#ifndef MD_RESAMPLE_H
#define MD_RESAMPLE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDR_HD __host__ __device__
#else
#define MDR_HD
#endif

#define MD_RESAMPLE_PRECISION_BITS 22            // Resample.c PRECISION_BITS: 32 - 8 - 2
#define MD_RESAMPLE_LDS_BYTES 32768              // source runs of a workgroup of the horizontal pass
#define MD_RESAMPLE_STRIP 64                     // output pixels of a strip of the horizontal pass at the most
#define MD_RESAMPLE_MAX_ROWS 8                   // rows a workgroup of the horizontal pass takes at the most

// ---- coefficient tables (host only: double arithmetic, once per distinct (in, out) pair) ---------------------------------

static inline double md_lanczos3(double x) {
    // Resample.c lanczos_filter over sinc_filter: truncated sinc, support 3
    if (!(-3.0 <= x && x < 3.0)) return 0.0;
    if (x == 0.0) return 1.0;
    const double a = x * M_PI, b = x / 3.0 * M_PI;
    return (sin(a) / a) * (x / 3.0 == 0.0 ? 1.0 : sin(b) / b);
}

// taps a line of the table has room for (Resample.c precompute_coeffs: ksize)
static inline int md_resample_ksize(int in_size, int out_size) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(3.0 * filterscale) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc: bounds[2 i] = first tap, bounds[2 i + 1] = count, kk[i ksize ..] the integer
// weights of output index i (zero behind the count); `work` holds ksize doubles
static inline void md_resample_coeffs(int in_size, int out_size, int ksize, int32_t* bounds, int32_t* kk, double* work) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > ksize) xmax = ksize;                                  // (never: ksize bounds the run)
        for (int x = 0; x < xmax; ++x) {
            const double w = md_lanczos3((x + xmin - center + 0.5) * ss);
            work[x] = w;
            ww += w;
        }
        int32_t* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < xmax; ++x) {
            const double w = ww != 0.0 ? work[x] / ww : work[x];
            k[x] = w < 0 ? (int32_t)(-0.5 + w * (1 << MD_RESAMPLE_PRECISION_BITS)) : (int32_t)(0.5 + w * (1 << MD_RESAMPLE_PRECISION_BITS));
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// ---- one output sample --------------------------------------------------------------------------------------------------

MDR_HD static inline uint8_t md_resample_clip8(int32_t ss) {
    ss >>= MD_RESAMPLE_PRECISION_BITS;                                   // (arithmetic: Resample.c clip8 indexes a table with it)
    return (uint8_t)(ss < 0 ? 0 : ss > 255 ? 255 : ss);
}

// the weighted sum of n samples `step` bytes apart.  32-bit wrap-around cannot happen: sum |k| < 2^23 for this filter
MDR_HD static inline uint8_t md_resample_dot(const uint8_t* p, long long step, const int32_t* k, int n) {
    int32_t ss = 1 << (MD_RESAMPLE_PRECISION_BITS - 1);
    for (int i = 0; i < n; ++i) ss += (int32_t)p[(long long)i * step] * k[i];
    return md_resample_clip8(ss);
}

// The horizontal pass in strips: a workgroup produces `strip` output pixels of `rows` rows from the source runs it holds
// on chip.  The run of a strip of output pixels [o0, o1) is [first(o0), max(first + count)) source pixels -- first is
// monotonic in the output index, first + count is too.  Returns 0 when even one output pixel's run does not fit.
struct MdResampleStrips {
    int32_t strip;                       // output pixels per strip
    int32_t rows;                        // rows per workgroup
    int32_t run_bytes;                   // bytes a row of the on-chip buffer has: the longest run, +3 for the alignment shift, whole dwords
};

static inline int md_resample_plan_strips(const int32_t* bounds, int out_size, int lds_bytes, MdResampleStrips* plan) {
    for (int strip = MD_RESAMPLE_STRIP; strip >= 1; strip >>= 1) {
        int longest = 0;
        for (int o0 = 0; o0 < out_size; o0 += strip) {
            const int o1 = o0 + strip < out_size ? o0 + strip : out_size;
            const int run = bounds[2 * (o1 - 1)] + bounds[2 * (o1 - 1) + 1] - bounds[2 * o0];
            if (run > longest) longest = run;
        }
        const int run_bytes = (longest * 3 + 3 + 3) / 4 * 4;
        if (run_bytes > lds_bytes) continue;
        int rows = lds_bytes / run_bytes;
        if (rows > MD_RESAMPLE_MAX_ROWS) rows = MD_RESAMPLE_MAX_ROWS;
        plan->strip = strip, plan->rows = rows, plan->run_bytes = run_bytes;
        return 1;
    }
    return 0;
}

// ---- drawing ------------------------------------------------------------------------------------------------------------

#define MD_DRAW_OP_WORDS 8               // int32 words of an operation in the lists of mdhip_draw_ops / mdjpeg_draw
#define MD_DRAW_RECT 0                   // [0, x0, y0, x1, y1, colour, 0, 0]: x0 .. x1 and y0 .. y1 INCLUSIVE, colour = R | G << 8 | B << 16
#define MD_DRAW_PATCH 1                  // [1, x, y, w, h, offset, 0, 0]: w x h pixels (R G B, 3 w bytes a row) at byte `offset` of the
                                         // patch buffer, their top left corner at (x, y) of the image
// Either kind may lie partly or wholly outside the image (negative coordinates included): what lies outside is not drawn.
// A rectangle with x1 < x0 or y1 < y0, or a patch with w or h of 0, draws nothing.

// 0 = the operation is well formed (and a patch lies inside the patch buffer)
MDR_HD static inline int md_draw_op_bad(const int32_t* op, long long patch_bytes) {
    if (op[0] == MD_DRAW_RECT) return 0;
    if (op[0] != MD_DRAW_PATCH) return 1;
    if (op[3] < 0 || op[4] < 0 || op[5] < 0) return 1;
    if (op[3] > 32767 || op[4] > 32767) return 1;                        // (no overflow below, and in x + w)
    return (long long)op[5] + (long long)op[3] * op[4] * 3 > patch_bytes;
}

// the value operations ops[0 .. n) give pixel (x, y): 1 and rgb[0 .. 2] when one of them covers it, else 0
MDR_HD static inline int md_draw_pixel(const int32_t* ops, int n, const uint8_t* patches, int x, int y, uint8_t* rgb) {
    for (int i = n - 1; i >= 0; --i) {
        const int32_t* op = ops + (long long)i * MD_DRAW_OP_WORDS;
        if (op[0] == MD_DRAW_RECT) {
            if (x < op[1] || x > op[3] || y < op[2] || y > op[4]) continue;
            const uint32_t c = (uint32_t)op[5];
            rgb[0] = (uint8_t)c, rgb[1] = (uint8_t)(c >> 8), rgb[2] = (uint8_t)(c >> 16);
            return 1;
        }
        const long long dx = (long long)x - op[1], dy = (long long)y - op[2];
        if (dx < 0 || dy < 0 || dx >= op[3] || dy >= op[4]) continue;
        const uint8_t* p = patches + op[5] + (dy * op[3] + dx) * 3;
        rgb[0] = p[0], rgb[1] = p[1], rgb[2] = p[2];
        return 1;
    }
    return 0;
}

#endif  // MD_RESAMPLE_H
