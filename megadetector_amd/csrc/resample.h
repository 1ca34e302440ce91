// Pillow's resize (LANCZOS for the annotated previews; bicubic, bilinear and LANCZOS for the classifier input and the
// thumbnails of the RDE review folder, at the end of this file), and the drawing of the previews, shared by the GPU kernels
// (preview_kernels.cpp, classify_kernels.cpp) and their host models (mdjpeg_resample, mdjpeg_draw, mdjpeg_classifier_input,
// mdjpeg_thumbnails in image_host.cpp): ONE computation of the coefficient tables, ONE weighted
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

#include <algorithm>
#include <vector>

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

// Pillow's other filters (Resample.c bicubic_filter with a = -0.5, bilinear_filter), for the classifier input
#define MD_FILTER_BICUBIC 0
#define MD_FILTER_BILINEAR 1
#define MD_FILTER_LANCZOS 2

static inline double md_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static inline double md_bilinear(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

static inline double md_filter_support(int filter) { return filter == MD_FILTER_BICUBIC ? 2.0 : filter == MD_FILTER_BILINEAR ? 1.0 : 3.0; }

static inline double md_filter_value(int filter, double x) {
    return filter == MD_FILTER_BICUBIC ? md_bicubic(x) : filter == MD_FILTER_BILINEAR ? md_bilinear(x) : md_lanczos3(x);
}

// taps a line of the table has room for (Resample.c precompute_coeffs: ksize)
static inline int md_resample_ksize_filter(int filter, int in_size, int out_size) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(md_filter_support(filter) * filterscale) * 2 + 1;
}

static inline int md_resample_ksize(int in_size, int out_size) { return md_resample_ksize_filter(MD_FILTER_LANCZOS, in_size, out_size); }

// precompute_coeffs + normalize_coeffs_8bpc for the output indices o0 .. o1 - 1 of an axis resampled in_size -> out_size
// with `filter`: bounds[2 i] = first tap, bounds[2 i + 1] = count, kk[i ksize ..] the integer weights of output index
// o0 + i (zero behind the count); `work` holds ksize doubles
static inline void md_resample_coeffs_filter(int filter, int in_size, int out_size, int o0, int o1, int ksize, int32_t* bounds,
                                             int32_t* kk, double* work) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = md_filter_support(filter) * filterscale;
    const double ss = 1.0 / filterscale;
    for (int xx = o0; xx < o1; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > ksize) xmax = ksize;                                  // (never: ksize bounds the run)
        for (int x = 0; x < xmax; ++x) {
            const double w = md_filter_value(filter, (x + xmin - center + 0.5) * ss);
            work[x] = w;
            ww += w;
        }
        int32_t* k = kk + (size_t)(xx - o0) * ksize;
        for (int x = 0; x < xmax; ++x) {
            const double w = ww != 0.0 ? work[x] / ww : work[x];
            k[x] = w < 0 ? (int32_t)(-0.5 + w * (1 << MD_RESAMPLE_PRECISION_BITS)) : (int32_t)(0.5 + w * (1 << MD_RESAMPLE_PRECISION_BITS));
        }
        for (int x = xmax; x < ksize; ++x) k[x] = 0;
        bounds[2 * (xx - o0)] = xmin;
        bounds[2 * (xx - o0) + 1] = xmax;
    }
}

// the whole table of the LANCZOS filter (the previews): output indices 0 .. out_size - 1
static inline void md_resample_coeffs(int in_size, int out_size, int ksize, int32_t* bounds, int32_t* kk, double* work) {
    md_resample_coeffs_filter(MD_FILTER_LANCZOS, in_size, out_size, 0, out_size, ksize, bounds, kk, work);
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

// The fan-out draw (mdhip_draw_ops_from / mdjpeg_draw_from): destinations are made from sources that stay as they are, so
// no destination may share a byte with a source or with another destination.  start[i] .. end[i] (exclusive) are the bytes
// of window i from its first pixel to the end of its last row, is_dst[i] whether it is written.  order: scratch of n ints.
// 1 when a destination overlaps any other window; sources may overlap each other.
static inline int md_draw_from_overlap(const uintptr_t* start, const uintptr_t* end, const uint8_t* is_dst, int n, int* order) {
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order, order + n, [start](int a, int b) { return start[a] < start[b]; });
    uintptr_t end_any = 0, end_dst = 0;                                   // the furthest end of the windows / destinations so far
    for (int k = 0; k < n; ++k) {
        const int i = order[k];
        if (start[i] < (is_dst[i] ? end_any : end_dst)) return 1;
        if (end[i] > end_any) end_any = end[i];
        if (is_dst[i] && end[i] > end_dst) end_dst = end[i];
    }
    return 0;
}

// ---- classifier input ---------------------------------------------------------------------------------------------------
//
// What the reference feeds a classifier for one detection (classification/crop_detections.py save_crop, then
// run_classifier.py: Resize(S, BICUBIC), CenterCrop(S), ToTensor, Normalize [3P: torchvision]): the crop is a CANVAS of
// canvas_w x canvas_h pixels of which the rectangle src_w x src_h at (off_x, off_y) holds image pixels and the rest is 0;
// the canvas is resized so that its shorter side is S (the longer int(S long / short)), the S x S centre is kept, and every
// byte v of channel c becomes (v / 255 - mean[c]) / std[c] in fp32, planar.  Only the S x S window is computed and the
// canvas is never built: a tap outside the rectangle contributes 0, but bounds and weights are those of the canvas.
//
// A workgroup takes `strip` output columns and `rows` output rows of a crop: the horizontal pass of the canvas rows its
// vertical taps cover goes into an 8-bit tile on chip (md_classify_hsample), the vertical pass reads the tile
// (md_classify_vsample).  Both are compiled by classify_kernels.cpp and by the host model mdjpeg_classifier_input.
//
// The same record and the same two functions make a THUMBNAIL (mdhip_thumbnails, mdjpeg_thumbnails; the tiles of the RDE
// review folder: Image.crop(box).resize((out_w, out_h)) pasted into a sheet): there the window is the whole resized canvas,
// out_w x out_h of any shape, and the bytes are stored interleaved at `dst` instead of going through the float table.

#define MD_CLASSIFY_LDS_BYTES 32768              // the 8-bit tile of a workgroup
#define MD_CLASSIFY_STRIP 64                     // output columns of a workgroup at the most
#define MD_CLASSIFY_MAX_ROWS 32                  // output rows of a workgroup at the most
#define MD_CLASSIFY_MAX_SIZE 4096                // S at the most

struct MdClassifyCrop {
    const uint8_t* src;                  // the first image pixel that lies in the canvas
    long long pitch;                     // bytes a row of the image
    int32_t src_w, src_h, off_x, off_y;  // the part of the canvas that holds image pixels
    int32_t out_w, out_h;                // the window: S x S for a classifier, the whole resized canvas for a thumbnail
    int32_t hb_off, hk_off, hks;         // horizontal table of output columns 0 .. out_w - 1 (int32 words into the table: bounds,
                                         // weights; taps a line); hks 0 = the width stays: column x is canvas column hb_off + x
    int32_t vb_off, vk_off, vks;         // vertical table of output rows 0 .. out_h - 1, likewise (vks 0: row y is canvas row vb_off + y)
    int32_t strip, rows;                 // output columns and rows of a workgroup
    int32_t strips, row_tiles;           // the crop runs strips * row_tiles workgroups
    uint8_t* dst;                        // a thumbnail: where pixel (0, 0) of the window goes, R G B interleaved (a classifier: unused)
    long long dst_pitch;                 // bytes a row of the sheet it lies in
};

// the resized size of the canvas and where the S x S window lies in it [3P: torchvision Resize(int) and CenterCrop]
static inline void md_classify_geometry(int canvas_w, int canvas_h, int size, int* resized_w, int* resized_h, int* left, int* top) {
    const int lo = canvas_w <= canvas_h ? canvas_w : canvas_h, hi = canvas_w <= canvas_h ? canvas_h : canvas_w;
    const int longer = (int)((double)((long long)size * hi) / (double)lo);
    *resized_w = canvas_w <= canvas_h ? size : longer;
    *resized_h = canvas_w <= canvas_h ? longer : size;
    // int(round((n - S) / 2.0)), Python's round: a half goes to the even neighbour
    const int dx = *resized_w - size, dy = *resized_h - size;
    *left = dx / 2 + ((dx & 1) && ((dx / 2) & 1));
    *top = dy / 2 + ((dy & 1) && ((dy / 2) & 1));
}

// canvas rows the output rows [r0, r1) of the window need: their first, and how many
MDR_HD static inline void md_classify_rows(const MdClassifyCrop& d, const int32_t* table, int r0, int r1, int* first, int* count) {
    if (!d.vks) { *first = d.vb_off + r0, *count = r1 - r0; return; }
    const int32_t* vb = table + d.vb_off;
    *first = vb[2 * r0];
    *count = vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - *first;
}

// the plan of a crop: the widest strip, then the most rows, whose tile fits lds_bytes.  vbounds: the vertical bounds of the
// window's rows, NULL when the height stays; size: the rows of the window.  Returns 0 when the taps of one output row do not
// fit even for one column.
static inline int md_classify_plan(const int32_t* vbounds, int size, int lds_bytes, int32_t* strip_out, int32_t* rows_out) {
    for (int strip = MD_CLASSIFY_STRIP; strip >= 1; strip >>= 1)
        for (int rows = MD_CLASSIFY_MAX_ROWS; rows >= 1; rows >>= 1) {
            long long longest = 0;
            for (int r0 = 0; r0 < size; r0 += rows) {
                const int r1 = r0 + rows < size ? r0 + rows : size;
                const long long n = vbounds ? (long long)vbounds[2 * (r1 - 1)] + vbounds[2 * (r1 - 1) + 1] - vbounds[2 * r0] : r1 - r0;
                if (n > longest) longest = n;
            }
            if (longest * strip * 3 > lds_bytes) continue;
            *strip_out = strip, *rows_out = rows;
            return 1;
        }
    return 0;
}

// byte c of output column x (of the window) in canvas row yy: the horizontal pass, or the canvas byte when the width stays
MDR_HD static inline uint8_t md_classify_hsample(const MdClassifyCrop& d, const int32_t* table, int yy, int x, int c) {
    const int sy = yy - d.off_y;
    if (sy < 0 || sy >= d.src_h) return 0;
    const uint8_t* row = d.src + (long long)sy * d.pitch + c;
    if (!d.hks) {
        const int sx = d.hb_off + x - d.off_x;
        return sx < 0 || sx >= d.src_w ? 0 : row[(long long)sx * 3];
    }
    const int32_t* hb = table + d.hb_off;
    const int32_t* k = table + d.hk_off + (long long)x * d.hks;
    const int first = hb[2 * x] - d.off_x;                               // of the run, in pixels of the rectangle
    const int i0 = first < 0 ? -first : 0;
    const int i1 = hb[2 * x + 1] < d.src_w - first ? hb[2 * x + 1] : d.src_w - first;
    if (i1 <= i0) return md_resample_clip8(1 << (MD_RESAMPLE_PRECISION_BITS - 1));
    return md_resample_dot(row + (long long)(first + i0) * 3, 3, k + i0, i1 - i0);
}

// byte b (3 x + c within the strip) of output row y (of the window) from the tile whose row 0 is canvas row `first`
MDR_HD static inline uint8_t md_classify_vsample(const MdClassifyCrop& d, const int32_t* table, const uint8_t* tile, int tile_pitch,
                                                 int first, int y, int b) {
    if (!d.vks) return tile[(long long)(d.vb_off + y - first) * tile_pitch + b];
    const int32_t* vb = table + d.vb_off;
    return md_resample_dot(tile + (long long)(vb[2 * y] - first) * tile_pitch + b, tile_pitch, table + d.vk_off + (long long)y * d.vks,
                           vb[2 * y + 1]);
}

// the 3 x 256 floats a byte of channel c becomes: ToTensor (v / 255) and Normalize ((x - mean) / std) in fp32, on the host
static inline void md_classify_lut(const float mean[3], const float std[3], float* lut) {
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            volatile float x = (float)v / 255.0f;                        // (volatile: each step rounds to fp32, no contraction)
            volatile float y = x - mean[c];
            lut[c * 256 + v] = y / std[c];
        }
}

// Tables and plan of the window out_w x out_h at (left, top) of a canvas resized to rw x rh, appended to `table` (int32
// words); fills everything of `d` but src / pitch / the rectangle / dst.  Returns 0 when no plan fits lds_bytes.  `work` is
// scratch.
static inline int md_classify_build_window(int filter, int canvas_w, int canvas_h, int rw, int rh, int left, int top, int out_w, int out_h,
                                           int lds_bytes, std::vector<int32_t>& table, std::vector<double>& work, MdClassifyCrop* d) {
    d->out_w = out_w, d->out_h = out_h;
    auto axis = [&](int in, int out, int o0, int n, int32_t* b_off, int32_t* k_off, int32_t* ks) {
        if (in == out) { *b_off = o0, *k_off = 0, *ks = 0; return; }
        const int ksize = md_resample_ksize_filter(filter, in, out);
        *ks = ksize;
        *b_off = (int32_t)table.size();
        *k_off = *b_off + 2 * n;
        table.resize(table.size() + 2 * (size_t)n + (size_t)n * ksize);
        work.resize((size_t)ksize);
        md_resample_coeffs_filter(filter, in, out, o0, o0 + n, ksize, table.data() + *b_off, table.data() + *k_off, work.data());
    };
    axis(canvas_w, rw, left, out_w, &d->hb_off, &d->hk_off, &d->hks);
    axis(canvas_h, rh, top, out_h, &d->vb_off, &d->vk_off, &d->vks);
    if (!md_classify_plan(d->vks ? table.data() + d->vb_off : nullptr, out_h, lds_bytes, &d->strip, &d->rows)) return 0;
    d->strips = (out_w + d->strip - 1) / d->strip;
    d->row_tiles = (out_h + d->rows - 1) / d->rows;
    return 1;
}

// a classifier's crop: the S x S centre of the canvas resized so that its shorter side is S
static inline int md_classify_build(int filter, int canvas_w, int canvas_h, int size, int lds_bytes, std::vector<int32_t>& table,
                                    std::vector<double>& work, MdClassifyCrop* d) {
    int rw, rh, left, top;
    md_classify_geometry(canvas_w, canvas_h, size, &rw, &rh, &left, &top);
    return md_classify_build_window(filter, canvas_w, canvas_h, rw, rh, left, top, size, size, lds_bytes, table, work, d);
}

// a thumbnail: the whole canvas resized to out_w x out_h (Image.crop(box).resize((out_w, out_h), filter))
static inline int md_thumbnail_build(int filter, int canvas_w, int canvas_h, int out_w, int out_h, int lds_bytes,
                                     std::vector<int32_t>& table, std::vector<double>& work, MdClassifyCrop* d) {
    return md_classify_build_window(filter, canvas_w, canvas_h, out_w, out_h, 0, 0, out_w, out_h, lds_bytes, table, work, d);
}

// one tile of a record on the host, as a workgroup runs it: strip k, row tile g.  `store(x, y, c, v)` takes byte v of channel
// c of window pixel (x, y).  Returns 0 when the tile does not fit lds_bytes (a plan that md_classify_plan did not make).
template <class Store>
static inline int md_classify_run_tile(const MdClassifyCrop& d, const int32_t* table, int k, int g, int lds_bytes, std::vector<uint8_t>& tile,
                                       Store store) {
    const int x0 = k * d.strip, nx = d.strip < d.out_w - x0 ? d.strip : d.out_w - x0;
    const int r0 = g * d.rows, nr = d.rows < d.out_h - r0 ? d.rows : d.out_h - r0;
    const int tile_pitch = nx * 3;
    int first, count;
    md_classify_rows(d, table, r0, r0 + nr, &first, &count);
    if ((long long)count * tile_pitch > lds_bytes) return 0;
    tile.assign((size_t)count * tile_pitch, 0);                          // (exact: the sanitizers see an access outside it)
    for (int i = 0; i < count * tile_pitch; ++i) {
        const int j = i / tile_pitch, b = i - j * tile_pitch;
        tile[(size_t)i] = md_classify_hsample(d, table, first + j, x0 + b / 3, b % 3);
    }
    for (int i = 0; i < nr * tile_pitch; ++i) {
        const int j = i / tile_pitch, b = i - j * tile_pitch;
        store(x0 + b / 3, r0 + j, b % 3, md_classify_vsample(d, table, tile.data(), tile_pitch, first, r0 + j, b));
    }
    return 1;
}

#endif  // MD_RESAMPLE_H
