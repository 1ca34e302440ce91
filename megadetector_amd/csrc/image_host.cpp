// libmdjpeg.so: the host models of the pixel kernels, each one image at a time with the statements the lanes run.
//   mdjpeg_blur_regions, _chunked, mdjpeg_blur_weights         device twin blur_kernels.cpp      shared code blur_box.h
//   mdjpeg_resample, mdjpeg_draw                               device twin preview_kernels.cpp   shared code resample.h
//   mdjpeg_classifier_input, _plan, mdjpeg_thumbnails          device twin classify_kernels.cpp  shared code resample.h

#include "../../include/mdjpeg.h"
#include "blur_box.h"
#include "resample.h"

#include <cmath>
#include <cstring>
#include <vector>

extern "C" {

// the rectangles of mdjpeg_blur_regions / mdjpeg_blur_regions_chunked, one after the other; lds_bytes 0: every row in one piece
static int blur_regions(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects, float radius,
                        int lds_bytes) {
    if (!rgb || width < 1 || height < 1 || pitch < int64_t(width) * 3 || n_rects < 0 || (n_rects && !rects)) return MDJPEG_EINVAL;
    if (!(radius >= 0.0f) || radius > MD_BLUR_MAX_RADIUS) return MDJPEG_EINVAL;
    for (int i = 0; i < n_rects; ++i) {
        const int32_t* q = rects + 4 * i;
        if (q[2] <= q[0] || q[3] <= q[1]) continue;
        if (q[0] < 0 || q[1] < 0 || q[2] > width || q[3] > height) return MDJPEG_EINVAL;
    }
    const MdBlurWeights wt = md_blur_weights(radius);
    std::vector<uint8_t> s0, s1, la, lb;
    for (int i = 0; i < n_rects; ++i) {
        const int32_t* q = rects + 4 * i;
        const int w = q[2] - q[0], h = q[3] - q[1];
        if (w <= 0 || h <= 0) continue;                                  // without area: nothing is pasted
        uint8_t* img = rgb + int64_t(q[1]) * pitch + int64_t(q[0]) * 3;
        const int64_t sp = int64_t(w) * 3;
        s0.assign(size_t(sp) * h, 0);
        s1.assign(size_t(sp) * h, 0);
        MdBlurXPlan plan;
        if (lds_bytes > 0) {
            if (!md_blur_plan_x(w, wt.r, lds_bytes, &plan)) return MDJPEG_EINVAL;
        } else {
            plan.rows = 1, plan.stride = md_blur_row_stride(w), plan.chunks = 1, plan.step = w, plan.halo = 0;
        }
        la.assign(size_t(plan.stride), 0);
        lb.assign(size_t(plan.stride), 0);
        // the row stage, as a workgroup runs it: load a chunk with its halo, three passes per channel, keep the middle
        for (int y = 0; y < h; ++y)
            for (int k = 0; k < plan.chunks; ++k) {
                int o0, o1, a, b;
                md_blur_chunk(plan, w, k, &o0, &o1, &a, &b);
                const int n = b - a;
                if (size_t(n) * 3 > la.size()) return MDJPEG_EINVAL;
                memcpy(la.data(), img + int64_t(y) * pitch + int64_t(a) * 3, size_t(n) * 3);
                for (int c = 0; c < 3; ++c) md_blur_line3(la.data() + c, lb.data() + c, 3, n, wt);
                memcpy(s0.data() + int64_t(y) * sp + int64_t(o0) * 3, lb.data() + size_t(o0 - a) * 3, size_t(o1 - o0) * 3);
            }
        // the column stage, as a lane runs it: one byte column through the three passes, the last one into the image
        for (int64_t t = 0; t < sp; ++t) {
            md_blur_line(s0.data() + t, sp, s1.data() + t, sp, h, wt.r, wt.ww, wt.fw);
            md_blur_line(s1.data() + t, sp, s0.data() + t, sp, h, wt.r, wt.ww, wt.fw);
            md_blur_line(s0.data() + t, sp, img + t, pitch, h, wt.r, wt.ww, wt.fw);
        }
    }
    return MDJPEG_OK;
}

int mdjpeg_blur_regions(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects, float radius) {
    return blur_regions(rgb, width, height, pitch, rects, n_rects, radius, 0);
}

int mdjpeg_blur_regions_chunked(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects,
                                float radius, int lds_bytes) {
    if (lds_bytes < 1) return MDJPEG_EINVAL;
    return blur_regions(rgb, width, height, pitch, rects, n_rects, radius, lds_bytes);
}

int mdjpeg_blur_weights(float radius, int32_t* r, uint32_t* ww, uint32_t* fw) {
    if (!(radius >= 0.0f) || radius > MD_BLUR_MAX_RADIUS || !r || !ww || !fw) return MDJPEG_EINVAL;
    const MdBlurWeights wt = md_blur_weights(radius);
    *r = wt.r, *ww = wt.ww, *fw = wt.fw;
    return MDJPEG_OK;
}

// The host model of mdhip_resample_lanczos for one image: the passes as the workgroups run them -- the horizontal one strip
// by strip out of a copy of the strip's source run (placed as the on-chip copy is), the vertical one byte column by byte column.
int mdjpeg_resample(const uint8_t* src, int32_t width, int32_t height, int64_t pitch, uint8_t* dst, int32_t dst_width, int32_t dst_height,
                    int64_t dst_pitch) {
    if (!src || !dst || width < 1 || height < 1 || dst_width < 1 || dst_height < 1 || width > 65535 || height > 65535 ||
        dst_width > 65535 || dst_height > 65535 || pitch < int64_t(width) * 3 || dst_pitch < int64_t(dst_width) * 3)
        return MDJPEG_EINVAL;
    const bool horizontal = dst_width != width, vertical = dst_height != height;
    if (!horizontal && !vertical) {
        for (int y = 0; y < height; ++y) memcpy(dst + int64_t(y) * dst_pitch, src + int64_t(y) * pitch, size_t(width) * 3);
        return MDJPEG_OK;
    }
    std::vector<int32_t> bounds, kk;
    std::vector<double> work;
    std::vector<uint8_t> between;
    const uint8_t* in = src;
    int64_t in_pitch = pitch;
    if (horizontal) {
        const int ksize = md_resample_ksize(width, dst_width);
        bounds.assign(size_t(dst_width) * 2, 0);
        kk.assign(size_t(dst_width) * ksize, 0);
        work.assign(size_t(ksize), 0.0);
        md_resample_coeffs(width, dst_width, ksize, bounds.data(), kk.data(), work.data());
        MdResampleStrips plan;
        if (!md_resample_plan_strips(bounds.data(), dst_width, MD_RESAMPLE_LDS_BYTES, &plan)) return MDJPEG_EUNSUPPORTED;
        uint8_t* out = dst;
        int64_t out_pitch = dst_pitch;
        if (vertical) {
            between.assign(size_t(dst_width) * 3 * height, 0);
            out = between.data(), out_pitch = int64_t(dst_width) * 3;
        }
        std::vector<uint8_t> run(size_t(plan.run_bytes), 0);
        for (int y = 0; y < height; ++y)
            for (int o0 = 0; o0 < dst_width; o0 += plan.strip) {
                const int o1 = o0 + plan.strip < dst_width ? o0 + plan.strip : dst_width;
                const int first = bounds[2 * o0];
                const int nb = (bounds[2 * (o1 - 1)] + bounds[2 * (o1 - 1) + 1] - first) * 3;
                const uint8_t* line = src + int64_t(y) * pitch + int64_t(first) * 3;
                const int sh = int(uintptr_t(line) & 3);
                if (sh + nb > plan.run_bytes) return MDJPEG_EINVAL;
                memcpy(run.data() + sh, line, size_t(nb));
                for (int o = o0; o < o1; ++o)
                    for (int c = 0; c < 3; ++c)
                        out[int64_t(y) * out_pitch + int64_t(o) * 3 + c] =
                            md_resample_dot(run.data() + sh + (bounds[2 * o] - first) * 3 + c, 3, kk.data() + size_t(o) * ksize, bounds[2 * o + 1]);
            }
        in = out, in_pitch = out_pitch;
    }
    if (vertical) {
        const int ksize = md_resample_ksize(height, dst_height);
        bounds.assign(size_t(dst_height) * 2, 0);
        kk.assign(size_t(dst_height) * ksize, 0);
        work.assign(size_t(ksize), 0.0);
        md_resample_coeffs(height, dst_height, ksize, bounds.data(), kk.data(), work.data());
        for (int y = 0; y < dst_height; ++y)
            for (int x = 0; x < dst_width * 3; ++x)
                dst[int64_t(y) * dst_pitch + x] =
                    md_resample_dot(in + int64_t(bounds[2 * y]) * in_pitch + x, in_pitch, kk.data() + size_t(y) * ksize, bounds[2 * y + 1]);
    }
    return MDJPEG_OK;
}

// the host model of mdhip_draw_ops for one image: every pixel takes the value of the last operation that covers it
int mdjpeg_draw(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* ops, int n_ops, const uint8_t* patches,
                int64_t patch_bytes) {
    if (!rgb || width < 1 || height < 1 || pitch < int64_t(width) * 3 || n_ops < 0 || (n_ops && !ops) || patch_bytes < 0) return MDJPEG_EINVAL;
    for (int i = 0; i < n_ops; ++i) {
        const int32_t* op = ops + size_t(i) * MD_DRAW_OP_WORDS;
        if (md_draw_op_bad(op, patch_bytes)) return MDJPEG_EINVAL;
        if (op[0] == MD_DRAW_PATCH && op[3] > 0 && op[4] > 0 && !patches) return MDJPEG_EINVAL;
    }
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            uint8_t v[3];
            if (!md_draw_pixel(ops, n_ops, patches, x, y, v)) continue;
            uint8_t* p = rgb + int64_t(y) * pitch + int64_t(x) * 3;
            p[0] = v[0], p[1] = v[1], p[2] = v[2];
        }
    return MDJPEG_OK;
}

// the host model of mdhip_draw_ops_from: every pixel of a destination takes the value of the last operation of the
// destination's list that covers it, or else its source's pixel; everything is checked before a byte is written
int mdjpeg_draw_from(const uint8_t* const* src, const int32_t* widths, const int32_t* heights, const int64_t* pitches, int n_src,
                     uint8_t* const* dst, const int32_t* dst_src, const int64_t* dst_pitches, int n_dst, const int32_t* op_image,
                     const int32_t* ops, int n_ops, const uint8_t* patches, int64_t patch_bytes) {
    if (n_dst == 0 && n_ops == 0) return MDJPEG_OK;
    if (!src || !widths || !heights || !pitches || !dst || !dst_src || !dst_pitches || n_src < 1 || n_dst < 1 || n_ops < 0 ||
        (n_ops && (!op_image || !ops)) || patch_bytes < 0)
        return MDJPEG_EINVAL;
    std::vector<std::vector<int32_t>> lists;
    lists.resize(size_t(n_dst));
    for (int i = 0; i < n_ops; ++i) {
        const int32_t* op = ops + size_t(i) * MD_DRAW_OP_WORDS;
        if (op_image[i] < 0 || op_image[i] >= n_dst || md_draw_op_bad(op, patch_bytes)) return MDJPEG_EINVAL;
        if (op[0] == MD_DRAW_PATCH && op[3] > 0 && op[4] > 0 && !patches) return MDJPEG_EINVAL;
        lists[size_t(op_image[i])].insert(lists[size_t(op_image[i])].end(), op, op + MD_DRAW_OP_WORDS);
    }
    const size_t n_win = size_t(n_src) + size_t(n_dst);
    std::vector<uintptr_t> start(n_win), end(n_win);
    std::vector<uint8_t> is_dst(n_win);
    std::vector<int> order(n_win);
    for (int i = 0; i < n_src; ++i) {
        if (!src[i] || widths[i] < 1 || heights[i] < 1 || pitches[i] < int64_t(widths[i]) * 3) return MDJPEG_EINVAL;
        start[size_t(i)] = uintptr_t(src[i]);
        end[size_t(i)] = start[size_t(i)] + uintptr_t(pitches[i] * (heights[i] - 1) + int64_t(widths[i]) * 3);
    }
    for (int m = 0; m < n_dst; ++m) {
        const int k = dst_src[m];
        if (k < 0 || k >= n_src || !dst[m] || dst_pitches[m] < int64_t(widths[k]) * 3) return MDJPEG_EINVAL;
        const size_t j = size_t(n_src) + size_t(m);
        start[j] = uintptr_t(dst[m]);
        end[j] = start[j] + uintptr_t(dst_pitches[m] * (heights[k] - 1) + int64_t(widths[k]) * 3);
        is_dst[j] = 1;
    }
    if (md_draw_from_overlap(start.data(), end.data(), is_dst.data(), int(n_win), order.data())) return MDJPEG_EINVAL;
    for (int m = 0; m < n_dst; ++m) {
        const int k = dst_src[m];
        const std::vector<int32_t>& list = lists[size_t(m)];
        const int n = int(list.size() / MD_DRAW_OP_WORDS);
        for (int y = 0; y < heights[k]; ++y) {
            const uint8_t* p = src[k] + int64_t(y) * pitches[k];
            uint8_t* q = dst[m] + int64_t(y) * dst_pitches[m];
            for (int x = 0; x < widths[k]; ++x) {
                uint8_t v[3] = {p[3 * x], p[3 * x + 1], p[3 * x + 2]};
                md_draw_pixel(list.data(), n, patches, x, y, v);
                q[3 * x] = v[0], q[3 * x + 1] = v[1], q[3 * x + 2] = v[2];
            }
        }
    }
    return MDJPEG_OK;
}

// The host model of mdhip_classifier_input for one crop: tile by tile as the workgroups run it -- the horizontal pass of the
// canvas rows a tile's vertical taps cover into an 8-bit tile of exactly that size, then the vertical pass and the lookup.
int mdjpeg_classifier_input(const uint8_t* src, int64_t pitch, int32_t src_w, int32_t src_h, int32_t canvas_w, int32_t canvas_h,
                            int32_t off_x, int32_t off_y, int32_t size, int32_t filter, const float mean[3], const float std[3], float* out) {
    if (!src || !mean || !std || !out || src_w < 1 || src_h < 1 || canvas_w < 1 || canvas_h < 1 || canvas_w > 65535 || canvas_h > 65535 ||
        pitch < int64_t(src_w) * 3 || off_x < 0 || off_y < 0 || off_x > canvas_w - src_w || off_y > canvas_h - src_h || size < 1 ||
        size > MD_CLASSIFY_MAX_SIZE || filter < MD_FILTER_BICUBIC || filter > MD_FILTER_LANCZOS)
        return MDJPEG_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f) return MDJPEG_EINVAL;
    std::vector<int32_t> table;
    std::vector<double> work;
    MdClassifyCrop d;
    memset(&d, 0, sizeof(d));
    if (!md_classify_build(filter, canvas_w, canvas_h, size, MD_CLASSIFY_LDS_BYTES, table, work, &d)) return MDJPEG_EUNSUPPORTED;
    d.src = src, d.pitch = pitch, d.src_w = src_w, d.src_h = src_h, d.off_x = off_x, d.off_y = off_y;
    std::vector<float> lut(3 * 256);
    md_classify_lut(mean, std, lut.data());
    std::vector<uint8_t> tile;
    for (int g = 0; g < d.row_tiles; ++g)
        for (int k = 0; k < d.strips; ++k)
            if (!md_classify_run_tile(d, table.data(), k, g, MD_CLASSIFY_LDS_BYTES, tile, [&](int x, int y, int c, uint8_t v) {
                    out[(size_t(c) * size + y) * size + x] = lut[size_t(c) * 256 + v];
                }))
                return MDJPEG_EINVAL;
    return MDJPEG_OK;
}

// The host model of mdhip_thumbnails: every tile is checked and planned before any is made, then made workgroup by workgroup
// with the statements the lanes run; the bytes go interleaved to their place in the sheet.
int mdjpeg_thumbnails(const mdjpeg_thumbnail* tiles, int n, int32_t filter) {
    if (n == 0) return MDJPEG_OK;
    if (!tiles || n < 0 || n > 65535 || filter < MD_FILTER_BICUBIC || filter > MD_FILTER_LANCZOS) return MDJPEG_EINVAL;
    std::vector<MdClassifyCrop> recs((size_t)n);
    std::vector<std::vector<int32_t>> tables((size_t)n);
    std::vector<double> work;
    for (int i = 0; i < n; ++i) {
        const mdjpeg_thumbnail& q = tiles[i];
        const bool empty = (q.src_w == 0 && q.src_h >= 0) || (q.src_h == 0 && q.src_w >= 0);      // no image pixel in the canvas: src is not read
        if (!q.dst || q.canvas_w < 1 || q.canvas_h < 1 || q.canvas_w > 65535 || q.canvas_h > 65535 ||
            (!empty && (!q.src || q.src_w < 1 || q.src_h < 1 || q.pitch < int64_t(q.src_w) * 3 || q.off_x < 0 || q.off_y < 0 ||
                        q.off_x > q.canvas_w - q.src_w || q.off_y > q.canvas_h - q.src_h)) ||
            q.out_w < 1 || q.out_h < 1 || q.out_w > 65535 || q.out_h > 65535 || q.dst_pitch < int64_t(q.out_w) * 3)
            return MDJPEG_EINVAL;
        MdClassifyCrop& d = recs[size_t(i)];
        memset(&d, 0, sizeof(d));
        if (!md_thumbnail_build(filter, q.canvas_w, q.canvas_h, q.out_w, q.out_h, MD_CLASSIFY_LDS_BYTES, tables[size_t(i)], work, &d))
            return MDJPEG_EUNSUPPORTED;
        if (!empty) d.src = q.src, d.pitch = q.pitch, d.src_w = q.src_w, d.src_h = q.src_h, d.off_x = q.off_x, d.off_y = q.off_y;
        d.dst = q.dst, d.dst_pitch = q.dst_pitch;
    }
    std::vector<uint8_t> tile;
    for (int i = 0; i < n; ++i) {
        const MdClassifyCrop& d = recs[size_t(i)];
        for (int g = 0; g < d.row_tiles; ++g)
            for (int k = 0; k < d.strips; ++k)
                if (!md_classify_run_tile(d, tables[size_t(i)].data(), k, g, MD_CLASSIFY_LDS_BYTES, tile, [&](int x, int y, int c, uint8_t v) {
                        d.dst[int64_t(y) * d.dst_pitch + int64_t(x) * 3 + c] = v;
                    }))
                    return MDJPEG_EINVAL;
    }
    return MDJPEG_OK;
}

// the tile a workgroup takes of a crop of this canvas: plan[0] output columns, plan[1] output rows; MDJPEG_EUNSUPPORTED when
// none fits lds_bytes (0: what the device has)
int mdjpeg_classifier_plan(int32_t canvas_w, int32_t canvas_h, int32_t size, int32_t filter, int32_t lds_bytes, int32_t plan[2]) {
    if (!plan || canvas_w < 1 || canvas_h < 1 || canvas_w > 65535 || canvas_h > 65535 || size < 1 || size > MD_CLASSIFY_MAX_SIZE ||
        filter < MD_FILTER_BICUBIC || filter > MD_FILTER_LANCZOS || lds_bytes < 0)
        return MDJPEG_EINVAL;
    std::vector<int32_t> table;
    std::vector<double> work;
    MdClassifyCrop d;
    memset(&d, 0, sizeof(d));
    if (!md_classify_build(filter, canvas_w, canvas_h, size, lds_bytes ? lds_bytes : MD_CLASSIFY_LDS_BYTES, table, work, &d)) return MDJPEG_EUNSUPPORTED;
    plan[0] = d.strip, plan[1] = d.rows;
    return MDJPEG_OK;
}
}  // extern "C"
