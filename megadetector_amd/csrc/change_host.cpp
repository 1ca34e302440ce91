// mdjpeg_change_detect: the host model of mdhip_change_detect (change_kernels.cpp) and the backend='host' leg of
// megadetector_amd/change_detection.py.  One step after the other as csrc/change_detect.h defines them, each written the plain
// way: the dilation runs iteration by iteration (the kernels fuse iterations), the regions come from a flood fill in raster
// order (the kernels merge labels) -- so that the two legs agree only if both are right.
#include <string.h>

#include <vector>

#include "../../include/mdjpeg.h"
#include "change_detect.h"

namespace {

// gray -> region of interest -> blur of one image into `out` (w x h, dense)
void blurred_gray(const uint8_t* rgb, int w, int h, int64_t pitch, const ChgWeights& wt, int y0, int y1, uint8_t* out) {
    const int r = wt.k / 2;
    std::vector<uint8_t> gray((size_t)w * h);
    for (int y = 0; y < h; ++y) {
        const uint8_t* row = rgb + (int64_t)y * pitch;
        const bool kept = y >= y0 && y < y1;
        for (int x = 0; x < w; ++x) gray[(size_t)y * w + x] = kept ? (uint8_t)chg_gray(row[3 * x], row[3 * x + 1], row[3 * x + 2]) : 0;
    }
    std::vector<uint16_t> first((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint32_t s = 0;
            for (int t = 0; t < wt.k; ++t) s += (uint32_t)wt.w[t] * gray[(size_t)y * w + chg_reflect101(x + t - r, w)];
            first[(size_t)y * w + x] = (uint16_t)s;
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint32_t s = 0;
            for (int t = 0; t < wt.k; ++t) s += (uint32_t)wt.w[t] * first[(size_t)chg_reflect101(y + t - r, h) * w + x];
            out[(size_t)y * w + x] = (uint8_t)((s + 32768u) >> 16);
        }
}

// one dilation with the k x k square, anchor k / 2: rows, then columns
void dilate_once(std::vector<uint8_t>& m, int w, int h, int k) {
    const int a = k / 2;
    std::vector<uint8_t> t((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint8_t v = 0;
            for (int d = 0; d < k; ++d) {
                const int xx = x - a + d;
                if (xx >= 0 && xx < w && m[(size_t)y * w + xx] > v) v = m[(size_t)y * w + xx];
            }
            t[(size_t)y * w + x] = v;
        }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint8_t v = 0;
            for (int d = 0; d < k; ++d) {
                const int yy = y - a + d;
                if (yy >= 0 && yy < h && t[(size_t)yy * w + x] > v) v = t[(size_t)yy * w + x];
            }
            m[(size_t)y * w + x] = v;
        }
}

// the 8-connected components of the non-zero pixels in raster order of their first pixel: a flood fill from every pixel that
// no earlier fill has reached.  -> the number of significant ones; the first `cap` of them to regions
int find_regions(const std::vector<uint8_t>& m, int w, int h, int min_area, int cap, int32_t* regions) {
    std::vector<uint8_t> seen((size_t)w * h, 0);
    std::vector<int32_t> stack;
    int found = 0;
    for (int64_t start = 0; start < (int64_t)w * h; ++start) {
        if (!m[(size_t)start] || seen[(size_t)start]) continue;
        int64_t area = 0;
        int xmin = w, ymin = h, xmax = -1, ymax = -1;
        seen[(size_t)start] = 1;
        stack.push_back((int32_t)start);
        while (!stack.empty()) {
            const int32_t i = stack.back();
            stack.pop_back();
            const int x = i % w, y = i / w;
            ++area;
            if (x < xmin) xmin = x;
            if (x > xmax) xmax = x;
            if (y < ymin) ymin = y;
            if (y > ymax) ymax = y;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx, yy = y + dy;
                    if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
                    const size_t j = (size_t)yy * w + xx;
                    if (!m[j] || seen[j]) continue;
                    seen[j] = 1;
                    stack.push_back((int32_t)j);
                }
        }
        if (area > min_area) {
            if (found < cap) {
                int32_t* q = regions + 5 * (size_t)found;
                q[0] = xmin, q[1] = ymin, q[2] = xmax - xmin + 1, q[3] = ymax - ymin + 1, q[4] = (int32_t)area;
            }
            ++found;
        }
    }
    return found;
}

}  // namespace

extern "C" int mdjpeg_change_detect(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                                    int n_images, uint8_t* const* blurred, const uint8_t* blurred_ready, const int32_t* pairs, int n_pairs,
                                    const mdjpeg_change_options* opt, int64_t* counts, uint32_t* hist, int32_t* thresholds,
                                    int32_t* n_regions, int32_t* regions, uint8_t* overflow, uint8_t* const* masks) {
    if (!opt || !chg_options_ok(opt->blur_kernel_size, opt->threshold_type, opt->threshold, opt->dilate_kernel_size, opt->dilate_iterations,
                                opt->min_area, opt->has_ignore, opt->ignore_fraction, opt->region_cap))
        return MDJPEG_EINVAL;
    if (!chg_args_ok(images, widths, heights, pitches, n_images, blurred, blurred_ready, pairs, n_pairs, counts, hist, thresholds, n_regions,
                     regions, overflow, opt->region_cap))
        return MDJPEG_EINVAL;
    ChgWeights wt;
    chg_blur_weights(opt->blur_kernel_size, &wt);
    for (int i = 0; i < n_images; ++i) {
        if (blurred_ready[i]) continue;
        int y0, y1;
        chg_roi_rows(opt->has_ignore, opt->ignore_fraction, heights[i], &y0, &y1);
        blurred_gray(images[i], widths[i], heights[i], pitches[i], wt, y0, y1, blurred[i]);
    }
    const int cap = opt->region_cap;
    for (int p = 0; p < n_pairs; ++p) {
        const int w = widths[pairs[2 * p]], h = heights[pairs[2 * p]];
        const uint8_t *a = blurred[pairs[2 * p]], *b = blurred[pairs[2 * p + 1]];
        const size_t px = (size_t)w * h;
        std::vector<uint8_t> m(px);
        uint32_t* hp = hist + 256 * (size_t)p;
        memset(hp, 0, 256 * sizeof(uint32_t));
        for (size_t i = 0; i < px; ++i) m[i] = (uint8_t)(a[i] > b[i] ? a[i] - b[i] : b[i] - a[i]);
        int thr = opt->threshold;
        if (opt->threshold_type == 1) {
            for (size_t i = 0; i < px; ++i) ++hp[m[i]];
            thr = chg_otsu(hp);
        }
        thresholds[p] = thr;
        int y0, y1;
        chg_roi_rows(opt->has_ignore, opt->ignore_fraction, h, &y0, &y1);
        int64_t count = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                m[i] = (m[i] > thr && y >= y0 && y < y1) ? 255 : 0;
                count += m[i] != 0;
            }
        counts[p] = count;
        for (int it = 0; it < opt->dilate_iterations; ++it) dilate_once(m, w, h, opt->dilate_kernel_size);
        if (masks && masks[p]) memcpy(masks[p], m.data(), px);
        if (cap) memset(regions + 5 * (size_t)cap * p, 0, 5 * (size_t)cap * sizeof(int32_t));
        n_regions[p] = find_regions(m, w, h, opt->min_area, cap, cap ? regions + 5 * (size_t)cap * p : nullptr);
        overflow[p] = n_regions[p] > cap ? 1 : 0;
    }
    return MDJPEG_OK;
}

#ifdef MDCHG_ASAN_MAIN
// `make asan-change`: hand-written cases under AddressSanitizer + UBSan, as a program of its own
#include <stdio.h>

static int run(const char* name, int w, int h, const std::vector<uint8_t>& prev, const std::vector<uint8_t>& curr, mdjpeg_change_options opt,
               int64_t want_count, int want_regions, int want_overflow, const std::vector<int32_t>& want_first) {
    std::vector<uint8_t> rgb[2] = {std::vector<uint8_t>((size_t)w * h * 3), std::vector<uint8_t>((size_t)w * h * 3)};
    for (size_t i = 0; i < (size_t)w * h; ++i)
        for (int c = 0; c < 3; ++c) rgb[0][3 * i + c] = prev[i], rgb[1][3 * i + c] = curr[i];
    std::vector<uint8_t> planes[2] = {std::vector<uint8_t>((size_t)w * h), std::vector<uint8_t>((size_t)w * h)}, mask((size_t)w * h);
    const uint8_t* images[2] = {rgb[0].data(), rgb[1].data()};
    uint8_t* blurred[2] = {planes[0].data(), planes[1].data()};
    uint8_t* masks[1] = {mask.data()};
    const int32_t widths[2] = {w, w}, heights[2] = {h, h}, pairs[2] = {0, 1};
    const int64_t pitches[2] = {3LL * w, 3LL * w};
    const uint8_t ready[2] = {0, 0};
    int64_t count = -1;
    uint32_t hist[256];
    int32_t thr = -1, n_regions = -1;
    std::vector<int32_t> regions(5 * (size_t)opt.region_cap + 1, -7);
    uint8_t overflow = 9;
    int rc = mdjpeg_change_detect(images, widths, heights, pitches, 2, blurred, ready, pairs, 1, &opt, &count, hist, &thr, &n_regions,
                                  regions.data(), &overflow, masks);
    bool ok = rc == MDJPEG_OK && count == want_count && n_regions == want_regions && overflow == want_overflow &&
              regions[5 * (size_t)opt.region_cap] == -7;
    for (size_t i = 0; ok && i < want_first.size(); ++i) ok = regions[i] == want_first[i];
    // once more with both planes carried: the images are not read
    const uint8_t ready2[2] = {1, 1};
    const uint8_t* none[2] = {nullptr, nullptr};
    int64_t count2 = -1;
    rc = mdjpeg_change_detect(none, widths, heights, pitches, 2, blurred, ready2, pairs, 1, &opt, &count2, hist, &thr, &n_regions,
                              regions.data(), &overflow, nullptr);
    ok = ok && rc == MDJPEG_OK && count2 == want_count;
    printf("%s: %s (count %lld, regions %d, overflow %d)\n", name, ok ? "ok" : "WRONG", (long long)count, n_regions, (int)overflow);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    mdjpeg_change_options o = {1, 0, 25, 5, 0, 0, 0, 4, 0.0};
    // a 3 x 2 rectangle appears: blur 1 and no dilation leave it as it is
    {
        std::vector<uint8_t> a(8 * 6, 10), b(8 * 6, 10);
        for (int y = 2; y < 4; ++y)
            for (int x = 1; x < 4; ++x) b[y * 8 + x] = 200;
        bad += run("rectangle", 8, 6, a, b, o, 6, 1, 0, {1, 2, 3, 2, 6});
    }
    // an image narrower than the blur radius (the reflection repeats), dilated twice: everything changes
    {
        mdjpeg_change_options q = o;
        q.blur_kernel_size = 21, q.dilate_iterations = 2;
        std::vector<uint8_t> a(3 * 40, 0), b(3 * 40, 255);
        bad += run("narrow", 3, 40, a, b, q, 120, 1, 0, {0, 0, 3, 40, 120});
    }
    // one pixel
    bad += run("1x1", 1, 1, {0}, {255}, o, 1, 1, 0, {0, 0, 1, 1, 1});
    // a dot grid: 12 dots at a cap of 4 (overflow), and exactly at a cap of 12 (none)
    {
        std::vector<uint8_t> a(9 * 7, 0), b(9 * 7, 0);
        for (int y = 0; y < 7; y += 2)
            for (int x = 0; x < 9; x += 4) b[y * 9 + x] = 255;
        bad += run("over the cap", 9, 7, a, b, o, 12, 12, 1, {0, 0, 1, 1, 1, 4, 0, 1, 1, 1});
        mdjpeg_change_options q = o;
        q.region_cap = 12;
        bad += run("at the cap", 9, 7, a, b, q, 12, 12, 0, {0, 0, 1, 1, 1});
        q.region_cap = 0;
        bad += run("cap 0", 9, 7, a, b, q, 12, 12, 1, {});
        q = o;
        q.threshold_type = 1, q.has_ignore = 1, q.ignore_fraction = -0.3;        // Otsu, the top two rows ignored
        bad += run("otsu, roi", 9, 7, a, b, q, 9, 9, 1, {0, 2, 1, 1, 1});
    }
    mdjpeg_change_options q = o;
    q.blur_kernel_size = 4;
    int64_t c;
    bad += mdjpeg_change_detect(nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &q, &c, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr) != MDJPEG_EINVAL;
    return bad ? 1 : 0;
}
#endif
