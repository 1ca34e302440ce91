// `make asan-jpeg`: the test program of libmdjpeg.so's sources (jpeg_entropy.cpp, jpeg_encode_host.cpp, image_host.cpp) under
// AddressSanitizer + UBSan.  Not part of the library; it calls only the C ABI of include/mdjpeg.h.  It decodes every file named
// on the command line into a heap buffer of exactly coef_count values, so that the sanitizers see any access outside it.
// Prints one line per file; the exit status is 0 unless a sanitizer fires.

#include "../../include/mdjpeg.h"
#include "resample.h"      // MD_DRAW_OP_WORDS, MD_FILTER_LANCZOS

#include <cstdio>
#include <cstring>
#include <vector>

// `--blur`: mdjpeg_blur_regions and its chunked form on heap images of exactly pitch x height bytes -- the whole image, single
// rows and columns, rectangles on every border and the sizes around the box radius -- so that the sanitizers see any
// access outside an image; the two forms must agree.
static int blur_matrix() {
    const int W = 97, H = 131;
    const int64_t pitch = 393;
    std::vector<int32_t> rects = {0, 0, W, H, 50, 60, 51, 61, 0, 70, W, 71, 33, 0, 34, H, 0, 0, 30, 20, W - 30, 0, W, 25, 0, H - 20, 41, H,
                                  W - 17, H - 33, W, H, 5, 5, 5, 9, 9, 5, 5, 9};
    for (int n : {5, 39, 40, 41, 79, 80, 81}) {
        rects.insert(rects.end(), {1, 3, 1 + n, 50});
        rects.insert(rects.end(), {3, 1, 26, 1 + n});
        rects.insert(rects.end(), {2, 4, 2 + n, 4 + n});
    }
    const int n_rects = int(rects.size() / 4);
    for (float radius : {40.0f, 2.0f, 7.5f, 100.0f, 0.0f, 512.0f})
        for (int k = 0; k < n_rects; ++k) {
            const size_t bytes = size_t(pitch) * (H - 1) + size_t(W) * 3;           // the last row ends with its last pixel
            uint8_t* a = new uint8_t[bytes];
            uint8_t* b = new uint8_t[bytes];
            uint32_t seed = 12345u + uint32_t(k);
            for (size_t i = 0; i < bytes; ++i) a[i] = b[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const int ra = mdjpeg_blur_regions(a, W, H, pitch, rects.data() + 4 * k, 1, radius);
            int32_t r;
            uint32_t ww, fw;
            mdjpeg_blur_weights(radius, &r, &ww, &fw);
            const int rb = mdjpeg_blur_regions_chunked(b, W, H, pitch, rects.data() + 4 * k, 1, radius, 2 * (18 * (r + 1) + 20));
            const bool same = memcmp(a, b, bytes) == 0;
            delete[] a;
            delete[] b;
            if (ra != MDJPEG_OK || rb != MDJPEG_OK || !same) { printf("blur: rectangle %d at radius %g: %d %d %d\n", k, double(radius), ra, rb, int(same)); return 5; }
        }
    // all rectangles one after the other in one image, and rectangles that leave it
    std::vector<uint8_t> img(size_t(pitch) * H, 77);
    if (mdjpeg_blur_regions(img.data(), W, H, pitch, rects.data(), n_rects, 40.0f) != MDJPEG_OK) return 5;
    const int32_t outside[8] = {0, 0, 5, 5, 90, 100, 98, 131};
    if (mdjpeg_blur_regions(img.data(), W, H, pitch, outside, 2, 40.0f) != MDJPEG_EINVAL) return 5;
    printf("blur: %d rectangles x 6 radii\n", n_rects);
    return 0;
}

// `--preview`: mdjpeg_resample and mdjpeg_draw on heap images of exactly pitch x (height - 1) + 3 x width bytes -- reducing,
// enlarging, one axis unchanged, a single pixel, a pitch above 3 x width, runs longer than a strip -- and operations that
// leave the image on every side, so that the sanitizers see any access outside an image.
static int preview_matrix() {
    const int shapes[][6] = {{97, 61, 40, 25, 0, 0}, {333, 500, 166, 249, 0, 0}, {50, 40, 120, 96, 0, 0}, {1000, 37, 70, 2, 0, 0}, {1, 1, 5, 5, 0, 0},
                             {640, 480, 640, 479, 0, 0}, {17, 9, 8, 4, 64, 29}, {1300, 40, 100, 3, 3907, 301}, {17, 9, 17, 9, 64, 64}, {3, 2000, 2, 1, 0, 0}};
    for (const auto& q : shapes) {
        const int w = q[0], h = q[1], dw = q[2], dh = q[3];
        const int64_t pitch = q[4] ? q[4] : int64_t(w) * 3, dpitch = q[5] ? q[5] : int64_t(dw) * 3;
        const size_t bytes = size_t(pitch) * (h - 1) + size_t(w) * 3, dbytes = size_t(dpitch) * (dh - 1) + size_t(dw) * 3;
        for (int shift = 0; shift < 4; ++shift) {                        // every alignment of the first byte
            uint8_t* a = new uint8_t[bytes + shift];
            uint8_t* b = new uint8_t[dbytes];
            uint32_t seed = 777u + uint32_t(w);
            for (size_t i = 0; i < bytes + shift; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const int rc = mdjpeg_resample(a + shift, w, h, pitch, b, dw, dh, dpitch);
            delete[] a;
            delete[] b;
            if (rc != MDJPEG_OK) { printf("preview: %dx%d -> %dx%d: %d\n", w, h, dw, dh, rc); return 6; }
        }
    }
    const int W = 53, H = 31;
    const int64_t pitch = 170;
    const size_t bytes = size_t(pitch) * (H - 1) + size_t(W) * 3;
    const int pw = 20, ph = 9;
    uint8_t* patch = new uint8_t[size_t(pw) * ph * 3 + 5];
    for (size_t i = 0; i < size_t(pw) * ph * 3 + 5; ++i) patch[i] = uint8_t(i);
    const int32_t ops[] = {0, 5, 5, 20, 12, 0x0000ff, 0, 0,   0, -7, -3, 2, 200, 0x00ff00, 0, 0,   0, 40, 25, 1000, 30, 0xff0000, 0, 0,
                           0, 10, 10, 9, 20, 0x123456, 0, 0,   0, -2147483647, -2147483647, 2147483647, 0, 0x654321, 0, 0,
                           1, -5, -4, pw, ph, 5, 0, 0,   1, W - 3, H - 2, pw, ph, 0, 0, 0,   1, 7, 11, pw, ph, 0, 0, 0,
                           1, 2147483000, 2147483000, pw, ph, 0, 0, 0,   1, -2147483647, 3, pw, ph, 0, 0, 0,   1, 30, 3, 0, 0, 0, 0, 0};
    const int n_ops = int(sizeof(ops) / sizeof(ops[0]) / MD_DRAW_OP_WORDS);
    uint8_t* img = new uint8_t[bytes];
    memset(img, 9, bytes);
    int rc = mdjpeg_draw(img, W, H, pitch, ops, n_ops, patch, int64_t(pw) * ph * 3 + 5);
    const int32_t outside[] = {1, 0, 0, pw, ph, 6, 0, 0};
    const int rb = mdjpeg_draw(img, W, H, pitch, outside, 1, patch, int64_t(pw) * ph * 3 + 5);
    const int32_t unknown[] = {2, 0, 0, 1, 1, 0, 0, 0};
    const int ru = mdjpeg_draw(img, W, H, pitch, unknown, 1, patch, 0);
    delete[] img;
    delete[] patch;
    if (rc != MDJPEG_OK || rb != MDJPEG_EINVAL || ru != MDJPEG_EINVAL) { printf("preview: draw %d %d %d\n", rc, rb, ru); return 6; }
    printf("preview: %d shapes x 4 alignments, %d operations\n", int(sizeof(shapes) / sizeof(shapes[0])), n_ops);
    return 0;
}

// `--draw-from`: mdjpeg_draw_from on heap images of exactly pitch x (height - 1) + 3 x width bytes against a copy followed by
// mdjpeg_draw -- the sizes whose rows are 3, 15, 21, 99 and 393 bytes, both pitches, a destination 0 .. 3 bytes off its
// source's alignment, three destinations on one source (one without an operation), a second source of another size in the
// same call, operations that hang over every edge, lie outside and cover the whole image -- and what it refuses.
static int draw_from_matrix() {
    const int sizes[][2] = {{1, 1}, {5, 3}, {7, 5}, {33, 17}, {131, 67}};
    const int pw = 9, ph = 4;
    const int64_t patch_bytes = int64_t(pw) * ph * 3 + 7;
    uint8_t* patch = new uint8_t[size_t(patch_bytes)];
    for (int64_t i = 0; i < patch_bytes; ++i) patch[i] = uint8_t(200 + i);
    int runs = 0;
    for (const auto& sz : sizes)
        for (int pad : {0, 5})
            for (int shift = 0; shift < 4; ++shift) {
                const int W = sz[0], H = sz[1], W2 = 6, H2 = 2;
                const int64_t pitch = int64_t(W) * 3 + pad, dpitch = int64_t(W) * 3 + (pad ? 5 : 0), pitch2 = int64_t(W2) * 3;
                const size_t bytes = size_t(pitch) * (H - 1) + size_t(W) * 3, dbytes = size_t(dpitch) * (H - 1) + size_t(W) * 3;
                const size_t bytes2 = size_t(pitch2) * (H2 - 1) + size_t(W2) * 3;
                uint8_t* s0 = new uint8_t[bytes];
                uint8_t* s1 = new uint8_t[bytes2];
                uint32_t seed = 31u + uint32_t(runs);
                for (size_t i = 0; i < bytes; ++i) s0[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
                for (size_t i = 0; i < bytes2; ++i) s1[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
                uint8_t* d[4];
                uint8_t* want[4];
                for (int m = 0; m < 3; ++m) d[m] = new uint8_t[dbytes + shift], want[m] = new uint8_t[dbytes];
                d[3] = new uint8_t[bytes2 + shift], want[3] = new uint8_t[bytes2];
                // destination 0: overlapping rectangles and patches, over every edge; 1: nothing; 2: the whole image, then a patch;
                // 3 (of the second source): a rectangle wholly outside and one inside
                const int32_t ops[] = {0, -3, -2, W / 2, H / 2, 0x0000ff, 0, 0,       0, W / 3, H / 3, W + 4, H + 9, 0x00ff00, 0, 0,
                                       1, -4, H - 2, pw, ph, 7, 0, 0,                 1, W - 2, -1, pw, ph, 0, 0, 0,
                                       0, W / 2, 0, W / 2, H - 1, 0x123456, 0, 0,     1, W + 1, H + 1, pw, ph, 0, 0, 0,
                                       0, -100, -100, 100000, 100000, 0xabcdef, 0, 0, 1, 0, 0, pw, ph, 3, 0, 0,
                                       0, W2, 0, W2 + 5, 3, 0x111111, 0, 0,           0, 1, 1, 3, 1, 0x222222, 0, 0};
                const int32_t op_image[] = {0, 0, 0, 0, 0, 0, 2, 2, 3, 3};
                const int first[] = {0, 6, 6, 8}, count[] = {6, 0, 2, 2};
                const uint8_t* src[2] = {s0, s1};
                const int32_t ws[2] = {W, W2}, hs[2] = {H, H2};
                const int64_t ps[2] = {pitch, pitch2};
                uint8_t* dst[4] = {d[0] + shift, d[1] + shift, d[2] + shift, d[3] + shift};
                const int32_t dst_src[4] = {0, 0, 0, 1};
                const int64_t dps[4] = {dpitch, dpitch, dpitch, pitch2};
                const int rc = mdjpeg_draw_from(src, ws, hs, ps, 2, dst, dst_src, dps, 4, op_image, ops, 10, patch, patch_bytes);
                bool same = rc == MDJPEG_OK;
                for (int m = 0; m < 4 && same; ++m) {
                    const int k = dst_src[m];
                    for (int y = 0; y < hs[k]; ++y) memcpy(want[m] + size_t(dps[m]) * y, src[k] + size_t(ps[k]) * y, size_t(ws[k]) * 3);
                    if (mdjpeg_draw(want[m], ws[k], hs[k], dps[m], ops + first[m] * MD_DRAW_OP_WORDS, count[m], patch, patch_bytes) != MDJPEG_OK) same = false;
                    for (int y = 0; y < hs[k] && same; ++y)
                        same = memcmp(want[m] + size_t(dps[m]) * y, dst[m] + size_t(dps[m]) * y, size_t(ws[k]) * 3) == 0;
                }
                // refused: a destination on its source, a source index and an operation's destination out of range, a patch beyond the buffer
                uint8_t* on_source[4] = {dst[0], const_cast<uint8_t*>(s0), dst[2], dst[3]};
                const int64_t on_pitch[4] = {dpitch, pitch, dpitch, pitch2};
                const int32_t bad_src[4] = {0, 2, 0, 1}, bad_image[] = {0, 0, 0, 0, 0, 0, 2, 4, 3, 3};
                const int r1 = mdjpeg_draw_from(src, ws, hs, ps, 2, on_source, dst_src, on_pitch, 4, op_image, ops, 10, patch, patch_bytes);
                const int r2 = mdjpeg_draw_from(src, ws, hs, ps, 2, dst, bad_src, dps, 4, op_image, ops, 10, patch, patch_bytes);
                const int r3 = mdjpeg_draw_from(src, ws, hs, ps, 2, dst, dst_src, dps, 4, bad_image, ops, 10, patch, patch_bytes);
                const int r4 = mdjpeg_draw_from(src, ws, hs, ps, 2, dst, dst_src, dps, 4, op_image, ops, 10, patch, int64_t(pw) * ph * 3 + 6);
                delete[] s0;
                delete[] s1;
                for (int m = 0; m < 4; ++m) { delete[] d[m]; delete[] want[m]; }
                if (!same || r1 != MDJPEG_EINVAL || r2 != MDJPEG_EINVAL || r3 != MDJPEG_EINVAL || r4 != MDJPEG_EINVAL) {
                    printf("draw-from: %dx%d pad %d shift %d: %d %d %d %d %d %d\n", W, H, pad, shift, rc, int(same), r1, r2, r3, r4);
                    delete[] patch;
                    return 9;
                }
                ++runs;
            }
    delete[] patch;
    printf("draw-from: %d runs\n", runs);
    return 0;
}

// `--classify`: mdjpeg_classifier_input on heap images of exactly pitch x (src_h - 1) + 3 x src_w bytes and an output of
// exactly 3 x size x size floats -- reducing, enlarging, a single column, an unchanged size, more than one strip, canvases
// with zeros on every side, the three filters -- so that the sanitizers see any access outside a rectangle or the tensor.
static int classify_matrix() {
    // src_w, src_h, canvas_w, canvas_h, off_x, off_y, size, pitch (0: 3 x src_w)
    const int shapes[][8] = {{97, 61, 97, 61, 0, 0, 32, 0},     {5, 7, 5, 7, 0, 0, 32, 0},         {1, 9, 1, 9, 0, 0, 32, 0},
                             {301, 187, 301, 187, 0, 0, 32, 908}, {333, 500, 333, 500, 0, 0, 80, 0}, {80, 200, 80, 200, 0, 0, 80, 245},
                             {640, 480, 640, 480, 0, 0, 224, 0}, {1300, 40, 1300, 40, 0, 0, 32, 0}, {40, 30, 50, 50, 10, 0, 32, 0},
                             {40, 30, 50, 50, 0, 20, 32, 0},     {40, 30, 50, 50, 0, 0, 32, 121},   {21, 17, 60, 60, 20, 30, 32, 0},
                             {13, 20, 20, 20, 4, 0, 32, 0},      {2, 2, 3000, 3000, 1500, 1500, 8, 0}};
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    int runs = 0;
    for (const auto& q : shapes)
        for (int filter = 0; filter < 3; ++filter) {
            const int64_t pitch = q[7] ? q[7] : int64_t(q[0]) * 3;
            const size_t bytes = size_t(pitch) * (q[1] - 1) + size_t(q[0]) * 3;
            const int shift = runs & 3;                                  // every alignment of the first byte
            uint8_t* a = new uint8_t[bytes + shift];
            float* o = new float[size_t(3) * q[6] * q[6]];
            uint32_t seed = 99u + uint32_t(runs);
            for (size_t i = 0; i < bytes + shift; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const int rc = mdjpeg_classifier_input(a + shift, pitch, q[0], q[1], q[2], q[3], q[4], q[5], q[6], filter, mean, stdv, o);
            delete[] a;
            delete[] o;
            if (rc != MDJPEG_OK) { printf("classify: %dx%d in %dx%d at %d, filter %d: %d\n", q[0], q[1], q[2], q[3], q[6], filter, rc); return 7; }
            ++runs;
        }
    uint8_t px[3] = {1, 2, 3};
    float o1[3];
    const float zero[3] = {0.229f, 0.0f, 0.225f};
    int32_t plan[2];
    const int bad[] = {mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 1, 3, mean, stdv, o1), mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 1, 0, mean, zero, o1),
                       mdjpeg_classifier_input(px, 3, 1, 1, 4, 4, 4, 0, 1, 0, mean, stdv, o1), mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 0, 0, mean, stdv, o1)};
    for (int rc : bad)
        if (rc != MDJPEG_EINVAL) { printf("classify: a bad argument gives %d\n", rc); return 7; }
    if (mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 1, 0, mean, stdv, o1) != MDJPEG_OK) return 7;
    if (mdjpeg_classifier_plan(65535, 65535, 8, MD_FILTER_LANCZOS, 0, plan) != MDJPEG_EUNSUPPORTED) { printf("classify: plan\n"); return 7; }
    printf("classify: %d runs\n", runs);
    return 0;
}

// `--thumbnails`: mdjpeg_thumbnails on heap images of exactly pitch x (src_h - 1) + 3 x src_w bytes and sheets of exactly
// dst_pitch x (out_h - 1) + 3 x out_w bytes -- reducing, enlarging, one axis unchanged, a copy, a single pixel either way,
// canvases with zeros on every side and wholly of zeros, a tap run longer than a strip, the three filters -- so that the
// sanitizers see any access outside a rectangle or a tile.
static int thumbnails_matrix() {
    // src_w, src_h, canvas_w, canvas_h, off_x, off_y, out_w, out_h, pitch (0: 3 x src_w), dst_pitch (0: 3 x out_w)
    const int shapes[][10] = {{97, 61, 97, 61, 0, 0, 13, 9, 0, 0},    {9, 7, 9, 7, 0, 0, 40, 31, 0, 121},  {40, 30, 40, 30, 0, 0, 40, 11, 0, 0},
                              {40, 30, 40, 30, 0, 0, 17, 30, 127, 0}, {31, 20, 31, 20, 0, 0, 31, 20, 0, 100}, {50, 40, 50, 40, 0, 0, 1, 1, 0, 0},
                              {1, 1, 1, 1, 0, 0, 5, 5, 0, 0},         {40, 30, 50, 30, 10, 0, 20, 12, 0, 0}, {40, 30, 50, 30, 0, 0, 20, 12, 0, 0},
                              {40, 30, 40, 41, 0, 11, 20, 12, 0, 0},  {40, 30, 40, 41, 0, 0, 20, 12, 0, 67}, {1, 1, 30, 30, 29, 29, 7, 7, 0, 0},
                              {1300, 40, 1300, 40, 0, 0, 20, 3, 0, 0}, {0, 0, 12, 9, 0, 0, 5, 4, 3, 0}, {0, 5, 12, 9, 0, 0, 12, 9, 3, 0}, {8, 8, 8, 60000, 0, 29000, 3, 40, 0, 0}};
    int runs = 0;
    for (const auto& q : shapes)
        for (int filter = 0; filter < 3; ++filter) {
            const int64_t pitch = q[8] ? q[8] : int64_t(q[0]) * 3, dpitch = q[9] ? q[9] : int64_t(q[6]) * 3;
            const size_t bytes = q[0] && q[1] ? size_t(pitch) * (q[1] - 1) + size_t(q[0]) * 3 : 0, dbytes =size_t(dpitch) * (q[7] - 1) + size_t(q[6]) * 3;
            const int shift = runs & 3;                                  // every alignment of the first byte
            uint8_t* a = new uint8_t[bytes + shift];
            uint8_t* o = new uint8_t[dbytes];
            uint32_t seed = 4242u + uint32_t(runs);
            for (size_t i = 0; i < bytes + shift; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const mdjpeg_thumbnail t = {a + shift, pitch, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], o, dpitch};
            const int rc = mdjpeg_thumbnails(&t, 1, filter);
            delete[] a;
            delete[] o;
            if (rc != MDJPEG_OK) { printf("thumbnails: %dx%d in %dx%d to %dx%d, filter %d: %d\n", q[0], q[1], q[2], q[3], q[6], q[7], filter, rc); return 8; }
            ++runs;
        }
    uint8_t px[3] = {1, 2, 3}, o1[3];
    const mdjpeg_thumbnail bad[] = {{px, 3, 1, 1, 4, 4, 4, 0, 1, 1, o1, 3}, {px, 3, 1, 1, 1, 1, 0, 0, 0, 1, o1, 3}, {px, 3, 1, 1, 1, 1, 0, 0, 1, 1, o1, 2},
                                    {nullptr, 3, 1, 1, 1, 1, 0, 0, 1, 1, o1, 3}, {px, 3, 1, 1, 1, 1, 0, 0, 1, 1, nullptr, 3}};
    for (const mdjpeg_thumbnail& t : bad)
        if (mdjpeg_thumbnails(&t, 1, 0) != MDJPEG_EINVAL) { printf("thumbnails: a bad argument is accepted\n"); return 8; }
    const mdjpeg_thumbnail good = {px, 3, 1, 1, 1, 1, 0, 0, 1, 1, o1, 3}, tall = {px, 3, 1, 1, 1, 60000, 0, 0, 1, 1, o1, 3};
    if (mdjpeg_thumbnails(&good, 1, 3) != MDJPEG_EINVAL || mdjpeg_thumbnails(&good, 1, 0) != MDJPEG_OK || o1[0] != 1 || o1[2] != 3) return 8;
    if (mdjpeg_thumbnails(&tall, 1, 0) != MDJPEG_EUNSUPPORTED) { printf("thumbnails: plan\n"); return 8; }
    printf("thumbnails: %d runs\n", runs);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--thumbnails")) return thumbnails_matrix();
    if (argc == 2 && !strcmp(argv[1], "--classify")) return classify_matrix();
    if (argc == 2 && !strcmp(argv[1], "--preview")) return preview_matrix();
    if (argc == 2 && !strcmp(argv[1], "--draw-from")) return draw_from_matrix();
    if (argc == 2 && !strcmp(argv[1], "--blur")) return blur_matrix();
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("%s: cannot open\n", argv[i]); continue; }
        std::vector<uint8_t> bytes;
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
        fclose(f);
        uint8_t* exact = new uint8_t[bytes.size() ? bytes.size() : 1];          // exact extent: reads past the file are seen
        memcpy(exact, bytes.data(), bytes.size());
        mdjpeg_info info;
        int rc = mdjpeg_parse(exact, bytes.size(), &info);
        if (rc == MDJPEG_OK) {
            int16_t* coef = new int16_t[size_t(info.coef_count)];
            rc = mdjpeg_decode(exact, bytes.size(), &info, coef, size_t(info.coef_count));
            const int sampling = info.h_samp[0] == 1 && info.v_samp[0] == 1 ? 0 : info.h_samp[0] == 2 && info.v_samp[0] == 1 ? 1
                                 : info.h_samp[0] == 2 && info.v_samp[0] == 2 ? 2 : -1;
            if (rc == MDJPEG_OK && info.components == 3 && sampling >= 0) {
                // and back: the host model of the GPU entropy ENCODER on these coefficients, output buffers of the exact size
                const int16_t* planes = coef;
                for (int chunk : {1, 3, 64}) {
                    int64_t off, size;
                    size_t need = 0;
                    int re = mdjpeg_encode_subsequences_sampled(&planes, &info.width, &info.height, &sampling, 1, chunk, nullptr, 0, &off, &size, &need);
                    if (re == MDJPEG_ECAPACITY) {
                        uint8_t* scan = new uint8_t[need];
                        re = mdjpeg_encode_subsequences_sampled(&planes, &info.width, &info.height, &sampling, 1, chunk, scan, need, &off, &size, &need);
                        delete[] scan;
                    }
                    if (re != MDJPEG_OK && re != MDJPEG_ECORRUPT) { printf("%s: encoding at chunk %d gives %d\n", argv[i], chunk, re); return 4; }
                }
            }
            delete[] coef;
            // the descriptor and the host model of the GPU decoder, at two subsequence lengths, into exact buffers too
            mdjpeg_scan_info sc;
            std::vector<uint32_t> seg(1);
            int rs = mdjpeg_scan(exact, bytes.size(), &sc, seg.data(), seg.size());
            if (rs == MDJPEG_ECAPACITY && sc.n_segments > 0) {
                uint32_t* segs = new uint32_t[size_t(sc.n_segments)];
                rs = mdjpeg_scan(exact, bytes.size(), &sc, segs, size_t(sc.n_segments));
                delete[] segs;
            }
            for (int bits : {64, 1024}) {
                mdjpeg_info info2;
                int16_t* coef2 = new int16_t[size_t(info.coef_count)];
                const int r2 = mdjpeg_decode_subsequences(exact, bytes.size(), bits, &info2, coef2, size_t(info.coef_count));
                delete[] coef2;
                if (r2 != rc) { printf("%s: subsequences of %d bits give %d, mdjpeg_decode %d\n", argv[i], bits, r2, rc); return 3; }
            }
        }
        printf("%s: rc %d %s\n", argv[i], rc, info.reason);
        delete[] exact;
    }
    return 0;
}
