// mdjpeg_gray_count: the host model of mdhip_gray_count (gray_kernels.cpp) and the counting of the backend='host' tests of
// megadetector_amd/gray_scale.py.  It asks csrc/gray_count.h's statement of every pixel of the window, one after the other, the
// plain way; mdjpeg_gray_count_walk takes the kernel's walk instead (head, groups of four pixels as three words, tail), so the
// walk is checked on the host -- under AddressSanitizer too (`make asan-gray`) -- before it runs on a device.
#include "../../include/mdjpeg.h"
#include "gray_count.h"

extern "C" int mdjpeg_gray_count(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                                 const int32_t* windows, int n, uint64_t* counts) {
    int bad;
    if (!gc_args_ok(images, widths, heights, pitches, windows, n, counts, &bad)) return MDJPEG_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int32_t* q = windows + 4 * (size_t)i;
        uint64_t c = 0;
        for (int y = q[1]; y < q[1] + q[3]; ++y) {
            const uint8_t* row = images[i] + (int64_t)y * pitches[i];
            for (int x = q[0]; x < q[0] + q[2]; ++x) c += gc_is_gray(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
        }
        counts[i] = c;
    }
    return MDJPEG_OK;
}

extern "C" int mdjpeg_gray_count_walk(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                                      const int32_t* windows, int n, uint64_t* counts) {
    int bad;
    if (!gc_args_ok(images, widths, heights, pitches, windows, n, counts, &bad)) return MDJPEG_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int32_t* q = windows + 4 * (size_t)i;
        const uint8_t* origin = images[i] + (int64_t)q[1] * pitches[i] + 3 * (int64_t)q[0];
        const uint32_t groups = gc_groups(q[2]), total = groups * (uint32_t)q[3];
        uint64_t c = 0;
        for (uint32_t k = 0; k < total; ++k) c += gc_count_group(origin + (int64_t)(k / groups) * pitches[i], q[2], k % groups);
        counts[i] = c;
    }
    return MDJPEG_OK;
}

#ifdef MDGRAY_ASAN_MAIN
// `make asan-gray`: both functions under AddressSanitizer + UBSan, as a program of its own.  Every image lies in a heap block
// of exactly its bytes at every byte offset 0 .. 7 of it, so a read before the first or behind the last byte of the rows is
// reported; the counts are compared with the known number of gray pixels.
#include <stdio.h>
#include <stdlib.h>

static int run(int w, int h, int pad, int offset, int wx, int wy, int ww, int wh) {
    const int64_t pitch = 3LL * w + pad;
    const size_t bytes = (size_t)((h - 1) * pitch + 3LL * w);
    uint8_t* block = (uint8_t*)malloc(offset + bytes);
    uint8_t* img = block + offset;
    for (size_t k = 0; k < bytes; ++k) img[k] = 0x55;                   // the padding between rows too: it must not be read as pixels
    uint64_t want = 0;
    uint32_t seed = (uint32_t)(w * 7919 + h * 104729 + pad * 31 + offset);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            seed = seed * 1664525u + 1013904223u;
            uint8_t* p = img + y * pitch + 3 * x;
            const int kind = (seed >> 24) % 4;                          // gray, R off, G off, B off
            p[0] = p[1] = p[2] = (uint8_t)(seed >> 8);
            if (kind) p[kind - 1] ^= 1;
            if (!kind && x >= wx && x < wx + ww && y >= wy && y < wy + wh) ++want;
        }
    const uint8_t* images[1] = {img};
    const int32_t widths[1] = {w}, heights[1] = {h}, window[4] = {wx, wy, ww, wh};
    const int64_t pitches[1] = {pitch};
    uint64_t plain = ~0ull, walk = ~0ull;
    const int rc0 = mdjpeg_gray_count(images, widths, heights, pitches, window, 1, &plain);
    const int rc1 = mdjpeg_gray_count_walk(images, widths, heights, pitches, window, 1, &walk);
    free(block);
    const bool ok = rc0 == MDJPEG_OK && rc1 == MDJPEG_OK && plain == want && walk == want;
    if (!ok)
        printf("WRONG: %dx%d pad %d offset %d window (%d, %d, %d, %d): plain %llu, walk %llu, want %llu\n", w, h, pad, offset, wx, wy, ww, wh,
               (unsigned long long)plain, (unsigned long long)walk, (unsigned long long)want);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0, cases = 0;
    const int widths[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33, 67};
    for (int w : widths)
        for (int h = 1; h <= 3; ++h)
            for (int pad = 0; pad <= 5; pad += (pad ? 4 : 1))              // 0, 1, 5
                for (int offset = 0; offset < 8; ++offset) {
                    bad += run(w, h, pad, offset, 0, 0, w, h), ++cases;
                    if (w > 5) bad += run(w, h, pad, offset, 1, 0, w - 1, h) + run(w, h, pad, offset, 5, h - 1, w - 5, 1), cases += 2;
                    if (w > 2) bad += run(w, h, pad, offset, 1, 0, 1, h), ++cases;
                }
    // what both refuse: a window that leaves its image, one without area, n = 0, a NULL image
    uint8_t px[12] = {0};
    const uint8_t* images[1] = {px};
    const uint8_t* none[1] = {nullptr};
    const int32_t two[1] = {2}, win_out[4] = {1, 0, 2, 2}, win_empty[4] = {0, 0, 0, 2}, win_ok[4] = {0, 0, 2, 2};
    const int64_t pitch[1] = {6};
    uint64_t c = 77;
    bad += mdjpeg_gray_count(images, two, two, pitch, win_out, 1, &c) != MDJPEG_EINVAL;
    bad += mdjpeg_gray_count(images, two, two, pitch, win_empty, 1, &c) != MDJPEG_EINVAL;
    bad += mdjpeg_gray_count(images, two, two, pitch, win_ok, 0, &c) != MDJPEG_EINVAL;
    bad += mdjpeg_gray_count_walk(none, two, two, pitch, win_ok, 1, &c) != MDJPEG_EINVAL;
    bad += c != 77;
    bad += mdjpeg_gray_count(images, two, two, pitch, win_ok, 1, &c) != MDJPEG_OK || c != 4;
    printf("%d cases, %d wrong\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
