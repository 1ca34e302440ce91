// The number of gray pixels (R == G and R == B) inside a rectangle of an RGB image: what the device kernel (gray_kernels.cpp,
// mdhip_gray_count) and the host model (gray_host.cpp, mdjpeg_gray_count) share, so that both judge a pixel with one statement.
// It is the numerator of the reference's visualization_utils.gray_scale_fraction, np.logical_and(r == g, r == b).sum().
//
// A window is a rectangle (x, y, w, h) of an image of `width` x `height` pixels, 3 bytes a pixel, `pitch` bytes a row, at any
// base address.  Only the 3 * w bytes of each of its h rows are ever read, by either leg.
//
// The walk of a row (gc_count_group), which the kernel takes and the host model can take (mdjpeg_gray_count_walk):
//   head    the first `row address & 3` pixels, byte by byte.  3 is its own inverse modulo 4, so after (address & 3) pixels the
//           address is a multiple of 4: address + 3 * (address & 3) = address + 4 * (address & 3) - (address & 3).
//   groups  from there four pixels at a time: 12 bytes, read as three aligned 32-bit words (gc_count_words)
//   tail    a last group of fewer than four pixels, byte by byte
// Group g of a row holds the pixels head + 4 g .. head + 4 g + 3; group 0 takes the head as well.  A row of w pixels has at
// most gc_groups(w) = (w + 3) / 4 groups with a pixel in them, whatever its head.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GC_HD __host__ __device__
#else
#define GC_HD
#endif

#define GC_MAX_IMAGES 65535       /* images of one call */
#define GC_MAX_SIDE 65535         /* width and height: 1 .. 65535 */

// THE counting statement
GC_HD inline uint32_t gc_is_gray(uint32_t r, uint32_t g, uint32_t b) { return (r == g && r == b) ? 1u : 0u; }

// byte k (0 .. 11) of twelve bytes held in three little-endian words
GC_HD inline uint32_t gc_byte(const uint32_t v[3], int k) { return (v[k >> 2] >> (8 * (k & 3))) & 255u; }

// the gray pixels among the four that three words hold
GC_HD inline uint32_t gc_count_words(const uint32_t v[3]) {
    uint32_t n = 0;
    for (int p = 0; p < 4; ++p) n += gc_is_gray(gc_byte(v, 3 * p), gc_byte(v, 3 * p + 1), gc_byte(v, 3 * p + 2));
    return n;
}

GC_HD inline uint32_t gc_groups(int w) { return ((uint32_t)w + 3u) / 4u; }

// the gray pixels of group g of a row of w pixels that starts at `row`; g < gc_groups(w)
GC_HD inline uint32_t gc_count_group(const uint8_t* row, int w, uint32_t g) {
    int head = (int)((uintptr_t)row & 3);
    if (head > w) head = w;
    uint32_t n = 0;
    if (g == 0)
        for (int x = 0; x < head; ++x) n += gc_is_gray(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    const long long x0 = (long long)head + 4 * (long long)g;
    if (x0 + 4 <= w) {
        uint32_t v[3];
        memcpy(v, __builtin_assume_aligned(row + 3 * x0, 4), 12);
        n += gc_count_words(v);
    } else {
        for (long long x = x0; x < w; ++x) n += gc_is_gray(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    }
    return n;
}

// what both entry points refuse (the images are never dereferenced here): a NULL array or image, n outside 1 .. GC_MAX_IMAGES,
// a side outside 1 .. GC_MAX_SIDE, a pitch below its row, an image whose last byte lies 2 GB or more behind its first, a
// window without area or one that leaves its image.  1 = fine; *bad: the first image that is not (-1: the arrays or n)
inline int gc_args_ok(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                      const int32_t* windows, int n, const void* counts, int* bad) {
    *bad = -1;
    if (!images || !widths || !heights || !pitches || !windows || !counts || n < 1 || n > GC_MAX_IMAGES) return 0;
    for (int i = 0; i < n; ++i) {
        *bad = i;
        const int32_t* q = windows + 4 * (size_t)i;
        if (!images[i] || widths[i] < 1 || heights[i] < 1 || widths[i] > GC_MAX_SIDE || heights[i] > GC_MAX_SIDE) return 0;
        if (pitches[i] < (long long)widths[i] * 3 || (long long)(heights[i] - 1) * pitches[i] + (long long)widths[i] * 3 > 0x7fff0000LL) return 0;
        if (q[0] < 0 || q[1] < 0 || q[2] < 1 || q[3] < 1 || q[2] > widths[i] - q[0] || q[3] > heights[i] - q[1]) return 0;
    }
    *bad = -1;
    return 1;
}
