// Pillow's Gaussian blur, shared by the GPU kernels (blur_kernels.cpp) and their host model (mdjpeg_blur_regions in
// image_host.cpp): ONE computation of the weights, ONE pass along a line, ONE plan for the row stage, compiled by both, so
// that the CPU suite and the host sanitizers exercise the very statements the lanes run (the arrangement of jpeg_subseq.h
// and jpeg_encode.h).
//
// What is computed (Pillow's BoxBlur.c, ImageFilter.GaussianBlur(radius) of an RGB image): three passes of an EXTENDED BOX
// FILTER along x, then three along y, every pass in 32-bit integers with an 8-bit rounding behind it:
//   box radius   radius -> fr, in fp32 except the square root (md_blur_box_radius); for radius 40: 39.49375...
//   weights      r = int(fr); ww = uint32(2^24 / (2 fr + 1)) (an fp32 division); fw = (2^24 - (2 r + 1) ww) / 2
//   one pass     out[x] = uint8((acc(x) ww + far(x) fw + 2^23) >> 24), acc(x) the sum of in[clamp(i)] for i = x - r .. x + r,
//                far(x) = in[clamp(x - r - 1)] + in[clamp(x + r + 1)], clamp to the line: the edges of the blurred
//                rectangle are replicated, not those of the image it was cut from
// The sums are exact in integers, so any order gives Pillow's bits: md_blur_line keeps a running sum -- two reads and one
// write a sample, and min(r, n - 1) reads to start a line -- and the cost follows the samples, not samples x (2 r + 1).
//
// The row stage in pieces (md_blur_plan_x): a workgroup keeps `rows` rows of a rectangle in two buffers of on-chip memory
// and a lane walks one channel of one row through the three passes.  A row that does not fit is cut into chunks with a
// halo: a pass is right at x as soon as x - r - 1 and x + r + 1 lie in what was loaded (or the rectangle ends there), so a
// pass spoils r + 1 samples at a cut and three passes spoil 3 (r + 1): a chunk loads that many samples beyond the outputs
// it keeps and runs the SAME line pass over all it loaded.
#ifndef MD_BLUR_BOX_H
#define MD_BLUR_BOX_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDB_HD __host__ __device__
#else
#define MDB_HD
#endif

#define MD_BLUR_MAX_RADIUS 512.0f        // of the API: the halo of a chunk, 3 (r + 1) samples on either side, must fit on chip
#define MD_BLUR_MAX_ROWS 64              // rows a workgroup of the row stage takes at the most (x 3 channels = 192 lanes)

struct MdBlurWeights {
    int32_t r;                           // whole samples on either side
    uint32_t ww, fw;                     // weight of a sample within r, and of the two samples at r + 1; (2 r + 1) ww + 2 fw <= 2^24
};

// _gaussian_blur_radius(radius, passes = 3) of BoxBlur.c: floats where it has floats, doubles where it has doubles, and no
// contraction into fused multiply-adds on a host that has them
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
static inline float md_blur_box_radius(float radius) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float sigma2 = radius * radius / 3;
    const float L = (float)sqrt(12.0 * sigma2 + 1.0);
    const float l = (float)floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    return l + a;
}

#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
static inline MdBlurWeights md_blur_weights(float radius) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float fr = md_blur_box_radius(radius);
    MdBlurWeights w;
    w.r = (int32_t)fr;
    w.ww = (uint32_t)(16777216.0f / (fr * 2 + 1));
    w.fw = (16777216u - (uint32_t)(2 * w.r + 1) * w.ww) / 2;
    return w;
}

// One pass along a line of n samples, `is` / `os` bytes from one sample to the next.  in and out must not overlap.
MDB_HD inline void md_blur_line(const uint8_t* __restrict__ in, int64_t is, uint8_t* __restrict__ out, int64_t os, int n, int r,
                                uint32_t ww, uint32_t fw) {
    const int last = n - 1;
    const int m = r < last ? r : last;
    // acc(0): samples -r .. 0 are in[0], samples 1 .. m are themselves, samples beyond the line are in[last]
    uint32_t acc = (uint32_t)(r + 1) * in[0];
    for (int i = 1; i <= m; ++i) acc += in[i * is];
    acc += (uint32_t)(r - m) * in[last * is];
    uint32_t left = in[0];                                   // in[clamp(x - r - 1)]
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
    for (int x = 0; x < n; ++x) {
        const int hi = x + r + 1 < last ? x + r + 1 : last;
        const int lo = x - r > 0 ? x - r : 0;
        const uint32_t a = in[hi * is], b = in[lo * is];
        out[x * os] = (uint8_t)((acc * ww + (left + a) * fw + (1u << 23)) >> 24);
        acc += a - b;
        left = b;
    }
}

// The three passes of one line between two buffers: p -> q -> p -> q; the result is in q.
MDB_HD inline void md_blur_line3(uint8_t* p, uint8_t* q, int64_t stride, int n, const MdBlurWeights& w) {
    md_blur_line(p, stride, q, stride, n, w.r, w.ww, w.fw);
    md_blur_line(q, stride, p, stride, n, w.r, w.ww, w.fw);
    md_blur_line(p, stride, q, stride, n, w.r, w.ww, w.fw);
}

// How the row stage takes a rectangle `width` samples wide with `lds_bytes` of on-chip memory for its two buffers.
struct MdBlurXPlan {
    int32_t rows;                        // rows a workgroup takes
    int32_t stride;                      // bytes from row to row in a buffer: a multiple of 4, an odd number of dwords
    int32_t chunks;                      // pieces a row is cut into (1: the whole row at once)
    int32_t step;                        // outputs a chunk keeps (the last one: what is left)
    int32_t halo;                        // samples a chunk loads beyond them on either side: 3 (r + 1)
};

MDB_HD inline int32_t md_blur_row_stride(int samples) { return ((samples * 3 + 3) / 4 * 4) | 4; }

// chunk k of a plan: keeps outputs [*o0, *o1) and loads samples [*a, *b) of the row
MDB_HD inline void md_blur_chunk(const MdBlurXPlan& p, int width, int k, int* o0, int* o1, int* a, int* b) {
    *o0 = k * p.step;
    *o1 = *o0 + p.step < width ? *o0 + p.step : width;
    *a = *o0 - p.halo > 0 ? *o0 - p.halo : 0;
    *b = *o1 + p.halo < width ? *o1 + p.halo : width;
}

// false: not even one row of a chunk with its halo fits (the API's bound on the radius keeps that from happening with
// the device's 48 KB).  A row that fits eight to a workgroup goes in one piece with as many rows as fit; a wider one is
// cut at the largest number of rows (8, 4, 2, 1) whose chunk is at least four halos long (at most half of what a chunk
// loads is thrown away), or goes in one piece as soon as it fits that number of rows.
MDB_HD inline bool md_blur_plan_x(int width, int r, int lds_bytes, MdBlurXPlan* p) {
    const int halo = 3 * (r + 1);
    p->halo = halo;
    for (int rows = 8; rows >= 1; rows >>= 1) {
        const int tile = (lds_bytes / (2 * rows) - 8) / 3;               // samples a row of a buffer can hold
        if (tile < 1) continue;
        if (width <= tile) {
            p->stride = md_blur_row_stride(width);
            p->rows = lds_bytes / (2 * p->stride);
            if (p->rows > MD_BLUR_MAX_ROWS) p->rows = MD_BLUR_MAX_ROWS;
            p->chunks = 1;
            p->step = width;
            return true;
        }
        if (tile >= 4 * halo || (rows == 1 && tile > 2 * halo)) {
            p->stride = md_blur_row_stride(tile);
            p->rows = rows;
            p->step = tile - 2 * halo;
            p->chunks = (width + p->step - 1) / p->step;
            return true;
        }
    }
    return false;
}

#endif
