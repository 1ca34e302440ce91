// The statements of libjpeg's integer encoder that more than one kernel file compiles: the colour conversion of a pixel, one
// pass of the "islow" forward DCT, and the quantisation of a coefficient.  jpeg_kernels.cpp (recompression of a window) and
// jpeg_encode.cpp (the coefficients the entropy encoder reads) share them, so that the two cannot drift apart.
#ifndef MDHIP_JPEG_DCT_H
#define MDHIP_JPEG_DCT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdhip {
namespace jpeg_dct {

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pixel of the window (clamped coordinates: the callers replicate edges) -> Y, Cb, Cr of jccolor.c
__device__ __forceinline__ void load_ycc(const uint8_t* src, long long pitch, int sx, int sy, int& y, int& cb, int& cr) {
    const uint8_t* p = src + (long long)sy * pitch + (long long)sx * 3;
    const int r = p[0], g = p[1], b = p[2];
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// one 1-D pass of jpeg_fdct_islow; pass 1 (rows) scales up by PASS1_BITS, pass 2 (columns) takes it out again
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int* d, int* o) {
    constexpr int n = FIRST ? 11 : 15;
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7];
    int tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5];
    int tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        o[0] = (tmp10 + tmp11) * 4;
        o[4] = (tmp10 - tmp11) * 4;
    } else {
        o[0] = descale(tmp10 + tmp11, 2);
        o[4] = descale(tmp10 - tmp11, 2);
    }
    int z1 = (tmp12 + tmp13) * 4433;
    o[2] = descale(z1 + tmp13 * 6270, n);
    o[6] = descale(z1 + tmp12 * (-15137), n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6;
    int z3 = tmp4 + tmp6;
    int z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446;
    tmp5 *= 16819;
    tmp6 *= 25172;
    tmp7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    o[7] = descale(tmp4 + z1 + z3, n);
    o[5] = descale(tmp5 + z2 + z4, n);
    o[3] = descale(tmp6 + z2 + z3, n);
    o[1] = descale(tmp7 + z1 + z4, n);
}

// magnitude of the quantised coefficient: division by 8 * table entry (the forward DCT leaves its output scaled by 8), rounded
// half away from zero
__device__ __forceinline__ unsigned quant_magnitude(int w, unsigned q) {
    const unsigned div = q * 8u;
    return (unsigned(w < 0 ? -w : w) + (div >> 1)) / div;
}

}  // namespace jpeg_dct
}  // namespace mdhip

#endif  // MDHIP_JPEG_DCT_H
