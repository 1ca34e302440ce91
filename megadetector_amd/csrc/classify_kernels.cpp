// GPU kernel of the classifier input (mdhip_classifier_input): n detections of a batch go from their images to ONE
// normalised fp32 tensor [n][3][S][S] in ONE launch -- canvas, Pillow's resize (bicubic, bilinear or LANCZOS, bit for
// bit), centre crop, ToTensor and Normalize.  The tables, the plan and the two per-byte functions are those of resample.h,
// which libmdjpeg.so's host model mdjpeg_classifier_input compiles too.  Integer arithmetic up to the table lookup, plain
// C++ and vector memory operations only.
//
//   classifier_input_kernel  the crop is blockIdx.y; blockIdx.x is a tile of `strip` (<= 64) output columns and `rows`
//                            (<= 32) output rows of its S x S window.  Stage 1: the horizontal pass of the canvas rows the
//                            tile's vertical taps cover, one lane per byte, into an 8-bit tile in LDS; the source bytes come
//                            through L1, and only bytes of the crop's rectangle are read -- a canvas row or a tap outside
//                            it is the canvas's zero.  Stage 2: one lane per output value sums the vertical taps from
//                            LDS, clips, looks the float up (3 x 256 entries made on the host) and stores it; neighbouring
//                            lanes own neighbouring x of one plane row, so a wave writes 256 contiguous bytes.
//                            Neighbouring row tiles repeat 2 support / rows of the horizontal pass.
//
// Bounds: a source read is row sy in [0, src_h) and pixel sx in [0, src_w) of the rectangle (md_classify_hsample clamps the
// run); the tile holds count x 3 strip bytes <= MD_CLASSIFY_LDS_BYTES (md_classify_plan, from the same tables); a store goes
// to crop < n, plane < 3, row < S, column < S of the output.

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "resample.h"

namespace mdhip {

namespace {

constexpr int LANES = 256;

static_assert(MD_CLASSIFY_LDS_BYTES <= 64 * 1024, "static LDS of a workgroup");

__global__ __launch_bounds__(LANES) void classifier_input_kernel(const MdClassifyCrop* __restrict__ crops, const int32_t* __restrict__ table,
                                                                 const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[MD_CLASSIFY_LDS_BYTES];
    const MdClassifyCrop d = crops[blockIdx.y];
    if ((int)blockIdx.x >= d.strips * d.row_tiles) return;              // (uniform: the whole workgroup leaves)
    const int t = threadIdx.x;
    const int g = blockIdx.x / d.strips, k = blockIdx.x - g * d.strips;
    const int x0 = k * d.strip, nx = min(d.strip, d.size - x0);
    const int r0 = g * d.rows, nr = min(d.rows, d.size - r0);
    const int pitch = nx * 3;
    int first, count;
    md_classify_rows(d, table, r0, r0 + nr, &first, &count);
    for (int i = t; i < count * pitch; i += LANES) {
        const int j = i / pitch, b = i - j * pitch;
        const int px = b / 3, c = b - px * 3;
        tile[i] = md_classify_hsample(d, table, first + j, x0 + px, c);
    }
    __syncthreads();
    float* plane0 = out + (size_t)blockIdx.y * 3 * d.size * d.size;
    for (int i = t; i < 3 * nr * nx; i += LANES) {
        const int q = i / nx, px = i - q * nx;
        const int c = q / nr, y = r0 + (q - c * nr);
        const uint8_t v = md_classify_vsample(d, table, tile, pitch, first, y, px * 3 + c);
        plane0[((size_t)c * d.size + y) * d.size + x0 + px] = lut[c * 256 + v];
    }
}

}  // namespace

hipError_t launch_classifier_input(const MdClassifyCrop* crops, int n, int max_blocks, const int32_t* table, const float* lut, float* out,
                                   hipStream_t s) {
    if (n < 1 || n > 65535 || max_blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(classifier_input_kernel, dim3((unsigned)max_blocks, (unsigned)n), dim3(LANES), 0, s, crops, table, lut, out);
    return hipGetLastError();
}

}  // namespace mdhip
