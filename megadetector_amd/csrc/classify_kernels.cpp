// GPU kernels of the classifier input (mdhip_classifier_input) and of the thumbnails (mdhip_thumbnails): ONE kernel body with
// two epilogues.  n detections of a batch go from their images to ONE normalised fp32 tensor [n][3][S][S] in ONE launch --
// canvas, Pillow's resize (bicubic, bilinear or LANCZOS, bit for bit), centre crop, ToTensor and Normalize; or n tiles go
// from their images to their places in sheets of interleaved bytes in ONE launch -- Image.crop(box).resize((w, h)) and
// Image.paste.  The tables, the plan and the two per-byte functions are those of resample.h, which libmdjpeg.so's host models
// mdjpeg_classifier_input and mdjpeg_thumbnails compile too.  Integer arithmetic up to the table lookup, plain C++ and vector
// memory operations only.
//
//   window_kernel<BYTES>     the record is blockIdx.y; blockIdx.x is a tile of `strip` (<= 64) output columns and `rows`
//                            (<= 32) output rows of its out_w x out_h window.  Stage 1: the horizontal pass of the canvas rows the
//                            tile's vertical taps cover, one lane per byte, into an 8-bit tile in LDS; the source bytes come
//                            through L1, and only bytes of the record's rectangle are read -- a canvas row or a tap outside
//                            it is the canvas's zero.  Stage 2, BYTES = false: one lane per output value sums the vertical
//                            taps from LDS, clips, looks the float up (3 x 256 entries made on the host) and stores it;
//                            neighbouring lanes own neighbouring x of one plane row, so a wave writes 256 contiguous bytes.
//                            BYTES = true: one lane per output byte, neighbouring lanes own neighbouring bytes of one row of
//                            the tile in its sheet (LDS reads of a wave are 64 neighbouring bytes of a tile row: no bank
//                            conflict beyond the 4 lanes that share a dword); only the 3 nx bytes of the row are stored.
//                            Neighbouring row tiles repeat 2 support / rows of the horizontal pass.
//
// Bounds: a source read is row sy in [0, src_h) and pixel sx in [0, src_w) of the rectangle (md_classify_hsample clamps the
// run); the tile holds count x 3 strip bytes <= MD_CLASSIFY_LDS_BYTES (md_classify_plan, from the same tables); a float store
// goes to crop < n, plane < 3, row < S, column < S of the output; a byte store to row < out_h and byte < 3 out_w of the tile
// at dst (mdhip_thumbnails checks the window against dst_pitch and that dst is device memory).

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "resample.h"

namespace mdhip {

namespace {

constexpr int LANES = 256;

static_assert(MD_CLASSIFY_LDS_BYTES <= 64 * 1024, "static LDS of a workgroup");

template <bool BYTES>
__global__ __launch_bounds__(LANES) void window_kernel(const MdClassifyCrop* __restrict__ crops, const int32_t* __restrict__ table,
                                                       const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[MD_CLASSIFY_LDS_BYTES];
    const MdClassifyCrop d = crops[blockIdx.y];
    if ((int)blockIdx.x >= d.strips * d.row_tiles) return;              // (uniform: the whole workgroup leaves)
    const int t = threadIdx.x;
    const int g = blockIdx.x / d.strips, k = blockIdx.x - g * d.strips;
    const int x0 = k * d.strip, nx = min(d.strip, d.out_w - x0);
    const int r0 = g * d.rows, nr = min(d.rows, d.out_h - r0);
    const int pitch = nx * 3;
    int first, count;
    md_classify_rows(d, table, r0, r0 + nr, &first, &count);
    for (int i = t; i < count * pitch; i += LANES) {
        const int j = i / pitch, b = i - j * pitch;
        const int px = b / 3, c = b - px * 3;
        tile[i] = md_classify_hsample(d, table, first + j, x0 + px, c);
    }
    __syncthreads();
    if (BYTES) {
        uint8_t* row0 = d.dst + (long long)x0 * 3;
        for (int i = t; i < nr * pitch; i += LANES) {
            const int j = i / pitch, b = i - j * pitch;
            row0[(long long)(r0 + j) * d.dst_pitch + b] = md_classify_vsample(d, table, tile, pitch, first, r0 + j, b);
        }
        return;
    }
    float* plane0 = out + (size_t)blockIdx.y * 3 * d.out_h * d.out_w;
    for (int i = t; i < 3 * nr * nx; i += LANES) {
        const int q = i / nx, px = i - q * nx;
        const int c = q / nr, y = r0 + (q - c * nr);
        const uint8_t v = md_classify_vsample(d, table, tile, pitch, first, y, px * 3 + c);
        plane0[((size_t)c * d.out_h + y) * d.out_w + x0 + px] = lut[c * 256 + v];
    }
}

}  // namespace

hipError_t launch_classifier_input(const MdClassifyCrop* crops, int n, int max_blocks, const int32_t* table, const float* lut, float* out,
                                   hipStream_t s) {
    if (n < 1 || n > 65535 || max_blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_kernel<false>, dim3((unsigned)max_blocks, (unsigned)n), dim3(LANES), 0, s, crops, table, lut, out);
    return hipGetLastError();
}

hipError_t launch_thumbnails(const MdClassifyCrop* tiles, int n, int max_blocks, const int32_t* table, hipStream_t s) {
    if (n < 1 || n > 65535 || max_blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_kernel<true>, dim3((unsigned)max_blocks, (unsigned)n), dim3(LANES), 0, s, tiles, table, (const float*)nullptr,
                       (float*)nullptr);
    return hipGetLastError();
}

}  // namespace mdhip
