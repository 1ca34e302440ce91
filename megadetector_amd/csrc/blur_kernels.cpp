// GPU Gaussian blur of rectangles of device images (mdhip_blur_regions): Pillow's ImageFilter.GaussianBlur, bit for bit,
// in place.  The weights, the pass along a line and the plan of the row stage are those of blur_box.h, which libmdjpeg.so's
// host model compiles too.  Integer arithmetic, plain C++ and vector memory operations only; every access to an image is
// a single byte, so nothing is read or written beside a rectangle whatever the pitch is.
//
// A rectangle takes two launches, and one launch serves one rectangle of EVERY image (blockIdx.y): the rectangles of one
// image are applied one after the other, the k-th rectangles of all images side by side.
//
//   blur_rows_kernel     a workgroup takes `rows` rows of a rectangle (or of one chunk of its rows, with the halo
//                        blur_box.h describes): bytes -> LDS buffer A, coalesced; then ONE LANE PER LINE -- a channel of a
//                        row -- walks the three passes A -> B -> A -> B with a running sum (two LDS reads and a write a
//                        sample; the reads do not depend on the sum, so they overlap); the bytes a chunk keeps go to the
//                        scratch plane S0, coalesced.  Rows are `stride` bytes apart, an odd number of dwords, so the
//                        lanes of a wave, which read the same x of different rows, fall on different banks.
//   blur_columns_kernel  one lane per BYTE COLUMN of the rectangle (3 w lanes, neighbours in x: every access of a wave is
//                        one run of bytes): S0 -> S1 -> S0 -> image, each pass a walk down the column with the running sum
//                        in a register.  A column is nobody else's, so the three passes need no barrier between them.
//
// The cost is two reads and a write per sample and pass; no lane ever loops over 2 r + 1 taps.

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "blur_box.h"

namespace mdhip {

namespace {

constexpr int ROW_LANES = MD_BLUR_MAX_ROWS * 3;      // one lane per line of the workgroup's rows
constexpr int COLUMN_LANES = 256;

static_assert(BLUR_LDS_BYTES <= 64 * 1024, "static LDS of a workgroup");

__global__ __launch_bounds__(ROW_LANES) void blur_rows_kernel(const BlurRect* __restrict__ rects, uint8_t* __restrict__ scratch,
                                                               const MdBlurWeights wt) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[BLUR_LDS_BYTES];
    const BlurRect d = rects[blockIdx.y];
    if ((int)blockIdx.x >= d.row_groups * d.chunks) return;              // (uniform: the whole workgroup leaves)
    const int t = threadIdx.x;
    const int g = blockIdx.x / d.chunks, k = blockIdx.x - g * d.chunks;
    const int y0 = g * d.rows;
    const int ny = min(d.rows, d.h - y0);
    MdBlurXPlan plan;
    plan.rows = d.rows, plan.stride = d.stride, plan.chunks = d.chunks, plan.step = d.step, plan.halo = d.halo;
    int o0, o1, a, b;
    md_blur_chunk(plan, d.w, k, &o0, &o1, &a, &b);
    const int n = b - a, nb = n * 3;                                     // nb <= stride, ny * stride * 2 <= BLUR_LDS_BYTES (md_blur_plan_x)
    uint8_t* A = lds;
    uint8_t* B = lds + d.rows * d.stride;
    const uint8_t* src = d.img + (long long)y0 * d.pitch + (long long)a * 3;
    for (int i = t; i < ny * nb; i += ROW_LANES) {
        const int j = i / nb, x = i - j * nb;
        A[j * d.stride + x] = src[(long long)j * d.pitch + x];
    }
    __syncthreads();
    if (t < ny * 3) {
        const int j = t / 3, c = t - j * 3;
        md_blur_line3(A + j * d.stride + c, B + j * d.stride + c, 3, n, wt);
    }
    __syncthreads();
    const int keep = (o1 - o0) * 3, skip = (o0 - a) * 3;
    uint8_t* dst = scratch + d.s0 + (long long)y0 * d.sp + (long long)o0 * 3;
    for (int i = t; i < ny * keep; i += ROW_LANES) {
        const int j = i / keep, x = i - j * keep;
        dst[(long long)j * d.sp + x] = B[j * d.stride + skip + x];
    }
}

__global__ __launch_bounds__(COLUMN_LANES) void blur_columns_kernel(const BlurRect* __restrict__ rects, uint8_t* __restrict__ scratch,
                                                                     const MdBlurWeights wt) {
    const BlurRect d = rects[blockIdx.y];
    const int t = blockIdx.x * COLUMN_LANES + threadIdx.x;
    if (t >= d.w * 3) return;
    uint8_t* s0 = scratch + d.s0 + t;
    uint8_t* s1 = scratch + d.s1 + t;
    md_blur_line(s0, d.sp, s1, d.sp, d.h, wt.r, wt.ww, wt.fw);
    md_blur_line(s1, d.sp, s0, d.sp, d.h, wt.r, wt.ww, wt.fw);
    md_blur_line(s0, d.sp, d.img + t, d.pitch, d.h, wt.r, wt.ww, wt.fw);
}

}  // namespace

hipError_t launch_blur_round(const BlurRect* rects, int n, int max_row_blocks, int max_width, uint8_t* scratch, int r, uint32_t ww,
                             uint32_t fw, hipStream_t s) {
    if (n < 1 || max_row_blocks < 1 || max_width < 1) return hipErrorInvalidValue;
    MdBlurWeights wt;
    wt.r = r, wt.ww = ww, wt.fw = fw;
    hipLaunchKernelGGL(blur_rows_kernel, dim3((unsigned)max_row_blocks, (unsigned)n), dim3(ROW_LANES), 0, s, rects, scratch, wt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned column_blocks = ((unsigned)max_width * 3 + COLUMN_LANES - 1) / COLUMN_LANES;
    hipLaunchKernelGGL(blur_columns_kernel, dim3(column_blocks, (unsigned)n), dim3(COLUMN_LANES), 0, s, rects, scratch, wt);
    return hipGetLastError();
}

}  // namespace mdhip
