// mdhip_gray_count: the gray pixels (R == G and R == B) inside a rectangle of each of n device images, in ONE launch.
// The statement and the walk of a row are csrc/gray_count.h's, which the host model compiles too.
//
// The work of an image is its window's rows x gc_groups(width) groups of four pixels, numbered row by row; workgroup
// blockIdx.x of image blockIdx.y takes the groups blockIdx.x * 256 + lane, then strides by the grid, so consecutive lanes read
// consecutive 12-byte groups (768 bytes a wave instruction) and an image of any size is covered by a grid sized for the
// largest.  Lane counts (at most 4 a group) -> the sum of a wave by shuffles -> the four wave sums through LDS -> ONE 64-bit
// atomicAdd a workgroup into the image's counter, which the entry point zeroes on the stream before the launch.  Integer sums:
// the result does not depend on the order in which workgroups arrive.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mdhip_internal.h"
#include "gray_count.h"

namespace mdhip {

namespace {

__global__ __launch_bounds__(256) void gray_count_kernel(const GrayWindow* __restrict__ windows) {
    __shared__ uint32_t wave_sum[4];
    const GrayWindow d = windows[blockIdx.y];
    const uint32_t groups = gc_groups(d.w), total = groups * (uint32_t)d.h;      // < 2^30: 16384 groups x 65535 rows
    uint32_t n = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t row = i / groups;
        n += gc_count_group(d.origin + (long long)row * d.pitch, d.w, i - row * groups);
    }
    for (int step = 32; step > 0; step >>= 1) n += __shfl_down(n, step, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (unsigned long long)wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        if (sum) atomicAdd(d.count, sum);
    }
}

}  // namespace

hipError_t launch_gray_count(const GrayWindow* windows, int n, long long max_groups, hipStream_t s) {
    if (n < 1) return hipSuccess;
    // four groups a lane where the largest window has them; at most 1024 workgroups an image
    const long long blocks = std::min<long long>(std::max<long long>((max_groups + 1023) / 1024, 1), 1024);
    hipLaunchKernelGGL(gray_count_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, windows);
    return hipGetLastError();
}

}  // namespace mdhip
