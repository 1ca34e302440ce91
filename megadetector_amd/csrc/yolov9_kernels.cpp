// Device work of the YOLOv9-C model (MDv1000-cedar) that the conv kernels do not cover, NHWC, 16-bit storage:
//   * the two pools of ADown: avg_pool2d(2, stride 1) of the input, then a channel split -- the first half feeds a
//     3x3 / s2 / p1 conv, the second half max_pool2d(3, 2, 1) and a 1x1 conv;
//   * CBFuse of the auxiliary branch: nearest-upsampled slices of CBLinear outputs added to a tensor.
// Both are memory-bound: one thread handles 8 channels (one 16-byte access) of one output pixel, the channel group is the
// fastest index.  Restated from the published architecture (WongKinYiu YOLOv9, [3P]); the CPU restatement is
// tests/yolov9_ref.py, which pins both kernels bit for bit.  Compiled without FMA contraction: the sums below are the
// documented ones.

#include "mdhip_internal.h"

namespace mdhip {

namespace {

template <bool F16> struct V9 {
    static __device__ __forceinline__ float ld(uint16_t h) { return F16 ? f16_to_f32(h) : bf16_to_f32(h); }
    static __device__ __forceinline__ uint16_t st(float f) { return F16 ? f32_to_f16(f) : f32_to_bf16(f); }
};

__device__ __forceinline__ void unpack8(const uint4& u, uint16_t (&h)[8]) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[2 * k] = (uint16_t)(w[k] & 0xffffu);
        h[2 * k + 1] = (uint16_t)(w[k] >> 16);
    }
}
__device__ __forceinline__ uint4 pack8(const uint16_t (&h)[8]) {
    return make_uint4((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16),
                      (uint32_t)h[4] | ((uint32_t)h[5] << 16), (uint32_t)h[6] | ((uint32_t)h[7] << 16));
}

// the 2x2 / stride-1 average at (y, x) of 8 channels, valid for y < H - 1, x < W - 1: ((a + b) + c) + d in fp32 over the
// window in row order, times 1/4 (exact: the same value as torch's sum / 4), rounded once to the storage type
template <bool F16>
__device__ __forceinline__ void avg2x2(const uint16_t* __restrict__ p, int ld, int W, uint16_t (&r)[8]) {
    uint16_t a[8], b[8], c[8], d[8];
    unpack8(*(const uint4*)p, a);
    unpack8(*(const uint4*)(p + ld), b);
    unpack8(*(const uint4*)(p + (size_t)W * ld), c);
    unpack8(*(const uint4*)(p + (size_t)W * ld + ld), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float s = ((V9<F16>::ld(a[k]) + V9<F16>::ld(b[k])) + V9<F16>::ld(c[k])) + V9<F16>::ld(d[k]);
        r[k] = V9<F16>::st(s * 0.25f);
    }
}

// ADown pools.  Items [0, na): (pixel y, x of H x W, group of the FIRST half) -> A[y][x] = avg2x2, zero in the last row
// and column (a 3x3 / s2 / p1 conv over this H x W buffer equals the conv over the (H-1) x (W-1) average: the taps that
// reach row / column H-1 read the zero padding either way).  Items [na, na + nb): (pixel oy, ox of H/2 x W/2, group of
// the SECOND half) -> B[oy][ox] = max over the 3x3 / s2 / p1 window, clipped to the (H-1) x (W-1) extent, of the rounded
// averages (torch's max_pool2d pads with -inf: the clipped max is the same).
template <bool F16>
__global__ __launch_bounds__(256) void adown_pool_kernel(const uint16_t* __restrict__ in, int ld_in, uint16_t* __restrict__ A, int ld_a,
                                                         uint16_t* __restrict__ B, int ld_b, int n, int H, int W, int half) {
    const int G = half >> 3;
    const long long na = (long long)n * H * W * G;
    const int Ho = H >> 1, Wo = W >> 1;
    const long long nb = (long long)n * Ho * Wo * G;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na + nb) return;
    if (i < na) {
        const int g = (int)(i % G);
        long long px = i / G;
        const int x = (int)(px % W);
        px /= W;
        const int y = (int)(px % H);
        const int b = (int)(px / H);
        uint16_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (y < H - 1 && x < W - 1)
            avg2x2<F16>(in + (((size_t)b * H + y) * W + x) * ld_in + g * 8, ld_in, W, r);
        *(uint4*)(A + (((size_t)b * H + y) * W + x) * ld_a + g * 8) = pack8(r);
        return;
    }
    i -= na;
    const int g = (int)(i % G);
    long long px = i / G;
    const int ox = (int)(px % Wo);
    px /= Wo;
    const int oy = (int)(px % Ho);
    const int b = (int)(px / Ho);
    const int y0 = max(2 * oy - 1, 0), y1 = min(2 * oy + 1, H - 2);
    const int x0 = max(2 * ox - 1, 0), x1 = min(2 * ox + 1, W - 2);
    float m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = -INFINITY;
    const uint16_t* base = in + (size_t)b * H * W * ld_in + half + g * 8;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            uint16_t r[8];
            avg2x2<F16>(base + ((size_t)y * W + x) * ld_in, ld_in, W, r);
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], V9<F16>::ld(r[k]));
        }
    uint16_t o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = V9<F16>::st(m[k]);        // a stored value: exact
    *(uint4*)(B + (((size_t)b * Ho + oy) * Wo + ox) * ld_b + g * 8) = pack8(o);
}

// CBFuse: out[y][x] = round( ((up(s0) + up(s1)) + up(s2)) + last ) in fp32 -- the sources in the order of CBFuse's
// inputs, the tensor of its last input added last (the order torch.stack(res + xs[-1:]) lists them in) -- with up(s_k)
// the nearest resize of source k by its integer factor f_k: pixel (y / f_k, x / f_k).
template <bool F16>
__global__ __launch_bounds__(256) void cbfuse_kernel(const CbfuseArgs a) {
    const int G = a.C >> 3;
    const long long total = (long long)a.n * a.H * a.W * G;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int g = (int)(i % G);
    long long px = i / G;
    const int x = (int)(px % a.W);
    px /= a.W;
    const int y = (int)(px % a.H);
    const int b = (int)(px / a.H);
    float acc[8];
    for (int s = 0; s < a.n_src; ++s) {
        const int f = a.factor[s];
        const int hs = a.H / f, ws = a.W / f;
        uint16_t v[8];
        unpack8(*(const uint4*)(a.src[s] + (((size_t)b * hs + y / f) * ws + x / f) * a.ld_src[s] + g * 8), v);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = s == 0 ? V9<F16>::ld(v[k]) : acc[k] + V9<F16>::ld(v[k]);
    }
    uint16_t l[8], o[8];
    unpack8(*(const uint4*)(a.last + (((size_t)b * a.H + y) * a.W + x) * a.ld_last + g * 8), l);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = V9<F16>::st(acc[k] + V9<F16>::ld(l[k]));
    *(uint4*)(a.out + (((size_t)b * a.H + y) * a.W + x) * a.ld_out + g * 8) = pack8(o);
}

}  // namespace

hipError_t launch_adown_pool(const uint16_t* in, int ld_in, uint16_t* A, int ld_a, uint16_t* B, int ld_b, int n, int H, int W,
                             int c_in, int f16, hipStream_t s) {
    const int half = c_in / 2;
    if (c_in % 16 || ld_in % 8 || ld_a % 8 || ld_b % 8 || ld_in < c_in || ld_a < half || ld_b < half || n < 1 || H < 2 || W < 2 ||
        (H % 2) || (W % 2))
        return hipErrorInvalidValue;
    const long long total = (long long)n * H * W * (half / 8) + (long long)n * (H / 2) * (W / 2) * (half / 8);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (f16)
        hipLaunchKernelGGL(adown_pool_kernel<true>, dim3(blocks), dim3(256), 0, s, in, ld_in, A, ld_a, B, ld_b, n, H, W, half);
    else
        hipLaunchKernelGGL(adown_pool_kernel<false>, dim3(blocks), dim3(256), 0, s, in, ld_in, A, ld_a, B, ld_b, n, H, W, half);
    return hipGetLastError();
}

hipError_t launch_cbfuse(const CbfuseArgs& a, int f16, hipStream_t s) {
    if (a.C % 8 || a.ld_out % 8 || a.ld_last % 8 || a.n_src < 1 || a.n_src > 3 || a.n < 1 || a.H < 1 || a.W < 1)
        return hipErrorInvalidValue;
    for (int k = 0; k < a.n_src; ++k)
        if (a.ld_src[k] % 8 || a.factor[k] < 1 || a.H % a.factor[k] || a.W % a.factor[k]) return hipErrorInvalidValue;
    const long long total = (long long)a.n * a.H * a.W * (a.C / 8);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (f16)
        hipLaunchKernelGGL(cbfuse_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(cbfuse_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdhip
