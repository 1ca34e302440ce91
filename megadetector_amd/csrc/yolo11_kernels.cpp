// Device work of the anchor-free YOLO11 models (MDv1000-larch / -sorrel) that the conv kernels do not cover:
//   * depthwise 3x3 convolution (DWConv of the Detect class branch, Attention.pe of C2PSA), NHWC, 16-bit storage;
//   * the spatial self-attention of C2PSA: one flash-style wavefront per (image, head, 16 queries);
//   * the DFL box decode of the anchor-free Detect head.
// Restated from the published architecture (ultralytics 8.3.x, [3P]); the CPU restatement is tests/yolo11_ref.py.

#include "mdhip_internal.h"

#include <cmath>

namespace mdhip {

namespace {

template <bool F16> struct St;
template <> struct St<false> {
    typedef short frag8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float load(uint16_t h) { return bf16_to_f32(h); }
    static __device__ __forceinline__ uint16_t store(float f) { return f32_to_bf16(f); }
    static __device__ __forceinline__ short elem(float f) { return (short)f32_to_bf16(f); }
    static __device__ __forceinline__ frag8 bits(const uint4& u) { return *(const frag8*)&u; }
    static __device__ __forceinline__ __attribute__((ext_vector_type(4))) float mfma(frag8 a, frag8 b, __attribute__((ext_vector_type(4))) float c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct St<true> {
    typedef _Float16 frag8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float load(uint16_t h) { return f16_to_f32(h); }
    static __device__ __forceinline__ uint16_t store(float f) { return f32_to_f16(f); }
    static __device__ __forceinline__ _Float16 elem(float f) { return (_Float16)f; }
    static __device__ __forceinline__ frag8 bits(const uint4& u) { return *(const frag8*)&u; }
    static __device__ __forceinline__ __attribute__((ext_vector_type(4))) float mfma(frag8 a, frag8 b, __attribute__((ext_vector_type(4))) float c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
typedef __attribute__((ext_vector_type(4))) float f32x4;

// ---------------------------------------------------------------------------------------------------------------------
// depthwise 3x3, stride 1, pad 1.  One thread = 8 channels (one 16-byte load per tap) of one output pixel; the channel
// group is the fastest index, so a wavefront reads 64 x 16 contiguous bytes per tap.  Output channel o reads input
// channel (o / grp) * grp_stride + grp_off + o % grp (grp = C: plain; Attention.pe: the v slices of the qkv tensor).
// fp32 accumulation in tap order, + bias, optional SiLU, optional add of `res` (after the activation), one rounding.
// ---------------------------------------------------------------------------------------------------------------------
template <bool F16>
__global__ void __launch_bounds__(256)
dwconv3x3_kernel(const uint16_t* __restrict__ in, int ld_in, const uint16_t* __restrict__ wgt /*[9][C]*/,
                 const float* __restrict__ bias, uint16_t* out, int ld_out, const uint16_t* res, int ld_res,
                 int n, int H, int W, int C, int grp, int grp_stride, int grp_off, int act) {
    const int C8 = C >> 3;
    const long long total = (long long)n * H * W * C8;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cg = (int)(t % C8);
    const long long pix = t / C8;
    const int x = (int)(pix % W);
    const int y = (int)((pix / W) % H);
    const long long img = pix / ((long long)W * H);
    const int o0 = cg * 8;
    const int ci0 = (o0 / grp) * grp_stride + grp_off + (o0 % grp);
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int yy = y + r - 1;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int xx = x + s - 1;
            if (xx < 0 || xx >= W) continue;
            const uint4 v = *(const uint4*)(in + ((img * H + yy) * W + xx) * (long long)ld_in + ci0);
            const uint4 wv = *(const uint4*)(wgt + (size_t)(r * 3 + s) * C + o0);
            const uint16_t* vh = (const uint16_t*)&v;
            const uint16_t* wh = (const uint16_t*)&wv;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += St<F16>::load(vh[k]) * St<F16>::load(wh[k]);
        }
    }
    uint4 o;
    uint16_t* oh = (uint16_t*)&o;
    uint4 rv = make_uint4(0, 0, 0, 0);
    if (res) rv = *(const uint4*)(res + pix * (long long)ld_res + o0);
    const uint16_t* rh = (const uint16_t*)&rv;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float v = acc[k] + bias[o0 + k];
        if (act) v = v * (1.0f / (1.0f + __expf(-v)));
        if (res) v = St<F16>::load(rh[k]) + v;
        oh[k] = St<F16>::store(v);
    }
    *(uint4*)(out + pix * (long long)ld_out + o0) = o;
}

// ---------------------------------------------------------------------------------------------------------------------
// C2PSA attention, one wavefront per (16 queries, head, image).  Per head the qkv tensor holds [q 32 | k 32 | v 64]
// channels at head * 128 (read in place, pixel pitch ld_qkv).  Scores are computed transposed, S^T = K Q^T
// (mfma_f32_16x16x32: A = 16 keys x 32 key channels, B = 32 key channels x 16 queries, key_dim 32 = one K step), so
// that lane l holds scores of query l & 15 -- the online softmax (fp32) reduces over the 4 lanes l & 15 + 16 g only.
// 32 keys per step: two score MFMAs; lane l (g = l >> 4) holds keys 4g .. 4g+3 and 16+4g .. 16+4g+3, which is the
// K order of the P V product's A operand (P rows = queries, P in 16 bits); V is staged through LDS and read in the same
// key order for the B operand.  Keys past N score -inf; queries past N are computed on zeros and not stored.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kAttnKd = 32, kAttnHd = 64, kAttnHeadCh = 2 * kAttnKd + kAttnHd;

template <bool F16>
__global__ void __launch_bounds__(64)
attn_kernel(const uint16_t* __restrict__ qkv, int ld_qkv, uint16_t* __restrict__ out, int ld_out, int N, float scale) {
    typedef typename St<F16>::frag8 frag8;
    __shared__ uint16_t vs[32][kAttnHd + 8];
    const int lane = threadIdx.x;
    const int g = lane >> 4, c16 = lane & 15;
    const int q0 = blockIdx.x * 16, head = blockIdx.y;
    const long long img = blockIdx.z;
    const uint16_t* base = qkv + img * (long long)N * ld_qkv + head * kAttnHeadCh;
    // B operand of S^T: Q^T[k = key channel 8g + j][col = query c16]
    uint4 qraw = make_uint4(0, 0, 0, 0);
    if (q0 + c16 < N) qraw = *(const uint4*)(base + (long long)(q0 + c16) * ld_qkv + 8 * g);
    const frag8 qf = St<F16>::bits(qraw);
    float m = -INFINITY, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) o[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < N; k0 += 32) {
        // stage V of keys k0 .. k0+31 (64 channels): 256 16-byte chunks, 4 per lane
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int chunk = it * 64 + lane;
            const int key = chunk >> 3, cc = (chunk & 7) * 8;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (k0 + key < N) v = *(const uint4*)(base + (long long)(k0 + key) * ld_qkv + 2 * kAttnKd + cc);
            *(uint4*)&vs[key][cc] = v;
        }
        // S^T for keys k0 + 16 h + (0..15): A = K[row = key c16][k = 8g + j]
        f32x4 s[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int key = k0 + 16 * h + c16;
            uint4 kraw = make_uint4(0, 0, 0, 0);
            if (key < N) kraw = *(const uint4*)(base + (long long)key * ld_qkv + kAttnKd + 8 * g);
            s[h] = St<F16>::mfma(St<F16>::bits(kraw), qf, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        // lane: query q0 + c16; p[j] = key k0 + 4g + j (j < 4), k0 + 16 + 4g + j - 4 (j >= 4)
        float p[8];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = k0 + (j < 4 ? 4 * g + j : 16 + 4 * g + j - 4);
            const float v = (key < N) ? s[j >> 2][j & 3] * scale : -INFINITY;
            p[j] = v;
            mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m, mx);
        const float alpha = __expf(m - m_new);
        float rs = 0.f;
        frag8 pa;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = __expf(p[j] - m_new);
            rs += e;
            pa[j] = St<F16>::elem(e);
        }
        rs += __shfl_xor(rs, 16);
        rs += __shfl_xor(rs, 32);
        l = l * alpha + rs;
        m = m_new;
        // O rows (queries 4g + r) rescale by the factor of their query (held by lane 4g + r)
        float ar[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * g + r);
        __syncthreads();
        // P V: A = P[row = query c16][k = 8g + j], B = V^T[k = 8g + j][col = channel 16 cb + c16], same key order
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            frag8 vb;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = j < 4 ? 4 * g + j : 16 + 4 * g + j - 4;
                const uint16_t hv = vs[key][16 * cb + c16];
                vb[j] = *(const __typeof__(vb[0])*)&hv;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) o[cb][r] *= ar[r];
            o[cb] = St<F16>::mfma(pa, vb, o[cb]);
        }
    }
    // O[query 4g + r][channel 16 cb + c16] / l(query)
    float lr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) lr[r] = __shfl(l, 4 * g + r);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int q = q0 + 4 * g + r;
        if (q >= N) continue;
        uint16_t* orow = out + (img * N + q) * (long long)ld_out + head * kAttnHd;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) orow[16 * cb + c16] = St<F16>::store(o[cb][r] / lr[r]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// DFL decode of one level (ultralytics Detect._inference, [3P]): per anchor, for each of the 4 sides a softmax over 16
// bins and its expectation; anchor point (x + 0.5, y + 0.5); x1y1 = p - lt, x2y2 = p + rb; cxcy = (x1y1 + x2y2) / 2,
// wh = x2y2 - x1y1, times the stride; class scores = sigmoid.  exp is evaluated in double and rounded once to fp32 (the
// CPU restatement does the same), sums run in bin order, no contraction: the same bits as tests/yolo11_ref.py.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float exp_r(float x) { return (float)exp((double)x); }

__global__ void __launch_bounds__(256)
dfl_decode_kernel(const float* __restrict__ box, int ld_box, const float* __restrict__ cls, int ld_cls, float* __restrict__ pred,
                  int n, int ny, int nx, int nc, int n_anchors, int level_off, float stride) {
#pragma clang fp contract(off)
    const int per_img = ny * nx;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n * per_img) return;
    const int b = (int)(t / per_img), a = (int)(t % per_img);
    const int y = a / nx, x = a % nx;
    const float* bl = box + t * ld_box;
    float d[4];
    for (int side = 0; side < 4; ++side) {
        const float* v = bl + side * 16;
        float mx = v[0];
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, v[i]);
        float e[16];
        float sum = 0.f;
        for (int i = 0; i < 16; ++i) { e[i] = exp_r(v[i] - mx); sum = sum + e[i]; }
        float acc = 0.f;
        for (int i = 0; i < 16; ++i) acc = acc + (e[i] / sum) * (float)i;
        d[side] = acc;
    }
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float x1 = px - d[0], y1 = py - d[1], x2 = px + d[2], y2 = py + d[3];
    float* o = pred + ((size_t)b * n_anchors + level_off + a) * (4 + nc);
    o[0] = ((x1 + x2) / 2.0f) * stride;
    o[1] = ((y1 + y2) / 2.0f) * stride;
    o[2] = (x2 - x1) * stride;
    o[3] = (y2 - y1) * stride;
    const float* cl = cls + t * ld_cls;
    for (int k = 0; k < nc; ++k) o[4 + k] = 1.0f / (1.0f + exp_r(-cl[k]));
}

}  // namespace

hipError_t launch_dwconv3x3(const uint16_t* in, int ld_in, const uint16_t* wgt, const float* bias, uint16_t* out, int ld_out,
                            const uint16_t* res, int ld_res, int n, int H, int W, int C, int grp, int grp_stride, int grp_off,
                            int act, int f16, hipStream_t s) {
    if (C % 8 || grp % 8 || grp_off % 8 || grp_stride % 8 || ld_in % 8 || ld_out % 8 || (res && ld_res % 8) || n < 1 || H < 1 || W < 1)
        return hipErrorInvalidValue;
    const long long total = (long long)n * H * W * (C / 8);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (f16)
        hipLaunchKernelGGL(dwconv3x3_kernel<true>, dim3(blocks), dim3(256), 0, s, in, ld_in, wgt, bias, out, ld_out, res, ld_res,
                           n, H, W, C, grp, grp_stride, grp_off, act);
    else
        hipLaunchKernelGGL(dwconv3x3_kernel<false>, dim3(blocks), dim3(256), 0, s, in, ld_in, wgt, bias, out, ld_out, res, ld_res,
                           n, H, W, C, grp, grp_stride, grp_off, act);
    return hipGetLastError();
}

hipError_t launch_attention(const uint16_t* qkv, int ld_qkv, uint16_t* out, int ld_out, int n, int N, int heads, int f16,
                            hipStream_t s) {
    if (ld_qkv < heads * kAttnHeadCh || ld_qkv % 8 || ld_out < heads * kAttnHd || n < 1 || N < 1 || heads < 1)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + 15) / 16), (unsigned)heads, (unsigned)n);
    const float scale = 0.17677669529663687f;          // key_dim ** -0.5, key_dim = 32 (rounded to fp32 as torch does)
    if (f16)
        hipLaunchKernelGGL(attn_kernel<true>, grid, dim3(64), 0, s, qkv, ld_qkv, out, ld_out, N, scale);
    else
        hipLaunchKernelGGL(attn_kernel<false>, grid, dim3(64), 0, s, qkv, ld_qkv, out, ld_out, N, scale);
    return hipGetLastError();
}

hipError_t launch_dfl_decode(const float* box, int ld_box, const float* cls, int ld_cls, float* pred, int n, int ny, int nx,
                             int nc, int n_anchors, int level_off, float stride, hipStream_t s) {
    if (ld_box < 64 || ld_cls < nc || nc < 1 || n < 1 || ny < 1 || nx < 1) return hipErrorInvalidValue;
    const long long total = (long long)n * ny * nx;
    hipLaunchKernelGGL(dfl_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, box, ld_box, cls, ld_cls, pred,
                       n, ny, nx, nc, n_anchors, level_off, stride);
    return hipGetLastError();
}

}  // namespace mdhip
