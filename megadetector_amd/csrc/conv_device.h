// The device-side prelude of the conv kernel translation units (conv_igemm / conv_v2 / conv_v5 / conv_v5s / conv_v5c / conv_v6 /
// conv_v7 / conv_f8 .cpp): vector types, the buffer-descriptor constants, the LDS-DMA and scheduling macros, the storage-type
// conversions and the epilogue helpers they all use.  Nothing here is seen by the host-only units (mdhip_internal.h is).
// gfx950 (MI355X / CDNA4) only.
#pragma once

#include "mdhip_internal.h"

namespace mdhip {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float mdhip_f32x2;
typedef mdhip_f32x2 f32x2;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((address_space(3))) char lds_char;

// buffer descriptors (__builtin_amdgcn_make_buffer_rsrc): every descriptor spans kNumRecords bytes with the flags word
// kRsrcFlags; a lane whose offset is kOOB (>= every descriptor's num_records) reads zeros and stores nothing
[[maybe_unused]] constexpr unsigned kOOB = 0x80000000u;
[[maybe_unused]] constexpr int kNumRecords = 0x7fffffff;
[[maybe_unused]] constexpr int kRsrcFlags = 0x00020000;

// 16 bytes per lane, HBM/L2 -> LDS directly: LDS address = m0-base (wave-uniform) + lane*16;
// source = descriptor base + voff (per lane) + soff (wave-uniform SGPR).  A lane whose voff is
// >= num_records reads zeros: that is how conv padding, K padding and ragged tiles are done.
#define MDHIP_DMA16(rsrc, lptr, voff, soff) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds((rsrc), (lptr), 16, (voff), (soff), 0, 0)
// nothing is scheduled across this point (the lock-stepped main loops: between two MFMA chunks)
#define MDHIP_FENCE() __builtin_amdgcn_sched_barrier(0)

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// Inside the conv units MDHIP_ST is the storage type's namespace (mdhip_internal.h), frag8_t the MFMA operand type,
// MDHIP_MFMA the 16x16x32 instruction, st_pack2 / st_unpack the epilogue conversions.
#if defined(MDHIP_ST_F16)
typedef _Float16 frag8_t __attribute__((ext_vector_type(8)));
#define MDHIP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ uint32_t st_pack2(float a, float b) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = {a, b};
    const h2 r = __builtin_convertvector(v, h2);
    return *(const uint32_t*)&r;
}
__device__ __forceinline__ float st_unpack(uint16_t h) { return f16_to_f32(h); }
#else
typedef short frag8_t __attribute__((ext_vector_type(8)));
#define MDHIP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
__device__ __forceinline__ uint32_t st_pack2(float a, float b) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = {a, b};
    const b2 r = __builtin_convertvector(v, b2);
    return *(const uint32_t*)&r;
}
__device__ __forceinline__ float st_unpack(uint16_t h) { return bf16_to_f32(h); }
#endif
// four fp32 values -> four e4m3 bytes (RNE, saturating at +-448): the out_f8 epilogue of the 16-bit kernels
__device__ __forceinline__ uint32_t pack_e4m3x4(float a, float b, float c, float d, float qscale) {
    a = __builtin_fminf(__builtin_fmaxf(a * qscale, -448.0f), 448.0f);
    b = __builtin_fminf(__builtin_fmaxf(b * qscale, -448.0f), 448.0f);
    c = __builtin_fminf(__builtin_fmaxf(c * qscale, -448.0f), 448.0f);
    d = __builtin_fminf(__builtin_fmaxf(d * qscale, -448.0f), 448.0f);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (uint32_t)r;
}
// a fragment that is not read from LDS (ablation variants of the kernels only)
__device__ __forceinline__ frag8_t frag_dummy(int v) {
    frag8_t z;
#pragma unroll
    for (int k = 0; k < 8; ++k) z[k] = (__typeof__(z[0]))(v + k);
    asm volatile("" : "+v"(z));
    return z;
}

// m / d for 0 <= m < 2^31, d >= 1, rcp = floor(2^32 / d): the estimate mulhi(m, rcp) is the quotient or one below it
// (m * (2^32 / d - rcp) / 2^32 < 1), one compare fixes it -- 5 instructions instead of the ~30 of a run-time division
__device__ __forceinline__ int conv_udiv(int m, int d, unsigned rcp) {
    unsigned q = __umulhi((unsigned)m, rcp);
    const unsigned r = (unsigned)m - q * (unsigned)d;
    return (int)(r >= (unsigned)d ? q + 1u : q);
}
// SiLU = x * sigmoid(x): v_mul, v_exp, v_add, v_rcp, v_mul (each <= 1 ulp: far inside the 16-bit rounding that follows).
// The scalar form, for conv_f8.cpp's epilogue; every other epilogue takes two values at a time:
__device__ __forceinline__ float silu_f32(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
// SiLU of two values at a time: the same operations and roundings as the scalar  x * rcp(1 + exp(-x))  of every kernel
// family (x * -log2(e), v_exp_f32, 1 + e, v_rcp_f32, x * r), with the four full-rate ones as packed fp32 instructions.
// The two transcendentals are quarter rate: for 1x1 convs with K <= 640 the activation is more VALU time than the
// layer's MFMAs are matrix time, so the epilogues are written around it.  (neg_log2e: -0x1.715476p+0f, passed in so that
// register-tight kernels can keep it out of the main loop.)
constexpr float kNegLog2e = -0x1.715476p+0f;
__device__ __forceinline__ mdhip_f32x2 silu_f32x2(mdhip_f32x2 x, float neg_log2e = kNegLog2e) {
    const mdhip_f32x2 u = x * mdhip_f32x2{neg_log2e, neg_log2e};
    const mdhip_f32x2 e = mdhip_f32x2{__builtin_amdgcn_exp2f(u[0]), __builtin_amdgcn_exp2f(u[1])} + mdhip_f32x2{1.0f, 1.0f};
    return x * mdhip_f32x2{__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
}
// v[0..3] = a[0..3] + b[0..3] (packed), the first half of every epilogue; the activation follows under one uniform branch
// per pixel row (mdhip_silu4), not as a select per value
template <typename A, typename B>
__device__ __forceinline__ void mdhip_bias4(const A& a, const B& b, float (&v)[4]) {
    const mdhip_f32x2 t0 = mdhip_f32x2{a[0], a[1]} + mdhip_f32x2{b[0], b[1]};
    const mdhip_f32x2 t1 = mdhip_f32x2{a[2], a[3]} + mdhip_f32x2{b[2], b[3]};
    v[0] = t0[0]; v[1] = t0[1]; v[2] = t1[0]; v[3] = t1[1];
}
__device__ __forceinline__ void mdhip_silu4(float (&v)[4], float neg_log2e = kNegLog2e) {
    const mdhip_f32x2 t0 = silu_f32x2(mdhip_f32x2{v[0], v[1]}, neg_log2e), t1 = silu_f32x2(mdhip_f32x2{v[2], v[3]}, neg_log2e);
    v[0] = t0[0]; v[1] = t0[1]; v[2] = t1[0]; v[3] = t1[1];
}
// The 16-byte store exchange of the 16-bit epilogues: a lane's values of two neighbouring fragment columns (four consecutive
// channels each, 16 channels apart) -> 8 consecutive channels of its pixel.  The pairs are exchanged across the four
// 16-lane rows of the wave (v_permlane32_swap, v_permlane16_swap): row q then holds channels q*8 .. q*8+7 of the pair's
// 32, and one store covers 64 contiguous bytes per pixel instead of 32.
// Used where the unit's gfx950 code is the same with it as written out: conv_igemm, conv_v5, conv_v5s, conv_v6, conv_v7.
// conv_v2.cpp and conv_f8.cpp keep it written out (through the helper their epilogues are scheduled differently);
// so do the inverse exchange of the residual (conv_v5.cpp, conv_v5s.cpp) and the persistent-stream tile assignment of
// every unit, which as functions moved registers and instruction order in conv_v5s.cpp.
__device__ __forceinline__ u32x4 conv_pack_pair(const float (&va)[4], const float (&vb)[4]) {
    const unsigned a0 = st_pack2(va[0], va[1]), a1 = st_pack2(va[2], va[3]);
    const unsigned b0 = st_pack2(vb[0], vb[1]), b1 = st_pack2(vb[2], vb[3]);
    const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
    const auto t0 = __builtin_amdgcn_permlane16_swap(s0[0], s0[1], false, false);
    const auto t1 = __builtin_amdgcn_permlane16_swap(s1[0], s1[1], false, false);
    return u32x4{t0[0], t1[0], t0[1], t1[1]};
}
// Detect decode in a conv epilogue (mdhip_decode_box, mdhip_internal.h): a lane's four consecutive logits (channels
// n .. n + 3 of output pixel m, n a multiple of 4, 8 outputs per anchor) -> its half of the prediction row of anchor n / 8:
// the box (n mod 8 == 0) or objectness + classes (n mod 8 == 4)
__device__ __forceinline__ void mdhip_decode_store(const ConvArgs& p, int m, int n, const float (&v)[4]) {
#pragma clang fp contract(off)
    const int b = conv_udiv(m, p.HoWo, p.rcp_howo);
    const int rem = m - b * p.HoWo;
    const int y = conv_udiv(rem, p.Wo, p.rcp_wo);
    const int x = rem - y * p.Wo;
    const int a = n >> 3;
    const int idx = p.dec_level_off + (a * p.Ho + y) * p.Wo + x;
    float* o = p.dec_pred + ((size_t)b * p.dec_n_anchors + idx) * 8 + (n & 4);
    float4 r;
    if ((n & 4) == 0) mdhip_decode_box(v[0], v[1], v[2], v[3], x, y, p.dec_stride, p.dec_anchors[a * 2 + 0], p.dec_anchors[a * 2 + 1], r.x, r.y, r.z, r.w);
    else r = make_float4(mdhip_sigmoid_exact(v[0]), mdhip_sigmoid_exact(v[1]), mdhip_sigmoid_exact(v[2]), mdhip_sigmoid_exact(v[3]));
    *(float4*)o = r;
}
#endif

}  // namespace mdhip
