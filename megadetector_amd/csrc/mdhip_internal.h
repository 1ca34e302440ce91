// Internal declarations shared by the kernel translation units and the C-ABI layer.
// gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

struct MdClassifyCrop;             // resample.h: the record of a crop of mdhip_classifier_input

struct ChgWeights;                 // change_detect.h: the blur's taps
struct MdjImage;
struct MdjEncCrop;
struct MdjEncTables;
struct MdjKeepRect;

namespace mdhip {

// ---------------------------------------------------------------------------------------
// storage-type helpers.  Activations and packed weights are 16-bit: bf16 (the configuration BASELINE.json
// names) or fp16 (same MFMA rate, 3 more mantissa bits; MDHIP_DTYPE_FP16).  Accumulation is fp32 either way.
// ---------------------------------------------------------------------------------------
__host__ __device__ inline uint16_t f32_to_bf16(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    uint32_t u = v.u;
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                            // RNE
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf16_to_f32(uint16_t h) {
    union { float f; uint32_t u; } v;
    v.u = ((uint32_t)h) << 16;
    return v.f;
}
__host__ __device__ inline uint16_t f32_to_f16(float f) {
    union { _Float16 h; uint16_t u; } v;
    v.h = (_Float16)f;                                                          // RNE, overflow -> inf
    return v.u;
}
__host__ __device__ inline float f16_to_f32(uint16_t h) {
    union { _Float16 h; uint16_t u; } v;
    v.u = h;
    return (float)v.h;
}
// OCP e4m3 (fn): round to nearest even, saturating at +-448 (the hardware conversion used by the kernels is fed
// clamped values, so both agree); NaN -> 0x7f
__host__ __device__ inline uint8_t f32_to_e4m3(float f) {
    union { float f; uint32_t u; } v;
    v.f = f;
    const uint32_t sign = (v.u >> 24) & 0x80u;
    uint32_t a = v.u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint8_t)(sign | 0x7f);
    if (a >= 0x43e00000u) return (uint8_t)(sign | 0x7e);            // >= 448 (incl. inf): saturate
    if (a < 0x3a800000u) {                                          // < 2^-10: below half of the smallest subnormal 2^-9
        return (uint8_t)sign;                                       // (2^-10 itself is a tie to even = 0)
    }
    const int e = (int)(a >> 23) - 127;                             // unbiased exponent, -10 .. 8
    if (e < -6) {                                                   // subnormal range: quantum 2^-9
        v.u = a;
        const float q = v.f * 512.0f;                               // exact
        // round to nearest even integer in [0, 8]
        const float r = q + 12582912.0f;                            // 1.5 * 2^23: the add rounds to an integer, RNE
        union { float f; uint32_t u; } w;
        w.f = r;
        const uint32_t m = w.u & 0xfu;                              // 0 .. 8 (8 = the smallest normal 2^-6)
        return (uint8_t)(sign | m);
    }
    uint32_t mant = a & 0x7fffffu;
    uint32_t keep = mant >> 20, rest = mant & 0xfffffu;
    uint32_t out = ((uint32_t)(e + 7) << 3) | keep;
    if (rest > 0x80000u || (rest == 0x80000u && (keep & 1u))) ++out;   // RNE; a carry moves into the exponent
    if (out > 0x7eu) out = 0x7eu;
    return (uint8_t)(sign | out);
}
__host__ __device__ inline float e4m3_to_f32(uint8_t h) {
    const uint32_t s = h >> 7, e = (h >> 3) & 15u, m = h & 7u;
    union { float f; uint32_t u; } v;
    if (e == 15u && m == 7u) { v.u = 0x7fc00000u; return v.f; }
    float f;
    if (e == 0u) f = (float)m * (1.0f / 512.0f);
    else { v.u = ((e + 120u) << 23) | (m << 20); f = v.f; }
    return s ? -f : f;
}
__host__ __device__ inline uint16_t f32_to_st(float f, int f16) { return f16 ? f32_to_f16(f) : f32_to_bf16(f); }
__host__ __device__ inline float st_to_f32(uint16_t h, int f16) { return f16 ? f16_to_f32(h) : bf16_to_f32(h); }

// The convolution translation units are compiled twice: as is (bf16, namespace mdhip::st_bf16) and with
// -DMDHIP_ST_F16 (fp16, namespace mdhip::st_f16).  Inside them MDHIP_ST is that namespace; conv_device.h holds what
// their kernels share.
#if defined(MDHIP_ST_F16)
#define MDHIP_ST st_f16
#define MDHIP_ST_LABEL "fp16"
#else
#define MDHIP_ST st_bf16
#define MDHIP_ST_LABEL "bf16"
#endif

// ---------------------------------------------------------------------------------------
// implicit-GEMM convolution (conv_igemm.cpp)
// ---------------------------------------------------------------------------------------
struct ConvArgs {
    const uint16_t* in;     // NHWC bf16 view: channel 0 of this conv's input, pixel stride ld_in
    const uint16_t* wgt;    // packed [n_rows][k_pad] bf16, k = (r*kw + s)*C_in_pad + c
    const float*    bias;   // [n_rows] fp32 (zero padded)
    void*           out;    // bf16 (or fp32 when out_f32) view, pixel stride ld_out
    const uint16_t* res;    // residual view (added after the activation) or nullptr
    const uint16_t* zero;   // >= 16 bytes of zeros: source of every padded / out-of-range chunk
    int ld_in, ld_out, ld_res;
    int H, W, C8;           // input spatial size, C_in_pad / 8
    int Ho, Wo, HoWo;
    int M, N, n_rows;       // GEMM rows (= batch*Ho*Wo), real out channels, packed rows (mult of 16)
    int k_pad;              // multiple of 64
    int ntaps, kw;
    int stride, pad;
    int act;                // 1 = SiLU
    int out_f32;            // 1 = fp32 output, no rounding (Detect logits)
    int tiles_n, tiles_m, tiles_per_xcd, m_streams;   // filled by the launch function of the kernel family
    // second packing (introduced by the row-patch kernel of round 1; read by conv_v5 / conv_v5s / conv_v5c / conv_v7 / conv_f8): weights packed [n_rows][groups*9*64], k = (cg, r, s, c % 64)
    const uint16_t* wgt4;   // nullptr when the op has no such packing
    int k_pad4, groups;
    // conv_v5.cpp, layers whose last channel group is at most half full (C_in mod 64 in 8 .. 32: the 160- and 480-channel
    // bottlenecks): the same packing with the last group's taps PAIRED -- per kernel row r one slab [ tap (r,0) ch 0..31 |
    // tap (r,1) ch 0..31 ] and one slab [ tap (r,2) ch 0..31 | zeros ], 6 slabs instead of 9 -- so that the group takes two
    // steps per kernel row instead of three half-empty ones (same MFMA chain per accumulator: same bits).  nullptr = none.
    const uint16_t* wgt4p;
    int k_pad4p;
    // fp8 path (conv_f8.cpp; MDHIP_DTYPE_FP8): the input view holds e4m3 bytes (ld_in, C8 then count BYTES and
    // 16-byte chunks = 16 channels), weights packed [n_rows][groups8*9*128] e4m3, k = (channel group of 128, tap,
    // channel in group), `scale` = per-output-channel fp32 factor (activation scale x weight scale) applied to the
    // fp32 accumulator before the bias; out_f8: the 16-bit kernels' epilogue writes e4m3(v * out_qscale) bytes
    const uint8_t* wgt8;
    const float*   scale;
    int k_pad8, groups8;
    int in_f8, out_f8;
    float out_qscale;
    void* dbg;              // instrumentation output of the profiling variants (tools/convbench.cpp), else nullptr
    int dev_param;          // free parameter of the developer variants (tools/convbench.cpp: env MDHIP_DEV_PARAM)
    // conv_v5c.cpp, fused bottleneck: the 1x1 conv in front of this 3x3 ([n_rows][k_pad_pre] 16-bit weights, k = input
    // channel; fp32 bias); nullptr = plain 3x3
    const uint16_t* wgt_pre;
    const float*    bias_pre;
    int k_pad_pre;
    // conv_v2.cpp, 1x1 convs behind Upsample + Concat: the first up_slabs 64-channel slabs of K are read from the
    // LOW-resolution tensor in_up (pixel (y, x) -> (y / 2, x / 2), pixel pitch ld_up) instead of their 4x copy in the
    // concat buffer; nullptr = everything from `in`
    const uint16_t* in_up;
    int ld_up, up_slabs;
    // Detect decode in the epilogue of the Detect 1x1 conv (out_f32 ops of a head with 8 outputs per anchor; conv_igemm.cpp /
    // conv_v2.cpp): dec_pred != nullptr -> instead of storing its four fp32 logits a lane decodes them (mdhip_decode_store
    // below: detect_decode_kernel's statements, the same bits) and writes 16 bytes of the prediction row
    // dec_pred[image][dec_level_off + (anchor * Ho + y) * Wo + x][8]; the logits tensor is then neither written nor read
    float* dec_pred;
    const float* dec_anchors;   // device, [na][2]: anchor sizes of this level in pixels
    float dec_stride;
    int dec_level_off, dec_n_anchors;
    // floor(2^32 / HoWo), floor(2^32 / Wo) (0xffffffff for a divisor of 1): the tile set-up of the implicit-GEMM kernels
    // splits an output pixel index into (image, row, column) with conv_udiv() instead of two run-time integer
    // divisions per row; filled by the launch functions that need them (conv_set_rcp), callers leave them alone
    unsigned rcp_howo, rcp_wo;
    // conv_v2.cpp, 1x1 convs whose weights fit a wave's registers (C_in = N = 160): the streaming body (conv_v2_stream.h: same
    // MFMA chain and epilogue per output, same bits) runs them 0 = never, 1 = from the pixel count on at which it is the faster
    // one, 2 = always (mdhip_set_option "pw_stream")
    int pw_stream;
};
inline unsigned conv_rcp32(int d) { return d <= 1 ? 0xffffffffu : (unsigned)(0x100000000ull / (unsigned)d); }
inline void conv_set_rcp(ConvArgs& p) { p.rcp_howo = conv_rcp32(p.HoWo); p.rcp_wo = conv_rcp32(p.Wo); }
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// Detect decode (yolov5 Detect.forward, inference): ONE definition for detect_decode_kernel
// (misc_kernels.cpp) and for the conv epilogues that decode in place (conv_device.h: mdhip_decode_store) -- same statements,
// no contraction: same bits
__device__ __forceinline__ float mdhip_sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ void mdhip_decode_box(float l0, float l1, float l2, float l3, int x, int y, float stride, float aw, float ah,
                                                 float& cx, float& cy, float& bw, float& bh) {
#pragma clang fp contract(off)
    const float s0 = mdhip_sigmoid_exact(l0), s1 = mdhip_sigmoid_exact(l1);
    const float s2 = mdhip_sigmoid_exact(l2), s3 = mdhip_sigmoid_exact(l3);
    cx = (s0 * 2.0f + ((float)x - 0.5f)) * stride;
    cy = (s1 * 2.0f + ((float)y - 0.5f)) * stride;
    const float w2 = s2 * 2.0f, h2 = s3 * 2.0f;
    bw = (w2 * w2) * aw;
    bh = (h2 * h2) * ah;
}
#endif

struct ConvCfg {
    int bm, bn, threads;
    size_t lds_bytes;
    int blocks_per_cu;      // residency the kernel is compiled for (LDS- and wave-limited)
    const char* name;
    float prior;            // first-generation tiles: the heuristic's measured prior (choose_cfg, mdhip_exec.cpp); else unused
};

// rows of a configuration list (an X-macro):  constexpr int n = 0 LIST(MDHIP_COUNT_ROW);
#define MDHIP_COUNT_ROW(...) +1

// the tile grid of the persistent kernels (conv_igemm / conv_v2 / conv_v5 / conv_v5s / conv_f8): about as many workgroups as
// fit on the chip at once (8 XCDs of 32 CUs), each a stream of M tiles whose load pipeline runs across its tile boundaries
inline dim3 conv_tile_grid(ConvArgs& p, const ConvCfg& c) {
    p.tiles_n = (p.n_rows + c.bn - 1) / c.bn;
    p.tiles_m = (p.M + c.bm - 1) / c.bm;
    p.tiles_per_xcd = (p.tiles_m + 7) / 8;
    p.m_streams = std::max(1, std::min(p.tiles_per_xcd, (32 * c.blocks_per_cu) / p.tiles_n));
    return dim3((unsigned)(8 * p.tiles_n * p.m_streams));
}

// A kernel family: what one conv translation unit exports, once per storage type (see MDHIP_ST above) and nothing else.
// A configuration is addressed by its family and a local id; the registry below numbers them globally, in this order:
//   CONV_IGEMM    : the first-generation implicit-GEMM kernel, every 16-bit shape (conv_igemm.cpp)
//   CONV_V2       : second-generation main loop; 1x1 configurations with an activation ring, upsample read in place, Detect
//                   decode in the epilogue (conv_v2.cpp)
//   CONV_V5_RUN   : 3x3 / stride 1 with row-segment reuse across the taps of a kernel row (conv_v5.cpp; its predecessor
//                   conv_v4.cpp, the row-patch direct convolution of round 1 and the origin of the (group, r, s, c) weight
//                   packing, left the build in round 5: no table entry had selected it since round 3)
//   CONV_V5_SMALL : the same for small launches (conv_v5s.cpp)
//   CONV_V5_STRIP : the same for 80 channels, alone or fused with the 1x1 in front (conv_v5c.cpp)
//   CONV_STEM     : the stem (3x3 over 16-channel space-to-depth pixels, N = 80) with its weights in registers (conv_v6.cpp)
//   CONV_F8       : conv_v5's structure on e4m3 operands with the block-scaled K = 128 MFMA (conv_f8.cpp)
//   CONV_V7       : 3x3 / STRIDE 2 with row-run reuse (odd / even input columns in two sub-buffers; conv_v7.cpp)
enum ConvFamilyId { CONV_IGEMM = 0, CONV_V2, CONV_V5_RUN, CONV_V5_SMALL, CONV_V5_STRIP, CONV_STEM, CONV_F8, CONV_V7, CONV_NUM_FAMILIES };

// One compiled kernel: configuration `local` of its family in the variant `key`, the family's own code for what its pick()
// chooses between at run time (conv_v2.cpp: plain / pointwise / upsample read in place ...; conv_v5.cpp: the last channel
// group x aligned rows).  One key is common to the families, CONV_KEY_DEC: the instantiation that decodes in its epilogue.
// Block size and LDS belong to the instantiation -- some kernels need more LDS than their configuration's ConvCfg says.
// A family's table of these (ConvFamily::insts) is the ONE list of the kernels it has: the registry raises the LDS limit
// of every row, a launch goes through a row, and a configuration decodes when it has a CONV_KEY_DEC row.
struct ConvInst {
    const void* fn;
    int local, key, threads;
    size_t lds_bytes;
};
struct ConvInstTable { const ConvInst* rows; int n; };
constexpr int CONV_KEY_DEC = 100;
// a row of a table:  MDHIP_INST(local, key, threads, lds_bytes, kernel<template arguments>)
#define MDHIP_INST(local, key, threads, lds, ...) {(const void*)(__VA_ARGS__), (local), (key), (threads), (size_t)(lds)},
inline const ConvInst* conv_find_inst(ConvInstTable t, int local, int key) {
    for (int i = 0; i < t.n; ++i)
        if (t.rows[i].local == local && t.rows[i].key == key) return &t.rows[i];
    return nullptr;
}
// every conv launch: the instantiation a family's pick() chose (nullptr: it has none for this op) on the family's own grid
inline hipError_t conv_launch_inst(const ConvInst* inst, dim3 grid, const ConvArgs& p, hipStream_t s) {
    if (!inst) return hipErrorInvalidValue;
    void* args[] = {(void*)&p};
    return hipLaunchKernel(inst->fn, grid, dim3((unsigned)inst->threads), args, inst->lds_bytes, s);
}

struct ConvFamily {
    ConvFamilyId id;
    const ConvCfg* cfgs;    // n_cfgs public configurations, then n_dev developer variants (tools/convbench.cpp: launch_dev)
    int n_cfgs, n_dev;
    bool bitwise;           // false: equals the implicit-GEMM kernels up to fp32 summation order only (other K order)
    bool f8_in;             // takes e4m3 activations (and nothing else)
    bool f8_out;            // its epilogue can write e4m3 (ConvArgs::out_f8)
    bool (*supports)(int local, const ConvArgs& a);
    hipError_t (*launch)(int local, const ConvArgs& a, hipStream_t s);   // hipSuccess or the launch error
    ConvInstTable (*insts)();
    // the key of the instantiation (ConvInst::key) the family's pick() chooses for this op, -1 for none; nullptr: the family
    // does not tell (mdhip_op_info::variant then reports -1)
    int (*variant)(int local, const ConvArgs& a);
};
// MDHIP_CONV_FAMILY(name, id, cfgs, n_cfgs, n_dev, bitwise, f8_in, f8_out, supports, launch, insts[, variant]) defines a translation
// unit's family object.  It is host data: the device pass must not emit a copy into the code object (a family's table is a
// function-local static of its insts() for the same reason: that names -- and so instantiates -- the kernels in both passes)
#if defined(__HIP_DEVICE_COMPILE__)
#define MDHIP_CONV_FAMILY(name, ...)
#else
#define MDHIP_CONV_FAMILY(name, ...) extern const ConvFamily name = {__VA_ARGS__};
#endif
inline bool conv_family_takes(const ConvFamily& f, const ConvArgs& a) { return f.f8_in == (a.in_f8 != 0) && (!a.out_f8 || f.f8_out); }
// (a.dec_pred: the op decodes in its epilogue -- only the configurations with such an instantiation take it)
inline bool conv_decode_ok(bool cfg_decodes, const ConvArgs& a) { return !a.dec_pred || (cfg_decodes && a.out_f32 && (a.N % 8) == 0); }
// what conv_v5.cpp, conv_v5s.cpp and conv_v5c.cpp all need of an op: 3x3 / stride 1 / pad 1 on the (group, r, s, c) packing,
// the rows a tile of bm pixels touches inside the 31-bit offset range
inline bool conv5_shape_ok(const ConvArgs& a, int bm) {
    return a.wgt4 != nullptr && a.ntaps == 9 && a.kw == 3 && a.stride == 1 && a.pad == 1 && a.Ho == a.H && a.Wo == a.W && a.C8 >= 8 &&
           (a.N % 8) == 0 && (long long)(2 * a.W + bm + 16) * a.ld_in * 2 + 4096 < 0x7fffffffLL;
}

// The registry: the families in id order.  Global configuration ids count through their public configurations in that order
// (tuned tables and mdhip_set_op_cfg name them); developer variants have no global id.
struct ConvRegistry {
    const ConvFamily* fam[CONV_NUM_FAMILIES];

    int num_cfgs() const {
        int n = 0;
        for (const ConvFamily* f : fam) n += f->n_cfgs;
        return n;
    }
    // family and local id of a global id; nullptr outside [0, num_cfgs())
    const ConvFamily* find(int cfg, int* local) const {
        if (cfg < 0) return nullptr;
        for (const ConvFamily* f : fam) {
            if (cfg < f->n_cfgs) { *local = cfg; return f; }
            cfg -= f->n_cfgs;
        }
        return nullptr;
    }
    ConvFamilyId family(int cfg) const {
        int l = 0;
        const ConvFamily* f = find(cfg, &l);
        return f ? f->id : CONV_NUM_FAMILIES;
    }
    const ConvCfg& cfg(int i) const {
        int l = 0;
        const ConvFamily* f = find(i, &l);
        return f ? f->cfgs[l] : fam[0]->cfgs[0];
    }
    const ConvCfg& dev_cfg(ConvFamilyId family, int k) const { return fam[family]->cfgs[fam[family]->n_cfgs + k]; }
    bool is_bitwise_family(int cfg) const {
        int l = 0;
        const ConvFamily* f = find(cfg, &l);
        return f ? f->bitwise : true;
    }
    // the configuration has an instantiation that decodes in its epilogue
    bool cfg_decodes(int cfg) const {
        int l = 0;
        const ConvFamily* f = find(cfg, &l);
        return f && conv_find_inst(f->insts(), l, CONV_KEY_DEC) != nullptr;
    }
    bool supports(int cfg, const ConvArgs& a) const {
        int l = 0;
        const ConvFamily* f = find(cfg, &l);
        return f && (!a.dec_pred || conv_decode_ok(cfg_decodes(cfg), a)) && conv_family_takes(*f, a) && f->supports(l, a);
    }
    // the configuration takes the op as one that decodes in its epilogue (of a.dec_pred only "is set" is ever read)
    bool supports_decoding(int cfg, const ConvArgs& a) const {
        float none = 0.f;
        ConvArgs d = a;
        if (!d.dec_pred) d.dec_pred = &none;
        return supports(cfg, d);
    }
    hipError_t launch(int cfg, const ConvArgs& a, hipStream_t s) const {
        int l = 0;
        const ConvFamily* f = find(cfg, &l);
        return f && conv_family_takes(*f, a) ? f->launch(l, a, s) : hipErrorInvalidValue;
    }
    int variant(int cfg, const ConvArgs& a) const {
        int l = 0;
        const ConvFamily* f = find(cfg, &l);
        return f && f->variant && conv_family_takes(*f, a) ? f->variant(l, a) : -1;
    }
    // developer variant k of a family (tools/convbench.cpp)
    hipError_t launch_dev(ConvFamilyId family, int k, const ConvArgs& a, hipStream_t s) const {
        const ConvFamily* f = fam[family];
        return k >= 0 && k < f->n_dev ? f->launch(f->n_cfgs + k, a, s) : hipErrorInvalidValue;
    }
    // raises the dynamic-LDS limit of every instantiation (one-off)
    hipError_t init() const {
        hipError_t e = hipSuccess;
        for (const ConvFamily* f : fam) {
            const ConvInstTable t = f->insts();
            for (int i = 0; i < t.n && e == hipSuccess; ++i)
                e = hipFuncSetAttribute(t.rows[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.rows[i].lds_bytes);
        }
        return e;
    }
};
#define MDHIP_CONV_FAMILIES extern const ConvFamily conv_igemm, conv_v2, conv_v5, conv_v5s, conv_v5c, conv_v6, conv_f8, conv_v7; \
                            extern const ConvRegistry conv_registry;   /* conv_registry.cpp */
namespace st_bf16 {
MDHIP_CONV_FAMILIES
}
namespace st_f16 {
MDHIP_CONV_FAMILIES
}
#undef MDHIP_CONV_FAMILIES

// ---------------------------------------------------------------------------------------
// memory-bound helpers (misc_kernels.cpp)
// ---------------------------------------------------------------------------------------
struct LetterboxDev {     // device copy of mdhip_letterbox + source pointer
    const uint8_t* src;
    int src_h, src_w, resized_h, resized_w, top, left;
    int interp;           // 0: cv2.INTER_LINEAR, 1: cv2.INTER_AREA (shrinking only)
    // cv2's bilinear scales  1.0 / ((double)resized / (double)src)  per axis, computed on the host with that very expression (IEEE
    // double on both sides: the bits the kernels' own linear_scale() produces); read by letterbox_linear_s2d_kernel
    double sx, sy;
};
// A window of a larger device image with a row pitch (a tile): d.src is the window's first pixel, d.src_h x d.src_w the
// window.  The streaming kernels read whole aligned dwords; inside the parent that is harmless, behind its end it is not:
// `readable` bounds every read.
struct LetterboxWin {
    LetterboxDev d;
    long long readable;   // bytes from d.src to the end of the parent allocation (the host clamps it below 2^31)
    int pitch;            // bytes between two rows of the parent
    int reserved;
};
// u8 HWC -> space-to-depth bf16 [n][out_h/2][out_w/2][16] (12 real channels: (dy,dx,c)), /255
// Three kernels, chosen per batch from the geometry: a streaming copy (no image resampled), a streaming bilinear kernel
// (cv2.INTER_LINEAR, every real camera image) and the general one (INTER_AREA, very wide sources); force_general = the last
// one whatever the batch (tests, A/B).  geom_host: the geometry in host memory (source pointers are device pointers); when
// letterbox_geometry_travels_inline(...) it is passed in the kernel arguments and geom_dev is not read (the caller skips
// the upload)
bool letterbox_geometry_travels_inline(const LetterboxDev* geom_host, int n, int out_w, bool force_general);
hipError_t launch_letterbox_s2d(const LetterboxDev* geom_dev, const LetterboxDev* geom_host, int n, int out_h, int out_w,
                                uint16_t* out, int f16, bool force_general, hipStream_t s);
// the same for windows of pitched images (sibling kernels built from the same bodies; the dense kernels do not change)
bool letterbox_geometry_travels_inline(const LetterboxWin* geom_host, int n, int out_w, bool force_general);
hipError_t launch_letterbox_s2d(const LetterboxWin* geom_dev, const LetterboxWin* geom_host, int n, int out_h, int out_w,
                                uint16_t* out, int f16, bool force_general, hipStream_t s);
// SPPF: three chained 5x5/s1/p2 max pools of slice 0 written to slices 1..3 of the same buffer
hipError_t launch_sppf_pool(uint16_t* buf, int ld, int c, int n, int h, int w, int k, int f16, hipStream_t s);
// nearest x2 upsample of a view into a view
hipError_t launch_upsample2x(const uint16_t* in, int ld_in, uint16_t* out, int ld_out, int c,
                             int n, int h, int w, hipStream_t s);
// strided channel-slice copy
hipError_t launch_copy_view(const uint16_t* in, int ld_in, uint16_t* out, int ld_out, int c,
                            long long pixels, hipStream_t s);
// max |x| of a 16-bit view, atomically max-ed into *out (a non-negative float, zero it first)
hipError_t launch_absmax_view(const uint16_t* in, int ld, int c, long long pixels, int f16, float* out, hipStream_t s);
// Detect decode of one level: logits fp32 [n*ny*nx][ld] -> pred[n][n_anchors][no].  A test-time-augmentation
// pass keeps anchors [keep_from, keep_to) of its own numbering, de-scales / un-flips the boxes and writes them
// at out_off of the concatenated prediction; the default is the plain forward.
struct DecodeTta {
    int keep_from = 0, keep_to = 0x7fffffff, out_off = 0;
    float scale = 1.0f;
    int flip_lr = 0;
    float img_w = 0.f;
};
hipError_t launch_detect_decode(const float* logits, int ld, float* pred, int n, int ny, int nx,
                                int na, int no, int n_anchors, int level_off, float stride,
                                const float* anchors_px /*device, [na][2]*/, const DecodeTta& tta, hipStream_t s);
// scale_img of yolov5's augmented inference: s2d input (h x w) -> s2d (oh x ow), bilinear to (sh x sw), pad 0.447
hipError_t launch_tta_scale(const uint16_t* in, uint16_t* out, int n, int h, int w, int sh, int sw, int oh, int ow,
                            int flip_lr, int f16, hipStream_t s);
// debug readback: NHWC bf16 view -> NCHW fp32
hipError_t launch_nhwc_to_nchw_f32(const uint16_t* in, int ld, float* out, int n, int c, int h,
                                   int w, int f16, hipStream_t s);
hipError_t launch_s2d_to_nchw_f32(const uint16_t* in, float* out, int n, int h, int w, int f16, hipStream_t s);

// ---------------------------------------------------------------------------------------
// NMS (nms_kernels.cpp)
// ---------------------------------------------------------------------------------------
constexpr int kNmsScanParts = 16;   // workgroups per image of the candidate scan (nms_kernels.cpp stage A)
struct NmsScratch {
    uint32_t* keys[3];     // [n][cap] each: 0 / 2 = the band being sorted (ping-pong), 1 = every candidate in anchor order
    uint32_t* vals[3];
    int cap;               // candidates capacity per image (= max anchors)
    uint32_t* seg_cnt;     // [n][kNmsScanParts] candidates found by each scan workgroup
};
// anchor_free: the ultralytics rule of the YOLO11 models (pred rows [cx, cy, w, h, cls0..], no objectness, conf = the
// largest class score, IoU on boxes shifted by cls * 7680, only the kNmsMaxNmsAnchorFree highest-ranked candidates)
hipError_t launch_nms(const float* pred, int n, int n_anchors, int no, float conf_thres,
                      float iou_thres, int max_det, const NmsScratch& scr, float* out /*device [n][max_det][6]*/,
                      int* counts /*device [n]*/, hipStream_t s, bool anchor_free = false);
constexpr int kNmsMaxDet = 1024;
constexpr int kNmsMaxNmsAnchorFree = 30000;   // ultralytics non_max_suppression max_nms

// ---------------------------------------------------------------------------------------
// YOLO11 blocks (yolo11_kernels.cpp)
// ---------------------------------------------------------------------------------------
// depthwise 3x3 / s1 / p1 over NHWC 16-bit views; wgt [9][C] 16-bit, bias [C] fp32; output channel o reads input channel
// (o / grp) * grp_stride + grp_off + o % grp; act 1 = SiLU; res (may be nullptr): added after the activation (in place:
// res == out is allowed).  C, grp, grp_stride, grp_off and every pitch multiples of 8.
hipError_t launch_dwconv3x3(const uint16_t* in, int ld_in, const uint16_t* wgt, const float* bias, uint16_t* out, int ld_out,
                            const uint16_t* res, int ld_res, int n, int H, int W, int C, int grp, int grp_stride, int grp_off,
                            int act, int f16, hipStream_t s);
// C2PSA attention: qkv [n][N][ld_qkv] with per head [q 32 | k 32 | v 64] channels at head * 128 -> out [n][N][ld_out],
// channels head * 64 .. + 63 = v softmax(q^T k / sqrt(32))^T
hipError_t launch_attention(const uint16_t* qkv, int ld_qkv, uint16_t* out, int ld_out, int n, int N, int heads, int f16,
                            hipStream_t s);
// DFL decode of one level: box logits fp32 [n*ny*nx][ld_box] (4 sides x 16 bins), class logits fp32 [n*ny*nx][ld_cls]
// -> pred[n][n_anchors][4 + nc] rows level_off + y * nx + x
hipError_t launch_dfl_decode(const float* box, int ld_box, const float* cls, int ld_cls, float* pred, int n, int ny, int nx,
                             int nc, int n_anchors, int level_off, float stride, hipStream_t s);

// ---------------------------------------------------------------------------------------
// YOLOv9-C blocks (yolov9_kernels.cpp)
// ---------------------------------------------------------------------------------------
// ADown pools of in [n][H][W][c_in] (H, W even): A [n][H][W][c_in / 2] = avg_pool2d(2, s1) of the first half, zero in the
// last row and column; B [n][H/2][W/2][c_in / 2] = max_pool2d(3, 2, 1) of avg_pool2d(2, s1) of the second half (windows
// clipped to the (H-1) x (W-1) extent).  Averages: ((a + b) + c) + d in fp32, times 1/4, rounded once to storage.
hipError_t launch_adown_pool(const uint16_t* in, int ld_in, uint16_t* A, int ld_a, uint16_t* B, int ld_b, int n, int H, int W,
                             int c_in, int f16, hipStream_t s);
// CBFuse: out [n][H][W][C] = round(((up(src0) + up(src1)) + up(src2)) + last), sums in fp32, up = nearest resize of
// source k ([n][H / factor_k][W / factor_k], pitch ld_src_k) by its integer factor
struct CbfuseArgs {
    const uint16_t* src[3];
    int ld_src[3];
    int factor[3];
    int n_src;
    const uint16_t* last;
    int ld_last;
    uint16_t* out;
    int ld_out;
    int n, H, W, C;
};
hipError_t launch_cbfuse(const CbfuseArgs& a, int f16, hipStream_t s);

// ---------------------------------------------------------------------------------------
// JPEG reconstruction (jpeg_kernels.cpp): one image, passed to the kernels by value
// ---------------------------------------------------------------------------------------
struct JpegDev {
    const int16_t* coef;          // quantised coefficients, 16-byte aligned; plane c at coef + coef_off[c]: [blocks_h][blocks_w][64]
    uint8_t* planes;              // scratch: u8 component planes, plane c at planes + plane_off[c], (blocks_h * 8) x (blocks_w * 8)
    uint8_t* out;                 // the rotated H x W x 3 RGB image
    long long coef_off[3];
    long long plane_off[3];
    int blocks_w[3], blocks_h[3];
    int width, height, components;
    int h_samp, v_samp;           // luma sampling factors (chroma 1 x 1)
    int rotation;                 // 0 / 90 / 180 / 270, counter-clockwise
    uint16_t quant[3][64];        // natural order
};
// de-quantisation + inverse DCT into the planes, then upsampling + colour conversion + rotation into `out`
hipError_t launch_jpeg_reconstruct(const JpegDev& d, hipStream_t s);
// JPEG recompression of a window (mdhip_jpeg_recompress): the encoder's lossy half on the width x height window at `src`
// (rows `pitch` bytes apart), then the reconstruction above from the planes on.  d: three components, 2 x 2 luma sampling,
// rotation 0, blocks_w / blocks_h each component's own whole blocks, quant = {luma, chroma, chroma}; d.coef is not read.
hipError_t launch_jpeg_recompress(const JpegDev& d, const uint8_t* src, long long pitch, hipStream_t s);

// ---------------------------------------------------------------------------------------
// JPEG entropy decoding (jpeg_huffman.cpp): one record per image of the batch, in device memory
// ---------------------------------------------------------------------------------------
struct JpegScanDev {
    const uint8_t*  scan;         // the entropy-coded bytes of the file
    int16_t*        coef;         // coef_count values, 16-byte aligned
    const ::MdjImage* im;
    const uint32_t* seg_off;      // [n_segments + 1] first byte of each segment; a segment ends 2 bytes in front of the next
    const uint32_t* seg_lane0;    // [n_segments + 1] first lane of each segment
    uint64_t*       lane_end;     // [n_lanes] packed MdjState: where the lane's decode ended
    uint64_t*       lane_start;   // [n_lanes] packed start it decoded from
    uint32_t*       lane_seg;     // [n_lanes]
    uint32_t*       lane_block;   // [n_lanes] blocks closed in front of the lane within its segment
    uint32_t*       energy;       // [coef_count / 64] AC energy of each block
    long long*      dc_sum;       // [sum of dc_chunks]
    uint32_t*       dc_reset;
    long long       coef_count;
    long long       dc_blocks[3], dc_chunks[3];
    uint32_t        n_segments, n_lanes;
};
void launch_jpeg_entropy_front(const JpegScanDev* devs, int n, unsigned max_lanes, hipStream_t s);
void launch_jpeg_entropy_sync(const JpegScanDev* devs, int n, unsigned max_lanes, unsigned long long* counters, hipStream_t s);
void launch_jpeg_entropy_back(const JpegScanDev* devs, int n, unsigned max_lanes, long long max_chunks, uint32_t* status, hipStream_t s);
int jpeg_entropy_dc_chunk();

// ---------------------------------------------------------------------------------------
// JPEG entropy encoding (jpeg_encode.cpp): one record for the whole batch, passed to the kernels by value
// ---------------------------------------------------------------------------------------
struct JpegEncDev {
    const ::MdjEncCrop*   crops;  // [n + 1] the crops (jpeg_encode.h); the last entry carries the totals
    const ::MdjEncTables* tables; // the standard's four tables as codes and lengths
    const uint16_t* quant;        // [pairs][2][64] luma, chroma; natural order; crop c takes pair crops[c].table
    int16_t*  coef;               // [blocks][64] quantised coefficients, MCU order, blocks transposed; 16-byte aligned
    uint32_t* len;                // [blocks] bit length of each block
    uint64_t* off;                // [blocks + 1] exclusive prefix sum of len
    uint64_t* partial;            // scratch of the prefix sums: one value per 1024 items
    uint32_t* bitbuf;             // the unstuffed bits: every crop's region at its bound, zeroed before the call
    uint32_t* count;              // [chunks] bytes each stuffing chunk writes
    uint64_t* start;              // [chunks + 1] exclusive prefix sum of count: where each chunk's output begins
    uint32_t* status;             // [n] MDJ_ENC_ERR_* bits of each crop, zeroed before the call
    long long* result;            // [2 n + 1] offsets, sizes, capacity needed
    uint8_t*  out;
    long long capacity;
    long long blocks, chunks;
    int n, chunk_bytes;
    // mdhip_jpeg_encode_kept (jpeg_keep.h); source NULL: every block comes from the pixels
    const int16_t* const* source; // [n] each crop's source planes, or NULL
    const ::MdjKeepRect*  rects;  // the changed rectangles, clipped, crop by crop
    const int32_t*        rect0;  // [n + 1] crop c's rectangles are rects[rect0[c] .. rect0[c + 1])
};
hipError_t launch_jpeg_encode(const JpegEncDev& d, hipStream_t s);
long long jpeg_encode_scan_tiles(long long n);

// ---------------------------------------------------------------------------------------
// Gaussian blur of rectangles (blur_kernels.cpp): one record per rectangle, read by the workgroups of a launch (blockIdx.y)
// ---------------------------------------------------------------------------------------
constexpr int BLUR_LDS_BYTES = 49152;  // the two row buffers of a workgroup of the row stage (blur_box.h md_blur_plan_x)
struct BlurRect {
    uint8_t*  img;                     // the rectangle's first byte in its image
    long long pitch;                   // bytes from row to row of the image
    long long s0, s1;                  // the rectangle's two planes in the scratch buffer: byte offsets, sp bytes a row
    int w, h;                          // pixels
    int sp;                            // bytes a row of a plane: >= 3 w
    int rows, stride, chunks, step, halo;  // blur_box.h MdBlurXPlan
    int row_groups;                    // (h + rows - 1) / rows: the row stage runs row_groups * chunks workgroups
    int pad;
};
// one rectangle of each of n images: rows -> scratch, columns -> image.  max_row_blocks / max_width: the largest
// row_groups * chunks and w among the n records
hipError_t launch_blur_round(const BlurRect* rects, int n, int max_row_blocks, int max_width, uint8_t* scratch, int r, uint32_t ww,
                             uint32_t fw, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Annotated previews (preview_kernels.cpp): LANCZOS resize and drawing, one record per image and pass (blockIdx.y / .z)
// ---------------------------------------------------------------------------------------
struct ResampleRows {                  // the horizontal pass of one image
    const uint8_t* src;
    uint8_t*  dst;                     // the image between the passes, or the destination when the height stays
    long long src_pitch, dst_pitch;    // bytes from row to row
    int rows, out_w;                   // rows of both images, pixels of an output row
    int ksize;                         // taps a line of the coefficient table has room for
    int strip, wg_rows, run_bytes;     // resample.h MdResampleStrips
    int strips, row_groups;            // the pass runs strips * row_groups workgroups
    int bounds_off, kk_off;            // of this (in, out) pair in the coefficient table, in int32 words
};
struct ResampleColumns {               // the vertical pass of one image
    const uint8_t* src;                // the image between the passes, or the source when the width stays
    uint8_t*  dst;
    long long src_pitch, dst_pitch;
    int row_bytes, out_h;              // bytes of a row that hold pixels (3 x width), output rows
    int ksize, bounds_off, kk_off;
    int pad;
};
struct DrawImage {
    uint8_t*  img;
    long long pitch;
    int x0, y0, x1, y1;                // what the image's operations cover, clipped to the image; inclusive
    int op_first, op_count;            // its operations in the list, in order
};
hipError_t launch_resample_rows(const ResampleRows* descs, int n, int max_blocks, const int32_t* table, hipStream_t s);
hipError_t launch_resample_columns(const ResampleColumns* descs, int n, int max_row_bytes, int max_out_h, const int32_t* table, hipStream_t s);
hipError_t launch_draw_ops(const DrawImage* images, int n, int max_w, int max_h, const int32_t* ops, const uint8_t* patches, hipStream_t s);
// The fan-out draw: a destination is its source's pixels under the destination's operations; the source is only read
struct DrawFrom {
    const uint8_t* src;
    uint8_t*  dst;
    long long src_pitch, dst_pitch;
    int row_bytes, height;             // 3 * width, and the rows
    int x0, y0, x1, y1;                // what the operations cover, clipped to the image; inclusive; x1 < x0: nothing
    int op_first, op_count;
};
hipError_t launch_draw_ops_from(const DrawFrom* images, int n, int max_row_bytes, int max_h, const int32_t* ops, const uint8_t* patches,
                                hipStream_t s);

// ---------------------------------------------------------------------------------------
// Classifier input (classify_kernels.cpp): n crops -> fp32 [n][3][S][S], one record per crop (blockIdx.y), one launch.
// The record (MdClassifyCrop) is resample.h's; max_blocks: the largest strips * row_tiles among the n records
// ---------------------------------------------------------------------------------------
hipError_t launch_classifier_input(const MdClassifyCrop* crops, int n, int max_blocks, const int32_t* table, const float* lut, float* out,
                                   hipStream_t s);
// Thumbnails (the same kernel body, bytes stored interleaved at each record's dst): n tiles, one launch
hipError_t launch_thumbnails(const MdClassifyCrop* tiles, int n, int max_blocks, const int32_t* table, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Change detection (change_kernels.cpp; the arithmetic is change_detect.h's): one record per image of the blur launches and
// one per pair of the others, read by the workgroups of a launch (blockIdx.z, or blockIdx.y of the one-dimensional kernels)
// ---------------------------------------------------------------------------------------
struct ChgImage {
    const uint8_t* rgb;                // the image, `pitch` bytes a row
    long long pitch;
    uint16_t* first;                   // w x h: the blur's first pass (along x), 16-bit sums
    uint8_t*  out;                     // w x h: the blurred gray image
    int w, h;
    int y0, y1;                        // rows the region of interest keeps: [y0, y1)
};
struct ChgPair {
    const uint8_t* a;                  // the two blurred gray images, w x h
    const uint8_t* b;
    uint8_t*  m[2];                    // w x h each: the thresholded mask (m[0]) and the dilation's other buffer
    uint32_t* label;                   // w x h: the parent links of the label merge (0xffffffff: background)
    uint32_t* stat;                    // 5 planes of w x h, read at a component's label: pixel count, xmin, ymin, xmax, ymax
    uint32_t* block_count;             // per 256 pixels the significant labels among them, and (behind them) the offset of the first
    uint32_t* hist;                    // 256
    unsigned long long* count;         // non-zero pixels of the thresholded mask
    int32_t*  n_regions;
    int32_t*  regions;                 // cap x 5
    int32_t*  label_out;               // nullptr, or w x h: every pixel's label (-1: background)
    int w, h;
    int y0, y1;
};
constexpr int CHG_DILATE_HALO = 32;    // reach of one dilation launch to either side, in pixels
hipError_t launch_chg_blur(const ChgImage* images, int n, int max_w, int max_h, const ChgWeights& wt, hipStream_t s);
// mode 0: the histogram of |a - b| (added to hist); mode 1: the thresholded mask m[0] with pair p's threshold thr[p], and its count
hipError_t launch_chg_diff(const ChgPair* pairs, int n, long long max_px, int mode, const int32_t* thr, hipStream_t s);
// `iterations` dilations with the k x k square, as many of them fused per launch as the halo allows; *sel: in, the buffer that
// holds the mask; out, the one that holds the result
hipError_t launch_chg_dilate(const ChgPair* pairs, int n, int max_w, int max_h, int k, int iterations, int* sel, hipStream_t s);
// the regions of m[sel]: labels, per-label sums, the significant ones (count > min_area) in ascending order, at most cap written
hipError_t launch_chg_regions(const ChgPair* pairs, int n, int max_w, int max_h, int sel, int min_area, int cap, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Gray pixels of a rectangle (gray_kernels.cpp; the statement is gray_count.h's): one record per image, read by the workgroups
// of blockIdx.y
// ---------------------------------------------------------------------------------------
struct GrayWindow {
    const uint8_t* origin;             // the window's first pixel, `pitch` bytes a row
    long long pitch;
    unsigned long long* count;         // the image's counter, zero before the launch
    int w, h;                          // of the window
};
// max_groups: the largest rows x gc_groups(width) of the n windows
hipError_t launch_gray_count(const GrayWindow* windows, int n, long long max_groups, hipStream_t s);

}  // namespace mdhip
