// The YOLO11 / YOLOv9 kernels and the region stage of the change detection in isolation (tests): the mdhip_*_on hooks of
// include/mdhip.h.
// host buffers in / out; scratch device memory is allocated per call (not for the product path)
// mdhip_tta_input_on is the one hook that works on the context's own buffers: the scaled input of an augmented pass.

#include <algorithm>
#include <vector>

#include "mdhip_ctx.h"
#include "change_detect.h"

namespace {
struct DevBufs {
    std::vector<void*> p;
    ~DevBufs() { for (void* q : p) (void)hipFree(q); }
    hipError_t get(size_t bytes, void** out) { *out = nullptr; hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 16)); if (e == hipSuccess) p.push_back(*out); return e; }
};
}  // namespace

extern "C" {

int mdhip_dwconv3x3_on(mdhip_ctx* ctx, const uint16_t* in, int ld_in, const float* weight, const float* bias, const uint16_t* res,
                       uint16_t* out, int n, int h, int w, int c, int grp, int grp_stride, int grp_off, int act, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !in || !weight || !bias || !out || n < 1 || h < 1 || w < 1 || c < 8 || c % 8 || grp < 8 || ld_in < 8)
        return MDHIP_EINVAL;
    if ((c / grp - 1) * grp_stride + grp_off + grp > ld_in || c % grp) return fail(ctx, MDHIP_EINVAL, "channel mapping outside ld_in");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int f16 = ctx->dtype == MDHIP_DTYPE_FP16;
    std::vector<uint16_t> wp((size_t)9 * c);
    for (int o = 0; o < c; ++o)
        for (int t = 0; t < 9; ++t) wp[(size_t)t * c + o] = f32_to_st(weight[(size_t)o * 9 + t], f16);
    const size_t px = (size_t)n * h * w;
    DevBufs d;
    void *din, *dw, *db, *dout, *dres = nullptr;
    HIP_TRY(ctx, d.get(px * ld_in * 2, &din));
    HIP_TRY(ctx, d.get(wp.size() * 2, &dw));
    HIP_TRY(ctx, d.get((size_t)c * 4, &db));
    HIP_TRY(ctx, d.get(px * c * 2, &dout));
    HIP_TRY(ctx, hipMemcpy(din, in, px * ld_in * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dw, wp.data(), wp.size() * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(db, bias, (size_t)c * 4, hipMemcpyHostToDevice));
    if (res) {
        HIP_TRY(ctx, d.get(px * c * 2, &dres));
        HIP_TRY(ctx, hipMemcpy(dres, res, px * c * 2, hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, launch_dwconv3x3((const uint16_t*)din, ld_in, (const uint16_t*)dw, (const float*)db, (uint16_t*)dout, c,
                                  (const uint16_t*)dres, c, n, h, w, c, grp, grp_stride, grp_off, act, f16, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMemcpy(out, dout, px * c * 2, hipMemcpyDeviceToHost));
    return MDHIP_OK;
}

int mdhip_attention_on(mdhip_ctx* ctx, const uint16_t* qkv, uint16_t* out, int n, int n_tokens, int heads, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !qkv || !out || n < 1 || n_tokens < 1 || heads < 1) return MDHIP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)n * n_tokens;
    DevBufs d;
    void *din, *dout;
    HIP_TRY(ctx, d.get(px * heads * 128 * 2, &din));
    HIP_TRY(ctx, d.get(px * heads * 64 * 2, &dout));
    HIP_TRY(ctx, hipMemcpy(din, qkv, px * heads * 128 * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, launch_attention((const uint16_t*)din, heads * 128, (uint16_t*)dout, heads * 64, n, n_tokens, heads,
                                  ctx->dtype == MDHIP_DTYPE_FP16, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMemcpy(out, dout, px * heads * 64 * 2, hipMemcpyDeviceToHost));
    return MDHIP_OK;
}

int mdhip_dfl_decode_on(mdhip_ctx* ctx, const float* box, const float* cls, int nc, int n, int ny, int nx, float stride, float* pred,
                        void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !box || !cls || !pred || nc < 1 || n < 1 || ny < 1 || nx < 1) return MDHIP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)n * ny * nx;
    DevBufs d;
    void *db, *dc, *dp;
    HIP_TRY(ctx, d.get(px * 64 * 4, &db));
    HIP_TRY(ctx, d.get(px * nc * 4, &dc));
    HIP_TRY(ctx, d.get(px * (4 + nc) * 4, &dp));
    HIP_TRY(ctx, hipMemcpy(db, box, px * 64 * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(dc, cls, px * nc * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, launch_dfl_decode((const float*)db, 64, (const float*)dc, nc, (float*)dp, n, ny, nx, nc, ny * nx, 0, stride, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMemcpy(pred, dp, px * (4 + nc) * 4, hipMemcpyDeviceToHost));
    return MDHIP_OK;
}

int mdhip_adown_pool_on(mdhip_ctx* ctx, const uint16_t* in, uint16_t* a, uint16_t* b, int n, int h, int w, int c_in,
                        void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !in || !a || !b || n < 1 || h < 2 || w < 2 || h % 2 || w % 2 || c_in < 16 || c_in % 16) return MDHIP_EINVAL;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)n * h * w, half = (size_t)c_in / 2;
    DevBufs d;
    void *din, *da, *db;
    HIP_TRY(ctx, d.get(px * c_in * 2, &din));
    HIP_TRY(ctx, d.get(px * half * 2, &da));
    HIP_TRY(ctx, d.get(px / 4 * half * 2, &db));
    HIP_TRY(ctx, hipMemcpy(din, in, px * c_in * 2, hipMemcpyHostToDevice));
    HIP_TRY(ctx, launch_adown_pool((const uint16_t*)din, c_in, (uint16_t*)da, (int)half, (uint16_t*)db, (int)half, n, h, w, c_in,
                                   ctx->dtype == MDHIP_DTYPE_FP16, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMemcpy(a, da, px * half * 2, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(b, db, px / 4 * half * 2, hipMemcpyDeviceToHost));
    return MDHIP_OK;
}

int mdhip_cbfuse_on(mdhip_ctx* ctx, const uint16_t* const* src, const int32_t* factor, int n_src, const uint16_t* last,
                    uint16_t* out, int n, int h, int w, int c, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !src || !factor || !last || !out || n_src < 1 || n_src > 3 || n < 1 || h < 1 || w < 1 || c < 8 || c % 8)
        return MDHIP_EINVAL;
    for (int k = 0; k < n_src; ++k)
        if (!src[k] || factor[k] < 1 || h % factor[k] || w % factor[k]) return fail(ctx, MDHIP_EINVAL, "bad CBFuse source %d", k);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)n * h * w;
    DevBufs d;
    CbfuseArgs a{};
    void *dl, *dout;
    for (int k = 0; k < n_src; ++k) {
        const size_t bytes = (size_t)n * (h / factor[k]) * (w / factor[k]) * c * 2;
        void* p;
        HIP_TRY(ctx, d.get(bytes, &p));
        HIP_TRY(ctx, hipMemcpy(p, src[k], bytes, hipMemcpyHostToDevice));
        a.src[k] = (const uint16_t*)p;
        a.ld_src[k] = c;
        a.factor[k] = factor[k];
    }
    HIP_TRY(ctx, d.get(px * c * 2, &dl));
    HIP_TRY(ctx, d.get(px * c * 2, &dout));
    HIP_TRY(ctx, hipMemcpy(dl, last, px * c * 2, hipMemcpyHostToDevice));
    a.n_src = n_src;
    a.last = (const uint16_t*)dl;
    a.ld_last = c;
    a.out = (uint16_t*)dout;
    a.ld_out = c;
    a.n = n;
    a.H = h;
    a.W = w;
    a.C = c;
    HIP_TRY(ctx, launch_cbfuse(a, ctx->dtype == MDHIP_DTYPE_FP16, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMemcpy(out, dout, px * c * 2, hipMemcpyDeviceToHost));
    return MDHIP_OK;
}

int mdhip_tta_input_on(mdhip_ctx* ctx, int n, int h, int w, int pass, float* out, int* oh, int* ow, void* hip_stream) {
    NEED_MODEL(ctx);
    if (ctx->anchor_free)
        return fail(ctx, MDHIP_EUNSUPPORTED, "mdhip_tta_input_on: augmented inference is implemented for YOLOv5 (anchor-based) "
                                             "models only, not for anchor-free (YOLO11) models");
    if (pass != 1 && pass != 2) return fail(ctx, MDHIP_EINVAL, "mdhip_tta_input_on: pass %d is not a scaled pass (1 or 2)", pass);
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (ctx->last_n < n || ctx->last_h != h || ctx->last_w != w)
        return fail(ctx, MDHIP_EINVAL, "mdhip_tta_input_on needs mdhip_preprocess of the same batch first");
    const TtaPass tp = tta_pass(ctx, h, w, pass);
    if (oh) *oh = tp.oh;
    if (ow) *ow = tp.ow;
    if (!out) return MDHIP_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int f16 = ctx->dtype == MDHIP_DTYPE_FP16;
    const size_t in_bytes = (size_t)n * (h / 2) * (w / 2) * 16 * 2, out_bytes = (size_t)n * 3 * tp.oh * tp.ow * 4;
    uint16_t* in = (uint16_t*)(ctx->arena + ctx->input.off);
    uint16_t* orig = (uint16_t*)(ctx->arena + ctx->input_orig.off);
    DevBufs d;
    void* tmp;
    HIP_TRY(ctx, d.get(out_bytes, &tmp));
    // as a scaled pass of mdhip_forward_tta: the batch goes to the scratch copy, the scaled input is written over `input`
    HIP_TRY(ctx, hipMemcpyAsync(orig, in, in_bytes, hipMemcpyDeviceToDevice, s));
    hipError_t e = launch_tta_scale(orig, in, n, h, w, tp.sh, tp.sw, tp.oh, tp.ow, tp.flip, f16, s);
    if (e == hipSuccess) e = launch_s2d_to_nchw_f32(in, (float*)tmp, n, tp.oh, tp.ow, f16, s);
    // `input` holds the batch again, whatever became of the launches
    hipError_t back = hipMemcpyAsync(in, orig, in_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = back;
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, out_bytes, hipMemcpyDeviceToHost, s);
    hipError_t done = hipStreamSynchronize(s);
    HIP_TRY(ctx, e);
    HIP_TRY(ctx, done);
    return MDHIP_OK;
}

// (reads no model: a context of mdhip_create_images serves)
int mdhip_label_regions_on(mdhip_ctx* ctx, const uint8_t* mask, int w, int h, int min_area, int cap, int32_t* labels, int32_t* n_regions,
                           int32_t* regions, uint8_t* overflow, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!mask || !labels || !n_regions || !overflow || w < 1 || h < 1 || w > CHG_MAX_SIDE || h > CHG_MAX_SIDE ||
        (long long)w * h > CHG_MAX_PIXELS || min_area < 0 || cap < 0 || cap > 65536 || (cap && !regions))
        return fail(ctx, MDHIP_EINVAL, "a NULL pointer, or %dx%d, min_area %d, cap %d outside their ranges", w, h, min_area, cap);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)w * h, nb = (px + 255) / 256;
    DevBufs d;
    void *dm, *dlabel, *dstat, *dblocks, *dn, *dregions, *dout, *drec;
    HIP_TRY(ctx, d.get(px, &dm));
    HIP_TRY(ctx, d.get(4 * px, &dlabel));
    HIP_TRY(ctx, d.get(20 * px, &dstat));
    HIP_TRY(ctx, d.get(8 * nb, &dblocks));
    HIP_TRY(ctx, d.get(4, &dn));
    HIP_TRY(ctx, d.get(20 * (size_t)cap, &dregions));
    HIP_TRY(ctx, d.get(4 * px, &dout));
    HIP_TRY(ctx, d.get(sizeof(ChgPair), &drec));
    ChgPair rec{};
    rec.m[0] = (uint8_t*)dm, rec.m[1] = nullptr;
    rec.label = (uint32_t*)dlabel, rec.stat = (uint32_t*)dstat, rec.block_count = (uint32_t*)dblocks;
    rec.n_regions = (int32_t*)dn, rec.regions = (int32_t*)dregions, rec.label_out = (int32_t*)dout;
    rec.w = w, rec.h = h, rec.y0 = 0, rec.y1 = h;
    HIP_TRY(ctx, hipMemcpy(dm, mask, px, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(drec, &rec, sizeof(rec), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(dregions, 0, std::max<size_t>(20 * (size_t)cap, 16)));
    HIP_TRY(ctx, launch_chg_regions((const ChgPair*)drec, 1, w, h, 0, min_area, cap, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMemcpy(labels, dout, 4 * px, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(n_regions, dn, 4, hipMemcpyDeviceToHost));
    if (cap) HIP_TRY(ctx, hipMemcpy(regions, dregions, 20 * (size_t)cap, hipMemcpyDeviceToHost));
    *overflow = *n_regions > cap ? 1 : 0;
    return MDHIP_OK;
}

}  // extern "C"
