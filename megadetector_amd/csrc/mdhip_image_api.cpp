// The image entry points of the C ABI (include/mdhip.h): letterbox (mdhip_preprocess*), JPEG (mdhip_jpeg_*), mdhip_blur_regions,
// the previews (mdhip_resample_lanczos, mdhip_draw_ops), the classifier input (mdhip_classifier_input), the thumbnails
// (mdhip_thumbnails), change detection (mdhip_change_detect), the gray pixels of a rectangle (mdhip_gray_count).
// None of them looks at the model: they check their arguments, lay out scratch in one of the context's growable buffers
// (mdhip_ctx.h DevBuffer) and launch.  What their checks have in common is written once, below; where two entry points
// apply the same checks in a different order, each keeps its own order (the first failing check is what a caller sees).

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "mdhip_ctx.h"
#include "jpeg_subseq.h"
#include "jpeg_encode.h"
#include "jpeg_keep.h"
#include "blur_box.h"
#include "resample.h"
#include "change_detect.h"
#include "gray_count.h"

namespace {

// device (or managed) memory?  (a pointer the runtime does not know is an error: cleared, or a later hipGetLastError reports it)
bool is_device_ptr(const void* p) {
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
}

// A pitched RGB window of `noun` i ("window", "image"): sides of 1 .. max_side pixels, rows that do not overlap, and no more
// bytes from its first pixel to the end of its last row (*extent) than the kernels' 32-bit offsets reach.
int check_window(mdhip_ctx* ctx, const char* noun, int i, int w, int h, long long pitch, int max_side = 65535, long long* extent = nullptr) {
    if (w < 1 || h < 1 || w > max_side || h > max_side) return fail(ctx, MDHIP_EINVAL, "%s %d: %dx%d", noun, i, w, h);
    const long long need = (long long)(h - 1) * pitch + (long long)w * 3;
    if (pitch < (long long)w * 3 || need > 0x7fff0000LL)
        return fail(ctx, MDHIP_EINVAL, "%s %d: pitch %lld for %d pixels per row (or %s %s above 2 GB)", noun, i, pitch, w,
                    strchr("aeiou", noun[0]) ? "an" : "a", noun);
    if (extent) *extent = need;
    return MDHIP_OK;
}

// The canvas of crop / tile i (mdhip_classifier_input, mdhip_thumbnails): its size, the rectangle of image pixels inside it,
// and that those pixels are device memory
int check_canvas(mdhip_ctx* ctx, const char* noun, int i, const uint8_t* src, long long pitch, int src_w, int src_h, int canvas_w, int canvas_h,
                 int off_x, int off_y) {
    if (canvas_w < 1 || canvas_h < 1 || canvas_w > 65535 || canvas_h > 65535)
        return fail(ctx, MDHIP_EINVAL, "%s %d: a canvas of %dx%d", noun, i, canvas_w, canvas_h);
    if (int rc = check_window(ctx, noun, i, src_w, src_h, pitch)) return rc;
    if (off_x < 0 || off_y < 0 || off_x > canvas_w - src_w || off_y > canvas_h - src_h)
        return fail(ctx, MDHIP_EINVAL, "%s %d: %dx%d pixels at (%d, %d) leave the %dx%d canvas", noun, i, src_w, src_h, off_x, off_y, canvas_w,
                    canvas_h);
    if (!src || !is_device_ptr(src)) return fail(ctx, MDHIP_EINVAL, "%s %d: NULL or a host pointer -- the pixels must be device memory", noun, i);
    return MDHIP_OK;
}

int check_quant_tables(mdhip_ctx* ctx, const uint16_t quant_luma[64], const uint16_t quant_chroma[64]) {
    for (int k = 0; k < 64; ++k)
        if (quant_luma[k] < 1 || quant_luma[k] > 255 || quant_chroma[k] < 1 || quant_chroma[k] > 255)
            return fail(ctx, MDHIP_EINVAL, "quantisation table entry %d outside 1 .. 255 (baseline JPEG)", k);
    return MDHIP_OK;
}

// The letterbox of `noun` i in two steps, because mdhip_preprocess_windows refuses a host pointer between them:
// the source exists and the resized image lies inside the out_h x out_w network input ...
int check_letterbox_fits(mdhip_ctx* ctx, const char* noun, int i, const uint8_t* src, const mdhip_letterbox& q, int out_h, int out_w) {
    if (!src || q.src_h < 1 || q.src_w < 1 || q.resized_h < 1 || q.resized_w < 1 || q.top < 0 || q.left < 0 ||
        q.top + q.resized_h > out_h || q.left + q.resized_w > out_w)
        return fail(ctx, MDHIP_EINVAL, "%s %d: letterbox geometry does not fit %dx%d", noun, i, out_h, out_w);
    return MDHIP_OK;
}

// ... and the interpolation is one the kernels have: the device record, with the two source steps per output pixel
int build_letterbox(mdhip_ctx* ctx, const char* noun, int i, const uint8_t* src, const mdhip_letterbox& q, LetterboxDev* d) {
    if (q.interp != 0 && q.interp != 1) return fail(ctx, MDHIP_EINVAL, "%s %d: interp %d (0 = linear, 1 = area)", noun, i, q.interp);
    if (q.interp == 1 && (q.resized_h > q.src_h || q.resized_w > q.src_w))
        return fail(ctx, MDHIP_EINVAL, "%s %d: INTER_AREA is implemented for shrinking only", noun, i);
    *d = LetterboxDev{src, q.src_h, q.src_w, q.resized_h, q.resized_w, q.top, q.left, q.interp,
                      1.0 / ((double)q.resized_w / (double)q.src_w), 1.0 / ((double)q.resized_h / (double)q.src_h)};
    return MDHIP_OK;
}

// a scratch layout: parts taken one after the other, each starting on a multiple of 256 bytes
struct ScratchLayout {
    size_t size = 0;
    size_t take(size_t bytes) { const size_t off = size; size = align_up(size + bytes, 256); return off; }
};

// the common end of mdhip_preprocess / mdhip_preprocess_windows: G = LetterboxDev (dense images) or LetterboxWin (windows)
template <class G>
int enqueue_letterbox(mdhip_ctx* ctx, const std::vector<G>& g, int n, int out_h, int out_w, hipStream_t s) {
    // the forward that still reads the input tensor (its stem) comes first, whatever stream it runs on
    if (ctx->input_free_valid) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->input_free, 0));
    if (!letterbox_geometry_travels_inline(g.data(), n, out_w, ctx->letterbox_general)) {
        // geometry goes through a 4-deep pinned ring so that the call never blocks on the stream
        const int slot = ctx->geom_slot;
        ctx->geom_slot = (slot + 1) & 3;
        HIP_TRY(ctx, hipEventSynchronize(ctx->geom_ev[slot]));          // slot's previous copy has completed
        uint8_t* gh = ctx->geom_host + (size_t)slot * ctx->max_batch * sizeof(LetterboxWin);
        memcpy(gh, g.data(), n * sizeof(G));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->arena + ctx->geom_off, gh, n * sizeof(G), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipEventRecord(ctx->geom_ev[slot], s));
    }
    HIP_TRY(ctx, launch_letterbox_s2d((const G*)(ctx->arena + ctx->geom_off), g.data(), n, out_h, out_w,
                                      (uint16_t*)(ctx->arena + ctx->input.off), ctx->dtype == MDHIP_DTYPE_FP16, ctx->letterbox_general, s));
    ctx->last_n = n;
    ctx->last_h = out_h;
    ctx->last_w = out_w;
    return MDHIP_OK;
}

}  // namespace

extern "C" {

int mdhip_preprocess(mdhip_ctx* ctx, const uint8_t* const* images, const mdhip_letterbox* geom,
                     int n, int out_h, int out_w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!images || !geom) return fail(ctx, MDHIP_EINVAL, "images/geom is NULL");
    if (int rc = check_shape(ctx, n, out_h, out_w)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<LetterboxDev> g(n);
    std::vector<long long> stage_off(n, -1);                    // of an image in host memory: where its copy is staged
    ScratchLayout stage;
    for (int i = 0; i < n; ++i) {
        const mdhip_letterbox& q = geom[i];
        if (int rc = check_letterbox_fits(ctx, "image", i, images[i], q, out_h, out_w)) return rc;
        if (!is_device_ptr(images[i])) stage_off[i] = (long long)stage.take((size_t)q.src_h * q.src_w * 3);
        if (int rc = build_letterbox(ctx, "image", i, images[i], q, &g[i])) return rc;
    }
    if (int rc = ctx->stage.reserve(ctx, stage.size, &s)) return rc;
    for (int i = 0; i < n; ++i) {
        if (stage_off[i] < 0) continue;
        g[i].src = (const uint8_t*)(ctx->stage.p + stage_off[i]);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->stage.p + stage_off[i], images[i], (size_t)g[i].src_h * g[i].src_w * 3, hipMemcpyHostToDevice, s));
    }
    return enqueue_letterbox(ctx, g, n, out_h, out_w, s);
}

int mdhip_preprocess_windows(mdhip_ctx* ctx, const uint8_t* const* windows, const mdhip_letterbox* geom,
                             const int64_t* pitches, const int64_t* readable, int n, int out_h, int out_w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!windows || !geom || !pitches || !readable) return fail(ctx, MDHIP_EINVAL, "windows/geom/pitches/readable is NULL");
    if (int rc = check_shape(ctx, n, out_h, out_w)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<LetterboxWin> g(n);
    for (int i = 0; i < n; ++i) {
        const mdhip_letterbox& q = geom[i];
        if (int rc = check_letterbox_fits(ctx, "window", i, windows[i], q, out_h, out_w)) return rc;
        if (!is_device_ptr(windows[i]))
            return fail(ctx, MDHIP_EINVAL, "window %d: host pointer -- a window must point into a device image (upload the parent image "
                        "once and pass pointers into it)", i);
        if (int rc = build_letterbox(ctx, "window", i, windows[i], q, &g[i].d)) return rc;
        // bytes from the window's first pixel to the end of its last row: all must be readable (no limit on a source's sides)
        long long need = 0;
        if (int rc = check_window(ctx, "window", i, q.src_w, q.src_h, pitches[i], INT_MAX, &need)) return rc;
        if (readable[i] < need)
            return fail(ctx, MDHIP_EINVAL, "window %d: %lld readable bytes, the window spans %lld", i, (long long)readable[i], need);
        // (the kernels look at most 16 bytes behind what they use: a larger figure says nothing more, and this one fits 32 bits)
        g[i].readable = std::min<long long>(readable[i], need + 64);
        g[i].pitch = (int)pitches[i];
        g[i].reserved = 0;
    }
    return enqueue_letterbox(ctx, g, n, out_h, out_w, s);
}

int mdhip_jpeg_reconstruct(mdhip_ctx* ctx, const mdhip_jpeg_image* images, int n, uint8_t* const* out_rgb, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!images || !out_rgb) return fail(ctx, MDHIP_EINVAL, "images/out_rgb is NULL");
    if (n < 1) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<JpegDev> devs(n);
    size_t planes_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const mdhip_jpeg_image& q = images[i];
        JpegDev& d = devs[i];
        if (q.width < 1 || q.height < 1 || q.width > 65535 || q.height > 65535 || (q.components != 1 && q.components != 3))
            return fail(ctx, MDHIP_EINVAL, "jpeg image %d: %dx%d with %d components", i, q.width, q.height, q.components);
        const bool samp_ok = q.components == 1 ? (q.h_samp == 1 && q.v_samp == 1)
                                               : ((q.h_samp == 1 && q.v_samp == 1) || (q.h_samp == 2 && q.v_samp == 1) ||
                                                  (q.h_samp == 2 && q.v_samp == 2));
        if (!samp_ok) return fail(ctx, MDHIP_EUNSUPPORTED, "jpeg image %d: luma sampling %dx%d", i, q.h_samp, q.v_samp);
        if (q.rotation != 0 && q.rotation != 90 && q.rotation != 180 && q.rotation != 270)
            return fail(ctx, MDHIP_EINVAL, "jpeg image %d: rotation %d", i, q.rotation);
        // the planes must cover what the kernels read: the luma plane the image, a chroma plane its downsampled size
        long long coef_off = 0;
        for (int c = 0; c < q.components; ++c) {
            const int hs = c == 0 ? 1 : q.h_samp, vs = c == 0 ? 1 : q.v_samp;
            const int need_w = ((q.width + hs - 1) / hs + 7) / 8, need_h = ((q.height + vs - 1) / vs + 7) / 8;
            if (q.blocks_w[c] < need_w || q.blocks_h[c] < need_h || q.blocks_w[c] > 16384 || q.blocks_h[c] > 16384)
                return fail(ctx, MDHIP_EINVAL, "jpeg image %d: plane %d of %dx%d blocks for a %dx%d image", i, c, q.blocks_w[c],
                            q.blocks_h[c], q.width, q.height);
            d.blocks_w[c] = q.blocks_w[c];
            d.blocks_h[c] = q.blocks_h[c];
            d.coef_off[c] = coef_off;
            d.plane_off[c] = (long long)planes_bytes;
            coef_off += (long long)q.blocks_w[c] * q.blocks_h[c] * 64;
            planes_bytes += (size_t)q.blocks_w[c] * q.blocks_h[c] * 64;
        }
        for (int c = q.components; c < 3; ++c) d.blocks_w[c] = d.blocks_h[c] = 0, d.coef_off[c] = d.plane_off[c] = 0;
        planes_bytes = align_up(planes_bytes, 256);
        if (!q.coef || !out_rgb[i] || ((uintptr_t)q.coef & 15))
            return fail(ctx, MDHIP_EINVAL, "jpeg image %d: coef / out_rgb is NULL or coef is not 16-byte aligned", i);
        if (!is_device_ptr(q.coef) || !is_device_ptr(out_rgb[i]))
            return fail(ctx, MDHIP_EINVAL, "jpeg image %d: coef and out_rgb must be device memory", i);
        d.coef = q.coef;
        d.out = out_rgb[i];
        d.width = q.width;
        d.height = q.height;
        d.components = q.components;
        d.h_samp = q.h_samp;
        d.v_samp = q.v_samp;
        d.rotation = q.rotation;
        memcpy(d.quant, q.quant, sizeof(d.quant));
    }
    if (int rc = ctx->jpeg_planes.reserve(ctx, planes_bytes)) return rc;
    for (int i = 0; i < n; ++i) {
        devs[i].planes = (uint8_t*)ctx->jpeg_planes.p;
        HIP_TRY(ctx, launch_jpeg_reconstruct(devs[i], s));
    }
    return MDHIP_OK;
}

int mdhip_jpeg_entropy_decode(mdhip_ctx* ctx, const mdhip_jpeg_scan* scans, int n, int subseq_bits, int32_t* status, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!scans || !status) return fail(ctx, MDHIP_EINVAL, "scans/status is NULL");
    if (n < 1) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    if (subseq_bits == 0) subseq_bits = 1024;
    if (subseq_bits < MDJ_MIN_SUBSEQ_BITS || subseq_bits > MDJ_MAX_SUBSEQ_BITS || subseq_bits % 8)
        return fail(ctx, MDHIP_EINVAL, "subseq_bits = %d (a multiple of 8 from %d to 65536)", subseq_bits, MDJ_MIN_SUBSEQ_BITS);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int chunk = jpeg_entropy_dc_chunk();
    // host image of the scratch: [JpegScanDev x n][status x n][counters][per image: MdjImage, seg_off, seg_lane0 | lane records, energy, dc]
    std::vector<JpegScanDev> devs(n);
    std::vector<MdjImage> ims(n);
    std::vector<std::vector<uint32_t>> seg_off(n), seg_lane0(n);
    struct Off { size_t im, seg_off, seg_lane0, lane_end, lane_start, lane_seg, lane_block, energy, dc_sum, dc_reset; };
    std::vector<Off> offs(n);
    ScratchLayout lay;
    lay.take(sizeof(JpegScanDev) * n);                          // (at offset 0)
    const size_t status_off = lay.take(4 * (size_t)n);
    const size_t counters_off = lay.take(16);
    unsigned max_lanes = 1;
    long long max_chunks = 1, total_lanes = 0;
    for (int i = 0; i < n; ++i) {
        const mdhip_jpeg_scan& q = scans[i];
        if (!q.desc || !q.seg_offsets || !q.scan || !q.coef || ((uintptr_t)q.coef & 15))
            return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: desc / seg_offsets / scan / coef is NULL or coef is not 16-byte aligned", i);
        const mdjpeg_scan_info& sc = *q.desc;
        const mdjpeg_info& in = sc.info;
        const long long bytes = sc.scan_end - sc.scan_begin;
        if (!in.supported || sc.scan_begin < 0 || bytes < 0 || bytes >= MDJ_MAX_SCAN_BYTES)
            return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: scan range %lld .. %lld of a file that is %ssupported", i, (long long)sc.scan_begin,
                        (long long)sc.scan_end, in.supported ? "" : "not ");
        if (!mdj_fill_image(sc, subseq_bits, ims[i]))
            return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: components, sampling or Huffman tables of the descriptor are not valid", i);
        const MdjImage& im = ims[i];
        // the geometry must be the one mdjpeg_parse derives: the kernels' bounds rest on it
        long long count = 0;
        bool ok = in.width >= 1 && in.height >= 1 && in.width <= 65535 && in.height <= 65535 && in.restart_interval >= 0 &&
                  in.mcus_x == (in.width + 8 * in.h_samp[0] - 1) / (8 * in.h_samp[0]) &&
                  in.mcus_y == (in.height + 8 * in.v_samp[0] - 1) / (8 * in.v_samp[0]);
        for (int c = 0; ok && c < in.components; ++c) {
            ok = in.blocks_w[c] == in.mcus_x * in.h_samp[c] && in.blocks_h[c] == in.mcus_y * in.v_samp[c] && in.plane_offset[c] == count;
            count += (long long)in.blocks_w[c] * in.blocks_h[c] * 64;
        }
        if (!ok || count != in.coef_count)
            return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: plane sizes and offsets contradict the image size and sampling", i);
        const long long nseg = (im.total_mcus + im.interval - 1) / im.interval;
        if (nseg != sc.n_segments) return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: %d segments for %lld MCUs at interval %lld", i, sc.n_segments,
                                               (long long)im.total_mcus, (long long)im.interval);
        seg_off[i].resize((size_t)nseg + 1);
        seg_lane0[i].resize((size_t)nseg + 1);
        long long lanes = 0;
        for (long long k = 0; k <= nseg; ++k) {
            const long long o = k < nseg ? (long long)q.seg_offsets[k] : bytes + 2;
            const long long prev = k ? (long long)seg_off[i][(size_t)k - 1] + 2 : 0;
            if (o < prev || o > bytes + 2) return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: segment offset %lld outside the scan or out of order", i, o);
            if (k == 0 && o != 0) return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: the first segment does not begin the scan", i);
            seg_off[i][(size_t)k] = (uint32_t)o;
            if (k) lanes += mdj_lanes_of((uint32_t)(o - 2 - seg_off[i][(size_t)k - 1]), (uint32_t)subseq_bits);
            seg_lane0[i][(size_t)k] = (uint32_t)lanes;
        }
        if (lanes > 0x7fffffffLL) return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: too many subsequences", i);
        if (!is_device_ptr(q.scan) || !is_device_ptr(q.coef))
            return fail(ctx, MDHIP_EINVAL, "jpeg scan %d: scan and coef must be device memory", i);
        JpegScanDev& d = devs[i];
        d.scan = q.scan;
        d.coef = q.coef;
        d.coef_count = in.coef_count;
        d.n_segments = (uint32_t)nseg;
        d.n_lanes = (uint32_t)lanes;
        long long chunks = 0;
        for (int c = 0; c < 3; ++c) {
            d.dc_blocks[c] = c < in.components ? (long long)in.blocks_w[c] * in.blocks_h[c] : 0;
            d.dc_chunks[c] = (d.dc_blocks[c] + chunk - 1) / chunk;
            chunks += d.dc_chunks[c];
        }
        max_lanes = std::max(max_lanes, d.n_lanes);
        max_chunks = std::max(max_chunks, chunks);
        total_lanes += lanes;
        Off& o = offs[i];
        o.im = lay.take(sizeof(MdjImage));
        o.seg_off = lay.take(4 * ((size_t)nseg + 1));
        o.seg_lane0 = lay.take(4 * ((size_t)nseg + 1));
    }
    const size_t upload_bytes = lay.size;                       // what follows is written on the device before it is read
    for (int i = 0; i < n; ++i) {
        Off& o = offs[i];
        const size_t lanes = devs[i].n_lanes, blocks = (size_t)(devs[i].coef_count / 64);
        const size_t chunks = (size_t)(devs[i].dc_chunks[0] + devs[i].dc_chunks[1] + devs[i].dc_chunks[2]);
        o.lane_end = lay.take(8 * lanes);
        o.lane_start = lay.take(8 * lanes);
        o.lane_seg = lay.take(4 * lanes);
        o.lane_block = lay.take(4 * lanes);
        o.energy = lay.take(4 * blocks);
        o.dc_sum = lay.take(8 * chunks);
        o.dc_reset = lay.take(4 * chunks);
    }
    if (int rc = ctx->jpeg_entropy.reserve(ctx, lay.size)) return rc;
    char* base = ctx->jpeg_entropy.p;
    std::vector<char> up(upload_bytes, 0);
    for (int i = 0; i < n; ++i) {
        const Off& o = offs[i];
        JpegScanDev& d = devs[i];
        d.im = (const MdjImage*)(base + o.im);
        d.seg_off = (const uint32_t*)(base + o.seg_off);
        d.seg_lane0 = (const uint32_t*)(base + o.seg_lane0);
        d.lane_end = (uint64_t*)(base + o.lane_end);
        d.lane_start = (uint64_t*)(base + o.lane_start);
        d.lane_seg = (uint32_t*)(base + o.lane_seg);
        d.lane_block = (uint32_t*)(base + o.lane_block);
        d.energy = (uint32_t*)(base + o.energy);
        d.dc_sum = (long long*)(base + o.dc_sum);
        d.dc_reset = (uint32_t*)(base + o.dc_reset);
        memcpy(up.data() + o.im, &ims[i], sizeof(MdjImage));
        memcpy(up.data() + o.seg_off, seg_off[i].data(), 4 * seg_off[i].size());
        memcpy(up.data() + o.seg_lane0, seg_lane0[i].data(), 4 * seg_lane0[i].size());
    }
    memcpy(up.data(), devs.data(), sizeof(JpegScanDev) * n);
    // (the upload is from pageable memory: the copy has left `up` when the call returns; status and counters arrive zeroed)
    HIP_TRY(ctx, hipMemcpyAsync(base, up.data(), upload_bytes, hipMemcpyHostToDevice, s));
    const JpegScanDev* ddevs = (const JpegScanDev*)base;
    uint32_t* dstatus = (uint32_t*)(base + status_off);
    unsigned long long* dcounters = (unsigned long long*)(base + counters_off);
    launch_jpeg_entropy_front(ddevs, n, max_lanes, s);
    HIP_TRY(ctx, hipGetLastError());
    // pass 2: until a launch moves no lane.  Every launch settles whole workgroups, so this is two launches unless a change
    // has to cross workgroups; a chain of lanes that never meet is bounded by the number of lanes.
    long long launches = 0;
    unsigned long long counters[2] = {0, 0};
    for (;;) {
        launch_jpeg_entropy_sync(ddevs, n, max_lanes, dcounters, s);
        HIP_TRY(ctx, hipGetLastError());
        ++launches;
        HIP_TRY(ctx, hipMemcpyAsync(counters, dcounters, sizeof(counters), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemsetAsync(dcounters + 1, 0, 8, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        if (!counters[1]) break;
        if (launches > (long long)max_lanes + 2) return fail(ctx, MDHIP_EHIP, "the subsequences did not synchronise in %lld launches", launches);
    }
    launch_jpeg_entropy_back(ddevs, n, max_lanes, max_chunks, dstatus, s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(status, dstatus, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->jpeg_entropy_stats[0] = total_lanes;
    ctx->jpeg_entropy_stats[1] = (long long)counters[0];
    ctx->jpeg_entropy_stats[2] = launches;
    ctx->jpeg_entropy_stats[3] = n;
    return MDHIP_OK;
}

int mdhip_jpeg_entropy_stats(mdhip_ctx* ctx, int64_t out[4]) {
    if (!ctx) return MDHIP_EINVAL;
    if (!out) return fail(ctx, MDHIP_EINVAL, "out is NULL");
    for (int i = 0; i < 4; ++i) out[i] = ctx->jpeg_entropy_stats[i];
    return MDHIP_OK;
}

int mdhip_jpeg_recompress(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                          const int64_t* pitches, int n, const uint16_t quant_luma[64], const uint16_t quant_chroma[64],
                          uint8_t* const* out_rgb, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!windows || !widths || !heights || !pitches || !quant_luma || !quant_chroma || !out_rgb)
        return fail(ctx, MDHIP_EINVAL, "windows/widths/heights/pitches/quant_luma/quant_chroma/out_rgb is NULL");
    if (n < 1) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    if (int rc = check_quant_tables(ctx, quant_luma, quant_chroma)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<JpegDev> devs(n);
    size_t planes_bytes = 0;
    for (int i = 0; i < n; ++i) {
        JpegDev& d = devs[i];
        const int w = widths[i], h = heights[i];
        if (int rc = check_window(ctx, "window", i, w, h, pitches[i])) return rc;
        if (!windows[i] || !out_rgb[i]) return fail(ctx, MDHIP_EINVAL, "window %d: windows / out_rgb is NULL", i);
        if (!is_device_ptr(windows[i]) || !is_device_ptr(out_rgb[i]))
            return fail(ctx, MDHIP_EINVAL, "window %d: host pointer -- windows and out_rgb must be device memory", i);
        d.coef = nullptr;
        d.out = out_rgb[i];
        d.width = w;
        d.height = h;
        d.components = 3;
        d.h_samp = d.v_samp = 2;
        d.rotation = 0;
        for (int c = 0; c < 3; ++c) {                                   // each component's own whole blocks (4:2:0)
            const int cw = c == 0 ? w : (w + 1) / 2, ch = c == 0 ? h : (h + 1) / 2;
            d.blocks_w[c] = (cw + 7) / 8;
            d.blocks_h[c] = (ch + 7) / 8;
            d.coef_off[c] = 0;
            d.plane_off[c] = (long long)planes_bytes;
            planes_bytes += (size_t)d.blocks_w[c] * d.blocks_h[c] * 64;
            memcpy(d.quant[c], c == 0 ? quant_luma : quant_chroma, sizeof(d.quant[c]));
        }
        planes_bytes = align_up(planes_bytes, 256);
    }
    if (int rc = ctx->jpeg_planes.reserve(ctx, planes_bytes)) return rc;
    for (int i = 0; i < n; ++i) {
        devs[i].planes = (uint8_t*)ctx->jpeg_planes.p;
        HIP_TRY(ctx, launch_jpeg_recompress(devs[i], windows[i], pitches[i], s));
    }
    return MDHIP_OK;
}

long long mdhip_jpeg_encode_bound(int width, int height) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return -1;
    return mdj_enc_bound_bytes(width, height);
}

long long mdhip_jpeg_encode_sampled_bound(int width, int height, int sampling) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || !mdj_enc_sampling_ok(sampling)) return -1;
    return mdj_enc_bound_bytes(width, height, sampling);
}

namespace {

// what mdhip_jpeg_encode_kept adds to a call
struct JpegKeepArgs {
    const mdhip_jpeg_source* sources;
    const int32_t* rect_image;
    const int32_t* rects;
    int n_rects;
    int32_t* status;
};

// mdhip_jpeg_encode, mdhip_jpeg_encode_sampled and mdhip_jpeg_encode_kept.  samplings NULL: h2v2 for every window; quant:
// n_tables pairs [luma 64][chroma 64], window i takes pair i when there are n of them and pair 0 when there is one; keep
// NULL: every block comes from the pixels.
int jpeg_encode_windows(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                        const int64_t* pitches, const int32_t* samplings, int n, const uint16_t* quant, int n_tables, uint8_t* out,
                        int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, void* hip_stream,
                        const JpegKeepArgs* keep = nullptr) {
    if (n < 1) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    if (keep) {
        if (keep->n_rects < 0) return fail(ctx, MDHIP_EINVAL, "n_rects = %d", keep->n_rects);
        for (int i = 0; i < keep->n_rects; ++i)
            if (keep->rect_image[i] < 0 || keep->rect_image[i] >= n)
                return fail(ctx, MDHIP_EINVAL, "rectangle %d: window %d of %d", i, keep->rect_image[i], n);
    }
    if (capacity < 0 || (capacity > 0 && !out)) return fail(ctx, MDHIP_EINVAL, "capacity %lld with out %p", (long long)capacity, (void*)out);
    for (int t = 0; t < n_tables; ++t)
        if (int rc = check_quant_tables(ctx, quant + 128 * (size_t)t, quant + 128 * (size_t)t + 64)) return rc;
    if (samplings)
        for (int i = 0; i < n; ++i)
            if (!mdj_enc_sampling_ok(samplings[i]))
                return fail(ctx, MDHIP_EINVAL, "window %d: sampling %d is none of h1v1 (0), h2v1 (1), h2v2 (2)", i, samplings[i]);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (capacity > 0 && !is_device_ptr(out)) return fail(ctx, MDHIP_EINVAL, "host pointer -- out must be device memory");
    const int chunk_bytes = 64;
    std::vector<MdjEncCrop> crops((size_t)n + 1);
    long long blocks = 0, words = 0, chunks = 0;
    for (int i = 0; i <= n; ++i) {
        MdjEncCrop& c = crops[i];
        memset(&c, 0, sizeof(c));
        c.block0 = blocks;
        c.word0 = words;
        c.chunk0 = chunks;
        if (i == n) break;
        const int w = widths[i], h = heights[i];
        if (int rc = check_window(ctx, "window", i, w, h, pitches[i])) return rc;
        if (!windows[i] || !is_device_ptr(windows[i])) return fail(ctx, MDHIP_EINVAL, "window %d: NULL or a host pointer -- windows must be device memory", i);
        const int sampling = samplings ? samplings[i] : MDJ_ENC_H2V2;
        const long long nb = mdj_enc_blocks(w, h, sampling);
        if (nb > MDJ_ENC_MAX_BLOCKS) return fail(ctx, MDHIP_EINVAL, "window %d: %dx%d is more than %lld blocks", i, w, h, (long long)MDJ_ENC_MAX_BLOCKS);
        c.src = windows[i];
        c.pitch = pitches[i];
        mdj_enc_set_layout(c, w, h, sampling);
        c.table = n_tables == 1 ? 0 : i;
        if (keep) {                                                     // the source's planes: the window's whole MCUs, on the device
            const mdhip_jpeg_source& src = keep->sources[i];
            for (int p = 0; p < 3; ++p)
                if (src.blocks_w[p] != c.mcus_x * (p == 0 ? c.hs : 1) || src.blocks_h[p] != c.mcus_y * (p == 0 ? c.vs : 1))
                    return fail(ctx, MDHIP_EINVAL, "window %d: plane %d of the source is %d x %d blocks, the window's MCUs make it %d x %d", i,
                                p, src.blocks_w[p], src.blocks_h[p], c.mcus_x * (p == 0 ? c.hs : 1), c.mcus_y * (p == 0 ? c.vs : 1));
            if (!src.coef || (reinterpret_cast<uintptr_t>(src.coef) & 15) || !is_device_ptr(src.coef))
                return fail(ctx, MDHIP_EINVAL, "window %d: the source's planes are NULL, not 16-byte aligned or a host pointer", i);
        }
        blocks += nb;
        words += mdj_enc_region_words(nb);
        chunks += mdj_enc_region_chunks(nb, chunk_bytes);
    }
    // the scratch: [crops][tables][quant] uploaded; [status][bit buffer] zeroed; the rest written before it is read
    ScratchLayout lay;
    const size_t o_crops = lay.take(sizeof(MdjEncCrop) * ((size_t)n + 1));
    const size_t o_tables = lay.take(sizeof(MdjEncTables));
    const size_t o_quant = lay.take(256 * (size_t)n_tables);
    // mdhip_jpeg_encode_kept: the rectangles clipped to their windows, window by window in the order of the list
    std::vector<MdjKeepRect> kept_rects;
    std::vector<int32_t> rect0;
    if (keep) {
        rect0.assign((size_t)n + 1, 0);
        std::vector<std::vector<MdjKeepRect>> per((size_t)n);
        for (int i = 0; i < keep->n_rects; ++i) {
            const int w = keep->rect_image[i];
            MdjKeepRect q;
            if (mdj_keep_clip(keep->rects + 4 * (size_t)i, widths[w], heights[w], &q)) per[(size_t)w].push_back(q);
        }
        for (int i = 0; i < n; ++i) {
            rect0[(size_t)i] = (int32_t)kept_rects.size();
            kept_rects.insert(kept_rects.end(), per[(size_t)i].begin(), per[(size_t)i].end());
        }
        rect0[(size_t)n] = (int32_t)kept_rects.size();
    }
    const size_t o_source = lay.take(keep ? sizeof(const int16_t*) * (size_t)n : 0);
    const size_t o_rect0 = lay.take(keep ? 4 * ((size_t)n + 1) : 0);
    const size_t o_rects = lay.take(sizeof(MdjKeepRect) * kept_rects.size());
    const size_t upload_bytes = lay.size;
    const size_t o_status = lay.take(4 * (size_t)n);
    const size_t o_bitbuf = lay.take(4 * (size_t)words);
    const size_t zero_bytes = lay.size - o_status;
    const size_t o_coef = lay.take(128 * (size_t)blocks);
    const size_t o_len = lay.take(4 * (size_t)blocks);
    const size_t o_off = lay.take(8 * ((size_t)blocks + 1));
    const size_t o_partial = lay.take(8 * (size_t)std::max(jpeg_encode_scan_tiles(blocks), jpeg_encode_scan_tiles(chunks)));
    const size_t o_count = lay.take(4 * (size_t)chunks);
    const size_t o_start = lay.take(8 * ((size_t)chunks + 1));
    const size_t o_result = lay.take(8 * (2 * (size_t)n + 1));
    if (int rc = ctx->jpeg_encode.reserve(ctx, lay.size)) return rc;
    char* base = ctx->jpeg_encode.p;
    std::vector<char> up(upload_bytes, 0);
    memcpy(up.data() + o_crops, crops.data(), sizeof(MdjEncCrop) * ((size_t)n + 1));
    MdjEncTables tables;
    mdj_enc_build_tables(tables);
    memcpy(up.data() + o_tables, &tables, sizeof(tables));
    memcpy(up.data() + o_quant, quant, 256 * (size_t)n_tables);
    if (keep) {
        for (int i = 0; i < n; ++i) memcpy(up.data() + o_source + sizeof(const int16_t*) * (size_t)i, &keep->sources[i].coef, sizeof(const int16_t*));
        memcpy(up.data() + o_rect0, rect0.data(), 4 * rect0.size());
        if (!kept_rects.empty()) memcpy(up.data() + o_rects, kept_rects.data(), sizeof(MdjKeepRect) * kept_rects.size());
    }
    // (the upload is from pageable memory: the copy has left `up` when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(base, up.data(), upload_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(base + o_status, 0, zero_bytes, s));
    JpegEncDev d;
    d.crops = (const MdjEncCrop*)(base + o_crops);
    d.tables = (const MdjEncTables*)(base + o_tables);
    d.quant = (const uint16_t*)(base + o_quant);
    d.coef = (int16_t*)(base + o_coef);
    d.len = (uint32_t*)(base + o_len);
    d.off = (uint64_t*)(base + o_off);
    d.partial = (uint64_t*)(base + o_partial);
    d.bitbuf = (uint32_t*)(base + o_bitbuf);
    d.count = (uint32_t*)(base + o_count);
    d.start = (uint64_t*)(base + o_start);
    d.status = (uint32_t*)(base + o_status);
    d.result = (long long*)(base + o_result);
    d.out = out;
    d.capacity = capacity;
    d.blocks = blocks;
    d.chunks = chunks;
    d.n = n;
    d.chunk_bytes = chunk_bytes;
    d.source = keep ? (const int16_t* const*)(base + o_source) : nullptr;
    d.rects = (const MdjKeepRect*)(base + o_rects);
    d.rect0 = (const int32_t*)(base + o_rect0);
    HIP_TRY(ctx, launch_jpeg_encode(d, s));
    std::vector<long long> result(2 * (size_t)n + 1);
    std::vector<uint32_t> status((size_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(result.data(), d.result, 8 * result.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(status.data(), d.status, 4 * status.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        offsets[i] = result[i];
        sizes[i] = result[(size_t)n + i];
    }
    *needed = result[2 * (size_t)n];
    if (keep)                                                           // a flagged window has no scan; the others are whole
        for (int i = 0; i < n; ++i) keep->status[i] = status[i] ? 1 : 0;
    for (int i = 0; i < n && !keep; ++i)
        if (status[i]) return fail(ctx, MDHIP_EINVAL, "window %d: a coefficient no baseline JPEG can hold (status %u)", i, status[i]);
    if (*needed > capacity)
        return fail(ctx, MDHIP_ECAPACITY, "the scans take %lld bytes, the output buffer has %lld", (long long)*needed, (long long)capacity);
    return MDHIP_OK;
}

}  // namespace

int mdhip_jpeg_encode(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                      const int64_t* pitches, int n, const uint16_t quant_luma[64], const uint16_t quant_chroma[64], uint8_t* out,
                      int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!windows || !widths || !heights || !pitches || !quant_luma || !quant_chroma || !offsets || !sizes || !needed)
        return fail(ctx, MDHIP_EINVAL, "windows/widths/heights/pitches/quant_luma/quant_chroma/offsets/sizes/needed is NULL");
    uint16_t pair[128];
    memcpy(pair, quant_luma, 128);
    memcpy(pair + 64, quant_chroma, 128);
    return jpeg_encode_windows(ctx, windows, widths, heights, pitches, nullptr, n, pair, 1, out, capacity, offsets, sizes, needed, hip_stream);
}

int mdhip_jpeg_encode_sampled(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                              const int64_t* pitches, const int32_t* samplings, int n, const uint16_t* quant, uint8_t* out,
                              int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!windows || !widths || !heights || !pitches || !samplings || !quant || !offsets || !sizes || !needed)
        return fail(ctx, MDHIP_EINVAL, "windows/widths/heights/pitches/samplings/quant/offsets/sizes/needed is NULL");
    return jpeg_encode_windows(ctx, windows, widths, heights, pitches, samplings, n, quant, n, out, capacity, offsets, sizes, needed, hip_stream);
}

int mdhip_jpeg_encode_kept(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                           const int64_t* pitches, const int32_t* samplings, int n, const uint16_t* quant,
                           const mdhip_jpeg_source* sources, const int32_t* rect_image, const int32_t* rects, int n_rects, uint8_t* out,
                           int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, int32_t* status, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!windows || !widths || !heights || !pitches || !samplings || !quant || !sources || !offsets || !sizes || !needed || !status ||
        (n_rects > 0 && (!rect_image || !rects)))
        return fail(ctx, MDHIP_EINVAL, "windows/widths/heights/pitches/samplings/quant/sources/rect_image/rects/offsets/sizes/needed/status is NULL");
    const JpegKeepArgs keep = {sources, rect_image, rects, n_rects, status};
    return jpeg_encode_windows(ctx, windows, widths, heights, pitches, samplings, n, quant, n, out, capacity, offsets, sizes, needed, hip_stream,
                               &keep);
}

int mdhip_blur_regions(mdhip_ctx* ctx, uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                       int n_images, const int32_t* rect_image, const int32_t* rects, int n_rects, float radius, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (n_rects == 0) return MDHIP_OK;
    if (!images || !widths || !heights || !pitches || !rect_image || !rects)
        return fail(ctx, MDHIP_EINVAL, "images/widths/heights/pitches/rect_image/rects is NULL");
    if (n_images < 1 || n_images > 65535 || n_rects < 0) return fail(ctx, MDHIP_EINVAL, "n_images = %d, n_rects = %d", n_images, n_rects);
    if (!(radius >= 0.0f) || radius > MD_BLUR_MAX_RADIUS) return fail(ctx, MDHIP_EINVAL, "radius %g outside 0 .. %g", (double)radius, (double)MD_BLUR_MAX_RADIUS);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const MdBlurWeights wt = md_blur_weights(radius);
    // every rectangle is checked before anything is launched; round k holds the k-th rectangle with area of every image
    std::vector<int> seen((size_t)n_images, -1), count((size_t)n_images, 0);
    std::vector<std::vector<BlurRect>> rounds;
    for (int i = 0; i < n_rects; ++i) {
        const int m = rect_image[i];
        if (m < 0 || m >= n_images) return fail(ctx, MDHIP_EINVAL, "rectangle %d: image %d of %d", i, m, n_images);
        const int32_t* q = rects + 4 * (size_t)i;
        if (q[2] <= q[0] || q[3] <= q[1]) continue;                     // without area: Pillow pastes nothing
        if (seen[m] < 0) {
            const int W = widths[m], H = heights[m];
            if (int rc = check_window(ctx, "image", m, W, H, pitches[m])) return rc;
            if (!images[m] || !is_device_ptr(images[m]))
                return fail(ctx, MDHIP_EINVAL, "image %d: NULL or a host pointer -- images must be device memory", m);
            seen[m] = 1;
        }
        if (q[0] < 0 || q[1] < 0 || q[2] > widths[m] || q[3] > heights[m])
            return fail(ctx, MDHIP_EINVAL, "rectangle %d: (%d, %d, %d, %d) leaves its %dx%d image", i, q[0], q[1], q[2], q[3], widths[m], heights[m]);
        BlurRect d;
        memset(&d, 0, sizeof(d));
        d.img = images[m] + (long long)q[1] * pitches[m] + (long long)q[0] * 3;
        d.pitch = pitches[m];
        d.w = q[2] - q[0];
        d.h = q[3] - q[1];
        d.sp = (int)align_up((size_t)d.w * 3, 64);
        MdBlurXPlan plan;
        if (!md_blur_plan_x(d.w, wt.r, BLUR_LDS_BYTES, &plan) || (long long)plan.rows * plan.stride * 2 > BLUR_LDS_BYTES)
            return fail(ctx, MDHIP_EUNSUPPORTED, "rectangle %d: no row plan for %d pixels at box radius %d", i, d.w, wt.r);
        d.rows = plan.rows, d.stride = plan.stride, d.chunks = plan.chunks, d.step = plan.step, d.halo = plan.halo;
        d.row_groups = (d.h + d.rows - 1) / d.rows;
        const size_t k = (size_t)count[m]++;
        if (rounds.size() <= k) rounds.resize(k + 1);
        rounds[k].push_back(d);
    }
    if (rounds.empty()) return MDHIP_OK;
    // the scratch: [records of all rounds][planes of one round]; the rounds run one after the other and share the planes
    size_t n_records = 0, plane_bytes = 0;
    for (auto& round : rounds) {
        ScratchLayout planes;
        for (BlurRect& d : round) {
            d.s0 = (long long)planes.take((size_t)d.sp * (size_t)d.h);
            d.s1 = (long long)planes.take((size_t)d.sp * (size_t)d.h);
        }
        plane_bytes = std::max(plane_bytes, planes.size);
        n_records += round.size();
    }
    const size_t o_planes = align_up(sizeof(BlurRect) * n_records, 256);
    const size_t total = o_planes + plane_bytes;
    if (int rc = ctx->blur.reserve(ctx, total)) return rc;
    std::vector<BlurRect> up;
    up.reserve(n_records);
    for (auto& round : rounds) up.insert(up.end(), round.begin(), round.end());
    // (the upload is from pageable memory: the copy has left `up` when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->blur.p, up.data(), sizeof(BlurRect) * n_records, hipMemcpyHostToDevice, s));
    size_t first = 0;
    for (auto& round : rounds) {
        int max_blocks = 1, max_width = 1;
        for (const BlurRect& d : round) {
            max_blocks = std::max(max_blocks, d.row_groups * d.chunks);
            max_width = std::max(max_width, d.w);
        }
        HIP_TRY(ctx, launch_blur_round((const BlurRect*)ctx->blur.p + first, (int)round.size(), max_blocks, max_width,
                                       (uint8_t*)ctx->blur.p + o_planes, wt.r, wt.ww, wt.fw, s));
        first += round.size();
    }
    return MDHIP_OK;
}

int mdhip_resample_lanczos(mdhip_ctx* ctx, const uint8_t* const* src, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                           int n, uint8_t* const* dst, const int32_t* dst_widths, const int32_t* dst_heights, const int64_t* dst_pitches,
                           void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (n == 0) return MDHIP_OK;
    if (!src || !widths || !heights || !pitches || !dst || !dst_widths || !dst_heights || !dst_pitches)
        return fail(ctx, MDHIP_EINVAL, "src/widths/heights/pitches/dst/dst_widths/dst_heights/dst_pitches is NULL");
    if (n < 1 || n > 65535) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // every image is checked and planned before anything is enqueued; one coefficient table per distinct (in, out) pair
    struct Coeffs { int ksize, bounds_off, kk_off; };
    std::map<std::pair<int, int>, Coeffs> pairs;
    std::vector<int32_t> table;
    std::vector<double> work;
    auto coeffs = [&](int in, int out) -> Coeffs {
        auto it = pairs.find({in, out});
        if (it != pairs.end()) return it->second;
        Coeffs c;
        c.ksize = md_resample_ksize(in, out);
        c.bounds_off = (int)table.size();
        c.kk_off = c.bounds_off + 2 * out;
        table.resize(table.size() + 2 * (size_t)out + (size_t)out * c.ksize);
        work.resize((size_t)c.ksize);
        md_resample_coeffs(in, out, c.ksize, table.data() + c.bounds_off, table.data() + c.kk_off, work.data());
        pairs[{in, out}] = c;
        return c;
    };
    std::vector<ResampleRows> rows;
    std::vector<ResampleColumns> columns;
    std::vector<int> copies;
    std::vector<long long> between((size_t)n, -1);                      // of an image that takes both passes: its 8-bit image between them
    ScratchLayout planes;
    for (int i = 0; i < n; ++i) {
        const int sw = widths[i], sh = heights[i], dw = dst_widths[i], dh = dst_heights[i];
        if (int rc = check_window(ctx, "source", i, sw, sh, pitches[i])) return rc;
        if (int rc = check_window(ctx, "destination", i, dw, dh, dst_pitches[i])) return rc;
        if (!src[i] || !dst[i] || !is_device_ptr(src[i]) || !is_device_ptr(dst[i]))
            return fail(ctx, MDHIP_EINVAL, "image %d: NULL or a host pointer -- sources and destinations must be device memory", i);
        const bool horizontal = dw != sw, vertical = dh != sh;
        if (!horizontal && !vertical) { copies.push_back(i); continue; }
        const int tmp_pitch = (int)align_up((size_t)dw * 3, 16);
        if (horizontal && vertical) between[i] = (long long)planes.take((size_t)tmp_pitch * (size_t)sh);
        if (horizontal) {
            const Coeffs c = coeffs(sw, dw);
            MdResampleStrips plan;
            if (!md_resample_plan_strips(table.data() + c.bounds_off, dw, MD_RESAMPLE_LDS_BYTES, &plan))
                return fail(ctx, MDHIP_EUNSUPPORTED, "image %d: the taps of one pixel of %d -> %d pixels do not fit on chip", i, sw, dw);
            ResampleRows d;
            memset(&d, 0, sizeof(d));
            d.src = src[i], d.src_pitch = pitches[i];
            d.dst = vertical ? nullptr : dst[i], d.dst_pitch = vertical ? tmp_pitch : dst_pitches[i];
            d.rows = sh, d.out_w = dw, d.ksize = c.ksize, d.bounds_off = c.bounds_off, d.kk_off = c.kk_off;
            d.strip = plan.strip, d.wg_rows = plan.rows, d.run_bytes = plan.run_bytes;
            d.strips = (dw + plan.strip - 1) / plan.strip;
            d.row_groups = (sh + plan.rows - 1) / plan.rows;
            if ((long long)d.strips * d.row_groups > 0x7fffffffLL) return fail(ctx, MDHIP_EUNSUPPORTED, "image %d: too many strips", i);
            rows.push_back(d);
        }
        if (vertical) {
            const Coeffs c = coeffs(sh, dh);
            ResampleColumns d;
            memset(&d, 0, sizeof(d));
            d.src = horizontal ? nullptr : src[i], d.src_pitch = horizontal ? tmp_pitch : pitches[i];
            d.dst = dst[i], d.dst_pitch = dst_pitches[i];
            d.row_bytes = dw * 3, d.out_h = dh, d.ksize = c.ksize, d.bounds_off = c.bounds_off, d.kk_off = c.kk_off;
            d.pad = i;                                                  // (the image, until the scratch is laid out)
            columns.push_back(d);
        }
    }
    for (int i : copies)
        HIP_TRY(ctx, hipMemcpy2DAsync(dst[i], (size_t)dst_pitches[i], src[i], (size_t)pitches[i], (size_t)widths[i] * 3, (size_t)heights[i],
                                      hipMemcpyDeviceToDevice, s));
    if (rows.empty() && columns.empty()) return MDHIP_OK;
    // the scratch: [coefficient tables][records of the rows pass][records of the columns pass][images between the passes]
    ScratchLayout lay;
    const size_t o_table = lay.take(table.size() * sizeof(int32_t));
    const size_t o_rows = lay.take(rows.size() * sizeof(ResampleRows));
    const size_t o_columns = lay.take(columns.size() * sizeof(ResampleColumns));
    const size_t o_planes = lay.take(planes.size);
    if (int rc = ctx->resample.reserve(ctx, lay.size)) return rc;
    uint8_t* base = (uint8_t*)ctx->resample.p;
    {
        size_t r = 0;
        for (int i = 0, c = 0; i < n; ++i) {
            const bool horizontal = dst_widths[i] != widths[i], vertical = dst_heights[i] != heights[i];
            if (horizontal && vertical) rows[r].dst = base + o_planes + between[i];
            if (horizontal) ++r;
            if (vertical) {
                if (horizontal) columns[c].src = base + o_planes + between[i];
                columns[c].pad = 0;
                ++c;
            }
        }
    }
    // (the uploads are from pageable memory: the copies have left the vectors when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(base + o_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (!rows.empty()) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_rows, rows.data(), rows.size() * sizeof(ResampleRows), hipMemcpyHostToDevice, s));
        int max_blocks = 1;
        for (const ResampleRows& d : rows) max_blocks = std::max(max_blocks, d.strips * d.row_groups);
        HIP_TRY(ctx, launch_resample_rows((const ResampleRows*)(base + o_rows), (int)rows.size(), max_blocks, (const int32_t*)(base + o_table), s));
    }
    if (!columns.empty()) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_columns, columns.data(), columns.size() * sizeof(ResampleColumns), hipMemcpyHostToDevice, s));
        int max_row_bytes = 1, max_out_h = 1;
        for (const ResampleColumns& d : columns) {
            max_row_bytes = std::max(max_row_bytes, d.row_bytes);
            max_out_h = std::max(max_out_h, d.out_h);
        }
        HIP_TRY(ctx, launch_resample_columns((const ResampleColumns*)(base + o_columns), (int)columns.size(), max_row_bytes, max_out_h,
                                             (const int32_t*)(base + o_table), s));
    }
    return MDHIP_OK;
}

int mdhip_draw_ops(mdhip_ctx* ctx, uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                   int n_images, const int32_t* op_image, const int32_t* ops, int n_ops, const uint8_t* patches, int64_t patch_bytes,
                   void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (n_ops == 0) return MDHIP_OK;
    if (!images || !widths || !heights || !pitches || !op_image || !ops)
        return fail(ctx, MDHIP_EINVAL, "images/widths/heights/pitches/op_image/ops is NULL");
    if (n_images < 1 || n_images > 65535 || n_ops < 0 || patch_bytes < 0 || patch_bytes > 0x7fff0000LL)
        return fail(ctx, MDHIP_EINVAL, "n_images = %d, n_ops = %d, patch_bytes = %lld", n_images, n_ops, (long long)patch_bytes);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // every operation is checked before anything is launched; an image's operations keep the order of the list
    std::vector<int> count((size_t)n_images, 0);
    bool any_patch = false;
    for (int i = 0; i < n_ops; ++i) {
        const int m = op_image[i];
        if (m < 0 || m >= n_images) return fail(ctx, MDHIP_EINVAL, "operation %d: image %d of %d", i, m, n_images);
        const int32_t* op = ops + (size_t)i * MD_DRAW_OP_WORDS;
        if (md_draw_op_bad(op, patch_bytes))
            return fail(ctx, MDHIP_EINVAL, "operation %d: kind %d, or a patch of %dx%d pixels at byte %d of %lld", i, op[0], op[3], op[4], op[5],
                        (long long)patch_bytes);
        any_patch |= op[0] == MD_DRAW_PATCH && op[3] > 0 && op[4] > 0;
        ++count[m];
    }
    if (any_patch && (!patches || !is_device_ptr(patches))) return fail(ctx, MDHIP_EINVAL, "patches: NULL or a host pointer");
    std::vector<DrawImage> recs;
    std::vector<int> rec_of((size_t)n_images, -1), fill((size_t)n_images, 0);
    int first = 0;
    for (int m = 0; m < n_images; ++m) {
        if (!count[m]) continue;
        if (int rc = check_window(ctx, "image", m, widths[m], heights[m], pitches[m])) return rc;
        if (!images[m] || !is_device_ptr(images[m]))
            return fail(ctx, MDHIP_EINVAL, "image %d: NULL or a host pointer -- images must be device memory", m);
        DrawImage d;
        memset(&d, 0, sizeof(d));
        d.img = images[m], d.pitch = pitches[m];
        d.x0 = widths[m], d.y0 = heights[m], d.x1 = -1, d.y1 = -1;
        d.op_first = first, d.op_count = count[m];
        first += count[m];
        rec_of[m] = (int)recs.size();
        recs.push_back(d);
    }
    std::vector<int32_t> sorted((size_t)n_ops * MD_DRAW_OP_WORDS);
    for (int i = 0; i < n_ops; ++i) {
        const int m = op_image[i];
        DrawImage& d = recs[(size_t)rec_of[m]];
        const int32_t* op = ops + (size_t)i * MD_DRAW_OP_WORDS;
        memcpy(sorted.data() + (size_t)(d.op_first + fill[m]++) * MD_DRAW_OP_WORDS, op, sizeof(int32_t) * MD_DRAW_OP_WORDS);
        // what the operation covers, clipped to the image (64-bit: a corner plus a size may pass 2^31)
        long long a = op[1], b = op[2], c = op[3], e = op[4];
        if (op[0] == MD_DRAW_PATCH) c = a + c - 1, e = b + e - 1;
        a = std::max(a, 0LL), b = std::max(b, 0LL);
        c = std::min(c, (long long)widths[m] - 1), e = std::min(e, (long long)heights[m] - 1);
        if (c < a || e < b) continue;
        d.x0 = std::min(d.x0, (int)a), d.y0 = std::min(d.y0, (int)b), d.x1 = std::max(d.x1, (int)c), d.y1 = std::max(d.y1, (int)e);
    }
    int max_w = 0, max_h = 0;
    for (const DrawImage& d : recs) {
        max_w = std::max(max_w, d.x1 - d.x0 + 1);
        max_h = std::max(max_h, d.y1 - d.y0 + 1);
    }
    if (max_w < 1 || max_h < 1) return MDHIP_OK;                         // nothing of any operation lies in its image
    ScratchLayout lay;
    const size_t o_recs = lay.take(recs.size() * sizeof(DrawImage));
    const size_t o_ops = lay.take(sorted.size() * sizeof(int32_t));
    if (int rc = ctx->draw.reserve(ctx, lay.size)) return rc;
    uint8_t* base = (uint8_t*)ctx->draw.p;
    HIP_TRY(ctx, hipMemcpyAsync(base + o_recs, recs.data(), recs.size() * sizeof(DrawImage), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_ops, sorted.data(), sorted.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_draw_ops((const DrawImage*)(base + o_recs), (int)recs.size(), max_w, max_h, (const int32_t*)(base + o_ops), patches, s));
    return MDHIP_OK;
}

int mdhip_draw_ops_from(mdhip_ctx* ctx, const uint8_t* const* src, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                        int n_src, uint8_t* const* dst, const int32_t* dst_src, const int64_t* dst_pitches, int n_dst, const int32_t* op_image,
                        const int32_t* ops, int n_ops, const uint8_t* patches, int64_t patch_bytes, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (n_dst == 0 && n_ops == 0) return MDHIP_OK;
    if (!src || !widths || !heights || !pitches || !dst || !dst_src || !dst_pitches || (n_ops && (!op_image || !ops)))
        return fail(ctx, MDHIP_EINVAL, "src/widths/heights/pitches/dst/dst_src/dst_pitches/op_image/ops is NULL");
    if (n_src < 1 || n_src > 65535 || n_dst < 1 || n_dst > 65535 || n_ops < 0 || patch_bytes < 0 || patch_bytes > 0x7fff0000LL)
        return fail(ctx, MDHIP_EINVAL, "n_src = %d, n_dst = %d, n_ops = %d, patch_bytes = %lld", n_src, n_dst, n_ops, (long long)patch_bytes);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // everything is checked before anything is launched: the operations as mdhip_draw_ops checks them, then the windows
    std::vector<int> count((size_t)n_dst, 0);
    bool any_patch = false;
    for (int i = 0; i < n_ops; ++i) {
        const int m = op_image[i];
        if (m < 0 || m >= n_dst) return fail(ctx, MDHIP_EINVAL, "operation %d: destination %d of %d", i, m, n_dst);
        const int32_t* op = ops + (size_t)i * MD_DRAW_OP_WORDS;
        if (md_draw_op_bad(op, patch_bytes))
            return fail(ctx, MDHIP_EINVAL, "operation %d: kind %d, or a patch of %dx%d pixels at byte %d of %lld", i, op[0], op[3], op[4], op[5],
                        (long long)patch_bytes);
        any_patch |= op[0] == MD_DRAW_PATCH && op[3] > 0 && op[4] > 0;
        ++count[m];
    }
    if (any_patch && (!patches || !is_device_ptr(patches))) return fail(ctx, MDHIP_EINVAL, "patches: NULL or a host pointer");
    const size_t n_win = (size_t)n_src + (size_t)n_dst;
    std::vector<uintptr_t> start(n_win), end(n_win);
    std::vector<uint8_t> is_dst(n_win);
    std::vector<int> order(n_win);
    for (int i = 0; i < n_src; ++i) {
        long long extent = 0;
        if (int rc = check_window(ctx, "source", i, widths[i], heights[i], pitches[i], 65535, &extent)) return rc;
        if (!src[i] || !is_device_ptr(src[i])) return fail(ctx, MDHIP_EINVAL, "source %d: NULL or a host pointer -- images must be device memory", i);
        start[(size_t)i] = (uintptr_t)src[i], end[(size_t)i] = (uintptr_t)src[i] + (uintptr_t)extent, is_dst[(size_t)i] = 0;
    }
    std::vector<DrawFrom> recs((size_t)n_dst);
    int first = 0, max_row_bytes = 0, max_h = 0;
    for (int m = 0; m < n_dst; ++m) {
        const int k = dst_src[m];
        if (k < 0 || k >= n_src) return fail(ctx, MDHIP_EINVAL, "destination %d: source %d of %d", m, k, n_src);
        long long extent = 0;
        if (int rc = check_window(ctx, "destination", m, widths[k], heights[k], dst_pitches[m], 65535, &extent)) return rc;
        if (!dst[m] || !is_device_ptr(dst[m]))
            return fail(ctx, MDHIP_EINVAL, "destination %d: NULL or a host pointer -- images must be device memory", m);
        const size_t j = (size_t)n_src + (size_t)m;
        start[j] = (uintptr_t)dst[m], end[j] = (uintptr_t)dst[m] + (uintptr_t)extent, is_dst[j] = 1;
        DrawFrom& d = recs[(size_t)m];
        memset(&d, 0, sizeof(d));
        d.src = src[k], d.dst = dst[m], d.src_pitch = pitches[k], d.dst_pitch = dst_pitches[m];
        d.row_bytes = widths[k] * 3, d.height = heights[k];
        d.x0 = widths[k], d.y0 = heights[k], d.x1 = -1, d.y1 = -1;
        d.op_first = first, d.op_count = count[m];
        first += count[m];
        max_row_bytes = std::max(max_row_bytes, d.row_bytes);
        max_h = std::max(max_h, d.height);
    }
    if (md_draw_from_overlap(start.data(), end.data(), is_dst.data(), (int)n_win, order.data()))
        return fail(ctx, MDHIP_EINVAL, "a destination overlaps a source or another destination");
    std::vector<int32_t> sorted((size_t)n_ops * MD_DRAW_OP_WORDS);
    std::vector<int> fill((size_t)n_dst, 0);
    for (int i = 0; i < n_ops; ++i) {
        const int m = op_image[i];
        DrawFrom& d = recs[(size_t)m];
        const int32_t* op = ops + (size_t)i * MD_DRAW_OP_WORDS;
        memcpy(sorted.data() + (size_t)(d.op_first + fill[m]++) * MD_DRAW_OP_WORDS, op, sizeof(int32_t) * MD_DRAW_OP_WORDS);
        // what the operation covers, clipped to the image (64-bit: a corner plus a size may pass 2^31)
        const long long w = d.row_bytes / 3, h = d.height;
        long long a = op[1], b = op[2], c = op[3], e = op[4];
        if (op[0] == MD_DRAW_PATCH) c = a + c - 1, e = b + e - 1;
        a = std::max(a, 0LL), b = std::max(b, 0LL);
        c = std::min(c, w - 1), e = std::min(e, h - 1);
        if (c < a || e < b) continue;
        d.x0 = std::min(d.x0, (int)a), d.y0 = std::min(d.y0, (int)b), d.x1 = std::max(d.x1, (int)c), d.y1 = std::max(d.y1, (int)e);
    }
    ScratchLayout lay;
    const size_t o_recs = lay.take(recs.size() * sizeof(DrawFrom));
    const size_t o_ops = lay.take(std::max(sorted.size(), (size_t)1) * sizeof(int32_t));
    if (int rc = ctx->draw.reserve(ctx, lay.size)) return rc;
    uint8_t* base = (uint8_t*)ctx->draw.p;
    HIP_TRY(ctx, hipMemcpyAsync(base + o_recs, recs.data(), recs.size() * sizeof(DrawFrom), hipMemcpyHostToDevice, s));
    if (!sorted.empty())
        HIP_TRY(ctx, hipMemcpyAsync(base + o_ops, sorted.data(), sorted.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_draw_ops_from((const DrawFrom*)(base + o_recs), n_dst, max_row_bytes, max_h, (const int32_t*)(base + o_ops), patches, s));
    return MDHIP_OK;
}

int mdhip_classifier_input(mdhip_ctx* ctx, const mdhip_classifier_crop* crops, int n, int size, int filter, const float mean[3],
                           const float std[3], float* out, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (n == 0) return MDHIP_OK;
    if (!crops || !mean || !std || !out) return fail(ctx, MDHIP_EINVAL, "crops/mean/std/out is NULL");
    if (n < 1 || n > 65535) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    if (size < 1 || size > MD_CLASSIFY_MAX_SIZE) return fail(ctx, MDHIP_EINVAL, "size = %d (1 .. %d)", size, MD_CLASSIFY_MAX_SIZE);
    if (filter != MD_FILTER_BICUBIC && filter != MD_FILTER_BILINEAR && filter != MD_FILTER_LANCZOS)
        return fail(ctx, MDHIP_EINVAL, "filter %d (0 = bicubic, 1 = bilinear, 2 = lanczos)", filter);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f)
            return fail(ctx, MDHIP_EINVAL, "channel %d: mean %g, std %g", c, (double)mean[c], (double)std[c]);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!is_device_ptr(out)) return fail(ctx, MDHIP_EINVAL, "host pointer -- out must be device memory");
    // every crop is checked and planned before anything is enqueued; crops of one canvas size share their tables
    std::map<std::pair<int, int>, MdClassifyCrop> planned;
    std::vector<MdClassifyCrop> recs((size_t)n);
    std::vector<int32_t> table;
    std::vector<double> work;
    int max_blocks = 1;
    for (int i = 0; i < n; ++i) {
        const mdhip_classifier_crop& q = crops[i];
        if (int rc = check_canvas(ctx, "crop", i, q.src, q.pitch, q.src_w, q.src_h, q.canvas_w, q.canvas_h, q.off_x, q.off_y)) return rc;
        auto it = planned.find({q.canvas_w, q.canvas_h});
        if (it == planned.end()) {
            MdClassifyCrop d;
            memset(&d, 0, sizeof(d));
            if (!md_classify_build(filter, q.canvas_w, q.canvas_h, size, MD_CLASSIFY_LDS_BYTES, table, work, &d))
                return fail(ctx, MDHIP_EUNSUPPORTED, "crop %d: the rows one output row of a %dx%d canvas at size %d needs do not fit on chip", i,
                            q.canvas_w, q.canvas_h, size);
            if (table.size() > 0x7fff0000u / sizeof(int32_t)) return fail(ctx, MDHIP_EUNSUPPORTED, "crop %d: the coefficient tables pass 2 GB", i);
            it = planned.emplace(std::make_pair(q.canvas_w, q.canvas_h), d).first;
        }
        MdClassifyCrop& d = recs[(size_t)i];
        d = it->second;
        d.src = q.src, d.pitch = q.pitch, d.src_w = q.src_w, d.src_h = q.src_h, d.off_x = q.off_x, d.off_y = q.off_y;
        if ((long long)d.strips * d.row_tiles > 0x7fffffffLL) return fail(ctx, MDHIP_EUNSUPPORTED, "crop %d: too many tiles", i);
        max_blocks = std::max(max_blocks, d.strips * d.row_tiles);
    }
    // the scratch: [float table][records][coefficient tables]
    ScratchLayout lay;
    const size_t o_lut = lay.take(3 * 256 * sizeof(float));
    const size_t o_recs = lay.take(recs.size() * sizeof(MdClassifyCrop));
    const size_t o_table = lay.take(std::max<size_t>(table.size(), 1) * sizeof(int32_t));
    if (int rc = ctx->classify.reserve(ctx, lay.size)) return rc;
    uint8_t* base = (uint8_t*)ctx->classify.p;
    float lut[3 * 256];
    md_classify_lut(mean, std, lut);
    // (the uploads are from pageable memory: the copies have left the buffers when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(base + o_lut, lut, sizeof(lut), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(base + o_recs, recs.data(), recs.size() * sizeof(MdClassifyCrop), hipMemcpyHostToDevice, s));
    if (!table.empty()) HIP_TRY(ctx, hipMemcpyAsync(base + o_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_classifier_input((const MdClassifyCrop*)(base + o_recs), n, max_blocks, (const int32_t*)(base + o_table),
                                         (const float*)(base + o_lut), out, s));
    return MDHIP_OK;
}

int mdhip_thumbnails(mdhip_ctx* ctx, const mdhip_thumbnail* tiles, int n, int filter, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (n == 0) return MDHIP_OK;
    if (!tiles) return fail(ctx, MDHIP_EINVAL, "tiles is NULL");
    if (n < 1 || n > 65535) return fail(ctx, MDHIP_EINVAL, "n = %d", n);
    if (filter != MD_FILTER_BICUBIC && filter != MD_FILTER_BILINEAR && filter != MD_FILTER_LANCZOS)
        return fail(ctx, MDHIP_EINVAL, "filter %d (0 = bicubic, 1 = bilinear, 2 = lanczos)", filter);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // every tile is checked and planned before anything is enqueued; tiles of one canvas and output size share their tables
    std::map<std::tuple<int, int, int, int>, MdClassifyCrop> planned;
    std::vector<MdClassifyCrop> recs((size_t)n);
    std::vector<int32_t> table;
    std::vector<double> work;
    int max_blocks = 1;
    for (int i = 0; i < n; ++i) {
        const mdhip_thumbnail& q = tiles[i];
        // (a canvas without image pixels -- a box wholly outside its image -- has a rectangle of no width or height: src is not read)
        const bool empty = (q.src_w == 0 && q.src_h >= 0) || (q.src_h == 0 && q.src_w >= 0);
        if (empty) {
            if (q.canvas_w < 1 || q.canvas_h < 1 || q.canvas_w > 65535 || q.canvas_h > 65535)
                return fail(ctx, MDHIP_EINVAL, "tile %d: a canvas of %dx%d", i, q.canvas_w, q.canvas_h);
        } else if (int rc = check_canvas(ctx, "tile", i, q.src, q.pitch, q.src_w, q.src_h, q.canvas_w, q.canvas_h, q.off_x, q.off_y)) {
            return rc;
        }
        if (int rc = check_window(ctx, "tile (output)", i, q.out_w, q.out_h, q.dst_pitch)) return rc;
        if (!q.dst || !is_device_ptr(q.dst)) return fail(ctx, MDHIP_EINVAL, "tile %d: NULL or a host pointer -- dst must be device memory", i);
        auto it = planned.find(std::make_tuple(q.canvas_w, q.canvas_h, q.out_w, q.out_h));
        if (it == planned.end()) {
            MdClassifyCrop d;
            memset(&d, 0, sizeof(d));
            if (!md_thumbnail_build(filter, q.canvas_w, q.canvas_h, q.out_w, q.out_h, MD_CLASSIFY_LDS_BYTES, table, work, &d))
                return fail(ctx, MDHIP_EUNSUPPORTED, "tile %d: the rows one output row of a %dx%d canvas reduced to %dx%d needs do not fit on chip",
                            i, q.canvas_w, q.canvas_h, q.out_w, q.out_h);
            if (table.size() > 0x7fff0000u / sizeof(int32_t)) return fail(ctx, MDHIP_EUNSUPPORTED, "tile %d: the coefficient tables pass 2 GB", i);
            it = planned.emplace(std::make_tuple(q.canvas_w, q.canvas_h, q.out_w, q.out_h), d).first;
        }
        MdClassifyCrop& d = recs[(size_t)i];
        d = it->second;
        if (!empty) d.src = q.src, d.pitch = q.pitch, d.src_w = q.src_w, d.src_h = q.src_h, d.off_x = q.off_x, d.off_y = q.off_y;
        d.dst = q.dst, d.dst_pitch = q.dst_pitch;
        if ((long long)d.strips * d.row_tiles > 0x7fffffffLL) return fail(ctx, MDHIP_EUNSUPPORTED, "tile %d: too many workgroups", i);
        max_blocks = std::max(max_blocks, d.strips * d.row_tiles);
    }
    // the scratch: [records][coefficient tables]
    ScratchLayout lay;
    const size_t o_recs = lay.take(recs.size() * sizeof(MdClassifyCrop));
    const size_t o_table = lay.take(std::max<size_t>(table.size(), 1) * sizeof(int32_t));
    if (int rc = ctx->classify.reserve(ctx, lay.size)) return rc;
    uint8_t* base = (uint8_t*)ctx->classify.p;
    // (the uploads are from pageable memory: the copies have left the buffers when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(base + o_recs, recs.data(), recs.size() * sizeof(MdClassifyCrop), hipMemcpyHostToDevice, s));
    if (!table.empty()) HIP_TRY(ctx, hipMemcpyAsync(base + o_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_thumbnails((const MdClassifyCrop*)(base + o_recs), n, max_blocks, (const int32_t*)(base + o_table), s));
    return MDHIP_OK;
}

int mdhip_change_detect(mdhip_ctx* ctx, const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                        int n_images, uint8_t* const* blurred, const uint8_t* blurred_ready, const int32_t* pairs, int n_pairs,
                        const mdhip_change_options* opt, int64_t* counts, uint32_t* hist, int32_t* thresholds, int32_t* n_regions,
                        int32_t* regions, uint8_t* overflow, uint8_t* const* masks, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    if (!opt || !chg_options_ok(opt->blur_kernel_size, opt->threshold_type, opt->threshold, opt->dilate_kernel_size, opt->dilate_iterations,
                                opt->min_area, opt->has_ignore, opt->ignore_fraction, opt->region_cap))
        return fail(ctx, MDHIP_EINVAL, "options: NULL, or a value outside its range (csrc/change_detect.h)");
    if (n_images > 65535 || n_pairs > 65535 ||
        !chg_args_ok(images, widths, heights, pitches, n_images, blurred, blurred_ready, pairs, n_pairs, counts, hist, thresholds, n_regions,
                     regions, overflow, opt->region_cap))
        return fail(ctx, MDHIP_EINVAL, "a NULL pointer, a size or pitch outside its range, an image neither given nor ready, or a pair that "
                    "names no image or two images of different sizes (%d images, %d pairs)", n_images, n_pairs);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n_images; ++i)
        if (!is_device_ptr(blurred[i]) || (!blurred_ready[i] && !is_device_ptr(images[i])))
            return fail(ctx, MDHIP_EINVAL, "image %d: the pixels and the blurred plane must be device memory", i);
    for (int p = 0; masks && p < n_pairs; ++p)
        if (masks[p] && !is_device_ptr(masks[p])) return fail(ctx, MDHIP_EINVAL, "pair %d: the mask must be device memory", p);
    const size_t budget = (size_t)1 << 30;              // scratch planes of one group of images or pairs (one that needs more is a group)
    ChgWeights wt;
    chg_blur_weights(opt->blur_kernel_size, &wt);

    // ---- gray and blur, once per image that does not come with its plane
    for (int first = 0; first < n_images;) {
        ScratchLayout lay;
        std::vector<ChgImage> recs;
        std::vector<size_t> o_first;
        int max_w = 1, max_h = 1, last = first;
        lay.take(sizeof(ChgImage) * (size_t)(n_images - first));        // (at offset 0; room for every image that is left)
        for (; last < n_images && (recs.empty() || lay.size < budget); ++last) {
            if (blurred_ready[last]) continue;
            ChgImage d{};
            d.rgb = images[last], d.pitch = pitches[last], d.out = blurred[last], d.w = widths[last], d.h = heights[last];
            chg_roi_rows(opt->has_ignore, opt->ignore_fraction, d.h, &d.y0, &d.y1);
            o_first.push_back(lay.take(2 * (size_t)d.w * d.h));
            max_w = std::max(max_w, d.w), max_h = std::max(max_h, d.h);
            recs.push_back(d);
        }
        first = last;
        if (recs.empty()) continue;
        if (int rc = ctx->change.reserve(ctx, lay.size, &s)) return rc;
        for (size_t k = 0; k < recs.size(); ++k) recs[k].first = (uint16_t*)(ctx->change.p + o_first[k]);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->change.p, recs.data(), sizeof(ChgImage) * recs.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, launch_chg_blur((const ChgImage*)ctx->change.p, (int)recs.size(), max_w, max_h, wt, s));
    }

    // ---- the pairs, in groups
    const int cap = opt->region_cap;
    for (int first = 0; first < n_pairs;) {
        struct Off { size_t m0, m1, label, stat, blocks; };
        ScratchLayout lay;
        std::vector<Off> offs;
        int last = first, max_w = 1, max_h = 1;
        long long max_px = 1;
        const size_t room = (size_t)(n_pairs - first);
        lay.take(sizeof(ChgPair) * room);                               // (at offset 0)
        const size_t o_thr = lay.take(4 * room), o_count = lay.take(8 * room), o_nreg = lay.take(4 * room);
        const size_t o_hist = lay.take(1024 * room), o_regions = lay.take(20 * (size_t)cap * room);
        const size_t o_planes = lay.size;
        for (; last < n_pairs && (offs.empty() || lay.size - o_planes < budget); ++last) {
            const size_t px = (size_t)widths[pairs[2 * last]] * heights[pairs[2 * last]], nb = (px + 255) / 256;
            Off o;
            o.m0 = lay.take(px), o.m1 = lay.take(px), o.label = lay.take(4 * px), o.stat = lay.take(20 * px), o.blocks = lay.take(8 * nb);
            offs.push_back(o);
        }
        const int n = last - first;
        if (int rc = ctx->change.reserve(ctx, lay.size, &s)) return rc;
        char* base = ctx->change.p;
        std::vector<ChgPair> recs((size_t)n);
        for (int k = 0; k < n; ++k) {
            const int p = first + k, a = pairs[2 * p], b = pairs[2 * p + 1];
            ChgPair& d = recs[(size_t)k];
            d.a = blurred[a], d.b = blurred[b];
            d.m[0] = (uint8_t*)(base + offs[k].m0), d.m[1] = (uint8_t*)(base + offs[k].m1);
            d.label = (uint32_t*)(base + offs[k].label), d.stat = (uint32_t*)(base + offs[k].stat);
            d.block_count = (uint32_t*)(base + offs[k].blocks);
            d.hist = (uint32_t*)(base + o_hist) + 256 * (size_t)k;
            d.count = (unsigned long long*)(base + o_count) + k;
            d.n_regions = (int32_t*)(base + o_nreg) + k;
            d.regions = (int32_t*)(base + o_regions) + 5 * (size_t)cap * k;
            d.label_out = nullptr;
            d.w = widths[a], d.h = heights[a];
            chg_roi_rows(opt->has_ignore, opt->ignore_fraction, d.h, &d.y0, &d.y1);
            max_w = std::max(max_w, d.w), max_h = std::max(max_h, d.h);
            max_px = std::max(max_px, (long long)d.w * d.h);
        }
        const ChgPair* dev = (const ChgPair*)base;
        HIP_TRY(ctx, hipMemcpyAsync(base, recs.data(), sizeof(ChgPair) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemsetAsync(base + o_thr, 0, o_planes - o_thr, s));            // thresholds, counts, histograms, regions
        std::vector<int32_t> thr((size_t)n, opt->threshold);
        if (opt->threshold_type == 1) {
            // the histogram comes to the host, where chg_otsu chooses the threshold for both legs
            HIP_TRY(ctx, launch_chg_diff(dev, n, max_px, 0, nullptr, s));
            HIP_TRY(ctx, hipMemcpyAsync(hist + 256 * (size_t)first, base + o_hist, 1024 * (size_t)n, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            for (int k = 0; k < n; ++k) thr[(size_t)k] = chg_otsu(hist + 256 * (size_t)(first + k));
        } else {
            memset(hist + 256 * (size_t)first, 0, 1024 * (size_t)n);
        }
        HIP_TRY(ctx, hipMemcpyAsync(base + o_thr, thr.data(), 4 * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, launch_chg_diff(dev, n, max_px, 1, (const int32_t*)(base + o_thr), s));
        int sel = 0;
        HIP_TRY(ctx, launch_chg_dilate(dev, n, max_w, max_h, opt->dilate_kernel_size, opt->dilate_iterations, &sel, s));
        HIP_TRY(ctx, launch_chg_regions(dev, n, max_w, max_h, sel, opt->min_area, cap, s));
        for (int k = 0; masks && k < n; ++k)
            if (masks[first + k])
                HIP_TRY(ctx, hipMemcpyAsync(masks[first + k], recs[(size_t)k].m[sel], (size_t)recs[(size_t)k].w * recs[(size_t)k].h,
                                            hipMemcpyDeviceToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(counts + first, base + o_count, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(n_regions + first, base + o_nreg, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
        if (cap)
            HIP_TRY(ctx, hipMemcpyAsync(regions + 5 * (size_t)cap * first, base + o_regions, 20 * (size_t)cap * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        for (int k = 0; k < n; ++k) {
            thresholds[first + k] = thr[(size_t)k];
            overflow[first + k] = n_regions[first + k] > cap ? 1 : 0;
        }
        first = last;
    }
    return MDHIP_OK;
}

int mdhip_gray_count(mdhip_ctx* ctx, const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                     const int32_t* windows, int n, uint64_t* counts, void* hip_stream) {
    if (!ctx) return MDHIP_EINVAL;
    int bad;
    if (!gc_args_ok(images, widths, heights, pitches, windows, n, counts, &bad)) {
        if (bad < 0) return fail(ctx, MDHIP_EINVAL, "images/widths/heights/pitches/windows/counts is NULL, or n = %d outside 1 .. %d", n, GC_MAX_IMAGES);
        return fail(ctx, MDHIP_EINVAL, "image %d: NULL, %dx%d at pitch %lld (sides 1 .. 65535, pitch >= 3 * width, under 0x7fff0000 bytes in all), or its window (%d, %d, %d, %d) is empty or leaves it", bad, widths[bad],
                    heights[bad], (long long)pitches[bad], windows[4 * bad], windows[4 * bad + 1], windows[4 * bad + 2], windows[4 * bad + 3]);
    }
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n; ++i)
        if (!is_device_ptr(images[i])) return fail(ctx, MDHIP_EINVAL, "image %d: a host pointer -- images must be device memory", i);
    // the scratch: [records][counters]
    ScratchLayout lay;
    lay.take(sizeof(GrayWindow) * (size_t)n);                           // (at offset 0)
    const size_t o_counts = lay.take(8 * (size_t)n);
    if (int rc = ctx->gray.reserve(ctx, lay.size, &s)) return rc;
    std::vector<GrayWindow> recs((size_t)n);
    long long max_groups = 1;
    for (int i = 0; i < n; ++i) {
        const int32_t* q = windows + 4 * (size_t)i;
        GrayWindow& d = recs[(size_t)i];
        d.origin = images[i] + (long long)q[1] * pitches[i] + 3LL * q[0];
        d.pitch = pitches[i];
        d.count = (unsigned long long*)(ctx->gray.p + o_counts) + i;
        d.w = q[2], d.h = q[3];
        max_groups = std::max(max_groups, (long long)gc_groups(d.w) * d.h);
    }
    // (the upload is from pageable memory: the copy has left `recs` when the call returns)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->gray.p, recs.data(), sizeof(GrayWindow) * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(ctx->gray.p + o_counts, 0, 8 * (size_t)n, s));
    HIP_TRY(ctx, launch_gray_count((const GrayWindow*)ctx->gray.p, n, max_groups, s));
    std::vector<uint64_t> got((size_t)n);                               // the caller's array stays as it is unless all of it arrives
    HIP_TRY(ctx, hipMemcpyAsync(got.data(), ctx->gray.p + o_counts, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    memcpy(counts, got.data(), 8 * (size_t)n);
    return MDHIP_OK;
}

}  // extern "C"
