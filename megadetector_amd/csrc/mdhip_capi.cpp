// C-ABI layer (include/mdhip.h): context creation and upload, the forwards, NMS, fp8 calibration, introspection and the setters.
//
// This is the native runtime under the Python detector seam
// (reference megadetector/detection/pytorch_detector.py:739 PTDetector):
//   mdhip_create      <- PTDetector.__init__/_load_model            (:745-959)
//   mdhip_forward     <- self.model(batch)[0]                       (:1313)
//   mdhip_nms         <- nms()                                      (:502-610, :1342)
// The context and what the host files share are in mdhip_ctx.h.  The image entry points (mdhip_preprocess <- letterbox +
// tensor prep :1104-1109, :1283-1310; the windows, JPEG and blur calls) are in mdhip_image_api.cpp, the single-kernel test
// hooks (mdhip_*_on) in mdhip_kernel_hooks.cpp.  The planner (model -> ops, arena, packed weights: all that mdhip_create does on
// the host) is mdhip_plan.cpp, the executor (what a pass launches: resolved once, then launched) mdhip_exec.cpp.

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mdhip_ctx.h"

static thread_local std::string g_create_error;   // of the last failed mdhip_create of this thread (there is no context yet)

int mdhip::fail(mdhip_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

int mdhip::check_shape(mdhip_ctx* ctx, int n, int h, int w) {
    if (n < 1 || n > ctx->max_batch) return fail(ctx, MDHIP_EINVAL, "batch %d outside [1,%d]", n, ctx->max_batch);
    if (h < ctx->max_stride || w < ctx->max_stride || h % ctx->max_stride || w % ctx->max_stride)
        return fail(ctx, MDHIP_EINVAL, "input %dx%d must be a positive multiple of the model stride %d", h, w, ctx->max_stride);
    if ((size_t)h * w > (size_t)ctx->max_h * ctx->max_w)
        return fail(ctx, MDHIP_ENOMEM, "input %dx%d exceeds the planned %dx%d", h, w, ctx->max_h, ctx->max_w);
    return MDHIP_OK;
}

int mdhip::need_model(mdhip_ctx* ctx, const char* call) {
    if (!ctx->images_only) return MDHIP_OK;
    return fail(ctx, MDHIP_EINVAL, "%s: this context has no model (mdhip_create_images): only the image entry points work on it", call);
}

TtaPass mdhip::tta_pass(const mdhip_ctx* ctx, int h, int w, int k) {
    static const float scales[3] = {1.0f, 0.83f, 0.67f};
    static const double scales_d[3] = {1.0, 0.83, 0.67};
    static const int flips[3] = {0, 1, 0};
    const int gs = ctx->max_stride;
    TtaPass p;
    p.sh = k ? (int)(h * scales_d[k]) : h;
    p.sw = k ? (int)(w * scales_d[k]) : w;
    p.oh = k ? (int)std::ceil(h * scales_d[k] / gs) * gs : h;
    p.ow = k ? (int)std::ceil(w * scales_d[k] / gs) * gs : w;
    p.flip = flips[k];
    p.scale = scales[k];
    return p;
}

namespace {

// the captured graphs go (after the device has finished with them: an executable may still be in flight on the caller's stream)
void drop_graphs(mdhip_ctx* ctx) {
    bool any = false;
    for (auto& kv : ctx->graphs) any |= kv.second.exec != nullptr;
    if (any) {
        (void)hipSetDevice(ctx->device);            // (the setters reach here without it: synchronise OUR device)
        (void)hipDeviceSynchronize();
    }
    for (auto& kv : ctx->graphs)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    ctx->graphs.clear();
}

// room for one more cached graph: the least recently used executable goes (its stream work is waited for first)
void evict_graph_if_full(mdhip_ctx* ctx) {
    int live = 0;
    for (auto& kv : ctx->graphs) live += kv.second.exec != nullptr;
    if (live < mdhip_ctx::kMaxGraphs) return;
    auto victim = ctx->graphs.end();
    for (auto it = ctx->graphs.begin(); it != ctx->graphs.end(); ++it)
        if (it->second.exec && (victim == ctx->graphs.end() || it->second.last_use < victim->second.last_use)) victim = it;
    if (victim == ctx->graphs.end()) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    (void)hipGraphExecDestroy(victim->second.exec);
    ctx->graphs.erase(victim);
}

// every call that changes what a forward launches: the resolved passes are void (mdhip_ctx::generation), the graphs dropped
void launches_changed(mdhip_ctx* ctx) {
    ++ctx->generation;
    drop_graphs(ctx);
}

// One pass over the ops, as mdhip_forward and its kin make it: the state the ops read while it lasts (the kind of pass, the
// anchor pitch of the prediction it writes; an augmented pass sets mdhip_ctx::cur_tta itself), and what it leaves to later calls.
struct Pass {
    mdhip_ctx* ctx;
    hipStream_t s;
    std::shared_ptr<Resolved> ran;
    Pass(mdhip_ctx* c, hipStream_t stream, int n_anchors, bool isolated = false, bool calibrating = false) : ctx(c), s(stream) {
        ctx->cur_tta = DecodeTta();
        ctx->cur_A = n_anchors;
        ctx->fuse_suspended = isolated;
        ctx->calibrating = calibrating;
    }
    ~Pass() { ctx->cur_tta = DecodeTta(); ctx->fuse_suspended = ctx->calibrating = false; }
    // the pass writes the other prediction buffer, once an NMS that may still read it on another stream is done
    int flip_prediction() {
        ctx->pred_cur ^= 1;
        ctx->pred_off = ctx->pred_offs[ctx->pred_cur];
        if (ctx->pred_read_valid[ctx->pred_cur]) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->pred_read[ctx->pred_cur], 0));
        return MDHIP_OK;
    }
    // launches ops [first, first + count) for n images of h x w on stream `on`
    int run(int n, int h, int w, hipStream_t on, size_t first = 0, size_t count = INT_MAX) {
        ran = resolved_for(ctx, n, h, w);
        return launch_ops(ctx, *ran, first, count, on);
    }
    // nothing behind this point reads the network input (mdhip_ctx::input_free); idle: the stream has been waited for
    int input_done(bool idle) {
        if (!idle) HIP_TRY(ctx, hipEventRecord(ctx->input_free, s));
        ctx->input_free_valid = !idle;
        return MDHIP_OK;
    }
    // the context's last forward is this pass of n images, h x w being the input's size
    void finish(int n, int h, int w) {
        ctx->last_n = n; ctx->last_h = h; ctx->last_w = w;
        ctx->last_A = ctx->cur_A;
        ctx->last_ran = ran;
        ctx->step_n = ctx->step_h = ctx->step_w = 0;
    }
};

int check_calibrated(mdhip_ctx* ctx) {
    if (ctx->dtype == MDHIP_DTYPE_FP8 && ctx->n_f8 > 0 && !ctx->calibrated)
        return fail(ctx, MDHIP_EINVAL, "fp8 context without activation scales: call mdhip_calibrate (or mdhip_fp8_set_scales) first");
    return MDHIP_OK;
}

// new range -> scale of an e4m3 tensor and the combined per-channel factors of the conv that reads it
int apply_fp8_scale(mdhip_ctx* ctx, Op& producer, float act_scale) {
    launches_changed(ctx);                          // (the quantisation scale is a launch argument)
    producer.act_scale = act_scale;
    Op& consumer = ctx->ops[producer.f8_peer];
    consumer.act_scale = act_scale;
    const PackedConv& pc = ctx->packed[consumer.pc];
    std::vector<float> sc(pc.n_rows, 0.f);
    for (int n = 0; n < pc.n_rows; ++n) sc[n] = act_scale * pc.wscale[n];
    HIP_TRY(ctx, hipMemcpy(ctx->warena + pc.scale_off, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
    return MDHIP_OK;
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char* mdhip_version(void) { return "mdhip 0.2 (gfx950: bf16 / fp16 storage, fp8 bottlenecks)"; }

const char* mdhip_last_error(mdhip_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// what mdhip_create and mdhip_plan_describe check before anything is planned
static int check_create_args(const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w) {
    if (!model || !model->layers || !model->convs || model->n_layers < 1)
        return fail(nullptr, MDHIP_EINVAL, "empty model description");
    if (dtype != MDHIP_DTYPE_BF16 && dtype != MDHIP_DTYPE_FP16 && dtype != MDHIP_DTYPE_FP8)
        return fail(nullptr, MDHIP_EUNSUPPORTED, "dtype %d not implemented (bf16, fp16, fp8)", dtype);
    if (max_batch < 1 || max_h < 64 || max_w < 64) return fail(nullptr, MDHIP_EINVAL, "bad capacity %d x %dx%d", max_batch, max_h, max_w);
    return MDHIP_OK;
}

int mdhip_create(const mdhip_model* model, int device, int dtype, int max_batch, int max_h,
                 int max_w, mdhip_ctx** out) {
    if (!out) return fail(nullptr, MDHIP_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = check_create_args(model, dtype, max_batch, max_h, max_w)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, MDHIP_EHIP, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, MDHIP_EINVAL, "device %d outside [0,%d)", device, ndev);

    mdhip_ctx* ctx = new mdhip_ctx();
    if (const char* ef = getenv("MDHIP_FUSE")) ctx->fuse_enabled = atoi(ef) != 0;      // A/B measurements
    if (const char* ep = getenv("MDHIP_PAIR")) ctx->pair_enabled = atoi(ep) != 0;      // A/B measurements, bit-identity test
    ctx->letterbox_general = getenv("MDHIP_LETTERBOX_GENERAL") != nullptr;             // (read once, not per mdhip_preprocess)
    ctx->device = device;
    PlannedWeights pw;
    std::string err;
    if (int rc = plan_context(ctx, model, dtype, max_batch, max_h, max_w, &pw, &err)) {
        delete ctx;
        return fail(nullptr, rc, "%s", err.c_str());
    }

    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = conv_api(ctx).init();
    if (e != hipSuccess) {
        delete ctx;
        return fail(nullptr, MDHIP_EHIP, "device init failed: %s", hipGetErrorString(e));
    }

#define CREATE_TRY(expr)                                                                        \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            std::string m = std::string(#expr) + " failed: " + hipGetErrorString(e__);          \
            mdhip_destroy(ctx);                                                                 \
            return fail(nullptr, e__ == hipErrorOutOfMemory ? MDHIP_ENOMEM : MDHIP_EHIP, "%s", m.c_str()); \
        }                                                                                       \
    } while (0)

    CREATE_TRY(hipMalloc((void**)&ctx->arena, ctx->arena_bytes));
    CREATE_TRY(hipMalloc((void**)&ctx->warena, ctx->warena_bytes));
    CREATE_TRY(hipMemset(ctx->warena, 0, 256));
    CREATE_TRY(hipHostMalloc((void**)&ctx->geom_host, (size_t)4 * max_batch * sizeof(LetterboxWin), hipHostMallocDefault));
    for (int i = 0; i < 4; ++i) CREATE_TRY(hipEventCreateWithFlags(&ctx->geom_ev[i], hipEventDisableTiming));
    CREATE_TRY(hipEventCreateWithFlags(&ctx->input_free, hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) CREATE_TRY(hipEventCreateWithFlags(&ctx->pred_read[i], hipEventDisableTiming));
    for (int i = 0; i < MDHIP_NMS_SLOTS; ++i) {
        CREATE_TRY(hipHostMalloc((void**)&ctx->nms_host_out[i], (size_t)max_batch * kNmsMaxDet * 6 * 4, hipHostMallocDefault));
        CREATE_TRY(hipHostMalloc((void**)&ctx->nms_host_cnt[i], (size_t)max_batch * 4, hipHostMallocDefault));
        CREATE_TRY(hipEventCreateWithFlags(&ctx->nms_ev[i], hipEventDisableTiming));
    }
    // The whole arena starts as zeros: no kernel's result may depend on memory nobody wrote (K-slab tails against zero
    // weights, pad channels, halo rows of a neighbouring tensor).  MDHIP_ARENA_POISON=1 (tests) fills it with 0xFF bytes
    // instead -- NaN in bf16, fp16 and fp32 -- so that any such read shows up as NaN in the output.
    {
        const char* pz = getenv("MDHIP_ARENA_POISON");
        CREATE_TRY(hipMemset(ctx->arena, (pz && atoi(pz) != 0) ? 0xff : 0, ctx->arena_bytes));
    }
    if (!ctx->strides.empty() && !ctx->anchor_free)      // (a model with an anchor-based Detect layer)
        CREATE_TRY(hipMemcpy(ctx->warena + ctx->anchors_off, model->anchors_px, (size_t)ctx->nl * ctx->na * 2 * 4, hipMemcpyHostToDevice));
    for (size_t i = 0; i < ctx->packed.size(); ++i) {
        const PackedConv& pc = ctx->packed[i];
        for (const PackedBlobs::Ref& b : pw.convs[i].refs())
            if (b.bytes) CREATE_TRY(hipMemcpy(ctx->warena + pc.*b.off, b.data, b.bytes, hipMemcpyHostToDevice));
        if (pc.scale_off) CREATE_TRY(hipMemset(ctx->warena + pc.scale_off, 0, (size_t)pc.n_rows * 4));
    }
    for (int i = 0; i < 3; ++i) {
        ctx->nms_scr.keys[i] = (uint32_t*)(ctx->arena + ctx->nms_kv_off[i]);
        ctx->nms_scr.vals[i] = (uint32_t*)(ctx->arena + ctx->nms_kv_off[3 + i]);
    }
    ctx->nms_scr.cap = ctx->a_cap;
    ctx->nms_scr.seg_cnt = (uint32_t*)(ctx->arena + ctx->nms_seg_off);
    CREATE_TRY(hipDeviceSynchronize());
#undef CREATE_TRY
    *out = ctx;
    return MDHIP_OK;
}

int mdhip_create_images(int device, mdhip_ctx** out) {
    if (!out) return fail(nullptr, MDHIP_EINVAL, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, MDHIP_EHIP, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, MDHIP_EINVAL, "device %d outside [0,%d)", device, ndev);
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, MDHIP_EHIP, "device init failed: %s", hipGetErrorString(e));
    mdhip_ctx* ctx = new mdhip_ctx();
    ctx->device = device;
    ctx->images_only = true;
    *out = ctx;
    return MDHIP_OK;
}

long long mdhip_plan_describe(const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w, char* buf, size_t cap) {
    if (int rc = check_create_args(model, dtype, max_batch, max_h, max_w)) return rc;
    mdhip_ctx ctx;                                      // thrown away: no device is touched, nothing to destroy
    PlannedWeights pw;
    std::string err;
    if (int rc = plan_context(&ctx, model, dtype, max_batch, max_h, max_w, &pw, &err)) return fail(nullptr, rc, "%s", err.c_str());
    const std::string text = describe_plan(&ctx, pw);
    if (buf && cap) snprintf(buf, cap, "%s", text.c_str());
    return (long long)text.size();
}

long long mdhip_launches_describe(const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w, const mdhip_tuned* tuned,
                                  int n_tuned, int n, int h, int w, unsigned flags, const int32_t* forced, int n_forced, char* buf,
                                  size_t cap) {
    if (int rc = check_create_args(model, dtype, max_batch, max_h, max_w)) return rc;
    if (n_tuned < 0 || (n_tuned > 0 && !tuned) || n_forced < 0 || (n_forced > 0 && !forced))
        return fail(nullptr, MDHIP_EINVAL, "mdhip_launches_describe: bad table or forced list");
    mdhip_ctx ctx;                                      // thrown away: no device is touched, nothing to destroy
    ctx.pair_enabled = !(flags & MDHIP_LAUNCHES_NO_PAIR);
    PlannedWeights pw;
    std::string err;
    if (int rc = plan_context(&ctx, model, dtype, max_batch, max_h, max_w, &pw, &err)) return fail(nullptr, rc, "%s", err.c_str());
    // the decisions read which pointers are null and which are equal and follow none of them: any two bases do
    ctx.arena = (char*)(uintptr_t)(1ull << 40);
    ctx.warena = (char*)(uintptr_t)(2ull << 40);
    int rc = check_shape(&ctx, n, h, w);
    if (!rc) rc = mdhip_set_tuned(&ctx, tuned, n_tuned);
    for (int i = 0; i < n_forced && !rc; ++i) rc = mdhip_set_op_cfg(&ctx, forced[2 * i], forced[2 * i + 1]);
    if (rc) return fail(nullptr, rc, "%s", ctx.err.empty() ? "mdhip_launches_describe: bad forced list" : ctx.err.c_str());
    const bool fuse = !(flags & MDHIP_LAUNCHES_NO_FUSE), fuse_decode = !(flags & MDHIP_LAUNCHES_NO_FUSE_DECODE);
    (void)mdhip_set_fuse(&ctx, fuse);
    (void)mdhip_set_option(&ctx, "fuse_decode", fuse_decode);
    (void)mdhip_set_option(&ctx, "pw_stream", !(flags & MDHIP_LAUNCHES_NO_PW_STREAM));
    // the pass as one of the forward-like calls would set it up (an augmented pass: any placement but the plain one)
    auto resolve_as = [&](unsigned kind, int rn, int rh, int rw) {
        Pass pass(&ctx, nullptr, num_anchors_for(&ctx, rh, rw), (kind & MDHIP_LAUNCHES_ISOLATED) != 0, (kind & MDHIP_LAUNCHES_CALIBRATING) != 0);
        if (kind & MDHIP_LAUNCHES_AUGMENTED) ctx.cur_tta.scale = 0.83f;
        return resolved_for(&ctx, rn, rh, rw);
    };
    if (flags & MDHIP_LAUNCHES_AFTER_OTHERS)
        for (int round = 0; round < 4; ++round) {       // as set, fuse flipped, fuse_decode flipped, back as set
            (void)mdhip_set_fuse(&ctx, round == 1 ? !fuse : fuse);
            (void)mdhip_set_option(&ctx, "fuse_decode", round == 2 ? !fuse_decode : fuse_decode);
            for (unsigned kind : {0u, (unsigned)MDHIP_LAUNCHES_ISOLATED, (unsigned)MDHIP_LAUNCHES_CALIBRATING, (unsigned)MDHIP_LAUNCHES_AUGMENTED}) {
                (void)resolve_as(kind, n, h, w);
                (void)resolve_as(kind, 1, ctx.max_stride * 2, ctx.max_stride * 3);
            }
        }
    const std::string text = describe_launches(&ctx, *resolve_as(flags, n, h, w));
    if (buf && cap) snprintf(buf, cap, "%s", text.c_str());
    return (long long)text.size();
}

void mdhip_destroy(mdhip_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    drop_graphs(ctx);
    if (ctx->capture_stream) (void)hipStreamDestroy(ctx->capture_stream);
    for (hipEvent_t ev : ctx->events) (void)hipEventDestroy(ev);
    for (int i = 0; i < mdhip_ctx::kFwdRing; ++i)
        for (int k = 0; k < 2; ++k)
            if (ctx->fwd_ev[i][k]) (void)hipEventDestroy(ctx->fwd_ev[i][k]);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->warena) (void)hipFree(ctx->warena);
    for (DevBuffer* b : {&ctx->stage, &ctx->jpeg_planes, &ctx->jpeg_entropy, &ctx->jpeg_encode, &ctx->blur, &ctx->resample, &ctx->draw, &ctx->classify, &ctx->change, &ctx->gray}) b->release();
    if (ctx->geom_host) (void)hipHostFree(ctx->geom_host);
    for (int i = 0; i < 4; ++i) if (ctx->geom_ev[i]) (void)hipEventDestroy(ctx->geom_ev[i]);
    if (ctx->input_free) (void)hipEventDestroy(ctx->input_free);
    for (int i = 0; i < 2; ++i)
        if (ctx->pred_read[i]) (void)hipEventDestroy(ctx->pred_read[i]);
    for (int i = 0; i < MDHIP_NMS_SLOTS; ++i) {
        if (ctx->nms_host_out[i]) (void)hipHostFree(ctx->nms_host_out[i]);
        if (ctx->nms_host_cnt[i]) (void)hipHostFree(ctx->nms_host_cnt[i]);
        if (ctx->nms_ev[i]) (void)hipEventDestroy(ctx->nms_ev[i]);
    }
    delete ctx;
}

int mdhip_max_stride(mdhip_ctx* ctx) { return ctx ? ctx->max_stride : MDHIP_EINVAL; }

int mdhip_num_anchors(mdhip_ctx* ctx, int h, int w) {
    NEED_MODEL(ctx);
    return num_anchors_for(ctx, h, w);
}

int mdhip_forward(mdhip_ctx* ctx, int n, int h, int w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (int rc = check_calibrated(ctx)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slot = (int)(ctx->fwd_count % mdhip_ctx::kFwdRing);
    if (ctx->time_forward) HIP_TRY(ctx, hipEventRecord(ctx->fwd_ev[slot][0], s));
    Pass pass(ctx, s, num_anchors_for(ctx, h, w));
    if (int rc = pass.flip_prediction()) return rc;
    const bool use_graph = (ctx->graph_mode == 1 || (ctx->graph_mode == 2 && n <= ctx->graph_max_n)) && !ctx->calibrating;
    bool launched = false;
    if (use_graph) {
        mdhip_ctx::GraphSlot& g = ctx->graphs[std::make_tuple(n, h, w, ctx->pred_cur)];
        g.last_use = ++ctx->graph_clock;
        if (g.exec) {
            HIP_TRY(ctx, hipGraphLaunch(g.exec, s));
            launched = true;
        } else if (!g.disabled && ++g.seen >= 2) {
            // the first forward of a shape runs eagerly (it settles the tile choices: a stale table entry is replaced on
            // its first failing launch); the second is captured on an internal stream and replayed from then on.  A
            // capture or instantiation that fails disables replay for this shape: the eager path below just worked.
            if (!ctx->capture_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->capture_stream, hipStreamNonBlocking));
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            bool ok = hipStreamBeginCapture(ctx->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                ok = pass.run(n, h, w, ctx->capture_stream) == MDHIP_OK;
                ok = (hipStreamEndCapture(ctx->capture_stream, &graph) == hipSuccess) && ok && graph != nullptr;
            }
            if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess && exec != nullptr;
            if (graph) (void)hipGraphDestroy(graph);
            if (!ok) {
                (void)hipGetLastError();
                if (exec) (void)hipGraphExecDestroy(exec);
                g.disabled = true;
            } else {
                // (evict_graph_if_full may erase other map entries: std::map references to `g` stay valid)
                evict_graph_if_full(ctx);
                g.exec = exec;
                HIP_TRY(ctx, hipGraphLaunch(g.exec, s));
                launched = true;
            }
        }
    }
    // eager: the ops up to the last one that reads the network input, then the rest; behind a replayed graph: none
    const size_t head = launched ? 0 : (size_t)ctx->last_input_op + 1, rest = launched ? 0 : ctx->ops.size();
    if (int rc = pass.run(n, h, w, s, 0, head)) return rc;
    if (int rc = pass.input_done(false)) return rc;
    if (int rc = pass.run(n, h, w, s, head, rest)) return rc;
    if (ctx->time_forward) {
        HIP_TRY(ctx, hipEventRecord(ctx->fwd_ev[slot][1], s));
        ++ctx->fwd_count;
    }
    pass.finish(n, h, w);
    return MDHIP_OK;
}

// yolov5 models/yolo.py:_forward_augment (what `model(batch, augment=True)` runs, reference
// pytorch_detector.py:1313): three passes at scales 1 / 0.83 (left-right flipped) / 0.67 of the letterboxed
// batch, boxes de-scaled and un-flipped, the largest-stride level of the first pass and the smallest-stride
// level of the last pass dropped (_clip_augmented), predictions concatenated along the anchor axis.
int mdhip_forward_tta(mdhip_ctx* ctx, int n, int h, int w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (ctx->anchor_free)
        return fail(ctx, MDHIP_EUNSUPPORTED, "mdhip_forward_tta: augmented inference is implemented for YOLOv5 (anchor-based) "
                                             "models only, not for anchor-free (YOLO11) models");
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (ctx->last_n < n || ctx->last_h != h || ctx->last_w != w)
        return fail(ctx, MDHIP_EINVAL, "mdhip_forward_tta needs mdhip_preprocess of the same batch first");
    if (int rc = check_calibrated(ctx)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    TtaPass g3[3];
    int A[3];
    for (int k = 0; k < 3; ++k) {
        g3[k] = tta_pass(ctx, h, w, k);
        A[k] = num_anchors_for(ctx, g3[k].oh, g3[k].ow);
    }
    long long g = 0, p4 = 1;
    for (int l = 0; l < ctx->nl; ++l) { g += p4; if (l + 1 < ctx->nl) p4 *= 4; }      // p4 = 4^(nl-1)
    const int i1 = (int)(A[0] / g), i3 = (int)((A[2] / g) * p4);
    const int total = (A[0] - i1) + A[1] + (A[2] - i3);
    if (total > ctx->a_cap || i1 >= A[0] || i3 >= A[2])
        return fail(ctx, MDHIP_ENOMEM, "augmented prediction of %d anchors exceeds the planned %d", total, ctx->a_cap);
    const size_t in_bytes = (size_t)n * (h / 2) * (w / 2) * 16 * 2;
    uint16_t* in = (uint16_t*)(ctx->arena + ctx->input.off);
    uint16_t* orig = (uint16_t*)(ctx->arena + ctx->input_orig.off);
    HIP_TRY(ctx, hipMemcpyAsync(orig, in, in_bytes, hipMemcpyDeviceToDevice, s));
    const int f16 = ctx->dtype == MDHIP_DTYPE_FP16;
    Pass pass(ctx, s, total);
    if (int rc = pass.flip_prediction()) return rc;
    int out_off = 0;
    for (int k = 0; k < 3; ++k) {
        const TtaPass& tp = g3[k];
        if (k) HIP_TRY(ctx, launch_tta_scale(orig, in, n, h, w, tp.sh, tp.sw, tp.oh, tp.ow, tp.flip, f16, s));
        DecodeTta t;
        t.keep_from = k == 2 ? i3 : 0;
        t.keep_to = k == 0 ? A[0] - i1 : A[k];
        t.out_off = out_off;
        t.scale = tp.scale;
        t.flip_lr = tp.flip;
        t.img_w = (float)w;
        ctx->cur_tta = t;
        if (int rc = pass.run(n, tp.oh, tp.ow, s)) return rc;
        out_off += t.keep_to - t.keep_from;
    }
    HIP_TRY(ctx, hipMemcpyAsync(in, orig, in_bytes, hipMemcpyDeviceToDevice, s));       // `input` holds the batch again
    if (int rc = pass.input_done(false)) return rc;
    pass.finish(n, h, w);
    return MDHIP_OK;
}

// fp8 mode (BASELINE.json configs[4]).  The reference has no reduced precision (pytorch_detector.py:848
// half_precision = False), so there is nothing upstream to mirror: post-training static quantisation of the hidden
// tensor of every bottleneck, per-tensor activation scale from the largest magnitude seen on the calibration batches
// (x FP8_RANGE_MARGIN head-room), per-output-channel weight scales fixed at mdhip_create.
static constexpr float kFp8RangeMargin = 2.0f;

int mdhip_calibrate(mdhip_ctx* ctx, int n, int h, int w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (ctx->dtype != MDHIP_DTYPE_FP8) return fail(ctx, MDHIP_EINVAL, "mdhip_calibrate: not an fp8 context");
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (ctx->last_n < n || ctx->last_h != h || ctx->last_w != w)
        return fail(ctx, MDHIP_EINVAL, "mdhip_calibrate needs mdhip_preprocess of the same batch first");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (Op& op : ctx->ops)
        if (op.f8_out) HIP_TRY(ctx, hipMemsetAsync(ctx->arena + op.amax_off, 0, 4, s));
    // one forward in 16 bits (every op, the 3x3 convs through their bf16 weights), ranges recorded on the way
    Pass pass(ctx, s, num_anchors_for(ctx, h, w), false, true);
    if (int rc = pass.run(n, h, w, s)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    (void)pass.input_done(true);
    for (Op& op : ctx->ops) {
        if (!op.f8_out) continue;
        float m = 0.f;
        HIP_TRY(ctx, hipMemcpy(&m, ctx->arena + op.amax_off, 4, hipMemcpyDeviceToHost));
        if (!(m == m) || m > 3.0e38f) return fail(ctx, MDHIP_EINVAL, "calibration saw a non-finite activation in %s", op.name.c_str());
        op.amax = std::max(op.amax, m);                                   // ranges accumulate over calibration calls
        const float scale = std::max(op.amax, 1e-20f) * kFp8RangeMargin / 448.0f;
        if (int r2 = apply_fp8_scale(ctx, op, scale)) return r2;
    }
    ctx->calibrated = true;
    pass.finish(ctx->last_n, h, w);                     // (the batch mdhip_preprocess wrote stays the context's)
    return MDHIP_OK;
}

int mdhip_fp8_num_tensors(mdhip_ctx* ctx) { return ctx ? ctx->n_f8 : MDHIP_EINVAL; }

int mdhip_f32_to_e4m3(const float* in, uint8_t* out, int n) {
    if (!in || !out || n < 0) return MDHIP_EINVAL;
    for (int i = 0; i < n; ++i) out[i] = f32_to_e4m3(in[i]);
    return MDHIP_OK;
}

int mdhip_fp8_get_scales(mdhip_ctx* ctx, float* scales, int32_t* layers, int32_t* ops, int max_n) {
    NEED_MODEL(ctx);
    if (!ctx || max_n < 0) return MDHIP_EINVAL;
    int k = 0;
    for (size_t i = 0; i < ctx->ops.size(); ++i) {
        const Op& op = ctx->ops[i];
        if (!op.f8_out) continue;
        if (k < max_n) {
            if (scales) scales[k] = op.act_scale;
            if (layers) layers[k] = op.layer;
            if (ops) ops[k] = (int32_t)i;
        }
        ++k;
    }
    return k;
}

int mdhip_fp8_set_scales(mdhip_ctx* ctx, const float* scales, int n) {
    NEED_MODEL(ctx);
    if (!ctx || !scales) return MDHIP_EINVAL;
    if (ctx->dtype != MDHIP_DTYPE_FP8) return fail(ctx, MDHIP_EINVAL, "mdhip_fp8_set_scales: not an fp8 context");
    if (n != ctx->n_f8) return fail(ctx, MDHIP_EINVAL, "%d scales for %d fp8 tensors", n, ctx->n_f8);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int k = 0;
    for (Op& op : ctx->ops) {
        if (!op.f8_out) continue;
        const float sc = scales[k++];
        if (!(sc > 0.f) || sc > 3.0e38f) return fail(ctx, MDHIP_EINVAL, "scale %d is not a positive finite number", k - 1);
        op.amax = sc * 448.0f / kFp8RangeMargin;
        if (int rc = apply_fp8_scale(ctx, op, sc)) return rc;
    }
    ctx->calibrated = true;
    return MDHIP_OK;
}

int mdhip_last_num_anchors(mdhip_ctx* ctx) { return ctx ? ctx->last_A : 0; }

int mdhip_time_forwards(mdhip_ctx* ctx, int enable) {
    NEED_MODEL(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (enable && !ctx->fwd_ev[0][0])
        for (int i = 0; i < mdhip_ctx::kFwdRing; ++i)
            for (int k = 0; k < 2; ++k) HIP_TRY(ctx, hipEventCreate(&ctx->fwd_ev[i][k]));
    ctx->time_forward = enable != 0;
    ctx->fwd_count = 0;
    return MDHIP_OK;
}

int mdhip_forward_times(mdhip_ctx* ctx, float* ms, int max_n) {
    NEED_MODEL(ctx);
    if (!ctx || !ms || max_n < 0) return MDHIP_EINVAL;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const long long have = std::min<long long>(ctx->fwd_count, mdhip_ctx::kFwdRing);
    const int n = (int)std::min<long long>(have, max_n);
    for (int i = 0; i < n; ++i) {                       // the most recent n forwards, oldest first
        const int slot = (int)((ctx->fwd_count - n + i) % mdhip_ctx::kFwdRing);
        HIP_TRY(ctx, hipEventSynchronize(ctx->fwd_ev[slot][1]));
        HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->fwd_ev[slot][0], ctx->fwd_ev[slot][1]));
    }
    return n;
}

int mdhip_forward_timed(mdhip_ctx* ctx, int n, int h, int w, float* ms, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !ms) return MDHIP_EINVAL;
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (int rc = check_calibrated(ctx)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t need = ctx->ops.size() + 1;
    while (ctx->events.size() < need) {
        hipEvent_t ev;
        HIP_TRY(ctx, hipEventCreate(&ev));
        ctx->events.push_back(ev);
    }
    HIP_TRY(ctx, hipEventRecord(ctx->events[0], s));
    Pass pass(ctx, s, num_anchors_for(ctx, h, w));
    for (size_t i = 0; i < ctx->ops.size(); ++i) {
        if (int rc = pass.run(n, h, w, s, i, 1)) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->events[i + 1], s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    (void)pass.input_done(true);
    for (size_t i = 0; i < ctx->ops.size(); ++i)
        HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->events[i], ctx->events[i + 1]));
    pass.finish(n, h, w);
    return MDHIP_OK;
}

int mdhip_time_op(mdhip_ctx* ctx, int op, int n, int h, int w, int iters, float* ms_avg, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !ms_avg || op < 0 || op >= (int)ctx->ops.size() || iters < 1) return MDHIP_EINVAL;
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (int rc = check_calibrated(ctx)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    while (ctx->events.size() < 2) {
        hipEvent_t ev;
        HIP_TRY(ctx, hipEventCreate(&ev));
        ctx->events.push_back(ev);
    }
    // one op in isolation: a bottleneck's two convs as the two launches they are, an upsample and a decode op as their own
    Pass pass(ctx, s, num_anchors_for(ctx, h, w), true);
    if (int rc = pass.run(n, h, w, s, op, 1)) return rc;              // warm
    HIP_TRY(ctx, hipEventRecord(ctx->events[0], s));
    for (int i = 0; i < iters; ++i)
        if (int rc = pass.run(n, h, w, s, op, 1)) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->events[1], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->events[0], ctx->events[1]));
    *ms_avg = ms / iters;
    return MDHIP_OK;
}

static int nms_common(mdhip_ctx* ctx, const float* pred_dev, int n, int n_anchors, float conf_thres,
                      float iou_thres, int max_det, float* out, int32_t* counts, hipStream_t s) {
    if (!out || !counts) return fail(ctx, MDHIP_EINVAL, "out/counts is NULL");
    if (n < 1 || n > ctx->max_batch) return fail(ctx, MDHIP_EINVAL, "batch %d outside [1,%d]", n, ctx->max_batch);
    if (max_det < 1 || max_det > kNmsMaxDet) return fail(ctx, MDHIP_EINVAL, "max_det %d outside [1,%d]", max_det, kNmsMaxDet);
    if (n_anchors < 1 || n_anchors > ctx->a_cap) return fail(ctx, MDHIP_EINVAL, "n_anchors %d outside [1,%d]", n_anchors, ctx->a_cap);
    float* out_dev = (float*)(ctx->arena + ctx->nms_out_off);
    int* cnt_dev = (int*)(ctx->arena + ctx->nms_cnt_off);
    HIP_TRY(ctx, launch_nms(pred_dev, n, n_anchors, ctx->no, conf_thres, iou_thres, max_det, ctx->nms_scr, out_dev, cnt_dev, s,
                            ctx->anchor_free));
    HIP_TRY(ctx, hipMemcpyAsync(out, out_dev, (size_t)n * max_det * 6 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(counts, cnt_dev, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return MDHIP_OK;
}

int mdhip_nms(mdhip_ctx* ctx, int n, float conf_thres, float iou_thres, int max_det, float* out,
              int32_t* counts, void* hip_stream) {
    NEED_MODEL(ctx);
    if (ctx->last_h == 0) return fail(ctx, MDHIP_EINVAL, "mdhip_nms before mdhip_forward");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int A = ctx->last_A;
    return nms_common(ctx, (const float*)(ctx->arena + ctx->pred_off), n, A, conf_thres, iou_thres,
                      max_det, out, counts, (hipStream_t)hip_stream);
}

int mdhip_nms_enqueue(mdhip_ctx* ctx, int n, float conf_thres, float iou_thres, int max_det, int slot,
                      void* hip_stream) {
    NEED_MODEL(ctx);
    if (ctx->last_h == 0) return fail(ctx, MDHIP_EINVAL, "mdhip_nms_enqueue before mdhip_forward");
    if (slot < 0 || slot >= MDHIP_NMS_SLOTS) return fail(ctx, MDHIP_EINVAL, "slot %d outside [0,%d)", slot, MDHIP_NMS_SLOTS);
    if (n < 1 || n > ctx->max_batch) return fail(ctx, MDHIP_EINVAL, "batch %d outside [1,%d]", n, ctx->max_batch);
    if (max_det < 1 || max_det > kNmsMaxDet) return fail(ctx, MDHIP_EINVAL, "max_det %d outside [1,%d]", max_det, kNmsMaxDet);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int A = ctx->last_A;
    float* out_dev = (float*)(ctx->arena + ctx->nms_out_off);
    int* cnt_dev = (int*)(ctx->arena + ctx->nms_cnt_off);
    HIP_TRY(ctx, launch_nms((const float*)(ctx->arena + ctx->pred_off), n, A, ctx->no, conf_thres, iou_thres, max_det,
                            ctx->nms_scr, out_dev, cnt_dev, s, ctx->anchor_free));
    HIP_TRY(ctx, hipEventRecord(ctx->pred_read[ctx->pred_cur], s));
    ctx->pred_read_valid[ctx->pred_cur] = true;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->nms_host_out[slot], out_dev, (size_t)n * max_det * 6 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->nms_host_cnt[slot], cnt_dev, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ctx->nms_ev[slot], s));
    ctx->nms_slot_n[slot] = n;
    return MDHIP_OK;
}

int mdhip_nms_wait(mdhip_ctx* ctx, int slot, const float** out, const int32_t** counts) {
    NEED_MODEL(ctx);
    if (!ctx || !out || !counts) return MDHIP_EINVAL;
    if (slot < 0 || slot >= MDHIP_NMS_SLOTS || ctx->nms_slot_n[slot] == 0)
        return fail(ctx, MDHIP_EINVAL, "nothing enqueued in slot %d", slot);
    HIP_TRY(ctx, hipEventSynchronize(ctx->nms_ev[slot]));
    *out = ctx->nms_host_out[slot];
    *counts = ctx->nms_host_cnt[slot];
    return MDHIP_OK;
}

int mdhip_nms_on(mdhip_ctx* ctx, const float* pred, int n, int n_anchors, float conf_thres,
                 float iou_thres, int max_det, float* out, int32_t* counts, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!pred) return fail(ctx, MDHIP_EINVAL, "pred is NULL");
    if (n < 1 || n > ctx->max_batch || n_anchors < 1 || n_anchors > ctx->a_cap)
        return fail(ctx, MDHIP_EINVAL, "n=%d n_anchors=%d outside the context capacity (%d x %d)", n, n_anchors, ctx->max_batch, ctx->a_cap);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float* pred_dev = (float*)(ctx->arena + ctx->pred_off);
    HIP_TRY(ctx, hipMemcpyAsync(pred_dev, pred, (size_t)n * n_anchors * ctx->no * 4, hipMemcpyHostToDevice, s));
    ctx->last_A = n_anchors;          // the context's prediction is now this tensor
    return nms_common(ctx, pred_dev, n, n_anchors, conf_thres, iou_thres, max_det, out, counts, s);
}

int mdhip_read_predictions(mdhip_ctx* ctx, int n, float* out, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !out) return MDHIP_EINVAL;
    if (ctx->last_h == 0 || n < 1 || n > ctx->last_n) return fail(ctx, MDHIP_EINVAL, "no forward result for n=%d", n);
    hipStream_t s = (hipStream_t)hip_stream;
    const int A = ctx->last_A;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->arena + ctx->pred_off, (size_t)n * A * ctx->no * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return MDHIP_OK;
}

int mdhip_read_input(mdhip_ctx* ctx, int n, int h, int w, float* out, void* hip_stream) {
    NEED_MODEL(ctx);
    if (!ctx || !out) return MDHIP_EINVAL;
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    float* tmp = nullptr;
    const size_t bytes = (size_t)n * 3 * h * w * 4;
    HIP_TRY(ctx, hipMalloc((void**)&tmp, bytes));
    hipError_t e = launch_s2d_to_nchw_f32((const uint16_t*)(ctx->arena + ctx->input.off), tmp, n, h, w, ctx->dtype == MDHIP_DTYPE_FP16, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    HIP_TRY(ctx, e);
    return MDHIP_OK;
}

int mdhip_read_layer(mdhip_ctx* ctx, int layer, int n, float* out, int* c, int* h, int* w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (layer < 0 || layer >= (int)ctx->layer_out.size() || !ctx->layer_out[layer].valid)
        return fail(ctx, MDHIP_EINVAL, "layer %d has no readable output", layer);
    if (ctx->last_h == 0) return fail(ctx, MDHIP_EINVAL, "mdhip_read_layer before mdhip_forward");
    const Tensor& t = ctx->layer_out[layer];
    const int H = ctx->last_h / t.div, W = ctx->last_w / t.div;
    if (c) *c = t.c;
    if (h) *h = H;
    if (w) *w = W;
    if (!out) return MDHIP_OK;
    if (n < 1 || n > ctx->last_n) return fail(ctx, MDHIP_EINVAL, "n=%d outside the last forward's batch %d", n, ctx->last_n);
    hipStream_t s = (hipStream_t)hip_stream;
    float* tmp = nullptr;
    const size_t bytes = (size_t)n * t.c * H * W * 4;
    HIP_TRY(ctx, hipMalloc((void**)&tmp, bytes));
    hipError_t e = launch_nhwc_to_nchw_f32((const uint16_t*)(ctx->arena + t.off), t.ld, tmp, n, t.c, H, W, ctx->dtype == MDHIP_DTYPE_FP16, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    HIP_TRY(ctx, e);
    return MDHIP_OK;
}

// ---- a forward op by op (tests/op_step.py): run a range of ops, read what an op reads and writes, read what it multiplies ----

int mdhip_run_ops(mdhip_ctx* ctx, int n, int h, int w, int first, int count, void* hip_stream) {
    NEED_MODEL(ctx);
    if (int rc = check_shape(ctx, n, h, w)) return rc;
    if (int rc = check_calibrated(ctx)) return rc;
    const int n_ops = (int)ctx->ops.size();
    if (first < 0 || count < 0 || first > n_ops || count > n_ops - first)
        return fail(ctx, MDHIP_EINVAL, "mdhip_run_ops: ops [%d,%d) outside [0,%d]", first, first + count, n_ops);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // every op as its own launch, as mdhip_time_op runs one
    Pass pass(ctx, s, num_anchors_for(ctx, h, w), true);
    if (first == 0)
        if (int rc = pass.flip_prediction()) return rc;
    if (int rc = pass.run(n, h, w, s, (size_t)first, (size_t)count)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (first + count == n_ops) {
        (void)pass.input_done(true);
        pass.finish(n, h, w);
    } else {
        ctx->last_ran = pass.ran;          // (mdhip_get_op_info: the tiles of the pass that is being stepped)
        ctx->step_n = n; ctx->step_h = h; ctx->step_w = w;
    }
    return MDHIP_OK;
}

int mdhip_read_op_tensor(mdhip_ctx* ctx, int op, int which, int n, float* out, int* c, int* h, int* w, void* hip_stream) {
    NEED_MODEL(ctx);
    if (op < 0 || op >= (int)ctx->ops.size()) return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_tensor: op %d outside [0,%d)", op, (int)ctx->ops.size());
    if (which < 0 || which > 6) return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_tensor: which %d outside [0,6]", which);
    const Op& o = ctx->ops[op];
    if (o.kind == OP_DECODE || o.kind == OP_DFL)
        return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_tensor: op %d (%s) is a decode: read the conv in front and mdhip_read_predictions", op, o.name.c_str());
    const bool f32 = which == 1 && o.kind == OP_CONV && o.out_f32;
    const Tensor& t = which == 0 ? o.in : which == 1 ? o.out : which == 2 ? o.res : which == 3 ? o.out2 : o.fsrc[which - 4];
    if (!t.valid || (which == 2 && !o.has_res) || (which >= 4 && which - 4 >= o.n_fsrc))
        return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_tensor: op %d (%s) has no tensor %d", op, o.name.c_str(), which);
    if (ctx->dtype == MDHIP_DTYPE_FP8 && ((which == 0 && o.f8_in) || (which == 1 && o.f8_out)))
        return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_tensor: tensor %d of op %d (%s) is e4m3", which, op, o.name.c_str());
    const int ph = ctx->step_h ? ctx->step_h : ctx->last_h, pw = ctx->step_h ? ctx->step_w : ctx->last_w;
    const int pn = ctx->step_h ? ctx->step_n : ctx->last_n;
    if (ph == 0) return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_tensor before mdhip_run_ops or mdhip_forward");
    const bool net_input = t.off == ctx->input.off;      // space-to-depth: returned as mdhip_read_input returns it
    const int H = net_input ? ph : ph / t.div, W = net_input ? pw : pw / t.div, C = net_input ? 3 : t.c;
    if (c) *c = C;
    if (h) *h = H;
    if (w) *w = W;
    if (!out) return MDHIP_OK;
    if (n < 1 || n > pn) return fail(ctx, MDHIP_EINVAL, "n=%d outside the last pass's batch %d", n, pn);
    if (net_input) return mdhip_read_input(ctx, n, ph, pw, out, hip_stream);
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (f32) {                       // fp32 logits [pixel][f32_ld]: transposed on the host
        const size_t px = (size_t)n * H * W;
        std::vector<float> host(px * o.f32_ld);
        HIP_TRY(ctx, hipMemcpyAsync(host.data(), ctx->arena + o.f32_off, host.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        for (int b = 0; b < n; ++b)
            for (int ch = 0; ch < C; ++ch)
                for (int p = 0; p < H * W; ++p) out[((size_t)b * C + ch) * H * W + p] = host[((size_t)b * H * W + p) * o.f32_ld + ch];
        return MDHIP_OK;
    }
    float* tmp = nullptr;
    const size_t bytes = (size_t)n * C * H * W * 4;
    HIP_TRY(ctx, hipMalloc((void**)&tmp, bytes));
    hipError_t e = launch_nhwc_to_nchw_f32((const uint16_t*)(ctx->arena + t.off), t.ld, tmp, n, C, H, W, ctx->dtype == MDHIP_DTYPE_FP16, s);
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    HIP_TRY(ctx, e);
    return MDHIP_OK;
}

int mdhip_read_op_weights(mdhip_ctx* ctx, int op, float* w, float* b, int* c_out, int* c_in, int* kh, int* kw) {
    NEED_MODEL(ctx);
    if (op < 0 || op >= (int)ctx->ops.size()) return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_weights: op %d outside [0,%d)", op, (int)ctx->ops.size());
    const Op& o = ctx->ops[op];
    if ((o.kind != OP_CONV && o.kind != OP_DW) || o.pc < 0)
        return fail(ctx, MDHIP_EINVAL, "mdhip_read_op_weights: op %d (%s) is neither a conv nor a depthwise conv", op, o.name.c_str());
    const PackedConv& pc = ctx->packed[o.pc];
    const bool stem = o.kind == OP_CONV && o.in.off == ctx->input.off;       // 6x6 taps over the space-to-depth cells
    const bool dw = o.kind == OP_DW;
    const int KH = stem ? 6 : pc.kh, KW = stem ? 6 : pc.kw, CI = stem ? 3 : dw ? 1 : pc.k_real / (pc.kh * pc.kw), CO = pc.c_out;
    if (c_out) *c_out = CO;
    if (c_in) *c_in = CI;
    if (kh) *kh = KH;
    if (kw) *kw = KW;
    if (!w && !b) return MDHIP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    const int f16 = ctx->dtype == MDHIP_DTYPE_FP16;
    if (b) HIP_TRY(ctx, hipMemcpy(b, ctx->warena + pc.b_off, (size_t)CO * 4, hipMemcpyDeviceToHost));
    if (!w) return MDHIP_OK;
    std::vector<uint16_t> p((size_t)pc.n_rows * pc.k_pad);
    HIP_TRY(ctx, hipMemcpy(p.data(), ctx->warena + pc.w_off, p.size() * 2, hipMemcpyDeviceToHost));
    for (int oc = 0; oc < CO; ++oc)
        for (int ci = 0; ci < CI; ++ci)
            for (int r = 0; r < KH; ++r)
                for (int q = 0; q < KW; ++q) {
                    size_t k;
                    if (dw) k = (size_t)(r * 3 + q) * CO + oc;                     // [9][C]
                    else if (stem) k = (size_t)oc * pc.k_pad + ((r >> 1) * 3 + (q >> 1)) * 16 + ((r & 1) * 2 + (q & 1)) * 3 + ci;
                    else k = (size_t)oc * pc.k_pad + (r * KW + q) * pc.cin_pad + ci;
                    w[(((size_t)oc * CI + ci) * KH + r) * KW + q] = st_to_f32(p[k], f16);
                }
    return MDHIP_OK;
}

int mdhip_num_ops(mdhip_ctx* ctx) { return ctx ? (int)ctx->ops.size() : MDHIP_EINVAL; }

int mdhip_get_op_info(mdhip_ctx* ctx, int op, mdhip_op_info* out) {
    NEED_MODEL(ctx);
    if (!ctx || !out || op < 0 || op >= (int)ctx->ops.size()) return MDHIP_EINVAL;
    const Op& o = ctx->ops[op];
    memset(out, 0, sizeof(*out));
    snprintf(out->name, sizeof(out->name), "%s", o.name.c_str());
    out->kind = o.kind == OP_DFL ? OP_DECODE : o.kind;       // (the DFL decode is reported as the decode op of its level)
    if (o.kind == OP_ADOWN || o.kind == OP_CBFUSE) out->kind = o.kind - 1;                  // 7 ADown pools, 8 CBFuse
    out->layer = o.layer;
    const Launch L = ctx->last_ran ? ctx->last_ran->ops[op] : Launch();      // (of the last forward; none yet: zeros)
    out->m = L.gm;
    out->n = L.gn;
    out->k = L.gk;
    out->flops = L.flops;
    out->bytes = L.bytes;
    // a conv with its own launch: its tile; -2 = a decode folded into the conv in front; -1 = anything else
    out->cfg = L.how == RUN_IN_FRONT ? -2 : (o.kind == OP_CONV && L.how == RUN_LAUNCH) ? L.cfg : -1;
    out->variant = -1;
    if (o.kind == OP_CONV && L.how == RUN_LAUNCH) {          // (the arguments as launch_op passes them on)
        ConvArgs a = L.a;
        float none = 0.f;
        a.dec_pred = L.decodes ? &none : nullptr;
        out->variant = conv_api(ctx).variant(L.cfg, a);
    }
    if (o.kind == OP_CONV || o.kind == OP_DW) {
        const PackedConv& pc = ctx->packed[o.pc];
        out->ntaps = pc.kh * pc.kw;
        out->stride = o.stride;
        out->has_res = o.has_res ? 1 : 0;
    }
    return MDHIP_OK;
}

int mdhip_num_conv_cfgs(void) { return conv_num_cfgs(); }

int mdhip_op_supports_cfg(mdhip_ctx* ctx, int op, int cfg) {
    NEED_MODEL(ctx);
    if (!ctx || op < 0 || op >= (int)ctx->ops.size()) return MDHIP_EINVAL;
    if (ctx->ops[op].kind != OP_CONV || cfg < 0 || cfg >= conv_num_cfgs()) return 0;
    ConvArgs a{};
    const int h = ctx->last_h ? ctx->last_h : ctx->max_stride, w = ctx->last_w ? ctx->last_w : ctx->max_stride;
    conv_args(ctx, ctx->ops[op], ctx->last_n ? ctx->last_n : 1, h, w, a);
    return conv_api(ctx).supports(cfg, a) ? 1 : 0;
}

const char* mdhip_conv_cfg_name(int cfg) { return (cfg >= 0 && cfg < conv_num_cfgs()) ? conv_cfg(cfg).name : ""; }

int mdhip_cfg_is_bitwise(int cfg) { return (cfg >= 0 && cfg < conv_num_cfgs() && conv_cfg_is_bitwise_family(cfg)) ? 1 : 0; }

int mdhip_set_tuned(mdhip_ctx* ctx, const mdhip_tuned* entries, int n) {
    NEED_MODEL(ctx);
    if (!ctx || n < 0 || (n > 0 && !entries)) return MDHIP_EINVAL;
    for (int i = 0; i < n; ++i)
        if (entries[i].cfg < 0 || entries[i].cfg >= conv_num_cfgs())
            return fail(ctx, MDHIP_EINVAL, "tuned entry %d: cfg %d outside [0,%d)", i, entries[i].cfg, conv_num_cfgs());
    ctx->tuned.assign(entries, entries + n);
    launches_changed(ctx);
    return MDHIP_OK;
}

int mdhip_set_fuse(mdhip_ctx* ctx, int on) {
    NEED_MODEL(ctx);
    ctx->fuse_enabled = on != 0;
    launches_changed(ctx);
    return MDHIP_OK;
}

int mdhip_set_option(mdhip_ctx* ctx, const char* name, int value) {
    NEED_MODEL(ctx);
    if (!ctx || !name) return MDHIP_EINVAL;
    if (!strcmp(name, "letterbox_general")) ctx->letterbox_general = value != 0;
    else if (!strcmp(name, "fuse_decode")) ctx->fuse_decode = value != 0;
    else if (!strcmp(name, "pw_stream")) ctx->pw_stream = value <= 0 ? 0 : value >= 2 ? 2 : 1;
    else return fail(ctx, MDHIP_EINVAL, "unknown option '%s'", name);
    launches_changed(ctx);
    return MDHIP_OK;
}

int mdhip_set_graph(mdhip_ctx* ctx, int mode, int max_n) {
    NEED_MODEL(ctx);
    if (!ctx || mode < 0 || mode > 2) return MDHIP_EINVAL;
    ctx->graph_mode = mode;
    if (max_n > 0) ctx->graph_max_n = max_n;
    if (mode == 0) drop_graphs(ctx);
    return MDHIP_OK;
}

int mdhip_set_op_cfg(mdhip_ctx* ctx, int op, int cfg) {
    NEED_MODEL(ctx);
    if (!ctx || op < 0 || op >= (int)ctx->ops.size()) return MDHIP_EINVAL;
    if (ctx->ops[op].kind != OP_CONV) return fail(ctx, MDHIP_EINVAL, "op %d is not a conv", op);
    if (cfg < -1 || cfg >= conv_num_cfgs()) return fail(ctx, MDHIP_EINVAL, "cfg %d outside [-1,%d)", cfg, conv_num_cfgs());
    ctx->ops[op].forced_cfg = cfg;
    launches_changed(ctx);
    return MDHIP_OK;
}

}  // extern "C"
