// The context behind the C ABI (include/mdhip.h) and what the host files that implement it share: mdhip_capi.cpp,
// mdhip_plan.cpp, mdhip_exec.cpp, mdhip_image_api.cpp, mdhip_kernel_hooks.cpp.  Private to these five: kernels and launchers see
// mdhip_internal.h alone.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mdhip.h"
#include "mdhip_internal.h"

using namespace mdhip;

namespace mdhip {

// records the text mdhip_last_error returns (ctx == nullptr: the one of a failed mdhip_create) and returns `code`
int fail(mdhip_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail(ctx, MDHIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                 \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int round_up(int x, int a) { return (x + a - 1) / a * a; }

// batch and input size against what the context was planned for
int check_shape(mdhip_ctx* ctx, int n, int h, int w);

// Pass k (0, 1, 2) of the augmented forward on an h x w input (mdhip_capi.cpp; yolov5 _forward_augment / scale_img): the batch,
// left-right flipped when `flip`, is resized to sh x sw and padded with 0.447 to oh x ow, the next multiple of the model stride.
// mdhip_forward_tta and the test hook mdhip_tta_input_on both take the geometry from here.
struct TtaPass { int sh, sw, oh, ow, flip; float scale; };
TtaPass tta_pass(const mdhip_ctx* ctx, int h, int w, int k);

// A context of mdhip_create_images has no plan, no weights and no arena: every entry point that reads one of them starts with
// NEED_MODEL, which refuses such a context (MDHIP_EINVAL, the call's name in mdhip_last_error) -- and a NULL one
int need_model(mdhip_ctx* ctx, const char* call);
#define NEED_MODEL(ctx)                                                   \
    do {                                                                  \
        if (!(ctx)) return MDHIP_EINVAL;                                  \
        if (int rc__ = need_model((ctx), __func__)) return rc__;          \
    } while (0)

// device scratch that a context keeps between calls: it grows to the largest request and never shrinks
struct DevBuffer {
    char* p = nullptr;
    size_t bytes = 0;
    // Work enqueued by an earlier call may still use the old memory, so growing waits first: for the stream `*wait`, or
    // for the whole device when `wait` is null.  A failed allocation leaves the buffer empty.
    int reserve(mdhip_ctx* ctx, size_t need, const hipStream_t* wait = nullptr) {
        if (need <= bytes) return MDHIP_OK;
        HIP_TRY(ctx, wait ? hipStreamSynchronize(*wait) : hipDeviceSynchronize());
        if (p) HIP_TRY(ctx, hipFree(p));
        p = nullptr;
        bytes = 0;
        char* q = nullptr;
        HIP_TRY(ctx, hipMalloc((void**)&q, need));
        p = q;
        bytes = need;
        return MDHIP_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

struct Tensor {
    size_t off = 0;   // byte offset into the arena
    int ld = 0;       // elements between consecutive pixels
    int c = 0;        // channels of the view
    int div = 1;      // spatial size = network input / div
    bool valid = false;
};

struct PackedConv {
    size_t w_off = 0, b_off = 0;     // byte offsets into the weight arena
    size_t w4_off = 0;               // second packing for the row-patch kernel (0 = none)
    int k_pad4 = 0, groups = 0;
    size_t w4p_off = 0;              // the same with the half-full last group's taps paired (conv_v5.cpp; 0 = none)
    int k_pad4p = 0;
    int n_rows = 0, k_pad = 0, cin_pad = 0, kh = 0, kw = 0, c_out = 0, k_real = 0;
    // fp8 form (MDHIP_DTYPE_FP8, 3x3 / stride-1 bottleneck convs): e4m3 weights [n_rows][groups8*9*128], quantised per
    // output channel (wscale[n] = max_k |w[n][k]| / 448); scale_off = device array of n_rows floats holding
    // activation scale x wscale[n], written by mdhip_calibrate / mdhip_fp8_set_scales
    size_t w8_off = 0, scale_off = 0;
    int k_pad8 = 0, groups8 = 0;
    std::vector<float> wscale;
};

enum OpKind { OP_CONV = 0, OP_POOL = 1, OP_UPSAMPLE = 2, OP_DECODE = 3, OP_COPY = 4, OP_DW = 5, OP_ATTN = 6, OP_DFL = 7,
              OP_ADOWN = 8, OP_CBFUSE = 9 };

struct Op {
    int kind = OP_CONV;
    int layer = -1;
    std::string name;
    Tensor in, out, res;
    bool has_res = false;
    int pc = -1;
    int stride = 1, pad = 0, act = 1, out_f32 = 0;
    int pool_k = 5;
    int level = 0;            // decode
    size_t f32_off = 0;       // decode: logits buffer offset ; conv with out_f32: same ; DFL decode: box logits
    int f32_ld = 0;
    size_t cls_off = 0;       // DFL decode: class logits (fp32, pitch cls_ld)
    int cls_ld = 0;
    int dw_grp = 0, dw_grp_stride = 0, dw_grp_off = 0;   // depthwise: input channel of output channel o (yolo11_kernels.cpp)
    int heads = 0;            // attention
    Tensor out2;              // ADown pools: the max-pooled half (out = the averaged half)
    Tensor fsrc[3];           // CBFuse: the CBLinear splits added to `in`, their nearest-resize factors
    int ffac[3] = {1, 1, 1};
    int n_fsrc = 0;
    int forced_cfg = -1;
    // fp8 mode: this op writes (f8_out) / reads (f8_in) an e4m3 tensor; f8_peer = the op at the other end of it;
    // act_scale = the tensor's scale (value = e4m3 x act_scale), 0 until calibrated; amax = largest |x| seen
    bool f8_out = false, f8_in = false;
    int f8_peer = -1;
    float act_scale = 0.f, amax = 0.f;
    // fused bottleneck (conv_v5c.cpp): fuse_role 1 = the 1x1 of bottleneck fuse_idx of C3 block fuse_group, 2 = its 3x3
    int fuse_group = -1, fuse_idx = -1, fuse_role = 0;
    // upsample read in place (conv_v2.cpp): an OP_UPSAMPLE whose only reader is the 1x1 conv `up_peer` (and vice versa)
    int up_peer = -1;
    size_t amax_off = 0;
};

// ---- mdhip_plan.cpp: everything mdhip_create does before its first device call ----

// the host copies of one packed conv's arrays, in the order they lie in the weight arena (an empty one has no place there)
struct PackedBlobs {
    std::vector<uint16_t> w;      // 16-bit weights [n_rows][k_pad]
    std::vector<float> b;         // bias [n_rows]
    std::vector<uint16_t> w4;     // row-patch packing
    std::vector<uint16_t> w4p;    // ... with the last group's taps paired
    std::vector<uint8_t> w8;      // e4m3 packing (its scales follow it in the arena: PackedConv::scale_off, zero until calibrated)
    struct Ref { const void* data; size_t bytes; size_t PackedConv::*off; };
    std::vector<Ref> refs() const {
        return {{w.data(), w.size() * 2, &PackedConv::w_off},    {b.data(), b.size() * 4, &PackedConv::b_off},
                {w4.data(), w4.size() * 2, &PackedConv::w4_off}, {w4p.data(), w4p.size() * 2, &PackedConv::w4p_off},
                {w8.data(), w8.size(), &PackedConv::w8_off}};
    }
};
struct PlannedWeights { std::vector<PackedBlobs> convs; };   // one per mdhip_ctx::packed entry

// Fills a fresh context from the model: sizes and strides, ops, layer views, packed convs (their host bytes go to `pw`), every
// arena and weight-arena offset.  Touches no device.  Returns MDHIP_OK, or the code mdhip_create fails with and its text in `err`.
int plan_context(mdhip_ctx* ctx, const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w, PlannedWeights* pw,
                 std::string* err);
// the planned context as text (mdhip_plan_describe)
std::string describe_plan(const mdhip_ctx* ctx, const PlannedWeights& pw);
int num_anchors_for(const mdhip_ctx* ctx, int h, int w);

// ---- mdhip_exec.cpp ----

// the conv kernel registry of the context's storage type (the kernels are compiled once per type, mdhip_internal.h)
const ConvRegistry& conv_api(const mdhip_ctx* ctx);
// tile configurations (count, names, families) are the same for both storage types
int conv_num_cfgs();
const ConvCfg& conv_cfg(int i);
bool conv_cfg_is_bitwise_family(int c);
void conv_args(const mdhip_ctx* ctx, const Op& op, int n, int h, int w, ConvArgs& a);

// What one op does in a pass, resolved for a shape and a kind of pass: its own launch (a conv: with tile `cfg`), inside the
// next op's launch (the 1x1 of a fused bottleneck), read in place by its consumer (an absorbed upsample), or decoded in the
// epilogue of the conv in front (a Detect decode).
enum RunHow { RUN_LAUNCH = 0, RUN_IN_NEXT = 1, RUN_IN_PLACE = 2, RUN_IN_FRONT = 3 };
struct Launch {
    int how = RUN_LAUNCH;
    int cfg = -1;
    bool from_table = false;      // the tile is a table entry: replaced by the heuristic if the launcher refuses it ...
    bool as_planned = true;       // ... and the op is neither fused nor reads an upsample in place
    bool decodes = false;         // this conv decodes its Detect level in its epilogue
    ConvArgs a{};                 // conv: the launch arguments that do not change between calls
    int gm = 0, gn = 0, gk = 0;   // statistics (mdhip_get_op_info)
    double flops = 0, bytes = 0;
};
struct Resolved {
    long long generation = 0;     // mdhip_ctx::generation it was resolved at
    int n = 0, h = 0, w = 0;
    std::vector<Launch> ops;      // one per mdhip_ctx::ops entry
};
std::shared_ptr<Resolved> resolved_for(mdhip_ctx* ctx, int n, int h, int w);
int launch_ops(mdhip_ctx* ctx, Resolved& r, size_t first, size_t count, hipStream_t s);
std::string describe_launches(const mdhip_ctx* ctx, const Resolved& r);

}  // namespace mdhip

struct mdhip_ctx {
    int device = 0;
    bool images_only = false;     // made by mdhip_create_images: nothing below but the DevBuffers, err and the device is in use
    int dtype = 0;
    int max_batch = 0, max_h = 0, max_w = 0;
    int nc = 0, na = 0, nl = 0, no = 0;
    bool anchor_free = false;     // the model ends in MDHIP_DETECT_DFL: predictions [cx, cy, w, h, cls...], ultralytics NMS
    std::vector<float> strides;
    int max_stride = 0;
    std::vector<mdhip_layer> layers;
    std::vector<Tensor> layer_out;
    std::vector<PackedConv> packed;
    std::vector<Op> ops;
    Tensor input;                 // space-to-depth network input (16 channels, div 2)
    Tensor input_orig;            // copy of it during test-time augmentation (the scaled passes overwrite `input`)
    DecodeTta cur_tta;            // how the Detect decode of the running pass places its anchors
    int cur_A = 0;                // anchors per image of the prediction being written (row pitch of `pred`)
    int last_A = 0;               // anchors per image of the last forward (plain or augmented)
    int a_cap = 0;                // capacity of `pred` and of the NMS scratch, anchors per image
    size_t arena_bytes = 0;
    char* arena = nullptr;
    char* warena = nullptr;       // packed weights + biases + zero page + anchors
    size_t warena_bytes = 0;
    size_t zero_off = 0, anchors_off = 0;
    // fp32 predictions [max_batch][a_cap][no], two of them: every forward writes the other one, so that the NMS of
    // batch i (on its own stream) may still read its predictions while the forward of batch i+1 runs
    size_t pred_offs[2] = {0, 0};
    int pred_cur = 0;
    size_t pred_off = 0;          // = pred_offs[pred_cur]: the prediction of the last forward
    int a_max = 0;
    NmsScratch nms_scr{};
    size_t nms_kv_off[6] = {}, nms_seg_off = 0;   // what nms_scr's keys / vals / seg_cnt point at once the arena exists
    size_t nms_out_off = 0, nms_cnt_off = 0;
    size_t geom_off = 0;
    DevBuffer stage;              // device staging for host images
    DevBuffer jpeg_planes;        // mdhip_jpeg_reconstruct / _recompress: u8 component planes between the IDCT and the colour kernel
    DevBuffer jpeg_entropy;       // mdhip_jpeg_entropy_decode: descriptors, lane records, block energies
    DevBuffer jpeg_encode;        // mdhip_jpeg_encode: crops, tables, coefficients, lengths, offsets, bit buffer
    DevBuffer blur;               // mdhip_blur_regions: the rectangles' records and their two planes
    DevBuffer resample;           // mdhip_resample_lanczos: coefficient tables, records, the images between the two passes
    DevBuffer draw;               // mdhip_draw_ops: the images' records and the operations
    DevBuffer classify;           // mdhip_classifier_input: the float table, the crops' records, the coefficient tables
    DevBuffer gray;               // mdhip_gray_count: the windows' records and their counters
    DevBuffer change;             // mdhip_change_detect: records, results, first-pass planes, masks, labels and sums of a group of pairs
    long long jpeg_entropy_stats[4] = {0, 0, 0, 0};   // of the last call: lanes, lanes decoded again, pass-2 launches, images
    int last_n = 0, last_h = 0, last_w = 0;
    int step_n = 0, step_h = 0, step_w = 0;   // of a pass that mdhip_run_ops has begun and not finished (0: none)
    std::string err;
    // fp8 mode: until every e4m3 tensor has a scale (mdhip_calibrate / mdhip_fp8_set_scales) the forward refuses
    // to run; `calibrating` (the pass of mdhip_calibrate) runs every op in 16 bits and records the range of the tensors
    bool calibrated = false, calibrating = false;
    int n_f8 = 0;
    // C3 blocks whose bottlenecks can run as one launch each (1x1 -> LDS -> 3x3): op indices of the 3x3s per block
    std::vector<std::vector<int>> fuse_groups;
    bool fuse_enabled = true, fuse_suspended = false;
    bool pair_enabled = true;         // paired taps of a half-full last channel group (conv_v5.cpp); MDHIP_PAIR=0 at create: off
    bool fuse_decode = true;          // Detect decode in the epilogue of the Detect 1x1 convs (mdhip_set_option "fuse_decode")
    int pw_stream = 1;                // streaming body for the 160 -> 160 channel 1x1 convs: ConvArgs::pw_stream (mdhip_set_option "pw_stream")
    bool letterbox_general = false;   // MDHIP_LETTERBOX_GENERAL at create: never take the streaming-copy letterbox (A/B, tests)
    std::vector<hipEvent_t> events;
    std::vector<mdhip_tuned> tuned;   // measured tile choices (tools/autotune.py)
    // optional event pair around every mdhip_forward (bench.py's live roofline measurement)
    static constexpr int kFwdRing = 64;
    bool time_forward = false;
    hipEvent_t fwd_ev[kFwdRing][2] = {};
    long long fwd_count = 0;
    // pinned host staging: letterbox geometry ring + asynchronous NMS result slots
    uint8_t* geom_host = nullptr;      // 4 slots of max_batch * sizeof(LetterboxWin) (the larger of the two geometry records)
    int geom_slot = 0;
    hipEvent_t geom_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float* nms_host_out[MDHIP_NMS_SLOTS] = {};
    int32_t* nms_host_cnt[MDHIP_NMS_SLOTS] = {};
    hipEvent_t nms_ev[MDHIP_NMS_SLOTS] = {};
    int nms_slot_n[MDHIP_NMS_SLOTS] = {};
    // mdhip_set_graph: the op sequence of a forward captured once per (batch, height, width, prediction buffer) and
    // replayed with one hipGraphLaunch (small batches are bound by ~160 launches of a few microseconds of work each)
    int graph_mode = 0;                                   // 0 = off, 1 = on, 2 = on for batches <= graph_max_n
    int graph_max_n = 8;
    hipStream_t capture_stream = nullptr;
    // `disabled`: capture or instantiation failed once for this shape -- it runs eagerly from then on; `last_use`: LRU stamp
    struct GraphSlot { hipGraphExec_t exec = nullptr; int seen = 0; bool disabled = false; long long last_use = 0; };
    std::map<std::tuple<int, int, int, int>, GraphSlot> graphs;
    static constexpr int kMaxGraphs = 32;                 // cached executables (letterbox shapes x batch sizes x 2 buffers)
    long long graph_clock = 0;
    // What a pass launches, resolved once (mdhip_exec.cpp resolve) per (batch, height, width, kind of pass: plain / isolated /
    // calibrating) and `generation`, which every call that changes what a forward launches bumps (launches_changed in
    // mdhip_capi.cpp).  last_ran: the list of the last pass, whose statistics mdhip_get_op_info reports.
    std::map<std::tuple<int, int, int, int>, std::shared_ptr<Resolved>> resolved;
    static constexpr int kMaxResolved = 64;
    long long generation = 0;
    std::shared_ptr<Resolved> last_ran;
    // recorded on the forward's stream behind the last op that reads the network input (last_input_op): a following
    // mdhip_preprocess -- possibly on ANOTHER stream, next to the rest of this forward -- waits for it before it overwrites
    // the input tensor
    hipEvent_t input_free = nullptr;
    bool input_free_valid = false;
    int last_input_op = 0;        // the last op that reads the network input (a model may have several stems)
    // the NMS that reads prediction buffer k (possibly on another stream: mdhip_nms_enqueue) records pred_read[k]; the
    // forward that is about to overwrite buffer k waits for it -- the ordering is the library's, not the caller's
    hipEvent_t pred_read[2] = {nullptr, nullptr};
    bool pred_read_valid[2] = {false, false};
};
