// The planner: lowers a mdhip_model to the flat op list of a context, lays out its arena and packs the weights -- everything
// mdhip_create (mdhip_capi.cpp) does before its first device call.  Nothing here touches a device: plan_context runs on any
// machine, and describe_plan writes its result as text (mdhip_plan_describe; tests/test_plan_cpu.py pins the plans with it).
//
// Planning turns the YOLOv5 module list into a flat list of ops over channel-strided NHWC
// bf16 views of one device arena:
//   * Concat never copies: producers write straight into their channel slice of the consumer's
//     buffer (a copy op is emitted only for a producer that already lives elsewhere).
//   * C3:  cv1 and cv2 read the same input -> ONE implicit GEMM with the two weight sets
//     stacked along N writes the [m-branch | cv2] concat buffer; the bottleneck chain then
//     updates the first half in place (1x1 -> scratch, 3x3 (+residual) -> slice).
//   * the 6x6/s2 stem runs as a 3x3/s1 conv over the space-to-depth input the letterbox
//     kernel produces.
//   * Detect: per level a 1x1 implicit GEMM with fp32 output followed by the decode kernel.
//   * YOLO11 (anchor-free) models: C3k2 runs on ONE concat buffer (cv1 writes the first 2c channels, inner block j
//     appends its c channels, cv2 reads all of it); C2PSA as cv1 -> per PSA block qkv 1x1, attention kernel, depthwise
//     pe(v) added to its output, proj (+x), ffn (+x) -> cv2; Detect as the box / class branches of every level (convs,
//     depthwise convs, fp32 logits) and the DFL decode kernel.  The 3x3/s2 stem is a 3x3/s1 conv over the
//     space-to-depth input with the weights of the +1 cell zero.
//   * YOLOv9-C (anchor-free) models: RepNCSPELAN4 on ONE concat buffer (cv1 writes c3 channels, each branch -- RepNCSP, i.e.
//     the C3k lowering with n bottlenecks, then a 3x3 -- appends its c4 channels, cv4 reads all of it); ADown as one pool
//     launch (yolov9_kernels.cpp) feeding the existing stride-2 3x3 and a 1x1; SPPELAN as SPPF; CBLinear as a 1x1 without
//     activation; CBFuse as one kernel; DDetect as the box / class branches of every level (the grouped box conv expanded
//     block-diagonally) and the DFL decode kernel.  Silence is an alias; every Conv that reads the network input (through
//     Silence or not) is a stem.  Under a DualDDetect only the layers that reach the head that runs are lowered.

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "mdhip_ctx.h"

namespace {

// ---------------------------------------------------------------------------------------
// planner
// Arena offsets and the indices into ctx->packed follow the ORDER of the alloc(), out_view() and pack() / conv() / dw() calls:
// one per statement, never two as arguments of one call (their evaluation order is unspecified).  tests/test_plan_cpu.py
// holds the plans of every model family and fails on a slip.
// ---------------------------------------------------------------------------------------
struct Planner {
    mdhip_ctx* ctx;
    const mdhip_model* model;
    size_t cursor = 0;
    std::vector<PackedBlobs>* blobs;             // the packed bytes, one entry per ctx->packed entry
    std::vector<int> layer_c, layer_div;
    std::vector<int> concat_target, concat_choff;   // per producer layer
    std::vector<Tensor> concat_buf;                  // per concat layer
    std::vector<char> reach;                         // per layer: lowered (feeds the Detect head that runs)
    std::string error;

    // ld >= c: pixel pitch in elements (a pitch that is a multiple of 64 keeps every 128-byte K-slab row of
    // a pixel inside one cache line; the pad channels are never read or written)
    Tensor alloc(int c, int div, int ld = 0) {
        Tensor t;
        t.off = cursor;
        t.ld = ld > c ? ld : c;
        t.c = c;
        t.div = div;
        t.valid = true;
        const size_t px = (size_t)ctx->max_batch * (ctx->max_h / div) * (ctx->max_w / div);
        cursor = align_up(cursor + px * t.ld * 2, 256);
        return t;
    }
    size_t alloc_bytes(size_t bytes) {
        const size_t off = cursor;
        cursor = align_up(cursor + bytes, 256);
        return off;
    }
    static Tensor slice(const Tensor& t, int ch_off, int c) {
        Tensor s = t;
        s.off = t.off + (size_t)ch_off * 2;
        s.c = c;
        return s;
    }

    // what pack() takes: one or more OIHW fp32 convs (stacked along N); s2d_stem: the 6x6 / stride-2 stem as a 3x3 over the
    // space-to-depth input; min_c_out: pad the output channels with zero rows (the class conv of the anchor-free head: 3 -> 8)
    struct Packing {
        std::vector<const mdhip_conv*> cs;
        bool s2d_stem = false;
        int min_c_out = 0;
    };

    // to bf16 / fp16 [n_rows][k_pad], k = (r,s,c)
    int pack(const Packing& pk) {
        const std::vector<const mdhip_conv*>& cs = pk.cs;
        const bool s2d_stem = pk.s2d_stem;
        const int min_c_out = pk.min_c_out;
        PackedConv pc;
        const int f16 = ctx->dtype == MDHIP_DTYPE_FP16;
        const mdhip_conv* c0 = cs[0];
        int c_out = 0;
        for (auto* c : cs) c_out += c->c_out;
        c_out = std::max(c_out, min_c_out);
        if (s2d_stem) {
            pc.kh = pc.kw = 3;
            pc.cin_pad = 16;
            pc.k_real = 6 * 6 * 3;
        } else {
            pc.kh = c0->kh;
            pc.kw = c0->kw;
            pc.cin_pad = round_up(c0->c_in, 8);
            pc.k_real = c0->kh * c0->kw * c0->c_in;
        }
        pc.c_out = c_out;
        pc.n_rows = round_up(c_out, 16);
        pc.k_pad = round_up(pc.kh * pc.kw * pc.cin_pad, 64);
        std::vector<uint16_t> w((size_t)pc.n_rows * pc.k_pad, 0);
        std::vector<float> b(pc.n_rows, 0.f);
        int row0 = 0;
        for (auto* c : cs) {
            for (int o = 0; o < c->c_out; ++o) {
                uint16_t* dst = &w[(size_t)(row0 + o) * pc.k_pad];
                b[row0 + o] = c->bias ? c->bias[o] : 0.f;
                if (s2d_stem) {
                    // w6[o][c][6][6] -> w3[o][r'][s'][(dy*2+dx)*3 + c], 6x6 index = 2*r'+dy
                    for (int ci = 0; ci < 3; ++ci)
                        for (int r = 0; r < 6; ++r)
                            for (int s = 0; s < 6; ++s) {
                                const float v = c->weight[(((size_t)o * 3 + ci) * 6 + r) * 6 + s];
                                const int rp = r >> 1, dy = r & 1, sp = s >> 1, dx = s & 1;
                                dst[(rp * 3 + sp) * 16 + (dy * 2 + dx) * 3 + ci] = f32_to_st(v, f16);
                            }
                } else {
                    for (int ci = 0; ci < c->c_in; ++ci)
                        for (int r = 0; r < c->kh; ++r)
                            for (int s = 0; s < c->kw; ++s) {
                                const float v =
                                    c->weight[(((size_t)o * c->c_in + ci) * c->kh + r) * c->kw + s];
                                dst[(r * c->kw + s) * pc.cin_pad + ci] = f32_to_st(v, f16);
                            }
                }
            }
            row0 += c->c_out;
        }
        // 3x3 convs with at least 64 input channels also get the row-patch order:
        // k = (channel group of 64, tap, channel in group), every (group, tap) slab 64 wide (zero padded)
        std::vector<uint16_t> w4;
        if (!s2d_stem && pc.kh == 3 && pc.kw == 3 && pc.cin_pad >= 64) {
            pc.groups = (pc.cin_pad + 63) / 64;
            pc.k_pad4 = pc.groups * 9 * 64;
            w4.assign((size_t)pc.n_rows * pc.k_pad4, 0);
            for (int o = 0; o < pc.n_rows; ++o)
                for (int t = 0; t < 9; ++t)
                    for (int ci = 0; ci < pc.cin_pad; ++ci)
                        w4[(size_t)o * pc.k_pad4 + ((ci / 64) * 9 + t) * 64 + (ci % 64)] =
                            w[(size_t)o * pc.k_pad + t * pc.cin_pad + ci];
        }
        // a last group of at most 32 channels: the paired packing of conv_v5.cpp -- groups 0 .. G-2 as above; last group:
        // per kernel row r the slabs [ tap (r,0) ch 0..31 | tap (r,1) ch 0..31 ] and [ tap (r,2) ch 0..31 | zeros ]
        std::vector<uint16_t> w4p;
        if (!w4.empty() && (pc.cin_pad % 64) != 0 && (pc.cin_pad % 64) <= 32) {
            const int G = pc.groups, tail = pc.cin_pad % 64;
            pc.k_pad4p = (9 * (G - 1) + 6) * 64;
            w4p.assign((size_t)pc.n_rows * pc.k_pad4p, 0);
            for (int o = 0; o < pc.n_rows; ++o) {
                const uint16_t* src = &w4[(size_t)o * pc.k_pad4];
                uint16_t* dst = &w4p[(size_t)o * pc.k_pad4p];
                std::copy(src, src + (size_t)9 * (G - 1) * 64, dst);
                for (int r = 0; r < 3; ++r)
                    for (int sx = 0; sx < 3; ++sx)
                        for (int ci = 0; ci < tail; ++ci)
                            dst[((G - 1) * 9 + 2 * r + (sx == 2 ? 1 : 0)) * 64 + (sx == 1 ? 32 : 0) + ci] =
                                src[((G - 1) * 9 + r * 3 + sx) * 64 + ci];
            }
        }
        // fp8 mode: 3x3 convs whose input channel count is a multiple of 16 also get the e4m3 packing of
        // conv_f8.cpp: k = (channel group of 128, tap, channel in group), quantised from the fp32 weights
        std::vector<uint8_t> w8;
        if (ctx->dtype == MDHIP_DTYPE_FP8 && !s2d_stem && cs.size() == 1 && pc.kh == 3 && pc.kw == 3 && (c0->c_in % 16) == 0) {
            pc.groups8 = (c0->c_in + 127) / 128;
            pc.k_pad8 = pc.groups8 * 9 * 128;
            pc.wscale.assign(pc.n_rows, 1.0f);
            w8.assign((size_t)pc.n_rows * pc.k_pad8, 0);
            for (int o = 0; o < c0->c_out; ++o) {
                const float* wo = c0->weight + (size_t)o * c0->c_in * 9;
                float amax = 0.f;
                for (int k = 0; k < c0->c_in * 9; ++k) amax = std::max(amax, std::fabs(wo[k]));
                const float sc = amax > 0.f ? amax / 448.0f : 1.0f;
                pc.wscale[o] = sc;
                for (int ci = 0; ci < c0->c_in; ++ci)
                    for (int t = 0; t < 9; ++t)
                        w8[(size_t)o * pc.k_pad8 + ((ci / 128) * 9 + t) * 128 + (ci % 128)] = f32_to_e4m3(wo[ci * 9 + t] / sc);
            }
        }
        ctx->packed.push_back(pc);
        blobs->push_back({std::move(w), std::move(b), std::move(w4), std::move(w4p), std::move(w8)});
        return (int)ctx->packed.size() - 1;
    }

    // a depthwise 3x3 conv (mdhip_conv with c_in = 1): [9][C] 16-bit weights (tap-major: 8 channels per 16-byte load)
    int pack_dw(const mdhip_conv* c) {
        PackedConv pc;
        const int f16 = ctx->dtype == MDHIP_DTYPE_FP16;
        pc.kh = pc.kw = 3;
        pc.cin_pad = 1;
        pc.c_out = pc.n_rows = c->c_out;
        pc.k_pad = 9;
        pc.k_real = 9;
        std::vector<uint16_t> w((size_t)9 * c->c_out);
        std::vector<float> b(c->c_out);
        for (int o = 0; o < c->c_out; ++o) {
            for (int t = 0; t < 9; ++t) w[(size_t)t * c->c_out + o] = f32_to_st(c->weight[(size_t)o * 9 + t], f16);
            b[o] = c->bias ? c->bias[o] : 0.f;
        }
        ctx->packed.push_back(pc);
        blobs->push_back({std::move(w), std::move(b), {}, {}, {}});
        return (int)ctx->packed.size() - 1;
    }

    // appends an op of `kind` with its name (printf-style; `ap` = the arguments of `fmt`), input and output; the caller fills
    // in the rest through the reference (valid until the next op is appended)
    Op& vop(int kind, int layer, const Tensor& in, const Tensor& out, const char* fmt, va_list ap) {
        char nm[96];
        vsnprintf(nm, sizeof(nm), fmt, ap);
        Op op;
        op.kind = kind;
        op.layer = layer;
        op.name = nm;
        op.in = in;
        op.out = out;
        ctx->ops.push_back(op);
        return ctx->ops.back();
    }
    __attribute__((format(printf, 6, 7)))
    Op& add_op(int kind, int layer, const Tensor& in, const Tensor& out, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        Op& op = vop(kind, layer, in, out, fmt, ap);
        va_end(ap);
        return op;
    }

    // a depthwise 3x3: packs `c` and appends the op
    __attribute__((format(printf, 11, 12)))
    void dw(int layer, const mdhip_conv* c, const Tensor& in, const Tensor& out, bool act, const Tensor* res, int grp, int grp_stride,
            int grp_off, const char* fmt, ...) {
        const int pc = pack_dw(c);
        va_list ap;
        va_start(ap, fmt);
        Op& op = vop(OP_DW, layer, in, out, fmt, ap);
        va_end(ap);
        op.pc = pc;
        op.act = act ? 1 : 0;
        if (res) { op.res = *res; op.has_res = true; }
        op.dw_grp = grp;
        op.dw_grp_stride = grp_stride;
        op.dw_grp_off = grp_off;
    }

    bool conv_is(const mdhip_conv& c, int c_in, int c_out, int k) const {
        return c.c_in == c_in && (c_out < 0 || c.c_out == c_out) && c.kh == k && c.kw == k && c.weight && c.c_out > 0 && c.c_out % 8 == 0;
    }

    // the 3x3 / stride-2 / pad-1 stem of YOLO11 as the 6x6 / stride-2 / pad-2 stem with zero outer taps: original row
    // 2y + r - 1 = 2y + (r + 1) - 2, i.e. the 3x3 kernel sits at offset (1, 1) of the 6x6 one (a 3x3 over the
    // space-to-depth cells whose +1 cell weights are zero)
    std::vector<float> stem6_w;
    mdhip_conv stem6;

    // as the `out` of conv(): fp32 output (Detect logits) of pitch n_rows in a buffer of its own, allocated here
    const Tensor f32_out;

    // a conv in one statement: packs the weights, appends the op and names it
    __attribute__((format(printf, 10, 11)))
    Op& conv(int layer, const Packing& pk, const Tensor& in, const Tensor& out, int stride, int pad, bool act, const Tensor* res,
             const char* fmt, ...) {
        const int pc = pack(pk);
        va_list ap;
        va_start(ap, fmt);
        Op& op = vop(OP_CONV, layer, in, out, fmt, ap);
        va_end(ap);
        op.pc = pc;
        op.stride = stride;
        op.pad = pad;
        op.act = act ? 1 : 0;
        if (res) { op.res = *res; op.has_res = true; }
        if (!out.valid) {
            op.out_f32 = 1;
            op.f32_ld = ctx->packed[pc].n_rows;
            const size_t px = (size_t)ctx->max_batch * (ctx->max_h / in.div) * (ctx->max_w / in.div);
            op.f32_off = alloc_bytes(px * op.f32_ld * 4);
            op.out = in;          // spatial size only
            op.out.c = ctx->packed[pc].c_out;
        }
        return op;
    }

    // RepNCSP (yolov9) and C3k (YOLO11), ops named "L<i> <block>.<tag>. ...": b = cv1, cv2 (1x1 -> h), cv3 (1x1 2h -> dst.c), then
    // per bottleneck j m.j.cv1 (3x3; RepConvN folded), m.j.cv2 (3x3, + residual with `shortcut`).  YK (2h channels) and TK (h)
    // are scratch.
    bool repncsp(int i, const char* block, const char* tag, const mdhip_conv* b, int n, bool shortcut, const Tensor& src,
                 const Tensor& dst, const Tensor& YK, const Tensor& TK) {
        const int h = b[0].c_out;
        bool ok = h % 8 == 0 && 2 * h == YK.c && h == TK.c && conv_is(b[0], src.c, h, 1) && conv_is(b[1], src.c, h, 1) &&
                  conv_is(b[2], 2 * h, dst.c, 1);
        for (int j = 0; j < n; ++j) ok = ok && conv_is(b[3 + 2 * j], h, h, 3) && conv_is(b[4 + 2 * j], h, h, 3);
        if (!ok) { error = "RepNCSP shape mismatch at layer " + std::to_string(i) + " (" + tag + ")"; return false; }
        const Tensor Y1 = slice(YK, 0, h);
        conv(i, {{&b[0], &b[1]}}, src, YK, 1, 0, true, nullptr, "L%d %s.%s.cv1|cv2 1x1", i, block, tag);
        for (int j = 0; j < n; ++j) {
            conv(i, {{&b[3 + 2 * j]}}, Y1, TK, 1, 1, true, nullptr, "L%d %s.%s.m%d.cv1 3x3", i, block, tag, j);
            conv(i, {{&b[4 + 2 * j]}}, TK, Y1, 1, 1, true, shortcut ? &Y1 : nullptr, "L%d %s.%s.m%d.cv2 3x3", i, block, tag, j);
        }
        conv(i, {{&b[2]}}, YK, dst, 1, 0, true, nullptr, "L%d %s.%s.cv3 1x1", i, block, tag);
        return true;
    }

    // the end of a level of both anchor-free heads: the class logits (nc rows padded to 8: zero weights, zero bias) and the DFL
    // decode of the level, which reads them and the box logits that op `box` wrote
    void dfl_tail(int i, int l, const char* head, int box, const mdhip_conv* cls, const Tensor& cls_in, const Tensor& x) {
        conv(i, {{cls}, false, 8}, cls_in, f32_out, 1, 0, false, nullptr, "L%d %s.cv3.%d.2 1x1 (cls)", i, head, l);
        const int cls_op = (int)ctx->ops.size() - 1;
        Op& dec = add_op(OP_DFL, i, x, Tensor(), "L%d %s.dfl_decode%d", i, head, l);
        dec.level = l;
        dec.f32_off = ctx->ops[box].f32_off;
        dec.f32_ld = ctx->ops[box].f32_ld;
        dec.cls_off = ctx->ops[cls_op].f32_off;
        dec.cls_ld = ctx->ops[cls_op].f32_ld;
    }

    bool plan() {
        const int nL = model->n_layers;
        layer_c.assign(nL, 0);
        layer_div.assign(nL, 1);
        concat_target.assign(nL, -1);
        concat_choff.assign(nL, 0);
        concat_buf.assign(nL, Tensor());
        ctx->layer_out.assign(nL, Tensor());
        // pass 0: a model ending in a YOLOv9 head lowers only the layers that reach the head that runs (its from[]): under
        // DualDDetect the branch that feeds the other head is skipped.  Every other model lowers every layer.
        reach.assign(nL, 1);
        if (model->layers[nL - 1].type == MDHIP_DETECT_DDFL) {
            reach.assign(nL, 0);
            reach[nL - 1] = 1;
            for (int i = nL - 1; i >= 0; --i) {
                const mdhip_layer& L = model->layers[i];
                if (L.n_from < 0 || L.n_from > 4) { error = "n_from outside [0, 4]"; return false; }
                for (int j = 0; j < L.n_from && reach[i]; ++j)
                    if (L.from[j] >= 0 && L.from[j] < i) reach[L.from[j]] = 1;
            }
        }

        // pass 1: channels / divisors / concat targets
        for (int i = 0; i < nL; ++i) {
            const mdhip_layer& L = model->layers[i];
            if (L.n_from < 0 || L.n_from > 4) { error = "n_from outside [0, 4]"; return false; }
            for (int j = 0; j < L.n_from; ++j)
                if (L.from[j] >= i || L.from[j] < -1) { error = "layer 'from' index out of order"; return false; }
            const int f0 = L.n_from > 0 ? L.from[0] : -1;
            const int in_div = f0 < 0 ? 1 : layer_div[f0];
            switch (L.type) {
                case MDHIP_CONV:
                    layer_c[i] = L.c_out;
                    layer_div[i] = in_div * L.s;
                    break;
                case MDHIP_C3:
                case MDHIP_SPPF:
                case MDHIP_C3K2:
                case MDHIP_C2PSA:
                case MDHIP_ELAN4:
                case MDHIP_CBLINEAR:
                    layer_c[i] = L.c_out;
                    layer_div[i] = in_div;
                    break;
                case MDHIP_ADOWN:
                    if (f0 < 0) { error = "ADown cannot read the network input"; return false; }
                    layer_c[i] = L.c_out;
                    layer_div[i] = in_div * 2;
                    break;
                case MDHIP_CBFUSE: {
                    if (L.n_from < 2) { error = "CBFuse needs a CBLinear input and a target"; return false; }
                    const int last = L.from[L.n_from - 1];
                    if (last < 0) { error = "CBFuse target cannot be the network input"; return false; }
                    layer_c[i] = layer_c[last];
                    layer_div[i] = layer_div[last];
                    break;
                }
                case MDHIP_SILENCE:
                    if (L.n_from != 1) { error = "Silence has one input"; return false; }
                    layer_c[i] = f0 < 0 ? 3 : layer_c[f0];
                    layer_div[i] = in_div;
                    break;
                case MDHIP_UPSAMPLE:
                    if (f0 < 0 || in_div % 2) { error = "bad upsample input"; return false; }
                    layer_c[i] = layer_c[f0];
                    layer_div[i] = in_div / 2;
                    break;
                case MDHIP_CONCAT: {
                    int c = 0;
                    for (int j = 0; j < L.n_from; ++j) {
                        const int f = L.from[j];
                        if (f < 0 || layer_div[f] != in_div) { error = "concat inputs differ in size"; return false; }
                        if (model->layers[f].type == MDHIP_SILENCE) { error = "a Silence output cannot be concatenated"; return false; }
                        if (concat_target[f] < 0 && reach[i]) { concat_target[f] = i; concat_choff[f] = c; }
                        c += layer_c[f];
                    }
                    layer_c[i] = c;
                    layer_div[i] = in_div;
                    break;
                }
                case MDHIP_DETECT:
                case MDHIP_DETECT_DFL:
                case MDHIP_DETECT_DDFL:
                    break;
                default:
                    error = "unknown layer type";
                    return false;
            }
            if (L.type != MDHIP_DETECT && L.type != MDHIP_DETECT_DFL && L.type != MDHIP_DETECT_DDFL && L.type != MDHIP_CONCAT &&
                L.type != MDHIP_SILENCE && (layer_c[i] % 8)) {
                error = "channel counts must be multiples of 8";
                return false;
            }
        }

        // network input (space-to-depth, 16 channels)
        ctx->input = alloc(16, 2);
        ctx->input_orig = alloc(16, 2);

        auto out_view = [&](int i) -> Tensor {
            const int tgt = concat_target[i];
            if (tgt >= 0) {
                if (!concat_buf[tgt].valid) concat_buf[tgt] = alloc(layer_c[tgt], layer_div[tgt]);
                return slice(concat_buf[tgt], concat_choff[i], layer_c[i]);
            }
            return alloc(layer_c[i], layer_div[i]);
        };

        // pass 2: ops
        // the network input, directly or through Silence layers
        auto reads_input = [&](int f) {
            while (f >= 0 && model->layers[f].type == MDHIP_SILENCE) f = model->layers[f].n_from > 0 ? model->layers[f].from[0] : -1;
            return f < 0;
        };
        for (int i = 0; i < nL; ++i) {
            const mdhip_layer& L = model->layers[i];
            const int f0 = L.n_from > 0 ? L.from[0] : -1;
            if (!reach[i]) continue;
            const bool from_input = L.type != MDHIP_CBFUSE && reads_input(f0);
            if (from_input && L.type != MDHIP_CONV && L.type != MDHIP_SILENCE) {
                error = "layer " + std::to_string(i) + ": only a stem conv (or Silence) may read the network input";
                return false;
            }
            if (L.type == MDHIP_SILENCE) {
                if (!from_input) ctx->layer_out[i] = ctx->layer_out[f0];   // (the network input has no layer view)
                continue;
            }
            if (L.type != MDHIP_DETECT && L.type != MDHIP_CONCAT && L.type != MDHIP_UPSAMPLE && L.type != MDHIP_CBFUSE &&
                (L.first_conv < 0 || L.first_conv >= model->n_convs)) { error = "first_conv out of range"; return false; }
            // convs a layer of this kind consumes (the C3 / SPPF / Detect rows are checked where they are read)
            auto need_convs = [&](int k) {
                if (L.first_conv + k > model->n_convs) { error = "layer " + std::to_string(i) + ": conv table too short"; return false; }
                return true;
            };
            switch (L.type) {
                case MDHIP_CONV: {
                    const mdhip_conv* c = &model->convs[L.first_conv];
                    Tensor out = out_view(i);
                    if (from_input) {
                        const bool stem6x6 = c->c_in == 3 && c->kh == 6 && c->kw == 6 && L.s == 2 && L.p == 2;
                        const bool stem3x3 = c->c_in == 3 && c->kh == 3 && c->kw == 3 && L.s == 2 && L.p == 1;
                        if (!stem6x6 && !stem3x3) {
                            error = "stem must be Conv(3->c, k=6, s=2, p=2) or Conv(3->c, k=3, s=2, p=1)";
                            return false;
                        }
                        if (stem3x3) {
                            stem6_w.assign((size_t)c->c_out * 3 * 36, 0.f);
                            for (int o = 0; o < c->c_out; ++o)
                                for (int ci = 0; ci < 3; ++ci)
                                    for (int r = 0; r < 3; ++r)
                                        for (int q = 0; q < 3; ++q)
                                            stem6_w[(((size_t)o * 3 + ci) * 6 + r + 1) * 6 + q + 1] = c->weight[(((size_t)o * 3 + ci) * 3 + r) * 3 + q];
                            stem6 = *c;
                            stem6.weight = stem6_w.data();
                            stem6.kh = stem6.kw = 6;
                        }
                        const Op& op = conv(i, {{stem3x3 ? &stem6 : c}, true}, ctx->input, out, 1, 1, true, nullptr,
                                            "L%d stem %s (3x3 s2d)", i, stem3x3 ? "3x3s2" : "6x6s2");
                        if (stem3x3) ctx->packed[op.pc].k_real = 27;
                    } else {
                        if (c->c_in != layer_c[f0] || c->kh != L.k || c->kw != L.k) { error = "conv shape mismatch"; return false; }
                        if (L.k != 1 && L.k != 3) { error = "only 1x1 and 3x3 convs supported"; return false; }
                        conv(i, {{c}}, ctx->layer_out[f0], out, L.s, L.p, true, nullptr, "L%d conv %dx%ds%d", i, L.k, L.k, L.s);
                    }
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_C3: {
                    const mdhip_conv* cv = &model->convs[L.first_conv];
                    const int ch = cv[0].c_out;          // hidden width c_
                    if (ch % 8 || cv[1].c_out != ch || cv[0].c_in != layer_c[f0]) { error = "C3 shape mismatch"; return false; }
                    Tensor out = out_view(i);
                    Tensor Y = alloc(2 * ch, layer_div[i]);
                    // (a line-aligned pixel pitch for the hidden tensor -- 160 -> 192, 480 -> 512 channels -- was
                    // measured: no gain, 36.0 vs 35.9 ms per forward)
                    Tensor T = alloc(ch, layer_div[i]);
                    Tensor Y1 = slice(Y, 0, ch);
                    conv(i, {{&cv[0], &cv[1]}}, ctx->layer_out[f0], Y, 1, 0, true, nullptr, "L%d C3.cv1|cv2 1x1", i);
                    for (int j = 0; j < L.n; ++j) {
                        const mdhip_conv* b1 = &cv[3 + 2 * j];
                        const mdhip_conv* b2 = &cv[4 + 2 * j];
                        if (b1->kh != 1 || b2->kh != 3) { error = "bottleneck must be 1x1 then 3x3"; return false; }
                        conv(i, {{b1}}, Y1, T, 1, 0, true, nullptr, "L%d C3.m%d.cv1 1x1", i, j);
                        conv(i, {{b2}}, T, Y1, 1, 1, true, L.shortcut ? &Y1 : nullptr, "L%d C3.m%d.cv2 3x3", i, j);
                        // candidates for the fused bottleneck kernel (decided per forward from the 3x3s' tiles): an
                        // even number of bottlenecks, so that ping-ponging Y1 <-> T ends in Y1.  The 80-channel block
                        // (the shape conv_v5c.cpp takes) stays in 16 bits in the fp8 mode too: fused it is faster than
                        // its 1x1 -> e4m3 -> 3x3 pair (4.0 against 4.4 ms per 32 images) and exact.
                        const bool strip_block = ch == 80 && (L.n % 2) == 0;
                        if ((L.n % 2) == 0 && (ctx->dtype != MDHIP_DTYPE_FP8 || strip_block)) {
                            const int o2 = (int)ctx->ops.size() - 1, o1 = o2 - 1;
                            if (j == 0) ctx->fuse_groups.emplace_back();
                            ctx->ops[o1].fuse_group = ctx->ops[o2].fuse_group = (int)ctx->fuse_groups.size() - 1;
                            ctx->ops[o1].fuse_idx = ctx->ops[o2].fuse_idx = j;
                            ctx->ops[o1].fuse_role = 1;
                            ctx->ops[o2].fuse_role = 2;
                            ctx->fuse_groups.back().push_back(o2);
                        }
                        if (ctx->packed[ctx->ops.back().pc].groups8 > 0 && !strip_block) {
                            // fp8 mode: the hidden tensor T of this bottleneck travels as e4m3 (1x1 writes, 3x3 reads)
                            const int o2 = (int)ctx->ops.size() - 1, o1 = o2 - 1;
                            ctx->ops[o1].f8_out = true;
                            ctx->ops[o1].f8_peer = o2;
                            ctx->ops[o2].f8_in = true;
                            ctx->ops[o2].f8_peer = o1;
                            ++ctx->n_f8;
                        }
                    }
                    conv(i, {{&cv[2]}}, Y, out, 1, 0, true, nullptr, "L%d C3.cv3 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_C3K2: {
                    // cv1, cv2, then per inner block j: Bottleneck  m.j.cv1, m.j.cv2 (3x3, 3x3)            (k == 0)
                    //                                   C3k         m.j.cv1, m.j.cv2, m.j.cv3, m.j.m.0.cv1, m.j.m.0.cv2,
                    //                                               m.j.m.1.cv1, m.j.m.1.cv2 (C3 with 3x3 -> 3x3 bottlenecks)
                    const int per = L.k ? 7 : 2;
                    if (!need_convs(2 + per * L.n)) return false;
                    const mdhip_conv* cv = &model->convs[L.first_conv];
                    const int c = cv[0].c_out / 2;
                    if (L.n < 1 || c % 8 || !conv_is(cv[0], layer_c[f0], 2 * c, 1) || !conv_is(cv[1], (2 + L.n) * c, L.c_out, 1)) {
                        error = "C3k2 shape mismatch at layer " + std::to_string(i);
                        return false;
                    }
                    Tensor out = out_view(i);
                    Tensor Y = alloc((2 + L.n) * c, layer_div[i]);
                    conv(i, {{&cv[0]}}, ctx->layer_out[f0], slice(Y, 0, 2 * c), 1, 0, true, nullptr, "L%d C3k2.cv1 1x1", i);
                    for (int j = 0; j < L.n; ++j) {
                        const mdhip_conv* b = &cv[2 + per * j];
                        const Tensor src = slice(Y, (1 + j) * c, c), dst = slice(Y, (2 + j) * c, c);
                        if (!L.k) {
                            const int h = b[0].c_out;
                            if (!conv_is(b[0], c, h, 3) || !conv_is(b[1], h, c, 3)) { error = "C3k2 bottleneck shape mismatch"; return false; }
                            Tensor T = alloc(h, layer_div[i]);
                            conv(i, {{&b[0]}}, src, T, 1, 1, true, nullptr, "L%d C3k2.m%d.cv1 3x3", i, j);
                            conv(i, {{&b[1]}}, T, dst, 1, 1, true, L.shortcut ? &src : nullptr, "L%d C3k2.m%d.cv2 3x3", i, j);
                        } else {
                            const int h = b[0].c_out;
                            if (h % 8 || !conv_is(b[0], c, h, 1) || !conv_is(b[1], c, h, 1) || !conv_is(b[2], 2 * h, c, 1)) {
                                error = "C3k shape mismatch";
                                return false;
                            }
                            for (int q = 3; q < 7; ++q)
                                if (!conv_is(b[q], h, h, 3)) { error = "C3k bottleneck must be 3x3 -> 3x3"; return false; }
                            Tensor YK = alloc(2 * h, layer_div[i]);
                            Tensor TK = alloc(h, layer_div[i]);
                            char tag[16];
                            snprintf(tag, sizeof(tag), "m%d", j);
                            if (!repncsp(i, "C3k2", tag, b, 2, L.shortcut != 0, src, dst, YK, TK)) return false;
                        }
                    }
                    conv(i, {{&cv[1]}}, Y, out, 1, 0, true, nullptr, "L%d C3k2.cv2 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_C2PSA: {
                    // cv1, cv2, then per PSA block j: m.j.attn.qkv, m.j.attn.proj, m.j.attn.pe, m.j.ffn.0, m.j.ffn.1
                    if (!need_convs(2 + 5 * L.n)) return false;
                    const mdhip_conv* cv = &model->convs[L.first_conv];
                    const int c = cv[0].c_out / 2;
                    const int heads = c / 64;
                    if (L.n < 1 || c % 64 || !conv_is(cv[0], layer_c[f0], 2 * c, 1) || !conv_is(cv[1], 2 * c, L.c_out, 1)) {
                        error = "C2PSA shape mismatch at layer " + std::to_string(i) + " (the attention needs c1 / 2 a multiple of 64)";
                        return false;
                    }
                    Tensor out = out_view(i);
                    Tensor Y = alloc(2 * c, layer_div[i]);
                    const Tensor B = slice(Y, c, c);
                    Tensor QKV = alloc(heads * 128, layer_div[i]);
                    Tensor A = alloc(c, layer_div[i]);
                    Tensor Fh = alloc(2 * c, layer_div[i]);
                    conv(i, {{&cv[0]}}, ctx->layer_out[f0], Y, 1, 0, true, nullptr, "L%d C2PSA.cv1 1x1", i);
                    for (int j = 0; j < L.n; ++j) {
                        const mdhip_conv* b = &cv[2 + 5 * j];
                        // Attention(dim = c, heads = c / 64, attn_ratio 0.5): key_dim 32, head_dim 64, qkv = c + 2 * heads * 32
                        if (!conv_is(b[0], c, heads * 128, 1) || !conv_is(b[1], c, c, 1) || !(b[2].c_in == 1 && b[2].c_out == c &&
                            b[2].kh == 3 && b[2].kw == 3) || !conv_is(b[3], c, 2 * c, 1) || !conv_is(b[4], 2 * c, c, 1)) {
                            error = "PSABlock shape mismatch at layer " + std::to_string(i) + " (key_dim 32, head_dim 64 expected)";
                            return false;
                        }
                        conv(i, {{&b[0]}}, B, QKV, 1, 0, false, nullptr, "L%d C2PSA.m%d.attn.qkv 1x1", i, j);
                        add_op(OP_ATTN, i, QKV, A, "L%d C2PSA.m%d.attn", i, j).heads = heads;
                        dw(i, &b[2], QKV, A, false, &A, 64, 128, 64, "L%d C2PSA.m%d.attn.pe dw3x3 (+=)", i, j);
                        conv(i, {{&b[1]}}, A, B, 1, 0, false, &B, "L%d C2PSA.m%d.attn.proj 1x1", i, j);
                        conv(i, {{&b[3]}}, B, Fh, 1, 0, true, nullptr, "L%d C2PSA.m%d.ffn.0 1x1", i, j);
                        conv(i, {{&b[4]}}, Fh, B, 1, 0, false, &B, "L%d C2PSA.m%d.ffn.1 1x1", i, j);
                    }
                    conv(i, {{&cv[1]}}, Y, out, 1, 0, true, nullptr, "L%d C2PSA.cv2 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_DETECT_DFL: {
                    // per level l: cv2.l.0 (3x3), cv2.l.1 (3x3), cv2.l.2 (1x1, 64 box logits), cv3.l.0.0 (dw 3x3), cv3.l.0.1 (1x1),
                    // cv3.l.1.0 (dw 3x3), cv3.l.1.1 (1x1), cv3.l.2 (1x1, nc class logits)
                    if (L.n_from != model->nl) { error = "Detect inputs != nl"; return false; }
                    if (!need_convs(8 * L.n_from)) return false;
                    for (int l = 0; l < L.n_from; ++l) {
                        const mdhip_conv* b = &model->convs[L.first_conv + 8 * l];
                        const int f = L.from[l];
                        const int cx = layer_c[f], c2 = b[0].c_out, c3 = b[4].c_out;
                        if (!conv_is(b[0], cx, c2, 3) || !conv_is(b[1], c2, c2, 3) || !(b[2].c_in == c2 && b[2].c_out == 64 && b[2].kh == 1) ||
                            !(b[3].c_in == 1 && b[3].c_out == cx && b[3].kh == 3 && b[3].kw == 3) || !conv_is(b[4], cx, c3, 1) ||
                            !(b[5].c_in == 1 && b[5].c_out == c3 && b[5].kh == 3 && b[5].kw == 3) || !conv_is(b[6], c3, c3, 1) ||
                            !(b[7].c_in == c3 && b[7].c_out == ctx->nc && b[7].kh == 1)) {
                            error = "anchor-free Detect level " + std::to_string(l) + ": conv shapes do not match (reg_max 16, "
                                    "class branch DWConv 3x3 -> Conv 1x1 -> DWConv 3x3 -> Conv 1x1 -> Conv2d 1x1)";
                            return false;
                        }
                        if (std::fabs(ctx->strides[l] - (float)layer_div[f]) > 1e-6f) { error = "Detect stride does not match the graph"; return false; }
                        const Tensor& x = ctx->layer_out[f];
                        const int dv = layer_div[f];
                        Tensor B1 = alloc(c2, dv), B2 = alloc(c2, dv);
                        Tensor C1 = alloc(cx, dv), C2 = alloc(c3, dv), C3 = alloc(c3, dv), C4 = alloc(c3, dv);
                        conv(i, {{&b[0]}}, x, B1, 1, 1, true, nullptr, "L%d Detect.cv2.%d.0 3x3", i, l);
                        conv(i, {{&b[1]}}, B1, B2, 1, 1, true, nullptr, "L%d Detect.cv2.%d.1 3x3", i, l);
                        const int box = (int)ctx->ops.size();
                        conv(i, {{&b[2]}}, B2, f32_out, 1, 0, false, nullptr, "L%d Detect.cv2.%d.2 1x1 (box)", i, l);
                        dw(i, &b[3], x, C1, true, nullptr, cx, cx, 0, "L%d Detect.cv3.%d.0.0 dw3x3", i, l);
                        conv(i, {{&b[4]}}, C1, C2, 1, 0, true, nullptr, "L%d Detect.cv3.%d.0.1 1x1", i, l);
                        dw(i, &b[5], C2, C3, true, nullptr, c3, c3, 0, "L%d Detect.cv3.%d.1.0 dw3x3", i, l);
                        conv(i, {{&b[6]}}, C3, C4, 1, 0, true, nullptr, "L%d Detect.cv3.%d.1.1 1x1", i, l);
                        dfl_tail(i, l, "Detect", box, &b[7], C4, x);
                    }
                    break;
                }
                case MDHIP_ELAN4: {
                    // cv1, RepNCSP cv2.0 (3 + 2n), cv2.1, RepNCSP cv3.0 (3 + 2n), cv3.1, cv4: one buffer [cv1 | cv2 | cv3]
                    const int rn = L.n;
                    if (rn < 1 || !need_convs(10 + 4 * rn)) { if (error.empty()) error = "RepNCSPELAN4 needs n >= 1"; return false; }
                    const mdhip_conv* cv = &model->convs[L.first_conv];
                    const mdhip_conv* ra = cv + 1;
                    const mdhip_conv* ca = cv + 4 + 2 * rn;
                    const mdhip_conv* rb = cv + 5 + 2 * rn;
                    const mdhip_conv* cb = cv + 8 + 4 * rn;
                    const mdhip_conv* c4v = cv + 9 + 4 * rn;
                    const int c3 = cv[0].c_out, c4 = ca->c_out;
                    if (c3 % 16 || c4 % 16 || !conv_is(cv[0], layer_c[f0], c3, 1) || !conv_is(*ca, c4, c4, 3) || !conv_is(*cb, c4, c4, 3) ||
                        !conv_is(*c4v, c3 + 2 * c4, L.c_out, 1)) {
                        error = "RepNCSPELAN4 shape mismatch at layer " + std::to_string(i);
                        return false;
                    }
                    Tensor out = out_view(i);
                    Tensor Y = alloc(c3 + 2 * c4, layer_div[i]);
                    Tensor T = alloc(c4, layer_div[i]);
                    Tensor YK = alloc(c4, layer_div[i]), TK = alloc(c4 / 2, layer_div[i]);
                    conv(i, {{&cv[0]}}, ctx->layer_out[f0], slice(Y, 0, c3), 1, 0, true, nullptr, "L%d ELAN.cv1 1x1", i);
                    if (!repncsp(i, "ELAN", "cv2.0", ra, rn, true, slice(Y, c3 / 2, c3 / 2), T, YK, TK)) return false;
                    conv(i, {{ca}}, T, slice(Y, c3, c4), 1, 1, true, nullptr, "L%d ELAN.cv2.1 3x3", i);
                    if (!repncsp(i, "ELAN", "cv3.0", rb, rn, true, slice(Y, c3, c4), T, YK, TK)) return false;
                    conv(i, {{cb}}, T, slice(Y, c3 + c4, c4), 1, 1, true, nullptr, "L%d ELAN.cv3.1 3x3", i);
                    conv(i, {{c4v}}, Y, out, 1, 0, true, nullptr, "L%d ELAN.cv4 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_ADOWN: {
                    // cv1 (3x3 / s2 / p1 over the averaged first half), cv2 (1x1 over the max-pooled second half)
                    if (!need_convs(2)) return false;
                    const mdhip_conv* cv = &model->convs[L.first_conv];
                    const int c1 = layer_c[f0], c = cv[0].c_out;
                    if (c1 % 16 || !conv_is(cv[0], c1 / 2, c, 3) || !conv_is(cv[1], c1 / 2, c, 1) || L.c_out != 2 * c) {
                        error = "ADown shape mismatch at layer " + std::to_string(i);
                        return false;
                    }
                    Tensor out = out_view(i);
                    Tensor A = alloc(c1 / 2, layer_div[f0]);
                    Tensor B = alloc(c1 / 2, layer_div[i]);
                    add_op(OP_ADOWN, i, ctx->layer_out[f0], A, "L%d ADown.pool avg2|max3s2", i).out2 = B;
                    conv(i, {{&cv[0]}}, A, slice(out, 0, c), 2, 1, true, nullptr, "L%d ADown.cv1 3x3s2", i);
                    conv(i, {{&cv[1]}}, B, slice(out, c, c), 1, 0, true, nullptr, "L%d ADown.cv2 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_CBLINEAR: {
                    if (!need_convs(1)) return false;
                    const mdhip_conv* c = &model->convs[L.first_conv];
                    if (!conv_is(*c, layer_c[f0], L.c_out, 1)) { error = "CBLinear shape mismatch at layer " + std::to_string(i); return false; }
                    Tensor out = out_view(i);
                    conv(i, {{c}}, ctx->layer_out[f0], out, 1, 0, false, nullptr, "L%d CBLinear 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_CBFUSE: {
                    const int nsrc = L.n_from - 1;
                    const int last = L.from[nsrc];
                    const int C = layer_c[last];
                    const int offs[3] = {L.k, L.s, L.p};
                    if (nsrc < 1 || nsrc > 3) { error = "CBFuse takes 1 to 3 CBLinear inputs"; return false; }
                    Tensor out = out_view(i);
                    Op& op = add_op(OP_CBFUSE, i, ctx->layer_out[last], out, "L%d CBFuse x%d", i, nsrc);
                    op.n_fsrc = nsrc;
                    for (int j = 0; j < nsrc; ++j) {
                        const int f = L.from[j];
                        const int ratio = f >= 0 ? layer_div[f] / layer_div[last] : 0;
                        if (f < 0 || model->layers[f].type != MDHIP_CBLINEAR || offs[j] < 0 || offs[j] % 8 || offs[j] + C > layer_c[f] ||
                            layer_div[f] % layer_div[last] || (ratio != 1 && ratio != 2 && ratio != 4)) {
                            error = "CBFuse input " + std::to_string(j) + " at layer " + std::to_string(i) +
                                    " must be a CBLinear split (channel offset a multiple of 8) at 1x, 1/2 or 1/4 the size";
                            return false;
                        }
                        op.fsrc[j] = slice(ctx->layer_out[f], offs[j], C);
                        op.ffac[j] = ratio;
                    }
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_DETECT_DDFL: {
                    // n heads of 6 nl convs each; head k runs: per level cv2.l.0 (3x3), cv2.l.1 (3x3, g = 4), cv2.l.2 (1x1, 64 box
                    // logits), cv3.l.0 (3x3), cv3.l.1 (3x3), cv3.l.2 (1x1, nc class logits)
                    const int nh = L.n, hsel = L.k, nl = model->nl;
                    if (nh < 1 || nh > 2 || hsel < 0 || hsel >= nh) { error = "DDetect: n (heads) must be 1 or 2 and k < n"; return false; }
                    if (L.n_from != nl) { error = "Detect inputs != nl"; return false; }
                    if (!need_convs(6 * nl * nh)) return false;
                    for (int l = 0; l < nl; ++l) {
                        const mdhip_conv* b = &model->convs[L.first_conv + (hsel * nl + l) * 6];
                        const int f = L.from[l];
                        const int cx = layer_c[f], c2 = b[0].c_out, c3 = b[3].c_out;
                        const bool grouped = b[1].c_in * 4 == c2 && b[1].c_out == c2 && b[1].kh == 3 && b[1].kw == 3 && b[1].weight;
                        if (!conv_is(b[0], cx, c2, 3) || c2 % 32 || !(grouped || conv_is(b[1], c2, c2, 3)) ||
                            !(b[2].c_in == c2 && b[2].c_out == 64 && b[2].kh == 1 && b[2].kw == 1) || !conv_is(b[3], cx, c3, 3) ||
                            !conv_is(b[4], c3, c3, 3) || !(b[5].c_in == c3 && b[5].c_out == ctx->nc && b[5].kh == 1 && b[5].kw == 1)) {
                            error = "DDetect level " + std::to_string(l) + ": conv shapes do not match (reg_max 16; box branch Conv 3x3 "
                                    "-> Conv 3x3 (g = 4) -> Conv2d 1x1, class branch Conv 3x3 -> Conv 3x3 -> Conv2d 1x1)";
                            return false;
                        }
                        if (std::fabs(ctx->strides[l] - (float)layer_div[f]) > 1e-6f) { error = "Detect stride does not match the graph"; return false; }
                        // the grouped conv as a dense one: output channel o reads the c2 / 4 inputs of its group, every other
                        // weight is an exact zero
                        std::vector<float> dense;
                        mdhip_conv b1 = b[1];
                        if (grouped) {
                            const int gi = c2 / 4;
                            dense.assign((size_t)c2 * c2 * 9, 0.f);
                            for (int o = 0; o < c2; ++o)
                                for (int ci = 0; ci < gi; ++ci)
                                    for (int t = 0; t < 9; ++t)
                                        dense[((size_t)o * c2 + (o / gi) * gi + ci) * 9 + t] = b[1].weight[((size_t)o * gi + ci) * 9 + t];
                            b1.weight = dense.data();
                            b1.c_in = c2;
                        }
                        const Tensor& x = ctx->layer_out[f];
                        const int dv = layer_div[f];
                        Tensor B1 = alloc(c2, dv), B2 = alloc(c2, dv), C1 = alloc(c3, dv), C2 = alloc(c3, dv);
                        conv(i, {{&b[0]}}, x, B1, 1, 1, true, nullptr, "L%d DDetect.cv2.%d.0 3x3", i, l);
                        conv(i, {{&b1}}, B1, B2, 1, 1, true, nullptr, "L%d DDetect.cv2.%d.1 3x3 g4", i, l);
                        const int box = (int)ctx->ops.size();
                        conv(i, {{&b[2]}}, B2, f32_out, 1, 0, false, nullptr, "L%d DDetect.cv2.%d.2 1x1 (box)", i, l);
                        conv(i, {{&b[3]}}, x, C1, 1, 1, true, nullptr, "L%d DDetect.cv3.%d.0 3x3", i, l);
                        conv(i, {{&b[4]}}, C1, C2, 1, 1, true, nullptr, "L%d DDetect.cv3.%d.1 3x3", i, l);
                        dfl_tail(i, l, "DDetect", box, &b[5], C2, x);
                    }
                    break;
                }
                case MDHIP_SPPF: {
                    const mdhip_conv* cv = &model->convs[L.first_conv];
                    const int ch = cv[0].c_out;
                    if (ch % 8) { error = "SPPF hidden width must be a multiple of 8"; return false; }
                    Tensor out = out_view(i);
                    Tensor Y = alloc(4 * ch, layer_div[i]);
                    conv(i, {{&cv[0]}}, ctx->layer_out[f0], slice(Y, 0, ch), 1, 0, true, nullptr, "L%d SPPF.cv1 1x1", i);
                    add_op(OP_POOL, i, slice(Y, 0, ch), Y, "L%d SPPF.pool x3 k%d", i, L.k).pool_k = L.k;
                    conv(i, {{&cv[1]}}, Y, out, 1, 0, true, nullptr, "L%d SPPF.cv2 1x1", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_UPSAMPLE: {
                    Tensor out = out_view(i);
                    add_op(OP_UPSAMPLE, i, ctx->layer_out[f0], out, "L%d upsample x2", i);
                    ctx->layer_out[i] = out;
                    break;
                }
                case MDHIP_CONCAT: {
                    if (!concat_buf[i].valid) concat_buf[i] = alloc(layer_c[i], layer_div[i]);
                    // a concat feeding another concat keeps its own buffer and is copied below
                    int c = 0;
                    for (int j = 0; j < L.n_from; ++j) {
                        const int f = L.from[j];
                        if (!(concat_target[f] == i && concat_choff[f] == c)) {
                            add_op(OP_COPY, i, ctx->layer_out[f], slice(concat_buf[i], c, layer_c[f]), "L%d concat copy of L%d", i, f);
                        }
                        c += layer_c[f];
                    }
                    ctx->layer_out[i] = concat_buf[i];
                    if (concat_target[i] >= 0) {
                        // nested concat: copy into the outer buffer
                        Tensor outer = out_view(i);
                        add_op(OP_COPY, i, concat_buf[i], outer, "L%d nested concat copy", i);
                    }
                    break;
                }
                case MDHIP_DETECT: {
                    if (L.n_from != model->nl) { error = "Detect inputs != nl"; return false; }
                    for (int l = 0; l < L.n_from; ++l) {
                        const mdhip_conv* c = &model->convs[L.first_conv + l];
                        const int f = L.from[l];
                        if (c->c_out != ctx->na * ctx->no || c->c_in != layer_c[f] || c->kh != 1) { error = "Detect conv shape mismatch"; return false; }
                        if (std::fabs(ctx->strides[l] - (float)layer_div[f]) > 1e-6f) { error = "Detect stride does not match the graph"; return false; }
                        const int cv = (int)ctx->ops.size();
                        conv(i, {{c}}, ctx->layer_out[f], f32_out, 1, 0, false, nullptr, "L%d Detect.m%d 1x1", i, l);
                        Op& dec = add_op(OP_DECODE, i, ctx->layer_out[f], Tensor(), "L%d Detect.decode%d", i, l);
                        dec.level = l;
                        dec.f32_off = ctx->ops[cv].f32_off;
                        dec.f32_ld = ctx->ops[cv].f32_ld;
                    }
                    break;
                }
            }
        }
        // an upsample whose output is the first part of a concatenated tensor that exactly one op reads, a 1x1 / stride 1
        // conv: that conv can read the low-resolution tensor in place (conv_v2.cpp) and the upsample need not run
        for (size_t u = 0; u < ctx->ops.size(); ++u) {
            Op& up = ctx->ops[u];
            if (up.kind != OP_UPSAMPLE) continue;
            int reader = -1, readers = 0;
            for (size_t k = 0; k < ctx->ops.size(); ++k) {
                const Op& o = ctx->ops[k];
                if (o.kind == OP_DECODE) continue;
                const bool overlaps = o.in.off == up.out.off || (o.has_res && o.res.off == up.out.off);
                if (k != u && overlaps) { ++readers; reader = (int)k; }
            }
            if (readers != 1) continue;
            Op& c = ctx->ops[reader];
            const PackedConv& pc = ctx->packed[c.pc >= 0 ? c.pc : 0];
            if (c.kind == OP_CONV && reader > (int)u && c.stride == 1 && pc.kh == 1 && pc.kw == 1 && !c.f8_in &&
                c.in.off == up.out.off && c.in.ld == up.out.ld && c.in.c > up.out.c && c.in.div == up.out.div) {
                up.up_peer = reader;
                c.up_peer = (int)u;
            }
        }
        return true;
    }
};

}  // namespace

int mdhip::num_anchors_for(const mdhip_ctx* ctx, int h, int w) {
    int a = 0;
    for (int l = 0; l < ctx->nl; ++l) {
        const int s = (int)ctx->strides[l];
        a += ctx->na * (h / s) * (w / s);
    }
    return a;
}

int mdhip::plan_context(mdhip_ctx* ctx, const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w, PlannedWeights* pw,
                        std::string* err) {
    ctx->dtype = dtype;
    ctx->max_batch = max_batch;
    ctx->nc = model->nc;
    ctx->na = model->na;
    ctx->nl = model->nl;
    ctx->no = model->nc + 5;
    bool has_detect = false;
    for (int i = 0; i < model->n_layers; ++i) {
        const int t = model->layers[i].type;
        has_detect |= t == MDHIP_DETECT || t == MDHIP_DETECT_DFL || t == MDHIP_DETECT_DDFL;
        ctx->anchor_free |= t == MDHIP_DETECT_DFL || t == MDHIP_DETECT_DDFL;
    }
    if (ctx->anchor_free) {
        // [cx, cy, w, h, cls0 .. cls(nc-1)]: no objectness, one prediction per cell
        ctx->no = model->nc + 4;
        ctx->na = 1;
        if (dtype == MDHIP_DTYPE_FP8) {
            *err = "MDHIP_DTYPE_FP8 is implemented for the YOLOv5 bottlenecks only, not for anchor-free (YOLO11, YOLOv9) models: "
                   "use bf16 or fp16";
            return MDHIP_EUNSUPPORTED;
        }
    }
    ctx->max_stride = 2;
    if (has_detect) {
        if (model->nl < 1 || !model->strides || (!ctx->anchor_free && !model->anchors_px) || model->nc < 1 || model->nc > 250) {
            *err = "Detect layer needs nl/strides/anchors/nc";
            return MDHIP_EINVAL;
        }
        ctx->strides.assign(model->strides, model->strides + model->nl);
        for (float s : ctx->strides) ctx->max_stride = std::max(ctx->max_stride, (int)s);
    }
    {   // largest stride of any layer (models without Detect, used by unit tests)
        std::vector<int> div(model->n_layers, 1);
        for (int i = 0; i < model->n_layers; ++i) {
            const mdhip_layer& L = model->layers[i];
            const int nf = std::min(std::max(L.n_from, 0), 4);
            const int f0 = nf > 0 ? L.from[L.type == MDHIP_CBFUSE ? nf - 1 : 0] : -1;
            const int d = (f0 < 0 || f0 >= i) ? 1 : div[f0];
            div[i] = L.type == MDHIP_CONV ? d * std::max(1, L.s) : (L.type == MDHIP_UPSAMPLE ? std::max(1, d / 2) :
                                                                     L.type == MDHIP_ADOWN ? d * 2 : d);
            ctx->max_stride = std::max(ctx->max_stride, div[i]);
        }
    }
    ctx->max_h = round_up(max_h, ctx->max_stride);
    ctx->max_w = round_up(max_w, ctx->max_stride);
    ctx->layers.assign(model->layers, model->layers + model->n_layers);
    Planner P;
    P.ctx = ctx;
    P.model = model;
    P.blobs = &pw->convs;
    if (!P.plan()) {
        *err = "model planning failed: " + P.error;
        return MDHIP_EINVAL;
    }
    // predictions, NMS scratch, letterbox geometry
    ctx->a_max = has_detect ? num_anchors_for(ctx, ctx->max_h, ctx->max_w) : 1;
    // room for the concatenated predictions of test-time augmentation (three passes, <= 3 x a_max)
    ctx->a_cap = has_detect ? 3 * ctx->a_max : 1;
    ctx->pred_offs[0] = P.alloc_bytes((size_t)max_batch * ctx->a_cap * ctx->no * 4);
    ctx->pred_offs[1] = P.alloc_bytes((size_t)max_batch * ctx->a_cap * ctx->no * 4);
    ctx->pred_off = ctx->pred_offs[0];
    for (int i = 0; i < 6; ++i) ctx->nms_kv_off[i] = P.alloc_bytes((size_t)max_batch * ctx->a_cap * 4);
    ctx->nms_seg_off = P.alloc_bytes((size_t)max_batch * kNmsScanParts * 4);
    ctx->nms_out_off = P.alloc_bytes((size_t)max_batch * kNmsMaxDet * 6 * 4);
    ctx->nms_cnt_off = P.alloc_bytes((size_t)max_batch * 4);
    ctx->geom_off = P.alloc_bytes((size_t)max_batch * sizeof(LetterboxWin));
    {   // fp8 calibration: one range word per e4m3 tensor
        const size_t base = P.alloc_bytes((size_t)std::max(1, ctx->n_f8) * 4);
        size_t k = 0;
        for (Op& op : ctx->ops)
            if (op.f8_out) op.amax_off = base + 4 * k++;
    }
    ctx->arena_bytes = P.cursor + 256;

    // weight arena
    size_t wcur = 0;
    ctx->zero_off = 0;
    wcur = 256;
    ctx->anchors_off = wcur;
    wcur = align_up(wcur + (size_t)std::max(1, ctx->nl * ctx->na * 2) * 4, 256);
    for (size_t i = 0; i < ctx->packed.size(); ++i) {
        PackedConv& pc = ctx->packed[i];
        const std::vector<PackedBlobs::Ref> refs = pw->convs[i].refs();
        for (size_t k = 0; k < refs.size(); ++k) {
            if (k >= 2 && !refs[k].bytes) continue;         // (weights and bias always have a place)
            pc.*refs[k].off = wcur;
            wcur = align_up(wcur + refs[k].bytes, 256);
        }
        if (pc.w8_off) {
            pc.scale_off = wcur;
            wcur = align_up(wcur + (size_t)pc.n_rows * 4, 256);
        }
    }
    ctx->warena_bytes = wcur;
    // mdhip_forward records `input_free` right behind the last op that reads the network input (only stem convs do)
    for (size_t oi = 0; oi < ctx->ops.size(); ++oi) {
        const Op& o = ctx->ops[oi];
        const bool reads = (o.in.valid && o.in.off == ctx->input.off) || (o.has_res && o.res.off == ctx->input.off);
        if (reads && o.kind != OP_CONV) {
            *err = "op " + std::to_string(oi) + " (" + o.name + ") reads the network input: only a stem conv may";
            return MDHIP_EINVAL;
        }
        if (reads) ctx->last_input_op = (int)oi;
    }
    return MDHIP_OK;
}

// ---------------------------------------------------------------------------------------
// the plan as text (mdhip_plan_describe): one line per record, fixed field order; nothing that only a forward sets
// ---------------------------------------------------------------------------------------
namespace {

uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    return h;
}

void put(std::string& s, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
}

void put_tensor(std::string& s, const char* tag, const Tensor& t) {
    put(s, " %s=%zu:%d:%d:%d:%d", tag, t.off, t.ld, t.c, t.div, (int)t.valid);
}

template <class T>
void put_blob(std::string& s, const char* tag, const std::vector<T>& v) {
    put(s, " %s=%zu:%016llx", tag, v.size(), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}

}  // namespace

std::string mdhip::describe_plan(const mdhip_ctx* ctx, const PlannedWeights& pw) {
    std::string s;
    put(s, "plan dtype=%d max_batch=%d max_stride=%d max_h=%d max_w=%d nc=%d na=%d nl=%d no=%d anchor_free=%d a_max=%d a_cap=%d\n",
        ctx->dtype, ctx->max_batch, ctx->max_stride, ctx->max_h, ctx->max_w, ctx->nc, ctx->na, ctx->nl, ctx->no,
        (int)ctx->anchor_free, ctx->a_max, ctx->a_cap);
    s += "arena";
    put_tensor(s, "input", ctx->input);
    put_tensor(s, "input_orig", ctx->input_orig);
    put(s, " pred=%zu,%zu nms_kv=", ctx->pred_offs[0], ctx->pred_offs[1]);
    for (int i = 0; i < 6; ++i) put(s, i ? ",%zu" : "%zu", ctx->nms_kv_off[i]);
    put(s, " nms_seg=%zu nms_out=%zu nms_cnt=%zu geom=%zu arena_bytes=%zu\n", ctx->nms_seg_off, ctx->nms_out_off, ctx->nms_cnt_off,
        ctx->geom_off, ctx->arena_bytes);
    put(s, "warena zero=%zu anchors=%zu warena_bytes=%zu n_f8=%d last_input_op=%d\n", ctx->zero_off, ctx->anchors_off,
        ctx->warena_bytes, ctx->n_f8, ctx->last_input_op);
    put(s, "fuse_groups %zu", ctx->fuse_groups.size());
    for (const auto& g : ctx->fuse_groups) {
        s += " [";
        for (size_t k = 0; k < g.size(); ++k) put(s, k ? ",%d" : "%d", g[k]);
        s += "]";
    }
    s += "\n";
    for (size_t i = 0; i < ctx->layer_out.size(); ++i) {
        put(s, "layer %zu", i);
        put_tensor(s, "out", ctx->layer_out[i]);
        s += "\n";
    }
    for (size_t i = 0; i < ctx->packed.size(); ++i) {
        const PackedConv& p = ctx->packed[i];
        const PackedBlobs& b = pw.convs[i];
        put(s, "packed %zu n_rows=%d k_pad=%d cin_pad=%d kh=%d kw=%d c_out=%d k_real=%d k_pad4=%d groups=%d k_pad4p=%d k_pad8=%d groups8=%d",
            i, p.n_rows, p.k_pad, p.cin_pad, p.kh, p.kw, p.c_out, p.k_real, p.k_pad4, p.groups, p.k_pad4p, p.k_pad8, p.groups8);
        put(s, " w_off=%zu b_off=%zu w4_off=%zu w4p_off=%zu w8_off=%zu scale_off=%zu", p.w_off, p.b_off, p.w4_off, p.w4p_off, p.w8_off,
            p.scale_off);
        put_blob(s, "w", b.w);
        put_blob(s, "b", b.b);
        put_blob(s, "w4", b.w4);
        put_blob(s, "w4p", b.w4p);
        put_blob(s, "w8", b.w8);
        put_blob(s, "wscale", p.wscale);
        s += "\n";
    }
    for (size_t i = 0; i < ctx->ops.size(); ++i) {
        const Op& o = ctx->ops[i];
        put(s, "op %zu kind=%d layer=%d name=\"%s\"", i, o.kind, o.layer, o.name.c_str());
        put_tensor(s, "in", o.in);
        put_tensor(s, "out", o.out);
        put_tensor(s, "res", o.res);
        put_tensor(s, "out2", o.out2);
        for (int k = 0; k < 3; ++k) put_tensor(s, k == 0 ? "fsrc0" : k == 1 ? "fsrc1" : "fsrc2", o.fsrc[k]);
        put(s, " pc=%d stride=%d pad=%d act=%d out_f32=%d pool_k=%d level=%d f32_off=%zu f32_ld=%d cls_off=%zu cls_ld=%d", o.pc, o.stride,
            o.pad, o.act, o.out_f32, o.pool_k, o.level, o.f32_off, o.f32_ld, o.cls_off, o.cls_ld);
        put(s, " dw=%d,%d,%d heads=%d n_fsrc=%d ffac=%d,%d,%d f8_in=%d f8_out=%d f8_peer=%d fuse=%d,%d,%d up_peer=%d has_res=%d amax_off=%zu\n",
            o.dw_grp, o.dw_grp_stride, o.dw_grp_off, o.heads, o.n_fsrc, o.ffac[0], o.ffac[1], o.ffac[2], (int)o.f8_in, (int)o.f8_out,
            o.f8_peer, o.fuse_group, o.fuse_idx, o.fuse_role, o.up_peer, (int)o.has_res, o.amax_off);
    }
    return s;
}
