// The executor behind mdhip_forward and its kin (mdhip_capi.cpp): the conv API of the context's storage type, the tile choice
// of a conv op (forced, remembered, from the measured table, heuristic), the fused-bottleneck and absorbed-upsample decisions
// and run_op, which launches one op of the plan (mdhip_plan.cpp) for a batch of n images of h x w.

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mdhip_ctx.h"

namespace mdhip {

// the conv API of the context's storage type (the kernels are compiled once per type, mdhip_internal.h)
const ConvApi g_conv_bf16 = {st_bf16::conv_num_cfgs, st_bf16::conv_cfg, st_bf16::conv_launch, st_bf16::conv_init,
                             st_bf16::conv_supports, st_bf16::conv_cfg_is_bitwise_family, st_bf16::conv_num_v1_cfgs, st_bf16::conv_cfg_decodes};
const ConvApi g_conv_f16 = {st_f16::conv_num_cfgs, st_f16::conv_cfg, st_f16::conv_launch, st_f16::conv_init,
                            st_f16::conv_supports, st_f16::conv_cfg_is_bitwise_family, st_f16::conv_num_v1_cfgs, st_f16::conv_cfg_decodes};
const ConvApi& conv_api(const mdhip_ctx* ctx) { return ctx->dtype == MDHIP_DTYPE_FP16 ? g_conv_f16 : g_conv_bf16; }
// tile configurations (count, names, families) are the same for both storage types
int conv_num_cfgs() { return g_conv_bf16.num_cfgs(); }
const ConvCfg& conv_cfg(int i) { return g_conv_bf16.cfg(i); }
bool conv_cfg_is_bitwise_family(int c) { return g_conv_bf16.is_bitwise_family(c); }
inline int conv_num_v1_cfgs() { return g_conv_bf16.num_v1_cfgs(); }

// heuristic tile choice; measured overrides arrive through mdhip_set_op_cfg
int choose_cfg(int M, int n_rows) {
    // prior from measurements on MI355X (profiles/autotune_r1.txt); tools/autotune.py refines it
    static const float quality[] = {0.92f, 1.00f, 0.55f, 0.95f, 0.45f, 0.70f, 0.85f, 0.85f, 0.95f, 0.55f, 0.45f, 0.65f,
                                    0.95f, 1.00f, 1.00f, 0.95f, 0.95f, 0.60f, 0.90f, 0.88f, 0.88f, 0.55f, 0.70f, 0.45f,
                                    0.50f, 0.50f, 0.50f, 0.50f};
    static_assert(sizeof(quality) / sizeof(quality[0]) == 28, "one prior per tile configuration");
    int best = 0;
    float best_score = -1.f;
    for (int i = 0; i < conv_num_v1_cfgs(); ++i) {
        const ConvCfg& c = conv_cfg(i);
        const int tn = (n_rows + c.bn - 1) / c.bn, tm = (M + c.bm - 1) / c.bm;
        const float useful = ((float)n_rows / (tn * c.bn)) * ((float)M / ((float)tm * c.bm));
        const float fill = std::min(1.0f, (float)tm * tn / 512.0f);
        const float score = useful * (0.35f + 0.65f * fill) * quality[i];
        if (score > best_score) { best_score = score; best = i; }
    }
    return best;
}

// tile choice without a table entry: the fill-aware heuristic over the first-generation configurations for a 16-bit
// op; for an op with an e4m3 operand, the best-filling configuration among those that take it
int choose_cfg_for(mdhip_ctx* ctx, const ConvArgs& a) {
    if (!a.in_f8 && !a.out_f8) return choose_cfg(a.M, a.n_rows);
    int best = -1;
    float best_score = -1.f;
    for (int i = 0; i < conv_num_cfgs(); ++i) {
        if (!conv_api(ctx).supports(i, a)) continue;
        const ConvCfg& c = conv_cfg(i);
        const int tn = (a.n_rows + c.bn - 1) / c.bn, tm = (a.M + c.bm - 1) / c.bm;
        const float useful = ((float)a.n_rows / (tn * c.bn)) * ((float)a.M / ((float)tm * c.bm));
        const float fill = std::min(1.0f, (float)tm * tn / (256.0f * c.blocks_per_cu));
        const float score = useful * (0.35f + 0.65f * fill) * (c.blocks_per_cu == 2 ? 1.0f : 0.95f);
        if (score > best_score) { best_score = score; best = i; }
    }
    return best < 0 ? 0 : best;
}

void fill_conv_args(mdhip_ctx* ctx, Op& op, int n, int h, int w, ConvArgs& a) {
    const PackedConv& pc = ctx->packed[op.pc];
    const int H = h / op.in.div, W = w / op.in.div;
    const int Ho = H / op.stride, Wo = W / op.stride;
    a.in = (const uint16_t*)(ctx->arena + op.in.off);
    a.wgt = (const uint16_t*)(ctx->warena + pc.w_off);
    a.bias = (const float*)(ctx->warena + pc.b_off);
    a.zero = (const uint16_t*)(ctx->warena + ctx->zero_off);
    a.ld_in = op.in.ld;
    a.H = H;
    a.W = W;
    a.C8 = pc.cin_pad / 8;
    a.Ho = Ho;
    a.Wo = Wo;
    a.HoWo = Ho * Wo;
    a.M = n * Ho * Wo;
    a.N = pc.c_out;
    a.n_rows = pc.n_rows;
    a.k_pad = pc.k_pad;
    a.ntaps = pc.kh * pc.kw;
    a.kw = pc.kw;
    a.stride = op.stride;
    a.pad = op.pad;
    a.act = op.act;
    a.out_f32 = op.out_f32;
    if (op.out_f32) {
        a.out = ctx->arena + op.f32_off;
        a.ld_out = op.f32_ld;
    } else {
        a.out = ctx->arena + op.out.off;
        a.ld_out = op.out.ld;
    }
    a.res = op.has_res ? (const uint16_t*)(ctx->arena + op.res.off) : nullptr;
    a.ld_res = op.has_res ? op.res.ld : 0;
    a.tiles_n = 1;
    a.dbg = nullptr;
    a.dev_param = 0;
    a.wgt8 = nullptr;
    a.scale = nullptr;
    a.k_pad8 = a.groups8 = 0;
    a.in_f8 = a.out_f8 = 0;
    a.out_qscale = 1.0f;
    a.wgt4 = pc.w4_off ? (const uint16_t*)(ctx->warena + pc.w4_off) : nullptr;
    a.k_pad4 = pc.k_pad4;
    a.groups = pc.groups;
    a.wgt4p = (pc.w4p_off && ctx->pair_enabled) ? (const uint16_t*)(ctx->warena + pc.w4p_off) : nullptr;
    a.k_pad4p = pc.k_pad4p;
    if (ctx->dtype == MDHIP_DTYPE_FP8 && !ctx->calibrating) {
        if (op.f8_in) {
            // the e4m3 tensor lives in the 16-bit tensor's allocation: same pixel pitch, counted in bytes
            a.in_f8 = 1;
            a.wgt8 = (const uint8_t*)(ctx->warena + pc.w8_off);
            a.scale = (const float*)(ctx->warena + pc.scale_off);
            a.k_pad8 = pc.k_pad8;
            a.groups8 = pc.groups8;
            a.C8 = (op.in.c + 15) / 16;
        }
        if (op.f8_out) {
            a.out_f8 = 1;
            a.out_qscale = 1.0f / op.act_scale;
        }
    }
    op.gm = a.M;
    op.gn = pc.c_out;
    op.gk = pc.k_real;
    op.flops = 2.0 * (double)a.M * pc.c_out * pc.k_real;
    const double in_px = (double)n * H * W;
    op.bytes = in_px * op.in.c * 2.0 + (double)a.M * pc.c_out * (op.out_f32 ? 4.0 : 2.0) +
               (double)pc.c_out * pc.k_real * 2.0 + (op.has_res ? (double)a.M * pc.c_out * 2.0 : 0.0);
}

// the tile configuration of a conv op for this call: forced (tests, autotune), remembered from the last call of the same
// shape, or from the table (see below); -1 = none of them applies (the caller falls back to the heuristic)
int select_cfg(mdhip_ctx* ctx, Op& op, const ConvArgs& a, int n, int h, int w, bool* from_table_out) {
    int cfg = op.forced_cfg;
    bool from_table = false;
    const bool memo_hit = cfg < 0 && op.memo_cfg >= 0 && op.memo_n == n && op.memo_h == h && op.memo_w == w;
    if (memo_hit) {
        cfg = op.memo_cfg;
        from_table = op.memo_from_table;
    } else if (cfg < 0) {
        const PackedConv& pc = ctx->packed[op.pc];
        // 1. The canonical entry: same layer geometry (N, K, taps, stride, residual), per-image M equal
        //    or nearest within 4x (the same layer at another image shape, e.g. 960x1280 instead of
        //    1280x1280), largest batch among equals.  It fixes the kernel FAMILY (= fp32 summation
        //    order) of the op -- per image, never per call, or an image's result would depend on the
        //    batch it travels in.
        // 2. Among the entries of that geometry, per-image M and family: the one measured at the
        //    nearest total M (= nearest batch size).  Small batches want smaller tiles.
        // 3. No entry within 4x of this call's total M: the fill-aware heuristic for the bitwise family,
        //    the canonical configuration otherwise.
        const double m_img = (double)a.M / n;
        const mdhip_tuned* canon = nullptr;
        double best = 1e30;
        for (const mdhip_tuned& t : ctx->tuned) {
            if (t.n != pc.c_out || t.k != pc.k_real || t.ntaps != a.ntaps || t.stride != a.stride ||
                t.has_res != (op.has_res ? 1 : 0) || t.m <= 0)
                continue;
            const int tb = t.batch > 0 ? t.batch : 32;
            const double t_img = (double)t.m / tb;
            const double r = t_img > m_img ? t_img / m_img : m_img / t_img;
            if (r > 4.0 || !conv_api(ctx).supports(t.cfg, a)) continue;
            const int cb = canon ? (canon->batch > 0 ? canon->batch : 32) : 0;
            if (r < best - 1e-9 || (r < best + 1e-9 && tb > cb)) {
                best = r;
                canon = &t;
            }
        }
        if (canon) {
            const bool fam = conv_cfg_is_bitwise_family(canon->cfg);
            const double c_img = (double)canon->m / (canon->batch > 0 ? canon->batch : 32);
            const mdhip_tuned* pick = nullptr;
            double best_m = 1e30;
            for (const mdhip_tuned& t : ctx->tuned) {
                if (t.n != canon->n || t.k != canon->k || t.ntaps != canon->ntaps || t.stride != canon->stride ||
                    t.has_res != canon->has_res || t.m <= 0 || conv_cfg_is_bitwise_family(t.cfg) != fam)
                    continue;
                const double t_img = (double)t.m / (t.batch > 0 ? t.batch : 32);
                if (t_img < c_img * 0.999 || t_img > c_img * 1.001 || !conv_api(ctx).supports(t.cfg, a)) continue;
                const double scaled = (double)t.m * (m_img / t_img);          // total M of that batch at this image shape
                const double r = scaled > a.M ? scaled / a.M : a.M / scaled;
                if (r < best_m) { best_m = r; pick = &t; }
            }
            if (pick && best_m <= 4.0) {
                cfg = pick->cfg;
                from_table = true;
            } else if (!fam) {
                cfg = canon->cfg;
                from_table = true;
            }                                   // else: heuristic below (bitwise family)
        }
    }
    *from_table_out = from_table;
    return cfg;
}

// ---- fused bottlenecks (conv_v5c.cpp) --------------------------------------------------------------------------
// A C3 block runs its bottlenecks as one launch each (1x1 -> T in LDS -> 3x3 + residual) when every 3x3 of the block
// resolves to a strip configuration for this call: the block then ping-pongs between its two buffers (Y1 -> T -> Y1 ..;
// the fused kernel must not write the tensor it reads halos from), so it is all bottlenecks of a block or none.
// Same arithmetic and K order as the two separate launches: the same bits.

// the 3x3 `op` (bottleneck j of its block) as a fused launch: x = Y1 for even j, T for odd j
void fused_args(mdhip_ctx* ctx, const Op& op, const Op& pre, ConvArgs& a) {
    const Tensor& X = (op.fuse_idx % 2 == 0) ? op.out : op.in;
    const Tensor& O = (op.fuse_idx % 2 == 0) ? op.in : op.out;
    const PackedConv& pp = ctx->packed[pre.pc];
    a.in = (const uint16_t*)(ctx->arena + X.off);
    a.ld_in = X.ld;
    a.out = ctx->arena + O.off;
    a.ld_out = O.ld;
    a.res = op.has_res ? a.in : nullptr;
    a.ld_res = op.has_res ? X.ld : 0;
    a.wgt_pre = (const uint16_t*)(ctx->warena + pp.w_off);
    a.bias_pre = (const float*)(ctx->warena + pp.b_off);
    a.k_pad_pre = pp.k_pad;
}

bool group_is_fused(mdhip_ctx* ctx, int group, int n, int h, int w) {
    if (group < 0 || !ctx->fuse_enabled || ctx->fuse_suspended) return false;
    for (int oi : ctx->fuse_groups[group]) {
        Op& op = ctx->ops[oi];
        const Op& pre = ctx->ops[oi - 1];
        const double f0 = op.flops, b0 = op.bytes;
        ConvArgs a{};
        fill_conv_args(ctx, op, n, h, w, a);
        op.flops = f0; op.bytes = b0;
        bool from_table = false;
        int cfg = select_cfg(ctx, op, a, n, h, w, &from_table);
        if (cfg < 0) cfg = choose_cfg_for(ctx, a);
        if (cfg < 0 || strncmp(conv_api(ctx).cfg(cfg).name, "v5:strip", 8) != 0) return false;
        fused_args(ctx, op, pre, a);
        if (!conv_api(ctx).supports(cfg, a)) return false;
    }
    return true;
}

// the 1x1 conv `conv` reads the first channels of its concatenated input from the low-resolution tensor of the upsample
// op in front of it (which is then not run) when its tile configuration is one of conv_v2.cpp's
void up_args(mdhip_ctx* ctx, const Op& up, ConvArgs& a) {
    a.in_up = (const uint16_t*)(ctx->arena + up.in.off);
    a.ld_up = up.in.ld;
    a.up_slabs = up.in.c / 64;
}

bool up_is_absorbed(mdhip_ctx* ctx, Op& conv, int n, int h, int w) {
    if (conv.up_peer < 0 || !ctx->fuse_enabled || ctx->fuse_suspended) return false;
    const Op& up = ctx->ops[conv.up_peer];
    if (up.in.c % 64) return false;
    const double f0 = conv.flops, b0 = conv.bytes;
    ConvArgs a{};
    fill_conv_args(ctx, conv, n, h, w, a);
    conv.flops = f0; conv.bytes = b0;
    bool from_table = false;
    int cfg = select_cfg(ctx, conv, a, n, h, w, &from_table);
    if (cfg < 0) cfg = choose_cfg_for(ctx, a);
    if (cfg < 0 || strncmp(conv_api(ctx).cfg(cfg).name, "v2:", 3) != 0) return false;
    up_args(ctx, up, a);
    return conv_api(ctx).supports(cfg, a);
}

int run_op(mdhip_ctx* ctx, Op& op, int n, int h, int w, hipStream_t s) {
    switch (op.kind) {
        case OP_CONV: {
            ConvArgs a{};
            const bool fused = op.fuse_role != 0 && group_is_fused(ctx, op.fuse_group, n, h, w);
            const bool up_in_place = op.up_peer >= 0 && up_is_absorbed(ctx, op, n, h, w);
            fill_conv_args(ctx, op, n, h, w, a);
            if (up_in_place) {
                up_args(ctx, ctx->ops[op.up_peer], a);
                op.bytes -= (double)a.M * ctx->ops[op.up_peer].in.c * 2.0 * 0.75;      // a quarter of those pixels is read
            }
            if (fused && op.fuse_role == 1) {            // this 1x1 runs inside the following 3x3's launch
                op.last_cfg = -1;
                op.pre_flops = op.flops;                  // accounted with the fused launch
                op.flops = op.bytes = 0;
                break;
            }
            if (fused) {
                const Op& pre = *(&op - 1);
                fused_args(ctx, op, pre, a);
                op.flops += pre.pre_flops;
                op.bytes -= (double)a.M * a.N * 2.0;       // T is neither written nor read
            }
            bool from_table = false;
            int cfg = select_cfg(ctx, op, a, n, h, w, &from_table);
            if (cfg < 0) cfg = choose_cfg_for(ctx, a);
            // Detect decode in this conv's epilogue (mdhip_decode_store): the plain forward of a head with 8 outputs per anchor,
            // on the two kernel families that take 1x1 / fp32-output ops; the augmented forward (anchors kept / de-scaled /
            // flipped per pass) and every other head keep the separate decode launch
            Op* dec = (op.out_f32 && (size_t)(&op - ctx->ops.data()) + 1 < ctx->ops.size() && (&op)[1].kind == OP_DECODE) ? &op + 1 : nullptr;
            if (dec) dec->dec_done = false;
            const bool plain_pass = ctx->cur_tta.keep_from == 0 && ctx->cur_tta.keep_to == 0x7fffffff && ctx->cur_tta.out_off == 0 &&
                                    ctx->cur_tta.scale == 1.0f && ctx->cur_tta.flip_lr == 0;
            // (pointwise with whole 64-channel slabs: what the decoding instantiations of conv_v2.cpp take)
            auto decodes_in_place = [&](int c) {
                return dec && ctx->fuse_decode && !ctx->fuse_suspended && ctx->no == 8 && plain_pass && !ctx->calibrating &&
                       conv_api(ctx).cfg_decodes(c) && (c < conv_num_v1_cfgs() || (a.C8 & 7) == 0);
            };
            auto set_decode = [&](int c) {
                a.dec_pred = nullptr;
                if (!decodes_in_place(c)) return;
                int level_off = 0;
                for (int l = 0; l < dec->level; ++l) {
                    const int sl = (int)ctx->strides[l];
                    level_off += ctx->na * (h / sl) * (w / sl);
                }
                a.dec_pred = (float*)(ctx->arena + ctx->pred_off);
                a.dec_anchors = (const float*)(ctx->warena + ctx->anchors_off) + dec->level * ctx->na * 2;
                a.dec_stride = ctx->strides[dec->level];
                a.dec_level_off = level_off;
                a.dec_n_anchors = ctx->cur_A;
            };
            set_decode(cfg);
            hipError_t le = conv_api(ctx).launch(cfg, a, s);
            if (le == hipErrorInvalidValue && from_table && !fused && !up_in_place) {
                // table entry from another build: not applicable.  Only for an op that is launched as planned: with
                // `fused` the arguments have in / out swapped and the 1x1 in front was skipped, with `up_in_place` the
                // upsample launch was skipped -- a kernel that ignores those fields would read tensors that were
                // never written, so those cases keep the error (group_is_fused / up_is_absorbed checked supports()
                // for this very configuration: reaching this is a bug, not a stale table).
                (void)hipGetLastError();
                cfg = choose_cfg_for(ctx, a);
                from_table = false;
                set_decode(cfg);
                le = conv_api(ctx).launch(cfg, a, s);
            }
            if (dec && a.dec_pred && le == hipSuccess) {
                dec->dec_done = true;
            }
            op.last_cfg = cfg;
            if (op.forced_cfg < 0 && le == hipSuccess) {
                op.memo_n = n; op.memo_h = h; op.memo_w = w; op.memo_cfg = cfg; op.memo_from_table = from_table;
            }
            HIP_TRY(ctx, le);
            if (ctx->calibrating && op.f8_out)
                HIP_TRY(ctx, launch_absmax_view((const uint16_t*)(ctx->arena + op.out.off), op.out.ld, op.out.c, (long long)a.M,
                                                0, (float*)(ctx->arena + op.amax_off), s));
            break;
        }
        case OP_POOL: {
            const int H = h / op.in.div, W = w / op.in.div;
            op.flops = 0;
            op.bytes = (double)n * H * W * op.in.c * 2.0 * 4.0;
            HIP_TRY(ctx, launch_sppf_pool((uint16_t*)(ctx->arena + op.out.off), op.out.ld, op.in.c, n, H, W, op.pool_k, ctx->dtype == MDHIP_DTYPE_FP16, s));
            break;
        }
        case OP_UPSAMPLE: {
            if (op.up_peer >= 0 && up_is_absorbed(ctx, ctx->ops[op.up_peer], n, h, w)) {     // read in place by its consumer
                op.bytes = 0;
                break;
            }
            const int H = h / op.in.div, W = w / op.in.div;
            op.bytes = (double)n * H * W * op.in.c * 2.0 * 5.0;
            HIP_TRY(ctx, launch_upsample2x((const uint16_t*)(ctx->arena + op.in.off), op.in.ld,
                                           (uint16_t*)(ctx->arena + op.out.off), op.out.ld, op.in.c, n, H, W, s));
            break;
        }
        case OP_COPY: {
            const long long px = (long long)n * (h / op.in.div) * (w / op.in.div);
            op.bytes = (double)px * op.in.c * 4.0;
            HIP_TRY(ctx, launch_copy_view((const uint16_t*)(ctx->arena + op.in.off), op.in.ld,
                                          (uint16_t*)(ctx->arena + op.out.off), op.out.ld, op.in.c, px, s));
            break;
        }
        case OP_DW: {
            const PackedConv& pc = ctx->packed[op.pc];
            const int H = h / op.in.div, W = w / op.in.div;
            const double px = (double)n * H * W;
            op.gm = n * H * W;
            op.gn = pc.c_out;
            op.gk = 9;
            op.flops = 2.0 * px * pc.c_out * 9;
            op.bytes = px * pc.c_out * 2.0 * (op.has_res ? 3.0 : 2.0) + (double)pc.c_out * (9 * 2 + 4);
            op.last_cfg = -1;
            HIP_TRY(ctx, launch_dwconv3x3((const uint16_t*)(ctx->arena + op.in.off), op.in.ld, (const uint16_t*)(ctx->warena + pc.w_off),
                                          (const float*)(ctx->warena + pc.b_off), (uint16_t*)(ctx->arena + op.out.off), op.out.ld,
                                          op.has_res ? (const uint16_t*)(ctx->arena + op.res.off) : nullptr, op.has_res ? op.res.ld : 0,
                                          n, H, W, pc.c_out, op.dw_grp, op.dw_grp_stride, op.dw_grp_off, op.act,
                                          ctx->dtype == MDHIP_DTYPE_FP16, s));
            break;
        }
        case OP_ATTN: {
            const int H = h / op.in.div, W = w / op.in.div;
            const double N = (double)H * W;
            // QK^T (32 channels) and PV (64 channels) per head: 2 N^2 (32 + 64) FLOPs
            op.gm = H * W;
            op.gn = H * W;
            op.gk = 32;
            op.flops = (double)n * op.heads * 2.0 * N * N * (32 + 64);
            op.bytes = (double)n * N * op.heads * (128 + 64) * 2.0;
            op.last_cfg = -1;
            HIP_TRY(ctx, launch_attention((const uint16_t*)(ctx->arena + op.in.off), op.in.ld, (uint16_t*)(ctx->arena + op.out.off),
                                          op.out.ld, n, H * W, op.heads, ctx->dtype == MDHIP_DTYPE_FP16, s));
            break;
        }
        case OP_DFL: {
            const int ny = h / op.in.div, nx = w / op.in.div;
            int level_off = 0;
            for (int l = 0; l < op.level; ++l) {
                const int sl = (int)ctx->strides[l];
                level_off += (h / sl) * (w / sl);
            }
            op.gm = n * ny * nx;
            op.flops = 0;
            op.bytes = (double)n * ny * nx * (64 + ctx->nc + ctx->no) * 4.0;
            op.last_cfg = -1;
            HIP_TRY(ctx, launch_dfl_decode((const float*)(ctx->arena + op.f32_off), op.f32_ld, (const float*)(ctx->arena + op.cls_off),
                                           op.cls_ld, (float*)(ctx->arena + ctx->pred_off), n, ny, nx, ctx->nc, ctx->cur_A, level_off,
                                           ctx->strides[op.level], s));
            break;
        }
        case OP_ADOWN: {
            const int H = h / op.in.div, W = w / op.in.div;
            const double half = op.out.c;
            // input read once, the averaged half written at H x W, the max-pooled half at H/2 x W/2
            op.gm = n * H * W;
            op.flops = 0;
            op.bytes = (double)n * H * W * half * 2.0 * 2.0 + (double)n * H * W * half * 2.0 + (double)n * (H / 2) * (W / 2) * half * 2.0;
            op.last_cfg = -1;
            HIP_TRY(ctx, launch_adown_pool((const uint16_t*)(ctx->arena + op.in.off), op.in.ld, (uint16_t*)(ctx->arena + op.out.off),
                                           op.out.ld, (uint16_t*)(ctx->arena + op.out2.off), op.out2.ld, n, H, W, op.in.c,
                                           ctx->dtype == MDHIP_DTYPE_FP16, s));
            break;
        }
        case OP_CBFUSE: {
            CbfuseArgs a{};
            a.n = n;
            a.H = h / op.in.div;
            a.W = w / op.in.div;
            a.C = op.in.c;
            a.n_src = op.n_fsrc;
            double bytes = 2.0 * n * a.H * a.W * a.C * 2.0;
            for (int k = 0; k < op.n_fsrc; ++k) {
                a.src[k] = (const uint16_t*)(ctx->arena + op.fsrc[k].off);
                a.ld_src[k] = op.fsrc[k].ld;
                a.factor[k] = op.ffac[k];
                bytes += (double)n * (a.H / op.ffac[k]) * (a.W / op.ffac[k]) * a.C * 2.0;
            }
            a.last = (const uint16_t*)(ctx->arena + op.in.off);
            a.ld_last = op.in.ld;
            a.out = (uint16_t*)(ctx->arena + op.out.off);
            a.ld_out = op.out.ld;
            op.gm = n * a.H * a.W;
            op.flops = 0;
            op.bytes = bytes;
            op.last_cfg = -1;
            HIP_TRY(ctx, launch_cbfuse(a, ctx->dtype == MDHIP_DTYPE_FP16, s));
            break;
        }
        case OP_DECODE: {
            if (op.dec_done) {                     // decoded in the epilogue of the conv in front (this forward)
                op.bytes = 0;
                op.last_cfg = -2;                  // (mdhip_get_op_info: -2 = folded into the conv in front, -1 = own launch)
                break;
            }
            op.last_cfg = -1;
            const int ny = h / op.in.div, nx = w / op.in.div;
            int level_off = 0;
            for (int l = 0; l < op.level; ++l) {
                const int sl = (int)ctx->strides[l];
                level_off += ctx->na * (h / sl) * (w / sl);
            }
            op.bytes = (double)n * ny * nx * ctx->na * ctx->no * 8.0;
            HIP_TRY(ctx, launch_detect_decode((const float*)(ctx->arena + op.f32_off), op.f32_ld,
                                              (float*)(ctx->arena + ctx->pred_off), n, ny, nx, ctx->na,
                                              ctx->no, ctx->cur_A, level_off, ctx->strides[op.level],
                                              (const float*)(ctx->warena + ctx->anchors_off) + op.level * ctx->na * 2,
                                              ctx->cur_tta, s));
            break;
        }
    }
    return MDHIP_OK;
}

}  // namespace mdhip
