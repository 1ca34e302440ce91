// The executor behind mdhip_forward and its kin (mdhip_capi.cpp), in two halves.  resolve() decides, on the host alone, what every
// op of the plan (mdhip_plan.cpp) does in a pass over n images of h x w: tiles (forced, from the measured table, heuristic), fused
// bottlenecks, upsamples read in place, Detect decodes in a conv's epilogue, launch arguments, statistics.  launch_ops() launches
// resolved ops.  describe_launches() writes a resolved pass as text (tests/test_launches_cpu.py pins the decisions with it).

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mdhip_ctx.h"

namespace mdhip {

const ConvRegistry& conv_api(const mdhip_ctx* ctx) { return ctx->dtype == MDHIP_DTYPE_FP16 ? st_f16::conv_registry : st_bf16::conv_registry; }
int conv_num_cfgs() { return st_bf16::conv_registry.num_cfgs(); }
const ConvCfg& conv_cfg(int i) { return st_bf16::conv_registry.cfg(i); }
bool conv_cfg_is_bitwise_family(int c) { return st_bf16::conv_registry.is_bitwise_family(c); }

// heuristic tile choice over the first-generation configurations (each with its measured prior, conv_igemm.cpp); measured
// overrides arrive through mdhip_set_op_cfg
int choose_cfg(int M, int n_rows) {
    const ConvFamily& v1 = *st_bf16::conv_registry.fam[CONV_IGEMM];
    int best = 0;
    float best_score = -1.f;
    for (int i = 0; i < v1.n_cfgs; ++i) {
        const ConvCfg& c = v1.cfgs[i];
        const int tn = (n_rows + c.bn - 1) / c.bn, tm = (M + c.bm - 1) / c.bm;
        const float useful = ((float)n_rows / (tn * c.bn)) * ((float)M / ((float)tm * c.bm));
        const float fill = std::min(1.0f, (float)tm * tn / 512.0f);
        const float score = useful * (0.35f + 0.65f * fill) * c.prior;
        if (score > best_score) { best_score = score; best = i; }
    }
    return best;
}

// tile choice without a table entry: the fill-aware heuristic over the first-generation configurations for a 16-bit
// op; for an op with an e4m3 operand, the best-filling configuration among those that take it
int choose_cfg_for(const mdhip_ctx* ctx, const ConvArgs& a) {
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

// the launch arguments of a conv op but for what changes from call to call (launch_ops fills that in)
void conv_args(const mdhip_ctx* ctx, const Op& op, int n, int h, int w, ConvArgs& a) {
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
    a.out_qscale = 1.0f;
    a.wgt4 = pc.w4_off ? (const uint16_t*)(ctx->warena + pc.w4_off) : nullptr;
    a.k_pad4 = pc.k_pad4;
    a.groups = pc.groups;
    a.wgt4p = (pc.w4p_off && ctx->pair_enabled) ? (const uint16_t*)(ctx->warena + pc.w4p_off) : nullptr;
    a.k_pad4p = pc.k_pad4p;
    a.pw_stream = ctx->pw_stream;
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
        a.out_f8 = op.f8_out ? 1 : 0;          // (out_qscale: the tensor's scale at launch)
    }
}

namespace {

void conv_stats(const mdhip_ctx* ctx, const Op& op, const ConvArgs& a, int n, Launch& L) {
    const PackedConv& pc = ctx->packed[op.pc];
    L.gm = a.M;
    L.gn = pc.c_out;
    L.gk = pc.k_real;
    L.flops = 2.0 * (double)a.M * pc.c_out * pc.k_real;
    L.bytes = (double)n * a.H * a.W * op.in.c * 2.0 + (double)a.M * pc.c_out * (op.out_f32 ? 4.0 : 2.0) +
              (double)pc.c_out * pc.k_real * 2.0 + (op.has_res ? (double)a.M * pc.c_out * 2.0 : 0.0);
}

// the tile configuration of a conv op: forced (tests, autotune), from the table, or the heuristic
int pick_cfg(const mdhip_ctx* ctx, const Op& op, const ConvArgs& a, int n, bool* from_table) {
    *from_table = false;
    if (op.forced_cfg >= 0) return op.forced_cfg;
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
            *from_table = true;
            return pick->cfg;
        } else if (!fam) {
            *from_table = true;
            return canon->cfg;
        }                                   // else: heuristic below (bitwise family)
    }
    return choose_cfg_for(ctx, a);
}

// ---- fused bottlenecks (conv_v5c.cpp) --------------------------------------------------------------------------
// A C3 block runs its bottlenecks as one launch each (1x1 -> T in LDS -> 3x3 + residual) when every 3x3 of the block
// resolves to a strip configuration for this call: the block then ping-pongs between its two buffers (Y1 -> T -> Y1 ..;
// the fused kernel must not write the tensor it reads halos from), so it is all bottlenecks of a block or none.
// Same arithmetic and K order as the two separate launches: the same bits.

// the 3x3 `op` (bottleneck j of its block) as a fused launch: x = Y1 for even j, T for odd j
void fused_args(const mdhip_ctx* ctx, const Op& op, const Op& pre, ConvArgs& a) {
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

// `op` resolves (with its plain arguments `a`) to a tile of the kernel family `family`, and that tile takes the arguments `with`
bool resolves_to(const mdhip_ctx* ctx, const Op& op, const ConvArgs& a, int n, ConvFamilyId family, const ConvArgs& with) {
    bool from_table = false;
    const int cfg = pick_cfg(ctx, op, a, n, &from_table);
    return conv_api(ctx).family(cfg) == family && conv_api(ctx).supports(cfg, with);
}

bool group_is_fused(const mdhip_ctx* ctx, const std::vector<int>& group, int n, int h, int w) {
    for (int oi : group) {
        ConvArgs a{};
        conv_args(ctx, ctx->ops[oi], n, h, w, a);
        ConvArgs f = a;
        fused_args(ctx, ctx->ops[oi], ctx->ops[oi - 1], f);
        if (!resolves_to(ctx, ctx->ops[oi], a, n, CONV_V5_STRIP, f)) return false;
    }
    return true;
}

// the 1x1 conv `conv` reads the first channels of its concatenated input from the low-resolution tensor of the upsample
// op in front of it (which is then not run) when its tile configuration is one of conv_v2.cpp's: `a` gets those arguments
bool absorb_upsample(const mdhip_ctx* ctx, const Op& conv, int n, ConvArgs& a) {
    const Op& up = ctx->ops[conv.up_peer];
    ConvArgs b = a;
    b.in_up = (const uint16_t*)(ctx->arena + up.in.off);
    b.ld_up = up.in.ld;
    b.up_slabs = up.in.c / 64;
    if (up.in.c % 64 || !resolves_to(ctx, conv, a, n, CONV_V2, b)) return false;
    a = b;
    return true;
}

bool plain_pass(const DecodeTta& t) {
    return t.keep_from == 0 && t.keep_to == 0x7fffffff && t.out_off == 0 && t.scale == 1.0f && t.flip_lr == 0;
}

// anchors of the levels in front of `level` in a prediction row of an h x w input, `per_cell` of them per grid cell
int level_offset(const mdhip_ctx* ctx, int level, int h, int w, int per_cell) {
    int off = 0;
    for (int l = 0; l < level; ++l) {
        const int sl = (int)ctx->strides[l];
        off += per_cell * (h / sl) * (w / sl);
    }
    return off;
}

// Detect decode in this conv's epilogue (mdhip_decode_store): the plain forward of a head with 8 outputs per anchor, on a
// tile that takes the op as a decoding one (the two kernel families that take 1x1 / fp32-output ops have such
// instantiations); the augmented forward (anchors kept / de-scaled / flipped per pass) and every other head keep the
// separate decode launch.  Settles the conv's record and the one of its decode op, the next op.
void resolve_decode(const mdhip_ctx* ctx, Resolved& r, size_t conv) {
    Launch& L = r.ops[conv];
    const Op& dec = ctx->ops[conv + 1];
    L.decodes = ctx->fuse_decode && !ctx->fuse_suspended && ctx->no == 8 && plain_pass(ctx->cur_tta) && !ctx->calibrating &&
                conv_api(ctx).supports_decoding(L.cfg, L.a);
    L.a.dec_anchors = (const float*)(ctx->warena + ctx->anchors_off) + dec.level * ctx->na * 2;
    L.a.dec_stride = ctx->strides[dec.level];
    L.a.dec_level_off = level_offset(ctx, dec.level, r.h, r.w, ctx->na);
    Launch& D = r.ops[conv + 1];
    D.how = L.decodes ? RUN_IN_FRONT : RUN_LAUNCH;
    D.bytes = L.decodes ? 0 : (double)r.n * (r.h / dec.in.div) * (r.w / dec.in.div) * ctx->na * ctx->no * 8.0;
}

void resolve_conv(const mdhip_ctx* ctx, Resolved& r, size_t i, bool fused) {
    const Op& op = ctx->ops[i];
    Launch& L = r.ops[i];
    ConvArgs& a = L.a;
    conv_args(ctx, op, r.n, r.h, r.w, a);
    conv_stats(ctx, op, a, r.n, L);
    const bool up_in_place = op.up_peer >= 0 && ctx->fuse_enabled && !ctx->fuse_suspended && absorb_upsample(ctx, op, r.n, a);
    if (up_in_place) {
        r.ops[op.up_peer].how = RUN_IN_PLACE;
        L.bytes -= (double)a.M * ctx->ops[op.up_peer].in.c * 2.0 * 0.75;      // a quarter of those pixels is read
    }
    if (fused && op.fuse_role == 1) {            // this 1x1 runs inside the following 3x3's launch, accounted there
        L.how = RUN_IN_NEXT;
        L.flops = L.bytes = 0;
        return;
    }
    if (fused) {
        const PackedConv& pp = ctx->packed[ctx->ops[i - 1].pc];
        fused_args(ctx, op, ctx->ops[i - 1], a);
        L.flops += 2.0 * (double)a.M * pp.c_out * pp.k_real;      // the 1x1 in front: the same pixels
        L.bytes -= (double)a.M * a.N * 2.0;       // T is neither written nor read
    }
    L.cfg = pick_cfg(ctx, op, a, r.n, &L.from_table);
    // with `fused` the arguments have in / out swapped and the 1x1 in front is skipped, with `up_in_place` the upsample
    // launch is skipped: no other tile may take this op's place at launch
    L.as_planned = !fused && !up_in_place;
    if (op.out_f32 && i + 1 < ctx->ops.size() && ctx->ops[i + 1].kind == OP_DECODE) resolve_decode(ctx, r, i);
}

// what the ops without a tile move and compute (mdhip_get_op_info)
void resolve_other(const mdhip_ctx* ctx, const Op& op, int n, int h, int w, Launch& L) {
    const int H = h / op.in.div, W = w / op.in.div;
    const double px = (double)n * H * W;
    switch (op.kind) {
        case OP_POOL: L.bytes = px * op.in.c * 2.0 * 4.0; break;
        case OP_UPSAMPLE: L.bytes = L.how == RUN_IN_PLACE ? 0 : px * op.in.c * 2.0 * 5.0; break;
        case OP_COPY: L.bytes = px * op.in.c * 4.0; break;
        case OP_DW: {
            const PackedConv& pc = ctx->packed[op.pc];
            L.gm = n * H * W;
            L.gn = pc.c_out;
            L.gk = 9;
            L.flops = 2.0 * px * pc.c_out * 9;
            L.bytes = px * pc.c_out * 2.0 * (op.has_res ? 3.0 : 2.0) + (double)pc.c_out * (9 * 2 + 4);
            break;
        }
        case OP_ATTN: {
            const double N = (double)H * W;
            // QK^T (32 channels) and PV (64 channels) per head: 2 N^2 (32 + 64) FLOPs
            L.gm = L.gn = H * W;
            L.gk = 32;
            L.flops = (double)n * op.heads * 2.0 * N * N * (32 + 64);
            L.bytes = (double)n * N * op.heads * (128 + 64) * 2.0;
            break;
        }
        case OP_DFL:
            L.gm = n * H * W;
            L.bytes = px * (64 + ctx->nc + ctx->no) * 4.0;
            break;
        case OP_ADOWN: {
            const double half = op.out.c;
            // input read once, the averaged half written at H x W, the max-pooled half at H/2 x W/2
            L.gm = n * H * W;
            L.bytes = px * half * 2.0 * 2.0 + px * half * 2.0 + (double)n * (H / 2) * (W / 2) * half * 2.0;
            break;
        }
        case OP_CBFUSE:
            L.gm = n * H * W;
            L.bytes = 2.0 * px * op.in.c * 2.0;
            for (int k = 0; k < op.n_fsrc; ++k) L.bytes += (double)n * (H / op.ffac[k]) * (W / op.ffac[k]) * op.in.c * 2.0;
            break;
        default: break;      // OP_CONV, OP_DECODE: settled by resolve_conv
    }
}

}  // namespace

// what every op does in a pass over n images of h x w in the context's current state (settings, table, forced tiles, kind of
// pass): each fused group and each upsample / consumer pair is decided once.  No device call, nothing written into the context.
std::shared_ptr<Resolved> resolve(const mdhip_ctx* ctx, int n, int h, int w) {
    auto r = std::make_shared<Resolved>();
    r->generation = ctx->generation;
    r->n = n; r->h = h; r->w = w;
    r->ops.resize(ctx->ops.size());
    std::vector<char> fused(ctx->fuse_groups.size(), 0);
    if (ctx->fuse_enabled && !ctx->fuse_suspended)
        for (size_t g = 0; g < fused.size(); ++g) fused[g] = group_is_fused(ctx, ctx->fuse_groups[g], n, h, w);
    // the convs decide (for their upsample in front and their decode op behind, too), the others follow
    for (size_t i = 0; i < ctx->ops.size(); ++i) {
        const Op& op = ctx->ops[i];
        if (op.kind == OP_CONV) resolve_conv(ctx, *r, i, op.fuse_role != 0 && op.fuse_group >= 0 && fused[op.fuse_group]);
    }
    for (size_t i = 0; i < ctx->ops.size(); ++i) resolve_other(ctx, ctx->ops[i], n, h, w, r->ops[i]);
    return r;
}

std::shared_ptr<Resolved> resolved_for(mdhip_ctx* ctx, int n, int h, int w) {
    const int pass = (plain_pass(ctx->cur_tta) ? 1 : 0) | (ctx->fuse_suspended ? 2 : 0) | (ctx->calibrating ? 4 : 0);
    const auto key = std::make_tuple(n, h, w, pass);
    auto it = ctx->resolved.find(key);
    if (it == ctx->resolved.end() || it->second->generation != ctx->generation) {
        if (ctx->resolved.size() >= (size_t)mdhip_ctx::kMaxResolved) ctx->resolved.clear();     // (a run has few shapes)
        it = ctx->resolved.insert_or_assign(key, resolve(ctx, n, h, w)).first;
    }
    return it->second;
}

namespace {

int launch_op(mdhip_ctx* ctx, Resolved& r, size_t i, hipStream_t s) {
    const Op& op = ctx->ops[i];
    Launch& L = r.ops[i];
    if (L.how != RUN_LAUNCH) return MDHIP_OK;
    const int n = r.n, H = r.h / op.in.div, W = r.w / op.in.div;
    const bool f16 = ctx->dtype == MDHIP_DTYPE_FP16;
    const uint16_t* in = (const uint16_t*)(ctx->arena + op.in.off);
    uint16_t* out = (uint16_t*)(ctx->arena + op.out.off);
    float* pred = (float*)(ctx->arena + ctx->pred_off);
    switch (op.kind) {
        case OP_CONV: {
            ConvArgs a = L.a;
            if (a.out_f8) a.out_qscale = 1.0f / op.act_scale;
            a.dec_pred = L.decodes ? pred : nullptr;
            a.dec_n_anchors = ctx->cur_A;
            hipError_t le = conv_api(ctx).launch(L.cfg, a, s);
            if (le == hipErrorInvalidValue && L.from_table && L.as_planned) {
                // table entry from another build: not applicable -> the heuristic, from now on.  (A fused or upsample-reading
                // launch keeps the error: resolve checked supports() for this very configuration, reaching this is a bug.)
                (void)hipGetLastError();
                L.cfg = choose_cfg_for(ctx, L.a);
                L.from_table = false;
                if (L.a.dec_anchors) resolve_decode(ctx, r, i);       // (set for a Detect conv, whose decode op is the next op)
                a.dec_pred = L.decodes ? pred : nullptr;
                le = conv_api(ctx).launch(L.cfg, a, s);
            }
            HIP_TRY(ctx, le);
            if (ctx->calibrating && op.f8_out)
                HIP_TRY(ctx, launch_absmax_view(out, op.out.ld, op.out.c, (long long)a.M, 0, (float*)(ctx->arena + op.amax_off), s));
            break;
        }
        case OP_POOL: HIP_TRY(ctx, launch_sppf_pool(out, op.out.ld, op.in.c, n, H, W, op.pool_k, f16, s)); break;
        case OP_UPSAMPLE: HIP_TRY(ctx, launch_upsample2x(in, op.in.ld, out, op.out.ld, op.in.c, n, H, W, s)); break;
        case OP_COPY: HIP_TRY(ctx, launch_copy_view(in, op.in.ld, out, op.out.ld, op.in.c, (long long)n * H * W, s)); break;
        case OP_DW: {
            const PackedConv& pc = ctx->packed[op.pc];
            HIP_TRY(ctx, launch_dwconv3x3(in, op.in.ld, (const uint16_t*)(ctx->warena + pc.w_off), (const float*)(ctx->warena + pc.b_off),
                                          out, op.out.ld, op.has_res ? (const uint16_t*)(ctx->arena + op.res.off) : nullptr,
                                          op.has_res ? op.res.ld : 0, n, H, W, pc.c_out, op.dw_grp, op.dw_grp_stride, op.dw_grp_off,
                                          op.act, f16, s));
            break;
        }
        case OP_ATTN: HIP_TRY(ctx, launch_attention(in, op.in.ld, out, op.out.ld, n, H * W, op.heads, f16, s)); break;
        case OP_DFL:
            HIP_TRY(ctx, launch_dfl_decode((const float*)(ctx->arena + op.f32_off), op.f32_ld, (const float*)(ctx->arena + op.cls_off),
                                           op.cls_ld, pred, n, H, W, ctx->nc, ctx->cur_A, level_offset(ctx, op.level, r.h, r.w, 1),
                                           ctx->strides[op.level], s));
            break;
        case OP_ADOWN:
            HIP_TRY(ctx, launch_adown_pool(in, op.in.ld, out, op.out.ld, (uint16_t*)(ctx->arena + op.out2.off), op.out2.ld, n, H, W,
                                           op.in.c, f16, s));
            break;
        case OP_CBFUSE: {
            CbfuseArgs a{};
            a.n = n;
            a.H = H;
            a.W = W;
            a.C = op.in.c;
            a.n_src = op.n_fsrc;
            for (int k = 0; k < op.n_fsrc; ++k) {
                a.src[k] = (const uint16_t*)(ctx->arena + op.fsrc[k].off);
                a.ld_src[k] = op.fsrc[k].ld;
                a.factor[k] = op.ffac[k];
            }
            a.last = in;
            a.ld_last = op.in.ld;
            a.out = out;
            a.ld_out = op.out.ld;
            HIP_TRY(ctx, launch_cbfuse(a, f16, s));
            break;
        }
        case OP_DECODE:
            HIP_TRY(ctx, launch_detect_decode((const float*)(ctx->arena + op.f32_off), op.f32_ld, pred, n, H, W, ctx->na, ctx->no,
                                              ctx->cur_A, level_offset(ctx, op.level, r.h, r.w, ctx->na), ctx->strides[op.level],
                                              (const float*)(ctx->warena + ctx->anchors_off) + op.level * ctx->na * 2, ctx->cur_tta, s));
            break;
    }
    return MDHIP_OK;
}

}  // namespace

// launches ops [first, first + count) of a resolved pass on `s`, with what changes from call to call: the prediction buffer,
// the anchor pitch and placement of the pass (mdhip_ctx::cur_A, cur_tta), the fp8 output scale
int launch_ops(mdhip_ctx* ctx, Resolved& r, size_t first, size_t count, hipStream_t s) {
    for (size_t i = first; i < first + count && i < r.ops.size(); ++i)
        if (int rc = launch_op(ctx, r, i, s)) return rc;
    return MDHIP_OK;
}

// a resolved pass as text (mdhip_launches_describe): one line per op
std::string describe_launches(const mdhip_ctx* ctx, const Resolved& r) {
    static const char* const how[] = {"plain", "in_next", "in_place", "in_front"};
    std::string text;
    char line[512];
    for (size_t i = 0; i < r.ops.size(); ++i) {
        const Launch& L = r.ops[i];
        const bool tile = ctx->ops[i].kind == OP_CONV && L.how == RUN_LAUNCH;
        snprintf(line, sizeof(line), "op %d \"%s\" %s cfg=%s table=%d decodes=%d m=%d n=%d k=%d flops=%.17g bytes=%.17g\n", (int)i,
                 ctx->ops[i].name.c_str(), tile ? "launch" : how[L.how], tile ? conv_cfg(L.cfg).name : "-", L.from_table ? 1 : 0,
                 L.decodes ? 1 : 0, L.gm, L.gn, L.gk, L.flops, L.bytes);
        text += line;
    }
    return text;
}

}  // namespace mdhip
