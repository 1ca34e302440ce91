"""
Three kernels of the forward element by element against float64: the C2PSA attention (attn_kernel) and the depthwise 3x3
(dwconv3x3_kernel) of yolo11_kernels.cpp, and the scaled input of an augmented pass (tta_scale_kernel, misc_kernels.cpp).  As in
tests/conv_probe.py every reference is float64 on exactly what the kernel read -- the stored values, weights rounded to storage --
and every element is held to a bound derived from the kernel's statements, not from a run.  tests/test_kernel_elements_cpu.py
shows without a GPU that float32 restatements of the kernels (emulated_attention, emulated_depthwise, emulated_tta) pass and that
planted mistakes (ATTN_MUTANTS, DW_MUTANTS, TTA_MUTANTS) do not; tests/test_gpu_kernel_elements.py runs the kernels through it, and
tests/op_step.py uses the first two for the ops of the real models.  u = U32 = 2^-24, u_st = half an ulp of the storage type
relative to its value (2^-8 bf16, 2^-11 fp16).

ATTENTION.  qkv (n, N, heads * 128), per head [q 32 | k 32 | v 64]; scale = 32^-0.5.  Reference, per (image, head, query i):
    s_j = q_i . k_j scale,  m = max_j s_j,  p_j = exp(s_j - m),  l = sum_j p_j,  y_c = sum_j p_j v_jc / l,  A_c = sum_j p_j |v_jc| / l.
The kernel walks the keys in steps of 32.  Per step: s^_j from an MFMA (32 exact products summed in fp32) times `scale`;
m_new = max(m, max_j s^_j);  alpha = __expf(m - m_new);  e_j = __expf(s^_j - m_new);  l = l alpha + sum_j e_j (8 adds in the lane, 2
across lanes);  P_j = e_j rounded to 16 bits;  O = O alpha, then O += P V by an MFMA (fp32);  at the end y^ = O / l, rounded once
to storage.  Write the computed O as sum_j p_j v_j (1 + eta_j) and l as sum_j p_j (1 + theta_j): eta_j and theta_j share a part
kappa_j (everything that happens to e_j before it is rounded to 16 bits, and the alphas, which multiply O and l alike), and have
parts of their own, eta'_j and theta'_j.  To first order
    y^ - y = sum_j p_j kappa_j (v_j - y) / l + sum_j p_j v_j eta'_j / l - y sum_j p_j theta'_j / l,
    |y^ - y| <= (2 max|kappa| + max|eta'| + max|theta'|) A                                   (|y| <= A).
A shift of all scores of a query cancels exactly, so the error of m itself does not enter.  The terms of  E = rel A:
    u_st                      eta': P_j rounded to 16 bits.
    2 max_j ds_j              kappa: the score's own error, ds = 40 u (|q| . |k|) scale: 32 products and the accumulator in any
                              order (32 + 4) u, the product with `scale` and scale's own rounding 2 u, taken as 40; twice, for
                              the (v_j - y) above.
    (4 + 2 max_j |s_j - m|) u kappa: __expf(x) is v_exp_f32(x log2 e).  The 4: the 1 ulp (2 u) of v_exp_f32 for e_j, twice.  The
                              argument: the subtraction and the product with log2 e round once each, |x| u each in the result.  The
                              alphas of the later steps multiply e_j; their arguments add up to m_final - m_step, so that the
                              arguments of e_j and of its alphas together are |s_j - m_final|: the chain costs no more than the
                              one exponential of the reference.  (Stated for the whole row by its largest |s - m|; the elements
                              that carry weight have small ones.)
    N u                       eta': the fp32 sum of the N nonzero products p_j v_j, in whatever order the MFMAs and their
                              accumulator chain add them (a padded key adds an exact zero).
    c1 ceil(N / 32) u         per 32-key step, on everything accumulated before it.  eta': O alpha (1), the step's sum added to
                              the accumulator (1).  theta': l alpha (1), + rs (1).  kappa: alpha's own v_exp_f32, 1 ulp = 2 u,
                              twice = 4 (it is exactly 1 while the running maximum stays).  c1 = 8.
    c2 u                      once.  theta': the 10 adds of a step's sum_j e_j (8 in the lane, 2 across).  eta': the division
                              O / l (IEEE, 1 u; taken as 2).  c2 = 12.
    rel = u_st + (c1 ceil(N / 32) + N + c2) u + (4 + 2 max_j |s_j - m|) u + 2 max_j ds_j.
(The issue that asked for this file measured c1 = 4, c2 = 16 as enough for a float32 restatement; the counts above are from
the statements and are a little wider, by 4 ceil(N / 32) - 4 units of u, against a u_st of 65536 u (bf16) or 8192 u (fp16).)
fp16 only: an e_j below 2^-14, the smallest normal, is stored as a subnormal fp16 or, should the MFMA flush its inputs, as nothing:
it loses at most all of itself.  small = sum_{j : p_j < 2^-14} p_j |v_j| / l is added to E.  p_j is measured against the final
maximum here, the kernel's e_j against the running one, which is never larger: e_j >= p_j, so the set is no smaller than the
kernel's.  (bf16 has the exponent range of fp32.)
    E = rel A + small,   tol = E + ulp_storage(|y| + E) / 2.

DEPTHWISE 3x3, stride 1, pad 1.  Output channel o reads input channel (o / grp) grp_stride + grp_off + o % grp.  Reference:
conv_probe.conv_reference's z, y, S with groups = C on the gathered channels, weights rounded to storage first, K = 9.  The kernel
adds nine fp32 products (exact: two 16-bit factors) in tap order and the bias: 10 adds, inside conv_probe's (K + 4) u S.  Its SiLU is
v * (1.0f / (1.0f + __expf(-v))): the negation is exact, the product with log2 e |z| u, v_exp_f32 2 u, the add 1 u, the IEEE
division 1 u, the product 1 u: (5 + |z|) u |y|, inside conv_error's (8 + 2 |z|) u |y| -- conv_error's SiLU term covers the
statement.  Without a residual: conv_tolerance.  With one, added after the activation in fp32 and rounded once (the E_res form of
op_step.StepChecker.conv):  y = silu(z) + r,  E_res = E + u |y|,  tol = E_res + ulp_storage(|y| + E_res) / 2.

TTA INPUT.  Reference: the oracle's scale_img (oracle/yolov5.py forward_augment) in float64: the batch flipped left to right
(pass 1), resized bilinearly, align_corners=False, to (sh, sw) = (int(h s), int(w s)), padded right and bottom with
round_storage(0.447) to the stride multiple.  TtaReference restates the interpolation (source coordinate
f = max(r (d + 0.5) - 0.5, 0), r = h / sh; the two neighbours, the second clamped to the last one) so that it can return the
terms of the bound with it; test_kernel_elements_cpu.py holds it against torch.nn.functional.interpolate in float64.
    blend       v = ly0 (lx0 p00 + lx1 p01) + ly1 (lx0 p10 + lx1 p11) in fp32 without contraction: every p passes two products and
                two adds, its weights lx0 = 1 - lx1 and ly0 = 1 - ly1 one rounding each: 6 u, taken as  8 u sum |weight p|.
    coordinate  the kernel forms f in fp32: r = (float) h / (float) sh (1 u), the product (1 u), - 0.5 (1 u), of a value below
                max(h, w): |df| <= 3 u max(h, w), taken as delta = 4 u max(h, w).  f - floor(f) is exact.  The interpolant is
                continuous and piecewise linear in f, also where floor(f) changes, with a slope of at most the difference of two
                neighbours: delta D, D the largest difference between horizontal or vertical neighbours in the window of the four
                source pixels widened by one pixel.
    rounding    tol = E + ulp_storage(|v| + E) / 2,   E = 8 u sum |weight p| + delta D.
The pad elements must be bit-exact.  Both scales are below 1: f <= h - 1 - (r - 1) / 2 < h - 1, the second neighbour's clamp is
never taken (TtaReference keeps the largest first neighbour so that a test can say so).  For the same reason no case is without
pad: int(h s) is a multiple of the stride only where h s is one exactly.  A forward takes multiples of the model's stride, so of the
shapes (64, 64), (96, 160), (128, 192), (192, 320) a stride-64 model runs three; a stride-32 model runs all four (TTA_CASES).

What the forms above leave out, so that nobody takes them for more than they are: log2 e as an fp32 is 0.22 u off, which adds
0.22 |x| u to an exponential's argument; the attention's argument term is counted once where the (v_j - y) form would allow it
twice; the TTA coordinate term takes one axis at its worst, not both.  Each is small against the term beside it at the shapes
tested (u_st is 8192 u and more; D is taken over a window wider than the four pixels), and the float32 restatements, which make
every one of these roundings, stay inside the bounds at every case; a kernel that does not is to be read against its statements
before a constant is touched.
"""

import numpy as np
import torch
import torch.nn.functional as F

from conv_probe import U32, MANT, Verdict, round_storage, ulp_storage, conv_error, conv_tolerance

KD, HD = 32, 64                        # key and value channels of a head
HEAD_CH = 2 * KD + HD
SCALE = float(np.float32(32.0 ** -0.5))          # launch_attention hands the kernel this fp32
ATTN_C1, ATTN_C2 = 8, 12
SMALL_P = 2.0 ** -14                   # the smallest normal of fp16
PAD_VALUE = 0.447
TTA_SCALES = {1: 0.83, 2: 0.67}
TTA_FLIPS = {1: True, 2: False}
#: the K order of the P V product: k index 8 g + j of lane group g holds key 4 g + j (j < 4) or 16 + 4 g + j - 4 of the step
MFMA_KEY_ORDER = np.array([(4 * g + j) if j < 4 else (16 + 4 * g + j - 4) for g in range(4) for j in range(8)])


def u_storage(dtype):
    return 2.0 ** -(MANT[dtype] + 1)


# ---- attention ----------------------------------------------------------------------------------------------------------------

class AttentionReference:
    """y, tol (n, N, heads * 64) float64 of stored qkv (n, N, heads * 128), and what the inputs exercise:
    small (n, N, heads * 64)  the fp16 small-P term (computed for both storage types, added to the bound for fp16 only),
    max_rises                 the largest number of 32-key steps in which a query's running maximum rises,
    s_min, s_max              the extreme scores,   x_max  the largest |s - m|."""

    def __init__(self, qkv, heads, dtype):
        qkv = np.asarray(qkv, dtype=np.float64)
        n, N, ch = qkv.shape
        assert ch == heads * HEAD_CH, (qkv.shape, heads)
        t = qkv.reshape(n, N, heads, HEAD_CH).transpose(0, 2, 1, 3)           # (n, heads, N, 128)
        q, k, v = t[..., :KD], t[..., KD:2 * KD], t[..., 2 * KD:]
        steps = -(-N // 32)
        y = np.empty((n, heads, N, HD))
        tol = np.empty_like(y)
        small = np.empty_like(y)
        self.max_rises, self.s_min, self.s_max, self.x_max = 0, np.inf, -np.inf, 0.0
        for i in range(n):
            for hd in range(heads):
                s = (q[i, hd] @ k[i, hd].T) * SCALE                           # (query, key)
                ds = 40 * U32 * (np.abs(q[i, hd]) @ np.abs(k[i, hd]).T) * SCALE
                m = s.max(axis=1, keepdims=True)
                p = np.exp(s - m)
                l = p.sum(axis=1, keepdims=True)
                av = np.abs(v[i, hd])
                y[i, hd] = (p @ v[i, hd]) / l
                A = (p @ av) / l
                small[i, hd] = (np.where(p < SMALL_P, p, 0.0) @ av) / l
                x = np.abs(s - m).max(axis=1, keepdims=True)
                rel = u_storage(dtype) + (ATTN_C1 * steps + N + ATTN_C2) * U32 + (4 + 2 * x) * U32 + 2 * ds.max(axis=1, keepdims=True)
                E = rel * A + (small[i, hd] if dtype == 'fp16' else 0.0)
                tol[i, hd] = E + 0.5 * ulp_storage(np.abs(y[i, hd]) + E, dtype)
                pad = np.full((N, steps * 32 - N), -np.inf)
                run = np.maximum.accumulate(np.concatenate([s, pad], axis=1).reshape(N, steps, 32).max(axis=2), axis=1)
                self.max_rises = max(self.max_rises, int((np.diff(run, axis=1) > 0).sum(axis=1).max()) if steps > 1 else 0)
                self.s_min, self.s_max = min(self.s_min, float(s.min())), max(self.s_max, float(s.max()))
                self.x_max = max(self.x_max, float(x.max()))

        def back(a):
            return np.ascontiguousarray(a.transpose(0, 2, 1, 3)).reshape(n, N, heads * HD)
        self.y, self.tol, self.small = back(y), back(tol), back(small)
        self.n, self.N, self.heads, self.dtype = n, N, heads, dtype

    def verdict(self, what, got):
        return Verdict(what, KD, np.asarray(got).reshape(self.y.shape), self.y, self.tol)


def norm_wise(got, want):
    """the figures of the bars these checks replace: (max |d| / max |ref|, mean |d| / mean |ref|)"""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float(d.max() / max(np.abs(want).max(), 1e-30)), float(d.mean() / max(np.abs(want).mean(), 1e-30))


ATTN_CLASSES = ('gauss075', 'gauss15', 'negative', 'ramp', 'large')
#: tokens: one key; around one 16-query block and one 32-key step; 48: the second score MFMA of the last step fully masked; many steps
ATTN_TOKENS = (1, 15, 16, 17, 31, 32, 33, 48, 300, 1000)
ATTN_HEADS = (1, 4)
ATTN_IMAGES = 2


def attention_input(cls, n, N, heads, dtype, seed=0):
    """stored qkv (n, N, heads * 128) float32 of an input class:
    gauss075  Gaussian times 0.75: no P below the fp16 normal range
    gauss15   Gaussian times 1.5: the small-P term is live
    negative  q = 0.3 + 0.9 |g| > 0, k = -(0.3 + 0.9 |g|) < 0: every score is negative, a key left at zero would win
    ramp      keys grow with their index: a query that agrees with them sees its running maximum rise in every 32-key step
    large     |q|, |k| near 4.2 with random signs: scores reach about +-100, exp(s) overflows without the maximum"""
    rng = np.random.default_rng([seed, N, heads, ATTN_CLASSES.index(cls)])
    g = rng.standard_normal((n, N, heads, HEAD_CH))
    if cls == 'gauss075':
        x = 0.75 * g
    elif cls == 'gauss15':
        x = 1.5 * g
    elif cls == 'negative':
        x = g.copy()
        x[..., :KD] = 0.3 + 0.9 * np.abs(g[..., :KD])
        x[..., KD:2 * KD] = -(0.3 + 0.9 * np.abs(g[..., KD:2 * KD]))
    elif cls == 'ramp':
        x = g.copy()
        ramp = (0.2 + 1.8 * (np.arange(N) + 1.0) / N).reshape(1, N, 1, 1)
        x[..., :KD] = 0.5 + 0.1 * g[..., :KD]                       # queries along (1, .., 1)
        x[..., KD:2 * KD] = ramp * (1.0 + 0.05 * g[..., KD:2 * KD])  # keys along it too, longer and longer
    elif cls == 'large':
        x = g.copy()
        sign = np.where(rng.random((n, N, heads, 1)) < 0.5, -1.0, 1.0)
        base = np.where(rng.random((1, 1, heads, KD)) < 0.5, -1.0, 1.0)          # one direction a head: q, k = +- 4.2 of it
        x[..., :KD] = sign * base * (4.2 + 0.05 * g[..., :KD])
        sign_k = np.where(rng.random((n, N, heads, 1)) < 0.5, -1.0, 1.0)
        x[..., KD:2 * KD] = sign_k * base * (4.2 + 0.05 * g[..., KD:2 * KD])
    else:
        raise ValueError(cls)
    return round_storage(x.reshape(n, N, heads * HEAD_CH), dtype)


def assert_attention_class(cls, ref):
    """the property an input class is in the set for, on the reference (both test files call it)"""
    steps = -(-ref.N // 32)
    if cls == 'gauss075':
        assert ref.small.max() == 0.0, 'a P below 2^-14: the small-P term is live'
    elif cls == 'gauss15' and ref.N >= 32:
        assert ref.small.max() > 0.0, 'no P below 2^-14'
    elif cls == 'negative':
        assert ref.s_max < 0.0
    elif cls == 'ramp':
        assert ref.max_rises == steps - 1, (ref.max_rises, steps)
        if ref.N >= 300:
            assert ref.max_rises > 1
    elif cls == 'large' and ref.N >= 15:
        assert ref.s_max > 88.8 and ref.s_min < -88.8, 'exp(s) does not overflow fp32'     # log(FLT_MAX) = 88.72


ATTN_MUTANTS = ('padded_key_scores_0', 'no_rescale_of_o', 'alpha_of_wrong_query', 'scale_of_key_dim_64', 'tail_query_rows_stored',
                'v_in_natural_key_order')


def emulated_attention(qkv, heads, dtype, mutant=None):
    """a float32 restatement of attn_kernel: 32 keys a step, the online softmax in float32, l from the unrounded exponentials,
    P rounded to storage for P V, V rows in the MFMA's key order; one rounding of O / l.  Returns (n, N, heads * 64) float32."""
    assert mutant is None or mutant in ATTN_MUTANTS
    qkv = np.asarray(qkv, dtype=np.float32)
    n, N, _ = qkv.shape
    t = qkv.reshape(n, N, heads, HEAD_CH)
    scale = np.float32(64.0 ** -0.5) if mutant == 'scale_of_key_dim_64' else np.float32(SCALE)
    rows = -(-N // 16) * 16                                                    # the queries of the last block run on zeros
    out = np.zeros((n * N + 16, heads * HD), dtype=np.float32)
    tails = []
    for i in range(n):
        for hd in range(heads):
            q = np.zeros((rows, KD), dtype=np.float32)
            q[:N] = t[i, :, hd, :KD]
            k, v = t[i, :, hd, KD:2 * KD], t[i, :, hd, 2 * KD:]
            m = np.full((rows, 1), -np.inf, dtype=np.float32)
            l = np.zeros((rows, 1), dtype=np.float32)
            O = np.zeros((rows, HD), dtype=np.float32)
            for k0 in range(0, N, 32):
                kb = np.zeros((32, KD), dtype=np.float32)
                vb = np.zeros((32, HD), dtype=np.float32)
                live = min(32, N - k0)
                kb[:live], vb[:live] = k[k0:k0 + live], v[k0:k0 + live]
                s = (q @ kb.T) * scale
                masked = live + (1 if mutant == 'padded_key_scores_0' else 0)
                s[:, masked:] = -np.inf
                m_new = np.maximum(m, s.max(axis=1, keepdims=True))
                with np.errstate(invalid='ignore'):
                    alpha = np.exp(m - m_new)                                  # exp(-inf) = 0 in the first step
                    e = np.exp(s - m_new)
                l = l * alpha + e[:, MFMA_KEY_ORDER].sum(axis=1, keepdims=True, dtype=np.float32)
                m = m_new
                P = round_storage(e, dtype)[:, MFMA_KEY_ORDER]
                a_o = alpha
                if mutant == 'no_rescale_of_o':
                    a_o = np.ones_like(alpha)
                elif mutant == 'alpha_of_wrong_query':                         # lane 4 g + r + 1 asked instead of 4 g + r
                    a_o = np.roll(alpha.reshape(-1, 16), -1, axis=1).reshape(-1, 1)
                vk = vb if mutant == 'v_in_natural_key_order' else vb[MFMA_KEY_ORDER]
                O = O * a_o + P @ vk
            y = round_storage(O / l, dtype)
            out[i * N:(i + 1) * N, hd * HD:(hd + 1) * HD] = y[:N]
            tails.append((i * N + N, hd, y[N:]))
    if mutant == 'tail_query_rows_stored':              # the blocks of all images run side by side: the tail rows land on the
        for row, hd, y in tails:                        # first rows of the next image (behind the buffer for the last one)
            out[row:row + y.shape[0], hd * HD:(hd + 1) * HD] = y
    return out[:n * N].reshape(n, N, heads * HD)


# ---- depthwise 3x3 ------------------------------------------------------------------------------------------------------------

def dw_channels(c, grp, grp_stride, grp_off):
    o = np.arange(c)
    return (o // grp) * grp_stride + grp_off + o % grp


def depthwise_reference(a, w, b, r, grp, grp_stride, grp_off, act, dtype):
    """a (n, c_in, h, w) stored values, w (c, 1, 3, 3) ALREADY rounded to storage, b (c,) fp32, r (n, c, h, w) stored values or
    None -> (y, tol) float64"""
    c = w.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)[:, dw_channels(c, grp, grp_stride, grp_off)]))
    w64 = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
    b64 = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64))
    z = F.conv2d(x, w64, b64, padding=1, groups=c)
    S = F.conv2d(x.abs(), w64.abs(), b64.abs(), padding=1, groups=c).numpy()
    y = (z * torch.sigmoid(z) if act else z).numpy()
    z = z.numpy()
    if r is None:
        return y, conv_tolerance(y, z, S, 9, dtype)
    E = conv_error(y, z, S, 9)
    y = y + np.asarray(r, dtype=np.float64)
    E = E + U32 * np.abs(y)
    return y, E + 0.5 * ulp_storage(np.abs(y) + E, dtype)


def depthwise_verdict(what, got, a, w, b, r, grp, grp_stride, grp_off, act, dtype):
    y, tol = depthwise_reference(a, w, b, r, grp, grp_stride, grp_off, act, dtype)
    return Verdict(what, 9, got, y, tol)


#: (name, c, ld_in, grp, grp_stride, grp_off): plain at three widths, plain inside a wider pixel, the pe mapping of four heads
#: (the v slices of a qkv tensor; 32 threads a pixel: the (2, 2) and (15, 20) maps fill their 256-thread blocks exactly)
DW_MAPPINGS = [('c8', 8, 8, 8, 8, 0), ('c24', 24, 24, 24, 24, 0), ('c64', 64, 64, 64, 64, 0), ('c24_ld40', 24, 40, 24, 24, 0),
               ('pe4', 256, 512, 64, 128, 64)]
DW_MAPS = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 9), (15, 20)]
DW_IMAGES = 2


def depthwise_case(hw, mapping, dtype, seed=0):
    """(a (n, ld_in, h, w), w (c, 1, 3, 3) fp32, b (c,), r (n, c, h, w)): smooth maps under noise -- neighbouring pixels are alike,
    so a tap taken from the wrong side or dropped at a border moves the sum --, the second image near zero"""
    _, c, ld_in, _, _, _ = mapping
    h, wd = hw
    rng = np.random.default_rng([seed, h, wd, c, ld_in])
    ys, xs = np.mgrid[0:h, 0:wd].astype(np.float64)
    ch = np.arange(ld_in).reshape(1, ld_in, 1, 1)
    a = np.empty((DW_IMAGES, ld_in, h, wd))
    for i in range(DW_IMAGES):
        a[i] = 1.5 * np.sin(xs / (3.0 + i) + 0.7 * ch[0] + i) * np.cos(ys / (2.5 + i) + 0.3 * ch[0]) + 0.4 + 0.15 * rng.standard_normal((ld_in, h, wd))
    a[1] /= 64
    w = rng.standard_normal((c, 1, 3, 3)) / 3 + 0.25 * np.sign(rng.standard_normal((c, 1, 1, 1)))
    b = 0.3 * rng.standard_normal(c) + 0.05 * np.arange(c)                    # every channel its own bias
    r = 0.8 * rng.standard_normal((DW_IMAGES, c, h, wd))
    r[1] /= 64
    return round_storage(a, dtype), w.astype(np.float32), b.astype(np.float32), round_storage(r, dtype)


def dw_threads(hw, mapping):
    return DW_IMAGES * hw[0] * hw[1] * mapping[1] // 8


DW_MUTANTS = ('taps_transposed', 'left_border_skips_the_right_tap', 'residual_added_before_silu', 'residual_rounded_first',
              'grp_off_ignored', 'bias_of_the_next_channel_group')


def emulated_depthwise(a, w, b, r, grp, grp_stride, grp_off, act, dtype, mutant=None):
    """a float32 restatement of dwconv3x3_kernel: nine fp32 taps in order, bias, SiLU, residual, one rounding.  `w` fp32."""
    assert mutant is None or mutant in DW_MUTANTS
    c = w.shape[0]
    n, _, h, wd = a.shape
    x = np.asarray(a, dtype=np.float32)[:, dw_channels(c, grp, grp_stride, 0 if mutant == 'grp_off_ignored' else grp_off)]
    ws = round_storage(w, dtype).reshape(c, 3, 3)
    if mutant == 'taps_transposed':
        ws = ws.transpose(0, 2, 1)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    acc = np.zeros((n, c, h, wd), dtype=np.float32)
    for rr in range(3):
        for ss in range(3):
            tap = xp[:, :, rr:rr + h, ss:ss + wd] * ws[:, rr, ss].reshape(1, c, 1, 1)
            if mutant == 'left_border_skips_the_right_tap' and ss == 2:
                tap = tap.copy()
                tap[..., 0] = 0                                  # in the first column the tap at x + 1 goes instead of x - 1
            acc = acc + tap
    bias = np.roll(b, -8) if mutant == 'bias_of_the_next_channel_group' else b
    v = acc + np.asarray(bias, dtype=np.float32).reshape(1, c, 1, 1)
    silu = (lambda t: t * (np.float32(1) / (np.float32(1) + np.exp(-t)))) if act else (lambda t: t)
    if r is None:
        return round_storage(silu(v), dtype)
    r = np.asarray(r, dtype=np.float32)
    if mutant == 'residual_added_before_silu':
        return round_storage(silu(v + r), dtype)
    if mutant == 'residual_rounded_first':
        return round_storage(round_storage(silu(v), dtype) + r, dtype)
    return round_storage(r + silu(v), dtype)


# ---- the TTA input ------------------------------------------------------------------------------------------------------------

TTA_SHAPES = [(64, 64), (96, 160), (128, 192), (192, 320)]
TTA_STRIDE = 64
#: (model stride, (h, w)): a forward takes multiples of the model's stride only, so the stride-64 model runs three of the four
#: shapes; a stride-32 model runs all four (and pads to multiples of 32: other pad widths for the same resized images)
TTA_CASES = [(64, hw) for hw in TTA_SHAPES if hw[0] % 64 == 0 and hw[1] % 64 == 0] + [(32, hw) for hw in TTA_SHAPES]


def tta_geometry(h, w, tta_pass, stride=TTA_STRIDE):
    """(sh, sw, oh, ow, flip) of scaled pass 1 or 2, as scale_img computes them"""
    import math
    s = TTA_SCALES[tta_pass]
    return int(h * s), int(w * s), math.ceil(h * s / stride) * stride, math.ceil(w * s / stride) * stride, TTA_FLIPS[tta_pass]


def _axis(size, out, dtype=np.float64):
    """source coordinates of `out` destination pixels on an axis of `size`: (first neighbour, second, weight of the second)"""
    d = np.arange(out, dtype=dtype)
    f = np.maximum(dtype(size) / dtype(out) * (d + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.floor(f).astype(np.int64)
    i1 = i0 + (i0 < size - 1)
    return i0, i1, f - i0.astype(dtype)


class TtaReference:
    """y, tol (n, 3, oh, ow) float64 of the stored batch x (n, 3, h, w); inside: the mask of the elements that are not pad;
    max_y0, max_x0: the largest first neighbours (the clamp of the second is taken only at h - 1, w - 1)"""

    def __init__(self, x, tta_pass, dtype, stride=TTA_STRIDE):
        x = np.asarray(x, dtype=np.float64)
        n, _, h, w = x.shape
        sh, sw, oh, ow, flip = tta_geometry(h, w, tta_pass, stride)
        src = x[..., ::-1] if flip else x
        y0, y1, ly = _axis(h, sh)
        x0, x1, lx = _axis(w, sw)
        self.max_y0, self.max_x0 = int(y0.max()), int(x0.max())
        ly, lx = ly.reshape(sh, 1), lx.reshape(1, sw)
        parts = [((1 - ly) * (1 - lx), src[:, :, y0][:, :, :, x0]), ((1 - ly) * lx, src[:, :, y0][:, :, :, x1]),
                 (ly * (1 - lx), src[:, :, y1][:, :, :, x0]), (ly * lx, src[:, :, y1][:, :, :, x1])]
        v = sum(wt * p for wt, p in parts)
        mag = sum(np.abs(wt * p) for wt, p in parts)
        # the largest neighbour difference in rows y0 - 1 .. y0 + 2, columns x0 - 1 .. x0 + 2 (clamped): a running maximum of
        # the difference maps over that window
        dx = np.abs(np.diff(src, axis=3))                                      # between columns j, j + 1
        dy = np.abs(np.diff(src, axis=2))
        D = np.zeros((n, 3, sh, sw))
        rows = [np.clip(y0 + k, 0, h - 1) for k in (-1, 0, 1, 2)]
        cols = [np.clip(x0 + k, 0, w - 1) for k in (-1, 0, 1, 2)]
        for ra in rows:
            for k in range(3):                                                 # column pairs (x0 - 1 + k, x0 + k)
                j = np.clip(x0 - 1 + k, 0, w - 2)
                D = np.maximum(D, dx[:, :, ra][:, :, :, j])
        for ca in cols:
            for k in range(3):
                i = np.clip(y0 - 1 + k, 0, h - 2)
                D = np.maximum(D, dy[:, :, i][:, :, :, ca])
        E = 8 * U32 * mag + 4 * U32 * max(h, w) * D
        pad = float(round_storage(np.array([PAD_VALUE]), dtype)[0])
        self.y = np.full((n, 3, oh, ow), pad)
        self.tol = np.zeros((n, 3, oh, ow))
        self.inside = np.zeros((n, 3, oh, ow), dtype=bool)
        self.y[:, :, :sh, :sw] = v
        self.tol[:, :, :sh, :sw] = E + 0.5 * ulp_storage(np.abs(v) + E, dtype)
        self.inside[:, :, :sh, :sw] = True
        self.geometry = (sh, sw, oh, ow, flip)

    def verdicts(self, what, got):
        """(the resized part against its bound, the pad bit for bit)"""
        from op_step import Exact
        got = np.asarray(got, dtype=np.float32)
        assert got.shape == self.y.shape, (what, got.shape, self.y.shape)
        sh, sw = self.geometry[:2]
        inner = Verdict(what + ' resized', 4, got[:, :, :sh, :sw], self.y[:, :, :sh, :sw], self.tol[:, :, :sh, :sw])
        outer = ~self.inside
        return inner, Exact(what + ' pad', got[outer], self.y[outer].astype(np.float32))


def torch_scale_img(x, tta_pass, dtype, stride=TTA_STRIDE):
    """scale_img as the oracle writes it, in float64 (the second source of TtaReference.y)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    h, w = t.shape[2:]
    sh, sw, oh, ow, flip = tta_geometry(h, w, tta_pass, stride)
    t = t.flip(3) if flip else t
    t = F.interpolate(t, size=(sh, sw), mode='bilinear', align_corners=False)
    return F.pad(t, [0, ow - sw, 0, oh - sh], value=float(round_storage(np.array([PAD_VALUE]), dtype)[0])).numpy()


def tta_images(n, h, w, seed=0):
    """HWC uint8: a left-to-right brightness ramp and a bright bar in the left third under smooth structure and noise (a flip of
    the wrong thing shows), the rows different from one another"""
    rng = np.random.default_rng([seed, h, w])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(n):
        base = 40 + 150 * xs / w + 40 * np.sin(xs / (5.0 + i) + ys / 9.0)
        base = base[..., None] + 25 * np.cos(ys[..., None] / (4.0 + i) + 2 * np.arange(3))
        base[:, w // 5:w // 5 + max(2, w // 16)] += 60
        out.append(np.clip(np.rint(base + rng.normal(0, 10, (h, w, 3))), 0, 255).astype(np.uint8))
    return out


def tta_input_tensor(imgs, dtype):
    """the stored network input of those images: / 255, CHW, rounded to storage"""
    return round_storage(np.stack([im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in imgs]), dtype)


TTA_MUTANTS = ('pad_value_0.5', 'no_half_pixel_offset', 'destination_flipped', 'second_row_not_clamped')


def emulated_tta(x, tta_pass, dtype, stride=TTA_STRIDE, mutant=None):
    """a float32 restatement of tta_scale_kernel on the stored batch x (n, 3, h, w): fp32 coordinates and blend"""
    assert mutant is None or mutant in TTA_MUTANTS
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    n, _, h, w = x.shape
    sh, sw, oh, ow, flip = tta_geometry(h, w, tta_pass, stride)

    def axis(size, out):
        d = np.arange(out, dtype=f32)
        r = f32(size) / f32(out)
        f = r * d if mutant == 'no_half_pixel_offset' else r * (d + f32(0.5)) - f32(0.5)
        f = np.maximum(f, f32(0))
        i0 = f.astype(np.int64)
        return i0, i0 + (i0 < size - 1), (f - i0.astype(f32)).astype(f32)

    y0, y1, ly1 = axis(h, sh)
    x0, x1, lx1 = axis(w, sw)
    if mutant == 'second_row_not_clamped':               # row h of an image is row 0 of the next one (zeros behind the last)
        y1 = y0 + 1
        x = np.concatenate([x, np.concatenate([x[1:, :, :1], np.zeros_like(x[:1, :, :1])], axis=0)], axis=2)
    flip_src = flip and mutant != 'destination_flipped'
    sx0, sx1 = (w - 1 - x0, w - 1 - x1) if flip_src else (x0, x1)
    ly1, lx1 = ly1.reshape(sh, 1), lx1.reshape(1, sw)
    ly0, lx0 = f32(1) - ly1, f32(1) - lx1
    p00, p01 = x[:, :, y0][:, :, :, sx0], x[:, :, y0][:, :, :, sx1]
    p10, p11 = x[:, :, y1][:, :, :, sx0], x[:, :, y1][:, :, :, sx1]
    v = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)
    out = np.full((n, 3, oh, ow), f32(0.5 if mutant == 'pad_value_0.5' else PAD_VALUE), dtype=f32)
    out[:, :, :sh, :sw] = v
    if flip and mutant == 'destination_flipped':          # the whole padded row is mirrored: the pad ends up on the left
        out = out[..., ::-1]
    return round_storage(out, dtype)
