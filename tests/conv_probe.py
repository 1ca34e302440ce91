"""
Probe networks: small YOLOv5-style yamls in which every layer is ONE conv op of a chosen shape, so that a test can compare
each conv of the library with a float64 evaluation of that one op on the input the op really read -- element by element,
with a bound derived from the arithmetic and not from a run.  (tests/test_conv_probe_cpu.py checks this file without a GPU;
tests/test_gpu_conv_probe.py runs the library through it; profiles/conv_probe_tests.txt holds the figures.)

A `source` below is anything with  input() -> (n, 3, h, w),  layer(i) -> (n, c, h, w)  and  predictions() -> (n, A, 5 + nc),
all float32 and all holding exactly what is stored: HipSource reads a HipContext, Emulated is a float32 restatement with
planted mistakes for the CPU tests.

The reference of one conv op (conv_reference): torch.nn.functional.conv2d in float64 on
    a  the producer's stored output (the stored network input for the stem),
    w  the fp32 weights rounded to the storage type (round to nearest even, as the packer does),  b  the fp32 bias:
    z = conv(a, w) + b,   y = z * sigmoid(z),   S = conv(|a|, |w|) + |b|.

The bound (conv_tolerance), u = 2^-24, K = c_in * kh * kw:
    fp32 accumulation in any order            |z^ - z| <= (K + 4) u S
    SiLU: slope within [-0.1, 1.1]; its five instructions (mul by -log2 e, v_exp_f32, add, v_rcp_f32, mul) round to <= 1 ulp
    each, the rounded exponent argument costs a relative |z| u:
                                              E = 1.1 (K + 4) u S + (8 + 2 |z|) u |y|
    one rounding to the storage type          tol = E + ulp_storage(|y| + E) / 2
(7 mantissa bits for bf16, 10 for fp16; below the smallest normal of the storage type its ulp there.)  Every element is
held to it.  The constants are derived; they are not widened for a run.
"""

import hashlib

import numpy as np
import torch
import torch.nn.functional as F

from megadetector_amd.yolo_model import MDHIP_CONV, MDHIP_UPSAMPLE, MDHIP_CONCAT, MDHIP_DETECT

U32 = 2.0 ** -24                               # unit roundoff of fp32
MANT = {'bf16': 7, 'fp16': 10}                 # stored mantissa bits
MIN_EXP = {'bf16': -126, 'fp16': -14}          # exponent of the smallest normal
TORCH_DTYPE = {'bf16': torch.bfloat16, 'fp16': torch.float16}
SHARP_K = 200                                  # up to this K the accumulation term leaves the storage rounding visible

_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]


def _yaml(rows, levels):
    return {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'anchors': [list(a) for a in _ANCHORS[:len(levels)]],
            'backbone': [list(r) for r in rows], 'head': [[list(levels), 1, 'Detect', ['nc', 'anchors']]]}


# network A ("wide"): 3 images of 24 x 320; maps 12 x 160, 6 x 80, 3 x 40
NET_A = _yaml([
    [-1, 1, 'Conv', [80, 6, 2, 2]],             # 0  6x6 stem, N = 80: stem: family
    [-1, 1, 'Conv', [80, 3, 1]],                # 1  80 -> 80 3x3, W % 80 == 0: v5:strip, v5:run aligned, half-full last group
    [-1, 1, 'Conv', [128, 1, 1]],               # 2  1x1, C = 80 (no whole 64-slabs), N = 128
    [-1, 1, 'Conv', [160, 3, 2]],               # 3  stride 2, C = 128, Wo = 80: v7 aligned, no tail
    [1, 1, 'Conv', [160, 3, 2]],                # 4  stride 2, C = 80, Wo = 80: v7 aligned, tail; writes a concat slice
    [[3, 4], 1, 'Concat', [1]],                 # 5
    [-1, 1, 'Conv', [320, 3, 1]],               # 6  320 -> 320 on 6 x 80: the 8-wave tiles; M = 1440; Detect level 0
    [-1, 1, 'Conv', [64, 1, 1]],                # 7  1x1 on whole slabs, K = 320: the /a3 ring
    [-1, 1, 'Conv', [160, 3, 2]],               # 8  stride 2, C = 64, Wo = 40: v7 unaligned, no tail
    [6, 1, 'Conv', [160, 3, 2]],                # 9  stride 2, C = 320, Wo = 40, M = 360: three images in one tile
    [6, 1, 'Conv', [72, 1, 1]],                 # 10 N = 72
    [-1, 1, 'Conv', [160, 3, 2]],               # 11 stride 2, C = 72: v7 unaligned, tail
    [[8, 9, 11], 1, 'Concat', [1]],             # 12 Detect level 1 (K = 480)
], [6, 12])

# network B ("odd"): 3 images of 72 x 104; maps 36 x 52, 18 x 26, 9 x 13
NET_B = _yaml([
    [-1, 1, 'Conv', [32, 3, 2, 1]],             # 0  3x3 stem (k_real = 27)
    [-1, 1, 'Conv', [64, 3, 2]],                # 1  stride 2, C = 32 (below one slab)
    [-1, 1, 'Conv', [72, 1, 1]],                # 2  small K: the rounding is checked sharply
    [-1, 1, 'Conv', [200, 3, 1]],               # 3  C = 72, N = 200 (N tail on every tile width), W = 26
    [-1, 1, 'Conv', [24, 3, 1]],                # 4  N = 24; writes the concat slice at channel 0
    [3, 1, 'Conv', [40, 1, 1]],                 # 5  writes the concat slice at channel 24
    [[4, 5], 1, 'Concat', [1]],                 # 6  Detect level 0
    [-1, 1, 'Conv', [160, 3, 2]],               # 7  stride 2 down to the odd map 9 x 13
    [-1, 1, 'Conv', [640, 3, 1]],               # 8  M = 351, three images inside one tile
    [-1, 1, 'Conv', [640, 3, 1]],               # 9  K = 5760, the largest the shipped models have
    [-1, 1, 'Conv', [8, 1, 1]],                 # 10 N = 8, Detect level 2 (its Detect conv has K = 8)
    [9, 1, 'nn.Upsample', [None, 2, 'nearest']],  # 11
    [[-1, 3], 1, 'Concat', [1]],                # 12 840 channels
    [-1, 1, 'Conv', [48, 1, 1]],                # 13 reader of the upsample, Detect level 1
], [6, 13, 10])

#: name -> yaml, the forward's (images, h, w), the context's capacity (mdhip_create wants max_h, max_w >= 64)
NETS = {
    'A': dict(yaml=NET_A, shape=(3, 24, 320), capacity=(3, 64, 320)),
    'B': dict(yaml=NET_B, shape=(3, 72, 104), capacity=(3, 72, 104)),
}
SEED = 5


def weights(net):
    from megadetector_amd import weights_io
    return weights_io.synthetic_weights(NETS[net]['yaml'], seed=SEED)


def images(net):
    """the input images of a network: HWC uint8, smooth structure with noise on it, one image nearly black (small values)"""
    n, h, w = NETS[net]['shape']
    rng = np.random.default_rng(100 + ord(net))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(n):
        base = 127 + 100 * np.sin(xs / (7.0 + 3 * i) + i)[..., None] * np.cos(ys[..., None] / (5.0 + i) + np.arange(3))
        img = base + rng.normal(0, 30, (h, w, 3))
        if i == 1:
            img = img / 16
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


# ---- number formats -----------------------------------------------------------------------------------------------------

def round_storage(x, dtype):
    """float32 values rounded to the storage type (nearest, ties to even), as float32"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(TORCH_DTYPE[dtype]).float().numpy()


def is_storage(x, dtype):
    """every value representable in the storage type (what read_layer promises)"""
    x = np.asarray(x, dtype=np.float32)
    return bool(np.array_equal(round_storage(x, dtype), x, equal_nan=True))


def ulp_storage(v, dtype):
    """spacing of the storage type at magnitude v >= 0 (float64 array); at and below the smallest normal the spacing there"""
    v = np.asarray(v, dtype=np.float64)
    _, e = np.frexp(v)                                   # v = m * 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    e = np.where(v < 2.0 ** MIN_EXP[dtype], MIN_EXP[dtype], e - 1)
    return np.ldexp(1.0, e - MANT[dtype])


def ulp_f32(v):
    v = np.asarray(v, dtype=np.float64)
    _, e = np.frexp(v)
    return np.ldexp(1.0, np.where(v < 2.0 ** -126, -126, e - 1) - 23)


# ---- one conv op in float64 ---------------------------------------------------------------------------------------------

def conv_reference(a, w, b, stride, pad, act=True):
    """a (n, c, h, w) stored values, w (o, c, kh, kw) ALREADY rounded to storage, b (o,) fp32 -> float64 (y, z, S)"""
    a64 = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    w64 = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
    b64 = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64))
    z = F.conv2d(a64, w64, b64, stride=stride, padding=pad)
    S = F.conv2d(a64.abs(), w64.abs(), b64.abs(), stride=stride, padding=pad)
    y = z * torch.sigmoid(z) if act else z
    return y.numpy(), z.numpy(), S.numpy()


def accumulation_bound(S, K):
    """|z^ - z| of an fp32 sum of K products and a bias in any order"""
    return (K + 4) * U32 * S


def conv_error(y, z, S, K):
    """E of the docstring: the fp32 value in front of the rounding to storage against y"""
    return 1.1 * accumulation_bound(S, K) + (8 + 2 * np.abs(z)) * U32 * np.abs(y)


def conv_tolerance(y, z, S, K, dtype):
    E = conv_error(y, z, S, K)
    return E + 0.5 * ulp_storage(np.abs(y) + E, dtype)


class Verdict:
    """one layer of one forward against its reference"""

    def __init__(self, what, K, got, y, tol):
        err = np.abs(np.asarray(got, dtype=np.float64) - y)
        with np.errstate(invalid='ignore'):
            ratio = err / tol
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)         # NaN or inf in the output: over every bound
        self.what, self.K, self.key = what, K, None          # key: the layer, or ('detect', level)
        self.over = int((ratio > 1).sum())
        self.size = ratio.size
        self.where = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
        self.worst = float(ratio[self.where])
        self.got, self.want = float(np.asarray(got)[self.where]), float(y[self.where])

    def __str__(self):
        index = '(image, channel, y, x)' if len(self.where) == 4 else '(image, anchor, column)'
        return '{}: K = {}, worst err / tol {:.3f} at {} = {} (got {!r}, reference {!r}), {} of {} over'.format(
            self.what, self.K, self.worst, index, self.where, self.got, self.want, self.over, self.size)


# ---- walking a probe network --------------------------------------------------------------------------------------------

def conv_layers(W):
    return [s.index for s in W.specs if s.type == MDHIP_CONV]


def stored_input(src, specs, layer):
    """what the consumer of `layer` reads, assembled from the stored outputs of the convs behind it: a Concat is its sources
    side by side, an Upsample its source repeated 2 x 2 (their own buffers are never read here: an upsample read in place
    leaves the first part of its concat buffer unwritten)"""
    if layer < 0:
        return src.input()
    s = specs[layer]
    if s.type == MDHIP_CONCAT:
        return np.concatenate([stored_input(src, specs, f) for f in s.frm], axis=1)
    if s.type == MDHIP_UPSAMPLE:
        return stored_input(src, specs, s.frm[0]).repeat(2, axis=2).repeat(2, axis=3)
    assert s.type == MDHIP_CONV, (layer, s.type)
    return src.layer(layer)


def detect_interval(z, delta, level, W):
    """float64 decode of one Detect level at z - delta and z + delta (every decoded quantity rises with its logit), widened
    by 8 fp32 ulps of the larger endpoint: (lo, hi) as (n, na * ny * nx, 5 + nc)"""
    n, _, ny, nx = z.shape
    na, no = W.na, W.nc + 5
    stride = float(W.strides[level])
    anchors = W.anchors_px[level].astype(np.float64).reshape(1, na, 1, 1, 2)
    gx = (np.arange(nx, dtype=np.float64) - 0.5).reshape(1, 1, 1, nx)
    gy = (np.arange(ny, dtype=np.float64) - 0.5).reshape(1, 1, ny, 1)

    def decode(v):
        s = np.exp(-np.logaddexp(0.0, -v.reshape(n, na, no, ny, nx)))         # the sigmoid, without overflow
        out = np.empty((n, na, ny, nx, no))
        out[..., 0] = (s[:, :, 0] * 2 + gx) * stride
        out[..., 1] = (s[:, :, 1] * 2 + gy) * stride
        out[..., 2:4] = (s[:, :, 2:4].transpose(0, 1, 3, 4, 2) * 2) ** 2 * anchors
        out[..., 4:] = s[:, :, 4:].transpose(0, 1, 3, 4, 2)
        return out.reshape(n, na * ny * nx, no)

    lo, hi = decode(z - delta), decode(z + delta)
    wide = 8 * ulp_f32(np.maximum(np.abs(lo), np.abs(hi)))
    return lo - wide, hi + wide


class Checker:
    """the references and bounds of one (network, storage type), cached by (layer, digest of the input bytes): forwards
    that only differ in tiles of one K order produce the same inputs, and the float64 work is done once"""

    def __init__(self, W, dtype):
        self.W, self.dtype = W, dtype
        self.specs = W.specs
        self.convs = conv_layers(W)
        self.detect = W.specs[-1]
        assert self.detect.type == MDHIP_DETECT
        self._w = {}
        self._cache = {}
        self.computed = 0

    def packed(self, name):
        """(weights rounded to storage, fp32 bias) of one conv"""
        if name not in self._w:
            self._w[name] = (round_storage(self.W.weights[name + '.weight'], self.dtype), self.W.weights[name + '.bias'])
        return self._w[name]

    def K(self, layer, level=None):
        w = self.W.weights[self.specs[layer].conv_names[level or 0] + '.weight']
        return int(w.shape[1] * w.shape[2] * w.shape[3])

    def _cached(self, key, a, make):
        key = key + (hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest(),)
        if key not in self._cache:
            self._cache[key] = make()
            self.computed += 1
        return self._cache[key]

    def reference(self, src, layer):
        """(y, tol) of a conv layer for the input it read in the source's forward"""
        s = self.specs[layer]
        a = stored_input(src, self.specs, s.frm[0])
        assert is_storage(a, self.dtype), ('layer', layer, 'reads values that are not of the storage type')

        def make():
            w, b = self.packed(s.conv_names[0])
            y, z, S = conv_reference(a, w, b, s.s, s.p)
            return y, conv_tolerance(y, z, S, self.K(layer), self.dtype)
        return self._cached((layer,), a, make)

    def check_layer(self, src, layer, what=''):
        y, tol = self.reference(src, layer)
        got = src.layer(layer)
        assert got.shape == y.shape, (what, layer, got.shape, y.shape)
        # (the same output for the same input was judged before: tiles of one K order)
        label = '{} layer {}'.format(what, layer).strip()
        v = self._cached(('verdict', layer, id(y)), got, lambda: Verdict(label, self.K(layer), got, y, tol))
        v.what, v.key = label, layer
        return v

    def check_detect(self, src, what=''):
        """the Detect convs (fp32 logits, no activation) through the decoded predictions: one Verdict per level, its
        `worst` the distance from the interval's middle in half widths"""
        pred = src.predictions()
        out, row = [], 0
        for level, f in enumerate(self.detect.frm):
            a = stored_input(src, self.specs, f)
            K = self.K(self.detect.index, level)

            def make():
                w, b = self.packed(self.detect.conv_names[level])
                _, z, S = conv_reference(a, w, b, 1, 0, act=False)
                return detect_interval(z, accumulation_bound(S, K), level, self.W)
            lo, hi = self._cached((self.detect.index, level), a, make)
            got = pred[:, row:row + lo.shape[1]]
            assert got.shape == lo.shape, (what, level, pred.shape, lo.shape)
            row += lo.shape[1]
            out.append(Verdict('{} Detect level {}'.format(what, level).strip(), K, got, (lo + hi) / 2, (hi - lo) / 2))
            out[-1].key = ('detect', level)
        assert row == pred.shape[1], (row, pred.shape)
        return out

    def check(self, src, what='', detect=True):
        """every conv layer and the Detect levels of one forward"""
        v = [self.check_layer(src, i, what) for i in self.convs]
        return v + (self.check_detect(src, what) if detect else [])


def failures(verdicts):
    return [str(v) for v in verdicts if v.over]


# ---- sources ------------------------------------------------------------------------------------------------------------

class HipSource:
    """the last forward of a HipContext"""

    def __init__(self, ctx, shape):
        self.ctx, self.shape = ctx, shape
        self._layers = {}

    def input(self):
        return self.ctx.read_input(*self.shape)

    def layer(self, i):
        if i not in self._layers:
            self._layers[i] = self.ctx.read_layer(i, self.shape[0])
        return self._layers[i]

    def predictions(self):
        return self.ctx.read_predictions(self.shape[0])


def conv_f32(a, w, b, stride, pad):
    return F.conv2d(a, w, b, stride=stride, padding=pad)


def conv_f32_blocks(a, w, b, stride, pad, block=32):
    """the same sum in another order: K in blocks of 32, the blocks from the last to the first, the bias at the end"""
    n, _, h, wd = a.shape
    o, _, kh, kw = w.shape
    cols = F.unfold(a, (kh, kw), padding=pad, stride=stride)              # (n, K, L)
    wk = w.reshape(o, -1)
    K = wk.shape[1]
    acc = torch.zeros((n, o, cols.shape[2]), dtype=torch.float32)
    for k0 in reversed(range(0, K, block)):
        acc = acc + torch.matmul(wk[:, k0:k0 + block], cols[:, k0:k0 + block])
    acc = acc + b.reshape(1, o, 1)
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    return acc.reshape(n, o, ho, wo)


MUTANTS = ('replicate_padding', 'rows_leak_between_images', 'last_8_input_channels_ignored', 'tap_dropped_in_first_column',
           'concat_slice_8_channels_off', 'n_tail_left_at_zero', 'truncating_store', 'bias_omitted', 'silu_is_identity')


class Emulated:
    """a float32 restatement of the forward of a probe network, standing in for a kernel: conv (torch float32) on the stored
    input and the storage-rounded weights, bias, SiLU, one rounding to storage.  `mutant` plants one mistake in every conv
    it applies to (MUTANTS); `conv` is the summation (conv_f32 or conv_f32_blocks)."""

    def __init__(self, W, dtype, x, conv=conv_f32, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.W, self.dtype, self.mutant, self.conv = W, dtype, mutant, conv
        self.specs = W.specs
        self.feeds_concat = {f for s in W.specs if s.type == MDHIP_CONCAT for f in s.frm}
        self._x = round_storage(x, dtype)
        self._out = {}
        with torch.no_grad():
            for s in W.specs:
                if s.type == MDHIP_CONV:
                    self._out[s.index] = self._conv_layer(s)
            self._pred = self._detect(W.specs[-1])

    def input(self):
        return self._x

    def layer(self, i):
        return self._out[i]

    def predictions(self):
        return self._pred

    def _store(self, v):
        if self.mutant == 'truncating_store':                   # toward zero: the low 16 bits of the fp32 cut off (bf16),
            if self.dtype == 'bf16':                            # the nearest fp16 of no larger magnitude (fp16)
                return (v.numpy().view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
            v = v.numpy()
            r = v.astype(np.float16)
            r = np.where(np.abs(r.astype(np.float32)) > np.abs(v), np.nextafter(r, np.float16(0)), r)
            return r.astype(np.float32)
        return v.to(TORCH_DTYPE[self.dtype]).float().numpy()

    def _sum(self, a, w, b, s):
        m = self.mutant
        k, pad = s.k, s.p
        if m == 'last_8_input_channels_ignored':
            w = w.clone()
            w[:, -8:] = 0
        if m == 'bias_omitted':
            b = torch.zeros_like(b)
        if m == 'replicate_padding' and pad:
            return self.conv(F.pad(a, (pad,) * 4, mode='replicate'), w, b, s.s, 0)
        if m == 'rows_leak_between_images' and pad:
            # the batch as one tall image: the rows above an image's first are the previous image's last
            n, c, h, wd = a.shape
            tall = a.permute(1, 0, 2, 3).reshape(1, c, n * h, wd)
            z = self.conv(tall, w, b, s.s, pad)
            return z.reshape(z.shape[1], n, z.shape[2] // n, z.shape[3]).permute(1, 0, 2, 3).contiguous()
        z = self.conv(a, w, b, s.s, pad)
        if m == 'tap_dropped_in_first_column' and k > 1:
            w2 = w.clone()
            w2[:, :, k // 2, k // 2] = 0
            z = z.clone()
            z[..., 0] = self.conv(a, w2, b, s.s, pad)[..., 0]
        return z

    def _conv_layer(self, s):
        a = torch.from_numpy(stored_input(self, self.specs, s.frm[0]))
        w = torch.from_numpy(round_storage(self.W.weights[s.conv_names[0] + '.weight'], self.dtype))
        b = torch.from_numpy(self.W.weights[s.conv_names[0] + '.bias'])
        z = self._sum(a, w, b, s)
        y = z if self.mutant == 'silu_is_identity' else z * torch.sigmoid(z)
        out = self._store(y)
        if self.mutant == 'n_tail_left_at_zero' and s.c_out % 16:
            out[:, -(s.c_out % 16):] = 0
        if self.mutant == 'concat_slice_8_channels_off' and s.index in self.feeds_concat:
            # written 8 channels further into the concat buffer: the slice of this layer holds whatever was there (zeros)
            # in its first 8 channels, then the output
            out = np.concatenate([np.zeros_like(out[:, :8]), out[:, :-8]], axis=1)
        return out

    def _detect(self, det):
        W, rows = self.W, []
        na, no = W.na, W.nc + 5
        for level, f in enumerate(det.frm):
            a = torch.from_numpy(stored_input(self, self.specs, f))
            w = torch.from_numpy(round_storage(W.weights[det.conv_names[level] + '.weight'], self.dtype))
            b = torch.from_numpy(W.weights[det.conv_names[level] + '.bias'])
            z = self._sum(a, w, b, det)
            if self.mutant == 'n_tail_left_at_zero':
                z[:, -(z.shape[1] % 16):] = 0
            n, _, ny, nx = z.shape
            s = torch.sigmoid(z.reshape(n, na, no, ny, nx).permute(0, 1, 3, 4, 2))
            yv, xv = torch.meshgrid(torch.arange(ny, dtype=torch.float32), torch.arange(nx, dtype=torch.float32), indexing='ij')
            grid = torch.stack((xv, yv), 2).reshape(1, 1, ny, nx, 2) - 0.5
            anchors = torch.from_numpy(W.anchors_px[level]).reshape(1, na, 1, 1, 2)
            xy = (s[..., :2] * 2 + grid) * float(W.strides[level])
            wh = (s[..., 2:4] * 2) ** 2 * anchors
            rows.append(torch.cat((xy, wh, s[..., 4:]), 4).reshape(n, na * ny * nx, no))
        return torch.cat(rows, 1).numpy()


def input_tensor(net):
    """the network input of the CPU tests: the images as the letterbox kernel leaves them (/ 255, CHW)"""
    return np.stack([im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in images(net)])


# ---- what the tile configurations claim ---------------------------------------------------------------------------------

PUBLIC_FAMILIES = ('v1', 'v2', 'v5:run', 'v5:run/r2p5', 'v5:strip', 'stem', 'v7')


def family(cfg_name):
    """tile family of a configuration name (the first-generation tiles carry no prefix); dev: and f8: are not public"""
    if ':' not in cfg_name:
        return 'v1'
    head = cfg_name.split(':')[0]
    if head == 'v5':
        if cfg_name.startswith('v5:strip'):
            return 'v5:strip'
        return 'v5:run/r2p5' if cfg_name.endswith('/r2p5') else 'v5:run'
    return head


def tile_of(cfg_name):
    """(tile M, tile N) of a configuration name: the first  <M>x<N>  in it"""
    import re
    m = re.search(r'(\d+)x(\d+)', cfg_name.split(':')[-1])
    return int(m.group(1)), int(m.group(2))


def op_shapes(net, W, infos):
    """per conv op of a context's op_infos (kind 0) the shape facts the coverage predicates speak about"""
    from megadetector_amd.yolo_model import layer_divisors
    n, h, w = NETS[net]['shape']
    div = layer_divisors(W.specs)
    out = {}
    for o in infos:
        if o['kind'] != 0:
            continue
        s = W.specs[o['layer']]
        if s.type == MDHIP_DETECT:
            level = int(o['name'].split('Detect.m')[1].split()[0])
            src, k, stride, key = s.frm[level], 1, 1, ('detect', level)
            c_in = W.weights[s.conv_names[level] + '.weight'].shape[1]
        else:
            assert s.type == MDHIP_CONV, o
            src, k, stride, c_in, key = s.frm[0], s.k, s.s, s.c_in, o['layer']
        d_in = 1 if src < 0 else div[src]
        H, Wd = h // d_in, w // d_in
        Ho, Wo = H // stride, Wd // stride
        assert o['m'] == n * Ho * Wo, (o, Ho, Wo)
        out[(net, o['op'])] = dict(net=net, op=o['op'], name=o['name'], layer=o['layer'], C=c_in, N=o['n'], K=o['k'], M=o['m'],
                                   ksize=k, stride=stride, H=H, W=Wd, Ho=Ho, Wo=Wo, images=n, stem=src < 0, key=key)
    return out


def unmet_coverage(claims, shapes):
    """claims: {configuration name: set of (net, op)} over BOTH probe networks, public families only; shapes: op_shapes of
    both.  Returns the coverage predicates that do not hold (an empty list: the probe networks reach what they are for)."""
    unmet = []

    def need(ok, what):
        if not ok:
            unmet.append(what)

    def ops_of(pred):
        return {k for c, ops in claims.items() if pred(c) for k in ops}

    def some(ops, pred):
        return any(pred(shapes[k]) for k in ops)

    fam = {f: ops_of(lambda c, f=f: family(c) == f) for f in PUBLIC_FAMILIES}
    for f in PUBLIC_FAMILIES:
        need(fam[f], 'family {} claims a probe op'.format(f))
    need(fam['v1'] | fam['v2'] == set(shapes), 'the first generation and v2: between them claim every op (missing: {})'.format(
        sorted(shapes[k]['name'] for k in set(shapes) - fam['v1'] - fam['v2'])))
    for aligned in (True, False):
        for tail in (True, False):
            need(some(fam['v7'], lambda s: (s['Wo'] % 80 == 0) == aligned and (s['C'] % 64 != 0) == tail),
                 'v7: claims an op with Wo % 80 {} 0 and C % 64 {} 0'.format('==' if aligned else '!=', '!=' if tail else '=='))
    run = fam['v5:run']
    need(some(run, lambda s: s['W'] % 80 == 0), 'v5:run claims an op with W % 80 == 0')
    need(some(run, lambda s: s['W'] % 80 != 0), 'v5:run claims an op with W % 80 != 0')
    half = lambda s: 0 < s['C'] % 64 <= 32
    need(some(run, half), 'v5:run claims an op whose last 64-channel group is at most half full')
    need(some(run, lambda s: not half(s)), 'v5:run claims an op whose last 64-channel group is more than half full')
    for tile in ('run160x320', 'run320x160'):
        need(some(ops_of(lambda c: family(c) == 'v5:run' and tile in c), lambda s: s['net'] == 'A' and s['layer'] == 6),
             'v5:{} claims layer 6 of network A'.format(tile))
    v2 = fam['v2']
    need(some(v2, lambda s: s['ksize'] == 3), 'v2: claims a 3x3')
    need(some(v2, lambda s: s['ksize'] == 1 and s['C'] % 64 == 0), 'v2: claims a 1x1 on whole 64-channel slabs')
    need(some(v2, lambda s: s['ksize'] == 1 and s['C'] % 64 != 0), 'v2: claims a 1x1 that is not on whole slabs')
    need(some(ops_of(lambda c: family(c) == 'v2' and c.endswith('/a3')), lambda s: s['ksize'] == 1 and s['K'] >= 192),
         'the /a3 ring configurations claim a 1x1 with K >= 192')
    pairs = [(tile_of(c), shapes[k]) for c, ops in claims.items() for k in ops]
    need(any(s['M'] % t[0] for t, s in pairs), 'a claimed op has M that is no multiple of the tile M')
    need(any(s['images'] > 1 and (s['Ho'] * s['Wo']) % t[0] for t, s in pairs), 'a claimed op has a tile that spans two images')
    need(any(s['N'] % t[1] for t, s in pairs), 'a claimed op has N that is no multiple of the tile N')
    need(any(s['K'] <= SHARP_K for _, s in pairs), 'a claimed op has K <= {}'.format(SHARP_K))
    return unmet
