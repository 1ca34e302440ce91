"""
A forward stepped op by op: every op of a plan against a float64 (or exact) evaluation of that ONE op on what it read.

tests/conv_probe.py holds the conv tiles on networks whose layers are one plain conv each.  Here a test stops between the ops of
any model (mdhip_run_ops), reads what the next op is about to read (mdhip_read_op_tensor: its `in`, its residual -- read BEFORE
the op runs, the op overwrites it), runs it alone, reads what it wrote and what it multiplied (mdhip_read_op_weights), and
compares:

    conv                 conv_probe.conv_reference / conv_tolerance, unchanged; `act`, `stride`, `pad` from the plan text
    conv with residual   y = z sigmoid(z) + r in float64.  The epilogue (conv_v2.cpp epilogue_t and its kin) adds the unpacked
                         residual to the fp32 SiLU in fp32 and rounds once:  E_res = E + u |y|  for that one add (E: conv_probe
                         conv_error of the SiLU),  tol = E_res + ulp_storage(|y| + E_res) / 2
    conv with fp32 out   (Detect / DFL logits, no activation, no rounding to storage)  tol = (K + 4) u S
    pool (SPPF)          y1 = maxpool_k(x), y2 = maxpool_k(y1), y3 = maxpool_k(y2), stride 1, -inf padding; the four slices of
                         the buffer bit for bit (slice 0 is the input and stays)
    upsample, copy       repeat 2 x 2, identity; bit for bit
    Detect decode        the fp32 logits of the conv in front decoded in float64 (decode_interval) against the predictions
    DFL decode           yolo11_ref.dfl_decode of the box and class logits, bit for bit (test_dfl_decode_bit_exact)
    depthwise 3x3        kernel_elements.depthwise_reference: float64 on the channels the plan's mapping gathers, conv_tolerance,
                         with a residual the E_res form above; every element
    attention            kernel_elements.AttentionReference: float64 softmax(q k^T scale) v on the view read in place, every
                         element against the bound derived there
    ADown pools, CBFuse  yolov9_ref.adown_pool / cbfuse, bit for bit

For YOLOv5 models the weights read back are also pinned against the model: the rows of an op must be round_storage of the convs
its NAME stands for ("L4 C3.cv1|cv2 1x1": model.4.cv1.conv then model.4.cv2.conv), the bias exactly theirs.

A `source` has  n, shape, plan (parse_plan),  tensor(op, which),  run(first, count),  op_weights(op),  predictions():
HipStepSource steps a HipContext, EmulatedSteps is a float32 restatement over a byte-for-byte model of the arena, with planted
mistakes (MUTANTS) for tests/test_op_step_cpu.py.  Network C (NET_C) is the probe network of this file.
"""

import collections
import re

import numpy as np
import torch
import torch.nn.functional as F

import conv_probe as P
import kernel_elements as KE
from conv_probe import Verdict, round_storage, ulp_storage, ulp_f32, conv_reference, conv_tolerance, conv_error, U32

# OpKind of mdhip_ctx.h, as mdhip_plan_describe writes it
CONV, POOL, UPSAMPLE, DECODE, COPY, DW, ATTN, DFL, ADOWN, CBFUSE = range(10)
KIND_NAMES = ('conv', 'pool', 'upsample', 'decode', 'copy', 'depthwise', 'attention', 'dfl decode', 'adown', 'cbfuse')
IN, OUT, RES, OUT2, FSRC0 = 0, 1, 2, 3, 4                 # `which` of mdhip_read_op_tensor
STEM_REASON = 'its `in` is the space-to-depth network input: conv_probe holds both stem kinds'

View = collections.namedtuple('View', 'off ld c div valid')
_VIEWS = ('in', 'out', 'res', 'out2', 'fsrc0', 'fsrc1', 'fsrc2')
_INTS = ('pc', 'stride', 'pad', 'act', 'out_f32', 'pool_k', 'level', 'f32_off', 'f32_ld', 'cls_off', 'cls_ld', 'heads', 'n_fsrc',
         'has_res', 'up_peer')


def _view(text):
    return View(*[int(v) for v in text.split(':')])


def parse_plan(text):
    """the text of mdhip_plan_describe -> dict(arena_bytes, input, layers [View], ops [dict])"""
    plan = dict(layers=[], ops=[])
    for line in text.splitlines():
        if line.startswith('arena '):
            plan['input'] = _view(re.search(r' input=(\S+)', line).group(1))
            plan['arena_bytes'] = int(re.search(r' arena_bytes=(\d+)', line).group(1))
        elif line.startswith('layer '):
            plan['layers'].append(_view(re.search(r' out=(\S+)', line).group(1)))
        elif line.startswith('op '):
            m = re.match(r'op (\d+) kind=(\d+) layer=(-?\d+) name="([^"]*)" (.*)', line)
            f = dict(kv.split('=', 1) for kv in m.group(5).split())
            op = dict(op=int(m.group(1)), kind=int(m.group(2)), layer=int(m.group(3)), name=m.group(4))
            for v in _VIEWS:
                op[v] = _view(f[v])
            for k in _INTS:
                op[k] = int(f[k])
            op['dw'] = [int(v) for v in f['dw'].split(',')]
            op['ffac'] = [int(v) for v in f['ffac'].split(',')]
            op['stem'] = op['kind'] == CONV and op['in'].off == plan['input'].off
            assert op['op'] == len(plan['ops'])
            plan['ops'].append(op)
    return plan


def plan_of(W, dtype, capacity):
    from megadetector_amd.hip_backend import describe_plan
    return parse_plan(describe_plan(W, dtype, *capacity))


def model_convs(name):
    """the state_dict prefixes an op of a YOLOv5 plan packs, in row order, parsed from its name as mdhip_plan.cpp writes it"""
    m = re.match(r'L(\d+) (\S+)', name)
    pre, what = 'model.' + m.group(1), m.group(2)
    if what in ('stem', 'conv'):
        return [pre + '.conv']
    block, _, rest = what.partition('.')
    if block == 'Detect':
        return ['{}.m.{}'.format(pre, int(rest[1:]))]
    assert block in ('C3', 'SPPF'), name
    if rest == 'cv1|cv2':
        return [pre + '.cv1.conv', pre + '.cv2.conv']
    b = re.match(r'm(\d+)\.(cv[12])$', rest)
    if b:
        return ['{}.m.{}.{}.conv'.format(pre, b.group(1), b.group(2))]
    assert rest in ('cv1', 'cv2', 'cv3'), name
    return ['{}.{}.conv'.format(pre, rest)]


# ---- network C -----------------------------------------------------------------------------------------------------------

NET_C = P._yaml([
    [-1, 1, 'Conv', [48, 6, 2, 2]],             # 0  6x6 stem to 48 channels
    [-1, 1, 'SPPF', [48, 5]],                   # 1  on the stride-2 map; hidden 24: three 8-channel chunks (a part-filled group)
    [-1, 2, 'C3', [160, True]],                 # 2  hidden 80, 2 bottlenecks: 3x3 + residual at the fused kernel's shape
    [-1, 1, 'Conv', [64, 3, 2]],                # 3  stride 2
    [-1, 1, 'C3', [64, False]],                 # 4  hidden 32 (below one slab), 1 bottleneck, no residual
    [-1, 3, 'C3', [80, True]],                  # 5  hidden 40, 3 bottlenecks: an N tail with residual; writes its concat slice
    [-1, 1, 'Conv', [64, 3, 2]],                # 6  stride 2; Detect level 1
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],   # 7  launched: writes the first 64 channels of layer 8
    [[-1, 5], 1, 'Concat', [1]],                # 8  144 channels
    [-1, 1, 'C3', [48, False]],                 # 9  behind the upsample; hidden 24
    [[-1, 5], 1, 'Concat', [1]],                # 10 layer 5 a second time: a launched concat copy; Detect level 0 (K = 128)
], [10, 6])
CAPACITY_C = (3, 96, 128)
#: (images, h, w) of the forwards; the SPPF map is (h / 2) x (w / 2)
SHAPES_C = [(3, 8, 16), (3, 24, 40), (2, 32, 32), (2, 32, 64), (2, 40, 56), (1, 64, 128), (2, 88, 104)]


def sppf_launch(h, w):
    """the launch of launch_sppf_pool (misc_kernels.cpp) for an h x w map, from its rule: an 8-channel chunk of the map takes two
    LDS buffers of 16 bytes a pixel; four chunks a workgroup while they fit 64 KiB -- two when that gives 512 .. 1024 (pixel,
    chunk) items --, else one chunk while it fits, else the three chained launches"""
    per_chunk = h * w * 16 * 2
    if per_chunk * 4 <= 65536:
        return '<2>' if 512 <= h * w * 2 <= 1024 else '<4>'
    return '<1>' if per_chunk <= 65536 else 'chained'


def weights_c(seed=P.SEED, **kw):
    from megadetector_amd import weights_io
    return weights_io.synthetic_weights(NET_C, seed=seed, **kw)


def images_c(shape):
    """HWC uint8 images of a forward of network C: smooth (a 1x1 conv of a smooth map keeps its sign over whole regions, so the
    SPPF input has windows of negative values only, at the border too) under a little noise; one image nearly black"""
    n, h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(n):
        base = 127 + 110 * np.sin(xs / (9.0 + 4 * i) + i)[..., None] * np.cos(ys[..., None] / (7.0 + 2 * i) + 2 * np.arange(3))
        img = base + rng.normal(0, 6, (h, w, 3))
        if i == 1:
            img = img / 16
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def input_tensor_c(shape):
    return np.stack([im.transpose(2, 0, 1).astype(np.float32) / np.float32(255) for im in images_c(shape)])


def pool_reference(x, k, pad_value=-np.inf):
    """the four slices of the SPPF buffer in float64: x and the three chained k x k / stride 1 max pools"""
    ys = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))]
    for _ in range(3):
        ys.append(F.max_pool2d(F.pad(ys[-1], (k // 2,) * 4, value=pad_value), k, 1, 0))
    return torch.cat(ys, 1).numpy()


def padding_shows(x, k):
    """a zero-padded pool of x differs from the -inf-padded one in a border element"""
    d = pool_reference(x, k) != pool_reference(x, k, 0.0)
    inner = np.zeros(d.shape, dtype=bool)
    inner[..., k // 2:d.shape[2] - k // 2, k // 2:d.shape[3] - k // 2] = True
    return bool((d & ~inner).any())


# ---- verdicts ------------------------------------------------------------------------------------------------------------

class Exact:
    """a bit-for-bit comparison with the attributes of a Verdict: `over` counts the elements whose bits differ"""

    def __init__(self, what, got, want):
        got = np.ascontiguousarray(got, dtype=np.float32)
        want = np.ascontiguousarray(want, dtype=np.float32)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        diff = got.view(np.uint32) != want.view(np.uint32)
        self.what, self.K, self.key = what, 0, None
        self.over, self.size = int(diff.sum()), diff.size
        self.where = tuple(int(v) for v in np.unravel_index(int(diff.argmax()), diff.shape)) if diff.size else ()
        self.worst = float('inf') if self.over else 0.0
        self.got = float(got[self.where]) if diff.size else 0.0
        self.want = float(want[self.where]) if diff.size else 0.0

    def __str__(self):
        if not self.over:
            return '{}: bit-exact, {} elements'.format(self.what, self.size)
        return '{}: {} of {} differ, the first at {} (got {!r}, reference {!r})'.format(self.what, self.over, self.size, self.where,
                                                                                      self.got, self.want)


def decode_interval(z, level, W):
    """The Detect decode of fp32 logits z (n, na * no, ny, nx) in float64, as (lo, hi) of shape (n, na * ny * nx, no).  The
    kernel's statements (mdhip_internal.h): s^ = 1 / (1 + expf(-z)) -- expf within 1 ulp (2u), the add and the division round
    once (u each): |s^ - s| <= 4u s to first order, taken as 5u s; every decoded quantity rises with s, so the endpoints are
    the decode of s (1 -+ 5u).  Then  (2 s^ + g) stride  and  (2 s^)^2 anchor  round twice each (2 s^ is exact): two fp32 ulps of
    the larger endpoint."""
    n, _, ny, nx = z.shape
    na, no = W.na, W.nc + 5
    stride = float(W.strides[level])
    anchors = W.anchors_px[level].astype(np.float64).reshape(1, na, 1, 1, 2)
    gx = (np.arange(nx, dtype=np.float64) - 0.5).reshape(1, 1, 1, nx)
    gy = (np.arange(ny, dtype=np.float64) - 0.5).reshape(1, 1, ny, 1)
    with np.errstate(invalid='ignore'):                 # (NaN logits stay NaN: over every bound)
        s0 = np.exp(-np.logaddexp(0.0, -np.asarray(z, dtype=np.float64).reshape(n, na, no, ny, nx)))

    def decode(s):
        out = np.empty((n, na, ny, nx, no))
        out[..., 0] = (s[:, :, 0] * 2 + gx) * stride
        out[..., 1] = (s[:, :, 1] * 2 + gy) * stride
        out[..., 2:4] = (s[:, :, 2:4].transpose(0, 1, 3, 4, 2) * 2) ** 2 * anchors
        out[..., 4:] = s[:, :, 4:].transpose(0, 1, 3, 4, 2)
        return out.reshape(n, na * ny * nx, no)

    lo, hi = decode(s0 * (1 - 5 * U32)), decode(s0 * (1 + 5 * U32))
    wide = 2 * ulp_f32(np.maximum(np.abs(lo), np.abs(hi)))
    return lo - wide, hi + wide


def _nhwc(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))


def _nchw(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


class Result:
    def __init__(self, num_ops):
        self.num_ops = num_ops
        self.verdicts, self.excluded, self.pins, self.passed_over = [], [], [], []

    def failures(self):
        return [str(v) for v in self.verdicts + self.pins if v.over]

    def worst(self):
        """kind -> the verdict with the largest err / tol"""
        out = {}
        for v in self.verdicts:
            if v.kind not in out or v.worst > out[v.kind].worst:
                out[v.kind] = v
        return out

    def report(self):
        lines = ['  {:3d} {}'.format(v.op, v) for v in self.verdicts]
        lines += ['  {:3d} excluded: {}: {}'.format(op, name, why) for op, name, why in self.excluded]
        return '\n'.join(lines)


class StepChecker:
    """the references of one (model, storage type).  check_all walks a source's ops in order."""

    def __init__(self, W, dtype, pin=None):
        self.W, self.dtype = W, dtype
        self.pin = (not getattr(W, 'anchor_free', False)) if pin is None else pin

    # -- one op ---------------------------------------------------------------------------------------------------------------
    def _stored(self, a, op, which):
        assert P.is_storage(a, self.dtype), (op['name'], 'tensor', which, 'holds values that are not of the storage type')
        return a

    def conv(self, op, a, r, got, w, b, what):
        K = int(w.shape[1] * w.shape[2] * w.shape[3])
        y, z, S = conv_reference(a, w, b, op['stride'], op['pad'], act=bool(op['act']))
        if op['out_f32']:
            assert r is None
            # (an all-zero row -- the class conv's rows padded to 8 -- has S = 0: it must be 0 exactly, not 0 / 0)
            v = Verdict(what, K, got, y, np.maximum(P.accumulation_bound(S, K), np.finfo(np.float64).tiny))
            v.kind = 'conv fp32 out'
        elif r is None:
            v = Verdict(what, K, got, y, conv_tolerance(y, z, S, K, self.dtype))
            v.kind = 'conv'
        else:
            E = conv_error(y, z, S, K)                          # of the SiLU (the bare sum without activation)
            y = y + np.asarray(r, dtype=np.float64)
            E = E + U32 * np.abs(y)                             # the one fp32 add
            v = Verdict(what, K, got, y, E + 0.5 * ulp_storage(np.abs(y) + E, self.dtype))
            v.kind = 'conv + residual'
        return v

    def pin_weights(self, op, w, b):
        names = model_convs(op['name'])
        want_w = np.concatenate([round_storage(self.W.weights[k + '.weight'], self.dtype) for k in names], axis=0)
        want_b = np.concatenate([self.W.weights[k + '.bias'] for k in names]).astype(np.float32)
        if op['stem'] and want_w.shape[2] == 3:                 # the 3x3 stem lies inside zero outer taps
            want_w = np.pad(want_w, ((0, 0), (0, 0), (1, 2), (1, 2)))
        if w.shape != want_w.shape:
            w = np.full(want_w.shape, np.nan, dtype=np.float32)
        out = [Exact('{} weights against {}'.format(op['name'], ' | '.join(names)), w, want_w),
               Exact('{} bias against {}'.format(op['name'], ' | '.join(names)), b, want_b)]
        for v in out:
            v.op, v.kind = op['op'], 'pin'
        return out

    def depthwise(self, op, a, r, got, w, b, what):
        assert P.is_storage(w, self.dtype), (op['name'], 'weights read back that are not of the storage type')
        grp, grp_stride, grp_off = op['dw']
        v = KE.depthwise_verdict(what, got, a, w, b, r, grp, grp_stride, grp_off, bool(op['act']), self.dtype)
        v.kind = 'depthwise'
        return v

    def attention(self, op, a, got, what):
        n, c, H, Wd = a.shape
        heads = op['heads']
        assert c == heads * KE.HEAD_CH and got.shape == (n, heads * KE.HD, H, Wd), (op['name'], a.shape, got.shape)
        ref = KE.AttentionReference(_nhwc(a).reshape(n, H * Wd, c), heads, self.dtype)

        def maps(t):                                            # (n, tokens, channels) -> NCHW, as `got` is
            return _nchw(t.reshape(n, H, Wd, heads * KE.HD))
        v = Verdict(what, KE.KD, got, maps(ref.y), maps(ref.tol))
        v.kind = 'attention'
        return v

    # -- the walk -------------------------------------------------------------------------------------------------------------
    def check_all(self, src, only=None, what=''):
        """every op of the source's plan, in order: read its inputs, run it alone, read its output, judge.  `only`: the ops to
        judge (the others are run and listed in Result.passed_over; None: all).  Returns a Result: one verdict per op but the
        excluded stems (Result.excluded, with the reason), and the packing pins."""
        ops = src.plan['ops']
        res = Result(len(ops))
        decodes = []
        i = 0
        while i < len(ops):
            op = ops[i]
            if only is not None and i not in only:
                j = i
                while j < len(ops) and j not in only:
                    res.passed_over.append(j)
                    j += 1
                src.run(i, j - i)
                i = j
                continue
            label = '{} op {} "{}"'.format(what, i, op['name']).strip()
            kind = op['kind']
            if kind in (CONV, DW):
                w, b = src.op_weights(i)
                if self.pin and kind == CONV:
                    res.pins += self.pin_weights(op, w, b)
            if op['stem']:
                src.run(i, 1)
                res.excluded.append((i, op['name'], STEM_REASON))
            elif kind == DECODE or kind == DFL:
                src.run(i, 1)
                decodes.append((len(res.verdicts), op, label))             # judged once the predictions can be read
                res.verdicts.append(None)
            else:
                a = self._stored(src.tensor(i, IN), op, IN)
                r = self._stored(src.tensor(i, RES), op, RES) if op['has_res'] else None
                extra = [self._stored(src.tensor(i, FSRC0 + k), op, FSRC0 + k) for k in range(op['n_fsrc'])]
                src.run(i, 1)
                got = src.tensor(i, OUT)
                if kind == CONV:
                    v = self.conv(op, a, r, got, w, b, label)
                elif kind == DW:
                    v = self.depthwise(op, a, r, got, w, b, label)
                elif kind == POOL:
                    v = Exact(label, got, pool_reference(a, op['pool_k']).astype(np.float32))
                elif kind == UPSAMPLE:
                    v = Exact(label, got, a.repeat(2, axis=2).repeat(2, axis=3))
                elif kind == COPY:
                    v = Exact(label, got, a)
                elif kind == ATTN:
                    v = self.attention(op, a, got, label)
                elif kind == ADOWN:
                    import yolov9_ref as R9
                    A, B = R9.adown_pool(_nhwc(a), self.dtype)
                    v = Exact(label, np.concatenate([got.ravel(), src.tensor(i, OUT2).ravel()]),
                              np.concatenate([_nchw(A).ravel(), _nchw(B).ravel()]))
                elif kind == CBFUSE:
                    import yolov9_ref as R9
                    v = Exact(label, got, _nchw(R9.cbfuse([_nhwc(s) for s in extra], op['ffac'][:op['n_fsrc']], _nhwc(a), self.dtype)))
                else:
                    raise AssertionError(('no reference for op kind', kind, op['name']))
                if not hasattr(v, 'kind'):
                    v.kind = KIND_NAMES[kind]
                v.op = v.key = i
                res.verdicts.append(v)
            i += 1
        if decodes:
            pred = src.predictions()
            for slot, op, label in decodes:
                res.verdicts[slot] = self.decode(src, op, pred, label)
                res.verdicts[slot].op = res.verdicts[slot].key = op['op']
        return res

    def decode(self, src, op, pred, label):
        """a decode op from the fp32 logits of the convs in front of it (still in place: nothing overwrites them in a pass)"""
        ops = src.plan['ops']
        n, h, w = src.shape
        strides = [int(s) for s in self.W.strides]
        per = self.W.na if op['kind'] == DECODE else 1
        row = sum(per * (h // s) * (w // s) for s in strides[:op['level']])
        box = [o for o in ops[:op['op']] if o['kind'] == CONV and o['out_f32'] and o['f32_off'] == op['f32_off']]
        assert len(box) == 1, op['name']
        z = src.tensor(box[0]['op'], OUT)
        if op['kind'] == DECODE:
            lo, hi = decode_interval(z, op['level'], self.W)
            v = Verdict(label, 0, pred[:, row:row + lo.shape[1]], (lo + hi) / 2, (hi - lo) / 2)
            v.kind = 'decode'
            return v
        import yolo11_ref as R11
        cls = [o for o in ops[:op['op']] if o['kind'] == CONV and o['out_f32'] and o['f32_off'] == op['cls_off']]
        assert len(cls) == 1, op['name']
        c = src.tensor(cls[0]['op'], OUT)[:, :self.W.nc]
        want = R11.dfl_decode(_nhwc(z), _nhwc(c), float(strides[op['level']]))
        v = Exact(label, pred[:, row:row + want.shape[1]], want)
        v.kind = 'dfl decode'
        return v


# ---- sources -------------------------------------------------------------------------------------------------------------

class HipStepSource:
    """a HipContext stepped with mdhip_run_ops; `plan`: plan_of the same weights, storage type and capacity"""

    def __init__(self, ctx, shape, plan):
        self.ctx, self.shape, self.plan, self.n = ctx, shape, plan, shape[0]
        self._w = {}

    def tensor(self, op, which):
        return self.ctx.read_op_tensor(op, which, self.n)

    def run(self, first, count):
        self.ctx.run_ops(*self.shape, first, count)

    def op_weights(self, op):
        if op not in self._w:
            self._w[op] = self.ctx.read_op_weights(op)
        return self._w[op]

    def predictions(self):
        return self.ctx.read_predictions(self.n)


MUTANTS = ('residual_added_before_silu', 'residual_rounded_first', 'residual_8_channels_off', 'residual_read_after_write',
           'pool_pads_with_zero', 'pool_window_3', 'pool_stage_reads_slice_0', 'pool_swaps_h_w', 'upsample_transposed',
           'copy_slice_8_channels_off', 'merged_cv1_cv2_halves_swapped')


class EmulatedSteps:
    """A float32 restatement of the ops of a YOLOv5 plan over a model of the arena: one float32 per 16-bit element, at the
    element offsets of the plan, NaN where nothing was written (the poisoned arena).  Every op reads and writes its views as
    the kernels do -- pixel pitch `ld`, in place where the plan says so: a conv reads its residual from the view it writes.
    `conv`: the summation (conv_probe.conv_f32 / conv_f32_blocks); `mutant`: one planted mistake (MUTANTS)."""

    def __init__(self, W, dtype, plan, x, conv=P.conv_f32, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.W, self.dtype, self.plan, self.conv, self.mutant = W, dtype, plan, conv, mutant
        self.x = round_storage(x, dtype)
        self.n = x.shape[0]
        self.shape = (x.shape[0], x.shape[2], x.shape[3])
        self.mem = np.full(plan['arena_bytes'] // 2, np.nan, dtype=np.float32)
        self.f32 = {}
        strides = [int(s) for s in W.strides]
        self.level_rows = [W.na * (self.shape[1] // s) * (self.shape[2] // s) for s in strides]
        self.pred = np.full((self.n, sum(self.level_rows), W.nc + 5), np.nan, dtype=np.float32)

    # -- the arena --------------------------------------------------------------------------------------------------------------
    def _index(self, v):
        n, h, w = self.shape
        H, Wd = h // v.div, w // v.div
        assert v.valid and v.off % 2 == 0
        idx = v.off // 2 + np.arange(n * H * Wd, dtype=np.int64)[:, None] * v.ld + np.arange(v.c, dtype=np.int64)
        return idx, (n, H, Wd, v.c)

    def _get(self, v):
        idx, shape = self._index(v)
        return _nchw(self.mem[idx].reshape(shape))

    def _put(self, v, val):
        idx, shape = self._index(v)
        assert val.shape == (shape[0], shape[3], shape[1], shape[2]), (val.shape, shape)
        self.mem[idx] = _nhwc(val).reshape(idx.shape)

    def _round(self, t):
        return t.to(P.TORCH_DTYPE[self.dtype]).float()

    # -- the source interface -----------------------------------------------------------------------------------------------------
    def tensor(self, op, which):
        o = self.plan['ops'][op]
        if which == IN and o['stem']:
            return self.x
        if which == OUT and o['out_f32']:
            return self.f32[op]
        return self._get(o[_VIEWS[which]])

    def op_weights(self, op):
        names = model_convs(self.plan['ops'][op]['name'])
        if self.mutant == 'merged_cv1_cv2_halves_swapped':
            names = names[::-1]
        w = np.concatenate([round_storage(self.W.weights[k + '.weight'], self.dtype) for k in names], axis=0)
        return w, np.concatenate([self.W.weights[k + '.bias'] for k in names]).astype(np.float32)

    def predictions(self):
        return self.pred

    def run(self, first, count):
        with torch.no_grad():
            for i in range(first, first + count):
                o = self.plan['ops'][i]
                {CONV: self._conv, POOL: self._pool, UPSAMPLE: self._upsample, COPY: self._copy, DECODE: self._decode}[o['kind']](o)

    # -- the ops ----------------------------------------------------------------------------------------------------------------
    def _conv(self, o):
        m = self.mutant
        w, b = [torch.from_numpy(v) for v in self.op_weights(o['op'])]
        if o['stem']:
            z = self.conv(torch.from_numpy(self.x), w, b, 2, 2)
        else:
            z = self.conv(torch.from_numpy(self._get(o['in'])), w, b, o['stride'], o['pad'])
        silu = (lambda t: t * torch.sigmoid(t)) if o['act'] else (lambda t: t)
        if o['out_f32']:
            self.f32[o['op']] = silu(z).numpy()
            return
        if not o['has_res']:
            self._put(o['out'], self._round(silu(z)).numpy())
            return
        r = torch.from_numpy(self._get(o['res']))
        if m == 'residual_8_channels_off':
            r = torch.roll(r, -8, 1)
        if m == 'residual_added_before_silu':
            y = self._round(silu(z + r))
        elif m == 'residual_rounded_first':
            y = self._round(self._round(silu(z)) + r)
        elif m == 'residual_read_after_write':
            y = self._round(silu(z) + self._round(silu(z)))
        else:
            y = self._round(silu(z) + r)
        self._put(o['out'], y.numpy())

    def _pool(self, o):
        m = self.mutant
        k = 3 if m == 'pool_window_3' else o['pool_k']
        x = torch.from_numpy(self._get(o['in']))
        n, c, H, Wd = x.shape

        def pool(t):
            if m == 'pool_swaps_h_w':                 # the map walked as W rows of H pixels
                return pool_plain(t.reshape(n, c, Wd, H)).reshape(n, c, H, Wd)
            return pool_plain(t)

        def pool_plain(t):
            return F.max_pool2d(F.pad(t, (k // 2,) * 4, value=0.0 if m == 'pool_pads_with_zero' else -np.inf), k, 1, 0)

        y1 = pool(x)
        y2 = pool(x if m == 'pool_stage_reads_slice_0' else y1)
        y3 = pool(y2)
        for s, y in enumerate((y1, y2, y3)):
            self._put(o['out']._replace(off=o['out'].off + (s + 1) * c * 2, c=c), y.numpy())

    def _upsample(self, o):
        x = self._get(o['in'])
        y = x.repeat(2, axis=2).repeat(2, axis=3)
        if self.mutant == 'upsample_transposed':      # out[y][x] = in[x / 2][y / 2], the rows as long as they are
            y = np.ascontiguousarray(y.transpose(0, 1, 3, 2)).reshape(y.shape)
        self._put(o['out'], y)

    def _copy(self, o):
        x = self._get(o['in'])
        if self.mutant == 'copy_slice_8_channels_off':        # written 8 channels further into the concat buffer
            self._put(o['out']._replace(off=o['out'].off + 16, c=o['out'].c - 8), x[:, :-8])
        else:
            self._put(o['out'], x)

    def _decode(self, o):
        W = self.W
        level, na, no = o['level'], W.na, W.nc + 5
        z = torch.from_numpy(self.f32[o['op'] - 1])
        n, _, ny, nx = z.shape
        s = torch.sigmoid(z.reshape(n, na, no, ny, nx).permute(0, 1, 3, 4, 2))
        yv, xv = torch.meshgrid(torch.arange(ny, dtype=torch.float32), torch.arange(nx, dtype=torch.float32), indexing='ij')
        grid = torch.stack((xv, yv), 2).reshape(1, 1, ny, nx, 2) - 0.5
        anchors = torch.from_numpy(W.anchors_px[level]).reshape(1, na, 1, 1, 2)
        xy = (s[..., :2] * 2 + grid) * float(W.strides[level])
        wh = (s[..., 2:4] * 2) ** 2 * anchors
        row = sum(self.level_rows[:level])
        self.pred[:, row:row + self.level_rows[level]] = torch.cat((xy, wh, s[..., 4:]), 4).reshape(n, na * ny * nx, no).numpy()
