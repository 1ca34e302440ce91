"""
Host-side model description for the HIP runtime: resolves a YOLOv5 yaml dict (the dict
pickled as `model.yaml` inside md_v5a.0.0.pt, or megadetector_amd.yolo_yaml.YOLOV5X6_MD) into
the flat layer / conv tables of include/mdhip.h, and holds BN-folded fp32 weights.

Mirrors what the reference obtains from `checkpoint['model'].float().fuse().eval()`
(reference megadetector/detection/pytorch_detector.py:957) -- a module list plus fused conv
weights -- without needing the yolov5 package.
"""

import math

import numpy as np

# module kinds of include/mdhip.h
MDHIP_CONV, MDHIP_C3, MDHIP_SPPF, MDHIP_UPSAMPLE, MDHIP_CONCAT, MDHIP_DETECT = range(6)
MDHIP_C3K2, MDHIP_C2PSA, MDHIP_DETECT_DFL = 6, 7, 8
MDHIP_ELAN4, MDHIP_ADOWN, MDHIP_CBLINEAR, MDHIP_CBFUSE, MDHIP_DETECT_DDFL, MDHIP_SILENCE = 9, 10, 11, 12, 13, 14

DETECT_TYPES = (MDHIP_DETECT, MDHIP_DETECT_DFL, MDHIP_DETECT_DDFL)
#: anchor-free heads: predictions [cx, cy, w, h, cls...] decoded with the DFL
ANCHOR_FREE_TYPES = (MDHIP_DETECT_DFL, MDHIP_DETECT_DDFL)
#: modules of other architectures that the ultralytics (YOLO11) resolver refuses (cedar's yolov9 modules among them)
_OTHER_ULTRALYTICS = ('RepNCSPELAN4', 'ADown', 'SPPELAN', 'CBLinear', 'CBFuse', 'DDetect', 'DualDDetect', 'Silence',
                      'C2f', 'RepC3', 'AConv', 'ELAN1', 'Segment', 'Pose', 'OBB', 'v10Detect')


def _make_divisible(x, divisor):
    return int(math.ceil(x / divisor) * divisor)


class LayerSpec:
    __slots__ = ('index', 'type', 'frm', 'c_in', 'c_out', 'k', 's', 'p', 'n', 'shortcut',
                 'hidden', 'conv_names')

    def __init__(self, **kw):
        for name in self.__slots__:
            setattr(self, name, kw.get(name))


def resolve_yaml(yaml, ch=3):
    """
    yaml dict -> list[LayerSpec]; every 'from' is an absolute layer index (-1 = network input);
    conv_names lists the state_dict prefixes ('model.2.cv1.conv', ...) of the layer's convs in
    the order include/mdhip.h prescribes.  YOLOv5, YOLO11 (ultralytics, anchor-free) and YOLOv9 (yolov9 package,
    anchor-free; chosen by its module names) yamls.
    """
    from .yolo_yaml import is_yolov9
    if is_yolov9(yaml):
        return resolve_yolov9_yaml(yaml, ch)
    if 'anchors' not in yaml:
        return resolve_yolo11_yaml(yaml, ch)
    anchors, nc = yaml['anchors'], yaml['nc']
    gd, gw = yaml['depth_multiple'], yaml['width_multiple']
    na = (len(anchors[0]) // 2) if isinstance(anchors, (list, tuple)) else int(anchors)
    no = na * (nc + 5)
    out_ch = []
    specs = []
    rows = list(yaml['backbone']) + list(yaml['head'])
    for i, (f, n, m, args) in enumerate(rows):
        args = list(args)
        n_rep = max(round(n * gd), 1) if n > 1 else n
        frm = [f] if isinstance(f, int) else list(f)
        frm = [(i - 1 if x == -1 else (x if x >= 0 else i + x)) for x in frm]   # absolute; layer -1 = input
        c_in = ch if frm[0] < 0 else out_ch[frm[0]]
        pre = 'model.{}'.format(i)
        if m == 'Conv':
            c2 = args[0] if args[0] == no else _make_divisible(args[0] * gw, 8)
            k = args[1] if len(args) > 1 else 1
            s = args[2] if len(args) > 2 else 1
            p = args[3] if len(args) > 3 else k // 2
            spec = LayerSpec(index=i, type=MDHIP_CONV, frm=frm, c_in=c_in, c_out=c2, k=k, s=s, p=p,
                             n=1, shortcut=0, conv_names=[pre + '.conv'])
        elif m == 'C3':
            c2 = _make_divisible(args[0] * gw, 8)
            shortcut = args[1] if len(args) > 1 else True
            names = [pre + '.cv1.conv', pre + '.cv2.conv', pre + '.cv3.conv']
            for j in range(n_rep):
                names += ['{}.m.{}.cv1.conv'.format(pre, j), '{}.m.{}.cv2.conv'.format(pre, j)]
            spec = LayerSpec(index=i, type=MDHIP_C3, frm=frm, c_in=c_in, c_out=c2, k=1, s=1, p=0,
                             n=n_rep, shortcut=int(bool(shortcut)), hidden=int(c2 * 0.5),
                             conv_names=names)
        elif m == 'SPPF':
            c2 = _make_divisible(args[0] * gw, 8)
            k = args[1] if len(args) > 1 else 5
            spec = LayerSpec(index=i, type=MDHIP_SPPF, frm=frm, c_in=c_in, c_out=c2, k=k, s=1,
                             p=k // 2, n=1, shortcut=0, hidden=c_in // 2,
                             conv_names=[pre + '.cv1.conv', pre + '.cv2.conv'])
        elif m in ('nn.Upsample', 'Upsample'):
            if args[1] != 2 or (len(args) > 2 and args[2] != 'nearest'):
                raise ValueError('only nearest x2 upsampling is supported')
            spec = LayerSpec(index=i, type=MDHIP_UPSAMPLE, frm=frm, c_in=c_in, c_out=c_in, k=0, s=1,
                             p=0, n=1, shortcut=0, conv_names=[])
        elif m == 'Concat':
            c2 = sum(out_ch[x] for x in frm)
            spec = LayerSpec(index=i, type=MDHIP_CONCAT, frm=frm, c_in=c_in, c_out=c2, k=0, s=1, p=0,
                             n=1, shortcut=0, conv_names=[])
        elif m == 'Detect':
            spec = LayerSpec(index=i, type=MDHIP_DETECT, frm=frm, c_in=c_in, c_out=no, k=1, s=1, p=0,
                             n=1, shortcut=0,
                             conv_names=['{}.m.{}'.format(pre, l) for l in range(len(frm))])
        else:
            raise ValueError('unsupported YOLOv5 module "{}" at layer {}'.format(m, i))
        specs.append(spec)
        out_ch.append(spec.c_out if m != 'Detect' else None)
    return specs


def resolve_yolo11_yaml(yaml, ch=3):
    """
    ultralytics yolo11.yaml dict -> list[LayerSpec] ([3P] ultralytics nn/tasks.py parse_model, restated):
    channels make_divisible(min(c, max_channels) * width, 8), repeats max(round(n * depth), 1) for n > 1, c3k forced on
    every C3k2 at the m / l / x scales, Detect hidden widths c2 = max(16, ch0 / 4, 64), c3 = max(ch0, min(nc, 100)).
    """
    nc = int(yaml['nc'])
    scale = yaml.get('scale')
    scales = yaml.get('scales') or {}
    if not scale or scale not in scales:
        raise ValueError('YOLO11 model description without a usable "scale" (got {!r}; scales {})'.format(
            scale, sorted(scales)))
    gd, gw, max_ch = scales[scale]
    out_ch, specs = [], []
    rows = list(yaml['backbone']) + list(yaml['head'])
    for i, (f, n, m, args) in enumerate(rows):
        args = list(args)
        m = m.split('.')[-1] if m.startswith('torch.nn.') else m
        n_rep = max(round(n * gd), 1) if n > 1 else n
        frm = [f] if isinstance(f, int) else list(f)
        frm = [(i - 1 if x == -1 else (x if x >= 0 else i + x)) for x in frm]
        c_in = ch if frm[0] < 0 else out_ch[frm[0]]
        pre = 'model.{}'.format(i)
        div = lambda c: _make_divisible(min(c, max_ch) * gw, 8)
        if m == 'Conv':
            c2 = div(args[0])
            k = args[1] if len(args) > 1 else 1
            s = args[2] if len(args) > 2 else 1
            p = args[3] if len(args) > 3 and args[3] is not None else k // 2
            spec = LayerSpec(index=i, type=MDHIP_CONV, frm=frm, c_in=c_in, c_out=c2, k=k, s=s, p=p,
                             n=1, shortcut=0, conv_names=[pre + '.conv'])
        elif m == 'C3k2':
            c2 = div(args[0])
            c3k = bool(args[1]) if len(args) > 1 else False
            e = args[2] if len(args) > 2 else 0.5
            if scale in 'mlx':
                c3k = True
            c = int(c2 * e)
            names = [pre + '.cv1.conv', pre + '.cv2.conv']
            for j in range(n_rep):
                b = '{}.m.{}'.format(pre, j)
                if c3k:
                    names += [b + '.cv1.conv', b + '.cv2.conv', b + '.cv3.conv']
                    names += ['{}.m.{}.cv{}.conv'.format(b, q, r) for q in range(2) for r in (1, 2)]
                else:
                    names += [b + '.cv1.conv', b + '.cv2.conv']
            spec = LayerSpec(index=i, type=MDHIP_C3K2, frm=frm, c_in=c_in, c_out=c2, k=int(c3k), s=1, p=0,
                             n=n_rep, shortcut=1, hidden=c, conv_names=names)
        elif m == 'C2PSA':
            c2 = div(args[0])
            if c2 != c_in:
                raise ValueError('C2PSA at layer {}: c1 {} != c2 {}'.format(i, c_in, c2))
            names = [pre + '.cv1.conv', pre + '.cv2.conv']
            for j in range(n_rep):
                b = '{}.m.{}'.format(pre, j)
                names += [b + '.attn.qkv.conv', b + '.attn.proj.conv', b + '.attn.pe.conv', b + '.ffn.0.conv',
                          b + '.ffn.1.conv']
            spec = LayerSpec(index=i, type=MDHIP_C2PSA, frm=frm, c_in=c_in, c_out=c2, k=0, s=1, p=0,
                             n=n_rep, shortcut=1, hidden=c2 // 2, conv_names=names)
        elif m == 'SPPF':
            c2 = div(args[0])
            k = args[1] if len(args) > 1 else 5
            spec = LayerSpec(index=i, type=MDHIP_SPPF, frm=frm, c_in=c_in, c_out=c2, k=k, s=1,
                             p=k // 2, n=1, shortcut=0, hidden=c_in // 2,
                             conv_names=[pre + '.cv1.conv', pre + '.cv2.conv'])
        elif m in ('nn.Upsample', 'Upsample'):
            if args[1] != 2 or (len(args) > 2 and args[2] != 'nearest'):
                raise ValueError('only nearest x2 upsampling is supported')
            spec = LayerSpec(index=i, type=MDHIP_UPSAMPLE, frm=frm, c_in=c_in, c_out=c_in, k=0, s=1,
                             p=0, n=1, shortcut=0, conv_names=[])
        elif m == 'Concat':
            c2 = sum(out_ch[x] for x in frm)
            spec = LayerSpec(index=i, type=MDHIP_CONCAT, frm=frm, c_in=c_in, c_out=c2, k=0, s=1, p=0,
                             n=1, shortcut=0, conv_names=[])
        elif m == 'Detect':
            names = []
            for l in range(len(frm)):
                names += ['{}.cv2.{}.0.conv'.format(pre, l), '{}.cv2.{}.1.conv'.format(pre, l), '{}.cv2.{}.2'.format(pre, l),
                          '{}.cv3.{}.0.0.conv'.format(pre, l), '{}.cv3.{}.0.1.conv'.format(pre, l),
                          '{}.cv3.{}.1.0.conv'.format(pre, l), '{}.cv3.{}.1.1.conv'.format(pre, l),
                          '{}.cv3.{}.2'.format(pre, l)]
            ch0 = out_ch[frm[0]]
            spec = LayerSpec(index=i, type=MDHIP_DETECT_DFL, frm=frm, c_in=c_in, c_out=4 + nc, k=1, s=1, p=0,
                             n=1, shortcut=0, hidden=(max(16, ch0 // 4, 64), max(ch0, min(nc, 100))), conv_names=names)
        elif m in _OTHER_ULTRALYTICS:
            raise ValueError('unsupported module "{}" at layer {} of an ultralytics (YOLO11) model description: cedar '
                             '(YOLOv9-C) is a yolov9-package model, described in the YOLOv5 yaml format (depth_multiple, '
                             'width_multiple, anchors), not by a scale-keyed yaml'.format(m, i))
        else:
            raise ValueError('unsupported YOLO11 module "{}" at layer {}'.format(m, i))
        specs.append(spec)
        out_ch.append(spec.c_out if spec.type != MDHIP_DETECT_DFL else None)
    return specs


def _repncsp_names(b, n):
    names = [b + '.cv1.conv', b + '.cv2.conv', b + '.cv3.conv']
    for j in range(n):
        names += ['{}.m.{}.cv1.conv'.format(b, j), '{}.m.{}.cv2.conv'.format(b, j)]
    return names


def resolve_yolov9_yaml(yaml, ch=3):
    """
    yolov9-package yaml dict (MDv1000-cedar) -> list[LayerSpec] ([3P] yolov9 models/yolo.py parse_model, restated):
    channels make_divisible(c2 * width_multiple, 8) for Conv / ADown / RepNCSPELAN4 / SPPELAN (their other width arguments
    are taken as they are), CBLinear outputs as listed, CBFuse = the channels of its last input, Silence = identity.
      RepNCSPELAN4 [c2, c3, c4, n]: hidden (c3, c4), n RepNBottlenecks per RepNCSP (RepConvN folded: one 3x3 conv)
      SPPELAN [c2, c3]: the SPPF lowering with hidden width c3 (convs cv1, cv5)
      CBLinear [[c...]]: hidden = the list of output splits
      CBFuse [[idx...]]: hidden = the channel offset of the chosen split in each CBLinear input; k / s / p carry them
      DDetect / DualDDetect: n = heads (1 / 2), k = the head whose output is post-processed (0: yolov9's NMS keeps
      prediction[0] of DualDDetect's [y_first, y_second]), hidden = (c2, c3) per head
    Anchor-free; the yaml's 'anchors' (an int) is not used.
    """
    nc = int(yaml['nc'])
    gd, gw = yaml.get('depth_multiple', 1.0), yaml.get('width_multiple', 1.0)
    out_ch, specs = [], []
    rows = list(yaml['backbone']) + list(yaml['head'])
    div8 = lambda c: _make_divisible(c * gw, 8)
    for i, (f, n, m, args) in enumerate(rows):
        args = list(args)
        m = m.split('.')[-1] if m.startswith('torch.nn.') else m
        n_rep = max(round(n * gd), 1) if n > 1 else n
        if n_rep != 1:
            raise ValueError('yolov9 layer {} ({}): repeated modules (n = {}) are not supported'.format(i, m, n))
        frm = [f] if isinstance(f, int) else list(f)
        frm = [(i - 1 if x == -1 else (x if x >= 0 else i + x)) for x in frm]
        c_in = ch if frm[0] < 0 else out_ch[frm[0]]
        pre = 'model.{}'.format(i)
        if m == 'Silence':
            spec = LayerSpec(index=i, type=MDHIP_SILENCE, frm=frm, c_in=c_in, c_out=c_in, k=0, s=1, p=0, n=1, shortcut=0,
                             conv_names=[])
        elif m == 'Conv':
            c2 = div8(args[0])
            k = args[1] if len(args) > 1 else 1
            s = args[2] if len(args) > 2 else 1
            p = args[3] if len(args) > 3 and args[3] is not None else k // 2
            spec = LayerSpec(index=i, type=MDHIP_CONV, frm=frm, c_in=c_in, c_out=c2, k=k, s=s, p=p,
                             n=1, shortcut=0, conv_names=[pre + '.conv'])
        elif m == 'RepNCSPELAN4':
            c2, c3, c4 = div8(args[0]), int(args[1]), int(args[2])
            rn = int(args[3]) if len(args) > 3 else 1
            names = ([pre + '.cv1.conv'] + _repncsp_names(pre + '.cv2.0', rn) + [pre + '.cv2.1.conv'] +
                     _repncsp_names(pre + '.cv3.0', rn) + [pre + '.cv3.1.conv', pre + '.cv4.conv'])
            spec = LayerSpec(index=i, type=MDHIP_ELAN4, frm=frm, c_in=c_in, c_out=c2, k=0, s=1, p=0, n=rn, shortcut=1,
                             hidden=(c3, c4), conv_names=names)
        elif m == 'ADown':
            c2 = div8(args[0])
            spec = LayerSpec(index=i, type=MDHIP_ADOWN, frm=frm, c_in=c_in, c_out=c2, k=3, s=2, p=1, n=1, shortcut=0,
                             hidden=c2 // 2, conv_names=[pre + '.cv1.conv', pre + '.cv2.conv'])
        elif m == 'SPPELAN':
            c2, c3 = div8(args[0]), int(args[1])
            spec = LayerSpec(index=i, type=MDHIP_SPPF, frm=frm, c_in=c_in, c_out=c2, k=5, s=1, p=2, n=1, shortcut=0,
                             hidden=c3, conv_names=[pre + '.cv1.conv', pre + '.cv5.conv'])
        elif m in ('nn.Upsample', 'Upsample'):
            if args[1] != 2 or (len(args) > 2 and args[2] != 'nearest'):
                raise ValueError('only nearest x2 upsampling is supported')
            spec = LayerSpec(index=i, type=MDHIP_UPSAMPLE, frm=frm, c_in=c_in, c_out=c_in, k=0, s=1,
                             p=0, n=1, shortcut=0, conv_names=[])
        elif m == 'Concat':
            c2 = sum(out_ch[x] for x in frm)
            spec = LayerSpec(index=i, type=MDHIP_CONCAT, frm=frm, c_in=c_in, c_out=c2, k=0, s=1, p=0,
                             n=1, shortcut=0, conv_names=[])
        elif m == 'CBLinear':
            splits = [int(c) for c in args[0]]
            spec = LayerSpec(index=i, type=MDHIP_CBLINEAR, frm=frm, c_in=c_in, c_out=sum(splits), k=1, s=1, p=0, n=1,
                             shortcut=0, hidden=splits, conv_names=[pre + '.conv'])
        elif m == 'CBFuse':
            idx = list(args[0])
            if len(idx) != len(frm) - 1 or not 1 <= len(idx) <= 3:
                raise ValueError('CBFuse at layer {}: 1 to 3 CBLinear inputs, one split index each'.format(i))
            c2 = out_ch[frm[-1]]
            offs = []
            for src, j in zip(frm[:-1], idx):
                if specs[src].type != MDHIP_CBLINEAR or not 0 <= j < len(specs[src].hidden) or specs[src].hidden[j] != c2:
                    raise ValueError('CBFuse at layer {}: input {} split {} does not match'.format(i, src, j))
                offs.append(sum(specs[src].hidden[:j]))
            ko = offs + [0] * (3 - len(offs))
            spec = LayerSpec(index=i, type=MDHIP_CBFUSE, frm=frm, c_in=c2, c_out=c2, k=ko[0], s=ko[1], p=ko[2], n=1,
                             shortcut=0, hidden=offs, conv_names=[])
        elif m in ('DDetect', 'DualDDetect'):
            heads = 2 if m == 'DualDDetect' else 1
            if len(frm) % heads:
                raise ValueError('{} at layer {}: inputs not divisible into {} heads'.format(m, i, heads))
            nl = len(frm) // heads
            names, hidden = [], []
            for h in range(heads):
                ch0 = out_ch[frm[h * nl]]
                hidden.append((_make_divisible(max(ch0 // 4, 64, 16), 4), max(ch0, min(2 * nc, 128))))
                a, b = ('cv2', 'cv3') if h == 0 else ('cv4', 'cv5')
                for l in range(nl):
                    names += ['{}.{}.{}.0.conv'.format(pre, a, l), '{}.{}.{}.1.conv'.format(pre, a, l), '{}.{}.{}.2'.format(pre, a, l),
                              '{}.{}.{}.0.conv'.format(pre, b, l), '{}.{}.{}.1.conv'.format(pre, b, l), '{}.{}.{}.2'.format(pre, b, l)]
            spec = LayerSpec(index=i, type=MDHIP_DETECT_DDFL, frm=frm, c_in=c_in, c_out=4 + nc, k=0, s=1, p=0, n=heads,
                             shortcut=0, hidden=hidden, conv_names=names)
        else:
            raise ValueError('unsupported yolov9 module "{}" at layer {} (cedar / YOLOv9-C modules: Silence, Conv, '
                             'RepNCSPELAN4, ADown, SPPELAN, nn.Upsample, Concat, CBLinear, CBFuse, DDetect, '
                             'DualDDetect)'.format(m, i))
        specs.append(spec)
        out_ch.append(spec.c_out if spec.type != MDHIP_DETECT_DDFL else None)
    if not specs or specs[-1].type != MDHIP_DETECT_DDFL:
        raise ValueError('yolov9 model description must end in DDetect or DualDDetect')
    return specs


def detect_inputs(spec):
    """the layers whose outputs the Detect head decodes: every input, or for DualDDetect those of the selected head"""
    if spec.type == MDHIP_DETECT_DDFL:
        nl = len(spec.frm) // spec.n
        return spec.frm[spec.k * nl:(spec.k + 1) * nl]
    return spec.frm


def layer_divisors(specs):
    """spatial divisor of every layer's output (network input / output size)"""
    div = []
    for s in specs:
        d = 1 if s.frm[-1 if s.type == MDHIP_CBFUSE else 0] < 0 else div[s.frm[-1 if s.type == MDHIP_CBFUSE else 0]]
        if s.type == MDHIP_CONV:
            d *= s.s
        elif s.type == MDHIP_ADOWN:
            d *= 2
        elif s.type == MDHIP_UPSAMPLE:
            d //= 2
        div.append(d)
    return div


def model_strides(specs):
    """Stride of every Detect input level, derived from the graph (== model.stride)."""
    div = layer_divisors(specs)
    det = specs[-1]
    if det.type not in DETECT_TYPES:
        return []
    return [float(div[f]) for f in detect_inputs(det)]


class YoloWeights:
    """
    BN-folded fp32 weights of a YOLOv5 model plus its description.

    weights: dict  state_dict-style name -> np.float32 array, e.g.
             'model.0.conv.weight' (OIHW), 'model.0.conv.bias', 'model.33.m.0.weight',
             'model.33.anchors' ((nl,na,2), in units of the level's stride, as in the checkpoint)
    """

    def __init__(self, yaml, weights, names=None, source='unknown'):
        self.yaml = yaml
        self.specs = resolve_yaml(yaml)
        self.weights = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items()}
        self.nc = int(yaml['nc'])
        self.strides = model_strides(self.specs)
        self.nl = len(self.strides)
        det = self.specs[-1]
        #: anchor-free (YOLO11) head: predictions [cx, cy, w, h, cls...], the ultralytics NMS and box rescale
        self.anchor_free = det.type in ANCHOR_FREE_TYPES
        #: the yolov9 package's post-processing (MDv1000-cedar): its NMS and its scale_boxes (the padding is not rounded)
        self.yolov9 = det.type == MDHIP_DETECT_DDFL
        if self.anchor_free:
            self.na = 1
            self.anchors_px = np.zeros((0, 0, 2), dtype=np.float32)
        elif det.type == MDHIP_DETECT:
            a = self.weights['model.{}.anchors'.format(det.index)].reshape(self.nl, -1, 2)
            self.na = a.shape[1]
            self.anchors_px = np.ascontiguousarray(
                a * np.asarray(self.strides, dtype=np.float32).reshape(-1, 1, 1), dtype=np.float32)
        else:
            self.na = 0
            self.anchors_px = np.zeros((0, 0, 2), dtype=np.float32)
        self.names = names or {0: 'animal', 1: 'person', 2: 'vehicle'}
        self.source = source
        self._check()

    def _check(self):
        for s in self.specs:
            for name in s.conv_names:
                w = self.weights.get(name + '.weight')
                b = self.weights.get(name + '.bias')
                if w is None or b is None:
                    raise KeyError('missing fused weights for {}'.format(name))
                if w.ndim != 4 or b.shape != (w.shape[0],):
                    raise ValueError('bad weight shape for {}: {} / {}'.format(name, w.shape, b.shape))

    @property
    def max_stride(self):
        return int(max(self.strides)) if self.strides else 2

    def torch_state(self):
        """weights as torch tensors (for the oracle in tests/bench -- not used by the product)."""
        import torch
        return {k: torch.from_numpy(v.copy()) for k, v in self.weights.items()}
