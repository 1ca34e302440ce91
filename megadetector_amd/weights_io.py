"""
Weights for the HIP detector: either lifted out of a real MegaDetector / YOLOv5 checkpoint
without importing the yolov5 package, or seeded synthetic weights on the same topology.

Checkpoint path mirrors reference megadetector/detection/pytorch_detector.py:913-959
(_load_model: torch.load(weights_only=False) -> checkpoint['model'].float().fuse().eval());
the Conv+BatchNorm folding that `.fuse()` performs in the third-party yolov5 package
(utils/torch_utils.py:fuse_conv_and_bn) is done here in fp32 on the host.
"""

import io
import pickle
import sys
import types
import zipfile

import numpy as np

from . import yolo_yaml
from .yolo_model import YoloWeights, resolve_yaml, MDHIP_DETECT, MDHIP_DETECT_DFL, MDHIP_DETECT_DDFL


# --------------------------------------------------------------------------------------
# seeded synthetic weights (no checkpoint available: there is no network in the build or
# bench environment; timing does not depend on the values, detections do)
# --------------------------------------------------------------------------------------

def synthetic_weights(yaml=None, seed=0, gain=1.75, res_gain=0.6, bias_std=0.1,
                      detect_gain=22.0, detect_obj_bias=-12.5):
    """
    Deterministic (numpy PCG64, platform independent) pseudo-trained weights.

    Conv weights are N(0, gain^2 / fan_in) with zero mean per output channel (what a folded
    BatchNorm achieves: no mean drift through the ~100 SiLU layers); the residual-branch 3x3 of
    every shortcut bottleneck is scaled by res_gain so the backbone does not blow up.  With
    gain below the critical value (~1.8) activations settle at std ~0.1-0.3.  The Detect biases
    make objectness rare, as in a trained detector: roughly one anchor in six clears the 1e-5
    batch-mode threshold (reference run_detector_batch.py:751 / pytorch_detector.py:1127) and
    a handful clear 0.005, so NMS sees a realistic candidate load.
    """
    from .yolo_model import model_strides
    yaml = yaml or yolo_yaml.YOLOV5X6_MD
    if yolo_yaml.is_yolo11(yaml):
        return synthetic_weights_yolo11(yaml, seed=seed)
    if yolo_yaml.is_yolov9(yaml):
        return synthetic_weights_yolov9(yaml, seed=seed)
    specs = resolve_yaml(yaml)
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {}
    nc = yaml['nc']
    for s in specs:
        if s.type == MDHIP_DETECT:
            na = len(yaml['anchors'][0]) // 2
            strides = model_strides(specs)
            for l, name in enumerate(s.conv_names):
                c_in = _channels_of(specs, s.frm[l])
                wt = rng.standard_normal((na * (nc + 5), c_in, 1, 1), dtype=np.float32)
                wt -= wt.mean(axis=1, keepdims=True)
                wt *= np.float32(detect_gain / np.sqrt(c_in))
                # box logits stay small: (2*sigmoid)^2 * anchor then gives boxes of 0.3x..2x the
                # anchor instead of degenerate slivers
                wt.reshape(na, nc + 5, c_in)[:, :4, :] *= np.float32(0.2)
                b = np.zeros((na, nc + 5), dtype=np.float32)
                b[:, 4] = detect_obj_bias
                b[:, 5:] = rng.standard_normal((na, nc), dtype=np.float32) * np.float32(0.5)
                w[name + '.weight'] = wt
                w[name + '.bias'] = b.reshape(-1)
            anchors = np.asarray(yaml['anchors'], dtype=np.float32).reshape(len(strides), -1, 2)
            anchors = anchors / np.asarray(strides, dtype=np.float32).reshape(-1, 1, 1)
            w['model.{}.anchors'.format(s.index)] = anchors.astype(np.float32)
            continue
        shapes = _conv_shapes(s)
        for name, (c2, c1, k) in zip(s.conv_names, shapes):
            wt = rng.standard_normal((c2, c1, k, k), dtype=np.float32)
            wt -= wt.mean(axis=(1, 2, 3), keepdims=True)
            g = gain
            if s.shortcut and '.m.' in name and name.endswith('.cv2.conv'):
                g = res_gain
            wt *= np.float32(g / np.sqrt(c1 * k * k))
            w[name + '.weight'] = wt
            w[name + '.bias'] = rng.standard_normal(c2, dtype=np.float32) * np.float32(bias_std)
    return YoloWeights(yaml, w, source='synthetic(seed={})'.format(seed))


def yolo11_conv_shapes(s, specs):
    """(name, (c_out, c_in, k)) of every conv of a YOLO11 layer, in the order of include/mdhip.h (c_in 1 = depthwise)"""
    from .yolo_model import MDHIP_C3K2, MDHIP_C2PSA
    names = s.conv_names
    if s.type == MDHIP_C3K2:
        c = s.hidden
        shapes = [(2 * c, s.c_in, 1), (s.c_out, (2 + s.n) * c, 1)]
        for _ in range(s.n):
            if s.k:
                h = c // 2
                shapes += [(h, c, 1), (h, c, 1), (c, 2 * h, 1)] + [(h, h, 3)] * 4
            else:
                shapes += [(c // 2, c, 3), (c, c // 2, 3)]
    elif s.type == MDHIP_C2PSA:
        c = s.hidden
        shapes = [(2 * c, s.c_in, 1), (s.c_out, 2 * c, 1)]
        for _ in range(s.n):
            shapes += [(2 * c, c, 1), (c, c, 1), (c, 1, 3), (2 * c, c, 1), (c, 2 * c, 1)]
    elif s.type == MDHIP_DETECT_DFL:
        c2, c3 = s.hidden
        nc = s.c_out - 4
        shapes = []
        for f in s.frm:
            cx = specs[f].c_out
            shapes += [(c2, cx, 3), (c2, c2, 3), (64, c2, 1), (cx, 1, 3), (c3, cx, 1), (c3, 1, 3), (c3, c3, 1), (nc, c3, 1)]
    else:
        shapes = _conv_shapes(s)
    assert len(shapes) == len(names), (s.index, len(shapes), len(names))
    return list(zip(names, shapes))


def synthetic_weights_yolo11(yaml, seed=0, gain=1.6, res_gain=0.5, bias_std=0.1, cls_bias=-12.0, cls_gain=1.5,
                             box_gain=0.5):
    """
    Seeded weights on a YOLO11 topology, built like the YOLOv5 set: zero-mean N(0, gain^2 / fan_in) kernels, the
    convs that end a residual branch (bottleneck cv2, attention proj, ffn.1) at res_gain, the ones without activation
    at gain 1.  Class biases of -12 with logits of std ~1.5 let about one anchor in six clear the 1e-5 batch-mode
    threshold (sigmoid(-11.5) = 1e-5), as the YOLOv5 set does; box logits stay small (boxes of a
    few cells).
    """
    specs = resolve_yaml(yaml)
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {}
    for s in specs:
        for name, (c2, c1, k) in yolo11_conv_shapes(s, specs):
            wt = rng.standard_normal((c2, c1, k, k), dtype=np.float32)
            fan = c1 * k * k
            if c1 > 1:
                wt -= wt.mean(axis=(1, 2, 3), keepdims=True)
            g = gain
            if name.endswith(('.attn.proj.conv', '.ffn.1.conv')) or (s.type != MDHIP_DETECT_DFL and name.endswith('.cv2.conv')
                                                                      and '.m.' in name):
                g = res_gain
            elif name.endswith(('.attn.qkv.conv', '.attn.pe.conv')):
                g = 1.0
            b = rng.standard_normal(c2, dtype=np.float32) * np.float32(bias_std)
            if s.type == MDHIP_DETECT_DFL and name.split('.')[-1] == '2':
                if name.split('.')[2] == 'cv2':       # box logits
                    g = box_gain * np.sqrt(fan)
                    b = rng.standard_normal(c2, dtype=np.float32) * np.float32(0.5)
                else:                                 # class logits
                    g = cls_gain * np.sqrt(fan)
                    b = np.float32(cls_bias) + rng.standard_normal(c2, dtype=np.float32) * np.float32(0.5)
            wt *= np.float32(g / np.sqrt(fan))
            w[name + '.weight'] = wt.astype(np.float32)
            w[name + '.bias'] = b.astype(np.float32)
    det = specs[-1]
    w['model.{}.dfl.conv.weight'.format(det.index)] = np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)
    return YoloWeights(yaml, w, source='synthetic(seed={})'.format(seed))


def yolov9_conv_shapes(s, specs):
    """(name, (c_out, c_in, k)) of every conv of a YOLOv9 layer, in the order of include/mdhip.h (the grouped box conv of
    the Detect head: c_in = c2 / 4, its checkpoint shape)"""
    from .yolo_model import MDHIP_ELAN4, MDHIP_ADOWN, MDHIP_CBLINEAR
    names = s.conv_names
    if s.type == MDHIP_ELAN4:
        c3, c4 = s.hidden

        def rep(c1, c2):
            h = c2 // 2
            return [(h, c1, 1), (h, c1, 1), (c2, 2 * h, 1)] + [(h, h, 3), (h, h, 3)] * s.n
        shapes = [(c3, s.c_in, 1)] + rep(c3 // 2, c4) + [(c4, c4, 3)] + rep(c4, c4) + [(c4, c4, 3), (s.c_out, c3 + 2 * c4, 1)]
    elif s.type == MDHIP_ADOWN:
        c = s.c_out // 2
        shapes = [(c, s.c_in // 2, 3), (c, s.c_in // 2, 1)]
    elif s.type == MDHIP_CBLINEAR:
        shapes = [(s.c_out, s.c_in, 1)]
    elif s.type == MDHIP_DETECT_DDFL:
        nc = s.c_out - 4
        nl = len(s.frm) // s.n
        shapes = []
        for h in range(s.n):
            c2, c3 = s.hidden[h]
            for f in s.frm[h * nl:(h + 1) * nl]:
                cx = specs[f].c_out
                shapes += [(c2, cx, 3), (c2, c2 // 4, 3), (64, c2, 1), (c3, cx, 3), (c3, c3, 3), (nc, c3, 1)]
    else:
        shapes = _conv_shapes(s)
    assert len(shapes) == len(names), (s.index, len(shapes), len(names))
    return list(zip(names, shapes))


def synthetic_weights_yolov9(yaml, seed=0, gain=1.5, res_gain=0.5, bias_std=0.1, cls_bias=-13.5, cls_gain=12.0,
                             box_gain=1.5):
    """
    Seeded weights on a YOLOv9 topology, built like the YOLO11 set: zero-mean N(0, gain^2 / fan_in) kernels, the second
    conv of every RepNBottleneck (the end of a residual branch) at res_gain, CBLinear (no activation) at gain 1.  The
    head's features have a standard deviation of ~0.1 whatever their width, so the final convs take gains of 12 (class)
    and 1.5 (box) over 1 / sqrt(fan_in): class logits of std ~1.5 around a bias of -13.5 (a minority of anchors clears the
    1e-5 batch-mode threshold), box logits of a few units.
    """
    from .yolo_model import MDHIP_CBLINEAR
    specs = resolve_yaml(yaml)
    rng = np.random.Generator(np.random.PCG64(seed))
    w = {}
    for s in specs:
        for name, (c2, c1, k) in yolov9_conv_shapes(s, specs):
            wt = rng.standard_normal((c2, c1, k, k), dtype=np.float32)
            fan = c1 * k * k
            wt -= wt.mean(axis=(1, 2, 3), keepdims=True)
            g = gain
            if '.m.' in name and name.endswith('.cv2.conv'):
                g = res_gain
            elif s.type == MDHIP_CBLINEAR:
                g = 1.0
            b = rng.standard_normal(c2, dtype=np.float32) * np.float32(bias_std)
            if s.type == MDHIP_DETECT_DDFL and name.split('.')[-1] == '2':
                if name.split('.')[2] in ('cv2', 'cv4'):       # box logits
                    g = box_gain
                    b = rng.standard_normal(c2, dtype=np.float32) * np.float32(0.5)
                else:                                          # class logits
                    g = cls_gain
                    b = np.float32(cls_bias) + rng.standard_normal(c2, dtype=np.float32) * np.float32(0.5)
            wt *= np.float32(g / np.sqrt(fan))
            w[name + '.weight'] = wt.astype(np.float32)
            w[name + '.bias'] = b.astype(np.float32)
    det = specs[-1]
    for h in range(det.n):
        w['model.{}.dfl{}.conv.weight'.format(det.index, '' if h == 0 else h + 1)] = \
            np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)
    return YoloWeights(yaml, w, source='synthetic(seed={})'.format(seed))


def _channels_of(specs, idx):
    return specs[idx].c_out


def _conv_shapes(s):
    from .yolo_model import MDHIP_CONV, MDHIP_C3, MDHIP_SPPF
    if s.type == MDHIP_CONV:
        return [(s.c_out, s.c_in, s.k)]
    if s.type == MDHIP_C3:
        h = s.hidden
        shapes = [(h, s.c_in, 1), (h, s.c_in, 1), (s.c_out, 2 * h, 1)]
        for _ in range(s.n):
            shapes += [(h, h, 1), (h, h, 3)]
        return shapes
    if s.type == MDHIP_SPPF:
        h = s.hidden
        return [(h, s.c_in, 1), (s.c_out, 4 * h, 1)]
    return []


# --------------------------------------------------------------------------------------
# real checkpoints
# --------------------------------------------------------------------------------------

class _StubModule:
    """Stand-in for any class of the yolov5 package (models.*, utils.*) found in the pickle."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)
        elif isinstance(state, tuple) and len(state) == 2 and isinstance(state[1], dict):
            if isinstance(state[0], dict):
                self.__dict__.update(state[0])
            self.__dict__.update(state[1])


def _stub_class(module, name):
    return type(name, (_StubModule,), {'__module__': module})


def _plain_numpy_scalar(scalar):
    """numpy's pickled-scalar constructor, refusing object dtypes: scalar(dtype('O'), bytes) unpickles `bytes` with the
    stock, unrestricted pickle on older numpy"""
    def checked(dtype, *args):
        if getattr(dtype, 'hasobject', True):
            raise pickle.UnpicklingError('refusing to unpickle a numpy scalar of dtype {}'.format(dtype))
        return scalar(dtype, *args)
    return checked


class _CheckpointUnpickler(pickle.Unpickler):
    """
    Resolves torch classes normally and fabricates attribute-bag stand-ins for everything from
    the yolov5 package, so `models.yolo.DetectionModel`, `models.common.Conv` ... unpickle
    without that package (reference pytorch_detector.py:950-957 needs them importable).
    """
    # Exact (module, name) pairs, not namespaces: `torch.*` / `numpy.*` as a whole also hold callables a crafted file
    # could REDUCE (torch.hub.load, torch.utils.cpp_extension.load_inline, numpy.load ...).  This narrows what a file
    # can reach; it is NOT a sandbox -- load checkpoints you trust (the reference does torch.load(weights_only=False),
    # pytorch_detector.py:929-948).
    _SAFE_GLOBALS = {
        ('collections', 'OrderedDict'), ('collections', 'defaultdict'),
        ('torch._utils', '_rebuild_tensor_v2'), ('torch._utils', '_rebuild_tensor'),
        ('torch._utils', '_rebuild_parameter'), ('torch._utils', '_rebuild_parameter_with_state'),
        ('torch._utils', '_rebuild_qtensor'),
        ('torch._tensor', '_rebuild_from_type_v2'), ('torch', 'Tensor'), ('torch', 'Size'), ('torch', 'device'),
        ('torch', 'dtype'), ('torch.nn.parameter', 'Parameter'), ('torch.serialization', '_get_layout'),
        ('torch.storage', 'TypedStorage'), ('torch.storage', 'UntypedStorage'),
        # NOT ('torch.storage', '_load_from_bytes'): it is torch.load(BytesIO(b), weights_only=False), i.e. an
        # unrestricted nested unpickle; torch.save checkpoints reference their storages through persistent_load
        ('numpy.core.multiarray', '_reconstruct'), ('numpy._core.multiarray', '_reconstruct'),
        ('numpy.core.multiarray', 'scalar'), ('numpy._core.multiarray', 'scalar'),
        ('numpy', 'ndarray'), ('numpy', 'dtype'), ('_codecs', 'encode'),
        ('pathlib', 'PosixPath'), ('pathlib', 'WindowsPath'), ('pathlib', 'PurePosixPath'), ('pathlib', 'PureWindowsPath'),
        ('pathlib', 'Path'),
    }
    _TORCH_STORAGE_OR_DTYPE = ('Storage',)          # torch.FloatStorage, torch.HalfStorage, ... (legacy typed storages)
    # plain data types only: `builtins` also holds eval / exec / getattr / __import__
    _SAFE_BUILTINS = ('set', 'frozenset', 'list', 'dict', 'tuple', 'slice', 'range', 'complex', 'int', 'float',
                      'bool', 'str', 'bytes', 'bytearray', 'object')

    def find_class(self, module, name):
        if module in ('builtins', '__builtin__'):          # '__builtin__': protocol-2 pickles (torch.save default)
            if name in self._SAFE_BUILTINS:
                import builtins
                return getattr(builtins, name)
            raise pickle.UnpicklingError('refusing to unpickle {}.{}'.format(module, name))
        if (module, name) in self._SAFE_GLOBALS:
            obj = super().find_class(module, name)
            if name == 'scalar' and module.endswith('multiarray'):
                return _plain_numpy_scalar(obj)
            return obj
        if module == 'torch' and name.endswith(self._TORCH_STORAGE_OR_DTYPE) and '.' not in name:
            return super().find_class(module, name)
        if module.startswith('torch.nn.modules.') and '.' not in name:
            # layer classes of torch.nn (Conv2d, BatchNorm2d, SiLU, Upsample, MaxPool2d, Sequential, ModuleList ...):
            # only actual nn.Module subclasses, never a function of those modules
            cls = super().find_class(module, name)
            import torch
            if isinstance(cls, type) and issubclass(cls, torch.nn.Module):
                return cls
            raise pickle.UnpicklingError('refusing to unpickle {}.{}'.format(module, name))
        if module.split('.')[0] in ('models', 'utils', 'yolov5', 'yolov9', 'ultralytics', '__main__'):
            return _stub_class(module, name)
        raise pickle.UnpicklingError('refusing to unpickle {}.{}'.format(module, name))


class _PickleModule(types.ModuleType):
    """pickle_module argument for torch.load"""

    def __init__(self):
        super().__init__('mdhip_pickle')
        self.Unpickler = _CheckpointUnpickler
        self.load = lambda f, **kw: _CheckpointUnpickler(f, **kw).load()
        self.__name__ = 'pickle'


def _modules(obj):
    return getattr(obj, '_modules', {})


def _param(obj, name):
    for bag in ('_parameters', '_buffers'):
        d = getattr(obj, bag, None)
        if d is not None and name in d and d[name] is not None:
            return d[name]
    v = obj.__dict__.get(name)
    if v is None:
        raise KeyError(name)
    return v


def _np32(t):
    return t.detach().float().cpu().numpy().astype(np.float32)


def _fold(conv_mod):
    """yolov5 Conv module (conv + bn [+ act]) -> (w, b) fp32, as fuse_conv_and_bn does."""
    mods = _modules(conv_mod)
    conv = mods['conv']
    w = _np32(_param(conv, 'weight')).astype(np.float64)
    c2 = w.shape[0]
    try:
        cb = _np32(_param(conv, 'bias')).astype(np.float64)
    except KeyError:
        cb = np.zeros(c2)
    if 'bn' not in mods:        # already fused
        return w.astype(np.float32), cb.astype(np.float32)
    bn = mods['bn']
    gamma = _np32(_param(bn, 'weight')).astype(np.float64)
    beta = _np32(_param(bn, 'bias')).astype(np.float64)
    mean = _np32(_param(bn, 'running_mean')).astype(np.float64)
    var = _np32(_param(bn, 'running_var')).astype(np.float64)
    eps = float(bn.__dict__.get('eps', 1e-3))
    # fp32 arithmetic in the same order as fuse_conv_and_bn
    scale = (gamma.astype(np.float32) / np.sqrt(np.float32(eps) + var.astype(np.float32))).astype(np.float32)
    wf = (scale[:, None] * w.astype(np.float32).reshape(c2, -1)).reshape(w.shape).astype(np.float32)
    bf = (scale * cb.astype(np.float32) +
          (beta.astype(np.float32) - gamma.astype(np.float32) * mean.astype(np.float32) /
           np.sqrt(var.astype(np.float32) + np.float32(eps)))).astype(np.float32)
    return wf, bf


def load_checkpoint(path):
    """
    Reads md_v5a.0.0.pt-style checkpoints: {'model': DetectionModel(yaml, model=Sequential[...])}.
    Returns YoloWeights (BN folded, fp32).
    """
    import torch
    ckpt = torch.load(path, map_location='cpu', weights_only=False, pickle_module=_PickleModule())
    model = ckpt['model'] if isinstance(ckpt, dict) and 'model' in ckpt else ckpt
    if isinstance(ckpt, dict) and ckpt.get('ema') is not None and not hasattr(model, 'yaml'):
        model = ckpt['ema']
    yaml = dict(model.__dict__['yaml'])
    if yolo_yaml.is_yolo11(yaml) or type(model).__module__.split('.')[0] == 'ultralytics':
        return _load_ultralytics(model, yaml, path)
    if yolo_yaml.is_yolov9(yaml):
        return _load_yolov9(model, yaml, path)
    if 'anchors' in yaml and not isinstance(yaml['anchors'], (list, tuple)):
        raise ValueError('checkpoint yaml has no explicit anchor list')
    seq = _modules(model)['model']
    layers = _modules(seq)
    specs = resolve_yaml(yaml)
    w = {}
    for s in specs:
        mod = layers[str(s.index)]
        if s.type == MDHIP_DETECT:
            ml = _modules(_modules(mod)['m'])
            for l, name in enumerate(s.conv_names):
                w[name + '.weight'] = _np32(_param(ml[str(l)], 'weight'))
                w[name + '.bias'] = _np32(_param(ml[str(l)], 'bias'))
            w['model.{}.anchors'.format(s.index)] = _np32(_param(mod, 'anchors'))
            continue
        for name in s.conv_names:
            sub = mod
            for part in name.split('.')[2:-1]:        # e.g. 'cv1' / 'm','0','cv1'
                sub = _modules(sub)[part]
            wf, bf = _fold(sub)
            w[name + '.weight'] = wf
            w[name + '.bias'] = bf
    names = model.__dict__.get('names')
    if isinstance(names, (list, tuple)):
        names = {i: n for i, n in enumerate(names)}
    return YoloWeights(yaml, w, names=names, source=path)


def _load_ultralytics(model, yaml, path):
    """
    An ultralytics checkpoint (MDv1000-larch / -sorrel: {'model': DetectionModel}, model.yaml = the yolo11 yaml dict with
    'scale').  What the reference runs is model.float().fuse() (pytorch_detector.py:957): every Conv / DWConv -- the
    Attention's qkv / proj / pe included -- with its BatchNorm folded; the Detect head's final Conv2d layers and the DFL
    conv have no BatchNorm.  The head must be the current one (class branch DWConv -> Conv -> DWConv -> Conv -> Conv2d):
    the older 'legacy' head (Conv 3x3 -> Conv 3x3 -> Conv2d) is refused.
    """
    if not yolo_yaml.is_yolo11(yaml):
        raise ValueError('{}: ultralytics checkpoint without a YOLO11 model description'.format(path))
    specs = resolve_yaml(yaml)           # refuses other ultralytics modules (cedar = YOLOv9c) by name
    layers = _modules(_modules(model)['model'])
    det = specs[-1]
    if det.type != MDHIP_DETECT_DFL:
        raise ValueError('{}: the last layer is not an anchor-free Detect head'.format(path))
    dmod = layers[str(det.index)]
    dm = _modules(dmod)
    if 'cv3' not in dm or 'dfl' not in dm:
        raise ValueError('{}: Detect head without cv3 / dfl'.format(path))
    for l in range(len(det.frm)):
        branch = _modules(_modules(dm['cv3'])[str(l)])
        first = branch.get('0')
        if first is None or 'conv' in _modules(first) or '0' not in _modules(first):
            raise ValueError('{}: legacy YOLO11 Detect head (class branch without DWConv) is not supported; only the '
                             'current head (DWConv 3x3 -> Conv 1x1 -> DWConv 3x3 -> Conv 1x1 -> Conv2d) is'.format(path))
    if getattr(dmod, 'end2end', False):
        raise ValueError('{}: end-to-end (one-to-one) Detect heads are not supported'.format(path))
    reg_max = int(getattr(dmod, 'reg_max', 16))
    dfl_w = _np32(_param(_modules(dm['dfl'])['conv'], 'weight')).reshape(-1)
    if reg_max != 16 or dfl_w.shape != (16,) or not np.array_equal(dfl_w, np.arange(16, dtype=np.float32)):
        raise ValueError('{}: DFL conv weight must be arange(16) (reg_max 16)'.format(path))
    w = {}
    for s in specs:
        mod = layers[str(s.index)]
        for name in s.conv_names:
            sub = mod
            parts = name.split('.')[2:]
            for part in (parts[:-1] if parts[-1] == 'conv' else parts):
                sub = _modules(sub)[part]
            if parts[-1] == 'conv':
                wf, bf = _fold(sub)
            else:                                         # a plain Conv2d of the Detect head (bias, no BatchNorm)
                wf = _np32(_param(sub, 'weight'))
                bf = _np32(_param(sub, 'bias'))
            w[name + '.weight'] = wf
            w[name + '.bias'] = bf
    w['model.{}.dfl.conv.weight'.format(det.index)] = dfl_w.reshape(1, 16, 1, 1)
    names = model.__dict__.get('names')
    if isinstance(names, (list, tuple)):
        names = {i: n for i, n in enumerate(names)}
    return YoloWeights(yaml, w, names=names, source=path)


def _fold_repconvn(mod):
    """
    yolov9 RepConvN (conv1: Conv 3x3 + BN, conv2: Conv 1x1 + BN, no identity branch, then SiLU) -> one 3x3 (w, b) fp32,
    as its fuse_convs() does: both branches BN-folded, the 1x1 kernel added at the centre tap, the biases summed.
    A module that is already fused (a plain `conv`) is read as it is.
    """
    mods = _modules(mod)
    if 'conv1' not in mods:
        return _fold(mod)
    if mods.get('bn') is not None:
        raise ValueError('RepConvN with an identity BatchNorm branch is not supported')
    w3, b3 = _fold(mods['conv1'])
    w1, b1 = _fold(mods['conv2'])
    if w3.shape[2:] != (3, 3) or w1.shape[2:] != (1, 1):
        raise ValueError('RepConvN: 3x3 and 1x1 branches expected, got {} / {}'.format(w3.shape, w1.shape))
    w = w3.copy()
    w[:, :, 1, 1] += w1[:, :, 0, 0]
    return w.astype(np.float32), (b3 + b1).astype(np.float32)


def _load_yolov9(model, yaml, path):
    """
    A yolov9-package checkpoint (MDv1000-cedar: {'model': models.yolo.DetectionModel} -- or the same under `yolov9.` --
    with model.yaml in the YOLOv5 format).  What the reference runs is model.float().fuse() (pytorch_detector.py:957):
    every Conv with its BatchNorm folded, every RepConvN folded into one 3x3 conv, the Detect head's grouped box conv as
    it is ([c2][c2 / 4][3][3]), its final Conv2d layers and CBLinear as plain convs with bias (no BatchNorm, no
    activation).  Both head forms load: DDetect (converted, GELAN-C) and DualDDetect (training form).
    """
    root = type(model).__module__.split('.')[0]
    if root not in ('models', 'yolov9'):
        raise ValueError('{}: yolov9 model description in a checkpoint of package "{}" (models.* or yolov9.* expected)'.format(
            path, type(model).__module__))
    specs = resolve_yaml(yaml)           # refuses unknown modules by name
    layers = _modules(_modules(model)['model'])
    det = specs[-1]
    dmod = layers[str(det.index)]
    dm = _modules(dmod)
    reg_max = int(getattr(dmod, 'reg_max', 16))
    dfl = {}
    for h in range(det.n):
        key = 'dfl' if h == 0 else 'dfl{}'.format(h + 1)
        if key not in dm:
            raise ValueError('{}: Detect head without {}'.format(path, key))
        dfl_w = _np32(_param(_modules(dm[key])['conv'], 'weight')).reshape(-1)
        if reg_max != 16 or dfl_w.shape != (16,) or not np.array_equal(dfl_w, np.arange(16, dtype=np.float32)):
            raise ValueError('{}: DFL conv weight must be arange(16) (reg_max 16)'.format(path))
        dfl['model.{}.{}.conv.weight'.format(det.index, key)] = dfl_w.reshape(1, 16, 1, 1)
    w = {}
    for s in specs:
        if not s.conv_names:
            continue
        mod = layers[str(s.index)]
        for name in s.conv_names:
            sub = mod
            parts = name.split('.')[2:]
            for part in (parts[:-1] if parts[-1] == 'conv' else parts):
                sub = _modules(sub)[part]
            if parts[-1] == 'conv':
                wf, bf = _fold_repconvn(sub)
            else:                                         # a plain Conv2d of the Detect head (bias, no BatchNorm)
                wf = _np32(_param(sub, 'weight'))
                bf = _np32(_param(sub, 'bias'))
            w[name + '.weight'] = wf
            w[name + '.bias'] = bf
    w.update(dfl)
    names = model.__dict__.get('names')
    if isinstance(names, (list, tuple)):
        names = {i: n for i, n in enumerate(names)}
    return YoloWeights(yaml, w, names=names, source=path)


def read_metadata_from_megadetector_model_file(model_file):
    """
    reference pytorch_detector.py:674-731: optional '<root>/megadetector_info.json' inside the
    .pt zip (absent for MDv5).  Returns dict or None.
    """
    import json
    try:
        with zipfile.ZipFile(model_file, 'r') as z:
            names = z.namelist()
            roots = set(n.split('/')[0] for n in names)
            if len(roots) != 1:
                return None
            target = next(iter(roots)) + '/megadetector_info.json'
            if target not in names:
                return None
            return json.loads(z.read(target).decode('utf-8'))
    except Exception:
        return None
