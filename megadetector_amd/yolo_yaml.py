"""
YOLOv5 model descriptions (pure data) for the MegaDetector v5 family.

The MDv5a/b checkpoints are YOLOv5x6 (P6, 1280 px) networks: the reference never
states the topology in-tree, it unpickles the nn.Module out of md_v5a.0.0.pt
(reference: megadetector/detection/pytorch_detector.py:929,957) and relies on the
third-party package ultralytics-yolov5==0.1.1 (reference: pyproject.toml:70) for
models/hub/yolov5x6.yaml.  What follows is that published model description
restated as Python data (SURVEY.md section 8(a), P4 layer table).

Each row is [from, number, module, args] exactly as in the YOLOv5 yaml format.
"""

# Default P6 anchors in pixels (yolov5 hub/yolov5*6.yaml); real checkpoints carry
# their own (possibly auto-anchored) values which always take precedence.
ANCHORS_P6 = [
    [19, 27, 44, 40, 38, 94],        # P3/8
    [96, 68, 86, 152, 180, 137],     # P4/16
    [140, 301, 303, 264, 238, 542],  # P5/32
    [436, 615, 739, 380, 925, 792],  # P6/64
]

ANCHORS_P5 = [
    [10, 13, 16, 30, 33, 23],        # P3/8
    [30, 61, 62, 45, 59, 119],       # P4/16
    [116, 90, 156, 198, 373, 326],   # P5/32
]

_BACKBONE_P6 = [
    [-1, 1, 'Conv', [64, 6, 2, 2]],    # 0-P1/2
    [-1, 1, 'Conv', [128, 3, 2]],      # 1-P2/4
    [-1, 3, 'C3', [128]],
    [-1, 1, 'Conv', [256, 3, 2]],      # 3-P3/8
    [-1, 6, 'C3', [256]],
    [-1, 1, 'Conv', [512, 3, 2]],      # 5-P4/16
    [-1, 9, 'C3', [512]],
    [-1, 1, 'Conv', [768, 3, 2]],      # 7-P5/32
    [-1, 3, 'C3', [768]],
    [-1, 1, 'Conv', [1024, 3, 2]],     # 9-P6/64
    [-1, 3, 'C3', [1024]],
    [-1, 1, 'SPPF', [1024, 5]],        # 11
]

_HEAD_P6 = [
    [-1, 1, 'Conv', [768, 1, 1]],
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 8], 1, 'Concat', [1]],       # cat backbone P5
    [-1, 3, 'C3', [768, False]],       # 15
    [-1, 1, 'Conv', [512, 1, 1]],
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 6], 1, 'Concat', [1]],       # cat backbone P4
    [-1, 3, 'C3', [512, False]],       # 19
    [-1, 1, 'Conv', [256, 1, 1]],
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 4], 1, 'Concat', [1]],       # cat backbone P3
    [-1, 3, 'C3', [256, False]],       # 23 (P3/8-small)
    [-1, 1, 'Conv', [256, 3, 2]],
    [[-1, 20], 1, 'Concat', [1]],      # cat head P4
    [-1, 3, 'C3', [512, False]],       # 26 (P4/16-medium)
    [-1, 1, 'Conv', [512, 3, 2]],
    [[-1, 16], 1, 'Concat', [1]],      # cat head P5
    [-1, 3, 'C3', [768, False]],       # 29 (P5/32-large)
    [-1, 1, 'Conv', [768, 3, 2]],
    [[-1, 12], 1, 'Concat', [1]],      # cat head P6
    [-1, 3, 'C3', [1024, False]],      # 32 (P6/64-xlarge)
    [[23, 26, 29, 32], 1, 'Detect', ['nc', 'anchors']],
]

_BACKBONE_P5 = [
    [-1, 1, 'Conv', [64, 6, 2, 2]],    # 0-P1/2
    [-1, 1, 'Conv', [128, 3, 2]],      # 1-P2/4
    [-1, 3, 'C3', [128]],
    [-1, 1, 'Conv', [256, 3, 2]],      # 3-P3/8
    [-1, 6, 'C3', [256]],
    [-1, 1, 'Conv', [512, 3, 2]],      # 5-P4/16
    [-1, 9, 'C3', [512]],
    [-1, 1, 'Conv', [1024, 3, 2]],     # 7-P5/32
    [-1, 3, 'C3', [1024]],
    [-1, 1, 'SPPF', [1024, 5]],        # 9
]

_HEAD_P5 = [
    [-1, 1, 'Conv', [512, 1, 1]],
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 6], 1, 'Concat', [1]],
    [-1, 3, 'C3', [512, False]],       # 13
    [-1, 1, 'Conv', [256, 1, 1]],
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 4], 1, 'Concat', [1]],
    [-1, 3, 'C3', [256, False]],       # 17 (P3/8-small)
    [-1, 1, 'Conv', [256, 3, 2]],
    [[-1, 14], 1, 'Concat', [1]],
    [-1, 3, 'C3', [512, False]],       # 20 (P4/16-medium)
    [-1, 1, 'Conv', [512, 3, 2]],
    [[-1, 10], 1, 'Concat', [1]],
    [-1, 3, 'C3', [1024, False]],      # 23 (P5/32-large)
    [[17, 20, 23], 1, 'Detect', ['nc', 'anchors']],
]


def make_yaml(depth_multiple, width_multiple, nc=3, p6=True, anchors=None):
    """Build a YOLOv5 yaml dict (same keys as the dict pickled as model.yaml)."""
    return {
        'nc': nc,
        'depth_multiple': depth_multiple,
        'width_multiple': width_multiple,
        'anchors': [list(a) for a in (anchors or (ANCHORS_P6 if p6 else ANCHORS_P5))],
        'backbone': [list(r) for r in (_BACKBONE_P6 if p6 else _BACKBONE_P5)],
        'head': [list(r) for r in (_HEAD_P6 if p6 else _HEAD_P5)],
    }


#: MDv5a / MDv5b / MDv1000-redwood: YOLOv5x6, nc=3 (reference: run_detector.py:177-223)
YOLOV5X6_MD = make_yaml(1.33, 1.25, nc=3, p6=True)

#: upstream COCO model, used only to cross-check FLOP/param counts against the
#: figures the reference cites (docs/release-notes/mdv1000-release.md:279)
YOLOV5X6_COCO = make_yaml(1.33, 1.25, nc=80, p6=True)

#: MDv1000-spruce: YOLOv5s (P5, 3 heads) (reference: pytorch_detector.py:827,842)
YOLOV5S_MD = make_yaml(0.33, 0.50, nc=3, p6=False)

#: small P6 network for fast tests (same module mix as x6, ~1/60 of the FLOPs)
YOLOV5N6_TEST = make_yaml(0.33, 0.25, nc=3, p6=True)

#: wider small P6 network (hidden widths 64..256 at strides 8 and 16): exercises the kernels that need
#: at least 64 input channels (row-patch 3x3) in the tests
YOLOV5S6_TEST = make_yaml(0.33, 0.50, nc=3, p6=True)

#: small P5 (3 heads, stride 32) network with 5 classes: the non-P6 family members (MDv1000-spruce is a
#: YOLOv5s) and a class count other than 3, in the tests
YOLOV5N_P5_TEST = make_yaml(0.33, 0.25, nc=5, p6=False)


# --------------------------------------------------------------------------------------
# YOLO11 (anchor-free) descriptions: MDv1000-larch (YOLO11-L, 640 px) and MDv1000-sorrel (YOLO11-s, 960 px)
# (reference docs/release-notes/mdv1000-release.md:278-284, :317).  The reference loads them through the third-party
# ultralytics package (8.3.x); its published yolo11.yaml is restated here in the ultralytics yaml format [3P]:
# 'scales' maps a scale to [depth, width, max_channels], 'scale' names the one in use (the checkpoint's model.yaml
# carries both).
# --------------------------------------------------------------------------------------

YOLO11_SCALES = {
    'n': [0.50, 0.25, 1024],
    's': [0.50, 0.50, 1024],
    'm': [0.50, 1.00, 512],
    'l': [1.00, 1.00, 512],
    'x': [1.00, 1.50, 512],
}

_BACKBONE_YOLO11 = [
    [-1, 1, 'Conv', [64, 3, 2]],               # 0-P1/2
    [-1, 1, 'Conv', [128, 3, 2]],              # 1-P2/4
    [-1, 2, 'C3k2', [256, False, 0.25]],
    [-1, 1, 'Conv', [256, 3, 2]],              # 3-P3/8
    [-1, 2, 'C3k2', [512, False, 0.25]],
    [-1, 1, 'Conv', [512, 3, 2]],              # 5-P4/16
    [-1, 2, 'C3k2', [512, True]],
    [-1, 1, 'Conv', [1024, 3, 2]],             # 7-P5/32
    [-1, 2, 'C3k2', [1024, True]],
    [-1, 1, 'SPPF', [1024, 5]],                # 9
    [-1, 2, 'C2PSA', [1024]],                  # 10
]

_HEAD_YOLO11 = [
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 6], 1, 'Concat', [1]],               # cat backbone P4
    [-1, 2, 'C3k2', [512, False]],             # 13
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 4], 1, 'Concat', [1]],               # cat backbone P3
    [-1, 2, 'C3k2', [256, False]],             # 16 (P3/8-small)
    [-1, 1, 'Conv', [256, 3, 2]],
    [[-1, 13], 1, 'Concat', [1]],              # cat head P4
    [-1, 2, 'C3k2', [512, False]],             # 19 (P4/16-medium)
    [-1, 1, 'Conv', [512, 3, 2]],
    [[-1, 10], 1, 'Concat', [1]],              # cat head P5
    [-1, 2, 'C3k2', [1024, True]],             # 22 (P5/32-large)
    [[16, 19, 22], 1, 'Detect', ['nc']],       # 23 Detect(P3, P4, P5)
]


def make_yolo11_yaml(scale, nc=3):
    """A YOLO11 yaml dict (the keys ultralytics pickles as model.yaml) at one scale."""
    return {
        'nc': nc,
        'scales': {k: list(v) for k, v in YOLO11_SCALES.items()},
        'scale': scale,
        'backbone': [list(r) for r in _BACKBONE_YOLO11],
        'head': [list(r) for r in _HEAD_YOLO11],
    }


#: MDv1000-larch: YOLO11-L, nc = 3, 640 px
YOLO11L_MD = make_yolo11_yaml('l', nc=3)

#: MDv1000-sorrel: YOLO11-s, nc = 3, 960 px
YOLO11S_MD = make_yolo11_yaml('s', nc=3)

#: small YOLO11 for fast tests (scale n: the same module mix, C3k2 without C3k blocks, 2 attention heads)
YOLO11N_TEST = make_yolo11_yaml('n', nc=3)

#: the upstream COCO models, only to cross-check the work / parameter counts against the published figures
YOLO11N_COCO = make_yolo11_yaml('n', nc=80)
YOLO11S_COCO = make_yolo11_yaml('s', nc=80)
YOLO11L_COCO = make_yolo11_yaml('l', nc=80)


def is_yolo11(yaml):
    """True for an ultralytics (anchor-free) yaml dict, False for a YOLOv5 one."""
    return 'anchors' not in yaml and ('scales' in yaml or 'scale' in yaml)


# --------------------------------------------------------------------------------------
# YOLOv9-C descriptions: MDv1000-cedar (YOLOv9c, 640 px; reference docs/release-notes/mdv1000-release.md:280, :319).
# The reference runs it through the third-party yolov9pip package (WongKinYiu's YOLOv9 code, pytorch_detector.py:348-368),
# whose yaml format is the YOLOv5 one ('depth_multiple', 'width_multiple', 'anchors' an int).  Restated [3P] from the
# published yolov9-c.yaml; a leading Silence keeps the layer numbers of that file in both forms:
#   converted (GELAN-C): layers 0-22 and DDetect over (16, 19, 22) -- 25.3 M parameters, 102.1 GFLOPs at nc = 80;
#   training (yolov9-c.yaml): adds the reversible auxiliary branch (CBLinear 23-25, a second stem 26 reading layer 0,
#   CBFuse 30 / 33 / 36) and DualDDetect over (31, 34, 37, 16, 19, 22).
# --------------------------------------------------------------------------------------

_BACKBONE_YOLOV9C = [
    [-1, 1, 'Silence', []],                              # 0
    [-1, 1, 'Conv', [64, 3, 2]],                         # 1-P1/2
    [-1, 1, 'Conv', [128, 3, 2]],                        # 2-P2/4
    [-1, 1, 'RepNCSPELAN4', [256, 128, 64, 1]],          # 3
    [-1, 1, 'ADown', [256]],                             # 4-P3/8
    [-1, 1, 'RepNCSPELAN4', [512, 256, 128, 1]],         # 5
    [-1, 1, 'ADown', [512]],                             # 6-P4/16
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 7
    [-1, 1, 'ADown', [512]],                             # 8-P5/32
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 9
]

_HEAD_YOLOV9C = [
    [-1, 1, 'SPPELAN', [512, 256]],                      # 10
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 7], 1, 'Concat', [1]],                         # cat backbone P4
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 13
    [-1, 1, 'nn.Upsample', [None, 2, 'nearest']],
    [[-1, 5], 1, 'Concat', [1]],                         # cat backbone P3
    [-1, 1, 'RepNCSPELAN4', [256, 256, 128, 1]],         # 16 (P3/8-small)
    [-1, 1, 'ADown', [256]],
    [[-1, 13], 1, 'Concat', [1]],                        # cat head P4
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 19 (P4/16-medium)
    [-1, 1, 'ADown', [512]],
    [[-1, 10], 1, 'Concat', [1]],                        # cat head P5
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 22 (P5/32-large)
]

_AUX_YOLOV9C = [
    [5, 1, 'CBLinear', [[256]]],                         # 23
    [7, 1, 'CBLinear', [[256, 512]]],                    # 24
    [9, 1, 'CBLinear', [[256, 512, 512]]],               # 25
    [0, 1, 'Conv', [64, 3, 2]],                          # 26-P1/2
    [-1, 1, 'Conv', [128, 3, 2]],                        # 27-P2/4
    [-1, 1, 'RepNCSPELAN4', [256, 128, 64, 1]],          # 28
    [-1, 1, 'ADown', [256]],                             # 29-P3/8
    [[23, 24, 25, -1], 1, 'CBFuse', [[0, 0, 0]]],        # 30
    [-1, 1, 'RepNCSPELAN4', [512, 256, 128, 1]],         # 31
    [-1, 1, 'ADown', [512]],                             # 32-P4/16
    [[24, 25, -1], 1, 'CBFuse', [[1, 1]]],               # 33
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 34
    [-1, 1, 'ADown', [512]],                             # 35-P5/32
    [[25, -1], 1, 'CBFuse', [[2]]],                      # 36
    [-1, 1, 'RepNCSPELAN4', [512, 512, 256, 1]],         # 37
]


def _scaled_rows(rows, div):
    """channel arguments divided by `div` (small test networks with the same module mix)"""
    if div == 1:
        return [list(r) for r in rows]
    out = []
    for f, n, m, args in rows:
        if m in ('Conv', 'ADown'):
            args = [args[0] // div] + list(args[1:])
        elif m in ('RepNCSPELAN4', 'SPPELAN'):
            args = [a // div for a in args[:3]] + list(args[3:])
        elif m == 'CBLinear':
            args = [[c // div for c in args[0]]]
        out.append([f, n, m, list(args)])
    return out


def make_yolov9_yaml(nc=3, dual=False, div=1):
    """A YOLOv9-C yaml dict (the keys the yolov9 package pickles as model.yaml): converted (DDetect) or training
    (dual, DualDDetect) form; div > 1 divides every channel argument (test networks)."""
    head = _scaled_rows(_HEAD_YOLOV9C, div)
    if dual:
        head += _scaled_rows(_AUX_YOLOV9C, div) + [[[31, 34, 37, 16, 19, 22], 1, 'DualDDetect', ['nc']]]
    else:
        head += [[[16, 19, 22], 1, 'DDetect', ['nc']]]
    return {
        'nc': nc,
        'depth_multiple': 1.0,
        'width_multiple': 1.0,
        'anchors': 3,
        'backbone': _scaled_rows(_BACKBONE_YOLOV9C, div),
        'head': head,
    }


#: MDv1000-cedar, converted (GELAN-C) form: nc = 3, 640 px
GELAN_C_MD = make_yolov9_yaml(nc=3)
#: MDv1000-cedar, training (yolov9-c.yaml) form with the auxiliary branch and DualDDetect
YOLOV9C_MD = make_yolov9_yaml(nc=3, dual=True)
#: small networks of the same module mix for fast tests (channel arguments / 4)
GELAN_TEST = make_yolov9_yaml(nc=3, div=4)
YOLOV9_DUAL_TEST = make_yolov9_yaml(nc=3, dual=True, div=4)
#: the upstream COCO models, only to cross-check the work / parameter counts against the published figures
GELAN_C_COCO = make_yolov9_yaml(nc=80)
YOLOV9C_COCO = make_yolov9_yaml(nc=80, dual=True)

#: module names that only the yolov9 package's yaml format uses: they select the yolov9 resolver
YOLOV9_MODULES = ('RepNCSPELAN4', 'ADown', 'SPPELAN', 'CBLinear', 'CBFuse', 'DDetect', 'DualDDetect', 'Silence')


def is_yolov9(yaml):
    """True for a yolov9-package yaml dict: the YOLOv5 format (no 'scales') with at least one yolov9 module."""
    if 'scales' in yaml or 'scale' in yaml:
        return False
    rows = list(yaml.get('backbone') or []) + list(yaml.get('head') or [])
    return any(len(r) > 2 and r[2] in YOLOV9_MODULES for r in rows)
