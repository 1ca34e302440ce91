"""
A small, independent torch.nn implementation of the YOLOv9-C architecture (Conv / RepConvN with UNFUSED branches /
RepNBottleneck / RepNCSP / RepNCSPELAN4 / ADown / SP / SPPELAN / Concat / CBLinear / CBFuse / Silence / DFL / DDetect /
DualDDetect / DetectionModel), registered under the module names the yolov9 package pickles (`models.common`,
`models.yolo`), so that `torch.save({'model': model.half(), ...})` writes a file with the pickle layout of
md_v1000.0.0-cedar.pt: whole-module pickles naming classes of a package that is NOT importable when the file is read.
save_checkpoint adds the `megadetector_info.json` record of the MDv1000 files (model_type yolov9, image size 640).

Test infrastructure only, written from the published architecture description ([3P], the issue's statement of the yolov9
modules), not from the yolov9 sources.  Same job as tests/fake_yolov5.py, which installs modules under the same
`models.*` names: uninstall() removes them again.
"""

import json
import math
import sys
import types
import zipfile

import torch
import torch.nn as nn
import torch.nn.functional as F

_NAMES = ('models', 'models.common', 'models.yolo')


def _md(x, d):
    return int(math.ceil(x / d) * d)


def _install():
    """Creates (or returns) the fake yolov9 modules: (common, yolo)."""
    if 'models.yolo' in sys.modules and getattr(sys.modules['models.yolo'], '_mdhip_fake_v9', False):
        return sys.modules['models.common'], sys.modules['models.yolo']
    mods = {n: types.ModuleType(n) for n in _NAMES}
    mods['models'].__path__ = []
    common, yolo = mods['models.common'], mods['models.yolo']
    yolo._mdhip_fake_v9 = True

    class Conv(nn.Module):
        def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
            super().__init__()
            self.conv = nn.Conv2d(c1, c2, k, s, k // 2 if p is None else p, groups=g, bias=False)
            self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
            self.act = nn.SiLU() if act is True else nn.Identity()

        def forward(self, x):
            return self.act(self.bn(self.conv(x)))

    class Silence(nn.Module):
        def forward(self, x):
            return x

    class RepConvN(nn.Module):
        """3x3 + 1x1 branches, each with BatchNorm, summed, SiLU (no identity branch): NOT fused in the checkpoint"""

        def __init__(self, c1, c2, k=3, s=1, p=1):
            super().__init__()
            self.act = nn.SiLU()
            self.bn = None
            self.conv1 = Conv(c1, c2, k, s, p=p, act=False)
            self.conv2 = Conv(c1, c2, 1, s, p=p - k // 2, act=False)

        def forward(self, x):
            return self.act(self.conv1(x) + self.conv2(x))

    class RepNBottleneck(nn.Module):
        def __init__(self, c1, c2, shortcut=True, e=1.0):
            super().__init__()
            c_ = int(c2 * e)
            self.cv1 = RepConvN(c1, c_, 3, 1)
            self.cv2 = Conv(c_, c2, 3, 1)
            self.add = shortcut and c1 == c2

        def forward(self, x):
            return x + self.cv2(self.cv1(x)) if self.add else self.cv2(self.cv1(x))

    class RepNCSP(nn.Module):
        def __init__(self, c1, c2, n=1, shortcut=True, e=0.5):
            super().__init__()
            c_ = int(c2 * e)
            self.cv1 = Conv(c1, c_, 1, 1)
            self.cv2 = Conv(c1, c_, 1, 1)
            self.cv3 = Conv(2 * c_, c2, 1)
            self.m = nn.Sequential(*(RepNBottleneck(c_, c_, shortcut, e=1.0) for _ in range(n)))

        def forward(self, x):
            return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))

    class RepNCSPELAN4(nn.Module):
        def __init__(self, c1, c2, c3, c4, c5=1):
            super().__init__()
            self.c = c3 // 2
            self.cv1 = Conv(c1, c3, 1, 1)
            self.cv2 = nn.Sequential(RepNCSP(c3 // 2, c4, c5), Conv(c4, c4, 3, 1))
            self.cv3 = nn.Sequential(RepNCSP(c4, c4, c5), Conv(c4, c4, 3, 1))
            self.cv4 = Conv(c3 + 2 * c4, c2, 1, 1)

        def forward(self, x):
            y = list(self.cv1(x).chunk(2, 1))
            y.extend(m(y[-1]) for m in [self.cv2, self.cv3])
            return self.cv4(torch.cat(y, 1))

    class ADown(nn.Module):
        def __init__(self, c1, c2):
            super().__init__()
            self.c = c2 // 2
            self.cv1 = Conv(c1 // 2, self.c, 3, 2, 1)
            self.cv2 = Conv(c1 // 2, self.c, 1, 1, 0)

        def forward(self, x):
            x = F.avg_pool2d(x, 2, 1, 0, False, True)
            x1, x2 = x.chunk(2, 1)
            x1 = self.cv1(x1)
            x2 = self.cv2(F.max_pool2d(x2, 3, 2, 1))
            return torch.cat((x1, x2), 1)

    class SP(nn.Module):
        def __init__(self, k=5, s=1):
            super().__init__()
            self.m = nn.MaxPool2d(kernel_size=k, stride=s, padding=k // 2)

        def forward(self, x):
            return self.m(x)

    class SPPELAN(nn.Module):
        def __init__(self, c1, c2, c3):
            super().__init__()
            self.c = c3
            self.cv1 = Conv(c1, c3, 1, 1)
            self.cv2, self.cv3, self.cv4 = SP(5), SP(5), SP(5)
            self.cv5 = Conv(4 * c3, c2, 1, 1)

        def forward(self, x):
            y = [self.cv1(x)]
            y.extend(m(y[-1]) for m in [self.cv2, self.cv3, self.cv4])
            return self.cv5(torch.cat(y, 1))

    class Concat(nn.Module):
        def __init__(self, dimension=1):
            super().__init__()
            self.d = dimension

        def forward(self, x):
            return torch.cat(x, self.d)

    class CBLinear(nn.Module):
        def __init__(self, c1, c2s):
            super().__init__()
            self.c2s = c2s
            self.conv = nn.Conv2d(c1, sum(c2s), 1, 1, 0, bias=True)

        def forward(self, x):
            return self.conv(x).split(self.c2s, dim=1)

    class CBFuse(nn.Module):
        def __init__(self, idx):
            super().__init__()
            self.idx = idx

        def forward(self, xs):
            size = xs[-1].shape[2:]
            res = [F.interpolate(x[self.idx[i]], size=size, mode='nearest') for i, x in enumerate(xs[:-1])]
            return torch.sum(torch.stack(res + xs[-1:]), dim=0)

    class DFL(nn.Module):
        def __init__(self, c1=16):
            super().__init__()
            self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
            self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
            self.c1 = c1

        def forward(self, x):
            b, _, a = x.shape
            return self.conv(x.view(b, 4, self.c1, a).transpose(2, 1).softmax(1)).view(b, 4, a)

    def _branches(ch, nc, reg_max):
        c2, c3 = _md(max(ch[0] // 4, reg_max * 4, 16), 4), max(ch[0], min(nc * 2, 128))
        box = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3, g=4), nn.Conv2d(c2, 4 * reg_max, 1)) for x in ch)
        cls = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, nc, 1)) for x in ch)
        return box, cls

    def _decode(xs, box_l, cls_l, dfl, strides, nc, reg_max):
        """(B, 4 + nc, anchors): [cx, cy, w, h] in pixels and sigmoid class scores (the yolov9 inference layout)"""
        outs, anchors, sts = [], [], []
        for i, x in enumerate(xs):
            y = torch.cat((box_l[i](x), cls_l[i](x)), 1)
            b, _, h, w = y.shape
            outs.append(y.view(b, 4 * reg_max + nc, -1))
            sy, sx = torch.meshgrid(torch.arange(h, dtype=torch.float) + 0.5, torch.arange(w, dtype=torch.float) + 0.5,
                                    indexing='ij')
            anchors.append(torch.stack((sx, sy), -1).view(-1, 2))
            sts.append(torch.full((h * w, 1), float(strides[i])))
        y = torch.cat(outs, 2)
        anchors = torch.cat(anchors).transpose(0, 1).unsqueeze(0)
        sts = torch.cat(sts).transpose(0, 1)
        box, cls = y.split((reg_max * 4, nc), 1)
        lt, rb = dfl(box).chunk(2, 1)
        x1y1, x2y2 = anchors - lt, anchors + rb
        return torch.cat((torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * sts, cls.sigmoid()), 1)

    class DDetect(nn.Module):
        def __init__(self, nc, ch):
            super().__init__()
            self.nc, self.nl, self.reg_max = nc, len(ch), 16
            self.stride = torch.zeros(self.nl)
            self.cv2, self.cv3 = _branches(ch, nc, self.reg_max)
            self.dfl = DFL(self.reg_max)

        def forward(self, xs):
            return _decode(xs, self.cv2, self.cv3, self.dfl, self.stride, self.nc, self.reg_max)

    class DualDDetect(nn.Module):
        def __init__(self, nc, ch):
            super().__init__()
            self.nc, self.nl, self.reg_max = nc, len(ch) // 2, 16
            self.stride = torch.zeros(self.nl)
            self.cv2, self.cv3 = _branches(ch[:self.nl], nc, self.reg_max)
            self.cv4, self.cv5 = _branches(ch[self.nl:], nc, self.reg_max)
            self.dfl = DFL(self.reg_max)
            self.dfl2 = DFL(self.reg_max)

        def forward(self, xs):
            return [_decode(xs[:self.nl], self.cv2, self.cv3, self.dfl, self.stride, self.nc, self.reg_max),
                    _decode(xs[self.nl:], self.cv4, self.cv5, self.dfl2, self.stride, self.nc, self.reg_max)]

    class DetectionModel(nn.Module):
        def __init__(self, yaml):
            super().__init__()
            self.yaml = dict(yaml)
            nc = yaml['nc']
            ch, layers, divs = [3], [], []
            for i, (f, n, m, args) in enumerate(list(yaml['backbone']) + list(yaml['head'])):
                src = f if isinstance(f, int) else f[-1]
                d_in = 1 if (src == -1 and i == 0) else divs[src if src >= 0 else i + src]
                c1 = ch[f] if isinstance(f, int) else None
                d_out = d_in
                if m == 'Silence':
                    mod, c2 = Silence(), c1
                elif m == 'Conv':
                    c2 = args[0]
                    mod = Conv(c1, c2, *args[1:])
                    d_out = d_in * (args[2] if len(args) > 2 else 1)
                elif m == 'RepNCSPELAN4':
                    c2 = args[0]
                    mod = RepNCSPELAN4(c1, *args)
                elif m == 'ADown':
                    c2 = args[0]
                    mod = ADown(c1, c2)
                    d_out = d_in * 2
                elif m == 'SPPELAN':
                    c2 = args[0]
                    mod = SPPELAN(c1, *args)
                elif m == 'nn.Upsample':
                    c2 = c1
                    mod = nn.Upsample(None, args[1], args[2])
                    d_out = d_in // 2
                elif m == 'Concat':
                    c2 = sum(ch[x] for x in f)
                    mod = Concat(args[0])
                elif m == 'CBLinear':
                    c2 = list(args[0])
                    mod = CBLinear(c1, c2)
                elif m == 'CBFuse':
                    c2 = ch[f[-1]]
                    mod = CBFuse(args[0])
                elif m in ('DDetect', 'DualDDetect'):
                    mod = (DDetect if m == 'DDetect' else DualDDetect)(nc, [ch[x] for x in f])
                    mod.stride = torch.tensor([float(divs[x]) for x in f[:mod.nl]])
                    c2 = None
                else:
                    raise ValueError(m)
                mod.i, mod.f, mod.type = i, f, m
                layers.append(mod)
                if i == 0:
                    ch = []
                ch.append(c2)
                divs.append(d_out)
            self.model = nn.Sequential(*layers)
            self.stride = layers[-1].stride
            self.names = {0: 'animal', 1: 'person', 2: 'vehicle'} if nc == 3 else {i: str(i) for i in range(nc)}

        def forward(self, x):
            """eval-mode output: (y, None) as model(x)[0] is what the reference passes on (DualDDetect: the list)"""
            y = []
            for m in self.model:
                if m.f != -1:
                    x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
                x = m(x)
                y.append(x)
            return x, None

    for cls in (Conv, Silence, RepConvN, RepNBottleneck, RepNCSP, RepNCSPELAN4, ADown, SP, SPPELAN, Concat, CBLinear,
                CBFuse, DFL):
        cls.__module__ = 'models.common'
    for cls in (DDetect, DualDDetect, DetectionModel):
        cls.__module__ = 'models.yolo'
    for cls in (Conv, Silence, RepConvN, RepNBottleneck, RepNCSP, RepNCSPELAN4, ADown, SP, SPPELAN, Concat, CBLinear,
                CBFuse, DFL, DDetect, DualDDetect, DetectionModel):
        cls.__qualname__ = cls.__name__
        setattr(mods[cls.__module__], cls.__name__, cls)
    mods['models'].common, mods['models'].yolo = common, yolo
    for n, m in mods.items():
        sys.modules[n] = m
    return common, yolo


def uninstall():
    for name in _NAMES:
        sys.modules.pop(name, None)


def build_model(yaml, seed=0, gain=1.5, res_gain=0.5, cls_bias=-4.0):
    """
    A DetectionModel with random conv weights AND non-trivial BatchNorm statistics (RepConvN branches unfused), in eval
    mode, fp16-representable (the checkpoint stores fp16).
    """
    common, yolo = _install()
    torch.manual_seed(seed)
    model = yolo.DetectionModel(yaml)
    g = torch.Generator().manual_seed(seed + 1)
    residual_end = {id(m.cv2) for m in model.modules() if isinstance(m, common.RepNBottleneck) and m.add}
    for m in model.modules():
        if isinstance(m, common.Conv):
            w = torch.randn(m.conv.weight.shape, generator=g)
            w -= w.mean(dim=(1, 2, 3), keepdim=True)
            fan = w.shape[1] * w.shape[2] * w.shape[3]
            gc = res_gain if id(m) in residual_end else (gain if isinstance(m.act, nn.SiLU) else 1.0)
            nf = m.bn.num_features
            m.bn.weight.data = 0.8 + 0.4 * torch.rand(nf, generator=g)
            m.bn.bias.data = 0.1 * torch.randn(nf, generator=g)
            m.bn.running_mean.data = 0.1 * torch.randn(nf, generator=g)
            m.bn.running_var.data = 0.7 + 0.6 * torch.rand(nf, generator=g)
            m.conv.weight.data = w * (gc / fan ** 0.5)
        elif isinstance(m, common.CBLinear):
            m.conv.weight.data = torch.randn(m.conv.weight.shape, generator=g) / m.conv.weight.shape[1] ** 0.5
            m.conv.bias.data = 0.1 * torch.randn(m.conv.bias.shape, generator=g)
        elif isinstance(m, (yolo.DDetect, yolo.DualDDetect)):
            pairs = [(m.cv2, m.cv3)] + ([(m.cv4, m.cv5)] if isinstance(m, yolo.DualDDetect) else [])
            for box, cls in pairs:
                for seq in box:
                    seq[2].weight.data = torch.randn(seq[2].weight.shape, generator=g) * (0.5 / seq[2].weight.shape[1] ** 0.5)
                    seq[2].bias.data = 0.5 * torch.randn(seq[2].bias.shape, generator=g)
                for seq in cls:
                    seq[2].weight.data = torch.randn(seq[2].weight.shape, generator=g) * (1.5 / seq[2].weight.shape[1] ** 0.5)
                    seq[2].bias.data = cls_bias + 0.5 * torch.randn(seq[2].bias.shape, generator=g)
    model = model.half().float()                   # what the checkpoint holds
    return model.eval()


def save_checkpoint(model, path, image_size=640):
    """the yolov9 container ({'model': fp16 module, ...}) plus <root>/megadetector_info.json"""
    import copy
    import os
    ck = {'epoch': -1, 'best_fitness': None, 'model': copy.deepcopy(model).half(), 'ema': None, 'updates': None,
          'optimizer': None, 'opt': {}, 'git': None, 'date': '2024-01-01T00:00:00'}
    for p in ck['model'].parameters():
        p.requires_grad = False
    torch.save(ck, path)
    with zipfile.ZipFile(path, 'r') as z:
        root = z.namelist()[0].split('/')[0]
    with zipfile.ZipFile(path, 'a') as z:
        z.writestr(root + '/megadetector_info.json', json.dumps({'image_size': int(image_size), 'model_type': 'yolov9',
                                                                 'model_name': os.path.basename(path)}))


def sparsify_classes(model, xs, conf_thr=0.005, per_row=(1, 4), logit_std=2.0):
    """tests/fake_ultralytics.py:sparsify_classes for the head whose output is post-processed (cv3: DDetect, and the first
    head of DualDDetect)"""
    common, yolo = _install()
    det = [m for m in model.modules() if isinstance(m, (yolo.DDetect, yolo.DualDDetect))][0]
    need = math.log(conf_thr / (1 - conf_thr))
    with torch.no_grad():
        feats = {i: [] for i in range(det.nl)}
        hooks = [seq[2].register_forward_pre_hook(lambda mod, inp, i=i: feats[i].append(inp[0].detach().double()))
                 for i, seq in enumerate(det.cv3)]
        for x in xs:
            model(x)
        for h in hooks:
            h.remove()
        for i, seq in enumerate(det.cv3):
            conv = seq[2]
            f = torch.cat([t.permute(1, 0, 2, 3).reshape(t.shape[1], -1) for t in feats[i]], 1)
            fbar = f.mean(1)
            for c in range(conv.weight.shape[0]):
                w0 = conv.weight.data[c].view(-1).double()
                b1 = float(conv.bias.data[c]) + float(w0 @ fbar)
                w1 = w0 - (w0 @ fbar) / (fbar @ fbar) * fbar
                w2 = (logit_std / float((w1 @ f).std()) * w1).half().double()
                logit = torch.sort(w2 @ f + b1, descending=True)[0]
                best = None
                for k in range(per_row[0], per_row[1] + 1):
                    gap = float(logit[k - 1] - logit[k])
                    if best is None or gap > best[0]:
                        best = (gap, float(need - 0.5 * float(logit[k - 1] + logit[k])))
                conv.weight.data[c] = w2.float().view(conv.weight.data[c].shape)
                conv.bias.data[c] = float(torch.tensor(b1 + best[1]).half())
    return model
