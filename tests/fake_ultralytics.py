"""
A small, independent torch.nn implementation of the YOLO11 architecture (Conv / DWConv / Bottleneck / C3k / C3k2 /
SPPF / Attention / PSABlock / C2PSA / Concat / DFL / Detect / DetectionModel), registered under the module names the
ultralytics package uses (`ultralytics.nn.modules.conv`, `.block`, `.head`, `ultralytics.nn.tasks`), so that
`torch.save({'model': model.half(), ...})` writes a file with the pickle layout of md_v1000.0.0-larch.pt / -sorrel.pt:
whole-module pickles naming classes of a package that is NOT importable when the file is read.  save_checkpoint adds
the `megadetector_info.json` record the MDv1000 files carry (image size 640 / 960).

Test infrastructure only, written from the published architecture description (the issue's statement of yolo11.yaml
and its blocks, [3P]), not from the ultralytics sources.  Same job as tests/fake_yolov5.py.
"""

import json
import math
import sys
import types
import zipfile

import torch
import torch.nn as nn

_NAMES = ('ultralytics', 'ultralytics.nn', 'ultralytics.nn.modules', 'ultralytics.nn.modules.conv',
          'ultralytics.nn.modules.block', 'ultralytics.nn.modules.head', 'ultralytics.nn.tasks')


def _install():
    """Creates (or returns) the fake ultralytics modules: (conv, block, head, tasks)."""
    if 'ultralytics.nn.tasks' in sys.modules and getattr(sys.modules['ultralytics.nn.tasks'], '_mdhip_fake', False):
        return tuple(sys.modules[n] for n in _NAMES[3:])
    mods = {}
    for n in _NAMES:
        m = types.ModuleType(n)
        m.__path__ = []
        mods[n] = m
    conv_m, block_m, head_m, tasks_m = (mods[n] for n in _NAMES[3:])
    tasks_m._mdhip_fake = True

    class Conv(nn.Module):
        def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
            super().__init__()
            self.conv = nn.Conv2d(c1, c2, k, s, k // 2 if p is None else p, groups=g, bias=False)
            self.bn = nn.BatchNorm2d(c2, eps=1e-3, momentum=0.03)
            self.act = nn.SiLU() if act is True else nn.Identity()

        def forward(self, x):
            return self.act(self.bn(self.conv(x)))

    class DWConv(Conv):
        def __init__(self, c1, c2, k=1, s=1, act=True):
            super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), act=act)

    class Concat(nn.Module):
        def __init__(self, dimension=1):
            super().__init__()
            self.d = dimension

        def forward(self, xs):
            return torch.cat(xs, self.d)

    class Bottleneck(nn.Module):
        def __init__(self, c1, c2, shortcut=True, e=0.5):
            super().__init__()
            c_ = int(c2 * e)
            self.cv1 = Conv(c1, c_, 3, 1)
            self.cv2 = Conv(c_, c2, 3, 1)
            self.add = shortcut and c1 == c2

        def forward(self, x):
            y = self.cv2(self.cv1(x))
            return x + y if self.add else y

    class C3k(nn.Module):
        def __init__(self, c1, c2, n=2, shortcut=True, e=0.5):
            super().__init__()
            c_ = int(c2 * e)
            self.cv1 = Conv(c1, c_, 1, 1)
            self.cv2 = Conv(c1, c_, 1, 1)
            self.cv3 = Conv(2 * c_, c2, 1)
            self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, e=1.0) for _ in range(n)))

        def forward(self, x):
            return self.cv3(torch.cat((self.m(self.cv1(x)), self.cv2(x)), 1))

    class C3k2(nn.Module):
        def __init__(self, c1, c2, n=1, c3k=False, e=0.5, shortcut=True):
            super().__init__()
            self.c = int(c2 * e)
            self.cv1 = Conv(c1, 2 * self.c, 1, 1)
            self.cv2 = Conv((2 + n) * self.c, c2, 1)
            self.m = nn.ModuleList(C3k(self.c, self.c, 2, shortcut) if c3k else Bottleneck(self.c, self.c, shortcut)
                                   for _ in range(n))

        def forward(self, x):
            y = list(self.cv1(x).chunk(2, 1))
            y.extend(m(y[-1]) for m in self.m)
            return self.cv2(torch.cat(y, 1))

    class SPPF(nn.Module):
        def __init__(self, c1, c2, k=5):
            super().__init__()
            c_ = c1 // 2
            self.cv1 = Conv(c1, c_, 1, 1)
            self.cv2 = Conv(c_ * 4, c2, 1, 1)
            self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

        def forward(self, x):
            y = [self.cv1(x)]
            y.extend(self.m(y[-1]) for _ in range(3))
            return self.cv2(torch.cat(y, 1))

    class Attention(nn.Module):
        def __init__(self, dim, num_heads=8, attn_ratio=0.5):
            super().__init__()
            self.num_heads = num_heads
            self.head_dim = dim // num_heads
            self.key_dim = int(self.head_dim * attn_ratio)
            self.scale = self.key_dim ** -0.5
            h = dim + self.key_dim * num_heads * 2
            self.qkv = Conv(dim, h, 1, act=False)
            self.proj = Conv(dim, dim, 1, act=False)
            self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

        def forward(self, x):
            B, C, H, W = x.shape
            N = H * W
            qkv = self.qkv(x)
            q, k, v = qkv.view(B, self.num_heads, self.key_dim * 2 + self.head_dim, N).split(
                [self.key_dim, self.key_dim, self.head_dim], dim=2)
            attn = (q.transpose(-2, -1) @ k) * self.scale
            attn = attn.softmax(dim=-1)
            x = (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self.pe(v.reshape(B, C, H, W))
            return self.proj(x)

    class PSABlock(nn.Module):
        def __init__(self, c, attn_ratio=0.5, num_heads=4, shortcut=True):
            super().__init__()
            self.attn = Attention(c, attn_ratio=attn_ratio, num_heads=num_heads)
            self.ffn = nn.Sequential(Conv(c, c * 2, 1), Conv(c * 2, c, 1, act=False))
            self.add = shortcut

        def forward(self, x):
            x = x + self.attn(x) if self.add else self.attn(x)
            return x + self.ffn(x) if self.add else self.ffn(x)

    class C2PSA(nn.Module):
        def __init__(self, c1, c2, n=1, e=0.5):
            super().__init__()
            assert c1 == c2
            self.c = int(c1 * e)
            self.cv1 = Conv(c1, 2 * self.c, 1, 1)
            self.cv2 = Conv(2 * self.c, c1, 1)
            self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

        def forward(self, x):
            a, b = self.cv1(x).split((self.c, self.c), dim=1)
            b = self.m(b)
            return self.cv2(torch.cat((a, b), 1))

    class DFL(nn.Module):
        def __init__(self, c1=16):
            super().__init__()
            self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
            self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
            self.c1 = c1

        def forward(self, x):
            b, _, a = x.shape
            return self.conv(x.view(b, 4, self.c1, a).transpose(2, 1).softmax(1)).view(b, 4, a)

    class Detect(nn.Module):
        def __init__(self, nc, ch, legacy=False):
            super().__init__()
            self.nc, self.nl, self.reg_max = nc, len(ch), 16
            self.no = nc + self.reg_max * 4
            self.stride = torch.zeros(self.nl)
            c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], min(self.nc, 100))
            self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * self.reg_max, 1))
                                     for x in ch)
            if legacy:
                self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, self.nc, 1)) for x in ch)
            else:
                self.cv3 = nn.ModuleList(nn.Sequential(nn.Sequential(DWConv(x, x, 3), Conv(x, c3, 1)),
                                                       nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)),
                                                       nn.Conv2d(c3, self.nc, 1)) for x in ch)
            self.dfl = DFL(self.reg_max)
            self.legacy = legacy
            self.end2end = False

        def forward(self, xs):
            """(B, anchors, 4 + nc): [cx, cy, w, h] in pixels and sigmoid class scores (the inference output, transposed)"""
            outs, anchors, strides = [], [], []
            for i in range(self.nl):
                x = torch.cat((self.cv2[i](xs[i]), self.cv3[i](xs[i])), 1)
                b, _, h, w = x.shape
                outs.append(x.view(b, self.no, -1))
                sy, sx = torch.meshgrid(torch.arange(h, dtype=torch.float) + 0.5, torch.arange(w, dtype=torch.float) + 0.5,
                                        indexing='ij')
                anchors.append(torch.stack((sx, sy), -1).view(-1, 2))
                strides.append(torch.full((h * w, 1), float(self.stride[i])))
            x = torch.cat(outs, 2)
            anchors = torch.cat(anchors).transpose(0, 1).unsqueeze(0)
            strides = torch.cat(strides).transpose(0, 1)
            box, cls = x.split((self.reg_max * 4, self.nc), 1)
            d = self.dfl(box)
            lt, rb = d.chunk(2, 1)
            x1y1, x2y2 = anchors - lt, anchors + rb
            dbox = torch.cat(((x1y1 + x2y2) / 2, x2y2 - x1y1), 1) * strides
            return torch.cat((dbox, cls.sigmoid()), 1).transpose(1, 2)

    class DetectionModel(nn.Module):
        def __init__(self, yaml, legacy=False):
            super().__init__()
            self.yaml = dict(yaml)
            nc = yaml['nc']
            depth, width, max_ch = yaml['scales'][yaml['scale']]
            ch, layers, divs = [3], [], []
            for i, (f, n, m, args) in enumerate(list(yaml['backbone']) + list(yaml['head'])):
                n = max(round(n * depth), 1) if n > 1 else n
                div = lambda c: int(math.ceil(min(c, max_ch) * width / 8) * 8)
                src = f if isinstance(f, int) else f[0]
                c1 = ch[f] if isinstance(f, int) else None
                d_in = 1 if i == 0 else divs[src if src >= 0 else i + src]
                d_out = d_in
                if m == 'Conv':
                    c2 = div(args[0])
                    mod = Conv(c1, c2, *args[1:])
                    d_out = d_in * (args[2] if len(args) > 2 else 1)
                elif m == 'C3k2':
                    c2 = div(args[0])
                    c3k = (args[1] if len(args) > 1 else False) or yaml['scale'] in 'mlx'
                    mod = C3k2(c1, c2, n, c3k, *(args[2:3]))
                elif m == 'SPPF':
                    c2 = div(args[0])
                    mod = SPPF(c1, c2, *args[1:])
                elif m == 'C2PSA':
                    c2 = div(args[0])
                    mod = C2PSA(c1, c2, n)
                elif m == 'nn.Upsample':
                    c2 = c1
                    mod = nn.Upsample(None, args[1], args[2])
                    d_out = d_in // 2
                elif m == 'Concat':
                    c2 = sum(ch[x] for x in f)
                    mod = Concat(args[0])
                elif m == 'Detect':
                    mod = Detect(nc, [ch[x] for x in f], legacy=legacy)
                    mod.stride = torch.tensor([float(divs[x]) for x in f])
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
            self.save = sorted(set(x % len(layers) for m in layers for x in ([m.f] if isinstance(m.f, int) else m.f)
                                   if x != -1))
            self.stride = layers[-1].stride
            self.names = {0: 'animal', 1: 'person', 2: 'vehicle'} if nc == 3 else {i: str(i) for i in range(nc)}

        def forward(self, x):
            y = []
            for m in self.model:
                if m.f != -1:
                    x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
                x = m(x)
                y.append(x if m.i in self.save else None)
            return x

    for cls in (Conv, DWConv, Concat):
        cls.__module__ = 'ultralytics.nn.modules.conv'
    for cls in (Bottleneck, C3k, C3k2, SPPF, Attention, PSABlock, C2PSA, DFL):
        cls.__module__ = 'ultralytics.nn.modules.block'
    Detect.__module__ = 'ultralytics.nn.modules.head'
    DetectionModel.__module__ = 'ultralytics.nn.tasks'
    for cls in (Conv, DWConv, Concat, Bottleneck, C3k, C3k2, SPPF, Attention, PSABlock, C2PSA, DFL, Detect, DetectionModel):
        cls.__qualname__ = cls.__name__
        setattr(mods[cls.__module__], cls.__name__, cls)
    for n, m in mods.items():
        sys.modules[n] = m
    return conv_m, block_m, head_m, tasks_m


def uninstall():
    for name in _NAMES:
        sys.modules.pop(name, None)


def build_model(yaml, seed=0, gain=1.6, res_gain=0.5, legacy=False, cls_bias=-4.0):
    """
    A DetectionModel with random conv weights AND non-trivial BatchNorm statistics, in eval mode, fp16-representable
    (the checkpoint stores fp16).  Zero-mean kernels, gain 1.6 per Conv, 0.5 on the convs that end a residual branch,
    1.0 on the convs without activation: activations stay O(1) through the 23 layers.
    """
    conv_m, block_m, head_m, tasks_m = _install()
    torch.manual_seed(seed)
    model = tasks_m.DetectionModel(yaml, legacy=legacy)
    g = torch.Generator().manual_seed(seed + 1)
    residual_end = set()
    for m in model.modules():
        if isinstance(m, block_m.Bottleneck) and m.add:
            residual_end.add(id(m.cv2))
        if isinstance(m, block_m.PSABlock):
            residual_end.add(id(m.attn.proj))
            residual_end.add(id(m.ffn[1]))
    for m in model.modules():
        if isinstance(m, conv_m.Conv):
            w = torch.randn(m.conv.weight.shape, generator=g)
            if w.shape[1] > 1:
                w -= w.mean(dim=(1, 2, 3), keepdim=True)
            fan = w.shape[1] * w.shape[2] * w.shape[3]
            gc = res_gain if id(m) in residual_end else (gain if isinstance(m.act, nn.SiLU) else 1.0)
            nf = m.bn.num_features
            m.bn.weight.data = 0.8 + 0.4 * torch.rand(nf, generator=g)
            m.bn.bias.data = 0.1 * torch.randn(nf, generator=g)
            m.bn.running_mean.data = 0.1 * torch.randn(nf, generator=g)
            m.bn.running_var.data = 0.7 + 0.6 * torch.rand(nf, generator=g)
            m.conv.weight.data = w * (gc / fan ** 0.5)
        elif isinstance(m, head_m.Detect):
            for seq in m.cv2:
                seq[2].weight.data = torch.randn(seq[2].weight.shape, generator=g) * (0.5 / seq[2].weight.shape[1] ** 0.5)
                seq[2].bias.data = 0.5 * torch.randn(seq[2].bias.shape, generator=g)
            for seq in m.cv3:
                seq[2].weight.data = torch.randn(seq[2].weight.shape, generator=g) * (1.5 / seq[2].weight.shape[1] ** 0.5)
                seq[2].bias.data = cls_bias + 0.5 * torch.randn(seq[2].bias.shape, generator=g)
    model = model.half().float()                   # what the checkpoint holds
    return model.eval()


def save_checkpoint(model, path, image_size=640):
    """the ultralytics container ({'model': fp16 module, ...}) plus <root>/megadetector_info.json"""
    import copy
    import os
    ck = {'epoch': -1, 'best_fitness': None, 'model': copy.deepcopy(model).half(), 'ema': None, 'updates': None,
          'optimizer': None, 'train_args': {}, 'date': '2025-01-01T00:00:00', 'version': '8.3.0'}
    for p in ck['model'].parameters():
        p.requires_grad = False
    torch.save(ck, path)
    with zipfile.ZipFile(path, 'r') as z:
        root = z.namelist()[0].split('/')[0]
    with zipfile.ZipFile(path, 'a') as z:
        z.writestr(root + '/megadetector_info.json', json.dumps({'image_size': int(image_size),
                                                                 'model_name': os.path.basename(path)}))


def sparsify_classes(model, xs, conf_thr=0.005, per_row=(1, 4), logit_std=2.0):
    """
    Turns the dense, nearly input-independent class scores of a random-weight model into a sparse set on the inputs xs
    (a list of NCHW batches, e.g. one letterboxed image each), as tests/fake_yolov5.py:sparsify_objectness does for
    YOLOv5.  Per (level, class) row of the final class conv: the row is made orthogonal to the mean feature vector (its
    constant part moves into the bias) and scaled to a logit standard deviation of `logit_std` over all positions of
    all inputs; then the bias is set so that only the k most confident positions (per_row[0] <= k <= per_row[1]) score
    above conf_thr, k chosen so that the threshold falls into the WIDEST gap between consecutive logits -- no anchor
    sits on the output threshold, where a rounding difference would create or remove a detection.
    """
    conv_m, block_m, head_m, tasks_m = _install()
    det = [m for m in model.modules() if isinstance(m, head_m.Detect)][0]
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
            f = torch.cat([t.permute(1, 0, 2, 3).reshape(t.shape[1], -1) for t in feats[i]], 1)     # (C, positions)
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
