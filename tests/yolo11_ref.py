"""
CPU restatement of the YOLO11 (anchor-free) detector path: forward, DFL decode, NMS and box rescale of the ultralytics
package (8.3.x) as the reference runs them for MDv1000-larch / -sorrel (pytorch_detector.py:371-458, :957, :1327-1344).
None of it is in the reference tree; every statement is restated from the published architecture [3P] and must be
re-checked against the package once it is importable (tools/parity_real.py).

Test infrastructure only (the product path is libmdhip.so).  Letterbox, greedy suppression and formatting helpers come
from oracle.pre_post, unchanged.
"""

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pre_post as O
from megadetector_amd.yolo_model import (MDHIP_CONV, MDHIP_C3K2, MDHIP_C2PSA, MDHIP_SPPF, MDHIP_UPSAMPLE,
                                         MDHIP_CONCAT, MDHIP_DETECT_DFL)

_F = np.float32


def _rounder(mode):
    if mode in (None, False):
        return None
    if mode == 'fp16':
        return lambda x: x.to(torch.float16).to(torch.float32)
    return lambda x: x.to(torch.bfloat16).to(torch.float32)


# --------------------------------------------------------------------------------------
# DFL decode [3P] (ultralytics Detect._inference / DFL / dist2bbox), in the operation order of the HIP kernel:
# exp evaluated in double and rounded once to fp32, sums in bin order -- bit for bit what dfl_decode_kernel computes
# --------------------------------------------------------------------------------------

def _exp_r(x):
    return np.exp(np.asarray(x, dtype=np.float32).astype(np.float64)).astype(np.float32)


def dfl_decode(box, cls, stride):
    """box: (B, ny, nx, 64) fp32 logits (4 sides x 16 bins), cls: (B, ny, nx, nc) fp32 logits -> (B, ny*nx, 4 + nc)"""
    box = np.asarray(box, dtype=_F)
    cls = np.asarray(cls, dtype=_F)
    B, ny, nx, _ = box.shape
    d = []
    for side in range(4):
        v = box[..., side * 16:(side + 1) * 16]
        mx = v[..., 0]
        for i in range(1, 16):
            mx = np.maximum(mx, v[..., i])
        e = [_exp_r(v[..., i] - mx) for i in range(16)]
        s = np.zeros_like(mx)
        for i in range(16):
            s = (s + e[i]).astype(_F)
        acc = np.zeros_like(mx)
        for i in range(16):
            acc = (acc + (e[i] / s).astype(_F) * _F(i)).astype(_F)
        d.append(acc)
    ys, xs = np.meshgrid(np.arange(ny, dtype=_F), np.arange(nx, dtype=_F), indexing='ij')
    px, py = (xs + _F(0.5))[None], (ys + _F(0.5))[None]
    x1, y1, x2, y2 = px - d[0], py - d[1], px + d[2], py + d[3]
    st = _F(stride)
    out = np.empty((B, ny, nx, 4 + cls.shape[-1]), dtype=_F)
    out[..., 0] = ((x1 + x2) / _F(2)) * st
    out[..., 1] = ((y1 + y2) / _F(2)) * st
    out[..., 2] = (x2 - x1) * st
    out[..., 3] = (y2 - y1) * st
    out[..., 4:] = _F(1) / (_F(1) + _exp_r(-cls))
    return out.reshape(B, ny * nx, -1)


# --------------------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------------------

class Forward:
    """
    Functional YOLO11 forward on CPU from BN-folded weights (megadetector_amd.yolo_model.YoloWeights).

    emulate=None  : the fp32 computation the reference performs (model.float().fuse(), pytorch_detector.py:957).
    emulate='bf16' / 'fp16': the storage rounding of the HIP path -- weights and every tensor the GPU stores rounded to
                    16 bits, fp32 accumulation, activation and residual add in fp32 before the one rounding, Detect
                    logits kept fp32; the attention output is rounded once (its kernel keeps P in 16 bits: not emulated,
                    covered by the tolerances).
    keep: optional dict, layer index -> output (NCHW fp32).
    """

    def __init__(self, weights, emulate=None, keep=None):
        self.W = weights
        self.round = _rounder(emulate)
        self.w = {}
        for k, v in weights.weights.items():
            t = torch.from_numpy(np.array(v, dtype=np.float32))
            if self.round is not None and k.endswith('.weight'):
                t = self.round(t)
            self.w[k] = t
        self.keep = keep

    def _r(self, y):
        return self.round(y) if self.round is not None else y

    def conv(self, x, name, k, s=1, act=True, residual=None, groups=1, rnd=True):
        y = F.conv2d(x, self.w[name + '.weight'], self.w[name + '.bias'], stride=s, padding=k // 2, groups=groups)
        if act:
            y = F.silu(y)
        if residual is not None:
            y = residual + y
        return self._r(y) if rnd else y

    def c3k2(self, x, L):
        pre = 'model.{}'.format(L.index)
        y = self.conv(x, pre + '.cv1.conv', 1)
        c = L.hidden
        ys = [y[:, :c], y[:, c:]]
        for j in range(L.n):
            b = '{}.m.{}'.format(pre, j)
            src = ys[-1]
            if L.k:
                y1 = self.conv(src, b + '.cv1.conv', 1)
                y2 = self.conv(src, b + '.cv2.conv', 1)
                for q in range(2):
                    t = self.conv(y1, '{}.m.{}.cv1.conv'.format(b, q), 3)
                    y1 = self.conv(t, '{}.m.{}.cv2.conv'.format(b, q), 3, residual=y1)
                ys.append(self.conv(torch.cat((y1, y2), 1), b + '.cv3.conv', 1))
            else:
                t = self.conv(src, b + '.cv1.conv', 3)
                ys.append(self.conv(t, b + '.cv2.conv', 3, residual=src))
        return self.conv(torch.cat(ys, 1), pre + '.cv2.conv', 1)

    def attention_core(self, qkv, heads):
        """(B, heads*128, H, W) -> softmax(q^T k * 32^-0.5) applied to v: (B, heads*64, H, W), fp32"""
        B, _, H, W = qkv.shape
        N = H * W
        q, k, v = qkv.reshape(B, heads, 128, N).split([32, 32, 64], dim=2)
        attn = (q.transpose(-2, -1) @ k) * (32 ** -0.5)
        attn = attn.softmax(dim=-1)
        return (v @ attn.transpose(-2, -1)).reshape(B, heads * 64, H, W), v.reshape(B, heads * 64, H, W)

    def c2psa(self, x, L):
        pre = 'model.{}'.format(L.index)
        c = L.hidden
        heads = c // 64
        y = self.conv(x, pre + '.cv1.conv', 1)
        a, b = y[:, :c], y[:, c:]
        for j in range(L.n):
            m = '{}.m.{}'.format(pre, j)
            qkv = self.conv(b, m + '.attn.qkv.conv', 1, act=False)
            o, v = self.attention_core(qkv, heads)
            o = self._r(o)
            o = self.conv(v, m + '.attn.pe.conv', 3, act=False, residual=o, groups=c)
            b = self.conv(o, m + '.attn.proj.conv', 1, act=False, residual=b)
            f = self.conv(b, m + '.ffn.0.conv', 1)
            b = self.conv(f, m + '.ffn.1.conv', 1, act=False, residual=b)
        return self.conv(torch.cat((a, b), 1), pre + '.cv2.conv', 1)

    def sppf(self, x, L):
        pre = 'model.{}'.format(L.index)
        y = [self.conv(x, pre + '.cv1.conv', 1)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], L.k, 1, L.k // 2))
        return self.conv(torch.cat(y, 1), pre + '.cv2.conv', 1)

    def detect_logits(self, xs, L):
        """per level (box logits (B, ny, nx, 64), class logits (B, ny, nx, nc)), fp32 (not rounded)"""
        pre = 'model.{}'.format(L.index)
        out = []
        for l, x in enumerate(xs):
            cx = x.shape[1]
            bx = self.conv(x, '{}.cv2.{}.0.conv'.format(pre, l), 3)
            bx = self.conv(bx, '{}.cv2.{}.1.conv'.format(pre, l), 3)
            bx = self.conv(bx, '{}.cv2.{}.2'.format(pre, l), 1, act=False, rnd=False)
            c = self.conv(x, '{}.cv3.{}.0.0.conv'.format(pre, l), 3, groups=cx)
            c = self.conv(c, '{}.cv3.{}.0.1.conv'.format(pre, l), 1)
            c = self.conv(c, '{}.cv3.{}.1.0.conv'.format(pre, l), 3, groups=c.shape[1])
            c = self.conv(c, '{}.cv3.{}.1.1.conv'.format(pre, l), 1)
            c = self.conv(c, '{}.cv3.{}.2'.format(pre, l), 1, act=False, rnd=False)
            out.append((bx.permute(0, 2, 3, 1).contiguous().numpy(), c.permute(0, 2, 3, 1).contiguous().numpy()))
        return out

    def __call__(self, x):
        """x: (B, 3, H, W) fp32 in [0, 1] -> predictions (B, anchors, 4 + nc) fp32 numpy"""
        with torch.no_grad():
            x = self._r(x)
            ys = []
            for L in self.W.specs:
                inp = x if L.frm[0] < 0 else ys[L.frm[0]]
                if L.type == MDHIP_CONV:
                    y = self.conv(inp, 'model.{}.conv'.format(L.index), L.k, L.s)
                elif L.type == MDHIP_C3K2:
                    y = self.c3k2(inp, L)
                elif L.type == MDHIP_C2PSA:
                    y = self.c2psa(inp, L)
                elif L.type == MDHIP_SPPF:
                    y = self.sppf(inp, L)
                elif L.type == MDHIP_UPSAMPLE:
                    y = F.interpolate(inp, scale_factor=2, mode='nearest')
                elif L.type == MDHIP_CONCAT:
                    y = torch.cat([ys[f] for f in L.frm], 1)
                elif L.type == MDHIP_DETECT_DFL:
                    self.logits = self.detect_logits([ys[f] for f in L.frm], L)
                    preds = [dfl_decode(b, c, s) for (b, c), s in zip(self.logits, self.W.strides)]
                    return np.concatenate(preds, axis=1)
                else:
                    raise ValueError(L.type)
                if self.keep is not None:
                    self.keep[L.index] = y
                ys.append(y)
        raise ValueError('model without Detect head')


# --------------------------------------------------------------------------------------
# NMS [3P]: ultralytics non_max_suppression (agnostic=False, multi_label=False, max_det=300, max_nms=30000, max_wh=7680)
# --------------------------------------------------------------------------------------

MAX_NMS = 30000
MAX_WH = 7680.0


def nms(prediction, conf_thres, iou_thres, max_det=300, max_nms=MAX_NMS):
    """
    prediction: (B, anchors, 4 + nc) fp32 ([cx, cy, w, h, cls...]).  Per image: conf, j = max over the classes (first
    maximum), keep conf > conf_thres (strict, no objectness), xyxy = xywh2xyxy, the max_nms most confident candidates
    (ties: increasing anchor index -- the package leaves them unspecified), ONE greedy NMS over boxes + j * 7680 (the
    IoU sees the shifted fp32 coordinates), the first max_det survivors.  Returns a list of (n, 6) fp32 arrays.
    """
    prediction = np.asarray(prediction, dtype=_F)
    out = []
    for x in prediction:
        cls = x[:, 4:]
        j = np.argmax(cls, axis=1)
        conf = cls[np.arange(cls.shape[0]), j]
        idx = np.nonzero(conf > _F(conf_thres))[0]
        if idx.size == 0:
            out.append(np.zeros((0, 6), dtype=_F))
            continue
        order = idx[np.argsort(-conf[idx], kind='stable')][:max_nms]
        c, jj = conf[order], j[order].astype(_F)
        b = x[order, :4]
        box = np.stack([b[:, 0] - b[:, 2] / _F(2), b[:, 1] - b[:, 3] / _F(2),
                        b[:, 0] + b[:, 2] / _F(2), b[:, 1] + b[:, 3] / _F(2)], 1).astype(_F)
        shifted = (box + (jj * _F(MAX_WH))[:, None]).astype(_F)
        keep = O._greedy_nms(torch.from_numpy(shifted), torch.from_numpy(c.copy()), iou_thres).numpy()[:max_det]
        out.append(np.concatenate([box[keep], c[keep, None], jj[keep, None]], 1).astype(_F))
    return out


# --------------------------------------------------------------------------------------
# box rescale [3P]: ultralytics scale_boxes (classic mode: ratio_pad None) rounds the padding
# --------------------------------------------------------------------------------------

def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None):
    boxes = boxes.clone()
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
               round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    boxes[:, [0, 2]] -= pad[0]
    boxes[:, [1, 3]] -= pad[1]
    boxes[:, :4] /= gain
    boxes[:, 0].clamp_(0, img0_shape[1])
    boxes[:, 1].clamp_(0, img0_shape[0])
    boxes[:, 2].clamp_(0, img0_shape[1])
    boxes[:, 3].clamp_(0, img0_shape[0])
    return boxes


def format_detections(det, batch_hw, img_original_shape, scaling_shape, detection_threshold):
    """reference pytorch_detector.py:1352-1422, classic mode, with the ultralytics scale_boxes"""
    detections, max_conf = [], 0.0
    det = torch.from_numpy(np.asarray(det, dtype=_F)).clone()
    if len(det) > 0:
        gn = torch.tensor(scaling_shape)[[1, 0, 1, 0]]
        det[:, :4] = scale_boxes(batch_hw, det[:, :4], img_original_shape).round()
        for *xyxy, conf, cls in reversed(det):
            if conf < detection_threshold:
                continue
            xywh = (O.xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()
            api_box = O.truncate_float_array(O.convert_yolo_to_xywh(xywh), precision=O.COORD_DIGITS)
            conf = O.truncate_float(conf.tolist(), precision=O.CONF_DIGITS)
            detections.append({'category': str(int(cls.tolist()) + 1), 'conf': conf, 'bbox': api_box})
            max_conf = max(max_conf, conf)
    return detections, max_conf


def detections(pred, infos, batch_hw, threshold, iou=0.45):
    """the restatement pipeline behind the forward: NMS + classic formatting, per image"""
    out = []
    for d, info in zip(nms(pred, threshold, iou), infos):
        lst, mx = format_detections(d, batch_hw, info['img_original'].shape, info['scaling_shape'], threshold)
        out.append({'detections': lst, 'max_detection_conf': mx})
    return out


# --------------------------------------------------------------------------------------
# work and parameters, counted from the graph
# --------------------------------------------------------------------------------------

def count_work(weights_or_yaml, h, w):
    """(GFLOPs at h x w as 2 x MACs of every conv, attention products included; parameters of the fused model)"""
    from megadetector_amd import weights_io
    from megadetector_amd.yolo_model import resolve_yaml, model_strides
    yaml = weights_or_yaml if isinstance(weights_or_yaml, dict) else weights_or_yaml.yaml
    specs = resolve_yaml(yaml)
    div = []
    for s in specs:
        d = 1 if s.frm[0] < 0 else div[s.frm[0]]
        if s.type == MDHIP_CONV:
            d *= s.s
        elif s.type == MDHIP_UPSAMPLE:
            d //= 2
        div.append(d)
    macs, params = 0.0, 0
    for s in specs:
        for name, (c2, c1, k) in weights_io.yolo11_conv_shapes(s, specs):
            if s.type == MDHIP_DETECT_DFL:
                lvl = int(name.split('.')[3])
                d = div[s.frm[lvl]]
            else:
                d = div[s.index] if s.type != MDHIP_CONV else div[s.index]
            px = (h // d) * (w // d)
            macs += px * c2 * c1 * k * k
            params += c2 * c1 * k * k + c2
        if s.type == MDHIP_C2PSA:
            n_tok = (h // div[s.index]) * (w // div[s.index])
            heads = s.hidden // 64
            macs += s.n * heads * n_tok * n_tok * (32 + 64)
    params += 16                                              # the DFL conv
    return 2 * macs / 1e9, params
