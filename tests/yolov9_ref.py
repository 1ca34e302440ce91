"""
CPU restatement of the YOLOv9-C (MDv1000-cedar) detector path: forward, the ADown / CBFuse pools in the operation order of
the HIP kernels, the yolov9 package's NMS and its box rescale, as the reference runs them through yolov9pip
(pytorch_detector.py:348-368, :957, :1327-1344).  None of it is in the reference tree; every statement is restated from
the published YOLOv9 architecture (WongKinYiu) [3P] and must be re-checked against the package once it is importable
(tools/parity_real.py).

Test infrastructure only (the product path is libmdhip.so).  The DFL decode and the greedy suppression are the YOLO11
ones (tests/yolo11_ref.py, oracle.pre_post), unchanged.
"""

import numpy as np
import torch
import torch.nn.functional as F

import yolo11_ref as R11
from oracle import pre_post as O
from megadetector_amd.yolo_model import (MDHIP_CONV, MDHIP_SPPF, MDHIP_UPSAMPLE, MDHIP_CONCAT, MDHIP_ELAN4, MDHIP_ADOWN,
                                         MDHIP_CBLINEAR, MDHIP_CBFUSE, MDHIP_DETECT_DDFL, MDHIP_SILENCE, layer_divisors)

_F = np.float32
dfl_decode = R11.dfl_decode


def _st(x, dtype):
    """fp32 numpy -> the storage type and back"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=_F))
    return t.to(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


# --------------------------------------------------------------------------------------
# the two memory-bound kernels, bit for bit (NHWC numpy, values representable in the storage type)
# --------------------------------------------------------------------------------------

def avgpool2x2(x, dtype):
    """[n][H][W][c] -> [n][H-1][W-1][c]: ((a + b) + c) + d in fp32 over the window in row order, / 4, rounded once"""
    x = np.asarray(x, dtype=_F)
    s = ((x[:, :-1, :-1] + x[:, :-1, 1:]).astype(_F) + x[:, 1:, :-1]).astype(_F) + x[:, 1:, 1:]
    return _st(s.astype(_F) * _F(0.25), dtype)


def adown_pool(x, dtype):
    """ADown's pools of [n][H][W][c]: (A [n][H][W][c/2] with a zero last row / column, B [n][H/2][W/2][c/2])"""
    n, H, W, c = x.shape
    a = avgpool2x2(x, dtype)
    A = np.zeros((n, H, W, c // 2), dtype=_F)
    A[:, :H - 1, :W - 1] = a[..., :c // 2]
    t = torch.from_numpy(np.ascontiguousarray(a[..., c // 2:])).permute(0, 3, 1, 2)
    B = F.max_pool2d(t, 3, 2, 1).permute(0, 2, 3, 1).numpy()
    return A, np.ascontiguousarray(B)


def cbfuse(srcs, factors, last, dtype):
    """((up(s0) + up(s1)) + up(s2)) + last in fp32, rounded once; up = nearest resize by the integer factor"""
    acc = None
    for s, f in zip(srcs, factors):
        u = np.repeat(np.repeat(np.asarray(s, dtype=_F), f, axis=1), f, axis=2)
        acc = u if acc is None else (acc + u).astype(_F)
    return _st((acc + np.asarray(last, dtype=_F)).astype(_F), dtype)


# --------------------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------------------

class Forward(R11.Forward):
    """
    Functional YOLOv9-C forward on CPU from folded weights (megadetector_amd.yolo_model.YoloWeights), as
    model.float().fuse() computes it (pytorch_detector.py:957).  emulate=None: fp32; 'bf16' / 'fp16': the storage rounding
    of the HIP path (weights and every stored tensor rounded, fp32 accumulation, the ADown average and the CBFuse sum
    rounded once).  Returns the predictions of the head the yolov9 NMS reads: DualDDetect returns [y_first, y_second]
    and non_max_suppression keeps prediction[0], the head over the first nl inputs [3P].  `self.heads` holds both.
    """

    def repncsp(self, x, b, n):
        y1 = self.conv(x, b + '.cv1.conv', 1)
        y2 = self.conv(x, b + '.cv2.conv', 1)
        for j in range(n):
            t = self.conv(y1, '{}.m.{}.cv1.conv'.format(b, j), 3)
            y1 = self.conv(t, '{}.m.{}.cv2.conv'.format(b, j), 3, residual=y1)
        return self.conv(torch.cat((y1, y2), 1), b + '.cv3.conv', 1)

    def elan4(self, x, L):
        pre = 'model.{}'.format(L.index)
        y = self.conv(x, pre + '.cv1.conv', 1)
        c3 = y.shape[1]
        ys = [y[:, :c3 // 2], y[:, c3 // 2:]]
        a = self.conv(self.repncsp(ys[-1], pre + '.cv2.0', L.n), pre + '.cv2.1.conv', 3)
        b = self.conv(self.repncsp(a, pre + '.cv3.0', L.n), pre + '.cv3.1.conv', 3)
        return self.conv(torch.cat(ys + [a, b], 1), pre + '.cv4.conv', 1)

    def adown(self, x, L):
        pre = 'model.{}'.format(L.index)
        x = self._r(F.avg_pool2d(x, 2, 1, 0, False, True))
        x1, x2 = x.chunk(2, 1)
        x1 = self.conv(x1, pre + '.cv1.conv', 3, 2)
        x2 = self.conv(F.max_pool2d(x2, 3, 2, 1), pre + '.cv2.conv', 1)
        return torch.cat((x1, x2), 1)

    def sppelan(self, x, L):
        pre = 'model.{}'.format(L.index)
        y = [self.conv(x, pre + '.cv1.conv', 1)]
        for _ in range(3):
            y.append(F.max_pool2d(y[-1], 5, 1, 2))
        return self.conv(torch.cat(y, 1), pre + '.cv5.conv', 1)

    def cbfuse(self, xs, L):
        tgt = xs[-1]
        acc = None
        for x, off in zip(xs[:-1], L.hidden):
            u = F.interpolate(x[:, off:off + tgt.shape[1]], size=tgt.shape[2:], mode='nearest')
            acc = u if acc is None else acc + u
        return self._r(acc + tgt)

    def ddetect(self, xs, L, head):
        pre = 'model.{}'.format(L.index)
        a, b = ('cv2', 'cv3') if head == 0 else ('cv4', 'cv5')
        out = []
        for l, x in enumerate(xs):
            bx = self.conv(x, '{}.{}.{}.0.conv'.format(pre, a, l), 3)
            bx = self.conv(bx, '{}.{}.{}.1.conv'.format(pre, a, l), 3, groups=4)
            bx = self.conv(bx, '{}.{}.{}.2'.format(pre, a, l), 1, act=False, rnd=False)
            c = self.conv(x, '{}.{}.{}.0.conv'.format(pre, b, l), 3)
            c = self.conv(c, '{}.{}.{}.1.conv'.format(pre, b, l), 3)
            c = self.conv(c, '{}.{}.{}.2'.format(pre, b, l), 1, act=False, rnd=False)
            out.append((bx.permute(0, 2, 3, 1).contiguous().numpy(), c.permute(0, 2, 3, 1).contiguous().numpy()))
        return out

    def __call__(self, x):
        """x: (B, 3, H, W) fp32 in [0, 1] -> predictions (B, anchors, 4 + nc) of the head yolov9's NMS reads"""
        with torch.no_grad():
            x = self._r(x)
            ys = []
            for L in self.W.specs:
                inp = x if L.frm[0] < 0 else ys[L.frm[0]]
                if L.type == MDHIP_SILENCE:
                    y = inp
                elif L.type == MDHIP_CONV:
                    y = self.conv(inp, 'model.{}.conv'.format(L.index), L.k, L.s)
                elif L.type == MDHIP_ELAN4:
                    y = self.elan4(inp, L)
                elif L.type == MDHIP_ADOWN:
                    y = self.adown(inp, L)
                elif L.type == MDHIP_SPPF:
                    y = self.sppelan(inp, L)
                elif L.type == MDHIP_UPSAMPLE:
                    y = F.interpolate(inp, scale_factor=2, mode='nearest')
                elif L.type == MDHIP_CONCAT:
                    y = torch.cat([ys[f] for f in L.frm], 1)
                elif L.type == MDHIP_CBLINEAR:
                    y = self.conv(inp, 'model.{}.conv'.format(L.index), 1, act=False)
                elif L.type == MDHIP_CBFUSE:
                    y = self.cbfuse([ys[f] for f in L.frm], L)
                elif L.type == MDHIP_DETECT_DDFL:
                    nl = len(L.frm) // L.n
                    self.heads = []
                    for h in range(L.n):
                        logits = self.ddetect([ys[f] for f in L.frm[h * nl:(h + 1) * nl]], L, h)
                        self.heads.append(np.concatenate([dfl_decode(b, c, s) for (b, c), s in zip(logits, self.W.strides)], 1))
                    return self.heads[0]
                else:
                    raise ValueError(L.type)
                if self.keep is not None and L.type != MDHIP_SILENCE:
                    self.keep[L.index] = y
                ys.append(y)
        raise ValueError('model without Detect head')


# --------------------------------------------------------------------------------------
# NMS [3P]: yolov9 utils.general.non_max_suppression (agnostic=False, multi_label=False, max_det=300, max_nms=30000,
# max_wh=7680).  A list / tuple input is unwrapped to its first element; candidates are sorted by confidence EVERY time
# (ultralytics sorts only above the cut) -- with ties in increasing anchor index that is the order the YOLO11 restatement
# and the HIP kernel already use.
# --------------------------------------------------------------------------------------

MAX_NMS = R11.MAX_NMS


def nms(prediction, conf_thres, iou_thres, max_det=300, max_nms=MAX_NMS):
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
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
        b = x[idx, :4]
        box = np.stack([b[:, 0] - b[:, 2] / _F(2), b[:, 1] - b[:, 3] / _F(2),
                        b[:, 0] + b[:, 2] / _F(2), b[:, 1] + b[:, 3] / _F(2)], 1).astype(_F)
        det = np.concatenate([box, conf[idx, None], j[idx, None].astype(_F)], 1)
        det = det[np.argsort(-det[:, 4], kind='stable')[:max_nms]]         # sort by confidence, remove the excess
        shifted = (det[:, :4] + (det[:, 5:6] * _F(R11.MAX_WH))).astype(_F)
        keep = O._greedy_nms(torch.from_numpy(shifted), torch.from_numpy(det[:, 4].copy()), iou_thres).numpy()[:max_det]
        out.append(det[keep].astype(_F))
    return out


# --------------------------------------------------------------------------------------
# box rescale [3P]: yolov9 scale_boxes == yolov5 scale_coords (the padding is NOT rounded)
# --------------------------------------------------------------------------------------

def scale_boxes(img1_shape, boxes, img0_shape):
    boxes = boxes.clone()
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    boxes[:, [0, 2]] -= pad[0]
    boxes[:, [1, 3]] -= pad[1]
    boxes[:, :4] /= gain
    boxes[:, 0].clamp_(0, img0_shape[1])
    boxes[:, 1].clamp_(0, img0_shape[0])
    boxes[:, 2].clamp_(0, img0_shape[1])
    boxes[:, 3].clamp_(0, img0_shape[0])
    return boxes


def format_detections(det, batch_hw, img_original_shape, scaling_shape, detection_threshold):
    """reference pytorch_detector.py:1352-1422, classic mode, with the yolov9 scale_boxes"""
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

def count_work(weights_or_yaml, h, w, heads=None):
    """(GFLOPs at h x w as 2 x MACs of every conv -- the grouped box conv at its real cost; parameters of the fused
    model, DFL conv included).  heads: which Detect heads to count (default: all of them)."""
    from megadetector_amd import weights_io
    from megadetector_amd.yolo_model import resolve_yaml
    yaml = weights_or_yaml if isinstance(weights_or_yaml, dict) else weights_or_yaml.yaml
    specs = resolve_yaml(yaml)
    div = layer_divisors(specs)
    macs, params = 0.0, 0
    for s in specs:
        for name, (c2, c1, k) in weights_io.yolov9_conv_shapes(s, specs):
            if s.type == MDHIP_DETECT_DDFL:
                part, lvl = name.split('.')[2], int(name.split('.')[3])
                h_idx = 0 if part in ('cv2', 'cv3') else 1
                if heads is not None and h_idx not in heads:
                    continue
                d = div[s.frm[h_idx * (len(s.frm) // s.n) + lvl]]
            else:
                d = div[s.index]
            macs += (h // d) * (w // d) * c2 * c1 * k * k
            params += c2 * c1 * k * k + c2
    det = specs[-1]
    params += 16 * (det.n if heads is None else len(heads))
    return 2 * macs / 1e9, params
