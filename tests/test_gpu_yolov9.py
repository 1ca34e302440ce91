"""
YOLOv9-C (MDv1000-cedar) on the HIP path, through the C ABI, against the CPU restatement tests/yolov9_ref.py: the two
new kernels bit for bit, every layer of three networks (both head forms), the anchor-free NMS against the yolov9 rule,
and the detector end to end on a fake yolov9 checkpoint.
"""

import glob
import json
import os

import numpy as np
import pytest
import torch

import parity_util as PU
import yolov9_ref as R
from oracle import pre_post as O
from test_gpu_parity import LAYER_MAX_TOL, F16_LAYER_MAX_TOL
from test_gpu_headline import LAYER_MEAN_TOL, F16_LAYER_MEAN_TOL

from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd import _lib
from megadetector_amd.hip_backend import HipContext
from megadetector_amd.yolo_model import MDHIP_SILENCE, detect_inputs

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']
HERE = os.path.dirname(os.path.abspath(__file__))

_CTX = {}


def _ctx(dtype, yaml_name='GELAN_TEST', max_batch=2, size=640, seed=0):
    key = (dtype, yaml_name, max_batch, size, seed)
    if key not in _CTX:
        W = weights_io.synthetic_weights(getattr(yolo_yaml, yaml_name), seed=seed)
        _CTX[key] = (HipContext(W, dtype=dtype, max_batch=max_batch, max_h=size, max_w=size), W)
    return _CTX[key]


def _bits(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to(torch.float16 if dtype == 'fp16' else torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def _from_bits(u, dtype):
    t = torch.from_numpy(np.ascontiguousarray(u).view(np.int16))
    return t.view(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels in isolation: bit-exact
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,h,w,c', [(1, 8, 8, 16), (2, 20, 14, 32), (3, 10, 22, 48), (1, 40, 40, 128), (4, 6, 2, 16)])
def test_adown_pool_bit_exact(dtype, n, h, w, c):
    ctx, _ = _ctx(dtype)
    rng = np.random.default_rng(n * 1000 + h * w + c)
    x = _from_bits(_bits(rng.standard_normal((n, h, w, c)) * 3, dtype), dtype)
    a = np.empty((n, h, w, c // 2), dtype=np.uint16)
    b = np.empty((n, h // 2, w // 2, c // 2), dtype=np.uint16)
    rc = ctx.lib.mdhip_adown_pool_on(ctx.h, _lib.np_ptr(_bits(x, dtype)), _lib.np_ptr(a), _lib.np_ptr(b), n, h, w, c, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    A, B = R.adown_pool(x, dtype)
    np.testing.assert_array_equal(_from_bits(a, dtype), A)
    np.testing.assert_array_equal(_from_bits(b, dtype), B)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,h,w,c,factors', [(1, 8, 8, 16, (1, 2, 4)), (2, 20, 12, 32, (1, 2)), (3, 4, 12, 8, (4,)),
                                             (2, 14, 6, 24, (2, 1))])
def test_cbfuse_bit_exact(dtype, n, h, w, c, factors):
    ctx, _ = _ctx(dtype)
    rng = np.random.default_rng(n * 100 + h + w + c)
    srcs = [_from_bits(_bits(rng.standard_normal((n, h // f, w // f, c)), dtype), dtype) for f in factors]
    last = _from_bits(_bits(rng.standard_normal((n, h, w, c)), dtype), dtype)
    keep = [_bits(s, dtype) for s in srcs]
    ptrs = (_lib.C.c_void_p * 3)(*([k.ctypes.data for k in keep] + [None] * (3 - len(keep))))
    fac = np.array(list(factors) + [1] * (3 - len(factors)), dtype=np.int32)
    out = np.empty((n, h, w, c), dtype=np.uint16)
    rc = ctx.lib.mdhip_cbfuse_on(ctx.h, ptrs, _lib.np_ptr(fac), len(factors), _lib.np_ptr(_bits(last, dtype)),
                                 _lib.np_ptr(out), n, h, w, c, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    np.testing.assert_array_equal(_from_bits(out, dtype), R.cbfuse(srcs, factors, last, dtype))


# ---------------------------------------------------------------------------------------------------------------------
# 2. every layer against the storage-emulating restatement
# ---------------------------------------------------------------------------------------------------------------------

def _letterboxed(n, h, w, size, seed):
    imgs = PU.structured_images(n, h, w, seed=seed)
    x, infos = PU.oracle_input(imgs, size, 32)
    lb = [np.ascontiguousarray(i['img_processed']) for i in infos]
    return x, lb


def _reachable(W):
    """the layers the library lowers: those that reach the Detect head that runs"""
    specs = W.specs
    reach = {specs[-1].index} | set(detect_inputs(specs[-1]))
    for s in reversed(specs[:-1]):
        if s.index in reach:
            reach |= {f for f in s.frm if f >= 0}
    return reach


def _layers(ctx, W, x, lb, dtype, worst):
    n, _, hh, ww = x.shape
    ctx.preprocess(lb, [(im.shape[0], im.shape[1], im.shape[0], im.shape[1], 0, 0) for im in lb], hh, ww)
    ctx.forward(n, hh, ww)
    keep = {}
    pred_ref = R.Forward(W, emulate=dtype, keep=keep)(x)
    max_tol = F16_LAYER_MAX_TOL if dtype == 'fp16' else LAYER_MAX_TOL
    mean_tol = F16_LAYER_MEAN_TOL if dtype == 'fp16' else LAYER_MEAN_TOL
    reach = _reachable(W)
    checked = 0
    for i in sorted(keep):
        if i not in reach or W.specs[i].type == MDHIP_SILENCE:
            continue
        emax, emean = PU.rel_err(ctx.read_layer(i, n), keep[i].numpy())
        worst[0] = max(worst[0], emax)
        worst[1] = max(worst[1], emean)
        checked += 1
        assert emax < max_tol and emean < mean_tol, (i, emax, emean)
    pred = ctx.read_predictions(n)
    assert pred.shape == pred_ref.shape
    e_box = PU.rel_err(pred[..., :4], pred_ref[..., :4])
    e_cls = float(np.abs(pred[..., 4:] - pred_ref[..., 4:]).max())
    print('{} {}x{} b{}: {} layers, worst max {:.2e} mean {:.2e}; box {:.2e} / {:.2e}, cls abs {:.2e}'.format(
        dtype, hh, ww, n, checked, worst[0], worst[1], e_box[0], e_box[1], e_cls))
    assert e_box[0] < max_tol and e_box[1] < mean_tol and e_cls < max_tol, (e_box, e_cls)
    return checked


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['GELAN_TEST', 'YOLOV9_DUAL_TEST'])
def test_small_nets_layers(dtype, name):
    ctx, W = _ctx(dtype, name)
    worst = [0.0, 0.0]
    for (h, w), seed in (((640, 640), 3), ((480, 640), 4)):
        x, lb = _letterboxed(2, h, w, 640, seed)
        checked = _layers(ctx, W, x, lb, dtype, worst)
    # the dual form lowers the auxiliary branch only: layers 10 .. 22 feed the head that does not run
    assert checked == (22 if name == 'GELAN_TEST' else 24)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gelan_c_md_layers(dtype):
    ctx, W = _ctx(dtype, 'GELAN_C_MD', max_batch=1, size=640)
    x, lb = _letterboxed(1, 640, 640, 640, 11)
    _layers(ctx, W, x, lb, dtype, [0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# 3. NMS: the anchor-free kernel against the yolov9 rule (sort every time), bit-exact
# ---------------------------------------------------------------------------------------------------------------------

def _af_predictions(seed, batch, n, img, nc=3, conf_lo=0.0, ties=False):
    g = torch.Generator().manual_seed(seed)
    p = PU.random_predictions(seed, batch, n, img=img)[..., :4]
    cls = torch.rand(batch, n, nc, generator=g) ** 4
    if conf_lo > 0:
        cls = conf_lo + (1 - conf_lo) * cls
    if ties:
        cls = (cls * 16).round() / 16
    return torch.cat([p, cls], 2).numpy().astype(np.float32)


@pytest.mark.parametrize('thr', [1e-5, 0.2])
@pytest.mark.parametrize('ties', [False, True])
def test_nms_bit_exact_against_yolov9(thr, ties):
    ctx, _ = _ctx('fp16', max_batch=2, size=640)
    pred = _af_predictions(5, 2, 8400, 640.0, ties=ties)
    out, counts = ctx.nms_on(pred, thr, 0.45, 300)
    ref = R.nms([pred, pred[:, ::-1].copy()], thr, 0.45, 300)          # (DualDDetect's list: the first element)
    for b in range(2):
        assert counts[b] == len(ref[b])
        np.testing.assert_array_equal(out[b, :counts[b]], ref[b])


def test_nms_30000_cut_against_yolov9():
    ctx, _ = _ctx('fp16', max_batch=1, size=1280)
    n = ctx.num_anchors(1280, 1280)
    assert n == 33600
    rng = np.random.default_rng(3)
    pred = np.zeros((1, n, 7), dtype=np.float32)
    conf = ((np.linspace(0.02, 0.99, n) * 64).round() / 64).astype(np.float32)[rng.permutation(n)]    # with ties
    pred[0, np.arange(n), 4 + rng.integers(0, 3, n)] = conf
    top = np.argsort(-conf, kind='stable')[:R.MAX_NMS]
    pred[0, :, 0:2] = rng.random((n, 2)).astype(np.float32) * 1200 + 40
    pred[0, :, 2:4] = 20
    pred[0, top, 0:2] = 300 + rng.random((top.size, 2)).astype(np.float32)
    pred[0, top, 2:4] = 200 + rng.random((top.size, 2)).astype(np.float32)
    for max_det in (300, 1000):
        out, counts = ctx.nms_on(pred, 1e-5, 0.45, max_det)
        ref = R.nms(pred, 1e-5, 0.45, max_det)
        assert counts[0] == len(ref[0])
        np.testing.assert_array_equal(out[0, :counts[0]], ref[0])
        assert len(ref[0]) < len(R.nms(pred, 1e-5, 0.45, max_det, max_nms=n)[0])     # the cut decides the answer


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end: fake yolov9 checkpoint -> load_detector / run_detector_batch
# ---------------------------------------------------------------------------------------------------------------------

def _bundled():
    from PIL import Image
    files = sorted(f for f in glob.glob(os.path.join(HERE, 'golden', 'bundled_images', '*.*')))
    return [np.asarray(Image.open(f).convert('RGB')) for f in files], files


@pytest.fixture(scope='module', params=['GELAN_TEST', 'YOLOV9_DUAL_TEST'])
def fake_cedar(request, tmp_path_factory):
    import fake_yolov9 as FV
    model = FV.build_model(getattr(yolo_yaml, request.param), seed=5)
    imgs, _ = _bundled()
    FV.sparsify_classes(model, [O.to_batch_tensor([O.preprocess_image_classic(im, image_size=640, stride=32)['img_processed']])
                                for im in imgs])
    path = str(tmp_path_factory.mktemp('y9') / 'md_v1000.0.0-cedar.pt')
    FV.save_checkpoint(model, path, image_size=640)
    FV.uninstall()
    return path


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_end_to_end_fake_cedar(fake_cedar, dtype):
    from megadetector_amd.run_detector import load_detector
    from megadetector_amd import run_detector_batch as RDB
    det = load_detector(fake_cedar, detector_options={'dtype': dtype, 'batch_size': 4})
    assert det.default_image_size == 640 and det.letterbox_stride == 32 and det.yolov9
    imgs, files = _bundled()
    ids = [os.path.basename(f) for f in files]
    thr = 1e-5
    res = det.generate_detections_one_batch(imgs, ids, detection_threshold=thr)
    W = weights_io.load_checkpoint(fake_cedar)
    worst = {}
    n_det = 0
    for mode in (dtype, None):
        errs = []
        for img, r in zip(imgs, res):
            info = O.preprocess_image_classic(img, image_size=640, stride=32)
            x = O.to_batch_tensor([info['img_processed']])
            pred = R.Forward(W, emulate=mode)(x)
            ref = R.detections(pred, [info], x.shape[2:], thr)[0]
            a = [d for d in r['detections'] if d['conf'] >= 0.005]
            b = [d for d in ref['detections'] if d['conf'] >= 0.005]
            n_det += len(b)
            errs.append(O.compare_detection_lists(a, b))
            assert r.get('failure') is None
        worst[mode] = (max(e[0] for e in errs), max(e[1] for e in errs))
    print('{} end to end vs emulating restatement: conf {:.4f} coord {:.4f}; vs fp32: conf {:.4f} coord {:.4f} ({} dets)'.format(
        dtype, *worst[dtype], *worst[None], n_det))
    assert n_det > 0
    if dtype == 'fp16':
        assert worst['fp16'][0] <= 0.005 and worst['fp16'][1] <= 0.001, worst
    # the batch driver (JSON) gives what the detector gives
    out = RDB.load_and_run_detector_batch(fake_cedar, files, quiet=True, confidence_threshold=0.005,
                                          detector_options={'dtype': dtype, 'batch_size': 4})
    out = json.loads(json.dumps(sorted(out, key=lambda r: r['file'])))
    direct = {os.path.basename(f): [d for d in r['detections'] if d['conf'] >= 0.005] for f, r in zip(files, res)}
    for r in out:
        assert r['detections'] == direct[os.path.basename(r['file'])]


def test_yolov9_refuses_augment_and_fp8(fake_cedar):
    from megadetector_amd.detector import HIPDetector
    det = HIPDetector(fake_cedar, {'dtype': 'fp16', 'batch_size': 2})
    imgs, files = _bundled()
    with pytest.raises(ValueError, match='YOLOv9'):
        det.generate_detections_one_batch(imgs[:1], [os.path.basename(files[0])], augment=True)
    with pytest.raises(ValueError, match='YOLOv9'):
        HIPDetector(fake_cedar, {'dtype': 'fp8', 'fp8_scales': [1.0]})
    assert det._ctx.lib.mdhip_forward_tta(det._ctx.h, 1, 640, 640, None) == -4


# ---------------------------------------------------------------------------------------------------------------------
# 5. batch invariance and graph replay (the dual form: two stems read the network input)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_invariance_and_graph_replay(dtype):
    ctx, W = _ctx(dtype, 'YOLOV9_DUAL_TEST', max_batch=8, size=640, seed=2)
    imgs = PU.structured_images(8, 480, 640, seed=21)
    x, infos = PU.oracle_input(imgs, 640, 32)
    lb = [np.ascontiguousarray(i['img_processed']) for i in infos]
    hh, ww = x.shape[2:]
    geoms = [(im.shape[0], im.shape[1], im.shape[0], im.shape[1], 0, 0) for im in lb]
    ctx.set_graph('off')
    ctx.preprocess(lb[3:4], geoms[3:4], hh, ww)
    ctx.forward(1, hh, ww)
    p1 = ctx.read_predictions(1).copy()
    d1, c1 = ctx.nms(1, 1e-5, 0.45, 300)
    d1 = d1[0, :c1[0]].copy()
    ctx.preprocess(lb, geoms, hh, ww)
    ctx.forward(8, hh, ww)
    p8 = ctx.read_predictions(8).copy()
    d8, c8 = ctx.nms(8, 1e-5, 0.45, 300)
    np.testing.assert_array_equal(p8[3], p1[0])
    np.testing.assert_array_equal(d8[3, :c8[3]], d1)
    ctx.set_graph('on')
    try:
        for _ in range(3):
            ctx.forward(8, hh, ww)
            np.testing.assert_array_equal(ctx.read_predictions(8), p8)
    finally:
        ctx.set_graph('off')
