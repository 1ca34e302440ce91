"""
YOLO11 (MDv1000-larch / -sorrel) on the HIP path, through the C ABI, against the CPU restatement tests/yolo11_ref.py:
the three new kernels in isolation, every layer of three YOLO11 networks, the anchor-free NMS, and the detector end to
end on a fake ultralytics checkpoint.
"""

import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_util as PU
import yolo11_ref as R
from oracle import pre_post as O
from test_gpu_parity import LAYER_MAX_TOL, F16_LAYER_MAX_TOL
from test_gpu_headline import LAYER_MEAN_TOL, F16_LAYER_MEAN_TOL

from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd import _lib
from megadetector_amd.hip_backend import HipContext

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']
HERE = os.path.dirname(os.path.abspath(__file__))

_CTX = {}


def _ctx(dtype, yaml_name='YOLO11N_TEST', max_batch=2, size=640, seed=0):
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


def _unit_tol(dtype):
    return 4e-3 if dtype == 'fp16' else 2e-2


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels in isolation
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', [(15, 20), (20, 20), (30, 30), (40, 40), (7, 9)])
def test_dwconv3x3_kernel(dtype, hw):
    ctx, _ = _ctx(dtype)
    h, w = hw
    n, c = 2, 64
    rng = np.random.default_rng(h * 100 + w)
    # plain depthwise conv with SiLU; then the pe form: v slices of a qkv tensor, added to a residual
    x = _from_bits(_bits(rng.standard_normal((n, h, w, c)), dtype), dtype)
    wt = rng.standard_normal((c, 1, 3, 3)).astype(np.float32) / 3
    b = rng.standard_normal(c).astype(np.float32) * 0.1
    out = np.empty((n, h, w, c), dtype=np.uint16)
    rc = ctx.lib.mdhip_dwconv3x3_on(ctx.h, _lib.np_ptr(_bits(x, dtype)), c, _lib.np_ptr(wt), _lib.np_ptr(b), None,
                                    _lib.np_ptr(out), n, h, w, c, c, c, 0, 1, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    wr = _from_bits(_bits(wt, dtype), dtype)
    ref = F.silu(F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wr), torch.from_numpy(b), padding=1,
                          groups=c)).permute(0, 2, 3, 1).numpy()
    emax, _ = PU.rel_err(_from_bits(out, dtype), ref)
    assert emax < _unit_tol(dtype), emax

    heads = 2
    qkv = _from_bits(_bits(rng.standard_normal((n, h, w, heads * 128)), dtype), dtype)
    res = _from_bits(_bits(rng.standard_normal((n, h, w, heads * 64)), dtype), dtype)
    c2 = heads * 64
    wt2 = rng.standard_normal((c2, 1, 3, 3)).astype(np.float32) / 3
    b2 = rng.standard_normal(c2).astype(np.float32) * 0.1
    out2 = np.empty((n, h, w, c2), dtype=np.uint16)
    rc = ctx.lib.mdhip_dwconv3x3_on(ctx.h, _lib.np_ptr(_bits(qkv, dtype)), heads * 128, _lib.np_ptr(wt2), _lib.np_ptr(b2),
                                    _lib.np_ptr(_bits(res, dtype)), _lib.np_ptr(out2), n, h, w, c2, 64, 128, 64, 0, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    v = qkv.reshape(n, h, w, heads, 128)[..., 64:].reshape(n, h, w, c2)
    ref2 = res + F.conv2d(torch.from_numpy(v).permute(0, 3, 1, 2), torch.from_numpy(_from_bits(_bits(wt2, dtype), dtype)),
                          torch.from_numpy(b2), padding=1, groups=c2).permute(0, 2, 3, 1).numpy()
    emax, _ = PU.rel_err(_from_bits(out2, dtype), ref2)
    assert emax < _unit_tol(dtype), emax


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hw', [(20, 20), (30, 30), (40, 40), (15, 20), (3, 5)])
def test_attention_kernel(dtype, hw):
    ctx, _ = _ctx(dtype)
    h, w = hw
    n, heads = 2, 4
    rng = np.random.default_rng(7 + h * w)
    qkv = _from_bits(_bits(rng.standard_normal((n, h, w, heads * 128)) * 1.5, dtype), dtype)
    out = np.empty((n, h * w, heads * 64), dtype=np.uint16)
    rc = ctx.lib.mdhip_attention_on(ctx.h, _lib.np_ptr(_bits(qkv, dtype)), _lib.np_ptr(out), n, h * w, heads, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    ref, _ = R.Forward.attention_core(None, torch.from_numpy(qkv).permute(0, 3, 1, 2), heads)
    ref = ref.permute(0, 2, 3, 1).reshape(n, h * w, heads * 64).numpy()
    emax, emean = PU.rel_err(_from_bits(out, dtype), ref)
    # P travels in 16 bits into the P V product: a few storage ulps of the output
    assert emax < 2 * _unit_tol(dtype) and emean < _unit_tol(dtype) / 4, (emax, emean)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(2, 20, 20, 32.0), (1, 15, 20, 8.0), (3, 7, 11, 16.0)])
def test_dfl_decode_bit_exact(dtype, shape):
    ctx, _ = _ctx(dtype)
    n, ny, nx, stride = shape
    nc = 3
    rng = np.random.default_rng(ny * nx)
    box = (rng.standard_normal((n, ny, nx, 64)) * 3).astype(np.float32)
    cls = (rng.standard_normal((n, ny, nx, nc)) * 6).astype(np.float32)
    pred = np.empty((n, ny * nx, 4 + nc), dtype=np.float32)
    rc = ctx.lib.mdhip_dfl_decode_on(ctx.h, _lib.np_ptr(box), _lib.np_ptr(cls), nc, n, ny, nx, float(stride),
                                     _lib.np_ptr(pred), None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    np.testing.assert_array_equal(pred, R.dfl_decode(box, cls, stride))


# ---------------------------------------------------------------------------------------------------------------------
# 2. every layer against the storage-emulating restatement
# ---------------------------------------------------------------------------------------------------------------------
# measured worst figures (max / mean of |d| / |ref| per layer, MI355X): recorded in profiles/yolo11_gpu_tests.txt

def _letterboxed(n, h, w, size, seed):
    imgs = PU.structured_images(n, h, w, seed=seed)
    x, infos = PU.oracle_input(imgs, size, 32)
    lb = [np.ascontiguousarray(i['img_processed']) for i in infos]
    return x, lb


def _layers(ctx, W, x, lb, dtype, worst):
    n, _, hh, ww = x.shape
    ctx.preprocess(lb, [(im.shape[0], im.shape[1], im.shape[0], im.shape[1], 0, 0) for im in lb], hh, ww)
    ctx.forward(n, hh, ww)
    keep = {}
    pred_ref = R.Forward(W, emulate=dtype, keep=keep)(x)
    max_tol = F16_LAYER_MAX_TOL if dtype == 'fp16' else LAYER_MAX_TOL
    mean_tol = F16_LAYER_MEAN_TOL if dtype == 'fp16' else LAYER_MEAN_TOL
    for i in sorted(keep):
        emax, emean = PU.rel_err(ctx.read_layer(i, n), keep[i].numpy())
        worst[0] = max(worst[0], emax)
        worst[1] = max(worst[1], emean)
        assert emax < max_tol and emean < mean_tol, (i, emax, emean)
    pred = ctx.read_predictions(n)
    assert pred.shape == pred_ref.shape
    e_box = PU.rel_err(pred[..., :4], pred_ref[..., :4])
    e_cls = float(np.abs(pred[..., 4:] - pred_ref[..., 4:]).max())
    print('{} {}x{} b{}: worst layer max {:.2e} mean {:.2e}; box {:.2e} / {:.2e}, cls abs {:.2e}'.format(
        dtype, hh, ww, n, worst[0], worst[1], e_box[0], e_box[1], e_cls))
    assert e_box[0] < max_tol and e_box[1] < mean_tol and e_cls < max_tol, (e_box, e_cls)


@pytest.mark.parametrize('dtype', DTYPES)
def test_yolo11n_layers(dtype):
    ctx, W = _ctx(dtype)
    worst = [0.0, 0.0]
    for (h, w), seed in (((640, 640), 3), ((480, 640), 4)):
        x, lb = _letterboxed(2, h, w, 640, seed)
        _layers(ctx, W, x, lb, dtype, worst)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,size', [('YOLO11L_MD', 640), ('YOLO11S_MD', 960)])
def test_md_models_layers(dtype, name, size):
    ctx, W = _ctx(dtype, name, max_batch=1, size=size)
    x, lb = _letterboxed(1, size, size, size, 11)
    _layers(ctx, W, x, lb, dtype, [0.0, 0.0])


# ---------------------------------------------------------------------------------------------------------------------
# 3. anchor-free NMS: bit-exact against the restatement
# ---------------------------------------------------------------------------------------------------------------------

def _af_predictions(seed, batch, n, img, nc=3, conf_lo=0.0):
    g = torch.Generator().manual_seed(seed)
    p = PU.random_predictions(seed, batch, n, img=img)[..., :4]
    cls = torch.rand(batch, n, nc, generator=g) ** 4
    if conf_lo > 0:
        cls = conf_lo + (1 - conf_lo) * cls
    return torch.cat([p, cls], 2).numpy().astype(np.float32)


@pytest.mark.parametrize('thr', [1e-5, 0.2])
def test_anchor_free_nms_bit_exact(thr):
    ctx, _ = _ctx('fp16', max_batch=2, size=640)
    pred = _af_predictions(5, 2, 8400, 640.0)
    out, counts = ctx.nms_on(pred, thr, 0.45, 300)
    ref = R.nms(pred, thr, 0.45, 300)
    for b in range(2):
        assert counts[b] == len(ref[b])
        np.testing.assert_array_equal(out[b, :counts[b]], ref[b])


def _cut_predictions(n, nc=3):
    """every anchor a candidate; the 30000 most confident boxes sit on one spot (a handful survive), the rest are spread
    out (each would survive): whether the rank cut is applied decides the answer"""
    rng = np.random.default_rng(3)
    pred = np.zeros((1, n, 4 + nc), dtype=np.float32)
    conf = np.linspace(0.02, 0.99, n, dtype=np.float32)[rng.permutation(n)]
    cls = rng.integers(0, nc, n)
    pred[0, np.arange(n), 4 + cls] = conf
    top = np.argsort(-conf, kind='stable')[:R.MAX_NMS]
    spread = np.setdiff1d(np.arange(n), top)
    pred[0, :, 0:2] = rng.random((n, 2)).astype(np.float32) * 1200 + 40
    pred[0, :, 2:4] = 20
    pred[0, top, 0:2] = 300 + rng.random((top.size, 2)).astype(np.float32)
    pred[0, top, 2:4] = 200 + rng.random((top.size, 2)).astype(np.float32)
    return pred, spread


def test_anchor_free_nms_class_shift():
    """the hand-built case of tests/test_yolo11_cpu.py: the IoU of the class-2 pair is computed on shifted boxes"""
    ctx, _ = _ctx('fp16', max_batch=2, size=640)
    cx, d = np.float32(100.3), np.float32(3.3333035)
    pred = np.zeros((1, 8400, 7), dtype=np.float32)
    pred[0, 0] = [cx, 200, 10, 10, 0, 0, 0.9]
    pred[0, 1] = [cx + d, 200, 10, 10, 0, 0, 0.8]
    out, counts = ctx.nms_on(pred, 0.1, 0.5, 300)
    assert counts[0] == 2
    np.testing.assert_array_equal(out[0, :2], R.nms(pred, 0.1, 0.5)[0])
    pred[0, :2, 4:] = pred[0, :2, [6, 5, 4]].T
    out, counts = ctx.nms_on(pred, 0.1, 0.5, 300)
    assert counts[0] == 1


def test_anchor_free_nms_30000_cut():
    ctx, _ = _ctx('fp16', max_batch=1, size=1280)
    n = ctx.num_anchors(1280, 1280)
    assert n == 33600
    pred, spread = _cut_predictions(n)
    for max_det in (300, 1000):
        out, counts = ctx.nms_on(pred, 1e-5, 0.45, max_det)
        ref = R.nms(pred, 1e-5, 0.45, max_det)
        assert counts[0] == len(ref[0])
        np.testing.assert_array_equal(out[0, :counts[0]], ref[0])
        # without the cut the spread-out boxes would survive
        assert len(ref[0]) <= 3 < len(R.nms(pred, 1e-5, 0.45, max_det, max_nms=n)[0])
    # clustered random boxes at 1280 x 1280: every anchor a candidate
    pred = _af_predictions(9, 1, n, 1280.0, conf_lo=0.01)
    out, counts = ctx.nms_on(pred, 1e-5, 0.45, 300)
    ref = R.nms(pred, 1e-5, 0.45, 300)
    assert counts[0] == len(ref[0])
    np.testing.assert_array_equal(out[0, :counts[0]], ref[0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end: fake ultralytics checkpoint -> load_detector -> generate_detections_one_batch
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def fake_larch(tmp_path_factory):
    import fake_ultralytics as FU
    model = FU.build_model(yolo_yaml.YOLO11N_TEST, seed=5)
    imgs, _ = _bundled()
    FU.sparsify_classes(model, [O.to_batch_tensor([O.preprocess_image_classic(im, image_size=640, stride=32)['img_processed']])
                                for im in imgs])
    path = str(tmp_path_factory.mktemp('y11') / 'md_v1000.0.0-larch.pt')
    FU.save_checkpoint(model, path, image_size=640)
    FU.uninstall()
    return path


def _bundled():
    from PIL import Image
    files = sorted(f for f in glob.glob(os.path.join(HERE, 'golden', 'bundled_images', '*.*')))
    return [np.asarray(Image.open(f).convert('RGB')) for f in files], [os.path.basename(f) for f in files]


@pytest.mark.parametrize('dtype', ['fp16', 'bf16'])
def test_end_to_end_fake_larch(fake_larch, dtype):
    from megadetector_amd.run_detector import load_detector
    det = load_detector(fake_larch, detector_options={'dtype': dtype, 'batch_size': 4})
    assert det.default_image_size == 640 and det.letterbox_stride == 32
    imgs, ids = _bundled()
    thr = 1e-5
    res = det.generate_detections_one_batch(imgs, ids, detection_threshold=thr)
    W = weights_io.load_checkpoint(fake_larch)
    worst = {}
    for mode in (dtype, None):
        errs = []
        for img, r in zip(imgs, res):
            info = O.preprocess_image_classic(img, image_size=640, stride=32)
            x = O.to_batch_tensor([info['img_processed']])
            pred = R.Forward(W, emulate=mode)(x)
            ref = R.detections(pred, [info], x.shape[2:], thr)[0]
            a = [d for d in r['detections'] if d['conf'] >= 0.005]
            b = [d for d in ref['detections'] if d['conf'] >= 0.005]
            errs.append(O.compare_detection_lists(a, b))
            assert r.get('failure') is None
        worst[mode] = (max(e[0] for e in errs), max(e[1] for e in errs))
    print('{} end to end vs emulating restatement: conf {:.4f} coord {:.4f}; vs fp32: conf {:.4f} coord {:.4f}'.format(
        dtype, *worst[dtype], *worst[None]))
    if dtype == 'fp16':
        assert worst['fp16'][0] <= 0.005 and worst['fp16'][1] <= 0.001, worst


def test_yolo11_refuses_augment_and_fp8(fake_larch):
    from megadetector_amd.detector import HIPDetector
    det = HIPDetector(fake_larch, {'dtype': 'fp16', 'batch_size': 2})
    imgs, ids = _bundled()
    with pytest.raises(ValueError):
        det.generate_detections_one_batch(imgs[:1], ids[:1], augment=True)
    with pytest.raises(ValueError):
        HIPDetector(fake_larch, {'dtype': 'fp8', 'fp8_scales': [1.0]})
    rc = det._ctx.lib.mdhip_forward_tta(det._ctx.h, 1, 640, 640, None)
    assert rc == -4


# ---------------------------------------------------------------------------------------------------------------------
# 5. batch invariance and graph replay
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_batch_invariance_and_graph_replay(dtype):
    ctx, W = _ctx(dtype, max_batch=8, size=640, seed=2)
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
    # graph replay: the second forward of a shape is captured, the third replays it
    ctx.set_graph('on')
    try:
        for _ in range(3):
            ctx.forward(8, hh, ww)
            np.testing.assert_array_equal(ctx.read_predictions(8), p8)
    finally:
        ctx.set_graph('off')
