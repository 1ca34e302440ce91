"""
YOLOv9-C (MDv1000-cedar) without a GPU: the model description, the yolov9 checkpoint loader (RepConvN folding, grouped
box convs, CBLinear, both head forms), and the CPU restatement of the yolov9 package's NMS and box rescale on hand-built
cases.  Statements tagged [3P] come from the published YOLOv9 architecture, not from the reference tree
(tests/yolov9_ref.py).
"""

import sys

import numpy as np
import pytest
import torch

import fake_yolov9 as FV
import yolov9_ref as R
import yolo11_ref as R11
from oracle import pre_post as O

from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd.postprocess import format_detections, letterbox_geometry
from megadetector_amd.yolo_model import (resolve_yaml, model_strides, MDHIP_ELAN4, MDHIP_ADOWN, MDHIP_CBLINEAR,
                                         MDHIP_CBFUSE, MDHIP_DETECT_DDFL, MDHIP_SILENCE, MDHIP_SPPF)


def _models_loaded():
    return any(m == 'models' or m.startswith('models.') for m in sys.modules)


@pytest.fixture(scope='module', params=['GELAN_TEST', 'YOLOV9_DUAL_TEST'])
def cedar_file(request, tmp_path_factory):
    model = FV.build_model(getattr(yolo_yaml, request.param), seed=2)
    path = str(tmp_path_factory.mktemp('y9cpu') / 'md_v1000.0.0-cedar.pt')
    FV.save_checkpoint(model, path, image_size=640)
    x = torch.rand(2, 3, 160, 224, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        y = model(x)[0]
    ref = [t.transpose(1, 2).numpy() for t in (y if isinstance(y, list) else [y])]
    FV.uninstall()
    return request.param, path, x, ref


# ---- model description ----------------------------------------------------------------------------------------------

def test_both_forms_resolve():
    conv = resolve_yaml(yolo_yaml.GELAN_C_MD)
    assert len(conv) == 24 and conv[0].type == MDHIP_SILENCE and conv[-1].type == MDHIP_DETECT_DDFL
    assert conv[-1].frm == [16, 19, 22] and conv[-1].n == 1 and conv[10].type == MDHIP_SPPF and conv[10].hidden == 256
    assert sum(s.type == MDHIP_ELAN4 for s in conv) == 8 and sum(s.type == MDHIP_ADOWN for s in conv) == 5
    assert model_strides(conv) == [8.0, 16.0, 32.0]
    dual = resolve_yaml(yolo_yaml.YOLOV9C_MD)
    assert len(dual) == 39 and dual[-1].frm == [31, 34, 37, 16, 19, 22] and dual[-1].n == 2 and dual[-1].k == 0
    assert [s.index for s in dual if s.type == MDHIP_CBLINEAR] == [23, 24, 25]
    assert [(s.index, s.hidden) for s in dual if s.type == MDHIP_CBFUSE] == [(30, [0, 0, 0]), (33, [256, 256]), (36, [768])]
    assert dual[26].frm == [0] and model_strides(dual) == [8.0, 16.0, 32.0]
    # the head: c2 = make_divisible(max(ch0 / 4, 64, 16), 4), c3 = max(ch0, min(2 nc, 128)) [3P]
    assert conv[-1].hidden == [(64, 256)]
    assert resolve_yaml(yolo_yaml.GELAN_C_COCO)[-1].hidden == [(64, 256)]


@pytest.mark.parametrize('name,gflops,mparams', [('GELAN_C_COCO', 102.1, 25.3)])
def test_work_and_parameters_against_published(name, gflops, mparams):
    """published nc = 80, 640 x 640 figures of yolov9-c (converted) [3P]; counted here from the graph"""
    g, p = R.count_work(getattr(yolo_yaml, name), 640, 640)
    print('{}: {:.2f} GFLOPs (published {}), {:.3f} M parameters (published {})'.format(name, g, gflops, p / 1e6, mparams))
    assert abs(g / gflops - 1) < 0.01, (g, gflops)
    assert abs(p / 1e6 / mparams - 1) < 0.01, (p, mparams)
    # the training form: the converted network plus the auxiliary branch and its head
    g2, p2 = R.count_work(yolo_yaml.YOLOV9C_COCO, 640, 640)
    print('YOLOV9C_COCO (training form): {:.2f} GFLOPs, {:.3f} M parameters'.format(g2, p2 / 1e6))
    assert g2 > 2 * g and p2 > 1.9 * p


def test_unknown_and_cedar_style_modules_refused():
    yaml = yolo_yaml.make_yolov9_yaml()
    yaml['head'][3] = [-1, 1, 'RepNCSPELAN5', [512, 512, 256, 1]]
    with pytest.raises(ValueError, match='unsupported yolov9 module "RepNCSPELAN5"'):
        resolve_yaml(yaml)
    yaml = yolo_yaml.make_yolov9_yaml()
    yaml['head'][-1] = [[16, 19, 22], 1, 'Detect', ['nc']]
    with pytest.raises(ValueError, match='unsupported yolov9 module "Detect"'):
        resolve_yaml(yaml)
    # a scale-keyed (ultralytics) yaml with yolov9 modules stays refused, naming cedar
    yaml = yolo_yaml.make_yolo11_yaml('l')
    yaml['backbone'][2] = [-1, 1, 'RepNCSPELAN4', [256, 128, 64, 1]]
    with pytest.raises(ValueError, match='cedar'):
        resolve_yaml(yaml)


def test_synthetic_weights_both_forms():
    for name in ('GELAN_TEST', 'YOLOV9_DUAL_TEST', 'GELAN_C_MD', 'YOLOV9C_MD'):
        W = weights_io.synthetic_weights(getattr(yolo_yaml, name))
        assert W.anchor_free and W.yolov9 and W.na == 1 and W.nl == 3 and W.max_stride == 32
        assert W.weights['model.{}.cv2.0.1.conv.weight'.format(W.specs[-1].index)].shape[1] * 4 == \
            W.weights['model.{}.cv2.0.1.conv.weight'.format(W.specs[-1].index)].shape[0]


# ---- checkpoint loader ----------------------------------------------------------------------------------------------

def test_repconvn_fold_equals_unfused_module_fp64():
    common, _ = FV._install()
    try:
        torch.manual_seed(0)
        m = common.RepConvN(16, 24).double().eval()
        g = torch.Generator().manual_seed(3)
        for conv in (m.conv1, m.conv2):
            nf = conv.bn.num_features
            conv.conv.weight.data = torch.randn(conv.conv.weight.shape, generator=g).double() / 6
            conv.bn.weight.data = (0.5 + torch.rand(nf, generator=g)).double()
            conv.bn.bias.data = (0.2 * torch.randn(nf, generator=g)).double()
            conv.bn.running_mean.data = (0.3 * torch.randn(nf, generator=g)).double()
            conv.bn.running_var.data = (0.5 + torch.rand(nf, generator=g)).double()
        x = torch.randn(2, 16, 9, 11, generator=g).double()
        with torch.no_grad():
            ref = m(x)
        w, b = weights_io._fold_repconvn(m.float())
        got = torch.nn.functional.silu(torch.nn.functional.conv2d(x, torch.from_numpy(w).double(),
                                                                  torch.from_numpy(b).double(), padding=1))
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < 1e-6, err          # the fold itself is exact; fp32 weights are all that differ
    finally:
        FV.uninstall()


def test_fake_cedar_checkpoint_loads(cedar_file):
    name, path, _, _ = cedar_file
    assert not _models_loaded()
    W = weights_io.load_checkpoint(path)
    assert not _models_loaded()                                             # nothing imported a yolov9 package
    assert W.anchor_free and W.yolov9 and W.nc == 3 and W.strides == [8.0, 16.0, 32.0]
    meta = weights_io.read_metadata_from_megadetector_model_file(path)
    assert meta['image_size'] == 640 and meta['model_type'] == 'yolov9'
    # the expected conv list: every conv of the description, in the order of include/mdhip.h, at its checkpoint shape
    specs = W.specs
    expect = [(n, shp) for s in specs for n, shp in weights_io.yolov9_conv_shapes(s, specs)]
    assert [n for n, _ in expect] == [n for s in specs for n in s.conv_names]
    for n, (c2, c1, k) in expect:
        assert W.weights[n + '.weight'].shape == (c2, c1, k, k), n
    det = specs[-1]
    assert det.n == (2 if name == 'YOLOV9_DUAL_TEST' else 1)
    assert len(det.conv_names) == 6 * 3 * det.n


def test_folded_weights_reproduce_the_module(cedar_file):
    _, path, x, ref = cedar_file
    W = weights_io.load_checkpoint(path)
    fw = R.Forward(W)
    out = fw(x)
    for h, r in enumerate(ref):
        got = fw.heads[h]
        err = np.abs(got - r).max() / np.abs(r).max()
        assert err <= 1e-5, (h, err)
    np.testing.assert_array_equal(out, fw.heads[0])                         # the head yolov9's NMS reads


def test_foreign_package_refused(tmp_path):
    """a yolov9 yaml in a checkpoint whose classes come from another package root"""
    import fake_ultralytics as FU
    model = FU.build_model(yolo_yaml.YOLO11N_TEST, seed=1)
    model.yaml = dict(yolo_yaml.GELAN_TEST)
    path = str(tmp_path / 'odd.pt')
    FU.save_checkpoint(model, path)
    FU.uninstall()
    with pytest.raises(ValueError):
        weights_io.load_checkpoint(path)


# ---- the two pools, restated ------------------------------------------------------------------------------------------

def test_adown_pool_restatement_matches_torch():
    """the zero-padded H x W average buffer under a 3x3 / s2 / p1 conv equals the conv over the (H-1) x (W-1) average, and
    the clipped max equals max_pool2d(3, 2, 1) [3P]"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 12, 10, generator=g).to(torch.bfloat16).float()
    A, B = R.adown_pool(x.permute(0, 2, 3, 1).numpy(), 'bf16')
    avg = torch.nn.functional.avg_pool2d(x, 2, 1, 0, False, True).to(torch.bfloat16).float()
    w = torch.randn(8, 8, 3, 3, generator=g)
    ref = torch.nn.functional.conv2d(avg[:, :8], w, stride=2, padding=1)
    got = torch.nn.functional.conv2d(torch.from_numpy(A).permute(0, 3, 1, 2), w, stride=2, padding=1)
    assert got.shape == ref.shape == (2, 8, 6, 5)
    torch.testing.assert_close(got, ref, rtol=0, atol=0)
    np.testing.assert_array_equal(B, torch.nn.functional.max_pool2d(avg[:, 8:], 3, 2, 1).permute(0, 2, 3, 1).numpy())


# ---- NMS [3P]: yolov9 against the YOLO11 rule the kernel implements ----------------------------------------------------

def test_yolov9_nms_equals_anchor_free_rule_and_unwraps_lists():
    """yolov9 sorts the candidates every time, ultralytics only above the cut: with ties kept in anchor order both give
    the same answer -- the HIP kernel's anchor-free mode serves both"""
    g = torch.Generator().manual_seed(4)
    n = 3000
    p = torch.rand(2, n, 7, generator=g)
    p[..., :2] *= 640
    p[..., 2:4] = 8 + 60 * p[..., 2:4]
    p[..., 4:] = (p[..., 4:] * 20).round() / 20               # many exact ties
    pred = p.numpy().astype(np.float32)
    for thr in (1e-5, 0.3):
        a, b = R.nms(pred, thr, 0.45), R11.nms(pred, thr, 0.45)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        c = R.nms([pred, pred[:, ::-1].copy()], thr, 0.45)   # DualDDetect's list: the first element is used
        for x, y in zip(c, a):
            np.testing.assert_array_equal(x, y)


def test_scale_boxes_does_not_round_the_padding():
    """yolov9's scale_boxes is YOLOv5's: format_detections with round_pad=False equals the restatement"""
    rng = np.random.default_rng(4)
    for img0 in ((333, 640, 3), (480, 640, 3), (21, 244, 3), (349, 156, 3)):
        gm = letterbox_geometry(img0[:2], new_shape=640, stride=32)
        batch_hw = gm['out_hw']
        k = 12
        xy = rng.random((k, 2)) * np.array([batch_hw[1], batch_hw[0]]) * 0.8
        wh = 5 + rng.random((k, 2)) * 60
        det = np.concatenate([xy, xy + wh, np.sort(rng.random((k, 1)), 0)[::-1], rng.integers(0, 3, (k, 1))], 1)
        det = det.astype(np.float32)
        a, ma = format_detections(det, batch_hw, img0, img0, 0.1, round_pad=False)
        b, mb = R.format_detections(det, batch_hw, img0, img0, 0.1)
        assert a == b and ma == mb
    # (352, 640) from (333, 640): pad 9.5, not the ultralytics 9
    box = torch.tensor([[100.0, 50.0, 200.0, 150.0]])
    assert float(R.scale_boxes((352, 640), box, (333, 640, 3))[0, 1]) == 40.5


def test_preprocess_only_on_fake_cedar(cedar_file):
    from megadetector_amd.detector import HIPDetector
    _, path, _, _ = cedar_file
    det = HIPDetector(path, {'preprocess_only': True})
    assert det.default_image_size == 640 and det.letterbox_stride == 32
    info = det.preprocess_image(np.zeros((480, 640, 3), dtype=np.uint8), 'x.jpg')
    assert info['img_processed'].shape == (480, 640, 3)


def test_parity_real_knows_cedar():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('parity_real', os.path.join(os.path.dirname(__file__), '..', 'tools',
                                                                              'parity_real.py'))
    PR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PR)
    assert 'MDV1000_CEDAR' in PR.MODEL_ENV
