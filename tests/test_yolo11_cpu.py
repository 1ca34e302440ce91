"""
YOLO11 (MDv1000-larch / -sorrel) without a GPU: the model description, the ultralytics checkpoint loader, and the CPU
restatement of the parts the package computes around the network (NMS, scale_boxes) on hand-built cases.  Statements
tagged [3P] come from the published ultralytics architecture, not from the reference tree (tests/yolo11_ref.py).
"""

import os
import pickle

import numpy as np
import pytest
import torch

import fake_ultralytics as FU
import yolo11_ref as R
from oracle import pre_post as O

from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd.postprocess import format_detections, letterbox_geometry
from megadetector_amd.yolo_model import resolve_yaml


@pytest.fixture(scope='module')
def larch_file(tmp_path_factory):
    model = FU.build_model(yolo_yaml.YOLO11N_TEST, seed=2)
    path = str(tmp_path_factory.mktemp('y11cpu') / 'md_v1000.0.0-larch.pt')
    FU.save_checkpoint(model, path, image_size=640)
    x = torch.rand(2, 3, 160, 224, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        ref = model(x).numpy()
    FU.uninstall()
    return path, x, ref


# ---- model description / loader -----------------------------------------------------------------------------------

def test_checkpoint_reads_without_ultralytics(larch_file):
    path, _, _ = larch_file
    import sys
    assert not any(m == 'ultralytics' or m.startswith('ultralytics.') for m in sys.modules)     # the fake is uninstalled
    W = weights_io.load_checkpoint(path)
    assert not any(m == 'ultralytics' or m.startswith('ultralytics.') for m in sys.modules)     # nothing imported it
    assert W.anchor_free and W.nc == 3 and W.strides == [8.0, 16.0, 32.0] and W.max_stride == 32
    assert weights_io.read_metadata_from_megadetector_model_file(path)['image_size'] == 640


def test_folded_weights_reproduce_the_module(larch_file):
    path, x, ref = larch_file
    W = weights_io.load_checkpoint(path)
    out = R.Forward(W)(x)
    err = np.abs(out - ref).max() / np.abs(ref).max()
    assert err <= 1e-5, err


def test_legacy_head_refused(tmp_path):
    model = FU.build_model(yolo_yaml.YOLO11N_TEST, seed=1, legacy=True)
    path = str(tmp_path / 'legacy.pt')
    FU.save_checkpoint(model, path)
    FU.uninstall()
    with pytest.raises(ValueError, match='legacy'):
        weights_io.load_checkpoint(path)


def test_cedar_style_modules_refused():
    yaml = yolo_yaml.make_yolo11_yaml('l')
    yaml['backbone'][2] = [-1, 1, 'RepNCSPELAN4', [256, 128, 64, 1]]
    with pytest.raises(ValueError, match='cedar'):
        resolve_yaml(yaml)
    yaml = yolo_yaml.make_yolo11_yaml('l')
    yaml['head'][-1] = [[16, 19, 22], 1, 'DualDDetect', ['nc']]
    with pytest.raises(ValueError, match='unsupported'):
        resolve_yaml(yaml)
    yaml = yolo_yaml.make_yolo11_yaml('l')
    del yaml['scale']
    with pytest.raises(ValueError, match='scale'):
        resolve_yaml(yaml)


class _Evil:
    def __reduce__(self):
        return (os.system, ('echo never',))


def test_foreign_callables_refused(tmp_path):
    path = str(tmp_path / 'evil.pt')
    torch.save({'model': _Evil()}, path)
    with pytest.raises(pickle.UnpicklingError):
        weights_io.load_checkpoint(path)


@pytest.mark.parametrize('name,gflops,mparams', [('YOLO11N_COCO', 6.5, 2.6), ('YOLO11S_COCO', 21.5, 9.4),
                                                  ('YOLO11L_COCO', 86.9, 25.3)])
def test_work_and_parameters_against_published(name, gflops, mparams):
    """published nc = 80, 640 x 640 figures of yolo11n / s / l [3P]; counted here from the graph (2 x MACs of every conv
    and of the two attention products; fused parameters)"""
    g, p = R.count_work(getattr(yolo_yaml, name), 640, 640)
    assert abs(g / gflops - 1) < 0.03, (g, gflops)
    assert abs(p / 1e6 / mparams - 1) < 0.03, (p, mparams)


def test_synthetic_weights_shapes_and_candidate_load():
    for name in ('YOLO11N_TEST', 'YOLO11S_MD', 'YOLO11L_MD'):
        W = weights_io.synthetic_weights(getattr(yolo_yaml, name))
        assert W.anchor_free and W.na == 1
    W = weights_io.synthetic_weights(yolo_yaml.YOLO11N_TEST)
    pred = R.Forward(W)(torch.rand(1, 3, 320, 320, generator=torch.Generator().manual_seed(1)))
    share = float((pred[..., 4:].max(-1) > 1e-5).mean())
    assert 0.02 < share < 0.6, share


# ---- NMS [3P]: hand-built known answers ----------------------------------------------------------------------------

def _row(cx, cy, w, h, *cls):
    return [cx, cy, w, h] + list(cls)


def test_nms_threshold_is_strict_and_has_no_objectness():
    pred = np.array([[_row(100, 100, 20, 20, 0.25, 0.1, 0.0),
                      _row(300, 300, 20, 20, 0.2, 0.0, 0.0),          # exactly at the threshold: dropped
                      _row(500, 500, 20, 20, 0.0, 0.0, 0.2000001)]], dtype=np.float32)
    out = R.nms(pred, 0.2, 0.45)[0]
    assert out.shape == (2, 6)
    np.testing.assert_array_equal(out[:, 5], [0, 2])
    np.testing.assert_array_equal(out[:, 4], np.float32([0.25, 0.2000001]))
    np.testing.assert_array_equal(out[0, :4], np.float32([90, 90, 110, 110]))


def test_nms_class_shift_changes_the_iou_rounding():
    """two 10 x 10 boxes 3.3333035 px apart: IoU = (10 - d) / (10 + d), a hair above 0.5.  As class 0 (no shift) the
    second box is suppressed; as class 2 the boxes are compared at x + 15360, where the fp32 coordinates round to a
    multiple of 2^-9 and the IoU no longer exceeds 0.5: both survive.  The HIP kernel compares the shifted boxes too."""
    cx, d = np.float32(100.3), np.float32(3.3333035)
    pred = np.array([[_row(cx, 200, 10, 10, 0, 0, 0.9), _row(cx + d, 200, 10, 10, 0, 0, 0.8)]], dtype=np.float32)
    out = R.nms(pred, 0.1, 0.5)[0]
    assert len(out) == 2
    np.testing.assert_array_equal(out[:, 0], [cx - np.float32(5), (cx + d) - np.float32(5)])     # unshifted output
    pred[0, :, 4:] = pred[0, :, [6, 5, 4]].T
    assert len(R.nms(pred, 0.1, 0.5)[0]) == 1


def test_nms_rank_cut_and_max_det():
    n = R.MAX_NMS + 50
    pred = np.zeros((1, n, 7), dtype=np.float32)
    conf = np.linspace(0.9, 0.1, n, dtype=np.float32)
    pred[0, :, 4] = conf
    pred[0, :R.MAX_NMS, 0:2] = 100                 # the 30000 most confident: one spot
    pred[0, :, 2:4] = 10
    pred[0, R.MAX_NMS:, 0] = 200 + 20 * np.arange(50, dtype=np.float32)
    pred[0, R.MAX_NMS:, 1] = 300
    assert len(R.nms(pred, 0.05, 0.45)[0]) == 1                              # the spread-out tail is cut
    assert len(R.nms(pred, 0.05, 0.45, max_nms=n)[0]) == 51
    assert len(R.nms(pred, 0.05, 0.45, max_det=7, max_nms=n)[0]) == 7


# ---- box rescale [3P] -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('img1,img0,expect_pad', [
    ((640, 640), (480, 640, 3), (0, 80)),          # gain 1: (640 - 480) / 2 - 0.1 = 79.9 -> 80
    ((384, 640), (300, 500, 3), (0, 0)),           # gain 1.28: no padding, round(-0.1) = 0
    ((640, 512), (1000, 750, 3), (16, 0)),         # gain 0.64: (512 - 480) / 2 - 0.1 = 15.9 -> 16
    ((352, 640), (333, 640, 3), (0, 9)),           # gain 1: (352 - 333) / 2 - 0.1 = 9.4 -> 9 (YOLOv5: 9.5)
])
def test_scale_boxes_rounds_the_padding(img1, img0, expect_pad):
    gain = min(img1[0] / img0[0], img1[1] / img0[1])
    pad = expect_pad
    box = torch.tensor([[100.0, 50.0, 200.0, 150.0]])
    got = R.scale_boxes(img1, box, img0)
    ref = box.clone()
    ref[:, [0, 2]] -= pad[0]
    ref[:, [1, 3]] -= pad[1]
    ref /= gain
    ref[:, [0, 2]] = ref[:, [0, 2]].clamp(0, img0[1])
    ref[:, [1, 3]] = ref[:, [1, 3]].clamp(0, img0[0])
    torch.testing.assert_close(got, ref, rtol=0, atol=0)


def test_format_detections_round_pad_matches_restatement():
    rng = np.random.default_rng(4)
    for img0 in ((333, 640, 3), (480, 640, 3), (21, 244, 3), (349, 156, 3)):
        g = letterbox_geometry(img0[:2], new_shape=640, stride=32)
        batch_hw = g['out_hw']
        k = 12
        xy = rng.random((k, 2)) * np.array([batch_hw[1], batch_hw[0]]) * 0.8
        wh = 5 + rng.random((k, 2)) * 60
        det = np.concatenate([xy, xy + wh, np.sort(rng.random((k, 1)), 0)[::-1], rng.integers(0, 3, (k, 1))], 1)
        det = det.astype(np.float32)
        a, ma = format_detections(det, batch_hw, img0, img0, 0.1, round_pad=True)
        b, mb = R.format_detections(det, batch_hw, img0, img0, 0.1)
        assert a == b and ma == mb
    # the keyword defaults to the YOLOv5 rescale
    det = np.array([[100.3, 80.2, 200.7, 180.9, 0.9, 0]], dtype=np.float32)
    a, _ = format_detections(det, (352, 640), (333, 640, 3), (333, 640, 3), 0.1)
    b, _ = O.format_detections(torch.from_numpy(det), (352, 640), (333, 640, 3), (333, 640, 3), 0.1)
    assert a == b


def test_letterbox_wrapper_arithmetic_matches_letterbox_geometry():
    """the reference's ultralytics letterbox wrapper (pytorch_detector.py:406-454) reverse-engineers ratio and pad as
    below; they equal letterbox_geometry's (what the HIP letterbox kernel uses)"""
    for shape in ((480, 640), (21, 244), (349, 156), (1000, 750), (640, 640), (333, 500)):
        for new_shape, stride in ((640, 32), (960, 32)):
            r = min(new_shape / shape[0], new_shape / shape[1])
            new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
            dw, dh = np.mod(new_shape - new_unpad[0], stride) / 2, np.mod(new_shape - new_unpad[1], stride) / 2
            g = letterbox_geometry(shape, new_shape=new_shape, stride=stride, auto=True, scaleup=True)
            assert g['ratio'] == (r, r) and tuple(g['new_unpad']) == new_unpad
            assert tuple(g['pad']) == (dw, dh)


def test_preprocess_only_on_fake_larch(larch_file):
    from megadetector_amd.detector import HIPDetector
    path, _, _ = larch_file
    det = HIPDetector(path, {'preprocess_only': True})
    assert det.default_image_size == 640 and det.letterbox_stride == 32
    info = det.preprocess_image(np.zeros((480, 640, 3), dtype=np.uint8), 'x.jpg')
    assert info['img_processed'].shape == (480, 640, 3)


def test_parity_real_takes_other_models(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location('parity_real', os.path.join(os.path.dirname(__file__), '..', 'tools',
                                                                              'parity_real.py'))
    PR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PR)
    f = tmp_path / 'md_v1000.0.0-larch.pt'
    f.write_bytes(b'x')
    for var in PR.MODEL_ENV:
        monkeypatch.delenv(var, raising=False)
    assert PR.resolve_model(None) is None
    assert PR.resolve_model(str(f)) == str(f)
    monkeypatch.setenv('MDV1000_LARCH', str(f))
    assert PR.resolve_model('MDV1000-larch') == str(f)
    assert PR.resolve_model(None) == str(f)
