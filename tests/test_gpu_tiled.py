"""
Tiled inference on the device: mdhip_preprocess_windows (the letterbox kernels reading WINDOWS of a larger pitched device
image) and HIPDetector.generate_detections_for_tiles.

The reference for a window is the dense path on its contiguous crop: the network input must be the same BIT FOR BIT,
and the detections the same dicts.  The parent image lives in an allocation of exactly H * W * 3 bytes, so the
bottom-right tile ends on the allocation's last byte -- the place the kernels' over-read guard exists for.
"""

import ctypes as C

import numpy as np
import pytest
import torch

from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd.detector import HIPDetector
from megadetector_amd.hip_backend import HipContext
from megadetector_amd.postprocess import letterbox_geometry, modern_geometry

pytestmark = pytest.mark.gpu

H, W = 3000, 4100                 # pitch 12300 bytes: row starts fall on every alignment
_STATE = {}


def _image():
    if 'img' not in _STATE:
        _STATE['img'] = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return _STATE['img']


def _parent():
    """the image in a device allocation of exactly its size"""
    if 'parent' not in _STATE:
        t = torch.empty(H * W * 3, dtype=torch.uint8, device='cuda:0')
        t.copy_(torch.from_numpy(_image().reshape(-1)))
        torch.cuda.synchronize()
        _STATE['parent'] = t
    return _STATE['parent']


def _ctx(dtype, max_batch=4, size=1280):
    key = (dtype, max_batch, size)
    if key not in _STATE:
        Wt = weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1)
        _STATE[key] = HipContext(Wt, dtype=dtype, max_batch=max_batch, max_h=size + 64, max_w=size + 64)
    return _STATE[key]


def _origins(tw, th):
    """x = 0, 1, 2, 3 (mod 4), the first and the last row, the bottom-right corner"""
    return [(0, 0), (1, 7), (2, H - th), (1283, 501), (W - tw - 1, 1), (W - tw - 2, 2), (W - tw, H - th), (W - tw, 0)]


def _classic_geom(th, tw, size=1280):
    g = letterbox_geometry((th, tw), new_shape=size, stride=64, auto=True, scaleup=True)
    return (th, tw, g['new_unpad'][1], g['new_unpad'][0], g['top'], g['left'], 0), g['out_hw']


def _modern_geom(th, tw, size=1280):
    m = modern_geometry((th, tw), size, 64)
    g = m['letterbox']
    return (th, tw, m['resized_hw'][0], m['resized_hw'][1], g['top'], g['left'], m['interp']), g['out_hw']


def _compare(ctx, tw, th, geom, out_hw, general=False):
    img, parent = _image(), _parent()
    origins = _origins(tw, th)
    assert {x % 4 for x, _ in origins} == {0, 1, 2, 3}
    pitch, total = W * 3, H * W * 3
    oh, ow = out_hw
    ctx.set_option('letterbox_general', 1 if general else 0)
    try:
        for s in range(0, len(origins), 4):
            chunk = origins[s:s + 4]
            n = len(chunk)
            offs = [y * pitch + x * 3 for x, y in chunk]
            ctx.preprocess_windows([parent.data_ptr() + o for o in offs], [geom] * n, [pitch] * n,
                                   [total - o for o in offs], oh, ow)
            got = ctx.read_input(n, oh, ow)
            crops = [np.ascontiguousarray(img[y:y + th, x:x + tw]) for x, y in chunk]
            ctx.preprocess(crops, [geom] * n, oh, ow)
            want = ctx.read_input(n, oh, ow)
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                'windows {}: {} values differ'.format(chunk, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    finally:
        ctx.set_option('letterbox_general', 0)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_copy_kernel_windows_bit_exact(dtype):
    geom, out_hw = _classic_geom(1280, 1280)
    assert geom[2:4] == (1280, 1280)
    _compare(_ctx(dtype), 1280, 1280, geom, out_hw)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('tile', [(640, 640), (1600, 1200)])
def test_bilinear_kernel_windows_bit_exact(dtype, tile):
    geom, out_hw = _classic_geom(tile[1], tile[0])
    assert geom[2:4] != (tile[1], tile[0])
    _compare(_ctx(dtype), tile[0], tile[1], geom, out_hw)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('tile', [(1280, 1280), (640, 640)])
def test_general_kernel_windows_bit_exact(dtype, tile):
    geom, out_hw = _classic_geom(tile[1], tile[0])
    _compare(_ctx(dtype), tile[0], tile[1], geom, out_hw, general=True)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_modern_mode_inter_area_windows_bit_exact(dtype):
    geom, out_hw = _modern_geom(1200, 1600)
    assert geom[6] == 1, 'a shrinking tile takes INTER_AREA'
    _compare(_ctx(dtype), 1600, 1200, geom, out_hw)


def test_host_pointer_is_rejected_with_a_reason():
    ctx = _ctx('fp16')
    host = np.ascontiguousarray(_image()[:1280, :1280])
    geom, out_hw = _classic_geom(1280, 1280)
    ptrs = (C.c_void_p * 1)(host.ctypes.data)
    from megadetector_amd import _lib
    g = (_lib.mdhip_letterbox * 1)()
    g[0].src_h, g[0].src_w, g[0].resized_h, g[0].resized_w, g[0].top, g[0].left, g[0].interp = geom
    pt = (C.c_int64 * 1)(1280 * 3)
    rd = (C.c_int64 * 1)(host.nbytes)
    rc = ctx.lib.mdhip_preprocess_windows(ctx.h, C.cast(ptrs, C.POINTER(C.c_void_p)), g, pt, rd, 1, out_hw[0], out_hw[1], None)
    assert rc == -1                                     # MDHIP_EINVAL
    assert 'host pointer' in ctx.lib.mdhip_last_error(ctx.h).decode()
    # too little readable memory for the window is refused as well (no kernel is launched)
    parent = _parent()
    with pytest.raises(Exception, match='readable'):
        ctx.preprocess_windows([parent.data_ptr()], [geom], [W * 3], [1279 * W * 3 + 1280 * 3 - 1], out_hw[0], out_hw[1])


# ---------------------------------------------------------------------------------------------------------------------
def _tiles_vs_crops(det, size, tile, n_tiles, augment=False, image_size=None):
    img = _image()[:1500, :2100]
    tw, th = tile
    rng = np.random.default_rng(3)
    origins = [(int(rng.integers(0, img.shape[1] - tw)), int(rng.integers(0, img.shape[0] - th))) for _ in range(n_tiles - 1)]
    origins.append((img.shape[1] - tw, img.shape[0] - th))
    ids = ['t{}'.format(i) for i in range(len(origins))]
    got = det.generate_detections_for_tiles(img, origins, tile, tile_ids=ids, detection_threshold=1e-5,
                                            image_size=image_size, augment=augment)
    crops = [np.ascontiguousarray(img[y:y + th, x:x + tw]) for x, y in origins]
    want = det.generate_detections_one_batch(crops, ids, detection_threshold=1e-5, image_size=image_size, augment=augment)
    assert all(r.get('failure') is None for r in want), want
    assert sum(len(r['detections']) for r in want) > 0
    assert got == want


def _detector(yaml_name, seed, batch, size=640):
    key = ('det', yaml_name, seed, batch, size)
    if key not in _STATE:
        Wt = weights_io.synthetic_weights(getattr(yolo_yaml, yaml_name), seed=seed)
        d = HIPDetector(Wt, {'batch_size': batch, 'max_image_size': size, 'device': 'cuda:0'})
        d.default_image_size = size
        _STATE[key] = d
    return _STATE[key]


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('n_tiles', [3, 9])            # below max_batch; above it and not a multiple of it
def test_yolov5x6_tiles_equal_crops(augment, n_tiles):
    _tiles_vs_crops(_detector('YOLOV5X6_MD', 0, 4), 640, (640, 640), n_tiles, augment=augment)


@pytest.mark.parametrize('yaml_name', ['YOLO11N_TEST', 'YOLOV9_DUAL_TEST'])
def test_anchor_free_models_tiles_equal_crops(yaml_name):
    _tiles_vs_crops(_detector(yaml_name, 0, 4), 640, (640, 480), 6)
    _tiles_vs_crops(_detector(yaml_name, 0, 4), 640, (500, 700), 5)


def test_modern_mode_tiles_equal_crops():
    Wt = weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1)
    d = HIPDetector(Wt, {'batch_size': 4, 'max_image_size': 640, 'device': 'cuda:0', 'compatibility_mode': 'modern'})
    d.default_image_size = 640
    _tiles_vs_crops(d, 640, (900, 700), 5)


def test_tile_outside_the_image_is_an_error():
    d = _detector('YOLO11N_TEST', 0, 4)
    with pytest.raises(ValueError, match='does not lie inside'):
        d.generate_detections_for_tiles(_image()[:700, :700], [(100, 100)], (640, 640))
