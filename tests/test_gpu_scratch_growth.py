"""
The scratch buffers a context keeps between calls (csrc/mdhip_ctx.h DevBuffer): first allocation, growth, reuse, release.

The context the other GPU tests share is warm, so none of them shows a buffer's first allocation or a growth.  Here every
test takes a FRESH context and makes three calls that use one buffer: an image of 16 x 16 (the first allocation), one of
72 x 40 (every buffer's layout is larger for it: the buffer grows) and 16 x 16 again (the grown buffer is reused).  Each
result is compared bit for bit with the host model the neighbouring GPU test of that entry point uses.  Then a second
context is created, the first destroyed (mdhip_destroy releases its buffers), and the small call repeated on the second.
"""

import numpy as np
import pytest
import torch

import jpeg_fixtures as JF
import parity_util as PU
from megadetector_amd import jpeg_host, weights_io, yolo_yaml
from megadetector_amd.hip_backend import HipContext
from test_blur_cpu import content, pillow_blur_regions
from test_gpu_jpeg_entropy import _entropy_decode, _scan_images
from test_gpu_tile_jpeg import _round_trip
from test_tile_jpeg_cpu import make_content, pillow_file

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (72, 40), (16, 16)]          # w x h
_STATE = {}


def _fresh():
    if 'weights' not in _STATE:
        _STATE['weights'] = weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1)
    return HipContext(_STATE['weights'], dtype='fp16', max_batch=2, max_h=320, max_w=320)


def _three_calls_then_a_second_context(call):
    """call(ctx, k, (w, h)) uses the entry point once on an image of that size and checks what it gave"""
    first = _fresh()
    try:
        for k, size in enumerate(SIZES):
            call(first, k, size)
        second = _fresh()
    finally:
        first.close()
    try:
        call(second, len(SIZES), SIZES[0])
    finally:
        second.close()


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to('cuda:0')
    torch.cuda.synchronize()
    return t


def test_stage_of_host_images():
    """mdhip_preprocess of an image in host memory stages 768, then 8640 bytes: the network input is the oracle's letterbox"""
    from megadetector_amd.postprocess import letterbox_geometry

    def call(ctx, k, size):
        w, h = size
        imgs = PU.structured_images(1, h, w, seed=k)
        g = letterbox_geometry((h, w), new_shape=64, stride=64)
        oh, ow = g['out_hw']
        ctx.preprocess(imgs, [(h, w, g['new_unpad'][1], g['new_unpad'][0], g['top'], g['left'])], oh, ow)
        x, _ = PU.oracle_input(imgs, 64, 64)
        assert tuple(x.shape[2:]) == (oh, ow)
        np.testing.assert_array_equal(ctx.read_input(1, oh, ow), x.half().float().numpy())

    _three_calls_then_a_second_context(call)


def test_jpeg_planes_of_a_recompressed_window():
    """mdhip_jpeg_recompress keeps 512, then 4864 bytes of component planes: the pixels are Pillow's save + open"""
    def call(ctx, k, size):
        w, h = size
        rgb = make_content('noise', w, h, seed=k)
        src = _device(rgb)
        out = torch.full((h * w * 3,), 0xA5, dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        ctx.jpeg_recompress([src.data_ptr()], [(w, h)], [w * 3], 95, [out.data_ptr()])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().reshape(h, w, 3), _round_trip(rgb, 95))

    _three_calls_then_a_second_context(call)


def test_jpeg_entropy_scratch(tmp_path):
    """mdhip_jpeg_entropy_decode of a 4:4:4 noise file of 12, then 135 blocks: the coefficients are mdjpeg_decode's"""
    J = JF.ensure_libmdjpeg()

    def call(ctx, k, size):
        w, h = size
        data = open(JF.write_jpeg(str(tmp_path / '{}.jpg'.format(k)), JF.content('noise', w, h, seed=k), '444', 95), 'rb').read()
        status, planes, _ = _entropy_decode(ctx, _scan_images([data]))
        assert status[0] == 0
        rc, _, want = J.decode(data)
        assert rc == 0
        np.testing.assert_array_equal(planes[0], want)

    _three_calls_then_a_second_context(call)


def test_jpeg_encode_scratch():
    """mdhip_jpeg_encode of a crop of 6, then 90 blocks: the file around the scan is the one Pillow saves"""
    def call(ctx, k, size):
        w, h = size
        rgb = make_content('noise', w, h, seed=k)
        src = _device(rgb)
        capacity = ctx.jpeg_encode_bound(w, h)
        buf = torch.full((capacity,), 0xA5, dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        fits, offs, lens, needed = ctx.jpeg_encode([src.data_ptr()], [(w, h)], [w * 3], 95, buf.data_ptr(), capacity)
        assert fits and offs[0] == 0 and lens[0] == needed
        scan = buf.cpu().numpy()[:needed].tobytes()
        assert jpeg_host.jfif_file(w, h, 95, scan) == pillow_file(rgb, 95)

    _three_calls_then_a_second_context(call)


def test_blur_scratch():
    """mdhip_blur_regions of the whole image, two planes of 1024, then 10240 bytes: the pixels are the host model's and Pillow's"""
    def call(ctx, k, size):
        w, h = size
        rgb = content(w, h, k)
        dev = _device(rgb)
        ctx.blur_regions([dev.data_ptr()], [(w, h)], [w * 3], [0], [(0, 0, w, h)], 4)
        torch.cuda.synchronize()
        want = rgb.copy()
        assert jpeg_host.blur_regions(want, [(0, 0, w, h)], 4) == jpeg_host.MDJPEG_OK
        np.testing.assert_array_equal(dev.cpu().numpy().reshape(rgb.shape), want)
        np.testing.assert_array_equal(want, pillow_blur_regions(rgb, [(0, 0, w, h)], 4))

    _three_calls_then_a_second_context(call)
