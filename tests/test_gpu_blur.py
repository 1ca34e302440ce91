"""
Privacy blurring on the device: mdhip_blur_regions (HipContext.blur_regions) against Pillow's ImageFilter.GaussianBlur, bit for
bit and byte-exact in place, and HIPDetector(blur=) against the reference's pipeline (blur_detections, save(quality=85)) on
the same pixels and detections.  The rectangle matrix, the contents and the Pillow pipeline are those of test_blur_cpu.py.
"""

import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from megadetector_amd import blur as B
from megadetector_amd import jpeg_host as J
from megadetector_amd._lib import HipError
from test_blur_cpu import (IMG_H, IMG_W, PITCH, content, pillow_blur_regions, rectangle_matrix, reference_blurred_file,
                           strided_image)
from test_gpu_tile_jpeg import _ctx

pytestmark = pytest.mark.gpu

_STATE = {}
FIRST = 3 * PITCH + 60                  # the image's first byte within its sentinel-filled allocation (strided_image)


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to('cuda:0')
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize('radius', [40, 2, 7.5, 100])
def test_rectangle_matrix_equals_pillow_and_nothing_else_is_written(radius):
    """every rectangle of the matrix in an image of its own -- ONE call, one launch round -- inside an allocation filled with
    a sentinel: the rectangle is Pillow's, every other byte of the allocation is what it was"""
    ctx, rects = _ctx(), rectangle_matrix()
    backing, view = strided_image()
    source = view.copy()
    n = len(rects)
    dev = _device(np.stack([backing] * n))
    per = backing.size
    ctx.blur_regions([dev.data_ptr() + i * per + FIRST for i in range(n)], [(IMG_W, IMG_H)] * n, [PITCH] * n, list(range(n)), rects, radius)
    torch.cuda.synchronize()
    got = dev.cpu().numpy().reshape((n,) + backing.shape)
    for i, rect in enumerate(rects):
        want = backing.copy()
        want[3:3 + IMG_H, 60:60 + IMG_W * 3] = pillow_blur_regions(source, [rect], radius).reshape(IMG_H, IMG_W * 3)
        np.testing.assert_array_equal(got[i], want, err_msg='rectangle {} {} at radius {}'.format(i, rect, radius))
    assert any(not np.array_equal(got[i], backing) for i in range(n))


def test_three_images_with_zero_one_and_three_rectangles_equal_the_host_model():
    ctx = _ctx()
    images = [content(64, 48, 1), content(301, 177, 2), content(150, 260, 3)]
    lists = [[], [(20, 30, 280, 170)], [(10, 10, 100, 200), (60, 120, 150, 260), (0, 0, 150, 40)]]      # the last three overlap
    devs = [_device(a) for a in images]
    # interleaved, so that the order within an image is the order of the list and not the position in the call
    order = [1, 0, 2, 3]
    flat = [(i, r) for i, l in enumerate(lists) for r in l]
    flat = [flat[k] for k in order]
    assert [r for i, r in flat if i == 2] == lists[2]
    ctx.blur_regions([d.data_ptr() for d in devs], [(a.shape[1], a.shape[0]) for a in images], [a.shape[1] * 3 for a in images],
                     [i for i, _ in flat], [r for _, r in flat], 40)
    torch.cuda.synchronize()
    for a, d, l in zip(images, devs, lists):
        want = a.copy()
        assert J.blur_regions(want, l, 40) == J.MDJPEG_OK
        np.testing.assert_array_equal(d.cpu().numpy().reshape(a.shape), want)
        np.testing.assert_array_equal(want, pillow_blur_regions(a, l, 40))
    assert np.array_equal(devs[0].cpu().numpy().reshape(images[0].shape), images[0])
    # the other order of the overlapping rectangles gives other pixels
    d = _device(images[2])
    ctx.blur_regions([d.data_ptr()], [(150, 260)], [450], [0, 0, 0], lists[2][::-1], 40)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy().reshape(images[2].shape), pillow_blur_regions(images[2], lists[2][::-1], 40))
    assert not np.array_equal(d.cpu().numpy(), devs[2].cpu().numpy())


@pytest.mark.parametrize('case', [(1021, 9, 40), (1022, 9, 40), (4100, 3, 200), (8200, 2, 350)], ids=str)
def test_rows_wider_than_one_chunk(case):
    """the row stage keeps eight rows of up to 1021 pixels on chip (blur_box.h md_blur_plan_x with 49152 bytes): 1021 is the
    widest row in one piece at radius 40, 1022 the narrowest in chunks with a halo; at radius 200 (halo 594) a row of 4100
    pixels is cut at two rows a workgroup, and at radius 350 one of 8200 at one row a workgroup"""
    w, h, radius = case
    ctx = _ctx()
    rgb = content(w, h, w)
    d = _device(rgb)
    ctx.blur_regions([d.data_ptr()], [(w, h)], [w * 3], [0], [(0, 0, w, h)], radius)
    torch.cuda.synchronize()
    want = np.asarray(Image.fromarray(rgb).filter(ImageFilter.GaussianBlur(radius)))
    np.testing.assert_array_equal(d.cpu().numpy().reshape(rgb.shape), want)


def test_bad_arguments_are_refused_and_nothing_is_changed():
    ctx = _ctx()
    rgb = content(64, 48, 4)
    d = _device(rgb)
    args = ([d.data_ptr()], [(64, 48)], [192])
    for rects in ([(0, 0, 65, 10)], [(0, 0, 10, 10), (-1, 0, 5, 5)], [(0, 40, 10, 49)]):
        with pytest.raises(HipError, match='leaves'):
            ctx.blur_regions(*args, [0] * len(rects), rects, 40)
    with pytest.raises(HipError):
        ctx.blur_regions(*args, [1], [(0, 0, 10, 10)], 40)
    with pytest.raises(HipError, match='radius'):
        ctx.blur_regions(*args, [0], [(0, 0, 10, 10)], -1)
    with pytest.raises(HipError, match='radius'):
        ctx.blur_regions(*args, [0], [(0, 0, 10, 10)], 513)
    with pytest.raises(HipError, match='pitch'):
        ctx.blur_regions([d.data_ptr()], [(64, 48)], [191], [0], [(0, 0, 10, 10)], 40)
    with pytest.raises(HipError, match='host pointer'):
        ctx.blur_regions([rgb.ctypes.data], [(64, 48)], [192], [0], [(0, 0, 10, 10)], 40)
    ctx.blur_regions(*args, [0, 0, 0], [(5, 5, 5, 9), (9, 5, 5, 9), (0, 0, 0, 0)], 40)          # without area: skipped
    ctx.blur_regions(*args, [], [], 40)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy().reshape(rgb.shape), rgb)


def _yolo_detector(batch):
    from megadetector_amd import weights_io, yolo_yaml
    from megadetector_amd.detector import HIPDetector
    key = ('det', batch)
    if key not in _STATE:
        d = HIPDetector(weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1), {'batch_size': batch, 'max_image_size': 320, 'device': 'cuda:0'})
        d.default_image_size = 320
        _STATE[key] = d
    return _STATE[key]


def test_detector_blur_synchronous_and_pipelined_equal_the_pillow_pipeline():
    from megadetector_amd import crops as K
    from test_gpu_tile_jpeg import _image
    det = _yolo_detector(4)
    imgs = [np.ascontiguousarray(_image()[y:y + h, x:x + w]) for x, y, w, h in
            [(0, 0, 400, 300), (1500, 100, 333, 257), (100, 400, 320, 240), (900, 900, 301, 199)]]
    names = ['a.jpg', 'd/b.jpeg', 'e.png', 'g.jpg']
    sources = [a.copy() for a in imgs]
    opt = B.BlurOptions(category_names=('animal', 'person', 'vehicle'), confidence_threshold=0.0)
    copt = K.CropOptions(confidence_threshold=0.0)
    plain = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5)
    cropped = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, crops=copt)
    before = dict(det.blur_counts)
    sync = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, blur=opt)
    both = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, crops=copt, blur=opt)
    tickets = [det.start_batch(imgs[:3], names[:3], detection_threshold=1e-5, crops=copt, blur=opt),
               det.start_batch(imgs[3:], names[3:], detection_threshold=1e-5, crops=copt, blur=opt)]
    piped = det.finish_batch(tickets[0]) + det.finish_batch(tickets[1])
    one = det.generate_detections_one_image(imgs[1], names[1], detection_threshold=1e-5, blur=opt)
    strip = lambda res, *keys: [{k: v for k, v in r.items() if k not in keys} for r in res]
    assert strip(sync, 'blurred') == plain and strip(both, 'blurred') == cropped and strip(cropped, 'crops') == plain
    assert both == piped and one == sync[1]
    assert [r['blurred'] for r in sync] == [r['blurred'] for r in both]
    assert all(np.array_equal(a, b) for a, b in zip(imgs, sources))
    blurred = 0
    for r, img in zip(sync, imgs):
        assert r.get('failure') is None
        want = reference_blurred_file(img, r['file'], r['detections'], opt)
        print(r['file'], len(r['detections']), 'detections;', None if want is None else len(want), 'bytes')
        assert r['blurred'] == want
        if want is not None:
            blurred += 1
            assert not np.array_equal(np.asarray(Image.open(io.BytesIO(want)).convert('RGB')), img)
    assert blurred >= 1, 'the test blurred nothing'
    n_png = int(sync[2]['blurred'] is not None)
    assert det.blur_counts['host'] - before['host'] == 3 * n_png
    assert det.blur_counts['gpu'] - before['gpu'] == 3 * (blurred - n_png) + int(one['blurred'] is not None)
    # only the categories and confidences asked for
    none = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, blur=B.BlurOptions(confidence_threshold=1.1))
    assert all(r['blurred'] is None for r in none) and strip(none, 'blurred') == plain
    assert 'blurred' not in plain[0]
