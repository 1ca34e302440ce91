"""
Privacy blurring, host side: the host model of the GPU blur (mdjpeg_blur_regions in libmdjpeg.so, compiled from
csrc/blur_box.h like the kernels) against Pillow's ImageFilter.GaussianBlur, bit for bit; the rectangles and the selection
of megadetector_amd.blur against the reference's statements; the written file against Image.save(quality=85); the driver's
options.  The rectangle matrix and the Pillow pipeline defined here are what tests/test_gpu_blur.py runs on the device.
"""

import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFilter

from megadetector_amd import blur as B
from megadetector_amd import jpeg_host as J

SIZES = [(1, 1), (1, 7), (5, 3), (37, 90), (200, 131), (81, 79), (82, 80), (300, 17)]          # w x h
RADII = [40, 2, 1, 7.5, 100]
IMG_W, IMG_H, PITCH = 97, 131, 393              # the image of the rectangle matrix; its pitch is 3 * 131


def content(w, h, seed):
    """noise; the larger sizes are half white, so that a blur has an edge to smear"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if w * h >= 1000:
        a[:, w // 2:] = 255
    return a


def pillow_blur_regions(rgb, rects, radius):
    """visualization_utils.blur_detections' crop / GaussianBlur / paste for pixel rectangles, in list order"""
    im = Image.fromarray(rgb)
    for left, top, right, bottom in rects:
        region = im.crop((left, top, right, bottom))
        im.paste(region.filter(ImageFilter.GaussianBlur(radius=radius)), (left, top))
    return np.asarray(im)


def reference_blur_detections(image, detections, blur_radius=40):
    """visualization_utils.py:497-531, statement for statement"""
    img_width, img_height = image.size
    for d in detections:
        x_norm, y_norm, width_norm, height_norm = d['bbox']
        x = int(x_norm * img_width)
        y = int(y_norm * img_height)
        width = int(width_norm * img_width)
        height = int(height_norm * img_height)
        left = max(0, x)
        top = max(0, y)
        right = min(img_width, x + width)
        bottom = min(img_height, y + height)
        region = image.crop((left, top, right, bottom))
        image.paste(region.filter(ImageFilter.GaussianBlur(radius=blur_radius)), (left, top))


def reference_blurred_file(rgb, name, detections, options):
    """what the reference writes for an image: the detections it would blur (separate_detections_into_folders.py:444-451, in
    the order of the results file), blur_detections, save(quality) in the format of the name; None without such a detection"""
    ids = options.category_ids()
    chosen = [d for d in B.output_order(detections, options.output_threshold)
              if d['conf'] >= options.confidence_threshold and d['category'] in ids]
    if not chosen:
        return None
    im = Image.fromarray(rgb)
    before = im.copy()
    reference_blur_detections(im, chosen, options.radius)
    if im.tobytes() == before.tobytes() and not B.rectangles_to_blur(detections, rgb.shape[1], rgb.shape[0], options, ids):
        return None                                  # only boxes without pixels: this project writes no copy (stated in blur.py)
    bio = io.BytesIO()
    im.save(bio, format=Image.registered_extensions()[os.path.splitext(name)[1].lower()], quality=options.quality)
    return bio.getvalue()


def rectangle_matrix():
    """(left, top, right, bottom) inside the 97 x 131 image: the whole image, 1 x 1, one row, one column, rectangles on
    every border, and the widths and heights around the box radius 39 of radius 40 (n <= r, r + 1, 2 r + 1, 2 r + 2)"""
    W, H = IMG_W, IMG_H
    rects = [(0, 0, W, H), (50, 60, 51, 61), (0, 70, W, 71), (33, 0, 34, H), (3, 9, 96, 10), (90, 2, 91, 130),
             (0, 0, 30, 20), (W - 30, 0, W, 25), (0, H - 20, 41, H), (W - 17, H - 33, W, H), (0, 40, 9, 90), (88, 40, W, 90),
             (10, 0, 60, 12), (10, H - 12, 60, H)]
    for i, n in enumerate([5, 39, 40, 41, 79, 80, 81]):
        rects.append((i + 1, 2 * i + 3, i + 1 + n, 2 * i + 3 + 47))                  # width n
        rects.append((2 * i + 3, i + 1, 2 * i + 3 + 23, i + 1 + n))                  # height n
        rects.append((i, i + 2, i + n, i + 2 + n))                                   # both
    assert all(0 <= l < r <= W and 0 <= t < b <= H for l, t, r, b in rects)
    return rects


def strided_image(seed=5, fill=0xA5):
    """the 97 x 131 image as a view with pitch 393 of a larger array filled with a sentinel: (backing array, view)"""
    backing = np.full((IMG_H + 6, PITCH), fill, dtype=np.uint8)
    view = backing[3:3 + IMG_H, 60:60 + IMG_W * 3].reshape(IMG_H, IMG_W, 3)
    view[...] = content(IMG_W, IMG_H, seed)
    assert view.base is not None and view.strides == (PITCH, 3, 1)
    return backing, view


def test_the_box_radius_and_weights_of_radius_40():
    r, ww, fw = J.blur_weights(40)
    assert (r, ww, fw) == (39, 209747, 103601)
    assert (2 * r + 1) * ww + 2 * fw in (1 << 24, (1 << 24) - 1)
    assert J.blur_weights(0) == (0, 1 << 24, 0)
    with pytest.raises(ValueError):
        J.blur_weights(-1)
    with pytest.raises(ValueError):
        J.blur_weights(float('nan'))
    with pytest.raises(ValueError):
        J.blur_weights(513)


@pytest.mark.parametrize('radius', RADII)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '{}x{}'.format(*s))
def test_host_model_equals_pillow(size, radius):
    w, h = size
    rgb = content(w, h, seed=w * 1000 + h)
    want = np.asarray(Image.fromarray(rgb).filter(ImageFilter.GaussianBlur(radius)))
    got = rgb.copy()
    assert J.blur_regions(got, [(0, 0, w, h)], radius) == J.MDJPEG_OK
    np.testing.assert_array_equal(got, want)
    # and in the chunks of a device with very little on-chip memory: rows cut in pieces with their halo
    for lds in (49152, 6000, 2 * (3 * 6 * (J.blur_weights(radius)[0] + 1) + 3 * 4 + 8)):
        got = rgb.copy()
        assert J.blur_regions(got, [(0, 0, w, h)], radius, lds_bytes=lds) == J.MDJPEG_OK
        np.testing.assert_array_equal(got, want, err_msg='lds_bytes {}'.format(lds))


@pytest.mark.parametrize('radius', [40, 2, 7.5, 100])
def test_rectangles_inside_an_image_with_pitch_393(radius):
    for k, rect in enumerate(rectangle_matrix()):
        backing, view = strided_image()
        source = view.copy()
        want = pillow_blur_regions(source, [rect], radius)
        assert J.blur_regions(view, [rect], radius) == J.MDJPEG_OK
        np.testing.assert_array_equal(view, want, err_msg='rectangle {} {}'.format(k, rect))
        l, t, r, b = rect
        outside = np.ones((IMG_H, IMG_W), bool)
        outside[t:b, l:r] = False
        assert (view[outside] == source[outside]).all()
        check = backing.copy()
        check[3:3 + IMG_H, 60:60 + IMG_W * 3] = 0xA5
        assert (check == 0xA5).all(), 'bytes beside the image were written'


def test_overlapping_rectangles_interact_and_their_order_matters():
    a, b = (10, 20, 70, 100), (40, 60, 95, 125)
    results = []
    for order in ([a, b], [b, a]):
        _, view = strided_image(seed=9)
        want = pillow_blur_regions(view.copy(), order, 40)
        assert J.blur_regions(view, order, 40) == J.MDJPEG_OK
        np.testing.assert_array_equal(view, want)
        results.append(view.copy())
    assert not np.array_equal(results[0], results[1])


def test_rectangles_without_area_are_skipped_as_pillow_pastes_nothing():
    im = Image.fromarray(content(20, 20, 1))
    before = im.tobytes()
    empty = im.crop((5, 5, 5, 9))
    assert empty.size == (0, 4)
    im.paste(empty.filter(ImageFilter.GaussianBlur(40)), (5, 5))                 # what blur_detections does with it
    assert im.tobytes() == before
    with pytest.raises(ValueError):
        im.crop((7, 5, 5, 9))                                                    # right < left: the reference stops here
    rgb = content(20, 20, 1)
    got = rgb.copy()
    assert J.blur_regions(got, [(5, 5, 5, 9), (7, 5, 5, 9), (3, 9, 8, 9), (0, 0, 0, 0)], 40) == J.MDJPEG_OK
    np.testing.assert_array_equal(got, rgb)
    # a rectangle WITH area that leaves the image is an error, and nothing is changed
    assert J.blur_regions(got, [(0, 0, 5, 5), (10, 10, 21, 12)], 40) == J.MDJPEG_EINVAL
    assert J.blur_regions(got, [(-1, 0, 5, 5)], 40) == J.MDJPEG_EINVAL
    np.testing.assert_array_equal(got, rgb)


BOXES = [[0.1, 0.2, 0.3, 0.4], [0.0, 0.0, 1.0, 1.0], [-0.2, -0.1, 0.5, 0.5], [0.8, 0.7, 0.5, 0.6], [0.3337, 0.2519, 0.1234, 0.4321],
         [0.999, 0.999, 0.2, 0.2], [0.5, 0.5, 0.0, 0.3], [0.5, 0.5, 0.004, 0.3], [0.2, 0.3, 0.3, 0.0], [-0.5, 0.1, 0.4, 0.4],
         [1.2, 0.1, 0.2, 0.2], [0.1, 1.5, 0.2, 0.2], [0.1, 0.1, -0.2, 0.2], [-0.004, -0.004, 0.5, 0.5]]


@pytest.mark.parametrize('size', [(97, 131), (640, 480), (2048, 1536), (1, 1)], ids=lambda s: '{}x{}'.format(*s))
def test_blur_rectangle_restates_blur_detections(size):
    W, H = size
    for bbox in BOXES:
        x, y, w, h = int(bbox[0] * W), int(bbox[1] * H), int(bbox[2] * W), int(bbox[3] * H)
        want = (max(0, x), max(0, y), min(W, x + w), min(H, y + h))
        got = B.blur_rectangle(bbox, W, H)
        if want[2] <= want[0] or want[3] <= want[1]:
            assert got is None, (bbox, want)
        else:
            assert got == want and 0 <= got[0] < got[2] <= W and 0 <= got[1] < got[3] <= H
    assert B.blur_rectangle([0.5, 0.5, 0.0, 0.3], 640, 480) is None and B.blur_rectangle([1.2, 0.1, 0.2, 0.2], 640, 480) is None
    # the whole pipeline on pixels, boxes past the border and without pixels included (the ones Image.crop refuses left out)
    if W * H > 1 and W <= 640:
        rgb = content(W, H, 3)
        dets = [{'category': '2', 'conf': 0.9 - 0.01 * i, 'bbox': b} for i, b in enumerate(BOXES)
                if b not in ([1.2, 0.1, 0.2, 0.2], [0.1, 1.5, 0.2, 0.2], [0.1, 0.1, -0.2, 0.2], [-0.5, 0.1, 0.4, 0.4])]
        im = Image.fromarray(rgb)
        reference_blur_detections(im, dets, 40)
        got = rgb.copy()
        opt = B.BlurOptions()
        assert J.blur_regions(got, B.rectangles_to_blur(dets, W, H, opt, opt.category_ids()), 40) == J.MDJPEG_OK
        np.testing.assert_array_equal(got, np.asarray(im))


def test_selection_by_category_and_threshold():
    dets = [{'category': '1', 'conf': 0.9, 'bbox': [0.1, 0.1, 0.2, 0.2]}, {'category': '2', 'conf': 0.19, 'bbox': [0.1, 0.1, 0.2, 0.2]},
            {'category': '2', 'conf': 0.2, 'bbox': [0.3, 0.1, 0.2, 0.2]}, {'category': '3', 'conf': 0.8, 'bbox': [0.1, 0.1, 0.2, 0.2]},
            {'category': '2', 'conf': 0.95, 'bbox': [0.5, 0.5, 0.2, 0.2]}]
    opt = B.BlurOptions()
    assert opt.category_names == ('person',) and opt.confidence_threshold == 0.2 and opt.radius == 40 and opt.quality == 85
    assert opt.category_ids() == {'2'}
    assert B.select_detections(dets, opt, opt.category_ids()) == [dets[4], dets[2]]          # the order of the results file
    both = B.BlurOptions(category_names='person, vehicle', confidence_threshold=0.5)
    assert both.category_ids() == {'2', '3'} and B.select_detections(dets, both, both.category_ids()) == [dets[4], dets[3]]
    cut = B.BlurOptions(confidence_threshold=0.0, output_threshold=0.5)
    assert B.select_detections(dets, cut, cut.category_ids()) == [dets[4]]
    assert B.select_detections([], opt, {'2'}) == [] and B.select_detections(None, opt, {'2'}) == []
    with pytest.raises(ValueError):
        B.BlurOptions(category_names=['cat']).category_ids()
    with pytest.raises(ValueError):
        B.BlurOptions(radius=-1)
    with pytest.raises(ValueError):
        B.BlurOptions(quality=0)


@pytest.mark.parametrize('name', ['a.jpg', 'sub/b.JPEG', 'c.png'])
def test_the_host_leg_writes_the_file_pillow_saves(name):
    rgb = content(320, 240, 7)
    dets = [{'category': '2', 'conf': 0.9, 'bbox': [0.1, 0.2, 0.4, 0.6]}, {'category': '1', 'conf': 0.9, 'bbox': [0.0, 0.0, 0.3, 0.3]},
            {'category': '2', 'conf': 0.5, 'bbox': [0.3, 0.3, 0.5, 0.9]}, {'category': '2', 'conf': 0.1, 'bbox': [0.6, 0.0, 0.2, 0.2]}]
    opt = B.BlurOptions()
    source = rgb.copy()
    got = B.blurred_file_of_host_image(rgb, name, dets, opt, opt.category_ids())
    np.testing.assert_array_equal(rgb, source)                                   # the caller's pixels are not touched
    im = Image.fromarray(source)
    reference_blur_detections(im, [dets[0], dets[2]], 40)
    bio = io.BytesIO()
    im.save(bio, format='PNG' if name.endswith('.png') else 'JPEG', quality=85)
    assert got == bio.getvalue() == reference_blurred_file(source, name, dets, opt)
    assert not np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert('RGB')), source)
    assert B.blurred_file_of_host_image(rgb, name, dets[1:2] + dets[3:], opt, opt.category_ids()) is None
    assert B.blurred_file_of_host_image(rgb, name, [{'category': '2', 'conf': 0.9, 'bbox': [0.5, 0.5, 0.0, 0.2]}], opt, opt.category_ids()) is None


def test_the_driver_writes_only_images_with_something_to_blur(tmp_path):
    """run_detector_batch's loop with the stub detector (no blur= of its own): the host leg, below the blur folder"""
    from megadetector_amd import run_detector_batch as RDB

    class TableDetector:
        """the 3-method duck type of the host path with detections from a table, and no blur= of its own"""
        default_image_size, letterbox_stride = 1280, 64

        def __init__(self, table):
            self.table = table

        def generate_detections_one_image(self, img, name='unknown', detection_threshold=1e-5, image_size=None, augment=False, verbose=False):
            dets = [dict(d) for d in self.table[name] if d['conf'] >= detection_threshold]
            return {'file': name, 'detections': dets, 'max_detection_conf': max([d['conf'] for d in dets] or [0.0])}

        def generate_detections_one_batch(self, imgs, names, detection_threshold=1e-5, image_size=None, augment=False, verbose=False):
            return [self.generate_detections_one_image(i, n, detection_threshold) for i, n in zip(imgs, names)]

    folder = tmp_path / 'images'
    (folder / 'sub').mkdir(parents=True)
    files = []
    for i, rel in enumerate(['a.jpg', 'sub/b.jpg', 'c.png', 'sub/d.jpg']):
        p = folder / rel
        Image.fromarray(content(160 + 8 * i, 120, 20 + i)).save(str(p), quality=92)
        files.append(str(p))
    person = lambda conf: {'category': '2', 'conf': conf, 'bbox': [0.2, 0.1, 0.5, 0.7]}
    table = {files[0]: [person(0.9), {'category': '1', 'conf': 0.8, 'bbox': [0.0, 0.0, 0.5, 0.5]}], files[1]: [person(0.15)],
             files[2]: [person(0.6), person(0.3)], files[3]: [{'category': '1', 'conf': 0.99, 'bbox': [0.1, 0.1, 0.5, 0.5]}]}
    det = TableDetector(table)
    for k, kw in enumerate([{}, {'batch_size': 2}, {'use_image_queue': True, 'batch_size': 2}]):
        out = tmp_path / 'blur{}'.format(k)
        plain = RDB.load_and_run_detector_batch('stub', files, quiet=True, detector=det, **kw)
        res = RDB.load_and_run_detector_batch('stub', files, quiet=True, detector=det, blur_folder=str(out), blur_base=str(folder), **kw)
        by_file = lambda rs: sorted(rs, key=lambda r: r['file'])          # (the image queue hands results on as they come)
        assert by_file(res) == by_file(plain) and all('blurred' not in r for r in res)
        written = sorted(os.path.relpath(os.path.join(d, f), str(out)).replace('\\', '/') for d, _, fs in os.walk(str(out)) for f in fs)
        assert written == ['a.jpg', 'c.png'], written
        assert RDB.last_blur_counts == {'files': 2, 'gpu': 0, 'host': 2}
        opt = B.BlurOptions()
        for rel in written:
            src = os.path.join(str(folder), rel)
            want = reference_blurred_file(np.asarray(RDB.load_image(src)), rel, table[src], opt)
            assert open(os.path.join(str(out), rel), 'rb').read() == want


def test_the_cli_refuses_blur_options_without_a_blur_folder(tmp_path):
    from megadetector_amd import run_detector_batch as RDB
    out = str(tmp_path / 'o.json')
    for extra in (['--blur_categories', 'person'], ['--blur_confidence_threshold', '0.3'], ['--blur_radius', '20'], ['--blur_quality', '90']):
        with pytest.raises(AssertionError, match='--blur_folder'):
            RDB.main(['synthetic:YOLOV5N6_TEST:1', str(tmp_path), out] + extra)
    assert not os.path.exists(out)
