"""
Annotated previews on the device: mdhip_resample_lanczos (HipContext.resample_lanczos) against Pillow's
Image.resize(LANCZOS), bit for bit and with nothing written beside the destinations' rows; mdhip_draw_ops
(HipContext.draw_ops) against its host model, byte for byte; HIPDetector(preview=) against the host leg on the same pixels
and detections.  The shapes, scenes and the restated renderer are those of test_preview_cpu.py.  At the end crops=, blur= and
preview= in one call against each alone, and already letterboxed inputs, where the products read different pixels.
"""

import numpy as np
import pytest
import torch

from megadetector_amd import jpeg_host as J
from megadetector_amd import preview as P
from megadetector_amd._lib import HipError
from test_preview_cpu import DRAW_CASES, EQUAL, LABEL_MAP, SCENE, SCENE_SIZE, noise, pillow_resize
from test_gpu_tile_jpeg import _ctx

pytestmark = pytest.mark.gpu

GUARD = 0xA5
LEAD = 37                               # bytes in front of an image in its allocation: an odd address


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to('cuda:0')
    torch.cuda.synchronize()
    return t


def _pitched(rgb, pitch):
    """rgb with `pitch` bytes a row inside an allocation filled with GUARD, LEAD bytes in front and 64 behind: the host copy"""
    h, w = rgb.shape[:2]
    buf = np.full(LEAD + pitch * h + 64, GUARD, np.uint8)
    for y in range(h):
        buf[LEAD + y * pitch:LEAD + y * pitch + w * 3] = rgb[y].reshape(-1)
    return buf


def _resample_and_check(ctx, cases):
    """cases: [(source array, source pitch, (dw, dh), destination pitch)] in ONE call; every destination is Pillow's and every
    other byte of its allocation -- in front, behind, in the pitch padding -- is what it was; the sources are unchanged"""
    srcs = [_device(_pitched(a, sp)) for a, sp, _, _ in cases]
    dsts = [_device(_pitched(np.full((dh, dw, 3), GUARD, np.uint8), dp)) for _, _, (dw, dh), dp in cases]
    ctx.resample_lanczos([t.data_ptr() + LEAD for t in srcs], [(a.shape[1], a.shape[0]) for a, _, _, _ in cases], [sp for _, sp, _, _ in cases],
                         [t.data_ptr() + LEAD for t in dsts], [size for _, _, size, _ in cases], [dp for _, _, _, dp in cases])
    torch.cuda.synchronize()
    for (a, sp, (dw, dh), dp), s, d in zip(cases, srcs, dsts):
        want = _pitched(pillow_resize(a, (dw, dh)), dp)
        got = d.cpu().numpy()
        assert int((got != want).sum()) == 0, '{}x{} -> {}x{}: {} bytes differ'.format(a.shape[1], a.shape[0], dw, dh, int((got != want).sum()))
        np.testing.assert_array_equal(s.cpu().numpy(), _pitched(a, sp))


def test_one_batched_call_equals_pillow_and_writes_nothing_else():
    """reducing, enlarging, odd sizes, a source pitch of 64 for 17 pixels; destination pitches with 0, 1 and 7 bytes of padding"""
    _resample_and_check(_ctx(), [(noise(97, 61, 1), 97 * 3, (40, 25), 40 * 3 + 1), (noise(50, 40, 2), 50 * 3, (120, 96), 120 * 3),
                                 (noise(333, 500, 3), 333 * 3 + 5, (166, 249), 166 * 3 + 7), (noise(17, 9, 4), 64, (8, 4), 8 * 3)])


def test_a_long_tap_run_in_more_than_one_strip_and_an_unchanged_axis():
    """1300 x 40 -> 100 x 3: 79 taps a pixel, two strips of 64 output pixels; 640 x 48 -> 640 x 47 and 64 x 48 -> 63 x 48 take one
    pass only; 31 x 20 -> 31 x 20 is a copy"""
    _resample_and_check(_ctx(), [(noise(1300, 40, 5), 1300 * 3, (100, 3), 100 * 3), (noise(640, 48, 6), 640 * 3, (640, 47), 640 * 3 + 2),
                                 (noise(64, 48, 7), 64 * 3 + 3, (63, 48), 63 * 3), (noise(31, 20, 8), 31 * 3, (31, 20), 31 * 3 + 1),
                                 (np.full((61, 97, 3), 255, np.uint8), 97 * 3, (40, 25), 40 * 3)])


def _planned(dets, size, opt, labels=True):
    return P.render_plan(dets, size[0], size[1], opt, LABEL_MAP, labels)


def test_the_six_box_scene_and_a_two_image_batch_equal_the_host_model():
    ctx = _ctx()
    W, H = SCENE_SIZE
    plans = [(noise(W, H, 21), _planned(SCENE, SCENE_SIZE, P.PreviewOptions())),
             (noise(301, 177, 22), _planned(EQUAL, (301, 177), P.PreviewOptions(box_expansion=10))),
             (noise(64, 48, 23), _planned(DRAW_CASES['outside'][0], (64, 48), P.PreviewOptions(box_thickness=2), labels=False))]
    assert len({len(p.ops) for _, p in plans}) == 3
    # one patch buffer for the call; the images' operations interleaved, so that the order within an image is the list's
    packed, op_image, ops = bytearray(), [], []
    for k, (_, plan) in enumerate(plans):
        base = len(packed)
        packed += plan.patches
        for op in plan.ops:
            op_image.append(k)
            ops.append(op[:5] + [op[5] + base] + op[6:] if op[0] == P.OP_PATCH else op)
    by_image = {k: [i for i in range(len(ops)) if op_image[i] == k] for k in range(3)}
    interleaved = [i for j in range(max(map(len, by_image.values()))) for k in range(3) for i in by_image[k][j:j + 1]]
    assert [i for i in interleaved if op_image[i] == 0] == by_image[0] and interleaved != sorted(interleaved)
    devs = [_device(_pitched(a, a.shape[1] * 3 + 2 * k)) for k, (a, _) in enumerate(plans)]
    patches = _device(np.frombuffer(bytes(packed), np.uint8).copy())
    ctx.draw_ops([t.data_ptr() + LEAD for t in devs], [(a.shape[1], a.shape[0]) for a, _ in plans],
                 [a.shape[1] * 3 + 2 * k for k, (a, _) in enumerate(plans)], [op_image[i] for i in interleaved], [ops[i] for i in interleaved],
                 patches.data_ptr(), len(packed))
    torch.cuda.synchronize()
    for k, ((a, plan), d) in enumerate(zip(plans, devs)):
        want = a.copy()
        assert J.draw_ops(want, plan.ops, bytes(plan.patches)) == J.MDJPEG_OK
        assert not np.array_equal(want, a)
        np.testing.assert_array_equal(d.cpu().numpy(), _pitched(want, a.shape[1] * 3 + 2 * k), err_msg='image {}'.format(k))


def test_bad_operations_are_refused_and_nothing_is_changed():
    ctx = _ctx()
    rgb = noise(64, 48, 24)
    d = _device(rgb)
    patches = _device(np.arange(36, dtype=np.uint8))
    args = ([d.data_ptr()], [(64, 48)], [192])
    rect = [0, 2, 2, 20, 20, 0x0000FF, 0, 0]
    with pytest.raises(HipError, match='image 1 of 1'):
        ctx.draw_ops(*args, [0, 1], [rect, rect], patches.data_ptr(), 36)
    with pytest.raises(HipError, match='image -1 of 1'):
        ctx.draw_ops(*args, [-1], [rect], patches.data_ptr(), 36)
    with pytest.raises(HipError, match='operation 1'):
        ctx.draw_ops(*args, [0, 0], [rect, [1, 0, 0, 4, 3, 1, 0, 0]], patches.data_ptr(), 36)     # a patch one byte past its buffer
    with pytest.raises(HipError, match='operation 0'):
        ctx.draw_ops(*args, [0], [[2, 0, 0, 4, 3, 0, 0, 0]], patches.data_ptr(), 36)
    with pytest.raises(HipError, match='host pointer'):
        ctx.draw_ops([rgb.ctypes.data], [(64, 48)], [192], [0], [rect])
    with pytest.raises(HipError, match='pitch'):
        ctx.draw_ops([d.data_ptr()], [(64, 48)], [191], [0], [rect])
    with pytest.raises(HipError, match='pitch'):
        ctx.resample_lanczos([d.data_ptr()], [(64, 48)], [191], [d.data_ptr()], [(32, 24)], [96])
    ctx.draw_ops(*args, [0, 0], [[0, 100, 100, 200, 200, 1, 0, 0], [0, 10, 10, 9, 9, 1, 0, 0]])          # nothing of them lies in the image
    ctx.draw_ops(*args, [], [])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy().reshape(rgb.shape), rgb)


def _known_detections():
    return [[{'category': '1', 'conf': 0.93, 'bbox': [0.1, 0.3, 0.2, 0.25]}, {'category': '2', 'conf': 0.5, 'bbox': [0.5, 0.01, 0.2, 0.3]},
             {'category': '2', 'conf': 0.31, 'bbox': [0.15, 0.35, 0.3, 0.3]}, {'category': '1', 'conf': 0.1, 'bbox': [0.4, 0.4, 0.1, 0.1]}],
            [{'category': '2', 'conf': 0.6, 'bbox': [0.2, 0.2, 0.5, 0.6]}, {'category': '3', 'conf': 0.6, 'bbox': [-0.1, 0.1, 0.5, 1.2]}],
            [],
            [{'category': '1', 'conf': 0.9, 'bbox': [0.4, 0.4, 0.004, 0.004]}, {'category': '2', 'conf': 0.8, 'bbox': [0.1, 0.1, 0.6, 0.6]}],
            [{'category': '2', 'conf': 0.7, 'bbox': [0.3, 0.2, 0.4, 0.5]}]]


@pytest.mark.parametrize('blur', [None, 'person'])
def test_device_previews_equal_the_host_leg_and_leave_the_sources_alone(blur):
    """known detections on device images: resized and not, a .png name, an image without boxes, one whose thin box sends it to
    the host leg, a resize target that is not positive"""
    ctx = _ctx()
    images = [noise(400, 300, 31), noise(333, 257, 32), noise(320, 240, 33), noise(301, 199, 34), noise(260, 200, 35), noise(4000, 2, 36)]
    names = ['a.jpg', 'd/b.jpeg', 'c.JPG', 'thin.jpg', 'e.png', 'flat.jpg']
    dets = _known_detections() + [[]]
    for width in (200, -1):
        opt = P.PreviewOptions(output_image_width=width, blur_categories=blur)
        tensors = [_device(a) for a in images]
        entries = [(t, a.shape[1], a.shape[0], n, d) for t, a, n, d in zip(tensors, images, names, dets)]
        out, counts = P.previews_of_device_images(ctx, entries, opt, LABEL_MAP)
        torch.cuda.synchronize()
        for t, a in zip(tensors, images):
            np.testing.assert_array_equal(t.cpu().numpy().reshape(a.shape), a)
        want = [P.preview_file_of_host_image(a, n, d, opt, LABEL_MAP) for a, n, d in zip(images, names, dets)]
        assert [data for data, _ in out] == want
        flat_leg = 'skipped' if width == 200 else 'gpu'
        assert [leg for _, leg in out] == ['gpu', 'gpu', 'gpu', 'host', 'host', flat_leg]
        assert want[5] is None if width == 200 else want[5] is not None
        assert counts == {'gpu': 3 + (flat_leg == 'gpu'), 'host': 2, 'skipped': int(flat_leg == 'skipped')}


def _yolo_detector(batch):
    from test_gpu_blur import _yolo_detector as make
    return make(batch)


def _threshold_for(results, size_of, width):
    """a confidence threshold, taken from the detections themselves, at which up to 12 boxes are drawn and no image is handed
    to the host leg by a thin box: the k-th highest confidence for the largest such k"""
    confs = sorted((d['conf'] for r in results for d in r['detections']), reverse=True)
    for k in range(min(12, len(confs)), 0, -1):
        opt = P.PreviewOptions(confidence_threshold=min(confs[k - 1], 1.0), output_image_width=width)
        try:
            for r in results:
                P.render_plan(r['detections'], *P.target_size(*size_of[r['file']], width), opt)
        except P.HostLeg:
            continue
        return opt.confidence_threshold, k
    raise AssertionError('every choice of boxes holds one the plan hands to the host leg: {}'.format(confs[:12]))


@pytest.mark.parametrize('blur', [None, 'animal,person,vehicle'])
def test_detector_preview_synchronous_and_pipelined_equal_the_host_leg(blur):
    from test_gpu_tile_jpeg import _image
    det = _yolo_detector(4)
    imgs = [np.ascontiguousarray(_image()[y:y + h, x:x + w]) for x, y, w, h in
            [(0, 0, 400, 300), (1500, 100, 333, 257), (100, 400, 320, 240), (900, 900, 301, 199)]]
    names = ['a.jpg', 'd/b.jpeg', 'e.png', 'g.jpg']
    sources = [a.copy() for a in imgs]
    plain = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5)
    assert all(r.get('failure') is None for r in plain) and 'preview' not in plain[0]
    size_of = {n: (a.shape[1], a.shape[0]) for n, a in zip(names, imgs)}
    threshold, k = _threshold_for(plain, size_of, 200)
    print('threshold {} draws {} boxes'.format(threshold, k))
    opt = P.PreviewOptions(confidence_threshold=threshold, output_image_width=200, blur_categories=blur)
    before = dict(det.preview_counts)
    sync = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, preview=opt)
    tickets = [det.start_batch(imgs[:3], names[:3], detection_threshold=1e-5, preview=opt),
               det.start_batch(imgs[3:], names[3:], detection_threshold=1e-5, preview=opt)]
    piped = det.finish_batch(tickets[0]) + det.finish_batch(tickets[1])
    one = det.generate_detections_one_image(imgs[1], names[1], detection_threshold=1e-5, preview=opt)
    strip = lambda res: [{k: v for k, v in r.items() if k != 'preview'} for r in res]
    assert strip(sync) == plain and sync == piped and one == sync[1]
    assert all(np.array_equal(a, b) for a, b in zip(imgs, sources))
    for r, img in zip(sync, imgs):
        want = P.preview_file_of_host_image(img, r['file'], r['detections'], opt)
        data, leg = r['preview']
        print(r['file'], len(r['detections']), 'detections;', len(want), 'bytes;', leg)
        assert data == want and leg == ('host' if r['file'].endswith('.png') else 'gpu')
    assert det.preview_counts['gpu'] - before['gpu'] == 2 * 3 + 1                  # the JPEG names of two batches and the single image
    assert det.preview_counts['host'] - before['host'] == 2 and det.preview_counts['skipped'] == before['skipped']
    # below the threshold with detections_only: no file; crops= and blur= beside preview= change nothing
    none = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5,
                                             preview=P.PreviewOptions(confidence_threshold=1.0, detections_only=True))
    assert all(r['preview'] == (None, 'skipped') for r in none) and strip(none) == plain
    from megadetector_amd import blur as B
    both = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, preview=opt, blur=B.BlurOptions(confidence_threshold=1.1))
    assert [r['preview'] for r in both] == [r['preview'] for r in sync]


# ---- crops=, blur= and preview= in one call -------------------------------------------------------------------------------

def _all_products():
    from megadetector_amd import blur as B, crops as K
    return dict(crops=K.CropOptions(confidence_threshold=0.0),
                blur=B.BlurOptions(category_names=('animal', 'person', 'vehicle'), confidence_threshold=0.0),
                preview=P.PreviewOptions(confidence_threshold=0.0, output_image_width=160))


def _threshold_with_every_product(results, size_of, products):
    """a detection threshold, taken from the detections themselves (the k-th highest confidence for the largest k up to 12), at
    which there is a crop and a rectangle to blur with area and at least one JPEG name whose preview the plan restates, so that
    it is made on the device.  Every product's own threshold is 0.0: what the detector returns is what they see"""
    from megadetector_amd import blur as B, crops as K
    confs = sorted((d['conf'] for r in results for d in r['detections']), reverse=True)
    for k in range(min(12, len(confs)), 0, -1):
        kept = {r['file']: [d for d in r['detections'] if d['conf'] >= confs[k - 1]] for r in results}
        on_device = 0
        for name, dets in kept.items():
            try:
                P.render_plan(dets, *P.target_size(*size_of[name], products['preview'].output_image_width), products['preview'])
                on_device += K.is_jpeg_name(name)
            except (P.HostLeg, P.RenderFailure):
                pass
        boxes = [(d['bbox'],) + size_of[name] for name, dets in kept.items() for d in dets]
        if on_device and any(K.crop_rectangle(*b) for b in boxes) and any(B.blur_rectangle(*b) for b in boxes):
            return confs[k - 1], k
    raise AssertionError('no choice of boxes gives every product: {}'.format(confs[:12]))


_PRODUCT_KEYS = ('crops', 'blurred', 'preview')
_COUNTS = ('crop_counts', 'blur_counts', 'preview_counts')


def _without_products(results):
    return [{k: v for k, v in r.items() if k not in _PRODUCT_KEYS} for r in results]


def _counts(det):
    return {name: dict(getattr(det, name)) for name in _COUNTS}


def _increase(det, before):
    return {name: {k: v - before[name][k] for k, v in getattr(det, name).items()} for name in _COUNTS}


def test_crops_blur_and_preview_together_equal_each_alone_synchronous_and_pipelined():
    """two tickets outstanding, the second with two shape groups, and once more so that staging buffers handed out while
    products were owed are themselves reused (as test_two_tickets_outstanding_and_the_second_holds_three_shape_groups)"""
    from test_gpu_tile_jpeg import _image
    det = _yolo_detector(4)
    cuts = [(0, 0, 400, 300), (1500, 100, 333, 257), (100, 400, 640, 480), (500, 0, 300, 400), (0, 1100, 600, 400), (900, 900, 301, 199)]
    imgs = [np.ascontiguousarray(_image()[y:y + h, x:x + w]) for x, y, w, h in cuts]
    names = ['a.jpg', 'd/b.jpeg', 'c.JPG', 'e.png', 'f.jpg', 'g.jpg']
    sources = [a.copy() for a in imgs]
    shape = lambda a: tuple(det.preprocess_image(a)['img_processed'].shape)
    assert len({shape(a) for a in imgs[:3]}) == 1 and len({shape(a) for a in imgs[3:]}) == 2
    products = _all_products()
    size_of = {n: (a.shape[1], a.shape[0]) for n, a in zip(names, imgs)}
    threshold, k = _threshold_with_every_product(det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5), size_of, products)
    print('detection threshold {} keeps {} boxes'.format(threshold, k))
    plain = det.generate_detections_one_batch(imgs, names, detection_threshold=threshold)
    assert all(r.get('failure') is None for r in plain) and not any(key in r for r in plain for key in _PRODUCT_KEYS)
    alone = {}
    for (kw, options), key in zip(products.items(), _PRODUCT_KEYS):
        res = det.generate_detections_one_batch(imgs, names, detection_threshold=threshold, **{kw: options})
        assert _without_products(res) == plain and all(set(r) - set(p) == {key} for r, p in zip(res, plain))
        alone[key] = [r[key] for r in res]

    def check(results):
        assert _without_products(results) == plain
        for key in _PRODUCT_KEYS:
            assert [r[key] for r in results] == alone[key], key

    before = _counts(det)
    check(det.generate_detections_one_batch(imgs, names, detection_threshold=threshold, **products))
    synchronous = _increase(det, before)
    for _ in range(2):
        before = _counts(det)
        tickets = [det.start_batch(imgs[:3], names[:3], detection_threshold=threshold, **products),
                   det.start_batch(imgs[3:], names[3:], detection_threshold=threshold, **products)]
        check(det.finish_batch(tickets[0]) + det.finish_batch(tickets[1]))
        assert _increase(det, before) == synchronous
    assert all(np.array_equal(a, b) for a, b in zip(imgs, sources))
    print('increase of the counts in one run:', synchronous)
    assert sum(len(c) for c in alone['crops']) >= 1 and sum(b is not None for b in alone['blurred']) >= 1
    assert sum(leg == 'gpu' for _, leg in alone['preview']) >= 1
    assert alone['preview'][3][1] in ('host', 'skipped')                              # the .png name: PIL saves it


def test_already_letterboxed_inputs_crops_read_the_letterbox_blur_and_preview_the_original():
    """the one branch where the products read different pixels: 'img_processed' is an array, so crops= cuts the letterboxed
    pixels on the device, while blur= and preview= go to their host legs with 'img_original'"""
    from megadetector_amd import blur as B
    from test_blur_cpu import reference_blurred_file
    from test_gpu_crop_encode import _host_crops
    from test_gpu_tile_jpeg import _image
    det = _yolo_detector(4)
    products = _all_products()
    batch = []
    for i, (name, (x, y, w, h)) in enumerate([('a.jpg', (0, 0, 400, 300)), ('d/b.jpg', (500, 0, 300, 400))]):
        info = det.preprocess_image(np.ascontiguousarray(_image()[y:y + h, x:x + w]), image_id=name)
        info['file'] = name
        hh, ww = info['img_processed'].shape[:2]
        info['img_processed'] = np.ascontiguousarray(_image()[700 + 40 * i:700 + 40 * i + hh, 1000:1000 + ww])
        assert info['img_processed'].shape == (hh, ww, 3) and info['img_processed'].dtype == np.uint8 and info['img_processed'].std() > 1
        batch.append(info)
    letterboxed = [info['img_processed'].copy() for info in batch]
    originals = [info['img_original'].copy() for info in batch]
    first = det.generate_detections_one_batch(batch, detection_threshold=1e-5)
    confs = sorted((d['conf'] for r in first for d in r['detections']), reverse=True)
    assert confs, 'the test has no detection'
    threshold = confs[min(8, len(confs)) - 1]
    plain = det.generate_detections_one_batch(batch, detection_threshold=threshold)
    before = _counts(det)
    got = det.generate_detections_one_batch(batch, detection_threshold=threshold, **products)
    assert _without_products(got) == plain and all(r.get('failure') is None for r in got)
    for r, info, lb, original in zip(got, batch, letterboxed, originals):
        assert np.array_equal(info['img_processed'], lb) and np.array_equal(info['img_original'], original)
        assert r['crops'] == _host_crops(lb, r['file'], r['detections'], products['crops'])
        assert r['blurred'] == reference_blurred_file(original, r['file'], r['detections'], products['blur'])
        data, leg = r['preview']
        assert leg == 'host' and data == P.preview_file_of_host_image(original, r['file'], r['detections'], products['preview'])
    n_crops, n_blurred = sum(len(r['crops']) for r in got), sum(r['blurred'] is not None for r in got)
    print('crops:', n_crops, 'blurred:', n_blurred)
    assert n_crops >= 1 and n_blurred >= 1
    assert _increase(det, before) == {'crop_counts': {'gpu': n_crops, 'host': 0, 'skipped': sum(len(r['detections']) for r in got) - n_crops},
                                      'blur_counts': {'gpu': 0, 'host': n_blurred}, 'preview_counts': {'gpu': 0, 'host': 2, 'skipped': 0}}
