"""
Classification in the same pass, on the device: mdhip_classifier_input against PIL and numpy bit for bit (the uint32 view of the
floats), its argument checks, and HIPDetector(classify=...) against the host leg.
"""

import numpy as np
import pytest
import torch

from megadetector_amd import classify as K
from megadetector_amd import jpeg_host as J
from megadetector_amd._lib import HipError
from test_classify_cpu import TinyClassifier, bits, noise
from test_gpu_preview import GUARD, LEAD, _device, _pitched
from test_gpu_tile_jpeg import _ctx

pytestmark = pytest.mark.gpu

_STATE = {}


def _images():
    """three images at odd addresses (LEAD bytes of lead) whose rows have 0, 1 and 5 bytes of padding: [(pixels, pitch, host
    copy of the allocation, device allocation)], made once and never changed"""
    if 'images' not in _STATE:
        out = []
        for k, (w, h, pad) in enumerate([(1310, 210, 0), (340, 510, 1), (650, 490, 5)]):
            a = noise(w, h, 40 + k)
            host = _pitched(a, w * 3 + pad)
            out.append((a, w * 3 + pad, host, _device(host)))
        _STATE['images'] = out
    return _STATE['images']


def _run_and_check(ctx, size, crops, interpolation='bicubic'):
    """crops: [(image, canvas)], canvas as classify.crop_canvas gives it.  ONE call for all of them; every value is the host
    leg's, every byte around the output tensor is what it was, and the sources are unchanged"""
    opt = K.ClassifyOptions(model=torch.nn.Identity(), image_size=size, interpolation=interpolation)
    images = _images()
    n = len(crops)
    lead = 64
    out = torch.full((lead + n * 3 * size * size * 4 + 64,), GUARD, dtype=torch.uint8, device='cuda:0')
    recs = []
    for m, (cw, ch, ox, oy, (x0, y0, x1, y1)) in crops:
        _, pitch, _, dev = images[m]
        recs.append((dev.data_ptr() + LEAD + y0 * pitch + x0 * 3, pitch, x1 - x0, y1 - y0, cw, ch, ox, oy))
    assert ctx.classifier_input(recs, size, out.data_ptr() + lead, opt.filter, opt.mean, opt.std)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[:lead] == GUARD).all() and (raw[-64:] == GUARD).all()
    got = raw[lead:-64].view(np.float32).reshape(n, 3, size, size)
    for i, (m, canvas) in enumerate(crops):
        want = K.classifier_input_host(images[m][0], canvas, opt)
        diff = int((bits(got[i]) != bits(want)).sum())
        assert diff == 0, 'crop {} ({} of image {}) at {}: {} values differ'.format(i, canvas, m, size, diff)
    for _, _, host, dev in images:
        np.testing.assert_array_equal(dev.cpu().numpy(), host)


def _plain(x, y, w, h):
    return w, h, 0, 0, (x, y, x + w, y + h)


# zeros on the left, right, top, bottom, and on two sides at once (the part smaller than the canvas, off_x and off_y > 0)
_BORDERS = [(1, (50, 30, 10, 0, (3, 5, 43, 35))), (1, (50, 30, 0, 0, (300, 480, 340, 510))), (1, (40, 50, 0, 20, (7, 0, 47, 30))),
            (1, (40, 50, 0, 0, (0, 9, 40, 39))), (1, (60, 60, 20, 30, (101, 203, 122, 220))), (2, (20, 20, 4, 0, (637, 470, 650, 490)))]


def test_one_call_of_mixed_crops_from_three_images_equals_pil_bit_for_bit():
    """S = 32: reduce, enlarge, one column (the centre 32 of 32 x 288), odd sizes, a wide canvas, zeros on every side"""
    crops = [(0, _plain(11, 3, 97, 61)), (1, _plain(335, 503, 5, 7)), (2, _plain(649, 481, 1, 9)), (2, _plain(1, 2, 301, 187)),
             (0, _plain(5, 101, 1300, 40))] + _BORDERS
    _run_and_check(_ctx(), 32, crops)


def test_more_than_one_strip_and_an_unchanged_size():
    """S = 80: two strips of 64 and 16 columns; 80 x 200 is not resampled at all, its centre 80 rows are copied"""
    _run_and_check(_ctx(), 80, [(1, _plain(7, 10, 333, 500)), (0, _plain(1201, 9, 80, 200)), (1, _BORDERS[4][1])])


def test_the_classifiers_own_size():
    _run_and_check(_ctx(), 224, [(2, _plain(10, 10, 640, 480))])


@pytest.mark.parametrize('interpolation', ['bicubic', 'bilinear', 'lanczos'])
def test_each_filter(interpolation):
    _run_and_check(_ctx(), 32, [(0, _plain(11, 3, 97, 61)), (1, _plain(335, 503, 5, 7)), _BORDERS[4]], interpolation)


def test_bad_arguments_are_refused_and_nothing_is_written():
    ctx = _ctx()
    _, pitch, _, dev = _images()[1]
    src = dev.data_ptr() + LEAD
    size = 8
    out = torch.full((3 * size * size * 4,), GUARD, dtype=torch.uint8, device='cuda:0')
    good = (src, pitch, 40, 30, 40, 30, 0, 0)
    host = np.zeros((30, 40, 3), np.uint8)
    std = K.IMAGENET_STD
    for recs, filt, sd in [([(host.ctypes.data, 120, 40, 30, 40, 30, 0, 0)], 0, std),             # a host pointer
                           ([good, (src, pitch, 40, 30, 45, 30, 6, 0)], 0, std),                   # the part leaves its canvas
                           ([good], 0, (0.229, 0.0, 0.225)),                                       # std = 0
                           ([good], 7, std)]:                                                      # an unknown filter
        with pytest.raises(HipError, match=r'\(-1\)'):
            ctx.classifier_input(recs, size, out.data_ptr(), filt, K.IMAGENET_MEAN, sd)
    with pytest.raises(HipError, match=r'\(-1\)'):
        ctx.classifier_input([good], 0, out.data_ptr())
    # a reduction too large for the chip: the first canvas for which the plan function finds no tile
    side = next(c for c in (1024, 4096, 16384, 65535) if J.classifier_plan(c, c, size, K.FILTERS['lanczos']) is None)
    assert J.classifier_plan(side // 4, side // 4, size, K.FILTERS['lanczos']) is not None
    assert ctx.classifier_input([good, (src, pitch, 4, 4, side, side, 0, 0)], size, out.data_ptr(), K.FILTERS['lanczos']) is False
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
    assert ctx.classifier_input([good], size, out.data_ptr()) is True
    torch.cuda.synchronize()
    assert int((bits(out.cpu().numpy().view(np.float32).reshape(3, size, size)) !=
                bits(K.classifier_input_host(_images()[1][0], _plain(0, 0, 40, 30), K.ClassifyOptions(torch.nn.Identity(), image_size=size)))).sum()) == 0


# ---- the detector ------------------------------------------------------------------------------------------------------------

def _spread_classifier():
    """the conv-free module of the CPU test with its weights scaled up, so that the five probabilities lie apart"""
    m = TinyClassifier()
    with torch.no_grad():
        m.fc.weight.mul_(6.0)
    return m.eval()


def _scene():
    from test_gpu_blur import _yolo_detector
    from test_gpu_tile_jpeg import _image
    if 'scene' not in _STATE:
        det = _yolo_detector(4)
        imgs = [np.ascontiguousarray(_image()[y:y + h, x:x + w]) for x, y, w, h in
                [(0, 0, 400, 300), (1500, 100, 333, 257), (100, 400, 320, 240), (900, 900, 301, 199)]]
        names = ['a.jpg', 'd/b.jpeg', 'e.png', 'g.jpg']
        plain = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5)
        assert all(r.get('failure') is None for r in plain)
        _STATE['scene'] = (det, imgs, names, plain)
    return _STATE['scene']


def _host_reference(imgs, plain, threshold, **kw):
    """the host leg on the CPU for every image: ([[(index, list)]], [inputs], [probabilities])"""
    opt = K.ClassifyOptions(_spread_classifier(), image_size=32, confidence_threshold=threshold, classification_threshold=0.1, **kw)
    lists, inputs, probs = [], [], []
    for img, r in zip(imgs, plain):
        lists.append(K.classifications_of_host_image(img, r['file'], r['detections'], opt)[0])
        for _, canvas in K.pick_crops(r['detections'], img.shape[1], img.shape[0], opt)[0]:
            inputs.append(K.classifier_input_host(img, canvas, opt))
            probs.append(K.run_model(opt.model_on(None), torch.from_numpy(inputs[-1])[None], 1)[0].numpy())
    return lists, inputs, probs


def _well_separated(probs, threshold=0.1, gap=1e-3):
    for p in probs:
        kept = np.sort(p[p >= threshold])
        if np.any(np.abs(p - threshold) < gap) or np.any(np.diff(kept) < gap):
            return False
    return True


def _threshold(imgs, plain):
    """a confidence threshold taken from the detections themselves -- the k-th highest confidence for the largest k up to 12 --
    at which, on the CPU, no two probabilities of a crop lie within 1e-3 of each other and none within 1e-3 of the threshold"""
    confs = sorted((d['conf'] for r in plain for d in r['detections']), reverse=True)
    for k in range(min(12, len(confs)), 0, -1):
        lists, inputs, probs = _host_reference(imgs, plain, confs[k - 1])
        if inputs and _well_separated(probs):
            return confs[k - 1], lists, inputs, probs
    raise AssertionError('no choice of detections separates the probabilities: {}'.format(confs[:12]))


def _hooked(seen):
    module = _spread_classifier()
    module.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().cpu().numpy().copy()))
    return module


def test_detector_classifies_what_the_host_leg_classifies():
    det, imgs, names, plain = _scene()
    threshold, lists, inputs, probs = _threshold(imgs, plain)
    print('threshold {} classifies {} detections'.format(threshold, len(inputs)))
    assert _well_separated(probs)                   # (so that the order below cannot fail for the reference alone)
    seen = []
    opt = K.ClassifyOptions(_hooked(seen), image_size=32, confidence_threshold=threshold, classification_threshold=0.1, batch_size=5)
    before = dict(det.classify_counts)
    res = det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, classify=opt)
    assert [{k: v for k, v in r.items() if k != 'classifications'} for r in res] == plain
    assert det.classify_counts['gpu'] - before['gpu'] == len(inputs) and det.classify_counts['host'] == before['host']
    got = np.concatenate(seen)
    assert got.shape == (len(inputs), 3, 32, 32)
    assert int((bits(got) != bits(np.stack(inputs))).sum()) == 0
    for r, want in zip(res, lists):
        assert [i for i, _ in r['classifications']] == [i for i, _ in want]
        for (_, a), (_, b) in zip(r['classifications'], want):
            assert [c for c, _ in a] == [c for c, _ in b]
            assert all(abs(x - y) <= 1e-4 + 1e-9 for (_, x), (_, y) in zip(a, b))
    # pipelined, and one image alone
    seen.clear()
    ticket = det.start_batch(imgs, names, detection_threshold=1e-5, classify=opt)
    piped = det.finish_batch(ticket)
    assert [r['classifications'] for r in piped] == [r['classifications'] for r in res]
    one = det.generate_detections_one_image(imgs[0], names[0], detection_threshold=1e-5, classify=opt)
    assert one['classifications'] == res[0]['classifications']


def test_jpeg_round_trip_of_the_crops_on_the_device():
    det, imgs, names, plain = _scene()
    confs = sorted((d['conf'] for r in plain for d in r['detections']), reverse=True)
    threshold = confs[min(6, len(confs)) - 1]
    _, inputs, _ = _host_reference(imgs, plain, threshold, jpeg_quality=75)
    assert inputs
    seen = []
    opt = K.ClassifyOptions(_hooked(seen), image_size=32, confidence_threshold=threshold, jpeg_quality=75)
    det.generate_detections_one_batch(imgs, names, detection_threshold=1e-5, classify=opt)
    got = np.concatenate(seen)
    assert got.shape == (len(inputs), 3, 32, 32)
    assert int((bits(got) != bits(np.stack(inputs))).sum()) == 0


def test_classify_beside_crops_blur_and_preview():
    from test_gpu_preview import _all_products, _threshold_with_every_product
    det, imgs, names, plain = _scene()
    products = _all_products()
    size_of = {n: (a.shape[1], a.shape[0]) for n, a in zip(names, imgs)}
    threshold, _ = _threshold_with_every_product(plain, size_of, products)
    base = det.generate_detections_one_batch(imgs, names, detection_threshold=threshold)
    products['classify'] = K.ClassifyOptions(_spread_classifier(), image_size=32, confidence_threshold=0.0)
    keys = {'crops': 'crops', 'blur': 'blurred', 'preview': 'preview', 'classify': 'classifications'}
    alone = {}
    for kw, options in products.items():
        res = det.generate_detections_one_batch(imgs, names, detection_threshold=threshold, **{kw: options})
        assert [{k: v for k, v in r.items() if k != keys[kw]} for r in res] == base
        alone[kw] = [r[keys[kw]] for r in res]
    assert sum(len(v) for v in alone['classify']) >= 1
    sources = [a.copy() for a in imgs]
    together = det.generate_detections_one_batch(imgs, names, detection_threshold=threshold, **products)
    assert [{k: v for k, v in r.items() if k not in keys.values()} for r in together] == base
    for kw, key in keys.items():
        assert [r[key] for r in together] == alone[kw], kw
    assert all(np.array_equal(a, b) for a, b in zip(imgs, sources))
