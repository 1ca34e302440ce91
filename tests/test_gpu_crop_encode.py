"""
Entropy encoding of crops on the device: mdhip_jpeg_encode (HipContext.jpeg_encode) against Pillow, byte for byte.

Windows of a parent image with an odd pitch (2101 pixels a row) at unaligned origins; the file jpeg_host.jfif_file builds
around each scan must be the bytes Image.fromarray(window).save(f, 'JPEG', quality=q) writes.  Canary bytes lie around the
output buffer; a capacity one byte short is refused with the need reported and nothing written beyond it.
"""

import os

import numpy as np
import pytest
import torch

from megadetector_amd import _lib, jpeg_host
from test_gpu_tile_jpeg import CANARY, H, W, _ctx, _image, _parent
from test_tile_jpeg_cpu import make_content, pillow_file

pytestmark = pytest.mark.gpu

_STATE = {}
SMALL = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 17), (33, 15), (100, 75), (17, 33), (33, 17)]      # w x h


def _encode(ctx, parent, wins, quality, capacity=None):
    """-> (fits, files or None, needed, canaries intact, bytes of the buffer)"""
    pitch = W * 3
    if capacity is None:
        capacity = sum(ctx.jpeg_encode_bound(w, h) for _, _, w, h in wins)
    buf = torch.full((capacity + 2 * CANARY,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    fits, offs, lens, needed = ctx.jpeg_encode([parent.data_ptr() + y * pitch + x * 3 for x, y, _, _ in wins],
                                               [(w, h) for _, _, w, h in wins], [pitch] * len(wins), quality,
                                               buf.data_ptr() + CANARY, capacity)
    host = buf.cpu().numpy()
    intact = bool((host[:CANARY] == 0xA5).all() and (host[CANARY + capacity:] == 0xA5).all())
    body = host[CANARY:CANARY + capacity]
    assert offs[0] == 0 and (offs[1:] == offs[:-1] + lens[:-1]).all() and offs[-1] + lens[-1] == needed
    files = None
    if fits:
        assert (body[needed:] == 0xA5).all(), 'bytes behind the last scan were written'
        files = [jpeg_host.jfif_file(w, h, quality, body[o:o + n].tobytes()) for (_, _, w, h), o, n in zip(wins, offs, lens)]
    return fits, files, needed, intact, body


def _check(img, wins, files, quality):
    for (x, y, w, h), got in zip(wins, files):
        want = pillow_file(np.ascontiguousarray(img[y:y + h, x:x + w]), quality)
        assert got == want, 'window {} at quality {}: {} bytes, Pillow wrote {}'.format((x, y, w, h), quality, len(got), len(want))


def _small_windows():
    """every small size over noise, checkerboard, gradient and constant fields, at odd origins and in the bottom-right corner"""
    out = []
    for i, (w, h) in enumerate(SMALL):
        out.append((601 + 2 * i, 3 + 2 * (i % 5), w, h))             # noise
        out.append((3 + 2 * i, 5 + 2 * i, w, h))                     # saturated checkerboard
        out.append((201 + 16 * i, 501 + i, w, h))                    # gradient
        out.append((11 + i, 1101 + i, w, h))                         # white
        out.append((250 + i, 1250 + i, w, h))                        # red / green border
        out.append((W - w, H - h, w, h))
    return out


@pytest.mark.parametrize('quality', [1, 50, 75, 95, 100])
def test_small_windows_equal_pillow_files(quality):
    img, parent, ctx = _image(), _parent(), _ctx()
    wins = _small_windows()
    assert all(x + w <= W and y + h <= H for x, y, w, h in wins)
    fits, files, _, intact, _ = _encode(ctx, parent, wins, quality)
    assert fits and intact
    _check(img, wins, files, quality)


def _mixed_windows():
    """at least 70 crops of mixed sizes in one call: 1 x 1, a 700 x 500 noise crop, one across several contents, many small"""
    rng = np.random.default_rng(17)
    wins = [(1301, 801, 700, 500), (W - 1, H - 1, 1, 1), (401, 1001, 333, 257), (1, 1, 640, 640)]
    while len(wins) < 72:
        w, h = int(rng.integers(1, 120)), int(rng.integers(1, 120))
        wins.append((int(rng.integers(0, W - w)), int(rng.integers(0, H - h)), w, h))
    return wins


def _noisy():
    """the parent's upper 700 rows (checkerboard, gradient, a bundled image), pure noise below: (host image, device copy)"""
    if 'noisy' not in _STATE:
        img = make_content('noise', W, H, seed=11)
        img[:700] = _image()[:700]
        t = torch.empty(H * W * 3, dtype=torch.uint8, device='cuda:0')
        t.copy_(torch.from_numpy(img.reshape(-1)))
        torch.cuda.synchronize()
        _STATE['noisy'] = (img, t)
    return _STATE['noisy']


def test_seventy_mixed_crops_in_one_call_at_quality_100():
    (img, parent), ctx = _noisy(), _ctx()
    wins = _mixed_windows()
    x, y, w, h = wins[0]
    assert len(wins) >= 70 and (w, h) == (700, 500) and (1, 1) in [(a[2], a[3]) for a in wins]
    assert np.array_equal(img[y:y + h, x:x + w], make_content('noise', W, H, seed=11)[y:y + h, x:x + w])      # the large crop is pure noise
    fits, files, needed, intact, _ = _encode(ctx, parent, wins, 100)
    assert fits and intact
    _check(img, wins, files, 100)
    assert np.array_equal(parent.cpu().numpy(), img.reshape(-1)), 'the parent image was written to'
    # and at the reference's quality, with an exact capacity
    fits, files, needed, intact, _ = _encode(ctx, parent, wins, 95, capacity=_encode(ctx, parent, wins, 95)[2])
    assert fits and intact
    _check(img, wins, files, 95)


def test_capacity_one_byte_short_is_refused_and_a_retry_succeeds():
    img, parent, ctx = _image(), _parent(), _ctx()
    wins = _mixed_windows()[:12]
    fits, files, needed, intact, full = _encode(ctx, parent, wins, 95)
    assert fits and intact
    pitch = W * 3
    ptrs = [parent.data_ptr() + y * pitch + x * 3 for x, y, _, _ in wins]
    buf = torch.full((needed + CANARY,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    import ctypes as C
    ql, qc = jpeg_host.quant_tables(95)
    n = len(wins)
    offs, lens, need = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int64(0)
    rc = ctx.lib.mdhip_jpeg_encode(ctx.h, C.cast((C.c_void_p * n)(*ptrs), C.POINTER(C.c_void_p)), (C.c_int32 * n)(*[a[2] for a in wins]),
                                   (C.c_int32 * n)(*[a[3] for a in wins]), (C.c_int64 * n)(*[pitch] * n), n,
                                   ql.ctypes.data_as(C.POINTER(C.c_uint16)), qc.ctypes.data_as(C.POINTER(C.c_uint16)),
                                   C.c_void_p(buf.data_ptr()), needed - 1, offs, lens, C.byref(need), None)
    assert rc == _lib.MDHIP_ECAPACITY == -5
    assert need.value == needed
    host = buf.cpu().numpy()
    assert (host[needed - 1:] == 0xA5).all(), 'a byte at or beyond the capacity was written'
    assert np.array_equal(host[:needed - 1], full[:needed - 1])
    fits, again, needed2, intact, _ = _encode(ctx, parent, wins, 95, capacity=need.value)
    assert fits and intact and needed2 == needed and again == files
    _check(img, wins, files, 95)


def test_host_pointers_and_bad_arguments_are_refused():
    ctx, parent = _ctx(), _parent()
    out = torch.empty(ctx.jpeg_encode_bound(64, 64), dtype=torch.uint8, device='cuda:0')
    host = np.zeros(64 * 64 * 3, np.uint8)
    from megadetector_amd._lib import HipError
    with pytest.raises(HipError, match='host pointer'):
        ctx.jpeg_encode([host.ctypes.data], [(64, 64)], [192], 95, out.data_ptr(), out.numel())
    with pytest.raises(HipError, match='host pointer'):
        ctx.jpeg_encode([parent.data_ptr()], [(64, 64)], [W * 3], 95, host.ctypes.data, host.size)
    with pytest.raises(HipError):
        ctx.jpeg_encode([parent.data_ptr()], [(0, 64)], [W * 3], 95, out.data_ptr(), out.numel())
    with pytest.raises(HipError):
        ctx.jpeg_encode([parent.data_ptr()], [(64, 64)], [191], 95, out.data_ptr(), out.numel())
    with pytest.raises(ValueError, match='1 to 100'):
        ctx.jpeg_encode([parent.data_ptr()], [(64, 64)], [W * 3], 0, out.data_ptr(), out.numel())
    assert ctx.jpeg_encode_bound(0, 1) == -1 and ctx.jpeg_encode_bound(1, 1) == jpeg_host.encode_bound(1, 1)


def _host_crops(img, name, dets, options):
    """PIL crop().save() of the detections on the host copy, by the reference's statements"""
    import io
    from PIL import Image
    from test_crops_cpu import reference_crop
    from megadetector_amd import crops as K
    pil = Image.fromarray(img)
    out = []
    ordered = K.output_order(dets, options.output_threshold)
    for i, det in enumerate(ordered):
        if det['conf'] < options.confidence_threshold:
            continue
        crop = reference_crop(pil, det['bbox'], options.expansion)
        if crop.size[0] <= 0 or crop.size[1] <= 0:
            continue
        bio = io.BytesIO()
        crop.save(bio, format=Image.registered_extensions()[os.path.splitext(name)[1].lower()], quality=options.quality)
        out.append((i, K.crop_filename(name, i), bio.getvalue()))
    return out


def test_crops_of_a_device_image_equal_pil_crop_and_save():
    """rectangles, ids, names and files of megadetector_amd.crops for an image in device memory, against PIL on the host copy"""
    from megadetector_amd import crops as K
    img, parent, ctx = _image(), _parent(), _ctx()
    rng = np.random.default_rng(23)
    confs = sorted(rng.random(14).round(3).tolist(), reverse=True)
    dets = [{'category': str(1 + i % 3), 'conf': c, 'bbox': [float(v) for v in (rng.random(2) * 0.8).tolist() + (rng.random(2) * 0.3).tolist()]}
            for i, c in enumerate(confs)]
    dets[1]['bbox'] = [0.95, 0.9, 0.2, 0.3]                          # past the border
    dets[2]['bbox'] = [0.4, 0.4, 0.0, 0.1]                           # no area
    dets[3]['bbox'] = [100.5 / W, 200.5 / H, 64.0 / W, 48.0 / H]
    warnings = []
    for name, expansion in (('cam/a.jpg', 0), ('b.JPEG', 9), ('c.png', 0)):
        opt = K.CropOptions(confidence_threshold=0.0, expansion=expansion)
        got, skipped = K.crops_of_device_image(ctx, parent, W, H, name, dets, opt, warn=warnings.append)
        assert skipped == (1 if expansion == 0 else 0)                # (expansion gives the line an area)
        assert got == _host_crops(img, name, dets, opt) and len(got) == len(dets) - skipped
    assert len(warnings) == 2 and all('detection 2' in w and ' of ' in w for w in warnings)


def _yolo_detector(batch):
    from megadetector_amd import weights_io, yolo_yaml
    from megadetector_amd.detector import HIPDetector
    key = ('det', batch)
    if key not in _STATE:
        d = HIPDetector(weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1), {'batch_size': batch, 'max_image_size': 320, 'device': 'cuda:0'})
        d.default_image_size = 320
        _STATE[key] = d
    return _STATE[key]


def test_detector_crops_synchronous_and_pipelined_equal_pil():
    from megadetector_amd import crops as K
    det = _yolo_detector(4)
    imgs = [np.ascontiguousarray(_image()[y:y + h, x:x + w]) for x, y, w, h in
            [(0, 0, 400, 300), (1500, 100, 500, 600), (100, 400, 640, 480), (500, 0, 333, 257), (0, 1100, 600, 400), (900, 900, 301, 199)]]
    names = ['a.jpg', 'd/b.jpeg', 'c.JPG', 'e.png', 'f.jpg', 'g.jpg']
    opt = K.CropOptions(confidence_threshold=0.0)
    plain = det.generate_detections_one_batch(imgs, names, detection_threshold=0.01)
    before = dict(det.crop_counts)
    sync = det.generate_detections_one_batch(imgs, names, detection_threshold=0.01, crops=opt)
    tickets = [det.start_batch(imgs[:4], names[:4], detection_threshold=0.01, crops=opt),
               det.start_batch(imgs[4:], names[4:], detection_threshold=0.01, crops=opt)]
    piped = det.finish_batch(tickets[0]) + det.finish_batch(tickets[1])
    one = det.generate_detections_one_image(imgs[1], names[1], detection_threshold=0.01, crops=opt)
    assert [{k: v for k, v in r.items() if k != 'crops'} for r in sync] == plain
    assert [r['crops'] for r in sync] == [r['crops'] for r in piped] and sync == piped and one == sync[1]
    total = 0
    for r, img in zip(sync, imgs):
        assert r.get('failure') is None
        assert r['crops'] == _host_crops(img, r['file'], r['detections'], opt)
        total += len(r['crops'])
    assert total >= 1, 'the test produced no crop'
    n_png = len(sync[3]['crops'])
    assert det.crop_counts['host'] - before['host'] == 2 * n_png and det.crop_counts['gpu'] - before['gpu'] == 2 * (total - n_png) + len(one['crops'])
    assert 'crops' not in det.generate_detections_one_batch(imgs[:1], names[:1])[0]


def test_two_tickets_outstanding_and_the_second_holds_three_shape_groups():
    """the second ticket's groups go through both staging buffers while the first ticket's crops are not encoded yet: the
    first ticket's pixels must survive (a buffer whose crops are owed is not reused).  Three groups, not more: the pipeline
    has four NMS slots, so the groups in flight of two outstanding tickets are at most four, with or without crops"""
    from megadetector_amd import crops as K
    det = _yolo_detector(4)
    img = _image()
    cut = lambda x, y, w, h: np.ascontiguousarray(img[y:y + h, x:x + w])
    first = [cut(0, 0, 400, 300), cut(1500, 100, 400, 300), cut(100, 400, 400, 300)]
    second = [cut(500, 0, 300, 400), cut(0, 1100, 400, 400), cut(900, 900, 600, 200),
              cut(1600, 200, 300, 400), cut(300, 300, 400, 400)]
    shapes = {tuple(det.preprocess_image(a)['img_processed'].shape) for a in second}
    assert len(shapes) == 3 and len({tuple(det.preprocess_image(a)['img_processed'].shape) for a in first}) == 1
    n1 = ['a{}.jpg'.format(i) for i in range(len(first))]
    n2 = ['b{}.jpg'.format(i) for i in range(len(second))]
    opt = K.CropOptions(confidence_threshold=0.0)
    want1 = det.generate_detections_one_batch(first, n1, detection_threshold=0.0005, crops=opt)
    want2 = det.generate_detections_one_batch(second, n2, detection_threshold=0.0005, crops=opt)
    ta = det.start_batch(first, n1, detection_threshold=0.0005, crops=opt)
    tb = det.start_batch(second, n2, detection_threshold=0.0005, crops=opt)
    got1, got2 = det.finish_batch(ta), det.finish_batch(tb)
    assert got1 == want1 and got2 == want2
    total = 0
    for r, a in zip(got1 + got2, first + second):
        assert r.get('failure') is None and r['crops'] == _host_crops(a, r['file'], r['detections'], opt)
        total += len(r['crops'])
    print('crops of the first ticket:', sum(len(r['crops']) for r in got1), 'all:', total)
    assert sum(len(r['crops']) for r in got1) >= 1 and total >= 2, 'the test produced no crop'
    # and once more, so that buffers handed out while crops were owed are themselves reused
    ta = det.start_batch(first, n1, detection_threshold=0.0005, crops=opt)
    tb = det.start_batch(second, n2, detection_threshold=0.0005, crops=opt)
    assert det.finish_batch(ta) == want1 and det.finish_batch(tb) == want2


def _cut(x, y, w, h):
    return np.ascontiguousarray(_image()[y:y + h, x:x + w])


def _three_one_shape_batches():
    """three batches of one letterboxed shape each, with names: for calls that are in flight together"""
    batches = [[_cut(0, 0, 400, 300), _cut(1500, 100, 400, 300), _cut(100, 400, 400, 300)],
               [_cut(500, 0, 300, 400), _cut(1600, 200, 300, 400)],
               [_cut(0, 1100, 400, 400), _cut(300, 300, 400, 400), _cut(900, 900, 333, 333)]]
    det = _yolo_detector(4)
    for b in batches:
        assert len({tuple(det.preprocess_image(a)['img_processed'].shape) for a in b}) == 1
    return batches, [['{}{}.jpg'.format(c, i) for i in range(len(b))] for c, b in zip('abc', batches)]


def _crops_equal_the_host_leg(results, images, opt):
    total = 0
    for r, a in zip(results, images):
        assert r.get('failure') is None and r['crops'] == _host_crops(a, r['file'], r['detections'], opt)
        total += len(r['crops'])
    return total


def test_a_synchronous_call_between_two_outstanding_tickets():
    """generate_detections_one_batch shares the NMS slots and the staging buffers with the tickets: three groups in flight
    (of four slots), the tickets' crops still owed while the call in the middle takes a staging buffer and makes its own"""
    from megadetector_amd import crops as K
    det = _yolo_detector(4)
    (first, second, third), (n1, n2, n3) = _three_one_shape_batches()
    opt = K.CropOptions(confidence_threshold=0.0)
    kw = dict(detection_threshold=0.0005, crops=opt)
    want1 = det.finish_batch(det.start_batch(first, n1, **kw))
    want2 = det.finish_batch(det.start_batch(second, n2, **kw))
    want3 = det.generate_detections_one_batch(third, n3, **kw)
    for _ in range(2):          # (the second time the buffers handed out while crops were owed are themselves reused)
        ta = det.start_batch(first, n1, **kw)
        tb = det.start_batch(second, n2, **kw)
        got3 = det.generate_detections_one_batch(third, n3, **kw)
        got1, got2 = det.finish_batch(ta), det.finish_batch(tb)
        assert got1 == want1 and got2 == want2 and got3 == want3
    total = _crops_equal_the_host_leg(got1 + got2 + got3, first + second + third, opt)
    print('crops:', [sum(len(r['crops']) for r in g) for g in (got1, got2, got3)])
    assert all(sum(len(r['crops']) for r in g) >= 1 for g in (got1, got2, got3)) and total >= 3, 'a call produced no crop'


@pytest.mark.parametrize('jpeg_quality', [None, 90])
def test_a_tiled_call_between_two_outstanding_tickets(jpeg_quality):
    """generate_detections_for_tiles runs on the streams and in the NMS slots of the tickets"""
    from megadetector_amd import crops as K
    det = _yolo_detector(4)
    (first, second, _), (n1, n2, _) = _three_one_shape_batches()
    opt = K.CropOptions(confidence_threshold=0.0)
    kw = dict(detection_threshold=0.0005, crops=opt)
    big = _cut(200, 300, 700, 900)
    origins = [(0, 0), (300, 600), (151, 299)]
    tiled = lambda: det.generate_detections_for_tiles(big, origins, (400, 300), detection_threshold=0.0005, jpeg_quality=jpeg_quality)
    want1 = det.finish_batch(det.start_batch(first, n1, **kw))
    want2 = det.finish_batch(det.start_batch(second, n2, **kw))
    want_tiles = tiled()
    assert len(want_tiles) == 3 and all(r.get('failure') is None for r in want_tiles)
    assert sum(len(r['detections']) for r in want_tiles) >= 1, 'the tiles gave no detection'
    ta = det.start_batch(first, n1, **kw)
    tb = det.start_batch(second, n2, **kw)
    got_tiles = tiled()
    got1, got2 = det.finish_batch(ta), det.finish_batch(tb)
    assert got_tiles == want_tiles and got1 == want1 and got2 == want2
    assert _crops_equal_the_host_leg(got1 + got2, first + second, opt) >= 2


@pytest.mark.parametrize('entry', ['one_batch', 'tickets'])
def test_a_failing_chunk_is_marked_alone_and_the_detector_recovers(entry):
    """nine images of one shape at max_batch 4 are three chunks; the forward of the second raises (a Python exception on the
    host, nothing is done to the device): its images fail, the chunks around it and the next call are undisturbed"""
    from megadetector_amd import crops as K
    from megadetector_amd._lib import HipError
    from megadetector_amd.constants import FAILURE_INFER
    det = _yolo_detector(4)
    imgs = [_cut(37 * i, 53 * i, 400, 300) for i in range(9)]
    names = ['f{}.jpg'.format(i) for i in range(9)]
    opt = K.CropOptions(confidence_threshold=0.0)
    if entry == 'one_batch':
        call = lambda: det.generate_detections_one_batch(imgs, names, detection_threshold=0.0005, crops=opt)
    else:
        call = lambda: det.finish_batch(det.start_batch(imgs, names, detection_threshold=0.0005, crops=opt))
    want = call()
    assert _crops_equal_the_host_leg(want, imgs, opt) >= 1
    forward, calls = det._ctx.forward, []

    def second_call_raises(*args, **kwargs):
        calls.append(args)
        if len(calls) == 2:
            raise HipError('mdhip_forward failed (test): raised by the test on the host')
        return forward(*args, **kwargs)
    det._ctx.forward = second_call_raises
    try:
        got = call()
    finally:
        del det._ctx.forward
    assert len(calls) == 3
    assert got[:4] == want[:4] and got[8:] == want[8:]
    for r, name in zip(got[4:8], names[4:8]):
        assert r == {'file': name, 'detections': None, 'failure': FAILURE_INFER, 'crops': []}
    assert call() == want


def test_a_group_whose_nms_slot_a_ticket_holds_is_refused():
    """the four NMS result slots are taken in turn: with two tickets outstanding the third chunk of a call in between would
    write into the first ticket's slot.  It fails instead, the tickets keep their results, and the detector goes on"""
    from megadetector_amd import crops as K
    from megadetector_amd.constants import FAILURE_INFER
    det = _yolo_detector(4)
    (first, second, _), (n1, n2, _) = _three_one_shape_batches()
    imgs = [_cut(37 * i, 53 * i, 400, 300) for i in range(9)]
    names = ['f{}.jpg'.format(i) for i in range(9)]
    kw = dict(detection_threshold=0.0005, crops=K.CropOptions(confidence_threshold=0.0))
    want1 = det.finish_batch(det.start_batch(first, n1, **kw))
    want2 = det.finish_batch(det.start_batch(second, n2, **kw))
    want = det.generate_detections_one_batch(imgs, names, **kw)
    ta = det.start_batch(first, n1, **kw)
    tb = det.start_batch(second, n2, **kw)
    got = det.generate_detections_one_batch(imgs, names, **kw)
    assert got[:8] == want[:8]
    assert got[8] == {'file': names[8], 'detections': None, 'failure': FAILURE_INFER, 'crops': []}
    assert det.finish_batch(ta) == want1 and det.finish_batch(tb) == want2
    assert det.generate_detections_one_batch(imgs, names, **kw) == want


def test_driver_three_feeds_write_the_second_pass(tmp_path):
    """a folder of Pillow-written .jpg files and one .png through run_detector_batch with a crop folder: the PIL feed, gpu_jpeg
    and gpu_jpeg='entropy' write identical folders, equal to the reference's second pass over the results; no .jpg crop
    took the host path"""
    import warnings
    from PIL import Image
    from megadetector_amd import run_detector, run_detector_batch as RDB
    from test_crops_cpu import _tree, second_pass
    folder = tmp_path / 'images'
    (folder / 'sub').mkdir(parents=True)
    rects = [(0, 0, 400, 300), (1500, 100, 500, 600), (100, 400, 640, 480), (500, 0, 333, 257), (0, 1100, 600, 400)]
    for i, (x, y, w, h) in enumerate(rects):
        Image.fromarray(np.ascontiguousarray(_image()[y:y + h, x:x + w])).save(str(folder / ('sub' if i % 2 else '.') / 'i{}.jpg'.format(i)), quality=90)
    Image.fromarray(np.ascontiguousarray(_image()[200:500, 300:700])).save(str(folder / 'p.png'))
    names = RDB.find_images(str(folder), recursive=True)
    model = 'synthetic:YOLOV5N6_TEST:1'
    trees, outs = [], []
    for k, gpu_jpeg in enumerate([False, True, 'entropy']):
        det = run_detector.load_detector(model, detector_options={'batch_size': 4})
        crop_folder = str(tmp_path / 'crops{}'.format(k))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = RDB.load_and_run_detector_batch(model, names, quiet=True, detector=det, batch_size=4, use_image_queue=True,
                                                  use_threads_for_queue=False, loader_workers=2, gpu_jpeg=gpu_jpeg,
                                                  confidence_threshold=0.0005, crop_folder=crop_folder, crop_base=str(folder),
                                                  crop_confidence_threshold=0.0)
        counts = dict(RDB.last_crop_counts)
        out = RDB.write_results_to_file(res, str(tmp_path / 'o{}.json'.format(k)), relative_path_base=str(folder), info={'format_version': '1.6'})
        tree = _tree(crop_folder)
        assert counts['host_jpeg'] == 0 and counts['files'] == len(tree)
        n_jpg, n_png = sum(n.endswith('.jpg') for n in tree), sum(n.endswith('.png') for n in tree)
        assert det.crop_counts['gpu'] == n_jpg and det.crop_counts['host'] == n_png, det.crop_counts      # which path made the bytes
        assert counts['gpu'] == sum(n.endswith('.jpg') for n in tree) and counts['host_other'] == sum(n.endswith('.png') for n in tree)
        if gpu_jpeg:
            assert det.jpeg_images_reconstructed == len(rects)
        trees.append(tree)
        outs.append(out)
    assert outs[0] == outs[1] == outs[2]
    want = second_pass(outs[0], str(folder), threshold=0.0)
    print('crops:', len(want), 'png:', sum(n.endswith('.png') for n in want))
    assert len(want) >= 1 and any(n.endswith('.png') for n in want) and any(n.startswith('sub/') for n in want)
    assert trees[0] == want and trees[1] == want and trees[2] == want
