"""
The GPU half of the JPEG feed on the device: mdhip_jpeg_reconstruct rebuilds, bit for bit, the pixels Pillow decodes; the
network input behind mdhip_preprocess is the same bits either way; and a run with gpu_jpeg=True writes the JSON of a run
without it.  All of these fail on a tree without the feature (no symbol, no keyword).
"""

import itertools
import json

import numpy as np
import pytest

import jpeg_fixtures as JF

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (333, 517), (640, 480)]          # one of them not a multiple of 16


@pytest.fixture(scope='module')
def J():
    return JF.ensure_libmdjpeg()


@pytest.fixture(scope='module')
def ctx():
    from megadetector_amd import weights_io, yolo_yaml
    from megadetector_amd.hip_backend import HipContext
    W = weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1)
    c = HipContext(W, device=0, dtype='fp16', max_batch=8, max_h=256, max_w=256)
    yield c
    c.close()


def _load(path):
    from megadetector_amd.feed import load_image
    return np.asarray(load_image(str(path)))


def _coefficient_image(J, path):
    from megadetector_amd import feed
    from megadetector_amd.jpeg_host import CoefficientImage
    _, rotation = feed.open_for_coefficients(str(path))
    rc, hd, coef = J.decode(open(path, 'rb').read())
    assert rc == 0, hd.reason
    return CoefficientImage.from_header(hd, coef, rotation)


def _reconstruct(ctx, images):
    """-> (pixels read back, the device tensors)"""
    import torch
    dev = torch.device('cuda', 0)
    coefs = [torch.from_numpy(np.array(im.coef)).to(dev) for im in images]
    outs = [torch.full((int(np.prod(im.shape)) + 64,), 0xA5, dtype=torch.uint8, device=dev) for im in images]
    torch.cuda.synchronize()
    ctx.jpeg_reconstruct(images, [c.data_ptr() for c in coefs], [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    got = []
    for im, o in zip(images, outs):
        host = o.cpu().numpy()
        n = int(np.prod(im.shape))
        assert (host[n:] == 0xA5).all(), 'bytes behind the image were written'
        got.append(host[:n].reshape(im.shape))
    return got, outs


@pytest.mark.parametrize('sampling', JF.SAMPLINGS)
def test_reconstruct_equals_pillow(J, ctx, tmp_path, sampling):
    """every sampling x every rotation x three sizes x restart markers on / off, one image per call"""
    p = str(tmp_path / 'g.jpg')
    for (w, h), orientation, rst in itertools.product(SIZES, JF.ORIENTATIONS, (None, 'blocks')):
        kind = JF.CONTENTS[(w + (orientation or 0)) % 3]
        q = (30, 75, 95, 100)[(h + (orientation or 0)) % 4]
        JF.write_jpeg(p, JF.content(kind, w, h), sampling, q, False, rst, orientation)
        im = _coefficient_image(J, p)
        got, _ = _reconstruct(ctx, [im])
        np.testing.assert_array_equal(got[0], _load(p), err_msg=str((sampling, w, h, orientation, rst, kind, q)))


def test_reconstruct_mixed_batch_of_five(J, ctx, tmp_path):
    """five images of different sizes, samplings and rotations in ONE call; then a second, smaller call on the same context"""
    specs = [('420', (333, 517), 6, 'rows', 'noise'), ('444', (17, 9), None, None, 'noise'), ('gray', (640, 480), 3, None, 'natural'),
             ('422', (1, 1), 8, None, 'noise'), ('420', (640, 480), 8, 'blocks', 'natural')]
    paths, images = [], []
    for i, (sampling, (w, h), orientation, rst, kind) in enumerate(specs):
        p = JF.write_jpeg(str(tmp_path / 'b{}.jpg'.format(i)), JF.content(kind, w, h), sampling, 90, True, rst, orientation)
        paths.append(p)
        images.append(_coefficient_image(J, p))
    got, _ = _reconstruct(ctx, images)
    for g, p in zip(got, paths):
        np.testing.assert_array_equal(g, _load(p), err_msg=p)
    got, _ = _reconstruct(ctx, images[1:3])
    for g, p in zip(got, paths[1:3]):
        np.testing.assert_array_equal(g, _load(p), err_msg=p)


def test_network_input_is_the_same_bits(J, ctx, tmp_path):
    """mdhip_preprocess of the reconstructed device images == mdhip_preprocess of the PIL pixels (mdhip_read_input)"""
    from megadetector_amd.postprocess import letterbox_geometry
    specs = [('420', (333, 517), 6), ('422', (640, 480), None), ('gray', (200, 120), None), ('444', (97, 131), 3)]
    paths, images = [], []
    for i, (sampling, (w, h), orientation) in enumerate(specs):
        p = JF.write_jpeg(str(tmp_path / 'n{}.jpg'.format(i)), JF.content('natural', w, h), sampling, 85, orientation=orientation)
        paths.append(p)
        images.append(_coefficient_image(J, p))
    pixels = [_load(p) for p in paths]
    geoms = []
    for px in pixels:
        g = letterbox_geometry(px.shape[:2], new_shape=256, stride=64, auto=False, scaleup=True)
        geoms.append((px.shape[0], px.shape[1], g['new_unpad'][1], g['new_unpad'][0], g['top'], g['left'], 0))
    ctx.preprocess(pixels, geoms, 256, 256)
    want = ctx.read_input(len(pixels), 256, 256)
    _, outs = _reconstruct(ctx, images)
    ctx.preprocess([o.data_ptr() for o in outs], geoms, 256, 256)
    got = ctx.read_input(len(pixels), 256, 256)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_reconstruct_refuses_bad_arguments(J, ctx, tmp_path):
    import torch
    from megadetector_amd._lib import HipError
    p = JF.write_jpeg(str(tmp_path / 'a.jpg'), JF.content('noise', 32, 32), '420')
    im = _coefficient_image(J, p)
    out = torch.empty(32 * 32 * 3, dtype=torch.uint8, device='cuda:0')
    host = np.array(im.coef)
    with pytest.raises(HipError, match='device memory'):
        ctx.jpeg_reconstruct([im], [host.ctypes.data // 16 * 16], [out.data_ptr()])
    dev = torch.from_numpy(host).to('cuda:0')
    im.blocks_w = (1, 1, 1)
    with pytest.raises(HipError, match='blocks'):
        ctx.jpeg_reconstruct([im], [dev.data_ptr()], [out.data_ptr()])


@pytest.mark.parametrize('batch_size', [1, 4])
def test_end_to_end_json_identical(J, tmp_path, batch_size):
    """a folder of supported JPEGs, a progressive JPEG, a PNG and an unreadable file through run_detector_batch with a
    seeded-weight detector: the JSON with gpu_jpeg=True equals the JSON without it byte for byte (except
    detection_completion_time), and the counters show the supported files went the coefficient way"""
    from PIL import Image
    from megadetector_amd import run_detector, run_detector_batch as RDB
    folder = tmp_path / 'images'
    folder.mkdir()
    rng = np.random.default_rng(11)
    names = []
    specs = [('420', (160, 120), None), ('420', (160, 120), 6), ('422', (100, 150), None), ('444', (160, 120), 3),
             ('gray', (160, 120), None), ('420', (333, 217), 8), ('422', (160, 120), 1)]
    for i, (sampling, (w, h), orientation) in enumerate(specs):
        base = rng.integers(0, 256, (h // 10 + 1, w // 10 + 1, 3), dtype=np.uint8)
        img = np.kron(base, np.ones((10, 10, 1), dtype=np.uint8))[:h, :w]
        names.append(JF.write_jpeg(str(folder / 'img_{:02d}.jpg'.format(i)), img, sampling, 90, restart='rows' if i % 2 else None,
                                   orientation=orientation))
    names.append(JF.write_jpeg(str(folder / 'prog.jpg'), JF.content('natural', 160, 120), '420', 80, progressive=True))
    Image.fromarray(JF.content('natural', 160, 120)).save(str(folder / 'pic.png'))
    names.append(str(folder / 'pic.png'))
    (folder / 'broken.jpg').write_bytes(b'not a jpeg')
    names.append(str(folder / 'broken.jpg'))
    model = 'synthetic:YOLOV5N6_TEST:1'

    def run(gpu_jpeg, out):
        det = run_detector.load_detector(model, detector_options={'batch_size': batch_size})
        res = RDB.load_and_run_detector_batch(model, names, quiet=True, detector=det, batch_size=batch_size, use_image_queue=True,
                                              use_threads_for_queue=False, loader_workers=2, include_image_size=True,
                                              gpu_jpeg=gpu_jpeg)
        RDB.write_results_to_file(sorted(res, key=lambda r: r['file']), str(out), detector_file=model)
        text = open(out).read()
        j = json.loads(text)
        stamp = j['info']['detection_completion_time']
        return text.replace(stamp, 'T'), j, det.jpeg_images_reconstructed, dict(RDB.last_feed_counts)

    plain, j, n0, c0 = run(False, tmp_path / 'plain.json')
    fast, _, n1, c1 = run(True, tmp_path / 'fast.json')
    assert n0 == 0 and c0 == {'jpeg': 0, 'slot': 9, 'array': 0, 'fail': 1}
    assert n1 == 7 and c1 == {'jpeg': 7, 'slot': 2, 'array': 0, 'fail': 1}
    assert fast == plain
    assert len(j['images']) == len(names)
    assert sum(1 for im in j['images'] if 'failure' in im) == 1
    assert any(im.get('detections') for im in j['images'])
