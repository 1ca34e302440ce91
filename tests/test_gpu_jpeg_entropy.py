"""
Entropy decoding of JPEG scans on the device (mdhip_jpeg_entropy_decode): the coefficient planes equal mdjpeg_decode's value
for value, the pixels mdhip_jpeg_reconstruct makes of them equal Pillow's, damaged files are flagged exactly where
mdjpeg_decode refuses them while their clean neighbours in the batch decode, and nothing is written behind a buffer.
All of these fail on a tree without the feature (no symbol).
"""

import json

import numpy as np
import pytest

import jpeg_fixtures as JF
from test_jpeg_cpu import _damaged_variants

pytestmark = pytest.mark.gpu

GUARD = 4096                      # int16 values of 0x5A5A behind every coefficient buffer


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


def _scan_images(datas):
    from megadetector_amd.jpeg_host import ScanImage
    out = []
    for data in datas:
        rc, im, why = ScanImage.from_bytes(data)
        assert rc == 0, why
        out.append(im)
    return out


def _entropy_decode(ctx, images, subseq_bits=0):
    """-> (statuses, coefficient planes read back, the device tensors); checks the guard behind every buffer"""
    import torch
    dev = torch.device('cuda', 0)
    scans = [torch.from_numpy(np.array(im.scan_bytes if im.nbytes else np.zeros(1, np.uint8))).to(dev) for im in images]
    coefs = [torch.full((im.coef_count + GUARD,), 0x5A5A, dtype=torch.int16, device=dev) for im in images]
    torch.cuda.synchronize()
    status = ctx.jpeg_entropy_decode(images, [s.data_ptr() for s in scans], [c.data_ptr() for c in coefs], subseq_bits)
    torch.cuda.synchronize()
    planes = []
    for im, c in zip(images, coefs):
        host = c.cpu().numpy()
        assert (host[im.coef_count:] == 0x5A5A).all(), 'values behind the planes were written'
        planes.append(host[:im.coef_count])
    return status, planes, coefs


def _pixels(ctx, images, coefs):
    import torch
    cis = [im.coefficient_image() for im in images]
    outs = [torch.empty(int(np.prod(ci.shape)), dtype=torch.uint8, device='cuda:0') for ci in cis]
    ctx.jpeg_reconstruct(cis, [c.data_ptr() for c in coefs], [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return [o.cpu().numpy().reshape(ci.shape) for o, ci in zip(outs, cis)]


def _pil(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


@pytest.mark.parametrize('subseq_bits', [64, 128, 0])
def test_coefficients_equal_mdjpeg_decode_and_pixels_equal_pillow(J, ctx, tmp_path, subseq_bits):
    """every sampling x restart kind at small odd sizes, one batch per sampling; 0 = the default of 1024 bits"""
    for sampling in JF.SAMPLINGS:
        paths = []
        for i, (rst, (w, h), q, opt) in enumerate([(None, (200, 150), 95, False), ('rows', (17, 33), 75, True), ('blocks', (7, 5), 95, False),
                                                   (None, (1, 1), 75, False), ('rows', (200, 150), 98, True), (None, (16, 16), 30, True)]):
            kind = JF.CONTENTS[i % 3]
            paths.append(JF.write_jpeg(str(tmp_path / '{}_{}.jpg'.format(sampling, i)), JF.content(kind, w, h), sampling, q, opt, rst))
        datas = [open(p, 'rb').read() for p in paths]
        images = _scan_images(datas)
        status, planes, coefs = _entropy_decode(ctx, images, subseq_bits)
        assert (status == 0).all(), (sampling, status)
        for data, got, p in zip(datas, planes, paths):
            rc, _, want = J.decode(data)
            assert rc == 0
            np.testing.assert_array_equal(got, want, err_msg=p)
        for px, p in zip(_pixels(ctx, images, coefs), paths):
            np.testing.assert_array_equal(px, _pil(p), err_msg=p)


def test_mixed_batch_of_five_and_a_large_image(J, ctx, tmp_path):
    """five images that differ in sampling, restart and size in ONE call, one of them 640 x 480 noise without restart markers
    (thousands of subsequences: several workgroups per pass, changes that cross workgroups); then a smaller call"""
    specs = [('420', (333, 217), 'rows', 'noise', 90), ('444', (17, 9), None, 'noise', 95), ('gray', (640, 480), None, 'natural', 90),
             ('422', (1, 1), None, 'noise', 75), ('420', (640, 480), None, 'noise', 95)]
    paths = [JF.write_jpeg(str(tmp_path / 'b{}.jpg'.format(i)), JF.content(kind, w, h), sampling, q, True, rst)
             for i, (sampling, (w, h), rst, kind, q) in enumerate(specs)]
    datas = [open(p, 'rb').read() for p in paths]
    images = _scan_images(datas)
    for sel in (slice(0, 5), slice(1, 3)):
        status, planes, coefs = _entropy_decode(ctx, images[sel])
        assert (status == 0).all(), status
        for data, got in zip(datas[sel], planes):
            np.testing.assert_array_equal(got, J.decode(data)[2])
        for px, p in zip(_pixels(ctx, images[sel], coefs), paths[sel]):
            np.testing.assert_array_equal(px, _pil(p), err_msg=p)
    st = ctx.jpeg_entropy_stats()
    assert st['images'] == 2 and st['subsequences'] > 256
    # the 640 x 480 noise scan alone, 64-bit subsequences (tens of thousands of lanes over many workgroups): lanes that began
    # inside a symbol decode again, and a block longer than a workgroup's reach makes a change cross workgroups -- which
    # takes a launch that moves lanes after the first one, and one more that moves none
    status, planes, _ = _entropy_decode(ctx, images[4:5], 64)
    assert status[0] == 0
    np.testing.assert_array_equal(planes[0], J.decode(datas[4])[2])
    st = ctx.jpeg_entropy_stats()
    assert st['subsequences'] > 40 * 256 and st['decoded_again'] > st['subsequences'] // 4 and st['sync_launches'] >= 2


def test_clean_and_flagged_files_in_one_batch(J, ctx, tmp_path):
    """the damaged set of the CPU suite (what mdjpeg_scan passes of it) together with clean files in one call: status != 0
    exactly where mdjpeg_decode refuses, equal coefficients everywhere else, guards intact"""
    clean = [open(JF.write_jpeg(str(tmp_path / 'c{}.jpg'.format(i)), JF.content('noise', 96, 64), s, 90, False, r), 'rb').read()
             for i, (s, r) in enumerate([('420', None), ('444', 'rows'), ('gray', 'blocks')])]
    datas = list(clean)
    for name, data in _damaged_variants(tmp_path):
        if J.scan(data)[0] == 0:
            datas.append(data)
    assert len(datas) > 20
    datas = datas[:2] + datas[3:] + datas[2:3]                  # clean files first, in between and last
    images = _scan_images(datas)
    want = [J.decode(d) for d in datas]
    assert sum(1 for rc, _, _ in want if rc != 0) >= 10
    for bits in (64, 0):
        status, planes, _ = _entropy_decode(ctx, images, bits)
        for i, ((rc, hd, coef), st, got) in enumerate(zip(want, status, planes)):
            assert (st != 0) == (rc != 0), (i, bits, int(st), rc, hd.reason)
            if rc == 0:
                np.testing.assert_array_equal(got, coef, err_msg=str(i))


def test_bad_arguments_are_refused(J, ctx, tmp_path):
    import torch
    from megadetector_amd._lib import HipError
    data = open(JF.write_jpeg(str(tmp_path / 'a.jpg'), JF.content('noise', 32, 32), '420', restart='rows'), 'rb').read()
    im, = _scan_images([data])
    scan = torch.from_numpy(np.array(im.scan_bytes)).to('cuda:0')
    coef = torch.zeros(im.coef_count, dtype=torch.int16, device='cuda:0')
    with pytest.raises(HipError, match='n = 0'):
        ctx.jpeg_entropy_decode([], [], [])
    host = np.array(im.scan_bytes)
    with pytest.raises(HipError, match='device memory'):
        ctx.jpeg_entropy_decode([im], [host.ctypes.data], [coef.data_ptr()])
    with pytest.raises(HipError, match='subseq_bits'):
        ctx.jpeg_entropy_decode([im], [scan.data_ptr()], [coef.data_ptr()], 32)
    keep = im.seg_offsets.copy()
    im.seg_offsets[1] = im.nbytes + 100
    with pytest.raises(HipError, match='segment offset'):
        ctx.jpeg_entropy_decode([im], [scan.data_ptr()], [coef.data_ptr()])
    im.seg_offsets[:] = keep
    im.desc.info.blocks_w[0] += 1
    with pytest.raises(HipError, match='contradict'):
        ctx.jpeg_entropy_decode([im], [scan.data_ptr()], [coef.data_ptr()])
    im.desc.info.blocks_w[0] -= 1
    im.desc.scan_end = im.desc.scan_begin - 1
    with pytest.raises(HipError, match='scan range'):
        ctx.jpeg_entropy_decode([im], [scan.data_ptr()], [coef.data_ptr()])


@pytest.mark.parametrize('batch_size', [1, 4])
def test_end_to_end_json_identical(J, tmp_path, batch_size):
    """a folder of supported JPEGs, a progressive JPEG, a PNG, an unreadable file, a JPEG whose damage only symbol decoding
    sees and PIL still decodes, and one PIL refuses too, through run_detector_batch with a seeded-weight detector: the JSON
    with gpu_jpeg='entropy' equals the JSON without the switch byte for byte (except detection_completion_time); the
    counters are what the folder implies; the old gpu_jpeg=True run still gives that JSON and its old counts"""
    import warnings
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
    # damage inside the scan that leaves every marker alone: mdjpeg_scan passes the file, mdjpeg_decode refuses it
    good = open(names[0], 'rb').read()
    a, b = JF.scan_range(good)
    n_flagged = 0
    for k, pos in enumerate((a + (b - a) // 3, a + (b - a) // 2, a + 2 * (b - a) // 3)):
        d = bytearray(good)
        d[pos] ^= 0x55
        if d[pos] == 0xFF or d[pos - 1] == 0xFF:
            continue
        d = bytes(d)
        if J.scan(d)[0] == 0 and J.decode(d)[0] == J.MDJPEG_ECORRUPT:
            p = folder / 'flip_{}.jpg'.format(k)
            p.write_bytes(d)
            names.append(str(p))
            n_flagged += 1
    assert n_flagged >= 1
    model = 'synthetic:YOLOV5N6_TEST:1'

    def run(gpu_jpeg, out):
        det = run_detector.load_detector(model, detector_options={'batch_size': batch_size})
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = RDB.load_and_run_detector_batch(model, names, quiet=True, detector=det, batch_size=batch_size, use_image_queue=True,
                                                  use_threads_for_queue=False, loader_workers=2, include_image_size=True,
                                                  gpu_jpeg=gpu_jpeg)
        RDB.write_results_to_file(sorted(res, key=lambda r: r['file']), str(out), detector_file=model)
        text = open(out).read()
        j = json.loads(text)
        stamp = j['info']['detection_completion_time']
        return (text.replace(stamp, 'T'), j, (det.jpeg_images_reconstructed, det.jpeg_images_entropy_decoded, det.jpeg_entropy_fallbacks),
                dict(RDB.last_feed_counts))

    plain, j, n0, c0 = run(False, tmp_path / 'plain.json')
    n_pil_fail = sum(1 for im in j['images'] if 'failure' in im)            # broken.jpg and the flipped files PIL refuses
    n_slot = 9 + n_flagged - (n_pil_fail - 1)
    assert n0 == (0, 0, 0) and c0 == {'jpeg': 0, 'slot': n_slot, 'array': 0, 'fail': n_pil_fail}
    fast, _, n1, c1 = run('entropy', tmp_path / 'fast.json')
    assert fast == plain
    assert n1 == (7, 7, n_flagged), n1
    assert c1 == {'jpeg': 0, 'scan': 7 + n_flagged, 'slot': 2, 'array': 0, 'fail': 1}
    old, _, n2, c2 = run(True, tmp_path / 'old.json')
    assert old == plain
    assert n2 == (7, 0, 0) and c2 == {'jpeg': 7, 'slot': 2 + n_flagged - (n_pil_fail - 1), 'array': 0, 'fail': n_pil_fail}
    assert len(j['images']) == len(names)
    assert any(im.get('detections') for im in j['images'])
