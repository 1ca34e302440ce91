"""
The device JPEG feed on files Pillow's encoder never writes (tests/jpeg_foreign.py; the host side is
test_jpeg_foreign_cpu.py): mdhip_jpeg_entropy_decode writes mdjpeg_decode's coefficients for every foreign anatomy -- six
Huffman tables, ids 0 / 3 / 1, 16-bit codes, one-MCU restart segments -- and flags exactly what mdjpeg_decode refuses;
mdhip_jpeg_reconstruct makes Pillow's pixels of them, also of blocks whose samples leave [-512, 511] and of 16-bit
quantisation tables.  Every comparison is equality.
"""

import io
import warnings

import numpy as np
import pytest

import jpeg_fixtures as JF
import jpeg_foreign as F
from test_jpeg_foreign_cpu import damaged_foreign

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


@pytest.fixture(scope='module')
def corpus(J, tmp_path_factory):
    return F.structural_corpus(J, tmp_path_factory.mktemp('foreign'))


def _load(data):
    from megadetector_amd.feed import load_image
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.asarray(load_image(io.BytesIO(data)))


def _scan_images(datas):
    """ScanImage of every file, with the rotation load_image would apply"""
    from megadetector_amd import feed
    from megadetector_amd.jpeg_host import ScanImage
    out = []
    for data in datas:
        _, rotation = feed.open_for_coefficients(io.BytesIO(data))
        rc, im, why = ScanImage.from_bytes(data, rotation)
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


def _reconstruct(ctx, cis, coefs):
    """pixels of CoefficientImages whose planes are the device tensors `coefs`; checks the bytes behind every image"""
    import torch
    outs = [torch.full((int(np.prod(ci.shape)) + 64,), 0xA5, dtype=torch.uint8, device='cuda:0') for ci in cis]
    torch.cuda.synchronize()
    ctx.jpeg_reconstruct(cis, [c.data_ptr() for c in coefs], [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    got = []
    for ci, o in zip(cis, outs):
        host = o.cpu().numpy()
        n = int(np.prod(ci.shape))
        assert (host[n:] == 0xA5).all(), 'bytes behind the image were written'
        got.append(host[:n].reshape(ci.shape))
    return got


@pytest.mark.parametrize('subseq_bits', [64, 0])
def test_structural_corpus_on_the_device(J, ctx, corpus, subseq_bits):
    """every knob alone and the camera-like combinations over four samplings and 1 x 1, in batches of 8: status 0, the planes
    of mdjpeg_decode (which are the serialised ones), guards intact, and Pillow's pixels behind mdhip_jpeg_reconstruct,
    rotation included; 0 = the default of 1024 bits"""
    assert len(corpus) == 5 * 28
    n_rotated = 0
    for at in range(0, len(corpus), 8):
        batch = corpus[at:at + 8]
        datas = [e[1] for e in batch]
        images = _scan_images(datas)
        status, planes, coefs = _entropy_decode(ctx, images, subseq_bits)
        assert (status == 0).all(), ([e[0] for e in batch], status)
        for (name, data, header, coef, knobs), got in zip(batch, planes):
            rc, _, want = J.decode(data)
            assert rc == 0
            np.testing.assert_array_equal(got, want, err_msg=name)
            np.testing.assert_array_equal(got, coef, err_msg=name)
        pixels = _reconstruct(ctx, [im.coefficient_image() for im in images], coefs)
        for (name, data, *_), px, im in zip(batch, pixels, images):
            np.testing.assert_array_equal(px, _load(data), err_msg=name)
            n_rotated += im.rotation != 0
    assert n_rotated == 4 * 3                                  # exif6, camera_a and camera_c of the colour bases


def _large_foreign(J, tmp_path, **knobs):
    p = JF.write_jpeg(str(tmp_path / 'large.jpg'), JF.content('noise', 200, 150), '420', 95)
    rc, header, coef = J.decode(open(p, 'rb').read())
    assert rc == 0
    return F.foreign_file(header, coef, **knobs), coef


@pytest.mark.parametrize('dri', [1, 7])
def test_one_mcu_segments_and_16_bit_codes(J, ctx, tmp_path, dri):
    """200 x 150 noise at quality 95 (130 MCUs of six blocks) with every code 16 bits long, so that every symbol takes the
    path behind the look-up table, at 64-bit subsequences.  Restart interval 1: 130 segments of one MCU each for the segment
    search, the segmented block scan and the DC prefix sums; interval 7 does not divide a row of 13 MCUs"""
    data, coef = _large_foreign(J, tmp_path, shape=('flat', 16), dri=dri, huff_per_component=True, table_ids=F.FOREIGN_IDS)
    images = _scan_images([data])
    assert images[0].desc.n_segments == -(-130 // dri) and images[0].desc.n_tables == 6
    assert all(set(bytes(images[0].desc.huff_counts[t])[:15]) == {0} for t in range(6))
    status, planes, coefs = _entropy_decode(ctx, images, 64)
    assert status[0] == 0
    np.testing.assert_array_equal(planes[0], coef)
    np.testing.assert_array_equal(planes[0], J.decode(data)[2])
    px, = _reconstruct(ctx, [images[0].coefficient_image()], coefs)
    np.testing.assert_array_equal(px, _load(data))
    assert ctx.jpeg_entropy_stats()['subsequences'] > 1000


def test_pillow_foreign_and_damaged_files_in_one_call(J, ctx, corpus, tmp_path):
    """Pillow files, foreign files and damaged foreign files (what mdjpeg_scan passes of them) mixed in ONE call: flagged
    exactly where mdjpeg_decode refuses, the clean neighbours exact, guards intact"""
    pillow = [open(JF.write_jpeg(str(tmp_path / 'c{}.jpg'.format(i)), JF.content('noise', 96, 64), s, 90, False, r), 'rb').read()
              for i, (s, r) in enumerate([('420', None), ('444', 'rows'), ('gray', 'blocks')])]
    by_name = {e[0]: e[1] for e in corpus}
    foreign = [by_name[k] for k in ('420_37x29_camera_a', '444_17x9_six031', '422_40x24_ladder', 'gray_33x31_camera_b', '420_1x1_flat16')]
    damaged = [data for _, data in damaged_foreign(corpus) if J.scan(data)[0] == 0]
    assert len(damaged) >= 20
    datas = []
    for i, d in enumerate(damaged):                            # a clean file in front, after every fourth damaged one, and last
        if i % 4 == 0:
            datas.append((pillow + foreign)[(i // 4) % 8])
        datas.append(d)
    datas += pillow[:1] + foreign[:1]
    from megadetector_amd.jpeg_host import ScanImage
    images = [ScanImage.from_bytes(d)[1] for d in datas]
    assert all(im is not None for im in images)
    want = [J.decode(d) for d in datas]
    assert sum(1 for rc, _, _ in want if rc != 0) >= 15 and sum(1 for rc, _, _ in want if rc == 0) >= 8
    for bits in (64, 0):
        status, planes, _ = _entropy_decode(ctx, images, bits)
        for i, ((rc, hd, coef), st, got) in enumerate(zip(want, status, planes)):
            assert (st != 0) == (rc != 0), (i, bits, int(st), rc, hd.reason)
            if rc == 0:
                np.testing.assert_array_equal(got, coef, err_msg=str(i))


@pytest.mark.parametrize('sampling', ['444', 'gray'])
def test_extreme_blocks_through_both_entry_points(J, ctx, sampling):
    """the extreme family -- spikes of +-400 .. 1028, single coefficients under 16-bit table values that de-quantise to
    1900 .. 2799 -- and the blocks beyond every energy bound.  Through mdhip_jpeg_entropy_decode: status != 0 exactly where
    mdjpeg_decode refuses, elsewhere the serialised planes and, behind mdhip_jpeg_reconstruct, Pillow's pixels.  Through
    mdhip_jpeg_reconstruct alone: the synthetic planes uploaded as they are, 16-bit tables included, give Pillow's pixels."""
    import torch
    from PIL import Image
    from megadetector_amd.jpeg_host import CoefficientImage
    family = [m for m in F.extreme_family() + F.extreme_family(singles=F.BEYOND, spikes=False) if m[0].startswith(sampling)]
    n_refused = n_equal = n_wide = 0
    for at in range(0, len(family), 64):
        batch = family[at:at + 64]
        datas = [F.foreign_file(header, coef, **knobs) for _, header, coef, _, _, knobs in batch]
        want = [J.decode(d) for d in datas]
        images = _scan_images(datas)
        status, planes, coefs = _entropy_decode(ctx, images, 64 if (at // 64) % 2 else 0)
        pils = [np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas]
        keep = [i for i, (rc, _, _) in enumerate(want) if rc == 0]
        for i, ((rc, hd, _), st) in enumerate(zip(want, status)):
            assert (st != 0) == (rc != 0), (batch[i][0], int(st), rc, hd.reason)
            if rc == 0:
                np.testing.assert_array_equal(planes[i], batch[i][2], err_msg=batch[i][0])
        n_refused += len(batch) - len(keep)
        if not keep:
            continue
        # the decoded planes, where they are
        pixels = _reconstruct(ctx, [images[i].coefficient_image() for i in keep], [coefs[i] for i in keep])
        for i, px in zip(keep, pixels):
            np.testing.assert_array_equal(px, pils[i], err_msg=batch[i][0] + ' (entropy decoded)')
        # the synthetic planes, uploaded
        cis = [CoefficientImage.from_header(batch[i][1], batch[i][2]) for i in keep]
        up = [torch.from_numpy(batch[i][2]).to('cuda:0') for i in keep]
        for i, px in zip(keep, _reconstruct(ctx, cis, up)):
            np.testing.assert_array_equal(px, pils[i], err_msg=batch[i][0] + ' (uploaded planes)')
            n_equal += 1
            n_wide += int(batch[i][1].quant.max()) > 255
    print('extreme blocks on the device, {}: {} files, {} flagged, {} equal to Pillow through both entry points, {} of them under 16-bit tables'.format(
        sampling, len(family), n_refused, n_equal, n_wide))
    assert n_refused == len(F.BEYOND) * (7 if sampling == '444' else 5) and n_equal == len(family) - n_refused
    assert n_wide >= 50
