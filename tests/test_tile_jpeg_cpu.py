"""
The JPEG round trip of tiled inference (run_tiled_inference tile_jpeg_quality, mdhip_jpeg_recompress), host side.

tests/jpeg_enc_ref.py restates the lossy half of libjpeg's encoder in NumPy; here it is pinned against Pillow, exactly:
for every quality x size x content below
  1. the quantisation tables of jpeg_host.quant_tables are those of the file Pillow wrote (Image.quantization);
  2. the quantised coefficients of the restatement are those the repository's entropy decoder (libmdjpeg.so) reads out
     of Pillow's file -- all three components, every block, the blocks that only fill up an MCU included;
  3. recompress(rgb, q) is what Pillow decodes from that file.
Crops of the bundled images come from the image repeated periodically, so that every size can be cut out of every image.

Then the driver: the quality range, the checkpoint rules, and that the keyword reaches the detector only when set.
"""

import io
import json
import os

import numpy as np
import pytest
from PIL import Image

from stub_detector import StubDetector
import jpeg_enc_ref as E
from megadetector_amd import jpeg_host
from megadetector_amd import run_tiled_inference as T

HERE = os.path.dirname(os.path.abspath(__file__))
BUNDLED = os.path.join(HERE, 'golden', 'bundled_images')
BUNDLED_NAMES = sorted(n for n in os.listdir(BUNDLED) if os.path.isfile(os.path.join(BUNDLED, n)))

QUALITIES = [95, 100, 90, 75, 30]
SIZES = [(1280, 1280), (640, 640), (16, 16), (8, 8), (100, 75), (17, 33), (33, 17), (1, 1), (1283, 641)]      # w x h
CONTENTS = ['noise', 'gradient', 'black', 'white', 'red', 'green', 'blue', 'checkerboard'] + \
           ['crop:' + n for n in BUNDLED_NAMES]
_CONSTANT = {'black': (0, 0, 0), 'white': (255, 255, 255), 'red': (255, 0, 0), 'green': (0, 255, 0), 'blue': (0, 0, 255)}
_BUNDLED = {}


def make_content(kind, w, h, seed=0):
    """the test images, also used by tests/test_gpu_tile_jpeg.py"""
    if kind == 'noise':
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'gradient':
        return np.stack([xx * 255 // max(1, w - 1), yy * 255 // max(1, h - 1), (xx + yy) * 255 // max(1, w + h - 2)],
                        axis=-1).astype(np.uint8)
    if kind in _CONSTANT:
        return np.broadcast_to(np.array(_CONSTANT[kind], dtype=np.uint8), (h, w, 3)).copy()
    if kind == 'checkerboard':                            # saturated, one pixel per field: drives the IDCT past 0 .. 255
        m = ((xx + yy) & 1).astype(np.uint8)
        return np.stack([m * 255, (1 - m) * 255, m * 255], axis=-1).astype(np.uint8)
    assert kind.startswith('crop:')
    name = kind[5:]
    if name not in _BUNDLED:
        _BUNDLED[name] = np.asarray(Image.open(os.path.join(BUNDLED, name)).convert('RGB'))
    a = _BUNDLED[name]
    x0, y0 = (7 + 13 * seed) % a.shape[1], (5 + 11 * seed) % a.shape[0]
    a = np.tile(a, (-(-(y0 + h) // a.shape[0]), -(-(x0 + w) // a.shape[1]), 1))
    return np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])


def pillow_file(rgb, quality):
    bio = io.BytesIO()
    Image.fromarray(rgb).save(bio, format='JPEG', quality=quality)
    return bio.getvalue()


def test_the_case_matrix_is_complete():
    assert len(BUNDLED_NAMES) >= 5 and len(CONTENTS) == 8 + len(BUNDLED_NAMES)


@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '{}x{}'.format(*s))
@pytest.mark.parametrize('quality', QUALITIES)
def test_encoder_restatement_equals_pillow(quality, size, content):
    w, h = size
    rgb = make_content(content, w, h, seed=quality)
    data = pillow_file(rgb, quality)
    im = Image.open(io.BytesIO(data))
    enc = E.encode(rgb, quality)
    # 1. tables
    ql, qc = jpeg_host.quant_tables(quality)
    assert ql.dtype == np.uint16 and ql.shape == (64,) and qc.shape == (64,)
    assert sorted(im.quantization) == [0, 1]
    assert list(im.quantization[0]) == ql.tolist() and list(im.quantization[1]) == qc.tolist()
    # 2. coefficients, padding blocks included
    rc, header, coef = jpeg_host.decode(data)
    assert rc == jpeg_host.MDJPEG_OK, header.reason
    assert header.components == 3 and header.h_samp == (2, 1, 1) and header.v_samp == (2, 1, 1)
    assert np.array_equal(header.quant, enc.quant)
    assert header.blocks_w == enc.blocks_w and header.blocks_h == enc.blocks_h
    for c, (got, want) in enumerate(zip(enc.planes(), header.planes(coef))):
        assert got.shape == want.shape
        bad = np.argwhere(got != want)
        assert len(bad) == 0, 'component {}: {} coefficients differ, first at [by, bx, k] = {}'.format(c, len(bad), bad[0])
    # 3. pixels
    want = np.asarray(im.convert('RGB'))
    got = E.recompress(rgb, quality)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), '{} bytes differ'.format(int((got != want).sum()))


@pytest.mark.parametrize('quality', [1, 2, 10, 49, 50, 51, 99])
def test_quant_tables_of_other_qualities(quality):
    im = Image.open(io.BytesIO(pillow_file(make_content('noise', 24, 24), quality)))
    ql, qc = jpeg_host.quant_tables(quality)
    assert list(im.quantization[0]) == ql.tolist() and list(im.quantization[1]) == qc.tolist()
    assert ql.min() >= 1 and qc.max() <= 255


# ---- the driver -----------------------------------------------------------------------------------------------------
class RecordingStub(StubDetector):
    """the stub detector with the tile method; keeps the keywords of every call"""

    def __init__(self):
        StubDetector.__init__(self)
        self.calls = []

    def generate_detections_for_tiles(self, image, origins, size, tile_ids=None, **kw):
        self.calls.append(kw)
        a = np.asarray(image)
        return [self._one(a[y:y + size[1], x:x + size[0]], n) for (x, y), n in zip(origins, tile_ids)]


def _folder(tmp_path, n=3):
    folder = str(tmp_path / 'imgs')
    os.makedirs(folder)
    for i in range(n):
        Image.fromarray(make_content('noise', 40, 30, seed=i)).save(os.path.join(folder, '{}.png'.format(i)))
    return folder


def _run(folder, out, det, **kw):
    return T.run_tiled_inference('md_v5a.0.0.pt', folder, None, str(out), tile_size_x=16, tile_size_y=12, detector=det,
                                 loader_workers=0, **kw)


@pytest.mark.parametrize('bad', [0, 101, -1, 95.0, '95', True])
def test_quality_outside_1_to_100_is_a_value_error(tmp_path, bad):
    with pytest.raises(ValueError, match='1 to 100'):
        jpeg_host.quant_tables(bad)
    det = RecordingStub()
    with pytest.raises(ValueError, match='1 to 100'):
        _run(_folder(tmp_path), tmp_path / 'o.json', det, tile_jpeg_quality=bad)
    assert det.calls == []


def test_cli_has_the_flag_and_names_the_reference_value(capsys):
    with pytest.raises(SystemExit):
        T.main(['--help'])
    text = capsys.readouterr().out
    assert '--tile_jpeg_quality' in text and '95' in text.split('--tile_jpeg_quality', 1)[1]


def test_keyword_reaches_the_detector_only_when_set(tmp_path):
    folder = _folder(tmp_path)
    off, on = RecordingStub(), RecordingStub()
    a = _run(folder, tmp_path / 'a.json', off)
    b = _run(folder, tmp_path / 'b.json', on, tile_jpeg_quality=95)
    assert len(off.calls) == 3 and all('jpeg_quality' not in kw for kw in off.calls)
    assert len(on.calls) == 3 and all(kw.get('jpeg_quality') == 95 for kw in on.calls)
    assert a['images'] == b['images']                    # (the stub ignores the keyword; the output format is the same)


def test_checkpoint_records_carry_the_setting_and_settings_are_not_mixed(tmp_path):
    folder = _folder(tmp_path)
    first = str(tmp_path / 'first.json')
    with open(first, 'w') as f:
        json.dump(['0.png', '1.png'], f)
    ck_on, ck_off = str(tmp_path / 'on.json'), str(tmp_path / 'off.json')
    _run(folder, tmp_path / 'p1.json', RecordingStub(), image_list=first, checkpoint_path=ck_on, checkpoint_frequency=1,
         tile_jpeg_quality=95)
    _run(folder, tmp_path / 'p2.json', RecordingStub(), image_list=first, checkpoint_path=ck_off, checkpoint_frequency=1)
    on = json.load(open(ck_on))['checkpoint']
    off = json.load(open(ck_off))['checkpoint']
    assert len(on) == 2 and all(r['tile_jpeg_quality'] == 95 for r in on)
    assert len(off) == 2 and all(set(r) == {'file', 'size', 'tiles'} for r in off)      # switch off: today's records
    assert [{k: v for k, v in r.items() if k != 'tile_jpeg_quality'} for r in on] == off
    # resuming with the same setting works and runs only what is left
    det = RecordingStub()
    _run(folder, tmp_path / 'full.json', det, checkpoint_path=ck_on, checkpoint_frequency=1, tile_jpeg_quality=95)
    assert len(det.calls) == 1
    det = RecordingStub()
    _run(folder, tmp_path / 'full_off.json', det, checkpoint_path=ck_off, checkpoint_frequency=1)
    assert len(det.calls) == 1
    # any other pairing is refused before the detector runs
    for ck, kw in ((ck_on, {}), (ck_on, {'tile_jpeg_quality': 90}), (ck_off, {'tile_jpeg_quality': 95})):
        det = RecordingStub()
        with pytest.raises(ValueError, match='tile_jpeg_quality'):
            _run(folder, tmp_path / 'x.json', det, checkpoint_path=ck, checkpoint_frequency=1, **kw)
        assert det.calls == []
