"""
Classification in the same pass, on the host: the rules of megadetector_amd/classify.py against PIL itself, the host model of
the GPU kernel (mdjpeg_classifier_input: the statements of csrc/resample.h the lanes run) against PIL and numpy bit for bit,
the classification lists, and the batch driver with a stub detector.
"""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

from conftest import REPO
from megadetector_amd import classify as K
from megadetector_amd import jpeg_host as J

# (src_w, src_h, canvas_w, canvas_h, off_x, off_y, S): the shapes of the GPU test -- reduce, enlarge, one column, odd sizes,
# more than one strip of 64 columns, an unchanged size, 224, a wide canvas, zeros on each side and on two sides at once
SHAPES = [(97, 61, 97, 61, 0, 0, 32), (5, 7, 5, 7, 0, 0, 32), (1, 9, 1, 9, 0, 0, 32), (301, 187, 301, 187, 0, 0, 32),
          (333, 500, 333, 500, 0, 0, 80), (80, 200, 80, 200, 0, 0, 80), (640, 480, 640, 480, 0, 0, 224), (1300, 40, 1300, 40, 0, 0, 32),
          (40, 30, 50, 30, 10, 0, 32), (40, 30, 50, 30, 0, 0, 32), (40, 30, 40, 50, 0, 20, 32), (40, 30, 40, 50, 0, 0, 32),
          (21, 17, 60, 60, 20, 30, 32), (13, 20, 20, 20, 4, 0, 32), (30, 15, 30, 30, 0, 8, 32)]


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def options(size=224, **kw):
    return K.ClassifyOptions(model=torch.nn.Identity(), image_size=size, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the crop ----------------------------------------------------------------------------------------------------------------

def save_crop_with_pil(img, bbox_norm, square_crop):
    """crop_detections.py:422-449 with PIL's own calls -> the crop as an image, or None"""
    img_w, img_h = img.size
    xmin, ymin = int(bbox_norm[0] * img_w), int(bbox_norm[1] * img_h)
    box_w, box_h = int(bbox_norm[2] * img_w), int(bbox_norm[3] * img_h)
    if square_crop:
        box_size = max(box_w, box_h)
        xmin = max(0, min(xmin - int((box_size - box_w) / 2), img_w - box_w))
        ymin = max(0, min(ymin - int((box_size - box_h) / 2), img_h - box_h))
        box_w, box_h = min(img_w, box_size), min(img_h, box_size)
    if box_w == 0 or box_h == 0:
        return None
    crop = img.crop(box=[xmin, ymin, xmin + box_w, ymin + box_h])
    if square_crop and (box_w != box_h):
        crop = ImageOps.pad(crop, size=(box_size, box_size), color=0)
    return crop


def index_coded(w, h):
    """pixel (x, y) holds 1 + its index in 24 bits: no image pixel is 0, and every pixel names its place"""
    i = np.arange(1, w * h + 1, dtype=np.uint32).reshape(h, w)
    return np.stack([i & 255, (i >> 8) & 255, (i >> 16) & 255], axis=2).astype(np.uint8)


BOXES = [[0.2, 0.3, 0.3, 0.2], [0.0, 0.0, 0.4, 0.2], [0.7, 0.1, 0.3, 0.25], [0.1, 0.8, 0.5, 0.2], [0.0, 0.3, 0.1, 0.6],   # inside, each edge
         [0.1, 0.0, 0.8, 1.0], [0.0, 0.05, 1.0, 0.9], [0.05, 0.1, 0.9, 0.85],      # larger than the short side: zeros and padding
         [0.3, 0.3, 0.001, 0.4], [0.3, 0.3, 0.4, 0.0], [0.3, 0.3, 0.001, 0.001],   # box_w = 0, box_h = 0, both (no crop when squared either)
         [0.9, 0.9, 0.3, 0.3], [0.5, 0.2, 0.13, 0.41], [0.333, 0.667, 0.3, 0.31], [0.0, 0.0, 1.0, 1.0]]


@pytest.mark.parametrize('square', [True, False])
@pytest.mark.parametrize('size', [(60, 40), (40, 60), (97, 61), (30, 30)])
def test_crop_canvas_is_what_pil_cuts_and_pads(size, square):
    w, h = size
    pixels = index_coded(w, h)
    img = Image.fromarray(pixels)
    seen = set()
    for bbox in BOXES:
        want = save_crop_with_pil(img, bbox, square)
        canvas = K.crop_canvas(bbox, w, h, square)
        if want is None:
            assert canvas is None, bbox
            seen.add('none')
            continue
        got = K.canvas_pixels(pixels, canvas)
        np.testing.assert_array_equal(got, np.asarray(want), err_msg=str(bbox))
        cw, ch, ox, oy, rect = canvas
        zeros = (got.reshape(-1, 3).max(axis=1) == 0).sum()
        assert zeros == cw * ch - (rect[2] - rect[0]) * (rect[3] - rect[1])
        seen.add('zeros' if zeros else 'full')
        seen.add('padded' if square and (ox or oy) else 'plain')
    # (the square around a box never leaves a square image, so such an image gets neither zeros nor padding)
    assert 'none' in seen and 'full' in seen and (square and w == h or 'zeros' in seen) and (not square or w == h or 'padded' in seen)


def test_pad_offsets_are_those_the_issue_pins():
    """13 in 20 gives 4, 15 in 30 gives 8 (ImageOps.pad: round((size - side) * 0.5), Python's round)"""
    for side, size, off in [(13, 20, 4), (15, 30, 8)]:
        p = np.asarray(ImageOps.pad(Image.fromarray(np.full((size, side, 3), 9, np.uint8)), size=(size, size), color=0))
        assert int(np.argmax(p[0, :, 0] > 0)) == off
    assert K.crop_canvas([0.0, 0.0, 13 / 20 + 1e-9, 1.0], 13, 20, True)[:4] == (20, 20, 4, 0)


# ---- the transform -----------------------------------------------------------------------------------------------------------

def test_host_leg_is_resize_center_crop_to_tensor_normalize():
    """classifier_input_host against the steps written out with PIL and torch ([3P] Resize, CenterCrop, ToTensor, Normalize)"""
    for w, h, size in [(97, 61, 32), (61, 97, 32), (50, 50, 32), (33, 100, 32), (32, 45, 32)]:
        a = noise(w, h, w)
        img = Image.fromarray(a)
        short, long = (w, h) if w <= h else (h, w)
        new = (size, int(size * long / short)) if w <= h else (int(size * long / short), size)
        img = img.resize(new, Image.BICUBIC) if new != (w, h) else img
        top, left = int(round((img.height - size) / 2.0)), int(round((img.width - size) / 2.0))
        img = img.crop((left, top, left + size, top + size))
        t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).to(torch.float32).div(255)
        t.sub_(torch.tensor(K.IMAGENET_MEAN)[:, None, None]).div_(torch.tensor(K.IMAGENET_STD)[:, None, None])
        got = K.classifier_input_host(a, (w, h, 0, 0, (0, 0, w, h)), options(size))
        assert got.shape == (3, size, size) and got.dtype == np.float32
        assert int((bits(got) != bits(t.numpy())).sum()) == 0


@pytest.mark.parametrize('interpolation', ['bicubic', 'bilinear', 'lanczos'])
def test_host_model_of_the_kernel_equals_pil_bit_for_bit(interpolation):
    for k, (sw, sh, cw, ch, ox, oy, size) in enumerate(SHAPES):
        opt = options(size, interpolation=interpolation)
        wide = noise(sw + 3, sh, 100 + k)
        a = wide[:, 1:1 + sw]                                        # rows 9 bytes longer than the pixels, an odd first byte
        want = K.classifier_input_host(a, (cw, ch, ox, oy, (0, 0, sw, sh)), opt)
        got = J.classifier_input(a, (cw, ch, ox, oy), size, opt.filter, opt.mean, opt.std)
        diff = int((bits(got) != bits(want)).sum())
        assert diff == 0, '{}x{} in {}x{} at {}: {} values differ'.format(sw, sh, cw, ch, size, diff)


def test_other_mean_and_std_and_the_arguments_the_model_refuses():
    a = noise(40, 30, 5)
    opt = options(16, mean=(0.5, 0.25, 0.0), std=(0.5, 1.0, 2.0))
    want = K.classifier_input_host(a, (40, 30, 0, 0, (0, 0, 40, 30)), opt)
    assert int((bits(J.classifier_input(a, (40, 30, 0, 0), 16, 0, opt.mean, opt.std)) != bits(want)).sum()) == 0
    for canvas, size, filt, std in [((39, 30, 0, 0), 16, 0, opt.std), ((50, 30, 11, 0), 16, 0, opt.std), ((40, 30, 0, 0), 0, 0, opt.std),
                                    ((40, 30, 0, 0), 16, 7, opt.std), ((40, 30, 0, 0), 16, 0, (1.0, 0.0, 1.0)), ((40, 30, -1, 0), 16, 0, opt.std)]:
        with pytest.raises(ValueError, match='returned -1'):
            J.classifier_input(a, canvas, size, filt, opt.mean, std)


def test_plan_follows_the_reduction():
    """the tile shrinks as the reduction grows, and the sizes the device refuses are those without a plan"""
    assert J.classifier_plan(640, 480, 224) == (64, 32)
    big = J.classifier_plan(6000, 6000, 224)
    assert big is not None and big[0] * big[1] < 64 * 32
    assert J.classifier_plan(65535, 65535, 8, K.FILTERS['lanczos']) is None
    assert J.classifier_plan(65535, 65535, 8, K.FILTERS['lanczos'], lds_bytes=1 << 22) is not None
    assert J.classifier_plan(640, 480, 224, lds_bytes=64) == (2, 1) and J.classifier_plan(640, 480, 224, lds_bytes=20) is None


def test_lanczos_tables_of_the_previews_are_unchanged():
    """md_resample_coeffs now forwards to the filter form: mdjpeg_resample must still be Pillow's LANCZOS"""
    for (w, h), size in [((97, 61), (40, 25)), ((50, 40), (120, 96))]:
        a = noise(w, h, 3)
        np.testing.assert_array_equal(J.resample_lanczos(a, size), np.asarray(Image.fromarray(a).resize(size, Image.LANCZOS)))


# ---- the list ----------------------------------------------------------------------------------------------------------------

def test_classification_list_threshold_rounding_order_and_ties():
    p = np.array([0.30004, 0.09999, 0.1, 0.30001, 0.19996, 0.00001], np.float32)
    assert K.classification_list(p, 0.1) == [['0', 0.3], ['3', 0.3], ['4', 0.2], ['2', 0.1]]      # ties keep the class order
    assert K.classification_list(p, 0.0)[-1] == ['5', 0.0]
    assert K.classification_list(np.array([0.25, 0.75], np.float32), 0.5) == [['1', 0.75]]
    # the value is the shortest decimal of the fp32 probability, not its double: 0.7f is below 0.7 as a double
    assert float(np.float32(0.7)) < 0.7 and K.classification_list(np.array([0.7, 0.3], np.float32), 0.7) == [['0', 0.7]]
    # the order is that of the ROUNDED values: the larger probability does not come first when both round to the same
    assert K.classification_list(np.array([0.12345, 0.12355], np.float32), 0.1) == [['0', 0.1235], ['1', 0.1235]]
    assert K.load_categories(None, 3) == {'0': '0', '1': '1', '2': '2'}
    assert K.load_categories({'1': 'b', '0': 'a'}) == {'0': 'a', '1': 'b'}


# ---- the driver ----------------------------------------------------------------------------------------------------------------

class TinyClassifier(torch.nn.Module):
    def __init__(self, classes=5):
        super().__init__()
        torch.manual_seed(11)
        self.pool, self.flat, self.fc = torch.nn.AdaptiveAvgPool2d(4), torch.nn.Flatten(), torch.nn.Linear(48, classes)

    def forward(self, x):
        return self.fc(self.flat(self.pool(x)))


def _validate_classified(d):
    """validate_batch_results.py:165-177, 230-248 restated"""
    assert 'classifier' in d['info'] and 'classification_completion_time' in d['info']
    for k, v in d['classification_categories'].items():
        assert isinstance(k, str) and str(int(k)) == k and isinstance(v, str)
    n = 0
    for im in d['images']:
        for det in im.get('detections') or []:
            for c in det.get('classifications') or []:
                assert isinstance(c[0], str) and c[0] in d['classification_categories']
                assert isinstance(c[1], float) and 0 <= c[1] <= 1
                n += 1
    return n


def test_batch_driver_with_a_stub_detector(tmp_path):
    from megadetector_amd import run_detector_batch as RDB
    from stub_detector import StubDetector, write_test_images
    folder = tmp_path / 'images'
    folder.mkdir()
    files = [os.path.join(str(folder), n) for n in write_test_images(str(folder))]
    cats = tmp_path / 'cats.json'
    cats.write_text(json.dumps({str(i): 'species {}'.format(i) for i in range(5)}))
    script = str(tmp_path / 'tiny.pt')
    torch.jit.script(TinyClassifier()).save(script)

    def run(out, **kw):
        res = RDB.load_and_run_detector_batch('stub', files, detector=StubDetector(), quiet=True, confidence_threshold=0.05,
                                              checkpoint_path=str(tmp_path / (out + '.ck')), checkpoint_frequency=4, batch_size=4, **kw)
        return res, RDB.write_results_to_file(res, str(tmp_path / out), relative_path_base=str(folder), detector_file='stub',
                                              info={'format_version': '1.4'})
    _, plain = run('plain.json')
    opt = K.ClassifyOptions(script, categories=str(cats), image_size=16, confidence_threshold=0.2, classification_threshold=0.15,
                            category_names_to_include=['animal', 'person'])
    res, final = run('with.json', classify_options=opt)
    assert (tmp_path / 'plain.json').read_bytes() == (tmp_path / 'with.json').read_bytes()
    assert (tmp_path / 'plain.json.ck').read_bytes() == (tmp_path / 'with.json.ck').read_bytes()
    assert not any('classifications' in r for r in res)
    counts = dict(RDB.last_classify_counts)
    assert counts['gpu'] == 0 and counts['host'] > 3 and counts['files'] == 0
    classified = RDB.write_classified_results(final, RDB.last_classifications, opt, str(tmp_path / 'c.json'), str(folder))
    assert json.loads((tmp_path / 'c.json').read_text()) == classified
    assert _validate_classified(classified) > 3
    assert classified['classification_categories']['4'] == 'species 4' and classified['info']['classifier'] == 'tiny.pt'
    # every detection the options select, and no other, has a list; the list is the model's on the reference's crop
    model, n = TinyClassifier().eval(), 0
    ids = opt.category_ids()
    for im, before in zip(classified['images'], plain['images']):
        pixels = np.asarray(Image.open(os.path.join(str(folder), im['file'])).convert('RGB'))
        assert [{k: v for k, v in d.items() if k != 'classifications'} for d in im['detections']] == before['detections']
        for det in im['detections']:
            crop = save_crop_with_pil(Image.fromarray(pixels), det['bbox'], True)
            selected = det['conf'] >= 0.2 and det['category'] in ids and crop is not None
            assert ('classifications' in det) == selected
            if not selected:
                continue
            x = K.classifier_input_host(np.asarray(crop), (crop.width, crop.height, 0, 0, (0, 0, crop.width, crop.height)), opt)
            with torch.no_grad():
                p = torch.softmax(model(torch.from_numpy(x)[None]), dim=1)[0].numpy()
            assert det['classifications'] == K.classification_list(p, 0.15)
            n += 1
    assert n == counts['host']
    # the sub-options need the switch
    with pytest.raises(AssertionError, match='need --classifier'):
        RDB.main(['stub', str(folder), str(tmp_path / 'x.json'), '--classifier_image_size', '64'])


# ---- sanitizers ----------------------------------------------------------------------------------------------------------------

def test_host_model_under_sanitizers(tmp_path):
    """mdjpeg_classifier_input in a stand-alone build of image_host.cpp with AddressSanitizer + UBSan (host code; `make
    asan-jpeg`, the --classify mode of host_asan_main.cpp): sources of their exact sizes at every alignment, outputs of exactly 3 S S floats, tiles
    of exactly the planned size -- any access outside them, and any undefined arithmetic, ends the run"""
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'jpeg_entropy_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-jpeg', 'ASAN_OUT=' + exe])
    r = subprocess.run([exe, '--classify'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'classify: 42 runs' in r.stdout
