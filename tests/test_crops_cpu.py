"""
Crop geometry, selection and naming (megadetector_amd/crops.py) against PIL and a restatement of the reference
(visualization_utils.crop_image, create_crop_folder.py:392-425 and :485-521).
"""

import copy
import os

import numpy as np
import pytest
from PIL import Image

from megadetector_amd import crops as K

W, H = 97, 61
IMG = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)

BOXES = [
    [0.1, 0.2, 0.3, 0.4],
    [10.5 / W, 20.5 / H, 30.0 / W, 11.0 / H],            # .5 coordinates: round half to even, both ways
    [11.5 / W, 21.5 / H, 30.0 / W, 11.0 / H],
    [0.5 / W, 1.5 / H, 2.0 / W, 3.0 / H],
    [0.0, 0.0, 1.0, 1.0],                                # reaching the border: clamped to width - 1 / height - 1
    [0.5, 0.5, 0.5, 0.5],
    [0.9, 0.9, 0.3, 0.3],                                # past the border
    [-0.1, -0.2, 0.5, 0.5],
    [0.3, 0.3, 0.0, 0.2],                                # no area
    [0.3, 0.3, 0.2, 0.0],
    [0.3, 0.3, 0.004, 0.004],                            # rounds to no area
    [1.2, 0.1, 0.1, 0.1],                                # outside: clamped to a line
]


def reference_crop(image, bbox, expansion):
    """visualization_utils.crop_image:464-486 for one detection"""
    x1, y1, w_box, h_box = bbox
    ymin, xmin, ymax, xmax = y1, x1, y1 + h_box, x1 + w_box
    im_width, im_height = image.size
    (left, right, top, bottom) = (xmin * im_width, xmax * im_width, ymin * im_height, ymax * im_height)
    if expansion > 0:
        left -= expansion
        right += expansion
        top -= expansion
        bottom += expansion
    left = max(left, 0); right = max(right, 0)
    top = max(top, 0); bottom = max(bottom, 0)
    left = min(left, im_width - 1); right = min(right, im_width - 1)
    top = min(top, im_height - 1); bottom = min(bottom, im_height - 1)
    return image.crop((left, top, right, bottom))


@pytest.mark.parametrize('expansion', [0, 1, 7, 200])
@pytest.mark.parametrize('bbox', BOXES, ids=lambda b: ','.join('{:.3f}'.format(v) for v in b))
def test_rectangle_equals_image_crop(bbox, expansion):
    pil = Image.fromarray(IMG)
    want = reference_crop(pil, bbox, expansion)
    r = K.crop_rectangle(bbox, W, H, expansion)
    if want.size[0] <= 0 or want.size[1] <= 0:
        assert r is None
        return
    x0, y0, x1, y1 = r
    assert (x1 - x0, y1 - y0) == want.size
    assert 0 <= x0 < x1 <= W - 1 and 0 <= y0 < y1 <= H - 1
    assert np.array_equal(IMG[y0:y1, x0:x1], np.asarray(want))


def test_matrix_holds_empty_and_clamped_rectangles():
    rects = [K.crop_rectangle(b, W, H, 0) for b in BOXES]
    assert sum(r is None for r in rects) >= 4
    assert K.crop_rectangle([0.0, 0.0, 1.0, 1.0], W, H, 0) == (0, 0, W - 1, H - 1)
    assert K.crop_rectangle(BOXES[1], W, H, 0)[:2] == (10, 20) and K.crop_rectangle(BOXES[2], W, H, 0)[:2] == (12, 22)
    assert K.crop_rectangle([0.3, 0.3, 0.0, 0.2], W, H, 5) is not None      # expansion gives a line an area


def reference_selection(images, confidence_threshold, category_ids_to_include):
    """create_crop_folder.py:392-425, the statements as they stand"""
    for im in images:
        if 'detections' not in im or im['detections'] is None or len(im['detections']) == 0:
            continue
        for i_detection, det in enumerate(im['detections']):
            if det['conf'] < confidence_threshold:
                continue
            if (category_ids_to_include is not None) and (det['category'] not in category_ids_to_include):
                continue
            if 'crop_id' not in det:
                det['crop_id'] = i_detection
            crop_id = det['crop_id']
            if isinstance(crop_id, int):
                crop_id = str(crop_id).zfill(3)
            name, ext = os.path.splitext(im['file'])
            det['crop_filename_relative'] = f'{name}.crop_{crop_id}{ext}'
    records = []
    for im in images:
        if 'detections' not in im or im['detections'] is None or len(im['detections']) == 0:
            continue
        for det in im['detections']:
            if 'crop_id' in det:
                records.append({'file': det['crop_filename_relative'],
                                'detections': [{'category': det['category'], 'conf': det['conf'], 'bbox': [0, 0, 1, 1],
                                                'crop_id': det['crop_id']}]})
    return records


def _results():
    rng = np.random.default_rng(4)
    images = []
    for i, name in enumerate(['a.jpg', 'sub/dir/b.JPG', 'c.png', 'no_extension', 'd.x.jpeg', 'failed.jpg', 'empty.jpg']):
        confs = sorted(rng.random(12).round(3).tolist(), reverse=True)
        dets = [{'category': str(1 + int(rng.integers(0, 3))), 'conf': c, 'bbox': rng.random(4).round(4).tolist()} for c in confs]
        images.append({'file': name, 'detections': dets})
    images[-2] = {'file': 'failed.jpg', 'failure': 'Failure image access', 'detections': None}
    images[-1]['detections'] = []
    images[0]['detections'][3]['conf'] = 0.1               # exactly at the threshold: kept
    return images


@pytest.mark.parametrize('names', [None, ['animal'], ['person', 'vehicle']])
@pytest.mark.parametrize('threshold', [0.1, 0.0, 0.5])
def test_ids_and_names_equal_the_reference_statements(threshold, names):
    cats = {'1': 'animal', '2': 'person', '3': 'vehicle'}
    opt = K.CropOptions(confidence_threshold=threshold, category_names_to_include=names)
    ids = K.category_ids_to_include(opt, cats)
    assert ids == (None if names is None else {k for k, v in cats.items() if v in names})
    want_images = _results()
    want_records = reference_selection(want_images, threshold, ids)
    got_images = _results()
    before = copy.deepcopy(got_images)
    got_records = K.annotate_results(got_images, opt, ids)
    assert got_images == want_images and got_records == want_records
    assert len(got_records) > 0 and got_images != before
    assert any(r['file'] == 'sub/dir/b.crop_000.JPG' for r in got_records) or threshold == 0.5 or names
    with pytest.raises(ValueError):
        K.category_ids_to_include(K.CropOptions(category_names_to_include=['bird']), cats)


def test_names_and_formats():
    assert K.crop_filename('a/b.c.jpg', 7) == 'a/b.c.crop_007.jpg'
    assert K.crop_filename('a/b', 1234) == 'a/b.crop_1234'
    assert K.crop_filename('x.png', 'k9') == 'x.crop_k9.png'
    assert all(K.is_jpeg_name(n) for n in ['a.jpg', 'A.JPG', 'b.jpeg', 'c.jpe', 'd.jfif'])
    assert not any(K.is_jpeg_name(n) for n in ['a.png', 'b.tif', 'c', 'd.jpg.bmp'])
    opt = K.CropOptions()
    assert (opt.confidence_threshold, opt.expansion, opt.quality, opt.category_names_to_include) == (0.1, 0, 95, None)
    with pytest.raises(ValueError, match='1 to 100'):
        K.CropOptions(quality=0)


def test_write_crops(tmp_path):
    paths = K.write_crops(str(tmp_path), [(0, 'a.crop_000.jpg', b'one'), (3, 'sub/b.crop_003.png', b'two')])
    assert [open(p, 'rb').read() for p in paths] == [b'one', b'two']
    assert paths[1].endswith('sub/b.crop_003.png')


# ---- the driver loop ------------------------------------------------------------------------------------------------
import io
import json

from stub_detector import StubDetector, write_test_images
from megadetector_amd import run_detector_batch as RDB
from megadetector_amd.feed import load_image

INFO = {'format_version': '1.6', 'detector': 'stub'}


class CroppingStub(StubDetector):
    """a detector with crops=: returns 'crops' as HIPDetector does (made on the host here), under names the driver replaces"""

    supports_crops = True

    def generate_detections_one_batch(self, imgs, names, crops=None, **kw):
        res = StubDetector.generate_detections_one_batch(self, imgs, names, **kw)
        if crops is not None:
            for r, im in zip(res, imgs):
                r['crops'] = K.crops_of_host_image(np.asarray(im), r['file'], r['detections'], crops, crops.category_ids(),
                                                   warn=lambda m: None)[0] if r.get('detections') is not None else []
        return res

    def generate_detections_one_image(self, img, name='unknown', detection_threshold=1e-5, crops=None, **kw):
        r = StubDetector.generate_detections_one_image(self, img, name, detection_threshold, **kw)
        if crops is not None:
            r['crops'] = K.crops_of_host_image(np.asarray(img), name, r['detections'], crops, crops.category_ids(), warn=lambda m: None)[0]
        return r


def _folder(tmp_path):
    folder = tmp_path / 'imgs'
    (folder / 'sub').mkdir(parents=True)
    files = write_test_images(str(folder))
    for i, f in enumerate(files[:6]):                    # some as JPEG, some in a sub-folder
        im = Image.open(f)
        new = str(folder / ('sub' if i % 2 else '.') / 'j{}.jpg'.format(i))
        im.save(new, quality=90)
        os.remove(f)
    return str(folder), RDB.find_images(str(folder), recursive=True)


def second_pass(final_output, folder, threshold=0.1, quality=95, expansion=0):
    """the reference's second pass over a results file: {crop name: bytes}"""
    want = {}
    for im in final_output['images']:
        for i, det in enumerate(im.get('detections') or []):
            if det['conf'] < threshold:
                continue
            crop = reference_crop(load_image(os.path.join(folder, im['file'])), det['bbox'], expansion)
            if crop.size[0] <= 0 or crop.size[1] <= 0:
                continue
            name, ext = os.path.splitext(im['file'])
            bio = io.BytesIO()
            crop.save(bio, format=Image.registered_extensions()[ext.lower()], quality=quality)
            want['{}.crop_{}{}'.format(name, str(i).zfill(3), ext)] = bio.getvalue()
    return want


def _tree(folder):
    out = {}
    for root, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(root, n)
            out[os.path.relpath(p, folder).replace('\\', '/')] = open(p, 'rb').read()
    return out


@pytest.mark.parametrize('mode', ['one_by_one', 'batched', 'queue'])
@pytest.mark.parametrize('stub', [StubDetector, CroppingStub])
def test_driver_writes_the_second_pass_and_leaves_the_results_alone(tmp_path, stub, mode):
    folder, files = _folder(tmp_path)
    kw = {'one_by_one': {}, 'batched': {'batch_size': 4}, 'queue': {'batch_size': 4, 'use_image_queue': True, 'loader_workers': 2}}[mode]
    plain = RDB.load_and_run_detector_batch('stub', files, detector=StubDetector(), quiet=True, confidence_threshold=0.05, **kw)
    crop_folder = str(tmp_path / 'crops')
    seen = []
    real_checkpoint = RDB.write_checkpoint

    def checking_checkpoint(path, results):
        """every result a checkpoint holds has its crops on disk already"""
        have = _tree(crop_folder) if os.path.isdir(crop_folder) else {}
        out = RDB.write_results_to_file(copy.deepcopy(results), str(tmp_path / 'ck_view.json'), relative_path_base=folder, info=dict(INFO))
        want = second_pass(out, folder)
        assert set(want) <= set(have), sorted(set(want) - set(have))[:3]
        seen.append(len(results))
        real_checkpoint(path, results)

    RDB.write_checkpoint = checking_checkpoint
    try:
        got = RDB.load_and_run_detector_batch('stub', files, detector=stub(), quiet=True, confidence_threshold=0.05,
                                              crop_folder=crop_folder, crop_base=folder, checkpoint_path=str(tmp_path / 'ck.json'),
                                              checkpoint_frequency=4, **kw)
    finally:
        RDB.write_checkpoint = real_checkpoint
    assert len(seen) >= 2
    assert all('crops' not in r for r in got)
    a = RDB.write_results_to_file(plain, str(tmp_path / 'a.json'), relative_path_base=folder, info=dict(INFO))
    b = RDB.write_results_to_file(got, str(tmp_path / 'b.json'), relative_path_base=folder, info=dict(INFO))
    assert open(str(tmp_path / 'a.json'), 'rb').read() == open(str(tmp_path / 'b.json'), 'rb').read()
    want = second_pass(b, folder)
    assert len(want) >= 10 and any(n.startswith('sub/') for n in want) and any(n.endswith('.png') for n in want)
    assert _tree(crop_folder) == want
    counts = RDB.last_crop_counts
    n_jpeg = sum(K.is_jpeg_name(n) for n in want)
    assert counts['files'] == len(want) and counts['host_other'] == len(want) - n_jpeg
    assert (counts['gpu'], counts['host_jpeg']) == ((n_jpeg, 0) if stub is CroppingStub else (0, n_jpeg))
    # the two extra files
    opt = K.CropOptions()
    RDB.write_crop_result_files(b, opt, folder, str(tmp_path / 'with_ids.json'), str(tmp_path / 'per_crop.json'))
    with_ids, per_crop = json.load(open(str(tmp_path / 'with_ids.json'))), json.load(open(str(tmp_path / 'per_crop.json')))
    ref = json.loads(json.dumps(b))
    ref_records = reference_selection(ref['images'], 0.1, None)
    assert with_ids == ref and per_crop['images'] == ref_records and per_crop['info'] == b['info']
    assert {r['file'] for r in ref_records} >= set(want)
    assert json.load(open(str(tmp_path / 'b.json'))) == b                    # the main results carry no crop fields


def test_resumed_run_leaves_no_gaps(tmp_path):
    folder, files = _folder(tmp_path)
    crop_folder = str(tmp_path / 'crops')
    kw = dict(detector=None, quiet=True, confidence_threshold=0.05, crop_folder=crop_folder, crop_base=folder, batch_size=4)
    kw['detector'] = StubDetector()
    first = RDB.load_and_run_detector_batch('stub', files[:5], **kw)
    kw['detector'] = StubDetector()
    full = RDB.load_and_run_detector_batch('stub', files, results=first, **kw)
    out = RDB.write_results_to_file(full, str(tmp_path / 'o.json'), relative_path_base=folder, info=dict(INFO))
    assert _tree(crop_folder) == second_pass(out, folder)


def test_cli_has_the_crop_flags(capsys):
    with pytest.raises(SystemExit):
        RDB.main(['--help'])
    text = capsys.readouterr().out
    for flag in ['--crop_folder', '--crop_confidence_threshold', '--crop_expansion', '--crop_quality', '--crop_categories',
                 '--crop_results_file', '--crops_output_file']:
        assert flag in text


def test_negative_box_is_skipped_where_pil_raises():
    """the stated deviation: Image.crop refuses a box whose right is left of its left; here it is a crop without area"""
    bad = [0.5, 0.2, -0.2, 0.3]
    with pytest.raises(ValueError):
        reference_crop(Image.fromarray(IMG), bad, 0)
    assert K.crop_rectangle(bad, W, H, 0) is None
