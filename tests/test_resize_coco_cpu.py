"""
COCO dataset resizing without a GPU (megadetector_amd/resize_coco_dataset.py):

  * the host leg equals what the reference's own data_management/resize_coco_dataset.py wrote, returned or raised for every case
    of resize_scene.COCO_CASES (tests/golden/resize_reference.json: the JSON text as write_json wrote it, the output tree, the
    exception's type and text): 'copy' and 'rewrite', 'omit' and 'error' with a missing file, a file that does not open, a target
    that is not positive and the truncated file (which the reference loads), an image without annotations, an annotation
    without 'bbox', the command line;
  * the device leg's planning, run on the host models, gives the host leg's bytes for every image it takes, and leaves to the host
    leg the copies and the files named here;
  * the box scaling and the per-image decision on hand-written values.
"""

import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import jpeg_enc_sampled_ref as E
import resize_scene as S
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return S.load_golden(os.path.join(GOLDEN, 'resize_reference.json'))


@pytest.fixture(scope='module')
def exact(golden, tmp_path_factory):
    folder = str(tmp_path_factory.mktemp('scene'))
    S.build(folder)
    return S.is_exact(golden, folder)


@pytest.fixture(scope='module', autouse=True)
def _built():
    import __graft_entry__ as G
    G.build()


def run_case(tmp, name, **extra):
    from megadetector_amd import resize_coco_dataset as RC
    text = io.StringIO()
    with redirect_stdout(text):
        got = S.run_coco_case(str(tmp), name, RC.resize_coco_dataset, RC.main, **extra)
    return got, text.getvalue()


def compare_case(got, want, exact):
    assert got.get('error') == want.get('error')
    if 'error' in want:
        return
    assert got['json'] == want['json'] and got['returned_equal']
    S.compare_tree(got['tree'], want['tree'], exact)


def test_the_cases_cover_what_they_must(golden):
    assert sorted(golden['coco']) == sorted(S.COCO_CASES)
    errors = {k: v['error'] for k, v in golden['coco'].items() if 'error' in v}
    assert errors['error_missing'] == ['FileNotFoundError', 'Could not find file {IN}/missing.jpg']
    assert errors['error_open'][1].startswith('Could not open image palette.png: ')
    assert errors['error_resize'] == ['Exception', 'Could not resize image thin.jpg: Invalid image resize target 64,0']
    assert errors['bad_handling'] == ['ValueError', 'Unrecognized value link for correct_size_image_handling']
    assert 'error' not in golden['coco']['error_truncated']                 # the reference loads a file that ends early
    d = json.loads(golden['coco']['omit_width_64']['json'])
    names = [im['file_name'] for im in d['images']]
    assert len(names) == 13 and not {'missing.jpg', 'palette.png', 'thin.jpg'} & set(names) and 'truncated.jpg' in names
    ids = {im['id'] for im in d['images']}
    assert all(a['image_id'] in ids for a in d['annotations']) and any('bbox' not in a for a in d['annotations'])
    assert next(im for im in d['images'] if im['file_name'] == 'a444.jpg')['id'] not in {a['image_id'] for a in d['annotations']}
    assert next(im for im in d['images'] if im['file_name'] == 'rot6.jpg')['width'] == 64      # after the EXIF rotation: 64 x 96
    assert golden['coco']['omit_width_64']['json'].startswith('{\n "info": {\n  "version": "1"\n },\n "images": [\n  {\n')


@pytest.mark.parametrize('name', list(S.COCO_CASES))
def test_host_leg_equals_the_reference(tmp_path, golden, exact, name):
    counts = {}
    got, printed = run_case(tmp_path, name, backend='host', **({} if name == 'cli' else {'counts': counts}))
    compare_case(got, golden['coco'][name], exact)
    if name == 'omit_width_64':
        assert "Can't find image missing.jpg, skipping" in printed and "Can't open image palette.png, skipping" in printed
        assert "Can't resize image thin.jpg, skipping" in printed
        assert counts['files'] == 16 and counts['omitted'] == 3 and counts['host'] == 16 and counts['gpu'] == 0
    if name == 'cli':
        assert printed.endswith('Dataset resizing complete\n')
    if name == 'omit_copy_no_target':
        source = str(tmp_path / 'in')
        for rel in got['tree']:
            with open(os.path.join(source, rel), 'rb') as a, open(os.path.join(str(tmp_path / 'out'), rel), 'rb') as b:
                assert a.read() == b.read(), rel                            # 'copy' is a byte copy


def test_pools_and_in_place(tmp_path, golden, exact):
    from megadetector_amd import resize_coco_dataset as RC
    source = str(tmp_path / 'in')
    S.build(source)
    coco = str(tmp_path / 'coco.json')
    with open(coco, 'w') as f:
        json.dump(S.coco_dataset(), f)
    kw = dict(S.COCO_CASES['omit_width_64'])
    want = json.loads(golden['coco']['omit_width_64']['json'])
    with redirect_stdout(io.StringIO()):
        for k, (pool_type, n) in enumerate([('thread', 3), ('process', 2)]):
            assert RC.resize_coco_dataset(source, coco, str(tmp_path / 'o{}'.format(k)), None, n_workers=n, pool_type=pool_type, backend='host', **kw) == want
        with pytest.raises(AssertionError, match='Illegal pool type'):
            RC.resize_coco_dataset(source, coco, str(tmp_path / 'o9'), None, n_workers=2, pool_type='fibre', backend='host', **kw)
        with pytest.raises(AssertionError, match='Illegal unavailable_image_handling'):
            RC.resize_coco_dataset(source, coco, str(tmp_path / 'o9'), None, unavailable_image_handling='skip', backend='host')
        # the output folder is the input folder: images are overwritten, and a 'copy' onto itself copies nothing
        assert RC.resize_coco_dataset(source, coco, source, None, backend='host', **kw) == want
        before = S.describe_tree(source)
        RC.resize_coco_dataset(source, coco, source, None, unavailable_image_handling='omit', backend='host')
        assert S.describe_tree(source) == before


#: what the device leg leaves to the host leg whatever the case: files the GPU's decoder does not take, a file that is missing,
#: one that does not open; with a width of 64 the 300 x 2 file, whose height becomes 0
HOST_FILES = {'sub/prog.jpg', 'pic.png', 'palette.png', 'truncated.jpg', 'missing.jpg'}


@pytest.mark.parametrize('name', ['omit_width_64', 'omit_rewrite_equal', 'omit_rewrite_no_target', 'omit_no_enlarge_100', 'omit_copy_equal'])
def test_device_leg_planning_on_the_host_models_gives_the_host_leg_bytes(tmp_path, name):
    from megadetector_amd import jpeg_host, resize_coco_dataset as RC
    from megadetector_amd.feed import load_image
    kw = dict(S.COCO_CASES[name])
    got, _ = run_case(tmp_path, name, backend='host')
    source, out = str(tmp_path / 'in'), str(tmp_path / 'out')
    target, handling = kw.get('target_size', (-1, -1)), kw.get('correct_size_image_handling', 'copy')
    to_host, planned = set(), {}
    for im in S.coco_dataset()['images']:
        rel = im['file_name']
        job = {'input': os.path.join(source, rel), 'output': os.path.join(out, rel)}
        try:
            RC.plan_job(job, target, handling, kw.get('no_enlarge_width', True))
        except Exception:
            to_host.add(rel)
            continue
        pixels = np.ascontiguousarray(np.asarray(load_image(job['input'])))
        if job['size'] != job['source_size']:
            pixels = jpeg_host.resample_lanczos(pixels, job['size'])
        coef = E.coefficients(pixels, job['sampling'], *job['quant'])
        rc, scans, _, _ = jpeg_host.encode_subsequences([coef], [job['size']], 64, samplings=[job['sampling']])
        assert rc == jpeg_host.MDJPEG_OK
        data = jpeg_host.sampled_file(job['size'][0], job['size'][1], job['quant'][0], job['quant'][1], job['sampling'], scans[0], job['exif'],
                                      job['comment'])
        with open(job['output'], 'rb') as f:
            assert f.read() == data, rel
        planned[rel] = job
    written = {im['file_name']: im for im in json.loads(got['json'])['images']}
    assert all((written[rel]['width'], written[rel]['height']) == job['size'] for rel, job in planned.items())
    if name == 'omit_width_64':
        assert to_host == HOST_FILES | {'thin.jpg'} and sum(j['resized'] for j in planned.values()) == 7
        assert planned['rot6.jpg']['exif'] != planned['rot6.jpg']['exif'].replace(b'a camera trap', b'') and not planned['rot6.jpg']['resized']
    elif name == 'omit_copy_equal':
        # 96 x 64 is the size of 'sub/com.jpg', and no_enlarge_width makes every narrower image "already that size": copies
        # are the host leg's; the wider ones and 97 x 61 are resized
        assert to_host == HOST_FILES | {'sub/com.jpg', 'grey_l.jpg', 'grey_rgb.jpg', 'rot6.jpg', 'rot3.jpg', 'sub/rot8.jpg', 'sub/icc.jpg'}
        assert sorted(planned) == ['a444.jpg', 'dusk420.jpg', 'rst422.jpg', 'thin.jpg'] and all(j['resized'] for j in planned.values())
    elif name == 'omit_rewrite_equal':
        assert to_host == HOST_FILES and not planned['sub/com.jpg']['resized'] and planned['sub/com.jpg']['sampling'] == 1
    elif name == 'omit_rewrite_no_target':
        assert to_host == HOST_FILES and not any(j['resized'] for j in planned.values())
    else:
        # narrower than 100: written at their own size ('rewrite'); the wider ones resized to a width of 100, but for the
        # 300 x 2 file, whose height becomes 0
        assert to_host == HOST_FILES | {'thin.jpg'} and {r for r, j in planned.items() if j['resized']} == {'dusk420.jpg', 'rst422.jpg'}


def test_orientation_leaves_the_resized_file_only(tmp_path):
    """tags_to_exclude=('Orientation',) applies to the resized save; 'rewrite' keeps the tag (the reference's quirk)"""
    from PIL import Image
    got, _ = run_case(tmp_path / 'a', 'omit_width_64', backend='host')
    assert 274 not in Image.open(str(tmp_path / 'a' / 'out' / 'rot3.jpg')).getexif() and Image.open(str(tmp_path / 'a' / 'out' / 'rot3.jpg')).getexif()[271] == 'turned'
    got, _ = run_case(tmp_path / 'b', 'omit_rewrite_no_target', backend='host')
    assert Image.open(str(tmp_path / 'b' / 'out' / 'rot3.jpg')).getexif()[274] == 3


def test_box_scaling_and_decision():
    from megadetector_amd.resize_coco_dataset import correct_size, finish_image
    im, anns = finish_image({'id': 1}, [{'bbox': [10, 20, 30, 40]}, {'category_id': 0}], (163, 121), (64, 47))
    assert im == {'id': 1, 'width': 64, 'height': 47}
    assert anns[0]['bbox'] == [10 * (64 / 163), 20 * (47 / 121), 30 * (64 / 163), 40 * (47 / 121)] and 'bbox' not in anns[1]
    same = [1.5, 2, 3, 4]
    assert finish_image({}, [{'bbox': same}], (10, 10), (10, 10))[1][0]['bbox'] is same
    assert finish_image({}, [{'bbox': same}], (10, 10), (10, 5))[1][0]['bbox'] == [1.5, 1.0, 3.0, 2.0]
    assert correct_size((96, 64), (96, 64), False) and correct_size((96, 64), (-1, -1), False) and not correct_size((96, 64), (96, -1), False)
    assert correct_size((96, 64), (100, -1), True) and not correct_size((96, 64), (100, -1), False) and not correct_size((100, 64), (100, -1), True)
