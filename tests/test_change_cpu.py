"""Change detection without a GPU: the host model (mdjpeg_change_detect) against an independent numpy / scipy restatement
(tests/change_ref.py) stage by stage and bit for bit; its labelling on masks dilation never makes; the tool
(megadetector_amd/change_detection.py, backend='host') against tests/golden/change_reference.json, which
tests/golden/gen_change_reference.py wrote from the reference's own module run with a stand-in cv2; refusals, the CLI's
defaults, the preview sampling, and the host model under AddressSanitizer + UBSan (`make asan-change`)."""

import json
import os
import subprocess

import numpy as np
import pytest

import change_ref as R
from conftest import REPO
from megadetector_amd import change_detection as CD
from megadetector_amd import jpeg_host

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'change_reference.json')

#: (height, width, keyword arguments of change_ref.pipeline): the issue's sizes and options
STAGE_CASES = [
    (131, 97, dict(min_area=0)),
    (97, 131, dict(min_area=500)),
    (40, 5, dict(blur_kernel_size=21, min_area=0)),                       # the reflection repeats along x
    (5, 40, dict(blur_kernel_size=21, min_area=0, dilate_iterations=0)),  # ... and along y
    (1, 1, dict(min_area=0)),
    (131, 97, dict(dilate_kernel_size=4, min_area=0)),                    # an even square
    (131, 97, dict(dilate_iterations=0, min_area=0, blur_kernel_size=5)),
    (131, 97, dict(ignore_fraction=-0.3, min_area=0)),
    (131, 97, dict(ignore_fraction=0.25, min_area=500)),
    (131, 97, dict(ignore_fraction=1.0, min_area=0)),
    (131, 97, dict(threshold_type='otsu', min_area=0, blur_kernel_size=7)),
    (131, 97, dict(threshold_type='otsu', min_area=0, blur_kernel_size=1, dilate_iterations=0, scene='two_level')),
    (64, 48, dict(threshold_type='otsu', min_area=0, scene='constant')),
    (90, 70, dict(blur_kernel_size=9, dilate_kernel_size=33, dilate_iterations=3, min_area=0)),
]


def stage_pair(h, w, scene=None):
    """previous and current image: a gradient with planted rectangles; 'two_level': a flat scene where one rectangle changes by
    one amount; 'constant': every pixel changes by the same amount"""
    if scene == 'two_level':
        base = R.background(h, w, 'flat')
        return base, R.planted(base, [(w // 4, h // 4, w // 3, h // 3, (190, 220, 160))])
    if scene == 'constant':
        return np.full((h, w, 3), 40, np.uint8), np.full((h, w, 3), 47, np.uint8)
    base = R.background(h, w)
    prev = R.planted(base, [(w // 5, h // 5, max(1, w // 3), max(1, h // 3), (250, 20, 30))])
    curr = R.planted(base, [(w // 2, h // 2, max(1, w // 4), max(1, h // 4), (10, 240, 200)), (0, 0, min(3, w), min(2, h), (255, 255, 255)),
                            (max(0, w - 4), max(0, h - 9), min(4, w), min(3, h), (0, 0, 0))])
    return prev, curr


def record_of(kw, cap=64):
    return jpeg_host.change_options(kw.get('blur_kernel_size', 21), 1 if kw.get('threshold_type') == 'otsu' else 0, kw.get('thr', 25),
                                    kw.get('dilate_kernel_size', 5), kw.get('dilate_iterations', 2), kw.get('min_area', 500),
                                    kw.get('ignore_fraction'), cap)


def regions_of(res, p=0):
    return [tuple(int(v) for v in r) for r in res['regions'][p][:int(res['n_regions'][p])]]


@pytest.mark.parametrize('h,w,kw', STAGE_CASES, ids=lambda v: None if isinstance(v, int) else '-'.join('{}{}'.format(k[:4], x) for k, x in v.items()))
def test_host_model_equals_the_restatement_stage_by_stage(h, w, kw):
    kw = dict(kw)
    prev, curr = stage_pair(h, w, kw.pop('scene', None))
    want = R.pipeline(prev, curr, **kw)
    got = jpeg_host.change_detect([prev, curr], [(0, 1)], record_of(kw), want_masks=True)
    np.testing.assert_array_equal(got['blurred'][0], want['blurred'][0])
    np.testing.assert_array_equal(got['blurred'][1], want['blurred'][1])
    assert int(got['counts'][0]) == want['count']
    np.testing.assert_array_equal(got['masks'][0], want['dilated'])
    assert not got['overflow'][0] and regions_of(got) == want['regions']
    if kw.get('threshold_type') != 'otsu':
        assert not got['hist'].any() and got['thresholds'][0] == 25
    else:
        diff = np.abs(want['blurred'][0].astype(int) - want['blurred'][1].astype(int))
        np.testing.assert_array_equal(got['hist'][0], np.bincount(diff.ravel(), minlength=256))


def test_the_stage_cases_are_not_trivial():
    """the scenes change something and the options bite: regions exist, min_area 500 drops some, the region of interest changes
    the count, Otsu on a constant difference chooses 0"""
    prev, curr = stage_pair(131, 97)
    all_regions = R.pipeline(prev, curr, min_area=0)['regions']
    assert len(all_regions) >= 2 and len(R.pipeline(prev, curr, min_area=500)['regions']) < len(all_regions)
    assert R.pipeline(prev, curr, min_area=0, ignore_fraction=-0.3)['count'] < R.pipeline(prev, curr, min_area=0)['count']
    assert R.pipeline(prev, curr, min_area=0, ignore_fraction=1.0)['count'] == 0
    const = jpeg_host.change_detect(list(stage_pair(64, 48, 'constant')), [(0, 1)], record_of(dict(threshold_type='otsu', min_area=0)))
    assert const['thresholds'][0] == 0 and const['counts'][0] == 64 * 48
    two = jpeg_host.change_detect(list(stage_pair(131, 97, 'two_level')), [(0, 1)],
                                  record_of(dict(threshold_type='otsu', min_area=0, blur_kernel_size=1, dilate_iterations=0)))
    assert two['counts'][0] == (97 // 3) * (131 // 3)


def test_blur_weights_and_reflection():
    for k in range(1, 128, 2):
        w = R.blur_weights(k)
        assert w.sum() == 256 and (w == w[::-1]).all() and (w >= 0).all()       # (the centre takes the remainder: not always the largest)
    assert R.reflect101(np.arange(-9, 12), 4).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1]
    assert R.reflect101(np.arange(-3, 4), 1).tolist() == [0] * 7


def test_carried_planes_and_several_pairs_in_one_call():
    """an image that comes with its blurred plane is not read; pairs of different sizes share a call"""
    a, b = stage_pair(60, 47)
    c, d = stage_pair(33, 80)
    rec = record_of(dict(min_area=0, blur_kernel_size=5))
    whole = jpeg_host.change_detect([a, b, c, d], [(0, 1), (2, 3), (1, 0)], rec, want_masks=True)
    carried = jpeg_host.change_detect([None, b, c, None], [(0, 1), (2, 3), (1, 0)], rec,
                                      blurred=[whole['blurred'][0], None, None, whole['blurred'][3]], want_masks=True)
    for key in ('counts', 'n_regions', 'regions', 'thresholds'):
        np.testing.assert_array_equal(whole[key], carried[key])
    for p, (x, y) in enumerate([(a, b), (c, d), (b, a)]):
        want = R.pipeline(x, y, min_area=0, blur_kernel_size=5)
        assert regions_of(whole, p) == want['regions'] and int(whole['counts'][p]) == want['count']
        np.testing.assert_array_equal(carried['masks'][p], want['dilated'])


def test_region_cap_and_bad_arguments():
    grid = np.zeros((21, 31, 3), np.uint8)
    grid[::2, ::2] = 255
    res = jpeg_host.change_detect([np.zeros_like(grid), grid], [(0, 1)], record_of(dict(blur_kernel_size=1, dilate_iterations=0, min_area=0), cap=10))
    assert res['overflow'][0] == 1 and res['n_regions'][0] == 11 * 16
    assert [tuple(r) for r in res['regions'][0]] == [(2 * k, 0, 1, 1, 1) for k in range(10)]
    a, b = stage_pair(20, 30)
    for bad in (dict(blur_kernel_size=4), dict(blur_kernel_size=129), dict(dilate_kernel_size=34), dict(dilate_iterations=65), dict(thr=256),
                dict(ignore_fraction=1.5), dict(min_area=-1)):
        with pytest.raises(ValueError):
            jpeg_host.change_detect([a, b], [(0, 1)], record_of(dict(dict(min_area=0), **bad)))
    with pytest.raises(ValueError):
        jpeg_host.change_detect([a, b[:10]], [(0, 1)], record_of({}))
    with pytest.raises(ValueError):
        jpeg_host.change_detect([a, b], [(0, 2)], record_of({}))


# ---- labelling on masks dilation never makes -------------------------------------------------------------------------------------

def adversarial_masks(h=37, w=70):
    """name -> mask (0 / 1).  At 37 x 70 every shape crosses the 64-pixel runs and the 4-row groups the device kernels work in."""
    yy, xx = np.mgrid[0:h, 0:w]
    masks = {'checkerboard': ((yy + xx) % 2 == 0), 'ones': np.ones((h, w), bool), 'zeros': np.zeros((h, w), bool),
             'diagonal': (yy == xx % h), 'anti_diagonal': (yy == (w - 1 - xx) % h)}
    spiral = np.zeros((h, w), bool)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    while top <= bottom and left <= right:                      # a one-pixel path winding inwards, two pixels between the turns
        spiral[top, left:right + 1] = True
        spiral[top:bottom + 1, right] = True
        if bottom - top >= 2:
            spiral[bottom, left + 2:right + 1] = True
        if right - left >= 4 and bottom - top >= 2:
            spiral[top + 2:bottom + 1, left + 2] = True
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        if top <= bottom and left <= right:
            spiral[top, left] = True
    masks['spiral'] = spiral
    comb = np.zeros((h, w), bool)                               # U-shapes that only meet in the last row
    comb[:, ::2] = True
    comb[h - 1, :] = True
    comb[0, :] = False
    comb[0, ::4] = True
    masks['comb'] = comb
    border = np.zeros((h, w), bool)                             # components touching every border, and the corners
    border[0, 3:9] = border[h - 1, 5:30] = border[4:20, 0] = border[10:h - 3, w - 1] = True
    border[0, 0] = border[0, w - 1] = border[h - 1, 0] = border[h - 1, w - 1] = True
    masks['borders'] = border
    rng = np.random.default_rng(5)
    masks['noise'] = rng.random((h, w)) < 0.45
    return {k: v.astype(np.uint8) for k, v in masks.items()}


@pytest.mark.parametrize('name', sorted(adversarial_masks()))
def test_host_labelling_on_adversarial_masks(name):
    mask = adversarial_masks()[name]
    _, want = R.regions(mask, 0)
    if name == 'checkerboard':
        assert len(want) == 1
    if name == 'comb':
        assert len(want) == 1
    rgb = np.repeat((mask * 255)[:, :, None], 3, 2)
    res = jpeg_host.change_detect([np.zeros_like(rgb), rgb], [(0, 1)], record_of(dict(blur_kernel_size=1, dilate_iterations=0, min_area=0), cap=2048),
                                  want_masks=True)
    np.testing.assert_array_equal(res['masks'][0], mask * 255)
    assert regions_of(res) == want and int(res['counts'][0]) == int(mask.sum())


# ---- the module against the reference's own -------------------------------------------------------------------------------------

def options_of(kwargs, **more):
    kw = dict(kwargs, **more)
    if 'threshold_type' in kw:
        kw['threshold_type'] = getattr(CD.ThresholdType, kw['threshold_type'])
    return CD.ChangeDetectionOptions(**kw)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    root = os.path.realpath(str(tmp_path_factory.mktemp('change_scene')))
    return root, R.build_reference_scene(root)


def test_the_fixture_is_the_one_the_generator_writes(golden):
    assert golden['option_sets'] == R.REFERENCE_OPTION_SETS and len(golden['runs']) == len(R.REFERENCE_OPTION_SETS) >= 10


@pytest.mark.parametrize('k', range(len(R.REFERENCE_OPTION_SETS)))
def test_rows_and_csv_text_equal_the_reference(golden, scene, tmp_path, k):
    root, folders = scene
    run = golden['runs'][k]
    out = str(tmp_path / 'out.csv')
    rows, counts = CD.process_folders(folders, options_of(R.REFERENCE_OPTION_SETS[k], workers=1), out, backend='host')
    want_rows = json.loads(json.dumps(run['rows']).replace('{ROOT}', root))
    assert [list(r) for r in rows] == [list(CD.COLUMNS)] * len(rows)
    assert rows == want_rows
    with open(out, newline='') as f:
        assert f.read() == run['csv'].replace('{ROOT}', root)
    assert counts == {'gpu_pairs': 0, 'host_pairs': 9, 'pil_decodes': 0}
    if k == 0:                                                  # a pool of workers gives the same rows
        assert CD.process_folders(folders, options_of(R.REFERENCE_OPTION_SETS[k], workers=3), None, backend='host')[0] == want_rows


def test_empty_folder_single_image_and_unreadable_rule(golden, scene, tmp_path):
    root, folders = scene
    out = str(tmp_path / 'e.csv')
    assert CD.process_folders([folders[3]], None, out, backend='host')[0] == []
    with open(out, newline='') as f:
        assert f.read() == golden['empty_csv']
    assert CD.process_camera_folder(folders[3]) == []
    single = CD.process_camera_folder(folders[2], CD.ChangeDetectionOptions(min_area=0))
    assert single == [CD.first_row('cam_single', os.path.join(folders[2], 'img_000.png'))]
    rows = CD.process_camera_folder(folders[0], CD.ChangeDetectionOptions(min_area=0))
    assert [r['motion_detected'] for r in rows] == [False, True, False, False, True, True]
    assert rows[2]['regions'] == rows[3]['regions'] == '' and rows[2]['diff_percentage'] == 0.0 and rows[3]['num_regions'] == 0


def test_detect_motion_and_pairs_of_different_sizes(scene, tmp_path, capsys):
    from PIL import Image
    root, folders = scene
    a, b = os.path.join(folders[0], 'img_000.png'), os.path.join(folders[0], 'img_001.png')
    res = CD.detect_motion(a, b, CD.ChangeDetectionOptions(min_area=0))
    want = R.pipeline(np.asarray(Image.open(a).convert('RGB')), np.asarray(Image.open(b).convert('RGB')), min_area=0)
    assert res['motion_detected'] and res['motion_regions'] == [r[:4] for r in want['regions']] and res['debug_images'] == {}
    assert res['diff_percentage'] == want['count'] / (72 * 96) * 100
    assert CD.detect_motion(None, b) == CD.empty_result()
    assert CD.detect_motion(a, os.path.join(folders[0], 'img_002.png')) == CD.empty_result()
    other = os.path.join(folders[1], 'img_000.png')             # another size: ours -- the empty result and a warning
    capsys.readouterr()
    assert CD.detect_motion(a, other) == CD.empty_result()
    assert 'differ in size' in capsys.readouterr().out


# ---- refusals, CLI, previews, sanitizers -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw', [dict(detection_method=CD.DetectionMethod.MOG2), dict(detection_method=CD.DetectionMethod.KNN),
                                dict(detection_method=CD.DetectionMethod.MOTION_HISTORY), dict(threshold_type=CD.ThresholdType.ADAPTIVE),
                                dict(verbose=True), dict(stop_at_token='x')], ids=lambda kw: next(iter(kw)) + '-' + str(next(iter(kw.values()))))
def test_what_is_not_restated_raises_before_anything_is_read(kw, tmp_path):
    missing = str(tmp_path / 'no_such_folder')
    options = CD.ChangeDetectionOptions(**kw)
    for backend in ('host', 'gpu'):
        with pytest.raises(NotImplementedError):
            CD.process_folders([missing], options, backend=backend)
        with pytest.raises(NotImplementedError):
            CD.process_camera_folder(missing, options, backend=backend)
        with pytest.raises(NotImplementedError):
            CD.detect_motion(missing, missing, options, backend=backend)


def test_option_values_and_backend_are_checked():
    for kw in (dict(blur_kernel_size=20), dict(dilate_kernel_size=0), dict(threshold=300), dict(ignore_fraction=-1.5), dict(min_area=-2)):
        with pytest.raises(ValueError):
            CD.check_options(CD.ChangeDetectionOptions(**kw))
    with pytest.raises(ValueError, match='backend'):
        CD.check_options(CD.ChangeDetectionOptions(), 'eager')
    with pytest.raises(NotImplementedError):
        CD.create_change_previews([], 'x')


def test_options_and_cli_defaults_are_the_references():
    o = CD.ChangeDetectionOptions()
    assert (o.min_area, o.threshold, o.blur_kernel_size, o.dilate_kernel_size, o.dilate_iterations, o.workers) == (500, 25, 21, 5, 2, 4)
    assert (o.history, o.var_threshold, o.mhi_duration, o.mhi_threshold, o.mhi_buffer_size) == (25, 16, 10.0, 30, 20)
    assert o.detection_method == CD.DetectionMethod.FRAME_DIFF and o.threshold_type == CD.ThresholdType.GLOBAL
    assert o.ignore_fraction is None and o.verbose is False and o.stop_at_token is None and not o.detect_shadows
    assert [m.name for m in CD.DetectionMethod] == ['FRAME_DIFF', 'MOG2', 'KNN', 'MOTION_HISTORY']
    assert [m.name for m in CD.ThresholdType] == ['GLOBAL', 'ADAPTIVE', 'OTSU']
    args = CD.build_parser().parse_args(['--root_dir', 'd'])
    assert (args.output_csv, args.min_area, args.threshold, args.detection_method, args.threshold_type) == (None, 500, 25, 'frame_diff', 'global')
    assert (args.history, args.var_threshold, args.mhi_duration, args.mhi_threshold, args.mhi_buffer_size) == (500, 16, 1.0, 30, 10)
    assert (args.adaptive_block_size, args.adaptive_c, args.ignore_fraction, args.workers, args.verbose) == (11, 2, None, 4, False)
    assert (args.create_previews, args.preview_folder, args.num_previews, args.backend, args.device) == (False, 'change_previews', 10, 'gpu', 0)
    o = CD.options_from_args(CD.build_parser().parse_args(['--root_dir', 'd', '--threshold_type', 'otsu', '--ignore_fraction', '-0.5']))
    assert o.threshold_type == CD.ThresholdType.OTSU and o.ignore_fraction == -0.5 and o.history == 500 and o.blur_kernel_size == 21


def test_cli_writes_the_csv_and_the_summary(golden, scene, tmp_path, capsys):
    root, folders = scene
    out = str(tmp_path / 'cli.csv')
    CD.main(['--root_dir', root, '--output_csv', out, '--min_area', '0', '--backend', 'host', '--workers', '1'])
    text = capsys.readouterr().out
    assert 'Found 4 camera folders' in text and 'Motion detection completed' in text
    assert 'Motion detected in 6 out of 12 images (50.00%)' in text
    with open(out, newline='') as f:
        got = sorted(f.read().splitlines())
    assert got == sorted(golden['runs'][1]['csv'].replace('{ROOT}', root).splitlines())      # (iterdir's order is the file system's)
    CD.main(['--root_dir', root, '--ignore_fraction', '2', '--backend', 'host'])
    assert 'Error: ignore_fraction must be between -1.0 and 1.0' in capsys.readouterr().out


def test_preview_sampling_equals_the_reference(golden, scene):
    root, folders = scene
    for k in (0, 3):
        rows = CD.process_folders(folders, options_of(R.REFERENCE_OPTION_SETS[k], workers=1), None, backend='host')[0]
        for key, want in golden['runs'][k]['sampled'].items():
            seed, num = key.split(',')
            picked = CD.sample_previews(rows, None if num == 'None' else int(num), int(seed))
            assert [CD.preview_name(r) for r in picked] == want
    assert CD.sample_previews([CD.first_row('c', 'x.png')], 3, 1) == []


def test_host_model_under_sanitizers(tmp_path):
    """change_host.cpp with a main of its own under AddressSanitizer + UBSan (`make asan-change`): buffers of their exact sizes,
    an image narrower than the blur radius, a pair over and exactly at the region cap"""
    exe = str(tmp_path / 'change_host_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-change', 'CHG_ASAN_OUT=' + exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(': ok') == 7 and 'WRONG' not in out.stdout
