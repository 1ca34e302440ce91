"""
Repeat-detection elimination without a GPU: megadetector_amd.repeat_detections with backend='host' (the host model
mdjpeg_repeat_detections, compiled from the header the kernels compile) against
  * tests/golden/rde_reference.json, recorded from the reference's own find_repeat_detections
    (tests/golden/gen_rde_golden_from_reference.py), and
  * a transcription of the rule in Python floats (tests/rde_cases.py),
plus hand-written structural cases, chunk independence, the capacity retry, the error cases and the entry points.
"""

import copy
import json
import os

import numpy as np
import pytest

import rde_cases as RC
from conftest import GOLDEN
from megadetector_amd import jpeg_host
from megadetector_amd import repeat_detections as RD


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'rde_reference.json')) as f:
        return json.load(f)


def golden_input(golden, case):
    """the results a golden case was run on; 'marked:<case>' is that case's input with that case's marks applied"""
    name = golden['cases'][case]['input']
    if name == 'nested':                                      # 'mixed' without the images that lie in no folder
        results = copy.deepcopy(golden['inputs']['mixed'])
        results['images'] = [im for im in results['images'] if '/' in im['file']]
        return results
    if not name.startswith('marked:'):
        return copy.deepcopy(golden['inputs'][name])
    base = golden['cases'][name[7:]]
    results = copy.deepcopy(golden['inputs'][base['input']])
    for im, neg in zip(results['images'], base['negative']):
        for d, s in zip(im.get('detections') or [], neg or []):
            if s and d['conf'] >= 0:
                d['conf'] = -d['conf']
    return results


def options_of(case_options):
    o = RD.RepeatDetectionOptions()
    for k, v in case_options.items():
        assert hasattr(o, k)
        setattr(o, k, v)
    return o


def check_against_golden(golden, case, out):
    want = golden['cases'][case]
    assert out.dirs == want['dirs']
    for d, locs in zip(out.dirs, out.suspicious_detections):
        got = {(loc.instances[0].filename, loc.instances[0].i_detection): [(i.filename, i.i_detection) for i in loc.instances]
               for loc in locs}
        assert len(got) == len(locs)
        ref = {tuple(c[0]): [tuple(i) for i in c] for c in want['locations'][d]}
        assert got == ref, (case, d)
        for loc in locs:
            assert loc.bbox == loc.instances[0].bbox and loc.relativeDir == d
        if want['options'].get('smartSort', 'xsort') == 'xsort':
            keys = [loc.bbox[0] + loc.bbox[2] / 2.0 for loc in locs]
            assert keys == sorted(keys)
        else:
            # in order of creation: by image, as the reference's (its order among the candidates of one image is its tree's)
            assert [loc.id for loc in locs] == sorted(loc.id for loc in locs)
    signs = [None if im.get('detections') is None else [1 if d['conf'] < 0 else 0 for d in im['detections']]
             for im in out.detectionResults['images']]
    assert signs == want['negative'], case


def test_golden_cases_cover_what_they_should(golden):
    cases = golden['cases']
    assert len(cases) >= 10
    opts = [c['options'] for c in cases.values()]
    for key in ('categoryAgnosticComparisons', 'excludeClasses', 'minSuspiciousDetectionSize', 'maxSuspiciousDetectionSize',
                'confidenceMax', 'nDirLevelsFromLeaf', 'maxImagesPerFolder', 'smartSort', 'excludeFolders'):
        assert any(key in o for o in opts), key
    assert all(o.get('occurrenceThreshold', 20) >= 2 for o in opts)
    mixed = golden['inputs']['mixed']['images']
    assert any('/' not in im['file'] for im in mixed) and any(im['file'].count('/') >= 3 for im in mixed)
    assert any('failure' in im for im in mixed) and any(im.get('detections') == [] for im in mixed)
    dets = [d for im in mixed for d in im.get('detections') or []]
    assert any(d['bbox'][2] == 0 for d in dets) and any(d['bbox'][2] < 0 for d in dets)
    assert any(c['input'].startswith('marked:') for c in cases.values())
    assert any(sum(len(x) for v in c['locations'].values() for x in v) > sum(sum(s) for s in c['negative'] if s)
               for c in cases.values()), 'no case with a box counted in two candidates'


def test_host_backend_reproduces_every_golden_case(golden, tmp_path):
    for case, want in golden['cases'].items():
        path = str(tmp_path / (case + '.json'))
        with open(path, 'w') as f:
            json.dump(golden_input(golden, case), f)
        out = RD.find_repeat_detections(path, None, options_of(want['options']), backend='host')
        check_against_golden(golden, case, out)


def host(boxes, thr, agnostic, occ, **kw):
    return RD.match_boxes(boxes, thr, agnostic, occ, backend='host', **kw)


def assert_same(got, want):
    for g, w, name in zip(got, want, ('is_candidate', 'n_instances', 'pairs')):
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize('name', sorted(RC.STRUCTURAL))
def test_structural_cases(name):
    boxes, thr, agnostic, occ, *want = RC.structural(name)
    assert_same(host(boxes, thr, agnostic, occ), want)
    assert_same(RC.py_repeat_detections(boxes, thr, agnostic, occ), want)


def test_python_restatement_on_seeded_scenes():
    for seed, decimals, thr, agnostic, occ in [(1, None, 0.8, 0, 3), (2, 3, 0.85, 0, 2), (3, None, 0.6, 1, 4), (4, 2, 0.9, 0, 1)]:
        boxes = RC.seeded_scene(3, 150, seed, decimals)
        got = host(boxes, thr, agnostic, occ)
        assert_same(got, RC.py_repeat_detections(boxes, thr, agnostic, occ))
        assert 0 < got[0].sum() < len(boxes)
    boxes = RC.seeded_scene(3, 150, 1)
    got = host(boxes, 0.8, 0, 1)
    assert RC.has_multi_match(got[2]) and RC.has_chain(boxes, got[0], 0.8)


def test_threshold_at_a_pairs_own_iou():
    """the comparison is `iou >= threshold` on the reference's doubles: at a pair's own IoU it matches, one ulp above it does not"""
    pairs = RC.threshold_pairs()
    assert len(pairs) == 200
    for boxes, iou in pairs:
        assert host(boxes, iou, 0, 1)[0].tolist() == [1, 0], (boxes, iou)
        assert host(boxes, RC.next_up(iou), 0, 1)[0].tolist() == [1, 1], (boxes, iou)


def test_chunk_independence_and_capacity_retry():
    boxes = RC.seeded_scene(2, 90, 7)[:200]
    assert len(boxes) == 200
    want = host(boxes, 0.8, 0, 2, chunk=0)
    assert len(want[2]) > 20
    for chunk in (1, 2, 63, 64, 65):
        assert_same(host(boxes, 0.8, 0, 2, chunk=chunk), want)
    # too small a buffer: the code, the needed capacity, nothing written; then the retry match_boxes makes
    lib = jpeg_host.load()
    import ctypes as C
    is_cand, n_inst = np.zeros(200, np.uint8), np.zeros(200, np.int32)
    pairs = np.full((5, 2), -7, np.int64)
    needed = C.c_int64(0)
    rc = lib.mdjpeg_repeat_detections(boxes.ctypes.data, 200, 0.8, 0, 2, 0, is_cand.ctypes.data, n_inst.ctypes.data, pairs.ctypes.data, 4,
                                      C.byref(needed))
    assert rc == jpeg_host.MDJPEG_ECAPACITY and needed.value == len(want[2]) and (pairs == -7).all()
    np.testing.assert_array_equal(is_cand, want[0])
    np.testing.assert_array_equal(n_inst, want[1])
    assert_same(host(boxes, 0.8, 0, 2, capacity=4), want)
    assert_same(host(boxes, 0.8, 0, 2, capacity=0), want)


def test_bad_arguments():
    boxes = RC.make_boxes([(0.1, 0.1, 0.2, 0.2, 1, 1), (0.1, 0.1, 0.2, 0.2, 0, 1)])
    with pytest.raises(ValueError):
        host(boxes, 0.9, 0, 1)                              # the group decreases
    good = boxes[::-1].copy()
    with pytest.raises(ValueError):
        host(good, float('nan'), 0, 1)
    with pytest.raises(ValueError):
        host(good, 0.9, 0, 1, chunk=-1)
    with pytest.raises(ValueError, match='backend'):
        RD.match_boxes(good, 0.9, 0, 1, backend='eager')
    assert host(good, 0.9, 0, 1)[0].tolist() == [1, 1]


def test_gpu_backend_without_a_device_is_an_error_not_a_fallback():
    import torch
    from megadetector_amd._lib import HipError
    boxes, thr, agnostic, occ, *want = RC.structural('drift_chain')
    with pytest.raises(ValueError, match='group'):             # the arguments are checked before the device is looked for
        RD.match_boxes(RC.make_boxes([(0.1, 0.1, 0.2, 0.2, 1, 1), (0.1, 0.1, 0.2, 0.2, 0, 1)]), thr, 0, 1,
                       backend='gpu')
    if torch.cuda.is_available():
        assert_same(RD.match_boxes(boxes, thr, agnostic, occ, backend='gpu'), want)
    else:
        with pytest.raises(HipError, match='no HIP device'):
            RD.match_boxes(boxes, thr, agnostic, occ, backend='gpu')


def test_option_errors(golden, tmp_path):
    path = str(tmp_path / 'in.json')
    with open(path, 'w') as f:
        json.dump(golden['inputs']['mixed'], f)
    o = RD.RepeatDetectionOptions()
    assert o.bWriteFilteringFolder is False and o.smartSort == 'xsort' and o.occurrenceThreshold == 20 and o.iouThreshold == 0.9
    assert (o.confidenceMin, o.confidenceMax, o.minSuspiciousDetectionSize, o.maxSuspiciousDetectionSize) == (0.1, 1.0, 0.0, 0.2)
    o.smartSort = 'clustersort'
    with pytest.raises(NotImplementedError, match='clustersort'):
        RD.find_repeat_detections(path, None, o, backend='host')
    for key, value in (('bWriteFilteringFolder', True), ('filterFileToLoad', 'x/detectionIndex.json'), ('bRenderDetectionTiles', True),
                       ('outputBase', '/tmp/review')):
        o = RD.RepeatDetectionOptions()
        setattr(o, key, value)
        with pytest.raises(NotImplementedError, match='review folder'):
            RD.find_repeat_detections(path, None, o, backend='host')
    o = RD.RepeatDetectionOptions()
    o.smartSort = 'sideways'
    with pytest.raises(ValueError):
        RD.find_repeat_detections(path, None, o, backend='host')


def test_output_files_and_command_line(golden, tmp_path):
    case = 'defaults_thr5'
    want = golden['cases'][case]
    results = golden_input(golden, case)
    results['info']['format_version'] = 1.4                   # a number in the file: written back as a string
    results['images'][0]['max_detection_conf'] = 0.99
    results['images'][1]['failure'] = None
    path = str(tmp_path / 'in.json')
    with open(path, 'w') as f:
        json.dump(results, f)
    out_fn = str(tmp_path / 'fn' / 'out.json')
    out = RD.find_repeat_detections(path, out_fn, options_of(want['options']), backend='host')
    check_against_golden(golden, case, out)
    written = json.load(open(out_fn))
    assert written['info']['format_version'] == '1.4' and written['detection_categories'] == results['detection_categories']
    assert len(written['images']) == len(results['images'])
    for a, b, neg in zip(results['images'], written['images'], want['negative']):
        assert 'max_detection_conf' not in b and b.get('failure', '') is not None
        assert set(a) - {'max_detection_conf', 'failure'} == set(b) - {'failure'}          # no key gained: no "detections": null
        for da, db, s in zip(a.get('detections') or [], b.get('detections') or [], neg or []):
            assert db['bbox'] == da['bbox'] and db['category'] == da['category']
            assert db['conf'] == (-da['conf'] if s else da['conf'])                        # not rounded, only negated
    index = json.load(open(out_fn + '.rde_index.json'))
    assert index['dirs'] == want['dirs'] and index['options']['occurrenceThreshold'] == 5
    for d, locs in zip(index['dirs'], index['suspicious_detections']):
        assert sorted((tuple(c['instances'][0][k] for k in ('filename', 'i_detection'))) for c in locs) == \
            sorted(tuple(c[0]) for c in want['locations'][d])
        assert all(set(c) >= {'bbox', 'category', 'id', 'instances'} for c in locs)
    # the command line writes the same two files
    out_cli = str(tmp_path / 'cli' / 'out.json')
    assert RD.main([path, '--outputFile', out_cli, '--occurrenceThreshold', '5', '--iouThreshold', '0.85', '--backend', 'host']) == 0
    assert open(out_cli, 'rb').read() == open(out_fn, 'rb').read()
    assert open(out_cli + '.rde_index.json', 'rb').read() == open(out_fn + '.rde_index.json', 'rb').read()
    # format < 1.3 keeps max_detection_conf, brought up to date
    results['info']['format_version'] = '1.2'
    with open(path, 'w') as f:
        json.dump(results, f)
    out12 = str(tmp_path / 'out12.json')
    RD.find_repeat_detections(path, out12, options_of(want['options']), backend='host')
    for im in json.load(open(out12))['images']:
        if im.get('detections'):
            assert im['max_detection_conf'] == max(d['conf'] for d in im['detections'])


def test_batch_driver_switch_leaves_the_main_results_alone(tmp_path, monkeypatch):
    from PIL import Image
    from megadetector_amd import run_detector_batch as RDB
    from stub_detector import StubDetector
    root = tmp_path / 'images'
    rng = np.random.default_rng(0)
    for cam in ('cam0', 'cam1'):
        os.makedirs(root / cam)
        for i in range(14):
            Image.fromarray(rng.integers(0, 256, (20 + i, 30, 3), dtype=np.uint8)).save(root / cam / 'img_{}.png'.format(i))
    monkeypatch.setattr(RDB.run_detector, 'load_detector', lambda *a, **k: StubDetector())
    monkeypatch.setattr(RDB, 'datetime', type('FixedClock', (), {'now': staticmethod(lambda: __import__('datetime').datetime(2024, 1, 2))}))
    plain, with_rde, rde = str(tmp_path / 'plain.json'), str(tmp_path / 'with.json'), str(tmp_path / 'rde.json')
    common = ['stub', str(root), None, '--output_relative_filenames', '--recursive', '--quiet']
    RDB.main(common[:2] + [plain] + common[3:])
    RDB.main(common[:2] + [with_rde] + common[3:] + ['--rde_results_file', rde, '--rde_occurrence_threshold', '3', '--rde_iou_threshold', '0.8',
                                                     '--rde_backend', 'host'])
    assert open(plain, 'rb').read() == open(with_rde, 'rb').read()
    main_results, marked = json.load(open(plain)), json.load(open(rde))
    # every stub image has the box [0, 0.05, 0.2, 0.3]: fourteen a camera, of three categories
    assert [im['file'] for im in marked['images']] == [im['file'] for im in main_results['images']]
    changed = 0
    for a, b in zip(main_results['images'], marked['images']):
        for da, db in zip(a['detections'], b['detections']):
            assert db['bbox'] == da['bbox'] and abs(db['conf']) == abs(da['conf'])
            changed += db['conf'] != da['conf']
    index = json.load(open(rde + '.rde_index.json'))
    assert index['dirs'] == ['cam0', 'cam1']
    assert changed > 0
    assert changed == sum(len({(i['filename'], i['i_detection']) for c in locs for i in c['instances']})
                          for locs in index['suspicious_detections'])
    with pytest.raises(AssertionError, match='--rde_results_file'):
        RDB.main(common[:2] + [str(tmp_path / 'x.json')] + common[3:] + ['--rde_iou_threshold', '0.8'])
