"""
Repeat-detection elimination on the GPU: mdhip_repeat_detections must equal its host model mdjpeg_repeat_detections array
for array -- is_candidate, n_instances, pairs.  The results are integers: no tolerance anywhere.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import rde_cases as RC
from conftest import GOLDEN
from megadetector_amd import repeat_detections as RD

pytestmark = pytest.mark.gpu


def both(boxes, thr, agnostic, occ, chunk=0, **kw):
    want = RD.match_boxes(boxes, thr, agnostic, occ, backend='host')
    got = RD.match_boxes(boxes, thr, agnostic, occ, backend='gpu', chunk=chunk, **kw)
    for g, w, name in zip(got, want, ('is_candidate', 'n_instances', 'pairs')):
        np.testing.assert_array_equal(g, w, err_msg='{} (chunk {})'.format(name, chunk))
    return got


@pytest.fixture(scope='module')
def scene_200():
    return RC.seeded_scene(2, 90, 7)[:200]


@pytest.fixture(scope='module')
def scene_4000():
    boxes = RC.seeded_scene(5, 790, 21)
    assert 3900 <= len(boxes) <= 4200
    return boxes


@pytest.mark.parametrize('name', sorted(RC.STRUCTURAL))
def test_structural_cases(name):
    boxes, thr, agnostic, occ, *want = RC.structural(name)
    for chunk in (0, 1, 2):
        got = both(boxes, thr, agnostic, occ, chunk=chunk)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 127, 128, 129, 200])
def test_chunk_and_word_boundaries(scene_200, n):
    got = both(scene_200[:n], 0.8, 0, 2, chunk=64)
    if n >= 127:
        assert len(got[2]) > 0 and 0 < got[0].sum() < n


@pytest.mark.parametrize('chunk', [1, 2, 63, 65, 0])
def test_results_do_not_depend_on_the_chunk(scene_200, chunk):
    both(scene_200, 0.8, 0, 2, chunk=chunk)


@pytest.mark.parametrize('first_group', [96, 128])
def test_group_boundary_inside_a_chunk_and_on_its_edge(scene_200, first_group):
    """chunk 64: a group that ends in the middle of the second chunk, and one that ends exactly where the third begins; the
    boxes on either side of the boundary are the same places, so only the group keeps them apart"""
    boxes = scene_200.copy()
    boxes['group'] = (np.arange(len(boxes)) >= first_group).astype(np.int32) * 3
    got = both(boxes, 0.8, 0, 2, chunk=64)
    assert got[0][first_group] == 1                           # the first box of a group is always a candidate
    assert (boxes['group'][got[2][:, 0]] == boxes['group'][got[2][:, 1]]).all()


def test_threshold_at_a_pairs_own_iou():
    """`iou >= threshold` on the reference's doubles: at a pair's own IoU the second box matches the first (in each of the
    three kernels that compare: within a chunk, against an earlier chunk's candidates, and when the instances are counted),
    one ulp above it does not.  A contracted multiply-add or a rewritten comparison fails here."""
    for boxes, iou in RC.threshold_pairs():
        for chunk in (0, 1):
            got = both(boxes, iou, 0, 1, chunk=chunk)
            assert got[0].tolist() == [1, 0] and got[1].tolist() == [2, 0], (boxes, iou)
            got = both(boxes, RC.next_up(iou), 0, 1, chunk=chunk)
            assert got[0].tolist() == [1, 1] and got[1].tolist() == [1, 1], (boxes, iou)


@pytest.mark.parametrize('chunk', [0, 256])
def test_seeded_scene(scene_4000, chunk):
    got = both(scene_4000, 0.8, 0, 3, chunk=chunk)
    everything = RD.match_boxes(scene_4000, 0.8, 0, 1, backend='host')
    assert RC.has_multi_match(everything[2]), 'the scene has no box between two candidates'
    assert RC.has_chain(scene_4000, got[0], 0.8), 'the scene has no drift chain'
    assert len(got[2]) > 1000 and 100 < got[0].sum() < len(scene_4000) // 2


def test_capacity_retry_and_errors(scene_200):
    from megadetector_amd import _lib
    lib = _lib.load()
    want = RD.match_boxes(scene_200, 0.8, 0, 2, backend='host')
    is_cand, n_inst = np.zeros(200, np.uint8), np.zeros(200, np.int32)
    pairs = np.full((5, 2), -7, np.int64)
    needed = C.c_int64(0)

    def call(boxes, n, thr=0.8, chunk=0, device=0, cap=4):
        return lib.mdhip_repeat_detections(device, boxes.ctypes.data, n, thr, 0, 2, chunk, is_cand.ctypes.data, n_inst.ctypes.data,
                                           pairs.ctypes.data, cap, C.byref(needed))
    assert call(scene_200, 200) == _lib.MDHIP_ECAPACITY
    assert needed.value == len(want[2]) and (pairs == -7).all()
    np.testing.assert_array_equal(is_cand, want[0])
    np.testing.assert_array_equal(n_inst, want[1])
    both(scene_200, 0.8, 0, 2, capacity=4)
    decreasing = scene_200.copy()
    decreasing['group'][100] = -1
    assert call(decreasing, 200) == -1 and b'group' in lib.mdhip_last_error(None)
    assert call(scene_200, -1) == -1
    assert call(scene_200, 200, thr=float('nan')) == -1
    assert call(scene_200, 200, chunk=1 << 20) == -1
    assert call(scene_200, 200, device=4096) == -1 and b'device' in lib.mdhip_last_error(None)
    assert (pairs == -7).all()


def test_golden_case_end_to_end(tmp_path):
    with open(os.path.join(GOLDEN, 'rde_reference.json')) as f:
        golden = json.load(f)
    want = golden['cases']['agnostic']
    path = str(tmp_path / 'in.json')
    with open(path, 'w') as f:
        json.dump(golden['inputs'][want['input']], f)
    options = RD.RepeatDetectionOptions()
    for k, v in want['options'].items():
        setattr(options, k, v)
    out = RD.find_repeat_detections(path, str(tmp_path / 'gpu.json'), options, backend='gpu')
    assert out.dirs == want['dirs']
    for d, locs in zip(out.dirs, out.suspicious_detections):
        got = {(loc.instances[0].filename, loc.instances[0].i_detection): [(i.filename, i.i_detection) for i in loc.instances]
               for loc in locs}
        assert got == {tuple(c[0]): [tuple(i) for i in c] for c in want['locations'][d]}
    signs = [None if im.get('detections') is None else [1 if d['conf'] < 0 else 0 for d in im['detections']]
             for im in out.detectionResults['images']]
    assert signs == want['negative']
    RD.find_repeat_detections(path, str(tmp_path / 'host.json'), options, backend='host')
    for name in ('{}.json', '{}.json.rde_index.json'):
        assert open(tmp_path / name.format('gpu'), 'rb').read() == open(tmp_path / name.format('host'), 'rb').read()
