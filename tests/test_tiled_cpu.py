"""
Host side of tiled inference (megadetector_amd/run_tiled_inference.py) against tests/golden/tiled_reference.json, which
tests/golden/gen_tiled_golden_from_reference.py records from the real reference: tile origins, the mapping of tile
detections to the image with its rounding, the cross-tile NMS, the failure records and the JSON files -- compared
exactly, as text.  Then the driver end to end with a stub detector, and checkpoint resume.

One case the reference cannot pin: with a FAILED tile the reference itself raises (its results writer gives a failed
tile 'detections': None, which the merge loop then iterates: the fixture records 'raises': 'TypeError').  The behaviour
its code states -- the image becomes a failure carrying the tile's failure string -- is what is asserted here.
"""

import glob
import json
import os
import re

import numpy as np
import pytest

from stub_detector import StubDetector
from megadetector_amd import run_tiled_inference as T

HERE = os.path.dirname(os.path.abspath(__file__))
TIME_RE = re.compile(r'("detection_completion_time": )"[^"]*"')

with open(os.path.join(HERE, 'golden', 'tiled_reference.json'), 'r') as f:
    GOLDEN = json.load(f)


def _read(path):
    with open(path, 'r', encoding='utf-8') as f:
        return TIME_RE.sub(r'\1"<time>"', f.read())


def _write_images(folder):
    from PIL import Image
    for name, w, h, seed in GOLDEN['images']:
        p = os.path.join(folder, name)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)


class CannedDetector:
    """returns the fixture's canned tile-level detections, keyed on the tile's name"""

    def __init__(self, canned):
        self.canned = canned

    def generate_detections_for_tiles(self, image, origins, size, tile_ids=None, detection_threshold=1e-5,
                                      image_size=None, augment=False, verbose=False):
        out = []
        for name in tile_ids:
            c = self.canned[os.path.splitext(os.path.basename(name))[0]]
            if 'failure' in c:
                out.append({'file': name, 'detections': None, 'failure': c['failure']})
            else:
                dets = [dict(d, bbox=list(d['bbox'])) for d in c['detections']]
                out.append({'file': name, 'detections': dets, 'max_detection_conf': max([d['conf'] for d in dets] + [0.0])})
        return out


class TileStub(StubDetector):
    """the stub detector with the tile method: numpy crops through its own _one"""

    def generate_detections_for_tiles(self, image, origins, size, tile_ids=None, detection_threshold=1e-5,
                                      image_size=None, augment=False, verbose=False):
        a = np.asarray(image)
        self.batches.append(len(origins))
        if any(n in self.fail_on for n in tile_ids):
            raise RuntimeError('simulated device failure')
        return [self._one(a[y:y + size[1], x:x + size[0]], n) for (x, y), n in zip(origins, tile_ids)]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', GOLDEN['boundaries'], ids=lambda c: '{}x{}_{}x{}_{}'.format(
    *c['image_size'], *c['tile'], c['overlap']))
def test_tile_origins(case):
    tile, overlap = case['tile'], case['overlap']
    stride = (round(tile[0] * (1.0 - overlap)), round(tile[1] * (1.0 - overlap)))
    if case['positions'] is None:
        with pytest.raises(AssertionError):
            T.get_patch_boundaries(case['image_size'], tile, stride)
        return
    got = T.get_patch_boundaries(case['image_size'], tile, stride)
    assert [list(p) for p in got] == case['positions']
    assert got[-1][0] + tile[0] == case['image_size'][0] and got[-1][1] + tile[1] == case['image_size'][1]


def test_default_stride_and_names():
    assert [list(p) for p in T.get_patch_boundaries([3000, 2000], [1280, 1280])] == GOLDEN['default_stride_positions']
    assert T.patch_info_to_patch_name('a.jpg', 10, 20) == GOLDEN['patch_name']
    assert [list(p) for p in T.get_patch_boundaries([3000, 2000], [1280, 1280], 0.5)] == GOLDEN['default_stride_positions']


def _run(tmp_path, canned, name='out.json', **kwargs):
    folder = str(tmp_path / 'Survey Imgs')
    tiling = str(tmp_path / 'tiling')
    if not os.path.isdir(folder):
        _write_images(folder)
    out = str(tmp_path / name)
    res = T.run_tiled_inference('md_v5a.0.0.pt', folder, tiling, out, tile_size_x=GOLDEN['tile'][0],
                                tile_size_y=GOLDEN['tile'][1], tile_overlap=GOLDEN['overlap'],
                                detector=CannedDetector(canned), **kwargs)
    return res, out, tiling


def test_mapping_rounding_and_merge_match_the_reference_exactly(tmp_path):
    ref = GOLDEN['run']
    assert 'raises' not in ref
    res, out, tiling = _run(tmp_path, ref['canned'])
    assert _read(glob.glob(os.path.join(tiling, '*_patch_level_results.json'))[0]) == ref['patch_level_text']
    assert _read(glob.glob(os.path.join(tiling, '*_image_level_results_pre_nms.json'))[0]) == ref['pre_nms_text']
    assert _read(out) == ref['output_text']
    assert json.loads(ref['output_text'])['images'] == res['images']
    # what the fixture must exercise: duplicates removed, a failure record, an image without detections
    pre = {im['file']: im for im in json.loads(ref['pre_nms_text'])['images']}
    post = {im['file']: im for im in res['images']}
    assert len(post['a.png']['detections']) < len(pre['a.png']['detections'])
    assert post['small.png']['failure'] == 'Patch generation error' and post['small.png']['detections'] is None
    assert post['empty.png']['detections'] == []
    confs = [d['conf'] for d in pre['a.png']['detections']]
    assert len(confs) != len(set(confs)), 'equal scores across tiles'
    # the tile record
    info_file = glob.glob(os.path.join(tiling, '*_patch_info.json'))
    assert len(info_file) == 1
    with open(info_file[0]) as f:
        info = json.load(f)
    for im in info:
        for p in im['patches']:
            assert not os.path.exists(p['patch_fn']), 'tile files are never written'
            p['patch_fn'] = os.path.relpath(p['patch_fn'], tiling)
        if im['error'] is not None:
            im['error'] = im['error'].split('\n')[0]
    assert info == ref['patch_info']
    assert not glob.glob(os.path.join(tiling, '*.jpg'))


def test_a_failed_tile_fails_its_image(tmp_path):
    ref = GOLDEN['run_with_failed_tile']
    assert ref.get('raises') == 'TypeError', 'the reference itself cannot finish this case (see the module docstring)'
    res, out, _ = _run(tmp_path, ref['canned'])
    by = {im['file']: im for im in res['images']}
    assert by['a.png'] == {'file': 'a.png', 'detections': None, 'failure': 'inference failure'}
    good = {im['file']: im for im in json.loads(GOLDEN['run']['output_text'])['images']}
    for k in by:
        if k != 'a.png':
            assert by[k] == good[k]
    assert json.load(open(out))['images'] == res['images']


def test_greedy_nms_is_the_pinned_one():
    z = np.load(os.path.join(HERE, 'golden', 'nms_reference.npz'))
    from oracle import pre_post as O
    import torch
    rng = np.random.default_rng(5)
    xy = rng.random((400, 2)).astype(np.float32)
    wh = (rng.random((400, 2)) * 0.2).astype(np.float32)
    boxes = np.concatenate([xy, xy + wh], 1)
    scores = np.round(rng.random(400), 1).astype(np.float32)            # many ties
    ref = O._greedy_nms(torch.from_numpy(boxes), torch.from_numpy(scores), 0.45).tolist()
    assert T.greedy_nms(boxes, scores, 0.45) == ref
    assert len(z.files) > 0


def test_unsupported_parameters():
    with pytest.raises(ValueError, match='yolo_inference_options'):
        T.run_tiled_inference('m.pt', '.', None, 'o.json', yolo_inference_options=object(), detector=TileStub())
    with pytest.raises(ValueError, match='create_tiles_only'):
        T.run_tiled_inference('m.pt', '.', None, 'o.json', create_tiles_only=True, detector=TileStub())


def test_end_to_end_with_stub_detector_and_checkpoint_resume(tmp_path):
    from PIL import Image
    folder = str(tmp_path / 'imgs')
    _write_images(folder)
    tile, overlap = (16, 12), 0.25
    det = TileStub()
    out = str(tmp_path / 'out.json')
    res = T.run_tiled_inference('md_v5a.0.0.pt', folder, None, out, tile_size_x=tile[0], tile_size_y=tile[1],
                                tile_overlap=overlap, detector=det, remove_tiles=True, overwrite_tiles=False,
                                n_patch_extraction_workers=4, pool_type='process', load_cached_tiles_if_available=True)
    with open(out) as f:
        on_disk = json.load(f)
    assert on_disk == res and set(on_disk) == {'info', 'detection_categories', 'images'}
    assert _read(out) == TIME_RE.sub(r'\1"<time>"', json.dumps(res, indent=1))
    files = [os.path.relpath(p, folder) for p in sorted(glob.glob(os.path.join(folder, '**', '*.png'), recursive=True))]
    assert [im['file'] for im in res['images']] == files            # input order
    # manual composition: crop -> stub -> threshold -> sort -> merge -> nms
    stride = (round(tile[0] * (1 - overlap)), round(tile[1] * (1 - overlap)))
    stub = StubDetector()
    for im in res['images']:
        a = np.asarray(Image.open(os.path.join(folder, im['file'])).convert('RGB'))
        h, w = a.shape[:2]
        if w < tile[0] or h < tile[1]:
            assert im['failure'] == 'Patch generation error' and im['detections'] is None
            continue
        patches, tiles = [], []
        for x, y in T.get_patch_boundaries((w, h), tile, stride):
            r = stub._one(a[y:y + tile[1], x:x + tile[0]], 't')
            r['detections'] = sorted([d for d in r['detections'] if d['conf'] >= 0.005], key=lambda d: -d['conf'])
            patches.append({'xmin': x, 'xmax': x + tile[0] - 1, 'ymin': y, 'ymax': y + tile[1] - 1})
            tiles.append(r)
        want = {'images': [T.merge_tile_results(im['file'], (w, h), patches, tiles, tile)]}
        T.in_place_nms(want, verbose=False)
        assert im == want['images'][0]
    # resume: a run that checkpoints after every image, cut short, then finished from the checkpoint
    ck = str(tmp_path / 'ck.json')
    n_images = len(res['images'])
    first = files[:2]
    lst = str(tmp_path / 'first.json')
    with open(lst, 'w') as f:
        json.dump(first, f)
    T.run_tiled_inference('md_v5a.0.0.pt', folder, None, str(tmp_path / 'part.json'), tile_size_x=tile[0],
                          tile_size_y=tile[1], tile_overlap=overlap, detector=TileStub(), image_list=lst,
                          checkpoint_path=ck, checkpoint_frequency=1)
    assert len(json.load(open(ck))['checkpoint']) == 2
    det2 = TileStub()
    out2 = str(tmp_path / 'out2.json')
    T.run_tiled_inference('md_v5a.0.0.pt', folder, None, out2, tile_size_x=tile[0], tile_size_y=tile[1],
                          tile_overlap=overlap, detector=det2, checkpoint_path=ck, checkpoint_frequency=2)
    assert _read(out2) == _read(out)
    assert len(det2.batches) < len(det.batches) and n_images > 2


def test_a_failing_device_call_is_an_inference_failure(tmp_path):
    folder = str(tmp_path / 'imgs')
    _write_images(folder)

    class Failing(TileStub):
        def generate_detections_for_tiles(self, image, origins, size, tile_ids=None, **kw):
            if np.asarray(image).shape[:2] == (12, 16):
                raise RuntimeError('simulated device failure')
            return TileStub.generate_detections_for_tiles(self, image, origins, size, tile_ids=tile_ids, **kw)

    res = T.run_tiled_inference('md_v5a.0.0.pt', folder, None, str(tmp_path / 'o.json'), tile_size_x=16, tile_size_y=12,
                                detector=Failing(), loader_workers=0)
    by = {im['file']: im for im in res['images']}
    assert by['c.png'] == {'file': 'c.png', 'detections': None, 'failure': 'inference failure'}
    assert by['a.png']['detections'] is not None
