"""
Generates tests/golden/rde_reference.json by running the *real* reference code: repeat_detections_core.find_repeat_detections
(with _find_matches_in_directory, _sort_detections_for_directory, _update_detection_table, load_api_results and
ct_utils.get_iou underneath it) on seeded results files.  The reference cannot travel with the tests, so what it computes is
committed as a small fixture together with this script.

Recorded per case: the options, the input (by name: all cases run on the one scene 'mixed', on it without its flat files
('nested'), or on it as an earlier case marked it), per location the suspicious candidates -- each the full instance list as
(file, i_detection) in the reference's order, so its first entry is the candidate's first instance -- and the sign of every
`conf` of the marked results.

cv2, jsonpickle and fastquadtree are absent here and are stubbed.  jsonpickle needs a no-op set_encoder_options.  The
stand-in for fastquadtree.pyqtree is an Index whose intersect() returns EVERY item whose rectangle touches the query: a
superset of what the quadtree answers, and since the IoU test decides, the matches are the same.  The reference runs with
bWriteFilteringFolder=False, bParallelizeComparisons=True, nWorkers=1 and threads (its serial branch trips over an unbound
`pool`).

Inputs keep coordinates and confidences to 3 decimals (the reference's writer rounds to 3: the identity here), boxes inside
[0, 1], and occurrenceThreshold >= 2 (its marking step raises on a malformed suspicious candidate).

Run:  python tests/golden/gen_rde_golden_from_reference.py <folder that holds the reference's megadetector package>
"""

import copy
import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def r3(v):
    return round(float(v), 3)


def make_scene(seed, cameras, images_per_camera):
    """A results file: per camera a few fixed spots (boxes that come back with a little jitter, some drifting, one spot with
    three categories) among random boxes; plus a failed image, images without detections, a w == 0 box and a negative-w box."""
    rng = np.random.default_rng(seed)
    images = []
    for cam in cameras:
        spots = []
        for k in range(4):
            w, h = r3(rng.uniform(0.08, 0.3)), r3(rng.uniform(0.08, 0.3))
            spots.append([r3(rng.uniform(0.02, 0.4)), r3(rng.uniform(0.02, 0.6)), w, h, str(1 + k % 3), r3(rng.uniform(0.0, 0.002))])
        n = images_per_camera + int(rng.integers(0, 7))
        for i in range(n):
            name = '{}{}I{:02d}.{}'.format(cam, '/' if cam else '', i, 'JPG' if i % 5 else 'jpg')
            dets = []
            for k, (x, y, w, h, cat, drift) in enumerate(spots):
                if rng.random() < 0.55:
                    jx, jy = rng.integers(-3, 4, 2) / 1000.0
                    dets.append({'category': cat, 'conf': r3(rng.uniform(0.05, 0.95)),
                                 'bbox': [r3(x + drift * i + jx), r3(y + jy), w, h]})
                    if k == 0 and rng.random() < 0.5:          # three categories at one spot
                        for other in ('2', '3'):
                            dets.append({'category': other, 'conf': r3(rng.uniform(0.15, 0.9)), 'bbox': [r3(x + drift * i), y, w, h]})
            for _ in range(int(rng.integers(0, 3))):
                w, h = r3(rng.uniform(0.03, 0.6)), r3(rng.uniform(0.03, 0.6))
                dets.append({'category': str(int(rng.integers(1, 4))), 'conf': r3(rng.uniform(0.0, 1.0)),
                             'bbox': [r3(rng.uniform(0, 1 - w)), r3(rng.uniform(0, 1 - h)), w, h]})
            if i % 17 == 3:                                  # the same place twice in ONE image
                dets.append(copy.deepcopy(dets[0]) if dets else {'category': '1', 'conf': 0.5, 'bbox': [0.4, 0.4, 0.1, 0.1]})
            if i % 13 == 5:
                dets.append({'category': '1', 'conf': 0.7, 'bbox': [0.3, 0.3, 0.0, 0.2]})        # w == 0: filtered out
            if i % 13 in (6, 7, 8):
                dets.append({'category': '1', 'conf': 0.7, 'bbox': [0.5, 0.3, -0.1, 0.2]})       # negative w: malformed for get_iou
            order = rng.permutation(len(dets))
            images.append({'file': name, 'detections': [dets[j] for j in order]})
        images.insert(len(images) - 3, {'file': '{}{}broken.jpg'.format(cam, '/' if cam else ''), 'failure': 'Failure image access'})
        images.insert(len(images) - 7, {'file': '{}{}empty.JPG'.format(cam, '/' if cam else ''), 'detections': []})
        images.insert(len(images) - 5, {'file': '{}{}notes.txt'.format(cam, '/' if cam else ''),
                                        'detections': [{'category': '1', 'conf': 0.9, 'bbox': list(spots[0][:4])}]})
    return {'info': {'format_version': '1.4', 'detector': 'seeded'},
            'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'}, 'images': images}


CAMERAS = ['', 'a/c1', 'a/c2', 'b/d/e/c3']


def nested_only(results):
    """the input 'nested': the input 'mixed' without the images that lie in no folder"""
    return dict(results, images=[im for im in results['images'] if '/' in im['file']])


#: case -> (input, options that differ from the reference's defaults)
CASES = {
    'defaults_thr5': ('mixed', {'occurrenceThreshold': 5, 'iouThreshold': 0.85}),
    'agnostic': ('mixed', {'occurrenceThreshold': 5, 'iouThreshold': 0.85, 'categoryAgnosticComparisons': True}),
    'exclude_classes': ('mixed', {'occurrenceThreshold': 4, 'iouThreshold': 0.8, 'excludeClasses': [2, 3]}),
    'size_limits': ('mixed', {'occurrenceThreshold': 3, 'iouThreshold': 0.8, 'minSuspiciousDetectionSize': 0.015,
                              'maxSuspiciousDetectionSize': 0.05}),
    'confidence_window': ('mixed', {'occurrenceThreshold': 3, 'iouThreshold': 0.8, 'confidenceMin': 0.25, 'confidenceMax': 0.8}),
    'levels_from_leaf': ('nested', {'occurrenceThreshold': 6, 'iouThreshold': 0.85, 'nDirLevelsFromLeaf': 1}),
    'max_images': ('nested', {'occurrenceThreshold': 4, 'iouThreshold': 0.85, 'maxImagesPerFolder': 21}),
    'no_sort': ('mixed', {'occurrenceThreshold': 4, 'iouThreshold': 0.75, 'smartSort': None}),
    'exclude_folders': ('nested', {'occurrenceThreshold': 4, 'iouThreshold': 0.85, 'excludeFolders': ['a/c2']}),
    'low_iou_multi_match': ('nested', {'occurrenceThreshold': 2, 'iouThreshold': 0.5}),
    # the marked results of 'defaults_thr5' go in again (negative confidences), with a lower threshold
    'marked_once': ('marked:defaults_thr5', {'occurrenceThreshold': 3, 'iouThreshold': 0.85}),
}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _AnyAttr(types.ModuleType):
    """stand-in for cv2: the reference reads constants of it while it is imported, and nothing of it on this path"""

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return 0


class Index:
    """stand-in for fastquadtree.pyqtree.Index: every item whose rectangle touches the query"""

    def __init__(self, bbox=None, **kwargs):
        self.items = []

    def insert(self, item, bbox):
        self.items.append((item, tuple(bbox)))

    def intersect(self, bbox):
        l, b, r, t = bbox
        return [item for item, (il, ib, ir, it) in self.items if not (ir < l or il > r or it < b or ib > t)]


def import_reference(root):
    sys.path.insert(0, root)
    for name in ('cv2', 'jsonpickle', 'humanfriendly'):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = _AnyAttr(name) if name == 'cv2' else types.ModuleType(name)
    if not hasattr(sys.modules['jsonpickle'], 'set_encoder_options'):
        sys.modules['jsonpickle'].set_encoder_options = lambda *a, **k: None
    try:
        import fastquadtree.pyqtree                                      # noqa: F401
    except ImportError:
        pkg = _stub('fastquadtree')
        pkg.pyqtree = _stub('fastquadtree.pyqtree', Index=Index)
    from megadetector.postprocessing.repeat_detection_elimination import repeat_detections_core as core
    return core


def run_case(core, tmp, results, options):
    path = os.path.join(tmp, 'in.json')
    with open(path, 'w') as f:
        json.dump(results, f)
    o = core.RepeatDetectionOptions()
    o.bWriteFilteringFolder = False
    o.bParallelizeComparisons = True
    o.nWorkers = 1
    o.parallelizationUsesThreads = True
    for k, v in options.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    with redirect_stdout(io.StringIO()):
        res = core.find_repeat_detections(path, output_file_name=os.path.join(tmp, 'out.json'), options=o)
    dirs = list(res.rows_by_directory.keys())
    locations = {}
    for d, locs in zip(dirs, res.suspicious_detections):
        locations[d] = [[[i.filename, i.i_detection] for i in loc.instances] for loc in locs]
    with open(os.path.join(tmp, 'out.json')) as f:
        written = json.load(f)
    signs = []
    for im in written['images']:
        dets = im.get('detections')
        signs.append(None if dets is None else [1 if d['conf'] < 0 else 0 for d in dets])
    # the writer's rounding must have been the identity, or the signs say nothing about our unrounded output
    for a, b in zip(results['images'], written['images']):
        assert a['file'] == b['file']
        for da, db in zip(a.get('detections') or [], b.get('detections') or []):
            assert da['bbox'] == db['bbox'] and abs(da['conf']) == abs(db['conf']), (a['file'], da, db)
    return {'dirs': dirs, 'locations': locations, 'negative': signs}, written


def main(root):
    core = import_reference(root)
    mixed = make_scene(11, CAMERAS, 14)
    inputs = {'mixed': mixed, 'nested': nested_only(mixed)}
    out = {'inputs': {'mixed': mixed}, 'cases': {}}
    marked = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (inp, options) in CASES.items():
            if inp.startswith('marked:'):
                base = CASES[inp[7:]][0]
                results = copy.deepcopy(inputs[base])
                for im, neg in zip(results['images'], marked[inp[7:]]):
                    for d, s in zip(im.get('detections') or [], neg or []):
                        d['conf'] = -d['conf'] if s and d['conf'] >= 0 else d['conf']
            else:
                results = copy.deepcopy(inputs[inp])
            expected, _ = run_case(core, tmp, results, options)
            marked[name] = expected['negative']
            out['cases'][name] = {'input': inp, 'options': options, **expected}
            n_loc = sum(len(v) for v in expected['locations'].values())
            n_inst = sum(len(c) for v in expected['locations'].values() for c in v)
            n_neg = sum(sum(s) for s in expected['negative'] if s)
            print('{}: {} dirs, {} suspicious candidates, {} instances, {} negative confidences'.format(
                name, len(expected['dirs']), n_loc, n_inst, n_neg))
    path = os.path.join(HERE, 'rde_reference.json')
    with open(path, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
    print('wrote {} ({} bytes)'.format(path, os.path.getsize(path)))


if __name__ == '__main__':
    main(sys.argv[1])
