"""
Generates tests/golden/tiled_reference.json by running the *real* reference detection/run_tiled_inference.py
(read-only checkout next to this repository) in the build container.  The reference cannot travel to the GPU box, so
what it emits is committed as a fixture together with this script; tests/test_tiled_cpu.py asserts that
megadetector_amd.run_tiled_inference reproduces it exactly.

What runs from the reference itself:
  * get_patch_boundaries on a grid of (image size, tile size, overlap) cases, and its assertion for an image smaller
    than the tile;
  * run_tiled_inference end to end (tile extraction with PIL, write_results_to_file, the mapping of tile detections to
    the image with its rounding, the failure records, in_place_nms, the JSON files) on a folder of small PNGs, with
      - load_and_run_detector_batch bound to a function that returns CANNED tile-level detections keyed on the tile's
        name (image, x, y): the fixture does not depend on JPEG codec versions;
      - torchvision.ops.nms bound to the oracle's greedy NMS (oracle/pre_post.py, pinned by nms_reference.npz).
The canned detections are part of the fixture: the test feeds the same ones to the package's merge stage.

Third-party modules absent from this container are stubbed as for gen_host_golden_from_reference.py.

Run (build container only):  python tests/golden/gen_tiled_golden_from_reference.py
"""

import glob
import io
import json
import os
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, HERE)
sys.path.insert(0, '/root/reference')

from gen_host_golden_from_reference import import_reference, TIME_RE, TIME_PLACEHOLDER  # noqa: E402

# (image (w, h), tile (w, h), overlap)
BOUNDARY_CASES = [
    [[1280, 1280], [1280, 1280], 0.5],          # size == tile
    [[1281, 1281], [1280, 1280], 0.5],          # size = tile + 1
    [[3200, 2560], [1280, 1280], 0.5],          # exact multiple of the stride
    [[6000, 4000], [1280, 1280], 0.0],
    [[6000, 4000], [1280, 1280], 0.25],
    [[6000, 4000], [1280, 1280], 0.5],
    [[6000, 4000], [1280, 1280], 0.8],
    [[5000, 3000], [1600, 1200], 0.5],          # non-square tiles
    [[4100, 3000], [640, 960], 0.25],
    [[15, 10], [10, 10], 0.0],                  # the docstring's "15 px wide, stride 10"
    [[1000, 2000], [1280, 1280], 0.5],          # image smaller than the tile
]

TILE = [16, 12]
OVERLAP = 0.5
# (relative name, w, h, seed)
IMAGES = [['a.png', 40, 30, 1], ['sub/B 2.png', 33, 25, 2], ['small.png', 10, 30, 3], ['c.png', 16, 12, 4],
          ['empty.png', 24, 12, 5]]
# objects in image pixels (x, y, w, h, conf, category): every tile that contains one reports it -> duplicates with
# equal scores across overlapping tiles
OBJECTS = {
    'a.png': [(18, 8, 5, 3, 0.9, '1'), (9, 7, 4, 4, 0.9, '2'), (30, 20, 6, 6, 0.314, '1'), (19, 9, 5, 3, 0.52, '3'),
              (2, 2, 3, 3, 0.0071, '1')],
    'sub/B 2.png': [(10, 8, 5, 4, 0.777, '2'), (17, 13, 7, 5, 0.777, '2'), (11, 8, 5, 4, 0.778, '1')],
    # tile == image: a nested pair whose IoU is 0.045 / 0.1 (0.45 in exact arithmetic: at the threshold), equal scores
    'c.png': [(0, 0, 8, 2.4, 0.6, '1'), (0, 0, 7.2, 1.2, 0.6, '2'), (8, 6, 4, 3, 0.6, '3')],
    'empty.png': [],
}
FAILED_TILE = ('a.png', 8, 6)       # used by the second run only


def canned_for_tile(image, x, y):
    dets = []
    for ox, oy, ow, oh, conf, cat in OBJECTS[image]:
        if ox >= x and oy >= y and ox + ow <= x + TILE[0] and oy + oh <= y + TILE[1]:
            dets.append({'category': cat, 'conf': conf,
                         'bbox': [round((ox - x) / TILE[0], 4), round((oy - y) / TILE[1], 4),
                                  round(ow / TILE[0], 4), round(oh / TILE[1], 4)]})
    return dets


def run_reference(rti, folder, tiling, with_failure):
    canned = {}

    def fake_batch(model_file, patch_file_names, **kwargs):
        out = []
        by_clean = {rti.path_utils.clean_filename(n, char_limit=None, force_lower=True): n for n, _, _, _ in IMAGES}
        for fn in patch_file_names:
            name = os.path.splitext(os.path.basename(fn))[0]
            clean, xs, ys = name.rsplit('_', 2)
            image, x, y = by_clean[clean], int(xs), int(ys)
            if with_failure and (image, x, y) == FAILED_TILE:
                canned[name] = {'failure': 'inference failure'}
                out.append({'file': fn, 'failure': 'inference failure'})
                continue
            dets = canned_for_tile(image, x, y)
            canned[name] = {'detections': dets}
            out.append({'file': fn, 'detections': [dict(d, bbox=list(d['bbox'])) for d in dets],
                        'max_detection_conf': max([d['conf'] for d in dets] + [0.0])})
        return out

    rti.load_and_run_detector_batch = fake_batch
    out_file = os.path.join(tiling, '..', 'out_{}.json'.format(int(with_failure)))
    record = {'canned': canned}
    try:
        with redirect_stdout(io.StringIO()):
            rti.run_tiled_inference('md_v5a.0.0.pt', folder, tiling, out_file, tile_size_x=TILE[0], tile_size_y=TILE[1],
                                    tile_overlap=OVERLAP)
    except Exception as e:
        record['raises'] = type(e).__name__
        return record
    read = lambda p: TIME_RE.sub(TIME_PLACEHOLDER, open(p, 'r', encoding='utf-8').read())
    record['output_text'] = read(out_file)
    record['pre_nms_text'] = read(glob.glob(os.path.join(tiling, '*_image_level_results_pre_nms.json'))[0])
    record['patch_level_text'] = read(glob.glob(os.path.join(tiling, '*_patch_level_results.json'))[0])
    info = json.load(open(glob.glob(os.path.join(tiling, '*_patch_info.json'))[0]))
    for im in info:
        for p in im['patches']:
            p['patch_fn'] = os.path.relpath(p['patch_fn'], tiling)
        if im['error'] is not None:
            im['error'] = im['error'].split('\n')[0]
    record['patch_info'] = info
    record['patch_info_name'] = os.path.basename(glob.glob(os.path.join(tiling, '*_patch_info.json'))[0]).replace(
        os.path.basename(folder), '<folder>')
    return record


def main():
    from PIL import Image
    import torch
    from oracle import pre_post as O
    import_reference()
    sys.modules['torchvision'].ops.nms = lambda b, s, t: O._greedy_nms(b.to(torch.float32), s.to(torch.float32), t)
    yv = sys.modules.setdefault('megadetector.detection.run_inference_with_yolov5_val',
                                type(sys)('megadetector.detection.run_inference_with_yolov5_val'))
    yv.YoloInferenceOptions = object
    yv.run_inference_with_yolo_val = None
    import megadetector.detection.run_tiled_inference as rti

    golden = {'boundaries': [], 'tile': TILE, 'overlap': OVERLAP, 'images': IMAGES}
    for image_size, tile, overlap in BOUNDARY_CASES:
        stride = (round(tile[0] * (1.0 - overlap)), round(tile[1] * (1.0 - overlap)))
        case = {'image_size': image_size, 'tile': tile, 'overlap': overlap}
        try:
            case['positions'] = [list(p) for p in rti.get_patch_boundaries(image_size, tile, stride)]
        except AssertionError:
            case['positions'] = None
        golden['boundaries'].append(case)
    golden['default_stride_positions'] = [list(p) for p in rti.get_patch_boundaries([3000, 2000], [1280, 1280])]
    golden['patch_name'] = rti.patch_info_to_patch_name('a.jpg', 10, 20)

    for key, with_failure in (('run', False), ('run_with_failed_tile', True)):
        with tempfile.TemporaryDirectory() as tmp:
            folder = os.path.join(tmp, 'Survey Imgs')
            tiling = os.path.join(tmp, 'tiling')
            for name, w, h, seed in IMAGES:
                p = os.path.join(folder, name)
                os.makedirs(os.path.dirname(p), exist_ok=True)
                Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
            golden[key] = run_reference(rti, folder, tiling, with_failure)
    out = os.path.join(HERE, 'tiled_reference.json')
    with open(out, 'w', newline='\n') as f:
        json.dump(golden, f, indent=1)
    print('wrote', out, os.path.getsize(out), 'bytes;', 'run with a failed tile:',
          golden['run_with_failed_tile'].get('raises', 'completed'))


if __name__ == '__main__':
    main()
