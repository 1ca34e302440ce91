"""
Generates tests/golden/preview_reference.json by running the *real* reference code: visualization_utils.resize_image,
render_detection_bounding_boxes and visualize_detector_output.visualize_detector_output itself.  The reference cannot travel
with the tests, so what it computes is committed as a small fixture together with this script.

What is exercised from the reference:
  * visualization_utils.resize_image on blank images of a table of sizes: the target sizes (None where it asserts)
  * visualize_detector_output on seeded PNG files in a scratch folder, once per option set: which images get a file and
    under which name, and -- with detector_label_map='no_detection_labels', so that no font enters -- the SHA-256 of the
    pixels of every file it writes (PNG in, PNG out: no JPEG codec enters either).  The run that blurs people needs the
    label map, so there the script's call of render_detection_bounding_boxes is passed on with label_map=None
  * render_detection_bounding_boxes with draw_bounding_boxes_on_image replaced by a recorder: the order the boxes are drawn
    in, their classes and their label strings

cv2, jsonpickle and humanfriendly are absent here and are stubbed as empty modules, as are three reference modules that
visualize_detector_output imports for paths this script never takes (run_detector, wi_taxonomy_utils,
write_html_image_list): nothing on this path touches them.

Run:  python tests/golden/gen_preview_golden_from_reference.py <folder that holds the reference's megadetector package>
"""

import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [(2048, 1536, 1000), (1920, 1080, 1000), (1000, 750, 1000), (1000, 751, 1000), (333, 500, 166), (3, 7, 1000), (4000, 3, 1000),
         (5000, 2, 1000), (4032, 3024, 1000), (1333, 1001, 1000), (999, 1000, 1000), (640, 480, -1), (640, 480, None), (97, 61, 40),
         (3001, 17, 1000), (1280, 1024, 300), (720, 1280, 1000), (2592, 1944, 1000), (1000, 3, 1000), (7, 7, 3)]

#: name -> (width, height, seed, detections); the names exercise the three replaced characters
IMAGES = {
    'a.png': (200, 150, 1, [{'category': '1', 'conf': 0.93, 'bbox': [0.1, 0.3, 0.2, 0.25]}, {'category': '2', 'conf': 0.5, 'bbox': [0.5, 0.01, 0.2, 0.3]},
                            {'category': '3', 'conf': 0.8, 'bbox': [0.02, 0.0, 0.3, 0.99]}, {'category': '1', 'conf': 0.3, 'bbox': [0.9, 0.5, 0.09, 0.2]},
                            {'category': '2', 'conf': 0.31, 'bbox': [0.15, 0.35, 0.3, 0.3]}, {'category': '1', 'conf': 0.31, 'bbox': [-0.1, -0.1, 1.3, 1.3]},
                            {'category': '1', 'conf': 0.1, 'bbox': [0.4, 0.4, 0.1, 0.1]}]),
    'sub/b.png': (97, 61, 2, [{'category': '2', 'conf': 0.6, 'bbox': [0.2, 0.2, 0.5, 0.6]}, {'category': '1', 'conf': 0.6, 'bbox': [0.3, 0.1, 0.5, 0.6]}]),
    'sub/deep:er/c.png': (120, 90, 3, [{'category': '1', 'conf': 0.12, 'bbox': [0.2, 0.2, 0.5, 0.6]}]),
    'd.png': (64, 48, 4, []),
    'failed.png': (64, 48, 5, None),
}

OPTION_SETS = {
    'defaults': {},
    'width_80': {'output_image_width': 80},
    'no_resize_detections_only': {'output_image_width': -1, 'render_detections_only': True},
    'preserve_paths_threshold': {'preserve_path_structure': True, 'confidence_threshold': 0.4, 'output_image_width': 150},
    'thick_expanded': {'box_thickness': 0.02, 'box_expansion': 10, 'output_image_width': 300},
    'blur_people': {'category_names_to_blur': ['person'], 'output_image_width': 160},
}


def seeded_image(width, height, seed):
    return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference(root):
    sys.path.insert(0, root)
    for name in ('cv2', 'jsonpickle', 'humanfriendly'):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                _stub(name)
    import megadetector.utils                                            # noqa: F401
    _stub('megadetector.detection.run_detector', get_typical_confidence_threshold_from_results=lambda results: 0.2)
    _stub('megadetector.utils.wi_taxonomy_utils', load_md_or_speciesnet_file=None)
    megadetector.utils.write_html_image_list = _stub('megadetector.utils.write_html_image_list')
    import megadetector.visualization.visualization_utils as vis_utils
    import megadetector.visualization.visualize_detector_output as vdo
    return vis_utils, vdo


def main(root):
    vis_utils, vdo = import_reference(root)
    out = {'pillow': Image.__version__, 'target_sizes': [], 'runs': {}, 'draw_order': {}}
    for w, h, tw in SIZES:
        try:
            size = list(vis_utils.resize_image(Image.new('RGB', (w, h)), tw).size)
        except AssertionError:
            size = None
        out['target_sizes'].append({'width': w, 'height': h, 'target_width': tw, 'size': size})

    with tempfile.TemporaryDirectory() as scratch:
        images_dir = os.path.join(scratch, 'images')
        for name, (w, h, seed, _) in IMAGES.items():
            path = os.path.join(images_dir, name)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(seeded_image(w, h, seed)).save(path)
        entries = []
        for name, (w, h, seed, dets) in IMAGES.items():
            e = {'file': name}
            if dets is None:
                e['failure'] = 'Failure image access'
            else:
                e['detections'] = dets
            entries.append(e)
        results = {'images': entries, 'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'}, 'info': {}}
        for key, kw in OPTION_SETS.items():
            out_dir = os.path.join(scratch, 'out_' + key)
            if 'category_names_to_blur' in kw:
                # the script needs the category names to find what to blur, so it gets the label map, and its call of
                # render_detection_bounding_boxes is made with label_map=None instead: still no font
                real_render = vis_utils.render_detection_bounding_boxes
                vis_utils.render_detection_bounding_boxes = lambda dets, image, label_map=None, **k: real_render(dets, image, label_map=None, **k)
                try:
                    paths = vdo.visualize_detector_output(results, out_dir, images_dir=images_dir, parallelize_rendering=False, **kw)
                finally:
                    vis_utils.render_detection_bounding_boxes = real_render
            else:
                paths = vdo.visualize_detector_output(results, out_dir, images_dir=images_dir, parallelize_rendering=False,
                                                      detector_label_map='no_detection_labels', **kw)
            files = {}
            for p in paths:
                rel = os.path.relpath(p, out_dir).replace('\\', '/')
                px = np.asarray(Image.open(p).convert('RGB'))
                files[rel] = {'size': [px.shape[1], px.shape[0]], 'sha256': hashlib.sha256(px.tobytes()).hexdigest()}
            out['runs'][key] = {'options': kw, 'files': files}

    recorded = {}

    def recorder(image, boxes, classes, display_strs=None, **kw):
        recorded['boxes'] = np.asarray(boxes).tolist()
        recorded['classes'] = list(classes)
        recorded['labels'] = [list(s) for s in display_strs]
    real = vis_utils.draw_bounding_boxes_on_image
    vis_utils.draw_bounding_boxes_on_image = recorder
    try:
        for name, (w, h, seed, dets) in IMAGES.items():
            if not dets:
                continue
            for threshold in (0.15, 0.4):
                recorded.clear()
                vis_utils.render_detection_bounding_boxes(dets, Image.new('RGB', (w, h)), label_map={'1': 'animal', '2': 'person', '3': 'vehicle'},
                                                          confidence_threshold=threshold)
                out['draw_order']['{}@{}'.format(name, threshold)] = dict(recorded)
    finally:
        vis_utils.draw_bounding_boxes_on_image = real

    with open(os.path.join(HERE, 'preview_reference.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print('wrote preview_reference.json: {} sizes, {} runs, {} draw orders'.format(len(out['target_sizes']), len(out['runs']), len(out['draw_order'])))


if __name__ == '__main__':
    main(sys.argv[1])
