"""
The scene of tests/test_separate_cpu.py and tests/test_gpu_separate.py: a folder of small generated images, a results file over
them and the option sets the reference's separate_detections_into_folders was run with for tests/golden/separate_reference.json
(tests/golden/gen_separate_golden_from_reference.py).  Everything comes from a seed, so any machine rebuilds the scene without
the reference.

The images (at most 96 x 64): 4:4:4, 4:2:2 and 4:2:0 RGB JPEGs at different qualities, one with an EXIF block and a COM segment,
one with EXIF orientation 6, one 'L' JPEG, one PNG, images in a sub-folder with classifications, an image that failed, an entry
whose file is missing, overlapping person boxes, detections exactly at a threshold.  Every box is at least 16 pixels wide and
high after its expansion, so that the default outline of 8 pixels is one the device restates.
"""

import hashlib
import json
import os

import numpy as np
from PIL import Image

SEED = 20240611
DETECTION_CATEGORIES = {'1': 'animal', '2': 'person', '3': 'vehicle'}
CLASSIFICATION_CATEGORIES = {'0': 'deer', '1': 'cow', '2': 'bird', '3': 'bear'}


def _content(rng, w, h):
    """smooth colour fields with some texture: what compresses like a photograph"""
    coarse = rng.integers(0, 256, ((h + 15) // 16 + 1, (w + 15) // 16 + 1, 3)).astype(np.float64)
    ys, xs = np.arange(h) / 16.0, np.arange(w) / 16.0
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    a = coarse[y0][:, x0] * (1 - fx) + coarse[y0][:, x0 + 1] * fx
    b = coarse[y0 + 1][:, x0] * (1 - fx) + coarse[y0 + 1][:, x0 + 1] * fx
    img = a * (1 - fy) + b * fy + rng.normal(0, 6, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _det(category, conf, bbox, classifications=None):
    d = {'category': category, 'conf': conf, 'bbox': bbox}
    if classifications is not None:
        d['classifications'] = classifications
    return d


#: file -> (width, height, how it is saved, detections; None: the image failed)
IMAGES = [
    ('a444.jpg', 96, 64, dict(quality=90, subsampling=0), [_det('1', 0.9, [0.1, 0.2, 0.5, 0.6])]),
    ('a422.jpg', 90, 61, dict(quality=80, subsampling=1), [_det('2', 0.8, [0.05, 0.1, 0.5, 0.7]), _det('2', 0.6, [0.3, 0.25, 0.6, 0.7])]),
    ('a420.jpg', 64, 48, dict(quality=75), [_det('3', 0.7, [0.2, 0.2, 0.6, 0.6])]),
    ('exif_com.jpg', 96, 64, dict(quality=85, subsampling=1, exif={271: 'a camera trap', 306: '2021:03:04 05:06:07'}, comment=b'station 12'),
     [_det('1', 0.85, [0.02, 0.1, 0.4, 0.8]), _det('2', 0.75, [0.5, 0.05, 0.45, 0.9])]),
    ('rot6.jpg', 96, 64, dict(quality=88, subsampling=2, exif={274: 6, 271: 'turned'}), [_det('2', 0.9, [0.1, 0.1, 0.6, 0.5]), _det('1', 0.5, [0.3, 0.5, 0.6, 0.45])]),
    ('grey.jpg', 80, 60, dict(quality=82, mode='L'), [_det('1', 0.6, [0.25, 0.2, 0.5, 0.6])]),
    ('pic.png', 72, 56, dict(), [_det('2', 0.7, [0.1, 0.1, 0.7, 0.8])]),
    ('sub/deer.jpg', 96, 64, dict(quality=92, subsampling=1), [_det('1', 0.9, [0.2, 0.2, 0.5, 0.6], [['0', 0.9], ['2', 0.05]])]),
    ('sub/multi.jpg', 96, 64, dict(quality=70, subsampling=0),
     [_det('1', 0.8, [0.05, 0.1, 0.4, 0.7], [['0', 0.8]]), _det('1', 0.7, [0.5, 0.2, 0.45, 0.7], [['1', 0.9]])]),
    ('sub/bird.jpg', 64, 48, dict(quality=75), [_det('1', 0.8, [0.2, 0.1, 0.6, 0.8], [['2', 0.95]])]),
    ('sub/edge.jpg', 64, 48, dict(quality=75, subsampling=1), [_det('1', 0.9, [0.1, 0.1, 0.7, 0.8], [['0', 0.75]])]),
    ('empty.jpg', 64, 48, dict(quality=75), [_det('1', 0.1, [0.2, 0.2, 0.5, 0.5])]),
    ('blank.jpg', 64, 48, dict(quality=75), []),
    ('thresh.jpg', 96, 64, dict(quality=95, subsampling=1), [_det('1', 0.2, [0.1, 0.1, 0.5, 0.6]), _det('3', 0.19999, [0.4, 0.3, 0.5, 0.6])]),
    ('failed.jpg', 64, 48, dict(quality=75), None),
    ('all3.jpg', 96, 64, dict(quality=60, subsampling=1),
     [_det('1', 0.95, [0.0, 0.1, 0.35, 0.8]), _det('2', 0.9, [0.3, 0.05, 0.4, 0.9]), _det('3', 0.8, [0.6, 0.2, 0.4, 0.7])]),
]
MISSING = 'sub/missing.jpg'

#: name -> attributes set on the options (allow_missing_files is on everywhere: the scene has an entry without a file)
OPTION_SETS = {
    'defaults': {},
    'per_category': {'category_name_to_threshold': {'animal': 0.55, 'person': 0.85, 'vehicle': None}, 'threshold': 0.65},
    'skip_empty': {'skip_empty_images': True, 'remove_empty_folders': True},
    'move': {'move_images': True},
    'render_boxes': {'render_boxes': True},
    'blur_and_boxes': {'render_boxes': True, 'category_names_to_blur': 'person', 'line_thickness': 3, 'box_expansion': 0},
    'blur_only': {'category_names_to_blur': ['person', 'vehicle']},
    'classification_labels': {'classification_thresholds': 'deer=0.75,cow=0.75', 'render_boxes': True, 'show_box_labels': True,
                              'line_thickness': 2},
    'classification_folders': {'classification_thresholds': {'deer': 0.75, 'cow': 0.75}},
    'no_overwrite': {'allow_existing_directory': True, 'overwrite': False, 'render_boxes': True},
}
#: what the 'no_overwrite' set finds in the target tree before it runs: files that must survive as they are
EXISTING = {'animals/a444.jpg': b'an older copy', 'notes.txt': b'kept'}

#: name -> (attributes, change to the results or the target folder) of the runs that must raise
ERROR_CASES = {
    'move_and_render': {'move_images': True, 'render_boxes': True},
    'move_and_blur': {'move_images': True, 'category_names_to_blur': 'person'},
    'target_not_empty': {'_existing': True},
    'absolute_path': {'_absolute': True},
    'bad_classification_threshold': {'classification_thresholds': 'deer=high'},
    'unknown_classification_category': {'classification_thresholds': 'moose=0.5'},
    'no_classification_results': {'classification_thresholds': 'deer=0.5', '_no_classification_categories': True},
    'missing_file': {'allow_missing_files': False},
}

MANIPULATING = [k for k, v in OPTION_SETS.items() if v.get('render_boxes') or v.get('category_names_to_blur')]


def results():
    images = []
    for name, _, _, _, dets in IMAGES:
        images.append({'file': name, 'detections': dets} if dets is not None else {'file': name, 'failure': 'Failure image access'})
    images.insert(9, {'file': MISSING, 'detections': [_det('1', 0.9, [0.1, 0.1, 0.5, 0.5])]})
    return {'info': {'detector': 'md_v5a.0.0.pt', 'format_version': '1.4'}, 'detection_categories': dict(DETECTION_CATEGORIES),
            'classification_categories': dict(CLASSIFICATION_CATEGORIES), 'images': images}


def build(folder):
    """writes the images below `folder` and results.json beside it; -> (image folder, results file)"""
    rng = np.random.default_rng(SEED)
    image_folder = os.path.join(folder, 'images')
    for name, w, h, how, _ in IMAGES:
        how = dict(how)
        path = os.path.join(image_folder, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        rgb = _content(rng, w, h)
        image = Image.fromarray(rgb)
        if how.pop('mode', None) == 'L':
            image = image.convert('L')
        if 'exif' in how:
            exif = Image.Exif()
            for tag, value in how['exif'].items():
                exif[tag] = value
            how['exif'] = exif
        image.save(path, **how)
    results_file = os.path.join(folder, 'results.json')
    with open(results_file, 'w') as f:
        json.dump(results(), f, indent=1)
    return image_folder, results_file


def apply_options(options, image_folder, results_file, output_folder, attributes):
    options.results_file, options.base_input_folder, options.base_output_folder = results_file, image_folder, output_folder
    options.allow_missing_files = True
    for k, v in attributes.items():
        if k.startswith('_'):
            continue
        setattr(options, k, dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v)
    return options


def prepare_error_case(attributes, results_file, output_folder):
    """the changes an error case makes to the scene: -> the results file to use"""
    if attributes.get('_existing'):
        os.makedirs(output_folder, exist_ok=True)
        with open(os.path.join(output_folder, 'old.txt'), 'w') as f:
            f.write('old')
    if attributes.get('_absolute') or attributes.get('_no_classification_categories'):
        with open(results_file) as f:
            data = json.load(f)
        if attributes.get('_absolute'):
            data['images'][3]['file'] = '/somewhere/' + data['images'][3]['file']
        else:
            del data['classification_categories']
        results_file = results_file[:-5] + '.changed.json'
        with open(results_file, 'w') as f:
            json.dump(data, f)
    return results_file


def prepare_existing(output_folder):
    for name, data in EXISTING.items():
        path = os.path.join(output_folder, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'wb') as f:
            f.write(data)


def segments(data):
    """the marker bytes of a JPEG's segments up to SOS, in order"""
    out, p = [], 2
    while p + 4 <= len(data) and data[p] == 0xFF:
        out.append(data[p + 1])
        if data[p + 1] == 0xDA:
            break
        p += 2 + ((data[p + 2] << 8) | data[p + 3])
    return out


def source_hashes(image_folder):
    """SHA-256 -> relative name of every scene image (taken before a run that moves them)"""
    sources = {}
    for root, _, names in os.walk(image_folder):
        for n in names:
            with open(os.path.join(root, n), 'rb') as f:
                sources[hashlib.sha256(f.read()).hexdigest()] = os.path.relpath(os.path.join(root, n), image_folder).replace(os.sep, '/')
    return sources


def describe_tree(output_folder, sources):
    """relative path -> what the file is: 'copy_of' names the scene image it is a byte copy of (sources: source_hashes), else
    None; its SHA-256 and size in bytes and, for a JPEG that is no copy, sampling, tables, dimensions and segment list (read
    by Pillow).  An empty folder is listed with a trailing slash."""
    tree = {}
    for root, dirs, names in os.walk(output_folder):
        rel_root = os.path.relpath(root, output_folder).replace(os.sep, '/')
        if not dirs and not names:
            tree[rel_root + '/'] = {'empty_folder': True}
        for n in names:
            path = os.path.join(root, n)
            with open(path, 'rb') as f:
                data = f.read()
            sha = hashlib.sha256(data).hexdigest()
            rel = os.path.relpath(path, output_folder).replace(os.sep, '/')
            entry = {'sha256': sha, 'bytes': len(data), 'copy_of': sources.get(sha)}
            if entry['copy_of'] is None and data[:2] == b'\xff\xd8':
                im = Image.open(path)
                entry['size'] = list(im.size)
                entry['quant'] = {str(k): [int(v) for v in t] for k, t in im.quantization.items()}
                entry['sampling'] = [list(layer[1:3]) for layer in im.layer]
                entry['segments'] = segments(data)
            tree[rel] = entry
    return tree
