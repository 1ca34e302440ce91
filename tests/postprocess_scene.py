"""
The scene of tests/test_postprocess_cpu.py and tests/test_gpu_postprocess.py: a folder of small generated images, a results
file over them and the option sets the reference's process_batch_results was run with for
tests/golden/postprocess_reference.json (tests/golden/gen_postprocess_reference.py).  Everything comes from a seed, so any
machine rebuilds the scene without the reference.

The images (61 x 97 up to 333 x 250, odd sizes among them): 4:4:4, 4:2:2 and 4:2:0 RGB JPEGs, one 'L' JPEG, one with EXIF
orientation 6, one PNG, nested folders, a name with a space and a '#', a path the results file writes with backslashes, an
image that failed, an entry whose file is missing; images with no, one and several boxes of the three categories around the
thresholds, four of them with classifications above, at and below 0.5; fields some images carry and others lack.  Every box
is at least a fifth of the image wide and high, so that at every width the sets render at its outline is one the device restates.
"""

import hashlib
import json
import os

import numpy as np
from PIL import Image

from separate_scene import _content, _det

SEED = 20240915
DETECTION_CATEGORIES = {'1': 'animal', '2': 'person', '3': 'vehicle'}
CLASSIFICATION_CATEGORIES = {'0': 'Deer', '1': 'cow', '2': 'red fox', '3': 'bear'}
CLASSIFICATION_DESCRIPTIONS = {'0': 'mammalia;cervidae;deer', '1': 'mammalia;bovidae;cow', '2': 'mammalia;canidae;red fox',
                               '3': 'mammalia;ursidae;bear'}

#: file -> (width, height, how it is saved, detections; None: the image failed, further fields of its entry)
IMAGES = [
    ('a444.jpg', 333, 250, dict(quality=90, subsampling=0), [_det('1', 0.9, [0.1, 0.2, 0.5, 0.6])], {'datetime': '2021-03-04 05:06:07', 'seq_num': 3}),
    ('a422.jpg', 61, 97, dict(quality=80, subsampling=1), [_det('2', 0.8, [0.05, 0.1, 0.5, 0.7]), _det('2', 0.6, [0.3, 0.25, 0.6, 0.7])], {}),
    ('a420.jpg', 200, 150, dict(quality=75), [_det('3', 0.7, [0.2, 0.2, 0.6, 0.6])], {'datetime': '2021-03-04 05:07:00', 'location': None}),
    ('rot6.jpg', 160, 121, dict(quality=88, subsampling=2, exif={274: 6, 271: 'turned'}),
     [_det('2', 0.9, [0.1, 0.1, 0.6, 0.5]), _det('1', 0.5, [0.3, 0.5, 0.6, 0.45])], {'seq_num': 4}),
    ('grey.jpg', 127, 95, dict(quality=82, mode='L'), [_det('1', 0.6, [0.25, 0.2, 0.5, 0.6])], {'location': 'ridge'}),
    ('pic.png', 144, 111, dict(), [_det('2', 0.7, [0.1, 0.1, 0.7, 0.8])], {}),
    ('sub/deer one#1.jpg', 180, 135, dict(quality=92, subsampling=1), [_det('1', 0.9, [0.2, 0.2, 0.5, 0.6], [['0', 0.9], ['2', 0.05]])], {}),
    ('sub/nested/multi.jpg', 240, 181, dict(quality=70, subsampling=0),
     [_det('1', 0.8, [0.05, 0.1, 0.4, 0.7], [['0', 0.8]]), _det('1', 0.7, [0.5, 0.2, 0.45, 0.7], [['1', 0.9], ['0', 0.4]])], {}),
    ('sub/nested/fox.jpg', 99, 75, dict(quality=75), [_det('1', 0.8, [0.2, 0.1, 0.6, 0.8], [['2', 0.45]])], {}),
    ('sub/edge.jpg', 120, 90, dict(quality=75, subsampling=1),
     [_det('1', 0.9, [0.1, 0.1, 0.7, 0.8], [['3', 0.5]]), _det('2', 0.3, [0.5, 0.3, 0.4, 0.5])], {}),
    ('empty.jpg', 100, 80, dict(quality=75), [_det('1', 0.1, [0.2, 0.2, 0.5, 0.5])], {}),
    ('blank.jpg', 64, 97, dict(quality=75), [], {}),
    ('thresh.jpg', 150, 113, dict(quality=95, subsampling=1), [_det('1', 0.2, [0.1, 0.1, 0.5, 0.6]), _det('3', 0.19999, [0.4, 0.3, 0.5, 0.6])], {}),
    ('almost.jpg', 111, 83, dict(quality=85), [_det('2', 0.17, [0.1, 0.2, 0.4, 0.6]), _det('3', 0.16, [0.5, 0.2, 0.4, 0.6])], {}),
    ('failed.jpg', 64, 48, dict(quality=75), None, {}),
    ('all3.jpg', 320, 240, dict(quality=60, subsampling=1),
     [_det('1', 0.95, [0.0, 0.1, 0.35, 0.8]), _det('2', 0.9, [0.3, 0.05, 0.4, 0.9]), _det('3', 0.8, [0.6, 0.2, 0.4, 0.7]),
      _det('1', 0.18, [0.4, 0.5, 0.3, 0.4])], {}),
]
MISSING = 'sub/gone.jpg'
BACKSLASHED = 'sub/nested/fox.jpg'               # written as sub\nested\fox.jpg in the results file

_NO_LINKS = {'link_images_to_originals': False, 'api_output_filename_replacements': {'gone': 'lost'}}

#: name -> attributes set on the options (num_images_to_sample is -1 unless a set says otherwise: the scene is the sample)
OPTION_SETS = {
    'defaults': {},
    'float_threshold': {'confidence_threshold': 0.5},
    'dict_threshold': {'confidence_threshold': {'animal': 0.55, 'person': 0.85, 'default': 0.65}},
    'almost_default': {'include_almost_detections': True},
    'almost_explicit': {'include_almost_detections': True, 'almost_detection_confidence_threshold': 0.1,
                        'confidence_threshold': {'animal': 0.55, 'default': 0.25}},
    'not_separated': {'separate_detections_by_category': False},
    'sample_6_seed_0': {'num_images_to_sample': 6, 'sample_seed': 0},
    'sample_6_seed_7': {'num_images_to_sample': 6, 'sample_seed': 7},
    'by_confidence': {'html_sort_order': 'confidence'},
    'pages_of_3': {'max_figures_per_html_file': 3},
    'bypass_non_detections': {'rendering_bypass_sets': ['non_detections']},
    'classification_report': {'sort_classification_results_by_count': True, 'category_name_to_sort_weight': {'cow': 1, 'unreliable': 2},
                              'include_category_descriptions_with_global_counts': True, 'job_name_string': 'a job',
                              'model_version_string': 'a model', 'footer_text': '<p>footer</p>', 'output_html_encoding': 'utf-8'},
    'fields_list': {'additional_image_fields_to_display': ['datetime', 'seq_num', 'location', 'nowhere'], 'include_size_range': True},
    'fields_dict': {'additional_image_fields_to_display': {'seq_num': 'Sequence', 'location': 'Site'}, 'include_size_range': True,
                    'line_thickness': 2, 'box_expansion': 3},
    'width_120': dict(_NO_LINKS, viz_target_width=120),
    'width_400': dict(_NO_LINKS, viz_target_width=400),
    'width_none': dict(_NO_LINKS, viz_target_width=None),
}
WIDTH_SETS = ('width_120', 'width_400', 'width_none')


def results():
    images = []
    for name, _, _, _, dets, fields in IMAGES:
        entry = {'file': name.replace('/', '\\') if name == BACKSLASHED else name}
        if dets is None:
            entry['failure'] = 'Failure image access'
        else:
            entry['detections'] = dets
        entry.update(fields)
        images.append(entry)
    images.insert(9, {'file': MISSING, 'detections': [_det('1', 0.9, [0.1, 0.1, 0.5, 0.5])]})
    return {'info': {'detector': 'md_v5a.0.0.pt', 'format_version': '1.4'}, 'detection_categories': dict(DETECTION_CATEGORIES),
            'classification_categories': dict(CLASSIFICATION_CATEGORIES),
            'classification_category_descriptions': dict(CLASSIFICATION_DESCRIPTIONS), 'images': images}


def build(folder):
    """writes the images below `folder` and results.json beside it; -> (image folder, results file)"""
    rng = np.random.default_rng(SEED)
    image_folder = os.path.join(folder, 'images')
    for name, w, h, how, _, _ in IMAGES:
        how = dict(how)
        path = os.path.join(image_folder, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        image = Image.fromarray(_content(rng, w, h))
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
    options.md_results_file, options.image_base_dir, options.output_dir = results_file, image_folder, output_folder
    options.num_images_to_sample = -1
    for k, v in attributes.items():
        setattr(options, k, dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v)
    return options


def scene_hash(image_folder):
    """a hash over the generated source files: the rendered files' hashes hold for this scene only"""
    h = hashlib.sha256()
    for root, dirs, names in os.walk(image_folder):
        dirs.sort()
        for n in sorted(names):
            with open(os.path.join(root, n), 'rb') as f:
                h.update(os.path.relpath(os.path.join(root, n), image_folder).replace(os.sep, '/').encode() + b'\0' + f.read())
    return h.hexdigest()


def describe_output(output_folder, folder):
    """What a run wrote: {'tree': every relative path (a folder without files with a trailing slash), 'html': name -> text of
    every HTML file with `folder`, the scene's own path, replaced by '<tmp>', 'sha256': relative path -> hash of every other
    file}"""
    import urllib.parse
    out = {'tree': [], 'html': {}, 'sha256': {}}
    for root, dirs, names in os.walk(output_folder):
        rel_root = os.path.relpath(root, output_folder).replace(os.sep, '/')
        if not dirs and not names:
            out['tree'].append(rel_root + '/')
        for n in names:
            path = os.path.join(root, n)
            rel = os.path.relpath(path, output_folder).replace(os.sep, '/')
            out['tree'].append(rel)
            with open(path, 'rb') as f:
                data = f.read()
            if n.endswith('.html'):
                text = data.decode('utf-8')
                out['html'][rel] = text.replace(urllib.parse.quote(folder, safe=':/'), '<tmp>').replace(folder, '<tmp>')
            else:
                out['sha256'][rel] = hashlib.sha256(data).hexdigest()
    out['tree'].sort()
    return out
