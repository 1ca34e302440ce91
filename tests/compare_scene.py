"""
The scene of tests/test_compare_cpu.py and tests/test_gpu_compare.py: a folder of a dozen small generated images, three results
files over them with planted disagreements (and a fourth that lacks one image) and the option sets the reference's
compare_batch_results was run with for tests/golden/compare_reference.json (tests/golden/gen_compare_reference.py).
Everything comes from a seed, so any machine rebuilds the scene without the reference.

The images (96 to 400 pixels on a side, odd sizes among them): 4:4:4, 4:2:2 and 4:2:0 RGB JPEGs, one 'L' JPEG, one with EXIF
orientation 6, one PNG, one file in a sub-folder, one whose entry is a failure in B.  Over the three comparisons a-b, a-c and b-c
every one of the five categories is non-empty somewhere and most files land in different categories in different comparisons.
Some detections carry 'transferred_from' (in both orders against the confidences: the reference indexes its custom strings by
the position in the SORTED list) and some carry classifications; c has no classification categories.  top.jpg has boxes
whose labels cannot go above them, bottom.jpg boxes whose labels cannot go below, tall.jpg boxes where neither fits.  One
box of b in thin.jpg is 0.002 of the image wide: thinner than twice any outline at every width, which is the one drawing the
plan hands to the host leg.  Every other box is at least a fifth of the image wide and high.
"""

import json
import os

import numpy as np
from PIL import Image

from postprocess_scene import describe_output, scene_hash  # noqa: F401  (used by the generator and the tests)
from separate_scene import _content, _det

SEED = 20241020
DETECTION_CATEGORIES = {'1': 'animal', '2': 'person', '3': 'vehicle'}
CLASSIFICATION_CATEGORIES = {'0': 'Deer', '1': 'cow', '2': 'red fox'}
PNG = 'pic.png'
THIN = 'thin.jpg'
FAILED_IN_B = 'fail_b.jpg'
MISSING_FROM_B_SHORT = 'c420.jpg'


def _from(det, name):
    return dict(det, transferred_from=name)


#: file -> (width, height, how it is saved, detections in a, in b, in c; None: the image failed)
IMAGES = [
    ('c444.jpg', 400, 300, dict(quality=90, subsampling=0),
     [_det('1', 0.9, [0.1, 0.2, 0.5, 0.6])], [_det('1', 0.85, [0.12, 0.22, 0.5, 0.6])], [_det('1', 0.1, [0.1, 0.2, 0.5, 0.55])]),
    ('c422.jpg', 97, 131, dict(quality=80, subsampling=1),
     [_det('2', 0.8, [0.05, 0.1, 0.5, 0.7])], [], [_det('2', 0.7, [0.3, 0.25, 0.6, 0.7])]),
    ('c420.jpg', 200, 150, dict(quality=75), [], [_det('3', 0.6, [0.2, 0.2, 0.6, 0.6])], []),
    ('grey.jpg', 127, 96, dict(quality=82, mode='L'),
     [_det('1', 0.6, [0.25, 0.2, 0.5, 0.6])], [_det('2', 0.7, [0.2, 0.25, 0.55, 0.6])], [_det('1', 0.5, [0.3, 0.2, 0.5, 0.6])]),
    ('rot6.jpg', 160, 121, dict(quality=88, subsampling=2, exif={274: 6, 271: 'turned'}),
     [_from(_det('2', 0.9, [0.1, 0.1, 0.6, 0.5]), 'merged.left.json'), _det('1', 0.5, [0.3, 0.45, 0.6, 0.45])],
     [_det('2', 0.88, [0.12, 0.1, 0.6, 0.5])],
     [_det('1', 0.2, [0.3, 0.5, 0.6, 0.4]), _from(_det('2', 0.3, [0.1, 0.1, 0.6, 0.5]), 'other')]),
    (PNG, 144, 111, dict(), [_det('2', 0.7, [0.1, 0.1, 0.7, 0.8])], [_det('2', 0.65, [0.15, 0.1, 0.7, 0.8])], []),
    ('sub/deep.jpg', 180, 135, dict(quality=92, subsampling=1),
     [_det('1', 0.9, [0.2, 0.2, 0.5, 0.6], [['0', 0.9], ['2', 0.05]])],
     [_from(_det('1', 0.8, [0.25, 0.2, 0.5, 0.6], [['1', 0.6], ['0', 0.35]]), 'md_v5a.0.0.pt')],
     [_det('1', 0.05, [0.2, 0.2, 0.5, 0.6])]),
    (FAILED_IN_B, 120, 96, dict(quality=75), [_det('1', 0.8, [0.2, 0.2, 0.5, 0.5])], None, [_det('1', 0.7, [0.25, 0.2, 0.5, 0.5])]),
    ('top.jpg', 150, 113, dict(quality=85, subsampling=1),
     [_det('1', 0.9, [0.1, 0.0, 0.5, 0.4])], [_det('1', 0.8, [0.3, 0.01, 0.5, 0.4])], []),
    ('bottom.jpg', 150, 120, dict(quality=85),
     [_det('3', 0.75, [0.1, 0.6, 0.4, 0.4])], [_det('3', 0.7, [0.5, 0.55, 0.4, 0.44])], [_det('3', 0.12, [0.1, 0.6, 0.4, 0.4])]),
    ('tall.jpg', 128, 96, dict(quality=70, subsampling=0),
     [_det('1', 0.6, [0.1, 0.01, 0.4, 0.98])], [_det('1', 0.55, [0.5, 0.0, 0.4, 1.0])], []),
    (THIN, 240, 180, dict(quality=95, subsampling=1),
     [_det('1', 0.9, [0.1, 0.2, 0.4, 0.5])], [_det('1', 0.9, [0.12, 0.2, 0.4, 0.5]), _det('2', 0.5, [0.7, 0.3, 0.002, 0.4])],
     [_det('1', 0.9, [0.1, 0.22, 0.4, 0.5])]),
]

FILES = [name for name, *_ in IMAGES]

#: name -> {'files': the results files compared (two: one pairwise comparison; three: n_way_comparison), 'options': attributes set on
#: the BatchComparisonOptions, 'pairwise': attributes set on the PairwiseBatchComparisonOptions}
OPTION_SETS = {
    'defaults': {},
    'float_thresholds': {'pairwise': {'detection_thresholds_a': 0.5, 'detection_thresholds_b': 0.6}},
    'dict_thresholds': {'pairwise': {'detection_thresholds_a': {'animal': 0.55, 'person': 0.85, 'default': 0.65},
                                     'detection_thresholds_b': {'vehicle': 0.65, 'default': 0.6},
                                     'rendering_confidence_threshold_a': 0.9, 'rendering_confidence_threshold_b': 0.5}},
    'class_agnostic': {'options': {'class_agnostic_comparison': True}},
    'category_names': {'options': {'category_names_to_include': 'animal'}},
    'filenames_to_include': {'options': {'filenames_to_include': ['grey.jpg', 'c444.jpg', 'sub/deep.jpg', 'c420.jpg']}},
    'required_token': {'options': {'required_token': 'c4'}},
    'sample_2_seed_0': {'options': {'max_images_per_category': 2, 'random_seed': 0}},
    'sample_2_seed_7': {'options': {'max_images_per_category': 2, 'random_seed': 7}},
    'width_none': {'options': {'target_width': None}},
    'width_80': {'options': {'target_width': 80}},
    'by_confidence': {'options': {'sort_by_confidence': True}},
    'pages_of_3': {'options': {'max_images_per_page': 3}},
    'display_fn': {'options': {'fn_to_display_fn': {f: 'shown as ' + f.upper() for f in FILES}, 'job_name': 'a job'}},
    'no_parse_links': {'options': {'parse_link_paths': False}},
    'no_category_names': {'options': {'show_category_names_on_detected_boxes': False}},
    'no_classification_categories': {'options': {'show_classification_categories': False}},
    'two_colours': {'options': {'colormap_a': ['Red', 'Gold'], 'colormap_b': ['RoyalBlue', 'Aqua']}},
    'non_matching': {'files': ('a', 'b_short'), 'options': {'error_on_non_matching_lists': False}},
    'n_way': {'files': ('a', 'b', 'c')},
    'n_way_80': {'files': ('a', 'b', 'c'), 'options': {'target_width': 80}},
    'n_way_none': {'files': ('a', 'b', 'c'), 'options': {'target_width': None}},
}
N_WAY_SETS = ('n_way', 'n_way_80', 'n_way_none')       # enlarging (the default of 800), reducing, as they are


def results(which):
    side = {'a': 0, 'b': 1, 'b_short': 1, 'c': 2}[which]
    images = []
    for name, _, _, _, *dets in IMAGES:
        if which == 'b_short' and name == MISSING_FROM_B_SHORT:
            continue
        entry = {'file': name.replace('/', '\\') if (which == 'b' and '/' in name) else name}
        if dets[side] is None:
            entry['failure'] = 'Failure image access'
        else:
            entry['detections'] = dets[side]
        images.append(entry)
    out = {'info': {'format_version': '1.4'}, 'detection_categories': dict(DETECTION_CATEGORIES), 'images': images}
    if which != 'c':
        out['classification_categories'] = dict(CLASSIFICATION_CATEGORIES)
        out['info']['detector'] = {'a': 'md_v5a.0.0.pt', 'b': 'md_v5b.0.0.pt', 'b_short': '5b (short list)'}[which]
    return out


def build(folder):
    """writes the images below `folder`/images and a.json, b.json, b_short.json, c.json beside them; -> (image folder,
    {name: results file})"""
    rng = np.random.default_rng(SEED)
    image_folder = os.path.join(folder, 'images')
    for name, w, h, how, *_ in IMAGES:
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
    files = {}
    for which in ('a', 'b', 'b_short', 'c'):
        files[which] = os.path.join(folder, which + '.json')
        with open(files[which], 'w') as f:
            json.dump(results(which), f, indent=1)
    return image_folder, files


def pack_golden(golden):
    """The recorded runs as the text of tests/golden/compare_reference.json, nothing left out: every distinct HTML text is
    kept once under 'texts' and a set's 'html' names it; a set's 'tree' keeps only what is neither an HTML nor a rendered
    file (a folder without files), the rest being the keys of 'html' and 'sha256'.  One line per text and per set."""
    import hashlib
    texts, lines = {}, []
    for name, record in sorted(golden['sets'].items()):
        html = {}
        for page, text in record['html'].items():
            html[page] = hashlib.sha256(text.encode()).hexdigest()[:12]
            assert texts.setdefault(html[page], text) == text
        files = set(record['html']) | set(record['sha256'])
        packed = dict(record, html=html, tree=[t for t in record['tree'] if t not in files])
        assert sorted(files | set(packed['tree'])) == record['tree']
        lines.append('  {}: {}'.format(json.dumps(name), json.dumps(packed, sort_keys=True)))
    head = {k: v for k, v in golden.items() if k != 'sets'}
    return ('{\n "head": ' + json.dumps(head, sort_keys=True) + ',\n "sets": {\n' + ',\n'.join(lines) + '\n },\n "texts": {\n'
            + ',\n'.join('  {}: {}'.format(json.dumps(k), json.dumps(t)) for k, t in sorted(texts.items())) + '\n }\n}\n')


def load_golden(path):
    """pack_golden's file as the generator recorded it: {'pillow', 'scene', 'sets': name -> describe_output's record with
    'sampled' and 'expected'}"""
    with open(path) as f:
        packed = json.load(f)
    golden = dict(packed['head'], sets={})
    for name, record in packed['sets'].items():
        html = {page: packed['texts'][key] for page, key in record['html'].items()}
        golden['sets'][name] = dict(record, html=html, tree=sorted(set(record['tree']) | set(html) | set(record['sha256'])))
    return golden


def _copy(v):
    return dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v


def run(module, name, image_folder, files, output_folder, **kwargs):
    """One option set on `module` (the reference's compare_batch_results module, or megadetector_amd.compare_batch_results,
    which also takes backend= and device= in kwargs), rendering on one worker.  -> its BatchComparisonResults"""
    spec = OPTION_SETS[name]
    options = module.BatchComparisonOptions()
    options.output_folder, options.image_folder = output_folder, image_folder
    options.n_rendering_workers = 1
    for k, v in spec.get('options', {}).items():
        setattr(options, k, _copy(v))
    which = spec.get('files', ('a', 'b'))
    if len(which) == 3:
        return module.n_way_comparison([files[w] for w in which], options, **kwargs)
    pairwise = module.PairwiseBatchComparisonOptions()
    pairwise.results_filename_a, pairwise.results_filename_b = files[which[0]], files[which[1]]
    for k, v in spec.get('pairwise', {}).items():
        setattr(pairwise, k, _copy(v))
    options.pairwise_options = [pairwise]
    return module.compare_batch_results(options, **kwargs)
