"""
The scene of tests/test_visualize_db_cpu.py and tests/test_gpu_visualize_db.py: a folder of small generated images, a COCO
Camera Traps database over them and the option sets the reference's visualize_db was run with for
tests/golden/visualize_db_reference.json (tests/golden/gen_visualize_db_reference.py).  Everything comes from a seed, so any
machine rebuilds the scene without the reference.

The images (64 x 48 up to 640 x 480): 4:4:4, 4:2:2 and 4:2:0 RGB JPEGs, one with EXIF orientation 6, one 'L' JPEG, an odd
333 x 251, one with a COM segment, one PNG, one file that is missing and one that does not open.  The database: absolute and
bbox_relative boxes (on different images), an image-level label without a box, a NaN box, `score` fields on some annotations
and a `q` field on all, an image without annotations, two categories on one image, seq_id / frame_num / seq_num_frames,
flags, an extra field, an id with '/', a blank and '#', boxes of 1 x 1, 3 x 2 and 7 x 20 pixels, a box partly outside the image.
No image is wider than 640 pixels, so the default viz_size (1000, -1) leaves all of them as they are (no_enlarge_width); the
sets with a viz_size of their own resize.  No two categories have the same number of images: the reference orders category
pages of equal counts by the iteration order of a set of strings.
"""

import hashlib
import itertools
import json
import os

import numpy as np
from PIL import Image

from separate_scene import _content

SEED = 20241104
CATEGORIES = [{'id': 1, 'name': 'Deer'}, {'id': 2, 'name': 'red fox'}, {'id': 3, 'name': 'Empty'}, {'id': 4, 'name': 'Bird "small"'}]
#: the class names of the images with several classes: the reference joins a set of them (normalise_titles)
MULTIPLE = [('Deer', 'red fox')]

#: file -> (width, height as stored, how it is saved; None: not written)
FILES = {
    'cam1/a444.jpg': (640, 480, dict(quality=90, subsampling=0)),
    'cam1/a422.jpg': (333, 251, dict(quality=80, subsampling=1)),
    'cam1/a420.jpg': (200, 150, dict(quality=75)),
    'cam2/rot6.jpg': (160, 121, dict(quality=88, subsampling=2, exif={274: 6, 271: 'turned'})),
    'cam2/grey.jpg': (127, 95, dict(quality=82, mode='L')),
    'cam2/com.jpg': (320, 240, dict(quality=85, subsampling=1, comment=b'camera 7, station ridge')),
    'cam2/pic.png': (144, 111, dict()),
    'cam2/blank.jpg': (64, 48, dict(quality=75)),
    'cam3/gone.jpg': None,
    'cam3/broken.jpg': 'not an image',
    'cam3/deer one#1.jpg': (180, 135, dict(quality=92, subsampling=1)),
    'cam3/edge.jpg': (120, 90, dict(quality=75, subsampling=1)),
    'cam3/solo.jpg': (100, 80, dict(quality=70)),
}
PNG, COM, MISSING, BROKEN = 'cam2/pic.png', 'cam2/com.jpg', 'cam3/gone.jpg', 'cam3/broken.jpg'
#: the images with a box thinner than twice the default outline (8 pixels) at every size the sets render them at
THIN = ('cam1/a444.jpg', 'cam1/a422.jpg')

IMAGES = [
    {'id': 'cam1/a444', 'file_name': 'cam1/a444.jpg', 'seq_id': 's1', 'frame_num': 0, 'seq_num_frames': 3, 'location': 'ridge'},
    {'id': 'cam1/a422.jpg', 'file_name': 'cam1/a422.jpg', 'seq_id': 's1', 'frame_num': 1, 'seq_num_frames': 3},
    {'id': 3, 'file_name': 'cam1/a420.jpg', 'seq_id': 's1', 'frame_num': 2, 'seq_num_frames': 3, 'flags': ''},
    {'id': 'rot6', 'file_name': 'cam2/rot6.jpg', 'flags': ['blurry', 'night'], 'width': 121, 'height': 160},
    {'id': 'grey.JPG', 'file_name': 'cam2\\grey.jpg', 'location': 'creek'},
    {'id': 'com:1', 'file_name': 'cam2/com.jpg', 'location': None},
    {'id': 'pic', 'file_name': 'cam2/pic.png'},
    {'id': 'blank', 'file_name': 'cam2/blank.jpg', 'seq_id': 's3', 'frame_num': 0},
    {'id': 'gone', 'file_name': 'cam3/gone.jpg'},
    {'id': 'broken%', 'file_name': 'cam3/broken.jpg'},
    {'id': 'Cam3/Deer one#1.JPG', 'file_name': 'cam3/deer one#1.jpg', 'seq_id': 's2', 'frame_num': -1},
    {'id': 'edge', 'file_name': 'cam3/edge.jpg', 'seq_id': 's2', 'frame_num': 1},
    {'id': 'solo', 'file_name': 'cam3/solo.jpg'},
]


def _ann(n, image_id, category_id, q, **fields):
    return dict({'id': 'ann{}'.format(n), 'image_id': image_id, 'category_id': category_id, 'q': q}, **fields)


ANNOTATIONS = [
    _ann(0, 'cam1/a444', 1, 0.9, bbox=[100, 120, 200, 150], score=0.934),
    _ann(1, 'cam1/a444', 1, 0.8, bbox=[400, 60, 0, 0]),                          # 1 x 1 pixels
    _ann(2, 'cam1/a444', 1, 0.7, bbox=[420.4, 200.7, 2.2, 1.1], score=0.5),      # 3 x 2
    _ann(3, 'cam1/a444', 1, 0.6, bbox=[500, 300, 6, 19], note='small'),          # 7 x 20
    _ann(4, 'cam1/a444', 1, 0.3, bbox=[300, 400, 40, 5]),                        # 41 x 6
    _ann(5, 'cam1/a422.jpg', 2, 0.9, bbox_relative=[0.1, 0.2, 0.5, 0.6], score=0.81),
    _ann(6, 'cam1/a422.jpg', 2, 0.55, bbox_relative=[0.7, 0.5, 0.004, 0.003]),
    _ann(7, 3, 3, 1.0, sequence_level_annotation=True),
    _ann(8, 'rot6', 1, 0.75, bbox=[10, 20, 80, 100], score=0.755),
    _ann(9, 'grey.JPG', 1, 0.65, bbox=[20, 10, 60, 70]),
    _ann(10, 'grey.JPG', 1, 0.95, bbox=float('nan')),
    _ann(11, 'com:1', 1, 0.85, bbox=[30, 40, 120, 100], score=0.85, note=''),
    _ann(12, 'com:1', 2, 0.45, bbox=[170, 90, 100, 120], score=0.449),
    _ann(13, 'pic', 2, 0.9, bbox=[14, 11, 100, 88]),
    _ann(14, 'gone', 1, 0.9, bbox=[1, 2, 30, 40]),
    _ann(15, 'broken%', 4, 0.9, bbox=[1, 2, 30, 40]),
    _ann(16, 'Cam3/Deer one#1.JPG', 1, 0.9, bbox=[-20, 60, 90, 110], sequence_level_annotation=False),
    _ann(17, 'Cam3/Deer one#1.JPG', 1, 0.2, sequence_level_annotation=True),
    _ann(18, 'edge', 2, 0.4, bbox=[5, 5, 60, 50], score=0.4),
    _ann(19, 'edge', 2, 0.8, bbox=[50, 30, 69, 59], score=0.8),
    _ann(20, 'solo', 3, 0.5, bbox=[0, 0, 100, 80], note='whole image'),
]

_SMALL = {'viz_size': (110, -1)}
_SAMPLE = {'num_to_visualize': 3, 'random_seed': 1}

#: name -> attributes set on the options
OPTION_SETS = {
    'defaults': {},
    'size_none': {'viz_size': None},
    'size_minus_one': {'viz_size': (-1, -1)},
    'size_400_300': {'viz_size': (400, 300)},
    'size_2000': {'viz_size': (2000, -1)},
    'size_110': dict(_SMALL),
    'sample_6_seed_3': dict(_SMALL, num_to_visualize=6, random_seed=3),
    'sample_5_random_sort': {'num_to_visualize': 5, 'random_seed': 7, 'sort_by_filename': False},
    'trim': {'trim_to_images_with_bboxes': True, 'variant': 'no_nan_box'},      # (with the NaN box the reference asserts)
    'include': {'classes_to_include': ['red fox', 'empty']},
    'exclude': {'classes_to_exclude': ['deer']},
    'multiple': {'classes_to_include': ['*multiple*', 'bird "small"']},
    'sequences_unlimited': dict(_SAMPLE, max_sequence_length=0),
    'sequences_of_2': dict(_SAMPLE, max_sequence_length=2, random_seed=2),
    'category_pages': {'create_category_pages': True},
    'category_pages_by_count': dict(_SMALL, create_category_pages=True, category_page_sort_order='image_count'),
    'confidence_threshold': dict(_SMALL, confidence_threshold=0.5, confidence_field_name='q'),
    'links': {'add_search_links': True, 'include_image_links': True, 'include_filename_links': True, 'show_full_paths': True},
    'extra_fields': {'extra_image_fields_to_print': 'location', 'extra_annotation_fields_to_print': ['q', 'note'],
                     'html_options': {'maxFiguresPerHtmlFile': 5}, 'parallelize_rendering': False},
    'quality_colormap': dict(_SMALL, quality=90, colormap=['Red', 'Lime', 'RoyalBlue'], box_thickness=2, box_expansion=3),
    'custom_mapping': dict(_SMALL, custom_category_mapping={1: 'cervid', 2: 'canid'}),
    'no_force_rendering': {'force_rendering': False, 'prefill': ['cam1~a444_gt.jpg', 'gone_gt.jpg']},
}
#: the sets that resize nothing
UNRESIZED_SETS = ('defaults', 'size_none', 'size_minus_one', 'size_2000', 'sample_5_random_sort', 'trim', 'include', 'exclude', 'multiple',
                  'sequences_unlimited', 'sequences_of_2', 'category_pages', 'links', 'extra_fields', 'no_force_rendering')
#: name -> (attributes, variant of the database): the reference raises; the fixture records the type and the message
ERROR_CASES = {
    'include_and_exclude': ({'classes_to_include': ['deer'], 'classes_to_exclude': ['empty']}, None),
    'include_not_a_list': ({'classes_to_include': 'deer'}, None),
    'exclude_not_a_list': ({'classes_to_exclude': 'deer'}, None),
    'threshold_without_field': ({'confidence_threshold': 0.5}, None),
    'trim_box_not_a_list': ({'trim_to_images_with_bboxes': True}, 'tuple_box'),
    'trim_nan_box': ({'trim_to_images_with_bboxes': True}, None),
    'both_box_fields': ({}, 'both_fields'),
    'absolute_and_relative': ({}, 'mixed_fields'),
    'float_box': ({}, 'float_box'),
    'duplicate_ids_in_sequences': ({'max_sequence_length': 0}, 'duplicate_ids'),
}
PREFILL_BYTES = b'already there'


def database(variant=None):
    db = {'info': {'version': 'scene'}, 'images': [dict(im) for im in IMAGES], 'annotations': [dict(a) for a in ANNOTATIONS],
          'categories': [dict(c) for c in CATEGORIES]}
    if variant == 'tuple_box':
        db['annotations'][0]['bbox'] = 'not a list'
    elif variant == 'both_fields':
        db['annotations'][0]['bbox_relative'] = [0.1, 0.1, 0.2, 0.2]
    elif variant == 'mixed_fields':
        del db['annotations'][1]['bbox']
        db['annotations'][1]['bbox_relative'] = [0.1, 0.1, 0.2, 0.2]
    elif variant == 'float_box':
        db['annotations'][0]['bbox'] = 0.5
    elif variant == 'duplicate_ids':
        db['images'].append(dict(db['images'][0]))
    elif variant == 'no_nan_box':
        db['annotations'] = [a for a in db['annotations'] if a.get('bbox') == a.get('bbox')]
    else:
        assert variant is None
    return db


def build(folder, variant=None):
    """writes the images below `folder` and db.json beside them; -> (image folder, database file)"""
    rng = np.random.default_rng(SEED)
    image_folder = os.path.join(folder, 'images')
    for name, spec in FILES.items():
        path = os.path.join(image_folder, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if spec is None:
            continue
        if isinstance(spec, str):
            with open(path, 'w') as f:
                f.write(spec)
            continue
        w, h, how = spec
        how = dict(how)
        image = Image.fromarray(_content(rng, w, h))
        if how.pop('mode', None) == 'L':
            image = image.convert('L')
        if 'exif' in how:
            exif = Image.Exif()
            for tag, value in how['exif'].items():
                exif[tag] = value
            how['exif'] = exif
        image.save(path, **how)
    db_file = os.path.join(folder, 'db.json')
    with open(db_file, 'w') as f:
        json.dump(database(variant), f, indent=1)
    return image_folder, db_file


def apply_options(options, output_folder, attributes):
    """sets the attributes of a set on a DbVizOptions (ours or the reference's); 'prefill': files put into rendered_images
    before the run; 'variant' is build's"""
    for k, v in attributes.items():
        if k == 'variant':
            continue
        if k == 'prefill':
            os.makedirs(os.path.join(output_folder, 'rendered_images'), exist_ok=True)
            for name in v:
                with open(os.path.join(output_folder, 'rendered_images', name), 'wb') as f:
                    f.write(PREFILL_BYTES)
        elif k == 'html_options':
            options.html_options.update(v)
        else:
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


def normalise_titles(text):
    """The class names of a title with several classes, sorted: the reference joins a set of strings, whose order depends on
    string hashing; this package writes them in first-seen order.  Every way the names are written -- as they are, in lower
    case (a class filter lowers them), as search links -- in every order becomes the sorted one."""
    link = '<a href="https://www.google.com/search?tbm=isch&q={}">{}</a>'
    for names in MULTIPLE:
        for lower in (False, True):
            for linked in (False, True):
                written = [n.lower() if lower else n for n in names]
                written = [link.format(n.replace('"', ''), n.replace('"', '')) if linked else n for n in written]
                for order in itertools.permutations(written):
                    text = text.replace(', '.join(order), ', '.join(sorted(written)))
    return text


def describe_output(output_folder, folder):
    """What a run wrote: {'tree': every relative path, 'html': name -> text of every HTML file with `folder`, the scene's own
    path, replaced by '<tmp>' and its titles normalised, 'sha256': relative path -> hash of every other file}"""
    import urllib.parse
    out = {'tree': [], 'html': {}, 'sha256': {}}
    for root, _, names in os.walk(output_folder):
        for n in names:
            path = os.path.join(root, n)
            rel = os.path.relpath(path, output_folder).replace(os.sep, '/')
            out['tree'].append(rel)
            with open(path, 'rb') as f:
                data = f.read()
            if n.endswith('.html'):
                text = data.decode('utf-8')
                text = text.replace(urllib.parse.quote(folder, safe=':/'), '<tmp>').replace(folder, '<tmp>')
                out['html'][rel] = normalise_titles(text)
            else:
                out['sha256'][rel] = hashlib.sha256(data).hexdigest()
    out['tree'].sort()
    return out
