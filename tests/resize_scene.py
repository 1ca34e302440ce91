"""
The scene of the dataset tools' tests (tests/test_resize_cpu.py, tests/test_gpu_resize.py, tests/test_gray_cpu.py,
tests/test_gpu_gray.py) and of the run of the reference's own functions that tests/golden/gen_resize_reference.py records in
tests/golden/resize_reference.json: a folder of small generated images, the option sets resize_image_folder is run with, and
the crops the gray shares are taken with.  Everything comes from a seed, so any machine rebuilds the scene without the
reference.

The images: 163 x 121 at 4:2:0 whose top half is gray (a "dusk" picture: some gray share strictly between 0 and 1, and another
one without the crop), 160 x 120 at 4:2:2 with restart markers, 97 x 61 at 4:4:4, a 64 x 48 'L' JPEG, an RGB JPEG of gray
pixels, EXIF orientations 6, 3 and 8 with other tags present and a gray band along one stored edge (so that a window taken in
the wrong orientation counts differently), a COM segment, an ICC profile, a progressive JPEG, a PNG, a palette PNG (one band),
a truncated JPEG, and 300 x 2 pixels.
"""

import hashlib
import json
import os

import numpy as np
from PIL import Image

SEED = 20240923


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


def _gray_rows(rgb, y0, y1):
    rgb[y0:y1] = rgb[y0:y1, :, 1:2]


#: file -> (width, height, stored rows [y0, y1) made gray, how it is saved)
IMAGES = [
    ('dusk420.jpg', 163, 121, (0, 60), dict(quality=90, subsampling=2)),
    ('rst422.jpg', 160, 120, (100, 120), dict(quality=85, subsampling=1, restart_marker_rows=2)),
    ('a444.jpg', 97, 61, None, dict(quality=92, subsampling=0)),
    ('grey_l.jpg', 64, 48, None, dict(quality=82, mode='L')),
    ('grey_rgb.jpg', 80, 56, (0, 56), dict(quality=88, subsampling=2)),
    ('rot6.jpg', 96, 64, (0, 24), dict(quality=88, subsampling=2, exif={274: 6, 271: 'a camera trap', 306: '2021:03:04 05:06:07'})),
    ('rot3.jpg', 90, 62, (0, 24), dict(quality=80, subsampling=1, exif={274: 3, 271: 'turned', 272: 'model 7'})),
    ('sub/rot8.jpg', 72, 50, (30, 50), dict(quality=84, subsampling=0, exif={274: 8, 271: 'turned'})),
    ('sub/com.jpg', 96, 64, None, dict(quality=85, subsampling=1, comment=b'station 12')),
    ('sub/icc.jpg', 64, 48, None, dict(quality=75, icc=True)),
    ('sub/prog.jpg', 96, 64, (0, 32), dict(quality=80, progressive=True)),
    ('pic.png', 72, 56, (0, 20), dict()),
    ('palette.png', 40, 30, None, dict(mode='P')),
    ('truncated.jpg', 96, 64, None, dict(quality=85, truncate=0.6)),
    ('thin.jpg', 300, 2, None, dict(quality=85)),
]

#: the crops the gray fractions are recorded for: (top, bottom)
CROPS = [(0.1, 0.1), (0, 0), (0.25, 0.05), (0.0, 0.4), (0.495, 0.495)]


def build(folder):
    """writes the images below `folder`; -> the files in the order of IMAGES, as absolute paths"""
    from PIL import ImageCms
    rng = np.random.default_rng(SEED)
    files = []
    for name, w, h, gray, how in IMAGES:
        how = dict(how)
        path = os.path.join(folder, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        rgb = _content(rng, w, h)
        if gray is not None:
            _gray_rows(rgb, *gray)
        image = Image.fromarray(rgb)
        mode = how.pop('mode', None)
        if mode == 'L':
            image = image.convert('L')
        elif mode == 'P':
            image = image.quantize(16)
        if 'exif' in how:
            exif = Image.Exif()
            for tag, value in how['exif'].items():
                exif[tag] = value
            how['exif'] = exif
        if how.pop('icc', False):
            profile = bytearray(ImageCms.ImageCmsProfile(ImageCms.createProfile('sRGB')).tobytes())
            profile[24:36] = bytes([7, 228, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0])         # the header's creation time: 2020-01-01 00:00:00
            how['icc_profile'] = bytes(profile)
        truncate = how.pop('truncate', None)
        image.save(path, **how)
        if truncate is not None:
            with open(path, 'rb') as f:
                data = f.read()
            with open(path, 'wb') as f:
                f.write(data[:int(len(data) * truncate)])
        files.append(path)
    return files


def scene_hash(folder):
    """one SHA-256 over the names and bytes of the scene's files: the fixture holds for this scene only"""
    h = hashlib.sha256()
    for name, *_ in IMAGES:
        with open(os.path.join(folder, name), 'rb') as f:
            h.update(json.dumps([name, hashlib.sha256(f.read()).hexdigest()]).encode())
    return h.hexdigest()


# ---- the resize runs -------------------------------------------------------------------------------------------------------------

#: name -> keyword arguments of resize_image_folder; keys with an underscore change the scene around the call
OPTION_SETS = {
    'width_64': dict(target_width=64),
    'width_200_enlarging': dict(target_width=200),
    'both_80': dict(target_width=80, target_height=80),
    'height_30': dict(target_height=30),
    'no_enlarge_200': dict(target_width=200, no_enlarge_width=True),
    'equal_to_some': dict(target_width=96, target_height=64),
    'no_target': dict(),
    'none_is_minus_one': dict(target_width=None, target_height=None, quality=95),
    'width_64_quality_50': dict(target_width=64, quality=50),
    'width_64_quality_95': dict(target_width=64, quality=95),
    'no_target_quality_50': dict(quality=50),
    'no_overwrite': dict(target_width=64, overwrite=False, _existing=True),
    'in_place': dict(target_width=64, _in_place=True),
    'files_relative': dict(target_width=64, image_files_relative=['sub/com.jpg', 'dusk420.jpg', 'sub/rot8.jpg', 'missing.jpg'], recursive=False),
    'not_recursive': dict(target_height=30, recursive=False),
}
#: what the 'no_overwrite' set finds in the target tree before it runs: files that must survive as they are
EXISTING = {'a444.jpg': b'an older copy', 'sub/com.jpg': b'another one', 'notes.txt': b'kept'}


def run_set(resize_image_folder, tmp, name, **extra):
    """builds the scene below tmp/in and runs one option set with the given resize_image_folder (the reference's or ours);
    -> (results with the folders replaced by {IN} and {OUT}, the output folder)"""
    kw = dict(OPTION_SETS[name])
    source = os.path.join(tmp, 'in')
    build(source)
    out = source if kw.pop('_in_place', False) else os.path.join(tmp, 'out')
    if kw.pop('_existing', False):
        for rel, data in EXISTING.items():
            path = os.path.join(out, rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'wb') as f:
                f.write(data)
    results = resize_image_folder(source, None if out == source else out, n_workers=1, **kw, **extra)
    return normalise(results, source, out), out


def normalise(results, source, out):
    def fix(s):
        if s is None:
            return None
        return s.replace(out + os.sep, '{OUT}/').replace(source + os.sep, '{IN}/').replace(os.sep, '/') if out != source else \
            s.replace(source + os.sep, '{IN}/').replace(os.sep, '/')
    return [{'input_fn': fix(r['input_fn']), 'output_fn': fix(r['output_fn']), 'status': r['status'], 'error': fix(r['error'])} for r in results]


def describe_tree(folder):
    """relative path -> SHA-256 and size in bytes and, for a JPEG, dimensions, sampling and tables as Pillow reads them"""
    tree = {}
    for root, _, names in os.walk(folder):
        for n in names:
            path = os.path.join(root, n)
            with open(path, 'rb') as f:
                data = f.read()
            entry = {'sha256': hashlib.sha256(data).hexdigest(), 'bytes': len(data)}
            if data[:2] == b'\xff\xd8':
                im = Image.open(path)
                entry['size'] = list(im.size)
                entry['quant'] = {str(k): [int(v) for v in t] for k, t in im.quantization.items()}
                entry['sampling'] = [list(layer[1:3]) for layer in im.layer]
            tree[os.path.relpath(path, folder).replace(os.sep, '/')] = entry
    return tree


def is_exact(golden, folder):
    """whether the bytes the fixture records can be expected: the recorded Pillow version, and `folder` holds the recorded scene.
    Without it the tests still assert everything that does not depend on the encoder's version"""
    import PIL
    return PIL.__version__ == golden['pillow'] and scene_hash(folder) == golden['scene']


def compare_tree(tree, want, exact):
    """describe_tree against the fixture's: names, dimensions, sampling and tables always; SHA-256 and size in bytes when exact"""
    assert sorted(tree) == sorted(want)
    for name, entry in want.items():
        got = tree[name]
        if exact:
            assert got['sha256'] == entry['sha256'] and got['bytes'] == entry['bytes'], '{}: the bytes differ'.format(name)
        for key in ('size', 'quant', 'sampling'):
            assert got.get(key) == entry.get(key), '{}: {}'.format(name, key)


# ---- the fixture's text -------------------------------------------------------------------------------------------------------------

def pack_tables(golden):
    """every quantisation table of the recorded trees stored once, in golden['tables'], and named by its index"""
    tables = []
    for run in list(golden['resize'].values()) + [r for r in golden.get('coco', {}).values() if 'tree' in r]:
        for entry in run['tree'].values():
            for k, table in entry.get('quant', {}).items():
                if table not in tables:
                    tables.append(table)
                entry['quant'][k] = tables.index(table)
    golden['tables'] = tables
    return golden


def load_golden(path):
    """tests/golden/resize_reference.json with the tables put back where pack_tables took them from"""
    with open(path) as f:
        golden = json.load(f)
    for run in list(golden['resize'].values()) + [r for r in golden.get('coco', {}).values() if 'tree' in r]:
        for entry in run['tree'].values():
            for k, index in entry.get('quant', {}).items():
                entry['quant'][k] = golden['tables'][index]
    return golden


def dump_rows(value, depth=0, rows_at=4):
    """JSON text with one row a line: dicts and lists are opened up to depth rows_at, what lies below is written compactly
    ('tables', 'gray' and 'gray_errors' hold their rows two levels down)"""
    if not isinstance(value, (dict, list)) or depth >= rows_at or not value:
        return json.dumps(value, sort_keys=True)
    pad = ' ' * (depth + 1)
    if isinstance(value, list):
        return '[\n' + ',\n'.join(pad + dump_rows(v, depth + 1, rows_at) for v in value) + ']'
    return '{\n' + ',\n'.join('{}{}: {}'.format(pad, json.dumps(k), dump_rows(v, depth + 1, 2 if depth == 0 and k not in ('resize', 'coco') else rows_at))
                              for k, v in sorted(value.items())) + '}'


# ---- the COCO runs -------------------------------------------------------------------------------------------------------------------

def coco_dataset(only=None):
    """a COCO dict over the scene (or the files of `only`) and a file that is missing: two boxes on most images, an image
    without annotations, an annotation without 'bbox'"""
    names = [name for name, *_ in IMAGES] + ['missing.jpg']
    images, annotations = [], []
    for k, name in enumerate(n for n in names if only is None or n in only):
        w, h = next(((w, h) for n, w, h, *_ in IMAGES if n == name), (10, 10))
        images.append({'id': 'im{}'.format(k), 'file_name': name, 'width': w, 'height': h, 'location': 'cam{}'.format(k % 3)})
        if name == 'a444.jpg':
            continue                                                    # an image without annotations
        annotations.append({'id': len(annotations), 'image_id': 'im{}'.format(k), 'category_id': 1, 'bbox': [w / 8, h / 4, w / 3, h / 2.5]})
        annotations.append({'id': len(annotations), 'image_id': 'im{}'.format(k), 'category_id': 2, 'bbox': [1, 2, 7.5, 3]} if k % 2 else
                           {'id': len(annotations), 'image_id': 'im{}'.format(k), 'category_id': 0})           # no 'bbox'
    return {'info': {'version': '1'}, 'images': images, 'annotations': annotations,
            'categories': [{'id': 0, 'name': 'empty'}, {'id': 1, 'name': 'deer'}, {'id': 2, 'name': 'fox'}]}


#: name -> keyword arguments of resize_coco_dataset; '_only': the files of the dataset, '_cli': the arguments of the command line
COCO_CASES = {
    'omit_width_64': dict(target_size=(64, -1), unavailable_image_handling='omit', no_enlarge_width=False),
    'omit_copy_equal': dict(target_size=(96, 64), unavailable_image_handling='omit'),
    'omit_rewrite_equal': dict(target_size=(96, 64), correct_size_image_handling='rewrite', unavailable_image_handling='omit'),
    'omit_copy_no_target': dict(unavailable_image_handling='omit'),
    'omit_rewrite_no_target': dict(correct_size_image_handling='rewrite', unavailable_image_handling='omit'),
    'omit_no_enlarge_100': dict(target_size=(100, -1), correct_size_image_handling='rewrite', unavailable_image_handling='omit'),
    'error_missing': dict(target_size=(64, -1), _only=['dusk420.jpg', 'missing.jpg']),
    'error_open': dict(target_size=(64, -1), _only=['dusk420.jpg', 'palette.png']),
    'error_resize': dict(target_size=(64, -1), no_enlarge_width=False, _only=['dusk420.jpg', 'thin.jpg', 'missing.jpg']),
    'error_truncated': dict(target_size=(64, -1), _only=['truncated.jpg', 'sub/rot8.jpg']),
    'bad_handling': dict(correct_size_image_handling='link', _only=['dusk420.jpg']),
    'cli': dict(_cli=['--target_size', '80,-1', '--correct_size_image_handling', 'rewrite'], _only=['dusk420.jpg', 'sub/rot8.jpg', 'grey_l.jpg', 'pic.png']),
}


def run_coco_case(tmp, name, resize_coco_dataset=None, main=None, **extra):
    """builds the scene and the COCO file below tmp and runs one case with the given function (or, for a '_cli' case, the given
    main(argv)) -> {'error': [type, text]} for a run that raises, else {'json': the text of the written file, 'returned_equal':
    whether the returned dict is what the file holds, 'tree': describe_tree of the output folder}"""
    kw = dict(COCO_CASES[name])
    source, out = os.path.join(tmp, 'in'), os.path.join(tmp, 'out')
    build(source)
    coco_in, coco_out = os.path.join(tmp, 'coco.json'), os.path.join(tmp, 'written', 'coco_resized.json')
    with open(coco_in, 'w') as f:
        json.dump(coco_dataset(kw.pop('_only', None)), f)
    cli = kw.pop('_cli', None)
    try:
        if cli is not None:
            main([source, coco_in, out, coco_out] + cli + [v for k, x in extra.items() for v in ('--' + k, str(x))])
            returned = None
        else:
            returned = resize_coco_dataset(source, coco_in, out, coco_out, **kw, **extra)
    except Exception as e:
        return {'error': [type(e).__name__, str(e).replace(source + os.sep, '{IN}/')]}
    with open(coco_out, newline='') as f:
        text = f.read()
    return {'json': text, 'returned_equal': returned is None or returned == json.loads(text), 'tree': describe_tree(out)}
