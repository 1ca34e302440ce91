"""
Generates tests/golden/resize_reference.json by running the reference's own functions (visualization/visualization_utils.py,
read-only) on the scene of tests/resize_scene.py.  The reference cannot travel to the GPU machine, so what it returns is
recorded as a fixture together with this script; the fixture holds recorded results only.

Recorded: per option set of resize_scene.OPTION_SETS what resize_image_folder returns (the folders replaced by {IN} and {OUT})
and the output tree it leaves -- every file's SHA-256 and size and, for a JPEG, its dimensions, sampling and tables (each table
stored once: resize_scene.pack_tables / load_golden; one row of the fixture a line: resize_scene.dump_rows); per case of
resize_scene.COCO_CASES what the reference's data_management/resize_coco_dataset.py wrote (the JSON text, the tree) or raised; per crop
of resize_scene.CROPS and per scene file what gray_scale_fraction returns, as float.hex(), or None where it raises (the type of the exception is recorded beside it); the Pillow version and a hash over the generated scene, for which
alone the numbers hold.

Third-party modules the reference imports and this container lacks are stubbed as for the other generators (cv2, jsonpickle,
humanfriendly, torchvision); none of them computes anything here.

Run:  python tests/golden/gen_resize_reference.py /path/to/reference
"""

import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stderr, redirect_stdout

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import resize_scene as S  # noqa: E402


class _AnyAttr(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return 0


def import_reference(root):
    sys.path.insert(0, root)
    sys.modules.setdefault('cv2', _AnyAttr('cv2'))
    sys.modules.setdefault('jsonpickle', types.ModuleType('jsonpickle'))
    hf = types.ModuleType('humanfriendly')
    hf.format_timespan = lambda s: '{:.2f} seconds'.format(s)
    sys.modules.setdefault('humanfriendly', hf)
    tv = types.ModuleType('torchvision')
    tv.ops = types.ModuleType('torchvision.ops')
    sys.modules.setdefault('torchvision', tv)
    sys.modules.setdefault('torchvision.ops', tv.ops)
    from megadetector.visualization import visualization_utils as ref
    return ref


def crop_key(crop):
    return '{},{}'.format(*crop)


def main():
    import PIL
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    golden = {'pillow': PIL.__version__, 'gray': {}, 'gray_errors': {}, 'resize': {}}
    for name in S.OPTION_SETS:
        with tempfile.TemporaryDirectory() as tmp, redirect_stdout(io.StringIO()), redirect_stderr(io.StringIO()):
            results, out = S.run_set(ref.resize_image_folder, os.path.realpath(tmp), name)
            golden['resize'][name] = {'results': results, 'tree': S.describe_tree(out)}
    golden['coco'] = {}
    from megadetector.data_management import resize_coco_dataset as ref_coco

    def ref_main(argv):
        sys.argv = ['resize_coco_dataset.py'] + argv
        ref_coco.main()

    for name in S.COCO_CASES:
        with tempfile.TemporaryDirectory() as tmp, redirect_stdout(io.StringIO()), redirect_stderr(io.StringIO()):
            golden['coco'][name] = S.run_coco_case(os.path.realpath(tmp), name, ref_coco.resize_coco_dataset, ref_main)
    with tempfile.TemporaryDirectory() as tmp:
        files = S.build(tmp)
        golden['scene'] = S.scene_hash(tmp)
        for crop in S.CROPS:
            fractions, errors = {}, {}
            for (name, *_), path in zip(S.IMAGES, files):
                try:
                    fractions[name] = float(ref.gray_scale_fraction(path, crop_size=crop)).hex()
                except Exception as e:
                    fractions[name] = None
                    errors[name] = type(e).__name__
            golden['gray'][crop_key(crop)] = fractions
            golden['gray_errors'][crop_key(crop)] = errors
        try:
            ref.gray_scale_fraction(files[0], crop_size=(0.5, 0.5))
            raise SystemExit('the reference accepted a crop of the whole image')
        except AssertionError as e:
            golden['illegal_crop'] = str(e)
    path = os.path.join(REPO, 'tests', 'golden', 'resize_reference.json')
    with open(path, 'w') as f:
        f.write(S.dump_rows(S.pack_tables(golden)) + '\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
