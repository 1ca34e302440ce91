"""
Generates tests/golden/visualize_db_reference.json by running the reference's own visualize_db
(visualization/visualize_db.py, read-only) on the scene of tests/visualize_db_scene.py, once per option set and once per
error case.  The reference cannot travel to the GPU machine, so what it writes is recorded as a fixture together with this
script; tests/test_visualize_db_cpu.py asserts that megadetector_amd.visualize_db reproduces it.

Recorded per option set: the output names in the order the reference renders them (the rendering runs serially, and the
stand-in for tqdm notes the list the rendering loop is given), the output tree, the text of every HTML file with the scene's
own folder replaced by '<tmp>', and the SHA-256 of every rendered file, under the recorded Pillow version and for the
recorded scene (a hash over the generated source files).  Every set seeds what it draws at random, so every order is pinned.
The reference joins a Python set of class names into a title, so a title with several classes depends on string hashing: the
names of such titles are sorted before they are recorded (visualize_db_scene.normalise_titles), and the test does the same to
what this package writes.  Per error case: the type and the message of what the reference raises.

Before anything is recorded the script asserts, on the CPU and with this project's own planning, what the GPU test relies on:
in every option set the only existing, opening image the device leg hands to the host leg is the PNG.

Third-party modules the reference imports that may not be installed are stubbed as for the other generators (cv2, jsonpickle,
humanfriendly); none of them computes anything here.

Run:  python tests/golden/gen_visualize_db_reference.py /path/to/reference
"""

import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import visualize_db_scene as S  # noqa: E402


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
    from megadetector.visualization import visualize_db as ref
    return ref


def host_leg_files(tmp, attributes):
    """the existing files this project's device leg would hand to the host leg before decoding anything"""
    from megadetector_amd import visualize_db as VD
    image_folder, db_file = S.build(tmp, attributes.get('variant'))
    options = S.apply_options(VD.DbVizOptions(), os.path.join(tmp, 'out'), {k: v for k, v in attributes.items() if k != 'prefill'})
    with open(db_file) as f:
        image_db = json.load(f)
    with redirect_stdout(io.StringIO()):
        images, image_id_to_annotations, label_map = VD.select_images(image_db, options)
    handed = []
    for img in images:
        info, _ = VD.describe_image(img, image_id_to_annotations.get(img['id'], []), image_folder, label_map, options)
        try:
            VD.plan_job(info, options, label_map)
        except Exception:
            handed.append(img['file_name'])
    return handed


def main():
    import PIL
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    for name, attributes in S.OPTION_SETS.items():
        with tempfile.TemporaryDirectory() as tmp:
            handed = host_leg_files(tmp, attributes)
            assert set(handed) <= {S.PNG, S.MISSING, S.BROKEN}, (name, handed)
    ref = import_reference(sys.argv[1])
    golden = {'pillow': PIL.__version__, 'sets': {}, 'errors': {}}
    order = []

    def noted(items, **kwargs):
        if isinstance(items, list) and items and isinstance(items[0], dict) and 'output_file_name' in items[0]:
            order[:] = [x['output_file_name'] for x in items]
        return items

    ref.tqdm = noted
    for name, attributes in S.OPTION_SETS.items():
        with tempfile.TemporaryDirectory() as tmp:
            image_folder, db_file = S.build(tmp, attributes.get('variant'))
            golden['scene'] = S.scene_hash(image_folder)
            out = os.path.join(tmp, 'out')
            options = S.apply_options(ref.DbVizOptions(), out, attributes)
            options.parallelize_rendering = False
            del order[:]
            with redirect_stdout(io.StringIO()):
                html_file, _ = ref.visualize_db(db_file, out, image_folder, options)
            assert html_file == os.path.join(out, 'index.html')
            record = S.describe_output(out, tmp)
            record['order'] = list(order)
            golden['sets'][name] = record
    for name, (attributes, variant) in S.ERROR_CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            image_folder, db_file = S.build(tmp, variant)
            out = os.path.join(tmp, 'out')
            options = S.apply_options(ref.DbVizOptions(), out, attributes)
            options.parallelize_rendering = False
            try:
                with redirect_stdout(io.StringIO()):
                    ref.visualize_db(db_file, out, image_folder, options)
            except Exception as e:
                golden['errors'][name] = {'type': type(e).__name__, 'message': str(e)}
            else:
                raise SystemExit('the reference raised nothing for {}'.format(name))
    path = os.path.join(REPO, 'tests', 'golden', 'visualize_db_reference.json')
    with open(path, 'w') as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
