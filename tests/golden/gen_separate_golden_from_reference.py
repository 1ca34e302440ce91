"""
Generates tests/golden/separate_reference.json by running the reference's own separate_detections_into_folders
(postprocessing/separate_detections_into_folders.py, read-only) on the scene of tests/separate_scene.py, once per option set.
The reference cannot travel to the GPU machine, so what it writes is recorded as a fixture together with this script;
tests/test_separate_cpu.py asserts that megadetector_amd.separate_detections reproduces it.

Recorded per option set: the relative path of every file (and empty folder) of the output tree; for a byte copy the scene image
it is a copy of; for a manipulated file its SHA-256, size, sampling, quantisation tables, dimensions and segment list, under
the recorded Pillow version and for the recorded scene (a hash over the generated source files).  Per error case: the type and
the message of what the reference raises.

Third-party modules the reference imports and this container lacks are stubbed as for the other generators (cv2, jsonpickle,
humanfriendly, torchvision); none of them computes anything here.

Run:  python tests/golden/gen_separate_golden_from_reference.py /path/to/reference
"""

import hashlib
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

import separate_scene as S  # noqa: E402


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
    from megadetector.postprocessing import separate_detections_into_folders as ref
    return ref


def scene_hash(sources):
    return hashlib.sha256(json.dumps(sorted(sources.items())).encode()).hexdigest()


def main():
    import PIL
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    golden = {'pillow': PIL.__version__, 'sets': {}, 'errors': {}}
    for name, attributes in S.OPTION_SETS.items():
        with tempfile.TemporaryDirectory() as tmp:
            image_folder, results_file = S.build(tmp)
            sources = S.source_hashes(image_folder)
            golden['scene'] = scene_hash(sources)
            out = os.path.join(tmp, 'out')
            if name == 'no_overwrite':
                S.prepare_existing(out)
            options = S.apply_options(ref.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out, attributes)
            with redirect_stdout(io.StringIO()):
                ref.separate_detections_into_folders(options)
            golden['sets'][name] = {'tree': S.describe_tree(out, sources),
                                    'sources_left': sorted(S.source_hashes(image_folder).values())}
    for name, attributes in S.ERROR_CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            image_folder, results_file = S.build(tmp)
            out = os.path.join(tmp, 'out')
            results_file = S.prepare_error_case(attributes, results_file, out)
            options = S.apply_options(ref.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out, attributes)
            try:
                with redirect_stdout(io.StringIO()):
                    ref.separate_detections_into_folders(options)
                raise SystemExit('{}: the reference raised nothing'.format(name))
            except (AssertionError, ValueError, KeyError) as e:
                golden['errors'][name] = {'type': type(e).__name__, 'message': str(e).replace(tmp, '<tmp>')}
    path = os.path.join(REPO, 'tests', 'golden', 'separate_reference.json')
    with open(path, 'w') as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
