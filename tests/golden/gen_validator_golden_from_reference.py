"""
Generates tests/golden/validator_reference.json: files the megadetector_amd host path writes, each with the verdict of
the *real* reference format validator (megadetector/postprocessing/validate_batch_results.py:71, read-only) on it.
The reference cannot travel with the repository, so the verdicts are committed as a fixture together with this script;
tests/test_host_path_reference.py asserts that megadetector_amd still writes exactly those files and that the
reference accepted every one of them.

Cases:
  * 'stub_images': the loop with the stub detector over the seeded PNGs of tests/stub_detector.py plus an unreadable
    file, plain and batched with image size / timestamp fields, written with absolute and with relative paths
  * 'bundled_images': BASELINE.json configs[0] on tests/golden/bundled_images (a few of the reference's own bundled
    images: JPEG, RGBA PNG, a `failure-examples` sub-folder), batch 8, image sizes, relative paths, image existence
    checked against the folder

Absolute image folders are written as '<images>' in the fixture (the test runs in its own temporary folder).
Third-party modules the reference imports but validation does not use are stubbed as empty modules (cv2, jsonpickle,
humanfriendly).

Run (where the reference tree is available):  python tests/golden/gen_validator_golden_from_reference.py <reference root>
"""

import io
import json
import os
import re
import shutil
import sys
import tempfile
import types
from contextlib import redirect_stdout

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

from megadetector_amd import run_detector_batch as RDB  # noqa: E402
from stub_detector import StubDetector, write_test_images  # noqa: E402

TIME_RE = re.compile(r'("detection_completion_time": )"[^"]*"')
BUNDLED = os.path.join(REPO, 'tests', 'golden', 'bundled_images')
PLACEHOLDER = '<images>'

STUB_RUNS = [('plain', {}), ('batched_sizes', dict(batch_size=4, include_image_size=True, include_image_timestamp=True))]


class _AnyAttr(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return 0


def import_validator(ref_root):
    sys.path.insert(0, ref_root)
    sys.modules.setdefault('cv2', _AnyAttr('cv2'))
    for n in ('jsonpickle', 'humanfriendly'):
        sys.modules.setdefault(n, types.ModuleType(n))
    from megadetector.postprocessing.validate_batch_results import validate_batch_results, ValidateBatchResultsOptions
    return validate_batch_results, ValidateBatchResultsOptions


def _quiet(fn, *a, **k):
    with redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _text(path, img_dir):
    with open(path, 'r', encoding='utf-8') as f:
        return TIME_RE.sub(r'\1"<time>"', f.read()).replace(img_dir, PLACEHOLDER)


def validate(validator, out, rel):
    validate_batch_results, Options = validator
    opts = Options()
    opts.raise_errors = True
    opts.return_data = True
    if rel is not None:
        opts.check_image_existence = True
        opts.relative_path_base = rel
    try:
        d = _quiet(validate_batch_results, out, opts)
    except Exception as e:
        return ['{}: {}'.format(type(e).__name__, e)]
    return [str(e) for e in d['validation_results']['errors']]


def stub_cases(validator, tmp):
    img_dir = os.path.join(tmp, 'imgs')
    os.mkdir(img_dir)
    names = write_test_images(img_dir)
    with open(os.path.join(img_dir, 'broken.jpg'), 'wb') as f:
        f.write(b'nope')
    names.append(os.path.join(img_dir, 'broken.jpg'))
    cases = []
    for run, kw in STUB_RUNS:
        res = _quiet(RDB.load_and_run_detector_batch, 'stub.pt', names, detector=StubDetector(), quiet=True, **kw)
        for rel in (None, img_dir):
            out = os.path.join(tmp, '{}_{}.json'.format(run, rel is not None))
            _quiet(RDB.write_results_to_file, res, out, relative_path_base=rel, detector_file='md_v5a.0.0.pt')
            cases.append({'run': run, 'relative': rel is not None, 'output_text': _text(out, img_dir),
                          'errors': validate(validator, out, rel)})
    return cases


def bundled_case(validator, tmp):
    img_dir = os.path.join(tmp, 'bundled')
    shutil.copytree(BUNDLED, img_dir)
    files = RDB.find_images(img_dir, recursive=True)
    res = _quiet(RDB.load_and_run_detector_batch, 'stub.pt', list(files), detector=StubDetector(), quiet=True, batch_size=8,
                 include_image_size=True)
    out = os.path.join(tmp, 'bundled.json')
    _quiet(RDB.write_results_to_file, res, out, relative_path_base=img_dir, detector_file='md_v5a.0.0.pt')
    return {'files': sorted(os.path.relpath(f, img_dir) for f in files), 'output_text': _text(out, img_dir),
            'errors': validate(validator, out, img_dir)}


def main():
    if len(sys.argv) != 2:
        raise SystemExit('usage: gen_validator_golden_from_reference.py <reference root>')
    validator = import_validator(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        fixture = {'stub_images': stub_cases(validator, tmp), 'bundled_images': bundled_case(validator, tmp)}
    out = os.path.join(REPO, 'tests', 'golden', 'validator_reference.json')
    with open(out, 'w') as f:
        json.dump(fixture, f, indent=0)
    n_err = sum(len(c['errors']) for c in fixture['stub_images']) + len(fixture['bundled_images']['errors'])
    print('wrote', out, os.path.getsize(out), 'bytes;', len(fixture['stub_images']) + 1, 'files,', n_err, 'validation errors')


if __name__ == '__main__':
    main()
