"""
Generates tests/golden/postprocess_reference.json by running the reference's own process_batch_results
(postprocessing/postprocess_batch_results.py, read-only) on the scene of tests/postprocess_scene.py, once per option set.
The reference cannot travel to the GPU machine, so what it writes is recorded as a fixture together with this script;
tests/test_postprocess_cpu.py asserts that megadetector_amd.postprocess_batch_results reproduces it.

Recorded per option set: the sampled files in the order the reference renders them (its _render_image_no_gt is wrapped, and
the rendering runs serially so that the order of the calls is the order of the sample), the output tree, the text of index.html
and of every sub-page with the scene's own folder replaced by '<tmp>', and the SHA-256 of every rendered file, under the
recorded Pillow version and for the recorded scene (a hash over the generated source files).

Before anything is recorded the script asserts, on the CPU and with this project's own planning, what the GPU test relies on:
in every option set the only images the device leg hands to the host leg are the PNG and the entry whose file is missing.

Third-party modules the reference imports that may not be installed are stubbed as for the other generators (cv2, jsonpickle,
humanfriendly); none of them computes anything here.  pandas, scikit-learn and matplotlib, which the reference imports too,
are needed for the run; the package itself uses none of them.

Run:  python tests/golden/gen_postprocess_reference.py /path/to/reference
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

import postprocess_scene as S  # noqa: E402


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
    from megadetector.postprocessing import postprocess_batch_results as ref
    return ref


def host_leg_files(tmp, attributes):
    """the files this project's device leg would hand to the host leg before decoding anything"""
    from megadetector_amd import postprocess_batch_results as PB
    image_folder, results_file = S.build(tmp)
    options = S.apply_options(PB.PostProcessingOptions(), image_folder, results_file, os.path.join(tmp, 'out'), attributes)
    with redirect_stdout(io.StringIO()):
        d = PB.decide_sample(options)
    handed = []
    for decision in d['decisions']:
        if decision['category_string'] in options.rendering_bypass_sets:
            continue
        try:
            PB._plan_job(decision, d['detection_categories'], d['classification_categories'], options)
        except Exception:
            handed.append(decision['file'])
    return handed


def main():
    import PIL
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    for name, attributes in S.OPTION_SETS.items():
        with tempfile.TemporaryDirectory() as tmp:
            handed = host_leg_files(tmp, attributes)
            assert set(handed) <= {'pic.png', S.MISSING, S.MISSING.replace('gone', 'lost')}, (name, handed)
    ref = import_reference(sys.argv[1])
    golden = {'pillow': PIL.__version__, 'sets': {}}
    render = ref._render_image_no_gt
    sampled = []

    def recorded(file_info, *args, **kwargs):
        sampled.append(file_info['file'])
        return render(file_info, *args, **kwargs)

    ref._render_image_no_gt = recorded
    for name, attributes in S.OPTION_SETS.items():
        with tempfile.TemporaryDirectory() as tmp:
            image_folder, results_file = S.build(tmp)
            golden['scene'] = S.scene_hash(image_folder)
            out = os.path.join(tmp, 'out')
            options = S.apply_options(ref.PostProcessingOptions(), image_folder, results_file, out, attributes)
            options.parallelize_rendering = False
            del sampled[:]
            with redirect_stdout(io.StringIO()):
                ppresults = ref.process_batch_results(options)
            assert ppresults.output_html_file == os.path.join(out, 'index.html')
            record = S.describe_output(out, tmp)
            record['sampled'] = list(sampled)
            golden['sets'][name] = record
    path = os.path.join(REPO, 'tests', 'golden', 'postprocess_reference.json')
    with open(path, 'w') as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
