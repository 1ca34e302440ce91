"""
Generates tests/golden/compare_reference.json by running the reference's own compare_batch_results / n_way_comparison
(postprocessing/compare_batch_results.py, read-only) on the scene of tests/compare_scene.py, once per option set, rendering on
one worker.  The reference cannot travel to the GPU machine, so what it writes is recorded as a fixture together with this
script; tests/test_compare_cpu.py asserts that megadetector_amd.compare_batch_results reproduces it.

Recorded per option set: the sampled files in the order the reference renders them (its _render_image_pair is wrapped:
[output folder below the run's, file]), the output tree, the text of every HTML file with the scene's own folder replaced by
'<tmp>', and the SHA-256 of every rendered file, under the recorded Pillow version and for the recorded scene (a hash over
the generated source files).  The file keeps every distinct HTML text once (compare_scene.pack_golden / load_golden): most pages
are the same in most option sets.

Before anything is recorded the script asserts, on the CPU and with this project's own planning, what the GPU test relies on:
in every option set the only jobs the device leg hands to the host leg are those of the PNG and those of thin.jpg in which
the results file with the planted thin box takes part.  For the n-way sets it records the counts that follow from that
planning ('expected': jobs, host jobs, distinct files PIL decodes, distinct JPEG files the device decodes).

Third-party modules the reference imports that may not be installed are stubbed as for the other generators (cv2, jsonpickle,
humanfriendly); none of them computes anything here.

Run:  python tests/golden/gen_compare_reference.py /path/to/reference
"""

import io
import json
import os
import sys
import tempfile
from contextlib import redirect_stdout

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tests', 'golden'))

import compare_scene as S  # noqa: E402
from gen_postprocess_reference import _AnyAttr  # noqa: E402,F401


def import_reference(root):
    import types
    sys.path.insert(0, root)
    sys.modules.setdefault('cv2', _AnyAttr('cv2'))
    sys.modules.setdefault('jsonpickle', types.ModuleType('jsonpickle'))
    hf = types.ModuleType('humanfriendly')
    hf.format_timespan = lambda s: '{:.2f} seconds'.format(s)
    sys.modules.setdefault('humanfriendly', hf)
    from megadetector.postprocessing import compare_batch_results as ref
    return ref


def device_planning(name):
    """this project's planning of the option set: -> {'jobs', 'host', 'files_decoded_pil', 'files_decoded_gpu'} after the
    assertion on which jobs go to the host leg"""
    from megadetector_amd import compare_batch_results as C
    captured = {}

    def plan_only(options, **kwargs):
        with redirect_stdout(io.StringIO()):
            copied, plans = C.plan_comparisons(options)
        captured['jobs'] = [job for plan in plans for job in plan['jobs']]
        captured['thin_in'] = [plan['output_index'] for plan in plans
                               if any(os.path.basename(f) in ('b.json', 'b_short.json')
                                      for f in (plan['pairwise_options'].results_filename_a, plan['pairwise_options'].results_filename_b))]
        raise StopIteration

    with tempfile.TemporaryDirectory() as tmp:
        image_folder, files = S.build(tmp)
        real = C.compare_batch_results
        C.compare_batch_results = plan_only
        try:
            S.run(C, name, image_folder, files, os.path.join(tmp, 'out'))
        except StopIteration:
            pass
        finally:
            C.compare_batch_results = real
        jobs = captured['jobs']
        planned, host, undecodable = C.plan_device_jobs(jobs)
    handed = sorted((j['comparison'], j['file']) for j in host)
    drawn_thin = [j for j in jobs if j['file'] == S.THIN and j['comparison'] in captured['thin_in']]
    want = sorted([(j['comparison'], j['file']) for j in jobs if j['file'] == S.PNG] + [(j['comparison'], j['file']) for j in drawn_thin])
    assert handed == want, (name, handed, want)
    assert undecodable == ([S.PNG] if any(j['file'] == S.PNG for j in jobs) else []), (name, undecodable)
    return {'jobs': len(jobs), 'host': len(host), 'files_decoded_pil': len(undecodable),
            'files_decoded_gpu': len({j['file'] for j in planned})}


def main():
    import PIL
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    expected = {name: device_planning(name) for name in S.OPTION_SETS}
    for name in S.N_WAY_SETS:
        assert 0 < expected[name]['host'] < expected[name]['jobs'] and expected[name]['files_decoded_gpu'] < expected[name]['jobs'] - expected[name]['host']
        print(name, expected[name])
    ref = import_reference(sys.argv[1])
    golden = {'pillow': PIL.__version__, 'sets': {}}
    render = ref._render_image_pair
    sampled = []

    def recorded(fn, image_pairs, category_folder, options, pairwise_options):
        sampled.append([os.path.relpath(category_folder, options.output_folder).replace(os.sep, '/'), fn])
        return render(fn, image_pairs, category_folder, options, pairwise_options)

    ref._render_image_pair = recorded
    for name in S.OPTION_SETS:
        with tempfile.TemporaryDirectory() as tmp:
            image_folder, files = S.build(tmp)
            golden['scene'] = S.scene_hash(image_folder)
            out = os.path.join(tmp, 'out')
            del sampled[:]
            with redirect_stdout(io.StringIO()):
                results = S.run(ref, name, image_folder, files, out)
            assert results.html_output_file == os.path.join(out, 'index.html')
            record = S.describe_output(out, tmp)
            record['sampled'] = [list(s) for s in sampled]
            record['expected'] = expected[name]
            golden['sets'][name] = record
    path = os.path.join(REPO, 'tests', 'golden', 'compare_reference.json')
    with open(path, 'w') as f:
        f.write(S.pack_golden(golden))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
