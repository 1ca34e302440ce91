"""
compare_batch_results on the device: the three-file n-way run on the scene of tests/compare_scene.py with backend='gpu' and
with backend='host', against each other file by file and against the recorded reference tree and HTML
(tests/golden/compare_reference.json), enlarging (the default width of 800), reducing (80) and at the files' own sizes.
The counts say where the work was done: the host leg got the planted jobs only (the PNG's and those with the thin box), and
each file was decoded ONCE for all the comparisons that draw on it.
"""

import io
import os
from contextlib import redirect_stdout

import pytest

import compare_scene as S
from conftest import REPO
from megadetector_amd import compare_batch_results as C

pytestmark = pytest.mark.gpu

GOLDEN = S.load_golden(os.path.join(REPO, 'tests', 'golden', 'compare_reference.json'))


def _run(tmp, name, backend):
    image_folder, files = S.build(tmp)
    out = os.path.join(tmp, 'out_' + backend)
    with redirect_stdout(io.StringIO()):
        results = S.run(C, name, image_folder, files, out, backend=backend)
    return out, S.describe_output(out, tmp), results.counts


@pytest.mark.parametrize('name', S.N_WAY_SETS)
def test_the_device_leg_writes_the_host_legs_files_and_decodes_each_file_once(tmp_path, name):
    tmp = str(tmp_path)
    want = GOLDEN['sets'][name]
    out_gpu, gpu, counts = _run(tmp, name, 'gpu')
    out_host, host, host_counts = _run(tmp, name, 'host')
    print(name, counts)
    assert gpu['tree'] == host['tree'] == want['tree']
    for page, text in want['html'].items():
        assert gpu['html'][page].replace('out_gpu', 'out') == text, page
        assert host['html'][page].replace('out_host', 'out') == text, page
    differing = [rel for rel in host['sha256'] if gpu['sha256'][rel] != host['sha256'][rel]]
    assert not differing, differing
    e = want['expected']
    assert counts['jobs'] == e['jobs'] == len(want['sha256']) and host_counts['host'] == e['jobs']
    # a condition, not a measurement: a device leg that hands everything to the host fails here
    assert counts['host'] == e['host'] and counts['gpu'] == e['jobs'] - e['host']
    assert counts['files_decoded_pil'] == e['files_decoded_pil'] == 1
    # each distinct JPEG once, not once per comparison
    assert counts['files_decoded_gpu'] == e['files_decoded_gpu'] < counts['gpu']
    assert counts['decode_chunks'] >= 1
    assert counts['resample_calls'] == (0 if name == 'n_way_none' else counts['decode_chunks'])
    assert counts['draw_calls'] == counts['encode_calls'] == counts['decode_chunks']
