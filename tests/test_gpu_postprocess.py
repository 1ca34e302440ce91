"""
postprocess_batch_results on the device: the scene of tests/postprocess_scene.py, rebuilt from its seed, through every option
set that renders, on both legs.  The two output trees must be equal file by file -- HTML and images -- and equal to the
reference's own tree, and the counts say which leg made each file: every JPEG of the scene -- 4:4:4, 4:2:2 and 4:2:0, the
rotated and the 'L' file, odd sizes, reduced, enlarged and left as they are -- must have been decoded, resampled, drawn on and
encoded on the device, in one call of each kind.  Only the PNG may be counted as host: a fallback cannot hide a wrong kernel.
"""

import os

import pytest

import postprocess_scene as S
from test_postprocess_cpu import GOLDEN, compare_output, run_set

pytestmark = pytest.mark.gpu


def _files(tmp):
    files = {}
    out = os.path.join(str(tmp), 'out')
    for root, _, names in os.walk(out):
        for n in names:
            with open(os.path.join(root, n), 'rb') as f:
                data = f.read()
            if n.endswith('.html'):
                data = data.replace(str(tmp).encode(), b'<tmp>')
            files[os.path.relpath(os.path.join(root, n), out).replace(os.sep, '/')] = data
    return files


def _both_legs(tmp_path, name):
    host, host_counts, _, _ = run_set(tmp_path / 'host', name, 'host')
    gpu, counts, _, exact = run_set(tmp_path / 'gpu', name, 'gpu', profile=True)
    print(counts)
    host_files, gpu_files = _files(tmp_path / 'host'), _files(tmp_path / 'gpu')
    assert sorted(gpu_files) == sorted(host_files)
    for rel in sorted(host_files):
        assert gpu_files[rel] == host_files[rel], '{}: the device leg wrote {} bytes, the host leg {}'.format(
            rel, len(gpu_files[rel]), len(host_files[rel]))
    compare_output(gpu, GOLDEN['sets'][name], exact)                     # and the reference's own tree, texts and files
    # which leg made what
    rendered = list(GOLDEN['sets'][name]['sha256'])
    on_host = [rel for rel in rendered if rel.endswith('.png')]
    assert counts['rendered'] == host_counts['rendered'] == len(rendered)
    assert counts['host'] == len(on_host) and counts['gpu'] == len(rendered) - len(on_host) and counts['gpu'] >= 4
    assert counts['files_decoded_gpu'] == counts['gpu'] and counts['files_decoded_pil'] == 0
    assert counts['unopened'] == host_counts['unopened'] == sum(1 for f in GOLDEN['sets'][name]['sampled'] if 'gone' in f or 'lost' in f)
    assert counts['bypassed'] == host_counts['bypassed'] and counts['sampled'] == host_counts['sampled']
    assert counts['decode_chunks'] == counts['draw_calls'] == counts['encode_calls'] == 1
    return counts


@pytest.mark.parametrize('name', [n for n in S.OPTION_SETS if n not in S.WIDTH_SETS])
def test_both_legs_write_the_same_tree_and_the_device_made_its_share(tmp_path, name):
    counts = _both_legs(tmp_path, name)
    assert counts['resample_calls'] == 1
    assert set(counts['ms']) >= {'decode', 'resample', 'draw', 'encode'}
    if 'sample' not in name:
        assert counts['unopened'] == 1


@pytest.mark.parametrize('name', S.WIDTH_SETS)
def test_reducing_enlarging_and_keeping_the_size(tmp_path, name):
    counts = _both_legs(tmp_path, name)
    assert counts['unopened'] == 1
    assert counts['resample_calls'] == (0 if name == 'width_none' else 1)
    assert counts['gpu'] == len(S.IMAGES) - 2                            # all but the PNG and the image that failed
