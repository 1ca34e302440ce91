"""
visualize_db on the device: the scene of tests/visualize_db_scene.py, rebuilt from its seed, through every option set, on both
legs.  The two output trees must be equal file by file -- HTML and images -- and equal to the reference's own tree, and the
counts say which leg made each file: every JPEG of the scene -- 4:4:4, 4:2:2 and 4:2:0, the rotated and the 'L' file, the one
with a COM segment, odd sizes, reduced and left as they are, with boxes down to one pixel -- must have been decoded, resampled,
drawn on and encoded on the device, in one call of each kind per chunk.  Only the PNG may be counted as host: a fallback cannot
hide a wrong kernel.
"""

import os

import pytest

import visualize_db_scene as S
from megadetector_amd import device_render as DR
from test_visualize_db_cpu import GOLDEN, compare_output, rendered_names, run_set

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


def _both_legs(tmp_path, name, chunks=1):
    host, host_counts, _, _, host_order, _ = run_set(tmp_path / 'host', name, 'host')
    gpu, counts, _, exact, order, infos = run_set(tmp_path / 'gpu', name, 'gpu', profile=True)
    print(counts)
    host_files, gpu_files = _files(tmp_path / 'host'), _files(tmp_path / 'gpu')
    assert sorted(gpu_files) == sorted(host_files)
    for rel in sorted(host_files):
        assert gpu_files[rel] == host_files[rel], '{}: the device leg wrote {} bytes, the host leg {}'.format(
            rel, len(gpu_files[rel]), len(host_files[rel]))
    want = GOLDEN['sets'][name]
    compare_output(gpu, want, exact)                                      # and the reference's own tree, texts and files
    assert order == host_order == want['order']
    # which leg made what: the planted host case is the PNG (the COM file is written as Pillow writes it, on the device)
    rendered = rendered_names(want)
    on_host = [rel for rel in rendered if rel == 'rendered_images/pic_gt.jpg']
    assert counts['rendered'] == host_counts['rendered'] == len(rendered)
    assert counts['host'] == len(on_host) and counts['gpu'] == len(rendered) - len(on_host) and counts['gpu'] >= 1
    assert counts['files_decoded_gpu'] == counts['gpu'] and counts['files_decoded_pil'] == 0
    prefilled = S.OPTION_SETS[name].get('prefill', [])                   # (an existing file is skipped before its source is looked for)
    assert counts['unopened'] == host_counts['unopened'] == sum(n in ('gone_gt.jpg', 'broken~_gt.jpg') and n not in prefilled for n in order)
    assert counts['skipped'] == host_counts['skipped'] == len(prefilled)
    assert counts['sampled'] == host_counts['sampled'] == len(order)
    assert counts['decode_chunks'] == counts['encode_calls'] == chunks
    drawing = any(i['bboxes'] for i in infos if 'rendered_images/' + i['output_file_name'] in rendered and not i['img_path'].endswith('.png'))
    assert counts['draw_calls'] == (chunks if drawing else 0)
    assert counts['resample_calls'] == (0 if name in S.UNRESIZED_SETS else chunks)
    assert set(counts['ms']) >= {'decode', 'encode'} | ({'draw'} if drawing else set()) | (set() if name in S.UNRESIZED_SETS else {'resample'})
    # the images with thin boxes were made on the device: their file exists, and only the PNG was not
    for f in S.THIN:
        made = 'rendered_images/' + f.replace('/', '~').replace('.jpg', '') + '_gt.jpg'
        assert (made in rendered) == any(i['img_path'].endswith(f) for i in infos) or 'prefill' in S.OPTION_SETS[name]
    return counts


@pytest.mark.parametrize('name', sorted(S.OPTION_SETS))
def test_both_legs_write_the_same_tree_and_the_device_made_its_share(tmp_path, name):
    counts = _both_legs(tmp_path, name)
    if name == 'defaults':
        assert counts['gpu'] == len(S.FILES) - 3 and counts['host'] == 1 and counts['unopened'] == 2


def test_three_chunks(tmp_path, monkeypatch):
    # the decoded scene is 1.6 MB, its largest image 0.9 MB: three chunks under a limit of 0.7 MB
    monkeypatch.setattr(DR, 'DECODE_CHUNK_BYTES', 700000)
    counts = _both_legs(tmp_path, 'defaults', chunks=3)
    assert counts['gpu'] == len(S.FILES) - 3


def test_without_thin_outlines_the_host_leg_takes_those_images(tmp_path):
    _, counts, _, _, _, _ = run_set(tmp_path / 'on', 'defaults', 'gpu')
    _, without, _, _, _, _ = run_set(tmp_path / 'off', 'defaults', 'gpu', thin_outlines=False)
    assert without['host'] == counts['host'] + len(S.THIN) and without['gpu'] == counts['gpu'] - len(S.THIN)
    assert _files(tmp_path / 'on') == _files(tmp_path / 'off')
