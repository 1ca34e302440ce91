"""
separate_detections on the device: the scene of tests/separate_scene.py, rebuilt from its seed, through every option set that
draws boxes or blurs, on both legs.  The two output trees must be equal file by file, and the counts say which leg made each
file: every baseline RGB JPEG of the scene with two 8-bit tables and 4:4:4, 4:2:2 or 4:2:0 sampling -- and the rotated and the
'L' file, which are saved with the quality-85 tables -- must have been decoded, blurred, drawn on and encoded on the device.
Only the PNG and the images whose boxes carry classification labels may be counted as host: a fallback cannot hide a wrong
kernel.
"""

import io
import os
from contextlib import redirect_stdout

import pytest

import separate_scene as S
from megadetector_amd import separate_detections as SD
from test_separate_cpu import GOLDEN, compare_tree

pytestmark = pytest.mark.gpu

CLASSIFIED = {name for name, _, _, _, dets in S.IMAGES if dets and any('classifications' in d for d in dets)}


def _run(folder, name, backend, **kw):
    image_folder, results_file = S.build(folder)
    sources = S.source_hashes(image_folder)
    out = os.path.join(folder, 'out')
    if name == 'no_overwrite':
        S.prepare_existing(out)
    options = S.apply_options(SD.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out, S.OPTION_SETS[name])
    with redirect_stdout(io.StringIO()):
        counts = SD.separate_detections_into_folders(options, backend=backend, **kw)
    files = {}
    for root, _, names in os.walk(out):
        for n in names:
            with open(os.path.join(root, n), 'rb') as f:
                files[os.path.relpath(os.path.join(root, n), out).replace(os.sep, '/')] = f.read()
    return files, counts, S.describe_tree(out, sources)


def test_the_manipulating_sets_are_those_of_the_issue():
    assert {'render_boxes', 'blur_and_boxes', 'classification_labels', 'no_overwrite'} <= set(S.MANIPULATING)
    assert CLASSIFIED == {'sub/deer.jpg', 'sub/multi.jpg', 'sub/bird.jpg', 'sub/edge.jpg'}


@pytest.mark.parametrize('name', S.MANIPULATING)
def test_both_legs_write_the_same_tree_and_the_device_made_its_share(tmp_path, name):
    (tmp_path / 'host').mkdir()
    (tmp_path / 'gpu').mkdir()
    host_files, host_counts, _ = _run(str(tmp_path / 'host'), name, 'host')
    gpu_files, counts, tree = _run(str(tmp_path / 'gpu'), name, 'gpu', profile=True)
    print(counts)
    assert sorted(gpu_files) == sorted(host_files)
    for rel in sorted(host_files):
        assert gpu_files[rel] == host_files[rel], '{}: the device leg wrote {} bytes, the host leg {}'.format(rel, len(gpu_files[rel]), len(host_files[rel]))
    compare_tree(tree, GOLDEN['sets'][name]['tree'], False)              # and the reference's own tree: paths, copies, forms
    # which leg made what: the rendered files are those that are no byte copies (and were not there before)
    rendered = [rel for rel, e in GOLDEN['sets'][name]['tree'].items()
                if not e.get('empty_folder') and e.get('copy_of') is None and not (name == 'no_overwrite' and rel in S.EXISTING)]
    on_host = [rel for rel in rendered if rel.endswith('.png') or
               (name == 'classification_labels' and any(rel.endswith('/' + c) for c in CLASSIFIED))]
    assert counts['rendered'] == host_counts['rendered'] == len(rendered)
    assert counts['host'] == len(on_host) and counts['gpu'] == len(rendered) - len(on_host)
    assert counts['gpu'] >= 8 and counts['files_decoded_gpu'] == counts['gpu'] and counts['files_decoded_pil'] == 0
    assert counts['decode_chunks'] == 1 and counts['encode_calls'] == 1
    assert set(counts['ms']) >= {'decode', 'draw', 'encode'}
    for k in ('missing', 'exists', 'skipped', 'copied', 'moved'):
        assert counts[k] == host_counts[k]


def test_a_context_of_the_caller_is_used_and_left_open(tmp_path):
    from megadetector_amd.hip_backend import HipContext
    ctx = HipContext.for_images(0)
    try:
        _, counts, _ = _run(str(tmp_path), 'blur_and_boxes', 'gpu', ctx=ctx)
        assert counts['gpu'] >= 8 and ctx.h.value
        assert ctx.jpeg_encode_sampled_bound(8, 8, 0) > 0
    finally:
        ctx.close()
