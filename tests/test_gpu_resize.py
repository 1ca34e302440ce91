"""
Folder resizing on the GPU (megadetector_amd/resize_images.py): the device leg against the host leg over the scene and every
option set of tests/resize_scene.py -- byte-equal trees and equal result lists, which also equal what the reference's own
function returned and wrote (tests/golden/resize_reference.json) -- with the counts asserted: which files go to the host leg,
how many PIL decoded, one resample call and one encode call a decode chunk, no resample call where nothing is resized.  The same
for resize_coco_dataset.py over resize_scene.COCO_CASES: equal trees, equal JSON text, equal returned dicts, equal exceptions.
"""

import io
from contextlib import redirect_stdout

import os

import pytest

import resize_scene as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

#: what the device leg leaves to the host leg whatever the options: the GPU's decoder takes neither the progressive file nor the
#: truncated one, the PNGs are no JPEGs; with a target width of 64 the 300 x 2 file as well, whose height becomes 0 -- the
#: assertion is raised, and its text made, by the host leg
HOST_FILES = {'sub/prog.jpg', 'pic.png', 'palette.png', 'truncated.jpg', 'missing.jpg'}
DECODED_BY_PIL = {'sub/prog.jpg', 'pic.png', 'truncated.jpg'}
NOTHING_RESIZED = ('no_target', 'none_is_minus_one', 'no_target_quality_50')


@pytest.fixture(scope='module')
def ctx():
    from megadetector_amd.hip_backend import HipContext
    c = HipContext.for_images(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def golden():
    return S.load_golden(os.path.join(GOLDEN, 'resize_reference.json'))


def file_bytes(folder):
    out = {}
    for root, _, names in os.walk(folder):
        for n in names:
            with open(os.path.join(root, n), 'rb') as f:
                out[os.path.relpath(os.path.join(root, n), folder).replace(os.sep, '/')] = f.read()
    return out


@pytest.mark.parametrize('name', list(S.OPTION_SETS))
def test_device_leg_equals_host_leg_and_reference(ctx, tmp_path, golden, name):
    from megadetector_amd import resize_images as R
    counts = {}
    got, out_gpu = S.run_set(R.resize_image_folder, str(tmp_path / 'gpu'), name, backend='gpu', ctx=ctx, counts=counts)
    want, out_host = S.run_set(R.resize_image_folder, str(tmp_path / 'host'), name, backend='host')
    assert got == want
    assert file_bytes(out_gpu) == file_bytes(out_host)
    assert got == golden['resize'][name]['results'] and S.describe_tree(out_gpu) == golden['resize'][name]['tree']
    listed = [r['input_fn'][len('{IN}/'):] for r in got]
    skipped = {rel for rel, r in zip(listed, got) if r['status'] == 'skipped'}
    host = (HOST_FILES | ({'thin.jpg'} if S.OPTION_SETS[name].get('target_width') == 64 else set())) & set(listed) - skipped
    assert counts['files'] == len(listed) and counts['skipped'] == len(skipped)
    assert counts['host'] == len(host) and counts['gpu'] == len(listed) - len(skipped) - len(host)
    assert counts['files_decoded_gpu'] == counts['gpu'] and counts['files_decoded_pil'] == len(DECODED_BY_PIL & host)
    assert counts['errors'] == sum(r['status'] == 'error' for r in got)
    assert counts['resized'] + counts['unresized'] == sum(r['status'] == 'success' for r in got)
    assert counts['decode_chunks'] == 1 and counts['encode_calls'] == 1
    assert counts['resample_calls'] == (0 if name in NOTHING_RESIZED else 1)
    if name in NOTHING_RESIZED:
        assert counts['resized'] == 0


def test_one_resample_and_one_encode_call_a_chunk_in_place(tmp_path, monkeypatch):
    """several decode chunks, resizing in place: every chunk's inputs are read before its outputs are written"""
    from megadetector_amd import device_render, resize_images as R
    monkeypatch.setattr(device_render, 'DECODE_CHUNK_BYTES', 100000)        # two or three scene images a chunk
    counts = {}
    got, out_gpu = S.run_set(R.resize_image_folder, str(tmp_path / 'gpu'), 'in_place', backend='gpu', device=0, counts=counts, profile=True)
    want, out_host = S.run_set(R.resize_image_folder, str(tmp_path / 'host'), 'in_place', backend='host')
    assert got == want and file_bytes(out_gpu) == file_bytes(out_host)
    assert counts['decode_chunks'] >= 4 and counts['encode_calls'] == counts['decode_chunks']
    assert 1 <= counts['resample_calls'] <= counts['decode_chunks']
    assert counts['gpu'] == 10 and counts['host'] == 5 and {'decode', 'resample', 'encode'} <= set(counts['ms'])


def test_command_line_on_the_device(tmp_path, golden, capsys):
    from megadetector_amd import resize_images as R
    source, out = str(tmp_path / 'in'), str(tmp_path / 'out')
    S.build(source)
    assert R.main([source, out, '--target_width', '64', '--n_workers', '2']) == 0
    assert S.describe_tree(out) == golden['resize']['width_64']['tree']
    assert '15 files: 10 resized, 3 written unresized, 0 skipped, 2 errors (10 on the device, 5 on the host)' in capsys.readouterr().out


# ---- the COCO tool -----------------------------------------------------------------------------------------------------------------

#: images narrower than 96 pixels after the EXIF rotation: with no_enlarge_width the reference calls them "already that size"
NARROW = {'grey_l.jpg', 'grey_rgb.jpg', 'rot6.jpg', 'rot3.jpg', 'sub/rot8.jpg', 'sub/icc.jpg'}
#: case -> (what goes to the host leg beside HOST_FILES, resample calls): a copy is the host leg's, and so is an image whose
#: target height becomes 0 (the host leg raises the reference's text)
COCO_HOST = {
    'omit_width_64': ({'thin.jpg'}, 1),
    'omit_copy_equal': (NARROW | {'sub/com.jpg'}, 1),
    'omit_rewrite_equal': (set(), 1),
    'omit_copy_no_target': ('all', 0),
    'omit_rewrite_no_target': (set(), 0),
    'omit_no_enlarge_100': ({'thin.jpg'}, 1),
    'error_truncated': ({'sub/rot8.jpg'}, 0),               # 50 x 72 after its rotation: narrower than 64, a copy
}


def run_coco(tmp, name, **extra):
    from megadetector_amd import resize_coco_dataset as RC
    with redirect_stdout(io.StringIO()):
        return S.run_coco_case(str(tmp), name, RC.resize_coco_dataset, RC.main, **extra)


@pytest.mark.parametrize('name', list(S.COCO_CASES))
def test_coco_device_leg_equals_host_leg_and_reference(ctx, tmp_path, golden, name):
    counts = {}
    got = run_coco(tmp_path / 'gpu', name, **({'backend': 'gpu'} if name == 'cli' else {'backend': 'gpu', 'ctx': ctx, 'counts': counts}))
    want = run_coco(tmp_path / 'host', name, backend='host')
    assert got.get('error') == want.get('error') == golden['coco'][name].get('error')
    if 'error' in want:
        return
    assert got['json'] == want['json'] == golden['coco'][name]['json'] and got['returned_equal']
    assert file_bytes(str(tmp_path / 'gpu' / 'out')) == file_bytes(str(tmp_path / 'host' / 'out'))
    assert got['tree'] == golden['coco'][name]['tree']
    if name == 'cli':
        return
    listed = [im['file_name'] for im in S.coco_dataset(S.COCO_CASES[name].get('_only'))['images']]
    host, resample_calls = COCO_HOST[name]
    host = set(listed) if host == 'all' else (HOST_FILES | host) & set(listed)
    assert counts['files'] == len(listed) and counts['host'] == len(host) and counts['gpu'] == len(listed) - len(host)
    assert counts['files_decoded_gpu'] == counts['gpu'] and counts['decode_chunks'] == 1
    assert counts['encode_calls'] == (1 if counts['gpu'] else 0) and counts['resample_calls'] == resample_calls
