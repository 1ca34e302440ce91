"""
visualize_video_output on the device: the small Motion-JPEG AVI files of tests/video_render_scene.py -- 64 x 48 and 70 x 50,
one each of 4:4:4, 4:2:2 (implied Huffman tables) and 4:2:0 (a dropped frame), and one with a progressive frame -- through
every quality mode, with and without blur, with and without classification labels, on both legs.  The files of the two legs
must be equal byte for byte, and the counts say which leg made each frame: only the progressive frame and the frame with a box
thinner than its outline may be counted under frames_host, so a fallback cannot hide a wrong kernel.  The four videos differ
in size and sampling and share ONE chunk: one decode, one blur, one draw and one encoder call.
"""

import json
import os

import pytest

import video_render_scene as S
from megadetector_amd import device_render as DR
from megadetector_amd import visualize_video_output as V
from test_video_render_cpu import MODES, host_run, quiet

pytestmark = pytest.mark.gpu

#: file -> the frames the device does not restate
ON_HOST = {'v444.avi': 1, 'v422.avi': 0, 'sub/v420.avi': 0, 'sub/prog.avi': 1}


@pytest.mark.parametrize('classified', [False, True])
@pytest.mark.parametrize('blur', [False, True])
@pytest.mark.parametrize('mode', sorted(MODES))
def test_both_legs_write_the_same_videos_and_the_device_made_its_share(tmp_path_factory, mode, blur, classified):
    host = host_run(tmp_path_factory, mode, blur, classified)
    profile = {'ms': {}}
    gpu = host_run(tmp_path_factory, mode, blur, classified, backend='gpu', profile=profile)
    print(profile, gpu['results'])
    touched = S.N_FRAMES if mode == 'q75' else 4
    for r, h in zip(gpu['results'], host['results']):
        assert r['success'] and r['error'] is None and r['frames_processed'] == S.N_FRAMES
        assert (r['file'], r['frames_copied'], r['frames_rendered']) == (h['file'], S.N_FRAMES - touched, touched) == \
            (h['file'], h['frames_copied'], h['frames_rendered'])
        assert r['frames_host'] == ON_HOST[r['file']], r
    for name in S.SMALL_VIDEOS:
        for i, (a, b) in enumerate(zip(gpu['out'][name], host['out'][name])):
            assert a == b, '{} frame {}: the device leg wrote {} bytes, the host leg {}'.format(name, i, len(a), len(b))
        assert gpu['raw'][name] == host['raw'][name]
    assert profile['chunks'] == 1 and profile['decode_calls'] == 1 and profile['draw_calls'] == 1 and profile['encode_calls'] == 1
    assert profile['blur_calls'] == (1 if blur else 0)
    assert set(profile['ms']) == {'decode', 'draw', 'encode_kept' if mode == 'keep_blocks' else 'encode'} | ({'blur'} if blur else set())


def test_a_chunk_of_several_videos_gives_the_files_of_one_video_a_chunk(tmp_path_factory, tmp_path):
    together = host_run(tmp_path_factory, 'keep_blocks', True, True, backend='gpu', profile={})
    video_dir, results_file, _ = S.build_small(str(tmp_path), classified=True, thin=True)
    with open(results_file) as f:
        results = json.load(f)
    sizes = {S.SMALL_VIDEOS[name]['size'] for name in S.SMALL_VIDEOS}
    assert len(sizes) == 2 and len({S.SMALL_VIDEOS[name]['sampling'] for name in S.SMALL_VIDEOS}) == 3
    for k, entry in enumerate(results['images']):
        one = str(tmp_path / 'one_{}.json'.format(k))
        with open(one, 'w') as f:
            json.dump(dict(results, images=[entry]), f)
        profile = {}
        out_dir = str(tmp_path / 'out_{}'.format(k))
        r = quiet(V.visualize_video_output, one, out_dir, video_dir, together['options'], backend='gpu', profile=profile)
        assert len(r) == 1 and r[0]['success'] and profile['chunks'] == 1
        with open(os.path.join(out_dir, entry['file']), 'rb') as f:
            assert f.read() == together['raw'][entry['file']], entry['file']


def test_small_chunks_give_the_same_files(tmp_path_factory, tmp_path, monkeypatch):
    """a chunk limit of two 70 x 50 frames: a video's frames arrive over several chunks, and chunks end inside a video"""
    together = host_run(tmp_path_factory, 'q75', True, False, backend='gpu', profile={})
    video_dir, results_file, _ = S.build_small(str(tmp_path), classified=False, thin=True)
    monkeypatch.setattr(DR, 'DECODE_CHUNK_BYTES', 2 * 70 * 50 * 3)
    profile = {}
    out_dir = str(tmp_path / 'out')
    quiet(V.visualize_video_output, results_file, out_dir, video_dir, together['options'], backend='gpu', profile=profile)
    assert profile['chunks'] >= 11 and profile['encode_calls'] == profile['chunks']
    for name in S.SMALL_VIDEOS:
        with open(os.path.join(out_dir, name), 'rb') as f:
            assert f.read() == together['raw'][name], name


def test_a_context_of_the_caller_is_used_and_left_open(tmp_path):
    from megadetector_amd.hip_backend import HipContext
    video_dir, results_file, _ = S.build_small(str(tmp_path))
    ctx = HipContext.for_images(0)
    try:
        results = quiet(V.visualize_video_output, results_file, str(tmp_path / 'out'), video_dir, backend='gpu', ctx=ctx)
        assert all(r['success'] for r in results) and ctx.h.value
        assert ctx.jpeg_encode_sampled_bound(8, 8, 0) > 0
    finally:
        ctx.close()


# ---- the same pass ---------------------------------------------------------------------------------------------------------------

IMAGE_SIZE = 256


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """the smallest checkpoint file of the GPU tests (test_gpu_parity: the pickle layout of md_v5a.0.0.pt, nano widths)"""
    import fake_yolov5 as FY
    from megadetector_amd import yolo_yaml
    path = str(tmp_path_factory.mktemp('ckpt') / 'md_fake.pt')
    FY.save_checkpoint(FY.build_model(yolo_yaml.YOLOV5N6_TEST, seed=5), path)
    return path


@pytest.fixture(scope='module')
def detector(checkpoint):
    from megadetector_amd import run_detector
    return run_detector.load_detector(checkpoint, detector_options={'batch_size': 4, 'max_image_size': IMAGE_SIZE})


def drawable_threshold(results_file):
    """Seeded weights give many small boxes, and a box thinner than its outline sends its frame to the host leg: the highest
    confidence of the file at which some frame has boxes and all of them can be planned, so that the run has a frame for the
    device to draw on.  Chooses the test's input; what is asserted does not depend on it."""
    from megadetector_amd import preview as PV_
    from megadetector_amd.constants import DEFAULT_DETECTOR_LABEL_MAP
    with open(results_file) as f:
        images = [im for im in json.load(f)['images'] if im.get('detections')]
    planner = V.FramePlanner(DEFAULT_DETECTOR_LABEL_MAP, {}, V.VideoVisualizationOptions())
    for c in sorted({d['conf'] for im in images for d in im['detections']}, reverse=True):
        for im in images:
            w, h = S.SMALL_VIDEOS[im['file']]['size']
            for n in im['frames_processed']:
                dets = [d for d in im['detections'] if d['frame_number'] == n and d['conf'] >= c]
                try:
                    if dets and planner.ops(dets, w, h)[0]:
                        return c
                except (PV_.HostLeg, PV_.RenderFailure):
                    pass
    raise AssertionError('no frame of the run can be drawn on the device at any threshold')


@pytest.mark.parametrize('name', ['blur_keep_blocks', 'default', 'q75_trim_fs'])
def test_the_pass_writes_the_tools_files_from_the_images_it_decoded(tmp_path, checkpoint, detector, name):
    """process_videos(mjpeg='gpu', render_folder=) with the stub-weights detector: the files the standalone tool writes from its
    JSON, the JSON of a run without the folder, and frames made by the detector's render= product from the device images"""
    from megadetector_amd import process_video as PV
    from test_video_render_pass_cpu import VARIANTS, json_text, options_of, plain, tree
    video_dir, _, _ = S.build_small(str(tmp_path))

    def options():
        o = options_of(name)
        o.confidence_threshold = threshold
        return o

    kw = dict(frame_sample=1, batch_size=4, detector=detector, image_size=IMAGE_SIZE, json_confidence_threshold=0.001, mjpeg='gpu')
    plain_json, pass_json = str(tmp_path / 'plain.json'), str(tmp_path / 'pass.json')
    quiet(PV.process_videos, checkpoint, video_dir, plain_json, **kw)
    threshold = drawable_threshold(plain_json)
    made_before, in_pass = detector.render_counts['gpu'], []
    quiet(PV.process_videos, checkpoint, video_dir, pass_json, render_folder=str(tmp_path / 'pass'), render_options=options(),
          render_results=in_pass, **kw)
    assert json_text(pass_json) == json_text(plain_json)
    tool = quiet(V.visualize_video_output, pass_json, str(tmp_path / 'tool'), video_dir, options(), backend='gpu')
    print(name, in_pass, tool)
    got, want = tree(str(tmp_path / 'pass')), tree(str(tmp_path / 'tool'))
    assert sorted(got) == sorted(want) and len(got) > 0
    for rel in sorted(want):
        assert got[rel] == want[rel], rel
    key = lambda r: r['file']
    assert plain(sorted(in_pass, key=key)) == plain(sorted(tool, key=key))
    on_device = sum(r['frames_rendered'] - r['frames_host'] for r in in_pass)
    assert on_device > 0 and detector.render_counts['gpu'] - made_before >= on_device
