"""
visualize_video_output without a GPU: the restated control flow against what the reference's own module decided
(tests/golden/video_render_reference.json), the AVI writer against the reader and against a second parser written from the
layout, and the host leg frame by frame against direct Pillow calls.
"""

import io
import json
import os
import struct
from contextlib import redirect_stdout

import numpy as np
import pytest
from PIL import Image, ImageFilter, JpegImagePlugin

import video_render_scene as S
from megadetector_amd import avi
from megadetector_amd import device_render as DR
from megadetector_amd import jpeg_host as J
from megadetector_amd import preview as PV
from megadetector_amd import visualize_video_output as V
from test_keep_blocks_cpu import _block_mask, changed_mcus

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'video_render_reference.json')) as _f:
    GOLDEN = json.load(_f)


def quiet(function, *args, **kwargs):
    with redirect_stdout(io.StringIO()):
        return function(*args, **kwargs)


# ---- the control flow ------------------------------------------------------------------------------------------------------------

def test_the_golden_is_of_this_scene_and_covers_what_it_must():
    assert GOLDEN['results'] == json.loads(json.dumps(S.RESULTS))
    assert set(GOLDEN['sets']) == set(S.OPTION_SETS) and len(S.OPTION_SETS) >= 10
    errors = {r['result']['error'] for recs in GOLDEN['sets'].values() for r in recs if r['result']['error']}
    for start in ('Ignoring failed video', 'Video not found', 'Skipped: ', 'Skipped, below minimum length', V.NO_FRAMES_STRING):
        assert any(e.startswith(start) for e in errors), start
    assert any(any('classifications' in d for dets in r.get('detections', []) for d in dets) for r in GOLDEN['sets']['default'])


def test_options_have_the_references_names_and_defaults():
    o = V.VideoVisualizationOptions()
    expected = dict(confidence_threshold=0.15, sample=-1, random_seed=None, classification_confidence_threshold=0.4, rendering_fs='auto',
                    trim_to_detections=False, output_extension=None, flatten_output=False, path_separator_replacement='#',
                    min_output_length_seconds=None, parallelize_rendering=True, parallelize_rendering_n_cores=8,
                    parallelize_rendering_with_threads=True, include_category_names_in_filenames=None,
                    exclude_category_name_strings=None, exclude_category_names=None, include_category_names=None,
                    fourcc='MJPG', blur_category_names=None, blur_radius=40, quality='keep', keep_source_blocks=False)
    assert vars(o) == expected


@pytest.mark.parametrize('name', sorted(S.OPTION_SETS))
def test_control_flow_is_the_references(tmp_path, name):
    """plan_video and the entry function's filter and sampling, per video: the result dict field for field, the output path,
    the frame rate, the frames requested and the detections handed to the renderer"""
    import random
    video_dir, results_file = S.build(str(tmp_path))
    out_dir = os.path.join(str(tmp_path), 'out')
    options = S.apply_options(V.VideoVisualizationOptions(), S.OPTION_SETS[name])
    entries = [e for e in S.RESULTS['images'] if V.is_video_file(e['file'])]
    if options.sample > 0 and len(entries) > options.sample:         # visualize_video_output :664-670
        random.seed(options.random_seed)
        entries = random.sample(entries, options.sample)
    records = GOLDEN['sets'][name]
    assert [e['file'] for e in entries] == [r['result']['file'] for r in records]
    for entry, record in zip(entries, records):
        result, plan = quiet(V.plan_video, entry, S.CLASSIFICATION_CATEGORIES, options, video_dir, out_dir)
        expected = dict(record['result'])
        if expected.pop('raises', None) is not None:
            # the reference formats a variable that was never bound: our reading skips the video
            assert plan is None and result == {'file': entry['file'], 'success': False, 'error': 'Skipped: none', 'frames_processed': 0}
            continue
        if expected['error'] is not None:
            expected['error'] = expected['error'].replace('<tmp>', str(tmp_path))
        if 'output' not in record:
            assert plan is None and result == expected
            continue
        assert plan is not None and result == {'file': entry['file'], 'success': False, 'error': None, 'frames_processed': 0}
        assert expected['success'] and expected['frames_processed'] == len(plan['frames']) == record['frames_written']
        assert os.path.relpath(plan['output'], out_dir).replace(os.sep, '/') == record['output']
        assert os.path.isdir(os.path.dirname(plan['output']))
        assert plan['fps'] == record['fps'] and plan['frames'] == record['frames']
        handed = [V._get_detections_for_frame(entry, n, options.confidence_threshold) for n in plan['frames']]
        assert json.loads(json.dumps(handed)) == record['detections']


def test_entry_function_filters_samples_and_reports_as_the_reference(tmp_path):
    """over files that are no AVI at all: every video the reference would open is 'not a Motion-JPEG AVI' here"""
    video_dir, results_file = S.build(str(tmp_path))
    options = S.apply_options(V.VideoVisualizationOptions(), S.OPTION_SETS['sample_3'])
    results = quiet(V.visualize_video_output, results_file, os.path.join(str(tmp_path), 'out'), video_dir, options, backend='host')
    records = GOLDEN['sets']['sample_3']
    assert [r['file'] for r in results] == [rec['result']['file'] for rec in records]
    for r, rec in zip(results, records):
        assert r['success'] is False and r['frames_processed'] == 0
        assert r['frames_copied'] == r['frames_rendered'] == r['frames_host'] == 0
        if rec['result']['success']:
            assert r['error'].startswith(V.NOT_MJPEG_STRING)
        else:
            assert r['error'] == rec['result']['error']
    with pytest.raises(ValueError, match='cannot be the same'):
        quiet(V.visualize_video_output, results_file, video_dir, video_dir, V.VideoVisualizationOptions(), backend='host')


def test_options_of_ours_are_checked():
    for attribute, value, error in (('fourcc', 'h264', NotImplementedError), ('fourcc', 'mp4v', NotImplementedError),
                                    ('quality', 96, ValueError), ('quality', 0, ValueError), ('blur_radius', -1, ValueError)):
        o = V.VideoVisualizationOptions()
        setattr(o, attribute, value)
        with pytest.raises(error):
            V.check_options(o)
    o = V.VideoVisualizationOptions()
    o.quality, o.keep_source_blocks = 75, True
    with pytest.raises(ValueError, match='keep_source_blocks'):
        V.check_options(o)


# ---- the writer ------------------------------------------------------------------------------------------------------------------

ODD_FRAMES = [b'\xff\xd8' + bytes(range(k)) + b'\xff\xd9' for k in (5, 8, 1, 0, 33)] + [b'']


def parse_avi(data):
    """a second reader, from the layout alone: -> dict of the header fields, the movi chunks and the index"""
    def u32(p):
        return struct.unpack_from('<I', data, p)[0]

    out = {}
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    out['riff_size'] = u32(4)
    assert out['riff_size'] == len(data) - 8
    p = 12
    assert data[p:p + 4] == b'LIST' and data[p + 8:p + 12] == b'hdrl'
    hdrl_end = p + 8 + u32(p + 4)
    q = p + 12
    assert data[q:q + 4] == b'avih' and u32(q + 4) == 56
    out['avih'] = struct.unpack_from('<14I', data, q + 8)
    q += 8 + 56
    assert data[q:q + 4] == b'LIST' and data[q + 8:q + 12] == b'strl'
    assert q + 8 + u32(q + 4) == hdrl_end, 'LIST strl ends where LIST hdrl ends'
    q += 12
    assert data[q:q + 4] == b'strh' and u32(q + 4) == 56
    out['strh'] = struct.unpack_from('<4s4sIHHIIIIIIII4H', data, q + 8)
    q += 8 + 56
    assert data[q:q + 4] == b'strf' and u32(q + 4) == 40
    out['strf'] = struct.unpack_from('<IiiHH4sIiiII', data, q + 8)
    q += 8 + 40
    assert q == hdrl_end
    p = hdrl_end
    assert data[p:p + 4] == b'LIST' and data[p + 8:p + 12] == b'movi'
    movi_tag, movi_end = p + 8, p + 8 + u32(p + 4)
    chunks, q = [], p + 12
    while q < movi_end:
        assert data[q:q + 4] == b'00dc'
        n = u32(q + 4)
        chunks.append((q, n, data[q + 8:q + 8 + n]))
        if n & 1:
            assert data[q + 8 + n] == 0, 'the pad byte'
        q += 8 + n + (n & 1)
        assert q % 2 == 0, 'every chunk begins at an even offset'
    assert q == movi_end
    out['chunks'], out['movi_tag'] = chunks, movi_tag
    p = movi_end
    assert data[p:p + 4] == b'idx1' and u32(p + 4) == 16 * len(chunks)
    out['idx1'] = [struct.unpack_from('<4sIII', data, p + 8 + 16 * k) for k in range(len(chunks))]
    assert p + 8 + 16 * len(chunks) == len(data)
    return out


@pytest.mark.parametrize('fps, rate_scale, usec', [(30, (30, 1), 33333), (12.5, (25, 2), 80000), (29.97, (2997, 100), 33367),
                                                   (1.4985, (749, 500), 667334), (7.5, (15, 2), 133333)])
def test_writer_layout_by_a_second_parser(tmp_path, fps, rate_scale, usec):
    path = str(tmp_path / 'out.avi')
    assert avi.write_mjpeg_avi(path, iter(ODD_FRAMES), fps, 70, 50) == len(ODD_FRAMES)
    assert not os.path.exists(path + '.part')
    with open(path, 'rb') as f:
        data = f.read()
    a = parse_avi(data)
    n, largest = len(ODD_FRAMES), max(len(f) for f in ODD_FRAMES)
    assert a['riff_size'] == avi.riff_size(len(f) for f in ODD_FRAMES) <= avi.RIFF_SIZE_LIMIT
    assert a['avih'] == (usec, 0, 0, 0x10, n, 0, 1, largest, 70, 50, 0, 0, 0, 0)
    assert usec == round(1e6 / fps)
    assert a['strh'] == (b'vids', b'MJPG', 0, 0, 0, 0, rate_scale[1], rate_scale[0], 0, n, largest, 0xFFFFFFFF, 0, 0, 0, 70, 50)
    assert a['strf'] == (40, 70, 50, 1, 24, b'MJPG', 70 * 50 * 3, 0, 0, 0, 0)
    assert [c[2] for c in a['chunks']] == ODD_FRAMES
    for (pos, size, _), (ckid, flags, offset, length) in zip(a['chunks'], a['idx1']):
        assert (ckid, flags, length) == (b'00dc', 0x10, size)
        assert a['movi_tag'] + offset == pos, 'an index offset counts from the movi tag to the chunk header'


def test_writer_round_trip_through_the_reader(tmp_path):
    frames = S.small_video(str(tmp_path / 'src' / 'a.avi'), (70, 50), '422', 9)
    path = str(tmp_path / 'out.avi')
    avi.write_mjpeg_avi(path, frames, 12.5, 70, 50)
    with avi.AviFile(path) as a:
        assert (a.n_frames, a.width, a.height, a.frame_rate) == (len(frames), 70, 50, 12.5)
        assert [a.read_frame(i) for i in range(a.n_frames)] == frames
    avi.write_mjpeg_avi(path, (f for f in frames[:2]), 29.97, 70, 50)         # an iterator, over an existing file
    with avi.AviFile(path) as a:
        assert a.n_frames == 2 and a.frame_rate == 29.97


class _Long(bytes):
    """three bytes that claim to be many"""
    claimed = 0

    def __len__(self):
        return self.claimed


def test_writer_refuses_a_file_past_2_31_before_it_writes(tmp_path):
    path = str(tmp_path / 'big.avi')
    big = _Long(b'abc')
    big.claimed = 1 << 30
    assert avi.riff_size([1 << 30, 1 << 30]) > avi.RIFF_SIZE_LIMIT >= avi.riff_size([1 << 30])
    with pytest.raises(avi.AviError, match='AVI 1.0'):
        avi.write_mjpeg_avi(path, [big, big], 30, 64, 48)
    assert os.listdir(str(tmp_path)) == []
    # an iterator's lengths are not known in front: the frame that passes the limit ends the writing, nothing stays
    small = b'\xff\xd8\xff\xd9'
    limit = avi.RIFF_SIZE_LIMIT
    try:
        avi.RIFF_SIZE_LIMIT = avi.riff_size([4, 4]) + 3
        with pytest.raises(avi.AviError, match='frame 2'):
            avi.write_mjpeg_avi(path, iter([small, small, small]), 30, 64, 48)
    finally:
        avi.RIFF_SIZE_LIMIT = limit
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(avi.AviError):
        avi.write_mjpeg_avi(path, [small], 0, 64, 48)
    # the exact boundary: the largest single frame
    room = avi.RIFF_SIZE_LIMIT - avi.riff_size([0])
    assert room % 2 == 1 and avi.riff_size([room - 1]) == avi.RIFF_SIZE_LIMIT - 1 and avi.riff_size([room]) == avi.RIFF_SIZE_LIMIT + 1


# ---- the host leg, frame by frame ------------------------------------------------------------------------------------------------

MODES = {'keep': dict(quality='keep'), 'keep_blocks': dict(quality='keep', keep_source_blocks=True), 'q75': dict(quality=75)}
_RUNS = {}


def host_run(tmp_path_factory, mode, blur=False, classified=False, backend='host', **kw):
    """the tool over the small scene, once per combination: -> dict(results, out={file: [frames]}, stored, video_dir, options)"""
    key = (mode, blur, classified, backend)
    if key not in _RUNS:
        tmp = str(tmp_path_factory.mktemp('vr_{}_{}_{}_{}'.format(*key)))
        video_dir, results_file, stored = S.build_small(tmp, classified=classified, thin=True)
        options = V.VideoVisualizationOptions()
        options.parallelize_rendering = False
        options.classification_confidence_threshold = 0.3
        for k, v in MODES[mode].items():
            setattr(options, k, v)
        if blur:
            options.blur_category_names = 'person'
            options.blur_radius = 6
        out_dir = os.path.join(tmp, 'out')
        results = quiet(V.visualize_video_output, results_file, out_dir, video_dir, options, backend=backend, **kw)
        out, raw = {}, {}
        for name in S.SMALL_VIDEOS:
            with open(os.path.join(out_dir, name), 'rb') as f:
                raw[name] = f.read()
            with avi.AviFile(os.path.join(out_dir, name)) as a:
                out[name] = [a.read_frame(i) for i in range(a.n_frames)]
                assert (a.width, a.height) == S.SMALL_VIDEOS[name]['size'] and a.frame_rate == 30.0
        _RUNS[key] = dict(results=results, out=out, raw=raw, stored=stored, options=options, results_file=results_file)
    return _RUNS[key]


def stored_frame(stored, name, i):
    """the stored frame as the reader serves it (a dropped frame repeats the one before), with its tables written in"""
    while stored[name][i] == b'':
        i -= 1
    return J.with_standard_tables(stored[name][i])


def frame_detections(results_file, name, i, threshold=0.15):
    with open(results_file) as f:
        entry = next(e for e in json.load(f)['images'] if e['file'] == name)
    return [d for d in entry['detections'] if d['frame_number'] == i and d['conf'] >= threshold]


def pillow_pixels(data, dets, blur, classified):
    """the frame as direct Pillow calls make it: decode, blur the people (most confident first), draw"""
    image = Image.open(io.BytesIO(data))
    image.load()
    if image.mode != 'RGB':
        image = image.convert('RGB')
    w, h = image.size
    if blur:
        for d in sorted((d for d in dets if d['category'] == '2'), key=lambda d: -d['conf']):
            x, y, bw, bh = d['bbox']
            rect = (max(0, int(x * w)), max(0, int(y * h)), min(w, int(x * w) + int(bw * w)), min(h, int(y * h) + int(bh * h)))
            image.paste(image.crop(rect).filter(ImageFilter.GaussianBlur(radius=6)), rect[:2])
    o = PV.PreviewOptions(confidence_threshold=0, output_image_width=None)
    if classified and any('classifications' in d for d in dets):
        PV.render_with_pil(image, dets, o, S.DETECTION_CATEGORIES, classification_label_map=S.CLASSIFICATION_CATEGORIES,
                           classification_confidence_threshold=PV.DEFAULT_CLASSIFICATION_CONFIDENCE_THRESHOLD)
    else:
        PV.render_with_pil(image, dets, o, label_map=S.DETECTION_CATEGORIES)
    return image


def pillow_file(image, mode):
    out = io.BytesIO()
    if mode == 'q75':
        image.save(out, 'JPEG', quality=75)
    else:
        image.save(out, 'JPEG', qtables=image.quantization, subsampling=JpegImagePlugin.get_sampling(image))
    return out.getvalue()


@pytest.mark.parametrize('classified', [False, True])
@pytest.mark.parametrize('blur', [False, True])
@pytest.mark.parametrize('mode', ['keep', 'q75'])
def test_host_leg_frames_are_pillows(tmp_path_factory, mode, blur, classified):
    run = host_run(tmp_path_factory, mode, blur, classified)
    for r in run['results']:
        assert r['success'] and r['error'] is None and r['frames_processed'] == S.N_FRAMES
        touched = 4 if mode == 'keep' else S.N_FRAMES
        assert (r['frames_copied'], r['frames_rendered'], r['frames_host']) == (S.N_FRAMES - touched, touched, touched)
    for name in S.SMALL_VIDEOS:
        assert len(run['out'][name]) == S.N_FRAMES
        for i in range(S.N_FRAMES):
            data = stored_frame(run['stored'], name, i)
            dets = frame_detections(run['results_file'], name, i)
            got = run['out'][name][i]
            if mode == 'keep' and not dets:
                assert i in (0, 3) and got == data, '{} frame {}: a pass-through frame is the stored frame'.format(name, i)
                continue
            image = pillow_pixels(data, dets, blur, classified)
            assert got == pillow_file(image, mode), '{} frame {}'.format(name, i)
            if mode == 'keep' and i != S.SMALL_VIDEOS[name].get('progressive_frame'):
                a, b = J.parse(got), J.parse(data)
                assert (a.quant == b.quant).all() and J.sampling_of(a) == J.sampling_of(b)


def test_pass_through_writes_the_implied_tables_in(tmp_path_factory):
    run = host_run(tmp_path_factory, 'keep')
    raw = run['stored']['v422.avi'][0]
    assert b'\xff\xc4' not in raw and J.with_standard_tables(raw) != raw
    assert run['out']['v422.avi'][0] == J.with_standard_tables(raw)
    Image.open(io.BytesIO(run['out']['v422.avi'][0])).load()
    assert run['stored']['sub/v420.avi'][3] == b'' and run['out']['sub/v420.avi'][3] == stored_frame(run['stored'], 'sub/v420.avi', 2)


def test_classification_threshold_reaches_the_labels(tmp_path_factory):
    """the 0.45 line of frame 4 is drawn at a threshold of 0.3 and not at one of 0.5"""
    run = host_run(tmp_path_factory, 'keep', False, True)
    data = stored_frame(run['stored'], 'v422.avi', 4)
    dets = frame_detections(run['results_file'], 'v422.avi', 4)
    options = V.VideoVisualizationOptions()
    options.classification_confidence_threshold = 0.5
    planner = V.FramePlanner(S.DETECTION_CATEGORIES, S.CLASSIFICATION_CATEGORIES, options)
    assert V.render_frame_host(data, dets, planner) != run['out']['v422.avi'][4]
    lines = lambda d: PV.classified_label_lines(d, planner.label_map, planner.classification_label_map,
                                                options.classification_confidence_threshold)
    assert [lines(d)[0] for d in dets if d['category'] == '1'] == [['animal: 40%']]
    options.classification_confidence_threshold = 0.3
    assert V.render_frame_host(data, dets, planner) == run['out']['v422.avi'][4]
    assert [lines(d) for d in dets if d['category'] == '1'] == [(['animal: 40%', 'red fox: 45.0%'], 3 + 1)]


@pytest.mark.parametrize('classified', [False, True])
def test_plan_is_what_pillow_draws(classified):
    """the plan of every touched frame of the scene, applied by the host model of mdhip_draw_ops, gives Pillow's pixels; the
    too-thin box is the plan's HostLeg"""
    options = V.VideoVisualizationOptions()
    options.classification_confidence_threshold = 0.3
    planner = V.FramePlanner(S.DETECTION_CATEGORIES, S.CLASSIFICATION_CATEGORIES, options)
    entry = S.small_results(classified=classified, thin=True)['images'][0]
    assert entry['file'] == 'v444.avi'
    n = 0
    for w, h in ((64, 48), (70, 50), (320, 240)):
        for i in range(S.N_FRAMES):
            dets = [d for d in entry['detections'] if d['frame_number'] == i and d['conf'] >= 0.15]
            if not dets:
                continue
            if i == 4 and w < 100:                           # (at 320 pixels the box is 17 wide and drawn)
                with pytest.raises(PV.HostLeg):
                    planner.ops(dets, w, h)
                dets = [d for d in dets if d['category'] != '3']
            ops, patches = planner.ops(dets, w, h)
            packed, rows = bytearray(), []
            for op in ops:
                if op[0] == PV.OP_PATCH:
                    data = patches[op[5]]
                    op = op[:5] + [len(packed)] + op[6:]
                    packed += data
                rows.append(op)
            rgb = np.ascontiguousarray(np.full((h, w, 3), 77, dtype=np.uint8))
            assert J.draw_ops(rgb, rows, bytes(packed)) == J.MDJPEG_OK
            image = Image.fromarray(np.full((h, w, 3), 77, dtype=np.uint8))
            planner.draw_with_pil(image, dets)
            assert np.array_equal(rgb, np.asarray(image)), 'frame {} at {} x {}'.format(i, w, h)
            n += 1
    assert n == 12


@pytest.mark.parametrize('blur', [False, True])
def test_keep_source_blocks_on_the_host_leg(tmp_path_factory, blur):
    """the guarantees of tests/test_keep_blocks_cpu.py per frame: an MCU no rectangle touches holds the stored frame's values,
    a touched one Pillow's; and the rectangles cover every pixel the drawing changed"""
    run = host_run(tmp_path_factory, 'keep_blocks', blur, False)
    whole = host_run(tmp_path_factory, 'keep', blur, False)
    planner = V.FramePlanner(S.DETECTION_CATEGORIES, S.CLASSIFICATION_CATEGORIES, run['options'])
    kept_blocks = differing = 0
    for name, args in S.SMALL_VIDEOS.items():
        w, h = args['size']
        s = {'444': 0, '422': 1, '420': 2}[args['sampling']]
        for i in range(S.N_FRAMES):
            data = stored_frame(run['stored'], name, i)
            dets = frame_detections(run['results_file'], name, i)
            got = run['out'][name][i]
            if not dets:
                assert got == data
                continue
            thin = name == 'v444.avi' and i == 4
            if i == args.get('progressive_frame') or thin:
                assert got == whole['out'][name][i]          # no blocks to keep, or a drawing the plan does not restate
                continue
            rects = planner.rectangles(dets, w, h)
            ops, _ = planner.ops(dets, w, h)
            changed = changed_mcus(w, h, s, DR.changed_rectangles(rects, ops))
            assert changed.any()
            image = pillow_pixels(data, dets, blur, False)
            before = np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).astype(int)
            differs = (np.asarray(image).astype(int) != before).any(axis=2)
            mw, mh = 8 * J.SAMPLING_FACTORS[s][0], 8 * J.SAMPLING_FACTORS[s][1]
            pixel_mask = np.repeat(np.repeat(changed, mh, axis=0), mw, axis=1)[:h, :w]
            assert not (differs & ~pixel_mask).any(), 'a changed pixel outside the changed MCUs'
            planes = {}
            for key, blob in (('source', data), ('pillow', pillow_file(image, 'keep')), ('written', got)):
                rc, header, coef = J.decode(blob)
                assert rc == J.MDJPEG_OK
                planes[key] = header.planes(coef)
            for p, mask in enumerate(_block_mask(changed, s)):
                assert np.array_equal(planes['written'][p][~mask], planes['source'][p][~mask]), '{} frame {} plane {}'.format(name, i, p)
                assert np.array_equal(planes['written'][p][mask], planes['pillow'][p][mask]), '{} frame {} plane {}'.format(name, i, p)
                kept_blocks += int((~mask).sum())
            if not changed.all():
                differing += got != whole['out'][name][i]
    assert kept_blocks > 100 and differing >= 3, 'a full re-encode keeps every block here: the test shows nothing'


def test_command_line_reaches_the_options(tmp_path):
    video_dir, results_file, _ = S.build_small(str(tmp_path))
    out_dir = str(tmp_path / 'out')
    argv = [results_file, out_dir, video_dir, '--backend', 'host', '--quality', '75', '--blur_category_names', 'person', '--blur_radius', '6',
            '--rendering_fs', '12', '--trim_to_detections']
    assert quiet(V.main, argv) == 0
    with avi.AviFile(os.path.join(out_dir, 'v444.avi')) as a:
        assert a.n_frames == 5 and a.frame_rate == 12.0
    with pytest.raises(NotImplementedError):
        quiet(V.main, [results_file, out_dir, video_dir, '--backend', 'host', '--fourcc', 'h264'])


def test_a_frame_pillow_refuses_is_that_videos_error_and_leaves_no_file(tmp_path):
    import avi_fixtures as A
    good = A.jpeg_bytes(A.block_noise(64, 48, 1), '420')
    video_dir = tmp_path / 'videos'
    video_dir.mkdir()
    A.write_avi(video_dir / 'bad.avi', [good, b'\xff\xd8 not a JPEG \xff\xd9', good], (64, 48), rate=30)
    A.write_avi(video_dir / 'good.avi', [good, good], (64, 48), rate=30)
    results = {'info': {}, 'detection_categories': S.DETECTION_CATEGORIES, 'images': [
        {'file': 'bad.avi', 'frame_rate': 30.0, 'frames_processed': [0, 1, 2], 'detections': []},
        {'file': 'good.avi', 'frame_rate': 30.0, 'frames_processed': [0, 1, 7], 'detections': []}]}
    results_file = str(tmp_path / 'results.json')
    with open(results_file, 'w') as f:
        json.dump(results, f)
    options = V.VideoVisualizationOptions()
    options.parallelize_rendering = False
    out = quiet(V.visualize_video_output, results_file, str(tmp_path / 'out'), str(video_dir), options, backend='host')
    assert not out[0]['success'] and out[0]['error'].startswith('Error processing video frames: ')
    assert (out[0]['frames_processed'], out[0]['frames_copied'], out[0]['frames_rendered']) == (0, 0, 0)
    assert out[1]['success'] and (out[1]['frames_processed'], out[1]['frames_copied']) == (2, 2)      # frame 7 is not in the file
    assert os.listdir(str(tmp_path / 'out')) == ['good.avi']
