"""
Motion-JPEG AVI files on the video path, host side: the container reader (megadetector_amd/avi.py) against files the tests'
own writer muxes (avi_fixtures.py), abbreviated JPEG streams (jpeg_host.with_standard_tables: frames without DHT segments)
against Pillow's decode of the same bytes, and the frame source / driver / command line with the stub detector.  Every test
here fails on a tree without the feature (no avi module, no with_standard_tables, no mjpeg= argument, no main()).
"""

import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import avi_fixtures as AF
import jpeg_fixtures as JF
from megadetector_amd import process_video as PV
from test_batch_loop import StubDetector, PipelinedStub

SIZE = (50, 34)


@pytest.fixture(scope='module')
def J():
    return JF.ensure_libmdjpeg()


@pytest.fixture(scope='module')
def frames():
    """nine 4:2:2 frames of odd byte lengths and even ones, as Pillow wrote them (tables included)"""
    out = [AF.jpeg_bytes(AF.block_noise(SIZE[0], SIZE[1], seed=i), '422', 90) for i in range(9)]
    assert any(len(f) & 1 for f in out) and any(not len(f) & 1 for f in out)
    return out


# ---- the container ----------------------------------------------------------------------------------------------------
CONTAINERS = {
    'plain': dict(),
    'no_idx1': dict(idx1=False),
    'audio': dict(audio=True),
    'audio_is_stream_0': dict(audio=True, audio_first=True),
    'junk': dict(junk=True),
    'rec_lists': dict(rec=True, audio=True),
    'avix': dict(avix_from=5, junk=True),
    'avix_rec_no_idx1': dict(avix_from=2, rec=True, idx1=False),
    'ntsc_rate': dict(rate=30000, scale=1001),
    'rate_from_main_header': dict(rate=25, scale=0, usec=40000),
    'lower_case_fourcc': dict(fourcc=b'mjpg'),
}


@pytest.mark.parametrize('name', sorted(CONTAINERS))
def test_reader_returns_what_the_writer_put_in(tmp_path, frames, name):
    from megadetector_amd import avi
    kw = CONTAINERS[name]
    path = AF.write_avi(tmp_path / 'a.avi', frames, SIZE, **kw)
    with avi.AviFile(path) as a:
        assert a.n_frames == len(frames)
        want = 25.0 if name == 'rate_from_main_header' else kw.get('rate', 30) / kw.get('scale', 1)
        assert a.frame_rate == want
        assert (a.width, a.height) == SIZE
        for i in (4, 0, 8, 1, 2, 3, 5, 6, 7):                 # any order
            assert a.read_frame(i) == frames[i], i
        with pytest.raises(IndexError):
            a.read_frame(len(frames))


def test_cut_off_file_and_dropped_frame(tmp_path, frames):
    from megadetector_amd import avi
    whole = AF.avi_bytes(frames, SIZE, idx1=False)
    # cut in the middle of the last chunk (its header is still there): one frame fewer
    cut = whole[:len(whole) - len(frames[-1]) // 2 - 1]
    p = tmp_path / 'cut.avi'
    p.write_bytes(cut)
    with avi.AviFile(str(p)) as a:
        assert a.n_frames == len(frames) - 1
        assert [a.read_frame(i) for i in range(a.n_frames)] == frames[:-1]
    # ... also when the cut is in an AVIX segment and when an index would have followed
    seg = AF.avi_bytes(frames, SIZE, avix_from=4)
    p.write_bytes(seg[:len(seg) - 10])
    with avi.AviFile(str(p)) as a:
        assert a.n_frames == len(frames) - 1 and a.read_frame(7) == frames[7]
    # a zero-length chunk in the middle: the frame keeps its number and repeats the one before it
    dropped = list(frames)
    dropped[3] = b''
    dropped[4] = b''
    with avi.AviFile(AF.write_avi(tmp_path / 'drop.avi', dropped, SIZE, audio=True)) as a:
        assert a.n_frames == len(frames)
        assert [a.read_frame(i) for i in range(9)] == frames[:3] + [frames[2], frames[2]] + frames[5:]
    with pytest.raises(avi.AviError, match='first video chunk is empty') as e:
        avi.AviFile(AF.write_avi(tmp_path / 'drop0.avi', [b''] + frames[:2], SIZE))
    assert e.value.mjpeg


def test_what_is_not_an_mjpeg_avi_is_refused(tmp_path, frames):
    from megadetector_amd import avi
    cases = {
        'h264.avi': (AF.avi_bytes(frames[:2], SIZE, fourcc=b'H264'), 'not MJPG'),
        'wave.avi': (AF.riff_list(b'WAVE', AF.chunk(b'fmt ', b'\x00' * 16), tag=b'RIFF'), 'not an AVI'),
        'audio_only.avi': (AF.avi_bytes(frames[:2], SIZE, video=False), 'no video stream'),
        'zero.avi': (b'0', 'not a RIFF'),
        'jpeg.avi': (frames[0], 'not a RIFF'),
        'no_rate.avi': (AF.avi_bytes(frames[:2], SIZE, rate=0, scale=0, usec=0), 'frame rate'),
    }
    for name, (data, why) in cases.items():
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(avi.AviError, match=why) as e:
            avi.AviFile(str(p))
        assert e.value.mjpeg == (name == 'no_rate.avi'), name
    assert issubclass(avi.AviError, Exception)


# ---- abbreviated streams ------------------------------------------------------------------------------------------------
SHAPES = {'444': (40, 40), '422': (50, 34), '420': (48, 40), 'gray': (33, 17)}


@pytest.mark.parametrize('sampling', sorted(SHAPES))
def test_frames_without_huffman_tables(J, sampling):
    w, h = SHAPES[sampling]
    full = AF.jpeg_bytes(AF.block_noise(w, h, seed=3), sampling, 90)
    raw = AF.strip_dht(full)
    assert b'\xff\xc4' not in raw[:raw.index(b'\xff\xda')] and len(raw) < len(full)
    # the gap: the project's decoder refuses the frame as it is stored
    assert J.scan(raw)[0] == J.MDJPEG_EUNSUPPORTED and J.decode(raw)[0] == J.MDJPEG_EUNSUPPORTED
    assert 'Huffman table' in J.parse(raw).reason
    fixed = J.with_standard_tables(raw)
    assert isinstance(fixed, bytes) and fixed is not raw
    assert fixed.count(b'\xff\xc4') == 1 and fixed.index(b'\xff\xc4') < fixed.index(b'\xff\xda')
    assert J.with_standard_tables(full) is full and J.with_standard_tables(fixed) is fixed
    as_array = np.frombuffer(raw, np.uint8)
    assert J.with_standard_tables(as_array) == fixed
    rc, sc, _ = J.scan(fixed)
    assert rc == 0 and sc.n_segments == 1
    rc0, h0, want = J.decode(full)
    rc1, h1, got = J.decode(fixed)
    assert rc0 == 0 and rc1 == 0 and h1.coef_count == h0.coef_count
    np.testing.assert_array_equal(got, want)
    for bits in (64, 1024):
        rc2, _, sub = J.decode_subsequences(fixed, bits)
        assert rc2 == 0
        np.testing.assert_array_equal(sub, want)
    from megadetector_amd.feed import load_image
    np.testing.assert_array_equal(np.asarray(load_image(io.BytesIO(fixed))), AF.pil_rgb(raw))
    np.testing.assert_array_equal(AF.pil_rgb(raw), AF.pil_rgb(full))


@pytest.mark.parametrize('sampling', ['422', 'gray'])
@pytest.mark.parametrize('drop', [{0x01, 0x11}, {0x10, 0x11}, {0x00, 0x01}, {0x00, 0x10}, {0x11}],
                         ids=['chroma', 'ac', 'dc', 'luma', 'chroma_ac'])
def test_partly_missing_tables_follow_pillow(J, sampling, drop):
    """Pillow (libjpeg) fills each of DC 0, AC 0, DC 1, AC 1 that a file does not define, one by one: it decodes every one
    of these to the pixels of the complete file, and so must the rewritten bytes"""
    w, h = SHAPES[sampling]
    full = AF.jpeg_bytes(AF.block_noise(w, h, seed=5), sampling, 90)
    raw = AF.strip_dht(full, drop)
    want = AF.pil_rgb(full)
    np.testing.assert_array_equal(AF.pil_rgb(raw), want)               # what Pillow does with the stored bytes
    fixed = J.with_standard_tables(raw)
    if sampling == 'gray' and not drop & {0x00, 0x10}:
        assert fixed is raw                                              # the scan names no chrominance table
    else:
        assert fixed is not raw and J.scan(raw)[0] != 0
    assert J.scan(fixed)[0] == 0
    np.testing.assert_array_equal(J.decode(fixed)[2], J.decode(full)[2])
    np.testing.assert_array_equal(AF.pil_rgb(fixed), want)


def test_tables_2_and_3_stay_refused_and_table_1_is_the_chrominance_pair(J):
    from PIL import Image
    w, h = SHAPES['gray']
    full = AF.jpeg_bytes(AF.block_noise(w, h, seed=6), 'gray', 90)
    for table_id in (2, 3):
        moved = AF.renumber_tables(full, table_id)
        np.testing.assert_array_equal(AF.pil_rgb(moved), AF.pil_rgb(full))     # a legal file while it has its tables
        raw = AF.strip_dht(moved)
        with pytest.raises(Exception):                                           # Pillow refuses it ...
            Image.open(io.BytesIO(raw)).load()
        assert J.with_standard_tables(raw) is raw and J.scan(raw)[0] != 0        # ... and so does everything here
    # a scan that names table 1 and leaves it implied gets the standard's CHROMINANCE pair, as in Pillow (this file was coded
    # with the luminance pair, so the pixels are not the original's: both sides make the same ones of it)
    raw = AF.strip_dht(AF.renumber_tables(full, 1))
    fixed = J.with_standard_tables(raw)
    assert fixed is not raw and fixed[fixed.index(b'\xff\xc4') + 4] == 0x01
    np.testing.assert_array_equal(AF.pil_rgb(fixed), AF.pil_rgb(raw))
    # bytes that are no JPEG, or end before a scan header, come back as they are
    for junk in (b'', b'0', b'\xff\xd8', b'\xff\xd8\xff\xe0\x00\x10JFIF', full[:full.index(b'\xff\xda')]):
        assert J.with_standard_tables(junk) is junk


# ---- frame source and driver -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clip(tmp_path_factory, frames):
    """a file of abbreviated frames with one dropped frame, and the frames Pillow decodes from what read_frame returns"""
    stored = [AF.strip_dht(f) for f in frames]
    stored[6] = b''
    path = AF.write_avi(tmp_path_factory.mktemp('clip') / 'clip.avi', stored, SIZE, rate=10, audio=True)
    shown = stored[:6] + [stored[5]] + stored[7:]
    return path, [AF.pil_rgb(d) for d in shown]


def _plain(results):
    return json.loads(json.dumps(results))


@pytest.mark.parametrize('kw', [dict(every_n_frames=1), dict(every_n_frames=3), dict(every_n_frames=-0.2), dict(every_n_frames=-0.45),
                                dict(frames_to_process=[1, 4, 6]), dict(frames_to_process=7)],
                         ids=['every', 'third', 'seconds_0.2', 'seconds_0.45', 'list', 'one'])
@pytest.mark.parametrize('batch_size,det_cls', [(1, StubDetector), (3, PipelinedStub), (8, PipelinedStub), (3, StubDetector)])
def test_source_equals_array_source(clip, kw, batch_size, det_cls):
    path, rgb = clip
    want = PV.run_detector_on_frames(det_cls(), PV.ArrayFrameSource(rgb, frame_rate=10.0), batch_size=batch_size,
                                     detection_threshold=0.0, **kw)
    src = PV.MJPEGAVIFrameSource(path, device=False)
    assert src.n_frames == 9 and src.frame_rate == 10.0 and src.frames_read == 0
    got = PV.run_detector_on_frames(det_cls(), src, batch_size=batch_size, detection_threshold=0.0, **kw)
    assert _plain(got) == _plain(want)
    assert len(got['results']) > 0 and all(r['detections'] for r in got['results'])
    assert src.frames_read == len(got['frame_filenames'])               # only the sampled chunks were read
    src.close()
    assert src.avi._f.closed


def test_device_leg_materialises_scan_images_without_a_device(clip, tmp_path, frames):
    """what the device leg hands the detector: ScanImage for a baseline frame (whose host-model decode gives the complete
    file's coefficients), Pillow's array for a progressive one, ScanFailure for bytes Pillow refuses too"""
    from megadetector_amd import jpeg_host as J
    prog = AF.jpeg_bytes(AF.block_noise(SIZE[0], SIZE[1], seed=40), '422', 90, progressive=True)
    stored = [AF.strip_dht(frames[0]), prog, b'\xff\xd8 not a frame', AF.strip_dht(frames[3])]
    src = PV.MJPEGAVIFrameSource(AF.write_avi(tmp_path / 'mixed.avi', stored, SIZE), device=True)
    got = [h.materialise() for h in src]
    assert src.frames_read == 4
    assert isinstance(got[0], J.ScanImage) and isinstance(got[3], J.ScanImage) and got[0].shape == (SIZE[1], SIZE[0], 3)
    np.testing.assert_array_equal(J.decode(got[0].file)[2], J.decode(frames[0])[2])
    assert isinstance(got[1], np.ndarray)
    np.testing.assert_array_equal(got[1], AF.pil_rgb(prog))
    assert isinstance(got[2], J.ScanFailure)
    src.close()
    # the host leg gives the same failure record for that frame through the driver, and the video goes on
    host = PV.MJPEGAVIFrameSource(src.avi.path, device=False)
    r = PV.run_detector_on_frames(PipelinedStub(), host, batch_size=3)
    assert [('failure' in x) for x in r['results']] == [False, False, True, False]
    host.close()


def _strip_time(path):
    return re.sub(r'"detection_completion_time": "[^"]*"', '', open(path).read())


@pytest.fixture(scope='module')
def folder(tmp_path_factory, frames):
    root = tmp_path_factory.mktemp('videos')
    (root / 'cam1').mkdir()
    a = [AF.strip_dht(f) for f in frames]
    b = [AF.jpeg_bytes(AF.block_noise(48, 40, seed=20 + i), '420', 90) for i in range(5)]
    AF.write_avi(root / 'a.avi', a, SIZE, rate=10, rec=True)
    AF.write_avi(root / 'cam1' / 'b.avi', b, (48, 40), rate=25, avix_from=3, idx1=False)
    AF.write_avi(root / 'cam1' / 'other_codec.avi', a[:2], SIZE, fourcc=b'XVID')
    (root / 'clip.mp4').write_bytes(b'\x00\x00\x00\x18ftypmp42' + b'\x00' * 64)
    return str(root), {'a.avi': (a, 10.0), 'cam1/b.avi': (b, 25.0)}


def _open_decoded(what):
    if what is None:
        raise RuntimeError('decoding video files needs opencv-python (cv2)')
    return PV.ArrayFrameSource([AF.pil_rgb(d) for d in what[0]], frame_rate=what[1])


def test_process_videos_over_a_folder(folder, tmp_path):
    try:
        import cv2  # noqa: F401
        pytest.skip('cv2 is installed here: the other two files may decode')
    except ImportError:
        pass
    root, good = folder
    names = ['a.avi', 'cam1/b.avi', 'cam1/other_codec.avi', 'clip.mp4']
    out = str(tmp_path / 'host.json')
    images = PV.process_videos('md_v5a.0.0.pt', root, out, frame_sample=2, batch_size=3, detector=PipelinedStub(),
                               json_confidence_threshold=0.0, mjpeg='host')
    j = json.load(open(out))
    assert [im['file'] for im in j['images']] == names and j['info']['format_version'] == '1.6'
    assert set(j['info']) >= {'detector', 'detection_completion_time', 'format_version'}
    assert set(j['detection_categories']) == {'1', '2', '3'}
    # the two AVIs: what the in-memory source gives for Pillow's decode of every stored frame
    want = PV.process_videos('md_v5a.0.0.pt', 'unused', str(tmp_path / 'want.json'), frame_sample=2, batch_size=3,
                             detector=PipelinedStub(), json_confidence_threshold=0.0, open_source=_open_decoded,
                             videos=[(n, good.get(n)) for n in names])
    assert _plain(images[:2]) == _plain(want[:2])
    assert images[0]['frames_processed'] == [0, 2, 4, 6, 8] and images[0]['frame_rate'] == 10.0
    assert images[1]['frames_processed'] == [0, 2, 4] and images[1]['frame_rate'] == 25.0
    assert len(images[0]['detections']) > 0 and all('frame_number' in d for d in images[0]['detections'])
    for im in j['images'][2:]:
        assert im['detections'] is None and 'opencv' in im['failure'] and im['frame_rate'] == -1.0
    # 'off': nothing changes -- without cv2 no file of the folder opens, as before
    off = PV.process_videos('md_v5a.0.0.pt', root, str(tmp_path / 'off.json'), frame_sample=2, batch_size=3,
                            detector=PipelinedStub(), json_confidence_threshold=0.0)
    assert [im['file'] for im in off] == names
    assert all(im['detections'] is None and 'opencv' in im['failure'] for im in off)
    # one file instead of a folder; time_sample; the arguments that cannot be combined
    one = PV.process_videos('md_v5a.0.0.pt', os.path.join(root, 'a.avi'), str(tmp_path / 'one.json'), time_sample=0.2,
                            batch_size=8, detector=StubDetector(), mjpeg='host')
    assert [im['file'] for im in one] == ['a.avi'] and one[0]['frames_processed'] == [0, 2, 4, 6, 8]
    with pytest.raises(ValueError, match='mjpeg'):
        PV.process_videos('m', root, out, detector=StubDetector(), mjpeg='yes')
    with pytest.raises(ValueError, match='open_source'):
        PV.process_videos('m', root, out, detector=StubDetector(), mjpeg='host', open_source=_open_decoded)
    with pytest.raises(ValueError, match='decode_scans'):
        PV.process_videos('m', root, out, detector=StubDetector(), mjpeg='gpu')


def _stub_worker(gpu, model_file, videos, opts, run_kwargs, n_gpus, out_q):
    try:
        out_q.put((gpu, PV.run_detector_on_videos(PipelinedStub(), videos, **run_kwargs), None))
    except Exception as e:
        out_q.put((gpu, None, repr(e)))


def test_two_shard_processes_equal_one_process(folder, tmp_path):
    """the opener travels to spawned processes (it is pickled): the merged JSON is the one-process JSON"""
    import pickle
    import functools
    opener = functools.partial(PV.open_video_source, mjpeg='host')
    assert pickle.loads(pickle.dumps(opener)).keywords == {'mjpeg': 'host'}
    root, _ = folder
    one, two = str(tmp_path / 'one.json'), str(tmp_path / 'two.json')
    kw = dict(frame_sample=3, batch_size=4, json_confidence_threshold=0.0, mjpeg='host')
    im1 = PV.process_videos('md_v5a.0.0.pt', root, one, detector=PipelinedStub(), **kw)
    im2 = PV.process_videos('md_v5a.0.0.pt', root, two, n_gpus=2, shard_worker=_stub_worker, **kw)
    assert _plain(im1) == _plain(im2) and _strip_time(one) == _strip_time(two)
    assert sum(1 for im in im2 if im['detections']) == 2


def test_command_line(folder, tmp_path, capsys):
    root, _ = folder
    out = str(tmp_path / 'cli.json')
    rc = PV.main(['md_v5a.0.0.pt', root, '--recursive', '--output_json_file', out, '--frame_sample', '2', '--batch_size', '3',
                  '--json_confidence_threshold', '0.0', '--mjpeg', 'host', '--detector_options', 'dtype=fp16', '--verbose'],
                 detector=PipelinedStub())
    assert rc == 0
    want = str(tmp_path / 'api.json')
    PV.process_videos('md_v5a.0.0.pt', root, want, frame_sample=2, batch_size=3, detector=PipelinedStub(),
                      json_confidence_threshold=0.0, mjpeg='host')
    assert _strip_time(out) == _strip_time(want)
    # without --recursive the sub-folder is not searched
    PV.main(['md_v5a.0.0.pt', root, '--output_json_file', out, '--time_sample', '0.2', '--mjpeg', 'host'], detector=StubDetector())
    assert [im['file'] for im in json.load(open(out))['images']] == ['a.avi', 'clip.mp4']
    for bad in (['m', root, '--frame_sample', '2', '--time_sample', '1'], ['m', root, '--mjpeg', 'maybe'], ['m', root, '--augment'],
                ['m', str(tmp_path / 'missing')]):
        with pytest.raises(SystemExit):
            PV.main(bad, detector=StubDetector())
    capsys.readouterr()
    # the module runs as a program
    from conftest import REPO
    r = subprocess.run([sys.executable, '-m', 'megadetector_amd.process_video', '--help'], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0 and '--mjpeg' in r.stdout and '--n_gpus' in r.stdout and '--augment' not in r.stdout
