"""
Motion-JPEG AVI files through the device's JPEG decoder (process_video.MJPEGAVIFrameSource(device=True), process_videos(mjpeg=
'gpu')): the first streams the entropy-decode and reconstruction kernels get from something other than a still-image file --
Huffman tables written in by the host (the frames carry none), tiny frames of one shape per batch, no restart markers, scans
from a fraction of one 1024-bit subsequence to several of them.  Every frame must equal Pillow's decode of the stored JPEG
bit for bit, and the JSON of a whole run must equal the host leg's and an in-memory run's byte for byte.  No damaged data is
fed here.  All of these fail on a tree without the feature (no frame source, no mjpeg= argument).
"""

import json
import re

import numpy as np
import pytest

import avi_fixtures as AF

pytestmark = pytest.mark.gpu

# sampling -> (width, height): a height that is no whole MCU, neither dimension a whole MCU, whole MCUs, odd grayscale
SHAPES = {'420': (48, 40), '422': (50, 34), '444': (40, 40), 'gray': (33, 17)}
N_FRAMES = {'420': 7, '422': 9, '444': 6, 'gray': 8}
FLAT_AT = 2
IMAGE_SIZE = 256


def _stored_frames(sampling, progressive_at=None):
    w, h = SHAPES[sampling]
    out = []
    for i in range(N_FRAMES[sampling]):
        arr = AF.flat(w, h) if i == FLAT_AT else AF.block_noise(w, h, seed=100 + i)
        if i == progressive_at:
            out.append(AF.jpeg_bytes(arr, sampling, 90, progressive=True))
        else:
            out.append(AF.strip_dht(AF.jpeg_bytes(arr, sampling, 90)))
    return out


@pytest.fixture(scope='module')
def clips(tmp_path_factory):
    """a folder with one file per sampling; {relative name: (stored chunks, frame rate)}"""
    root = tmp_path_factory.mktemp('mjpeg')
    files = {}
    for k, sampling in enumerate(sorted(SHAPES)):
        stored = _stored_frames(sampling)
        name = 'clip_{}.avi'.format(sampling)
        AF.write_avi(root / name, stored, SHAPES[sampling], rate=10 + k, audio=(k % 2 == 0), rec=(k == 1), idx1=(k != 2))
        files[name] = (stored, float(10 + k))
    return str(root), files


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """the smallest checkpoint file of the GPU tests (test_gpu_parity: the pickle layout of md_v5a.0.0.pt, nano widths)"""
    import fake_yolov5 as FY
    from megadetector_amd import yolo_yaml
    path = str(tmp_path_factory.mktemp('ckpt') / 'md_fake.pt')
    FY.save_checkpoint(FY.build_model(yolo_yaml.YOLOV5N6_TEST, seed=5), path)
    return path


@pytest.fixture(scope='module')
def detectors(checkpoint):
    from megadetector_amd import run_detector
    made = {}

    def get(batch_size):
        if batch_size not in made:
            made[batch_size] = run_detector.load_detector(checkpoint, detector_options={'batch_size': batch_size,
                                                                                        'max_image_size': IMAGE_SIZE})
        return made[batch_size]
    return get


def _counts(det):
    return det.jpeg_images_entropy_decoded, det.jpeg_entropy_fallbacks


@pytest.mark.parametrize('sampling', sorted(SHAPES))
def test_every_frame_equals_pillow(clips, detectors, sampling):
    import torch
    from megadetector_amd import jpeg_host, process_video as PV
    root, files = clips
    name = 'clip_{}.avi'.format(sampling)
    stored = files[name][0]
    det = detectors(4)
    src = PV.MJPEGAVIFrameSource('{}/{}'.format(root, name), device=True)
    assert src.n_frames == len(stored)
    images = [handle.materialise() for handle in src]
    src.close()
    assert all(isinstance(im, jpeg_host.ScanImage) for im in images)
    sizes = [im.nbytes for im in images]
    assert sizes[FLAT_AT] < 128 and max(sizes) > 2 * 128, sizes       # less than one 1024-bit subsequence / several
    assert all(im.desc.n_segments == 1 and im.desc.info.restart_interval == 0 for im in images)
    before = _counts(det)
    decoded = det.decode_scans(images)
    assert _counts(det) == (before[0] + len(stored), before[1])
    assert all(isinstance(im, jpeg_host.DeviceCoefficientImage) for im in decoded)
    torch.cuda.synchronize()
    outs = [torch.empty(int(np.prod(im.shape)), dtype=torch.uint8, device='cuda:0') for im in decoded]
    det._ctx.jpeg_reconstruct(decoded, [im.coef.data_ptr() for im in decoded], [o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    for i, (im, o, chunk) in enumerate(zip(decoded, outs, stored)):
        # the planes are the host decoder's of the frame with its tables written in, the pixels Pillow's of the stored chunk
        want = jpeg_host.decode(jpeg_host.with_standard_tables(chunk))[2]
        np.testing.assert_array_equal(im.coef.tensor().cpu().numpy(), want, err_msg='{} frame {}'.format(name, i))
        np.testing.assert_array_equal(o.cpu().numpy().reshape(im.shape), AF.pil_rgb(chunk), err_msg='{} frame {}'.format(name, i))


def _open_decoded(what):
    from megadetector_amd import process_video as PV
    return PV.ArrayFrameSource([AF.pil_rgb(d) for d in what[0]], frame_rate=what[1])


def _json_text(path):
    return re.sub(r'"detection_completion_time": "[^"]*"', '', open(path).read())


@pytest.mark.parametrize('frame_sample', [1, 2])
@pytest.mark.parametrize('batch_size', [1, 4])
def test_three_legs_write_the_same_json(clips, detectors, checkpoint, tmp_path, batch_size, frame_sample):
    from megadetector_amd import process_video as PV
    root, files = clips
    det = detectors(batch_size)
    kw = dict(frame_sample=frame_sample, batch_size=batch_size, detector=det, image_size=IMAGE_SIZE, json_confidence_threshold=0.001)
    out = {leg: str(tmp_path / '{}.json'.format(leg)) for leg in ('gpu', 'host', 'array')}
    before = _counts(det)
    PV.process_videos(checkpoint, root, out['gpu'], mjpeg='gpu', **kw)
    sampled = sum(len(range(0, len(stored), frame_sample)) for stored, _ in files.values())
    assert _counts(det) == (before[0] + sampled, before[1])
    PV.process_videos(checkpoint, root, out['host'], mjpeg='host', **kw)
    PV.process_videos(checkpoint, 'unused', out['array'], videos=sorted(files.items()), open_source=_open_decoded, **kw)
    assert _counts(det) == (before[0] + sampled, before[1])             # the other two legs decode nothing on the device
    gpu, host, array = (_json_text(out[leg]) for leg in ('gpu', 'host', 'array'))
    assert gpu == host
    assert gpu == array
    j = json.load(open(out['gpu']))
    assert [im['file'] for im in j['images']] == sorted(files)
    for im in j['images']:
        assert 'failure' not in im and im['frame_rate'] == files[im['file']][1]
        assert im['frames_processed'] == list(range(0, len(files[im['file']][0]), frame_sample))
    assert sum(len(im['detections']) for im in j['images']) > 0


def test_progressive_frame_in_a_file_goes_through_pillow(detectors, checkpoint, tmp_path):
    from megadetector_amd import process_video as PV
    stored = _stored_frames('422', progressive_at=4)
    folder = tmp_path / 'v'
    folder.mkdir()
    AF.write_avi(folder / 'mixed.avi', stored, SHAPES['422'], rate=15)
    det = detectors(4)
    kw = dict(batch_size=4, detector=det, image_size=IMAGE_SIZE, json_confidence_threshold=0.001)
    before, rebuilt = _counts(det), det.jpeg_images_reconstructed
    PV.process_videos(checkpoint, str(folder), str(tmp_path / 'gpu.json'), mjpeg='gpu', **kw)
    # all frames but one were Huffman-decoded and rebuilt on the device; the frame mdjpeg_scan refuses arrived as Pillow's
    # pixels and never reached the device's decoder, so it is no fallback of a flagged scan either
    assert _counts(det) == (before[0] + len(stored) - 1, before[1])
    assert det.jpeg_images_reconstructed == rebuilt + len(stored) - 1
    reconstructed = det.jpeg_images_reconstructed
    PV.process_videos(checkpoint, str(folder), str(tmp_path / 'host.json'), mjpeg='host', **kw)
    assert det.jpeg_images_reconstructed == reconstructed
    assert _json_text(str(tmp_path / 'gpu.json')) == _json_text(str(tmp_path / 'host.json'))
    j = json.load(open(tmp_path / 'gpu.json'))
    assert j['images'][0]['frames_processed'] == list(range(len(stored))) and len(j['images'][0]['detections']) > 0
