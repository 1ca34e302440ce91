"""
The JPEG round trip of tiled inference on the device: mdhip_jpeg_recompress (HipContext.jpeg_recompress),
HIPDetector.generate_detections_for_tiles(jpeg_quality=...) and run_tiled_inference(tile_jpeg_quality=...).

The reference for a tile is what the reference's detector reads: the PIL crop after an actual Image.save(quality=q) and
Image.open.  Every comparison is exact: bytes of the recompressed window, bits of the network input, equal result dicts.
"""

import ctypes as C
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

from megadetector_amd import run_tiled_inference as T
from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd.detector import HIPDetector
from megadetector_amd.hip_backend import HipContext
from megadetector_amd.jpeg_host import quant_tables
from test_tile_jpeg_cpu import SIZES, make_content

pytestmark = pytest.mark.gpu

H, W = 1500, 2101                 # pitch 6303 bytes: row starts fall on every alignment
CANARY = 256
_STATE = {}


def _round_trip(rgb, quality):
    bio = io.BytesIO()
    Image.fromarray(rgb).save(bio, format='JPEG', quality=quality)
    return np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert('RGB'))


def _image():
    """noise, with a saturated checkerboard, a smooth gradient, constant fields and a bundled image pasted in"""
    if 'img' not in _STATE:
        img = make_content('noise', W, H, seed=11)
        img[0:400, 0:500] = make_content('checkerboard', 500, 400)
        img[400:1100, 100:1500] = make_content('gradient', 1400, 700)
        img[1100:1300, 0:300] = make_content('white', 300, 200)
        img[1100:1300, 300:600] = make_content('black', 300, 200)
        img[1300:1500, 0:300] = make_content('red', 300, 200)
        img[1300:1500, 300:600] = make_content('green', 300, 200)
        img[1300:1500, 600:900] = make_content('blue', 300, 200)
        img[100:700, 1500:2000] = make_content('crop:anaconda-prompt-base.jpg', 500, 600)
        _STATE['img'] = img
    return _STATE['img']


def _parent():
    """the image in a device allocation of exactly its size"""
    if 'parent' not in _STATE:
        t = torch.empty(H * W * 3, dtype=torch.uint8, device='cuda:0')
        t.copy_(torch.from_numpy(_image().reshape(-1)))
        torch.cuda.synchronize()
        _STATE['parent'] = t
    return _STATE['parent']


def _ctx():
    if 'ctx' not in _STATE:
        Wt = weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1)
        _STATE['ctx'] = HipContext(Wt, dtype='fp16', max_batch=2, max_h=320, max_w=320)
    return _STATE['ctx']


def _windows():
    """(x, y, w, h): every size of the CPU matrix at an odd origin, and each ending in the parent's bottom-right corner"""
    out = []
    for i, (w, h) in enumerate(SIZES):
        out.append((2 * i + 1, 2 * (i % 5) + 3, w, h))
        out.append((W - w, H - h, w, h))
    out.append((401, 1001, 333, 257))
    return out


@pytest.mark.parametrize('quality', [95, 75, 30, 100])
def test_recompressed_windows_equal_pillow_round_trip(quality):
    img, parent, ctx = _image(), _parent(), _ctx()
    wins = _windows()
    assert all(x + w <= W and y + h <= H for x, y, w, h in wins)
    assert any(x + w == W and y + h == H for x, y, w, h in wins) and any(x % 2 == 1 and y % 2 == 1 for x, y, _, _ in wins)
    pitch = W * 3
    offs, cur = [], CANARY
    for x, y, w, h in wins:
        offs.append(cur)
        cur += h * w * 3 + CANARY
    out = torch.full((cur,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    for s in range(0, len(wins), 7):                      # several windows of different sizes per call
        part = list(range(s, min(s + 7, len(wins))))
        ctx.jpeg_recompress([parent.data_ptr() + wins[i][1] * pitch + wins[i][0] * 3 for i in part],
                            [(wins[i][2], wins[i][3]) for i in part], [pitch] * len(part), quality,
                            [out.data_ptr() + offs[i] for i in part])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.array_equal(parent.cpu().numpy(), img.reshape(-1)), 'the parent image was written to'
    mask = np.ones(cur, dtype=bool)
    for (x, y, w, h), o in zip(wins, offs):
        mask[o:o + h * w * 3] = False
        got = host[o:o + h * w * 3].reshape(h, w, 3)
        want = _round_trip(np.ascontiguousarray(img[y:y + h, x:x + w]), quality)
        assert np.array_equal(got, want), 'window {} at quality {}: {} bytes differ'.format(
            (x, y, w, h), quality, int((got != want).sum()))
    assert (host[mask] == 0xA5).all(), 'canary bytes around the outputs were overwritten'


def test_host_pointers_and_bad_arguments_are_refused():
    ctx, parent = _ctx(), _parent()
    host = np.ascontiguousarray(_image()[:64, :64])
    out = torch.empty(64 * 64 * 3, dtype=torch.uint8, device='cuda:0')
    ql, qc = quant_tables(95)
    u16 = C.POINTER(C.c_uint16)

    def call(win, outp, w=64, h=64, pitch=W * 3, luma=ql):
        return ctx.lib.mdhip_jpeg_recompress(ctx.h, C.cast((C.c_void_p * 1)(win), C.POINTER(C.c_void_p)), (C.c_int32 * 1)(w),
                                             (C.c_int32 * 1)(h), (C.c_int64 * 1)(pitch), 1, luma.ctypes.data_as(u16),
                                             qc.ctypes.data_as(u16), C.cast((C.c_void_p * 1)(outp), C.POINTER(C.c_void_p)), None)

    assert call(host.ctypes.data, out.data_ptr(), pitch=64 * 3) == -1                   # MDHIP_EINVAL
    assert 'host pointer' in ctx.lib.mdhip_last_error(ctx.h).decode()
    assert call(parent.data_ptr(), host.ctypes.data) == -1
    assert 'host pointer' in ctx.lib.mdhip_last_error(ctx.h).decode()
    assert call(parent.data_ptr(), out.data_ptr(), w=0) == -1
    assert call(parent.data_ptr(), out.data_ptr(), pitch=64 * 3 - 1) == -1
    assert call(parent.data_ptr(), out.data_ptr(), luma=np.zeros(64, np.uint16)) == -1
    assert call(parent.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='1 to 100'):
        ctx.jpeg_recompress([parent.data_ptr()], [(64, 64)], [W * 3], 0, [out.data_ptr()])


# ---------------------------------------------------------------------------------------------------------------------
def _detector(yaml_name, seed, batch, size=640):
    key = ('det', yaml_name, seed, batch, size)
    if key not in _STATE:
        Wt = weights_io.synthetic_weights(getattr(yolo_yaml, yaml_name), seed=seed)
        d = HIPDetector(Wt, {'batch_size': batch, 'max_image_size': size, 'device': 'cuda:0'})
        d.default_image_size = size
        _STATE[key] = d
    return _STATE[key]


def _origins(img, tile, n_tiles):
    tw, th = tile
    rng = np.random.default_rng(3)
    origins = [(int(rng.integers(0, img.shape[1] - tw)), int(rng.integers(0, img.shape[0] - th))) for _ in range(n_tiles - 1)]
    origins.append((img.shape[1] - tw, img.shape[0] - th))
    return origins


def _last_input(det, tile, n):
    """the network input the last chunk of a call left in the context (n = tiles in that chunk)"""
    h, w = det.preprocess_image(np.zeros((tile[1], tile[0], 3), np.uint8))['img_processed'].shape[:2]
    return det._ctx.read_input(n, h, w).view(np.uint32)


def _tiles_vs_files(det, tile, n_tiles, augment=False, quality=95):
    img = _image()
    tw, th = tile
    origins = _origins(img, tile, n_tiles)
    ids = ['t{}'.format(i) for i in range(len(origins))]
    last = (n_tiles - 1) % det.max_batch + 1
    got = det.generate_detections_for_tiles(img, origins, tile, tile_ids=ids, detection_threshold=1e-5, augment=augment,
                                            jpeg_quality=quality)
    got_in = _last_input(det, tile, last)
    files = [_round_trip(np.ascontiguousarray(img[y:y + th, x:x + tw]), quality) for x, y in origins]
    want = det.generate_detections_one_batch(files, ids, detection_threshold=1e-5, augment=augment)
    want_in = _last_input(det, tile, last)
    assert all(r.get('failure') is None for r in want), want
    assert sum(len(r['detections']) for r in want) > 0
    assert got_in.shape == want_in.shape and np.array_equal(got_in, want_in), \
        '{} values of the network input differ'.format(int((got_in != want_in).sum()))
    assert got == want
    return origins, ids, got, got_in


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('n_tiles', [3, 9])            # below max_batch; above it and not a multiple of it
def test_yolov5x6_tiles_equal_tile_files(augment, n_tiles):
    _tiles_vs_files(_detector('YOLOV5X6_MD', 0, 4), (640, 640), n_tiles, augment=augment)


@pytest.mark.parametrize('yaml_name', ['YOLO11N_TEST', 'YOLOV9_DUAL_TEST'])
def test_anchor_free_models_tiles_equal_tile_files(yaml_name):
    _tiles_vs_files(_detector(yaml_name, 0, 4), (640, 480), 6)
    _tiles_vs_files(_detector(yaml_name, 0, 4), (500, 700), 5)


def test_switch_off_is_the_call_without_the_argument():
    det = _detector('YOLO11N_TEST', 0, 4)
    img, tile = _image(), (640, 480)
    origins = _origins(img, tile, 3)
    a = det.generate_detections_for_tiles(img, origins, tile, detection_threshold=1e-5)
    a_in = _last_input(det, tile, 3)
    # (a recompressed call in between: the switch leaves nothing behind)
    c = det.generate_detections_for_tiles(img, origins, tile, detection_threshold=1e-5, jpeg_quality=30)
    c_in = _last_input(det, tile, 3)
    b = det.generate_detections_for_tiles(img, origins, tile, detection_threshold=1e-5, jpeg_quality=None)
    b_in = _last_input(det, tile, 3)
    assert np.array_equal(a_in, b_in) and a == b
    assert not np.array_equal(a_in, c_in), 'quality 30 must change the pixels'
    with pytest.raises(ValueError, match='1 to 100'):
        det.generate_detections_for_tiles(img, origins, tile, jpeg_quality=101)


def test_run_tiled_inference_equals_a_run_on_tile_files(tmp_path):
    """the reference's way, built here: write every tile with PIL at quality 95, detect on the decoded files, merge, NMS"""
    det = _detector('YOLOV5X6_MD', 0, 4)
    folder = tmp_path / 'imgs'
    folder.mkdir()
    img = np.ascontiguousarray(_image()[:1100, :1500])
    Image.fromarray(img).save(str(folder / 'big.png'))
    tile, overlap = (640, 640), 0.5
    out = str(tmp_path / 'out.json')
    res = T.run_tiled_inference('md_v5a.0.0.pt', str(folder), None, out, tile_size_x=tile[0], tile_size_y=tile[1],
                                tile_overlap=overlap, detector=det, tile_jpeg_quality=95, loader_workers=0)
    with open(out) as f:
        assert json.load(f)['images'] == res['images']
    origins = T.get_patch_boundaries((1500, 1100), tile, (320, 320))
    xs, ys = sorted({x for x, _ in origins}), sorted({y for _, y in origins})
    assert len(xs) >= 3 and len(ys) >= 3 and xs[-1] - xs[-2] != 320 and ys[-1] - ys[-2] != 320      # flush-moved last tiles
    tiles_dir = tmp_path / 'tiles'
    tiles_dir.mkdir()
    patches, names = [], []
    for x, y in origins:
        fn = str(tiles_dir / (T.patch_info_to_patch_name('big.png', x, y) + '.jpg'))
        Image.fromarray(img).crop((x, y, x + tile[0], y + tile[1])).save(fn, quality=95)
        names.append(fn)
        patches.append({'xmin': x, 'xmax': x + tile[0] - 1, 'ymin': y, 'ymax': y + tile[1] - 1})
    decoded = [np.asarray(Image.open(fn).convert('RGB')) for fn in names]
    tile_results = []
    for s in range(0, len(names), det.max_batch):
        tile_results += det.generate_detections_one_batch(decoded[s:s + det.max_batch], names[s:s + det.max_batch])
    assert all(r.get('failure') is None for r in tile_results)
    assert sum(len(r['detections']) for r in tile_results) > 0
    for r in tile_results:
        r['detections'] = sorted([d for d in r['detections'] if d['conf'] >= 0.005], key=lambda d: -d['conf'])
    print('tile-level detections at the output threshold: {}'.format(sum(len(r['detections']) for r in tile_results)))
    want = {'images': [T.merge_tile_results('big.png', (1500, 1100), patches, tile_results, list(tile))]}
    T.in_place_nms(want, verbose=False)
    assert res['images'] == want['images']
