"""
The RDE review folder on the device: mdhip_thumbnails against Pillow bit for bit in ONE call (every byte around the tiles
unchanged), its refusals, the context without a model (mdhip_create_images), and write_review_folder with backend='gpu'
against backend='host' file by file, with the counts that say every file was decoded once.
"""

import copy
import datetime
import json
import os

import numpy as np
import pytest
import torch

import rde_review_scene as S
import thumbnail_cases as T
from megadetector_amd import rde_review as RV
from megadetector_amd import repeat_detections as RD
from megadetector_amd._lib import HipError
from megadetector_amd.hip_backend import HipContext
from test_rde_review_cpu import NOW, rde_options, review_options

pytestmark = pytest.mark.gpu

_STATE = {}


def _images_ctx():
    if 'ctx' not in _STATE:
        _STATE['ctx'] = HipContext.for_images(0)
    return _STATE['ctx']


def _model_ctx():
    from test_gpu_tile_jpeg import _ctx
    return _ctx()


def _matrix():
    """the matrix, its placement, the sheets and Pillow's result: computed once and never changed"""
    if 'matrix' not in _STATE:
        matrix = T.cases()
        where, heights = T.place([size for _, _, size in matrix])
        sheets = T.Sheets(heights)
        _STATE['matrix'] = (matrix, where, sheets, T.expected(matrix, where, sheets))
    return _STATE['matrix']


def _run_matrix(ctx):
    matrix, where, sheets, want = _matrix()
    device = [torch.from_numpy(b.copy()).to('cuda:0') for b in sheets.backing]
    sources, tiles = {}, []
    for (pixels, box, size), (s, x, y) in zip(matrix, where):
        if id(pixels) not in sources:
            # at an odd address too: one byte of lead
            sources[id(pixels)] = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), pixels.reshape(-1)])).to('cuda:0')
        h, w = pixels.shape[:2]
        (sx, sy, sw, sh), (cw, ch, ox, oy) = T.canvas_of(box, w, h)
        src = sources[id(pixels)].data_ptr() + 1 + (sy * w + sx) * 3 if sw else 0
        tiles.append((src, w * 3, sw, sh, cw, ch, ox, oy, size[0], size[1],
                      device[s].data_ptr() + T.GUARD + y * sheets.pitches[s] + x * 3, sheets.pitches[s]))
    assert ctx.thumbnails(tiles) is True                              # ONE call
    torch.cuda.synchronize()
    for s in range(3):
        got = device[s].cpu().numpy()
        bad = np.flatnonzero(got != want[s])
        assert bad.size == 0, 'sheet {}: {} bytes differ, the first at {}'.format(s, bad.size, bad[:5])
    for (pixels, _, _) in matrix[:14]:
        assert np.array_equal(sources[id(pixels)].cpu().numpy()[1:], pixels.reshape(-1))


def test_kernel_matrix_in_one_call():
    _run_matrix(_model_ctx())


def test_refusals_write_nothing():
    ctx = _model_ctx()
    src = torch.arange(0, 8 * 8 * 3, dtype=torch.int32, device='cuda:0').to(torch.uint8)
    dst = torch.full((64,), 7, dtype=torch.uint8, device='cuda:0')
    host = np.zeros(8 * 8 * 3, np.uint8)
    good = (src.data_ptr(), 24, 8, 8, 8, 8, 0, 0, 4, 4, dst.data_ptr(), 12)
    for bad in ((host.ctypes.data, 24, 8, 8, 8, 8, 0, 0, 4, 4, dst.data_ptr(), 12),           # host pixels
                (src.data_ptr(), 24, 8, 8, 8, 8, 0, 0, 4, 4, host.ctypes.data, 12),           # a host destination
                (src.data_ptr(), 24, 8, 8, 10, 8, 3, 0, 4, 4, dst.data_ptr(), 12),            # the rectangle leaves its canvas
                (src.data_ptr(), 24, 8, 8, 8, 8, 0, 0, 0, 4, dst.data_ptr(), 12),             # a size of 0
                (src.data_ptr(), 24, 8, 8, 8, 70000, 0, 0, 4, 4, dst.data_ptr(), 12)):        # a canvas above 65535
        with pytest.raises(HipError, match=r'\(-1\)'):
            ctx.thumbnails([good, bad])
    with pytest.raises(HipError, match=r'\(-1\)'):
        ctx.thumbnails([good], filter=3)
    # a canvas of height 60000 around 8 rows, reduced to one output row: MDHIP_EUNSUPPORTED (the canvas is virtual)
    assert ctx.thumbnails([good, (src.data_ptr(), 24, 8, 8, 8, 60000, 0, 100, 4, 1, dst.data_ptr() + 48, 12)]) is False
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == 7).all()
    assert ctx.thumbnails([good]) is True
    torch.cuda.synchronize()
    assert (dst.cpu().numpy()[:48] != 7).any() and (dst.cpu().numpy()[48:] == 7).all()


def test_context_without_a_model():
    from megadetector_amd import jpeg_host as J
    from PIL import Image
    import io
    ctx = _images_ctx()
    _run_matrix(ctx)
    # a JPEG decode on it: entropy decode and reconstruction against PIL
    rng = np.random.default_rng(1)
    bio = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).resize((160, 120)).save(bio, format='JPEG', quality=85)
    data = bio.getvalue()
    rc, scan, _ = J.ScanImage.from_bytes(data, 0)
    assert rc == J.MDJPEG_OK
    compressed = torch.from_numpy(np.frombuffer(bytes(scan.scan_bytes) + bytes(512), np.uint8).copy()).to('cuda:0')
    coefs = torch.empty(scan.coef_count + 128, dtype=torch.int16, device='cuda:0')
    out = torch.empty(120 * 160 * 3, dtype=torch.uint8, device='cuda:0')
    assert ctx.jpeg_entropy_decode([scan], [compressed.data_ptr()], [coefs.data_ptr()]).tolist() == [0]
    ctx.jpeg_reconstruct([scan.coefficient_image()], [coefs.data_ptr()], [out.data_ptr()])
    torch.cuda.synchronize()
    want = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    assert np.array_equal(out.cpu().numpy().reshape(120, 160, 3), want)
    # what needs the plan or the weights is refused: MDHIP_EINVAL
    for call in (lambda: ctx.forward(1, 64, 64), lambda: ctx.nms(1, 0.1, 0.5),
                 lambda: ctx.preprocess([np.zeros((64, 64, 3), np.uint8)], [(64, 64, 64, 64, 0, 0)], 64, 64), lambda: ctx.read_predictions(1, 64, 64),
                 lambda: ctx.set_fuse(True), lambda: ctx.set_graph(1)):
        with pytest.raises(HipError, match=r'\(-1\).*no model'):
            call()


def _variety(tmp_path_factory):
    if 'variety' not in _STATE:
        folder = str(tmp_path_factory.mktemp('rde_review_variety'))
        _STATE['variety'] = (folder, S.make_scene(folder, variety=True))
    return _STATE['variety']


def _files(folder):
    out = {}
    for name in sorted(os.listdir(folder)):
        with open(os.path.join(folder, name), 'rb') as f:
            out[name] = f.read()
    return out


@pytest.mark.parametrize('changes', [{}, {'bRenderDetectionTiles': False}, {'detectionTilesPrimaryImageLocation': 'left'}],
                         ids=['defaults', 'no_tiles', 'primary_left'])
def test_gpu_leg_against_host_leg(tmp_path_factory, tmp_path, changes):
    folder, results = _variety(tmp_path_factory)
    legs = {}
    for backend in ('host', 'gpu'):
        rde = RD.mark_repeat_detections(copy.deepcopy(results), rde_options(), backend=backend)
        legs[backend] = RV.write_review_folder(rde, review_options(folder, tmp_path / backend, changes), backend=backend, now=NOW,
                                               rde_options=rde_options())
        if backend == 'gpu':
            flat = [loc for locs in rde.suspicious_detections for loc in locs]
    host, gpu = _files(legs['host']['folder']), _files(legs['gpu']['folder'])
    assert sorted(host) == sorted(gpu) and len(host) == 5              # four samples and the index
    for name in host:
        if name == RV.INDEX_NAME:                                        # (it names the output folder, which differs)
            a, b = json.loads(host[name]), json.loads(gpu[name])
            a['review_options'].pop('outputBase'), b['review_options'].pop('outputBase')
            assert a == b
            continue
        assert host[name] == gpu[name], name
    counts = legs['gpu']
    # every file decoded once, per location (camA, camB); only the PNG and the progressive file by PIL
    needed = [set() for _ in S.CAMERAS]
    tiles = changes.get('bRenderDetectionTiles', True)
    for loc in flat:
        k = S.CAMERAS.index(loc.relativeDir)
        needed[k] |= {i.filename for i in (loc.instances if tiles else loc.instances[:1])}
    by_pil = {f for files in needed for f in files if f.endswith('.png') or f == 'camA/I06.jpg'}
    if tiles:
        assert counts['files_decoded_pil'] == 2 == len(by_pil)
        assert counts['tile_calls'] == counts['decode_chunks'] == 2     # one chunk a location
    else:
        assert counts['files_decoded_pil'] == len(by_pil) and counts['tile_calls'] == 0
    assert counts['files_decoded_gpu'] == sum(len(f) for f in needed) - len(by_pil)
    assert (counts['sheets'], counts['gpu'], counts['host']) == (4, 4, 0)
    if changes:
        return
    # the removal pass after deleting two samples: the same result from either folder
    original = tmp_path / 'in.json'
    original.write_text(json.dumps(results))
    removed = {}
    samples = sorted(n for n in host if n.endswith('.jpg'))
    for backend in ('host', 'gpu'):
        for i in S.DELETED:
            os.remove(os.path.join(legs[backend]['folder'], samples[i]))
        RV.remove_repeat_detections(str(original), str(tmp_path / (backend + '.json')), legs[backend]['folder'], backend=backend)
        removed[backend] = (tmp_path / (backend + '.json')).read_bytes()
    assert removed['host'] == removed['gpu']
    assert sum(d['conf'] < 0 for im in json.loads(removed['gpu'])['images'] for d in im['detections']) > 0


def test_gpu_leg_on_a_detector_context_and_a_sheet_for_the_host_leg(tmp_path_factory, tmp_path):
    """on a context WITH a model (what run_detector_batch hands over), with a line too thick for a box: that sheet's drawing is
    not restated (preview.HostLeg) and the host leg makes it, the others stay on the device; the files are the host leg's"""
    folder, results = _variety(tmp_path_factory)
    changes = {'lineThickness': 24, 'detectionTilesMaxCrops': 3}
    legs = {}
    for backend in ('host', 'gpu'):
        rde = RD.mark_repeat_detections(copy.deepcopy(results), rde_options(), backend=backend)
        legs[backend] = RV.write_review_folder(rde, review_options(folder, tmp_path / backend, changes), backend=backend, now=NOW,
                                               ctx=_model_ctx() if backend == 'gpu' else None)
    host, gpu = _files(legs['host']['folder']), _files(legs['gpu']['folder'])
    assert sorted(host) == sorted(gpu) and all(host[n] == gpu[n] for n in host if n != RV.INDEX_NAME)
    assert legs['gpu']['host'] > 0 and legs['gpu']['gpu'] + legs['gpu']['host'] == 4
