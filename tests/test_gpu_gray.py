"""
The gray-pixel count on the GPU: mdhip_gray_count against numpy and its host model mdjpeg_gray_count over the sentinel-filled
case list of tests/gray_cases.py (every width, height, base offset, pitch and window; a read outside a window's rows miscounts),
what the call refuses with the counters untouched, many images of different sizes in one call, an image large enough for the
grid's cap and its strides; and gray_scale.gray_scale_fractions on the device against its host leg and against what the
reference's own function returned for the scene (tests/golden/resize_reference.json), with the counts asserted.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import gray_cases
import resize_scene as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from megadetector_amd.hip_backend import HipContext
    c = HipContext.for_images(0)
    yield c
    c.close()


def upload(cases):
    """every case's allocation in one device tensor, each at a multiple of 256 bytes (so a case's offset is its offset within an
    aligned allocation) -> (the tensor, per case the device address of its first pixel)"""
    import torch
    starts, total = [], 0
    for c in cases:
        starts.append(total)
        total += (c['buffer'].size + 255) // 256 * 256
    host = np.zeros(total, np.uint8)
    for c, s in zip(cases, starts):
        host[s:s + c['buffer'].size] = c['buffer']
    dev = torch.from_numpy(host).to(torch.device('cuda', 0))
    assert dev.data_ptr() % 256 == 0
    return dev, [dev.data_ptr() + s + c['offset'] for c, s in zip(cases, starts)]


def device_counts(ctx, cases, ptrs):
    return ctx.gray_count(ptrs, [(c['w'], c['h']) for c in cases], [c['pitch'] for c in cases], [c['window'] for c in cases])


@pytest.fixture(scope='module')
def case_list():
    cases = gray_cases.cases()
    dev, ptrs = upload(cases)
    return cases, dev, ptrs


def test_kernel_equals_numpy_and_the_host_model_in_one_call(ctx, case_list):
    """all cases as the images of ONE call: widths 1 .. 33, heights 1 and 2, base offsets 0, 1, 3 and 7, tight (odd) and padded
    pitches, windows at x = 1 and x = 5, all-gray images, one pixel that is not gray at each corner and at pixel 5, each with
    sentinels that look gray and with sentinels that do not"""
    from megadetector_amd import jpeg_host
    cases, _, ptrs = case_list
    got = device_counts(ctx, cases, ptrs)
    model = jpeg_host.gray_count([gray_cases.view(c) for c in cases], [c['window'] for c in cases])
    wrong = [(c['name'], g, c['want']) for c, g in zip(cases, got) if g != c['want']]
    assert not wrong, (len(wrong), wrong[:8])
    assert got == model
    # the counters are zeroed by every call: the same call again gives the same counts, not their double
    assert device_counts(ctx, cases, ptrs) == got


def test_kernel_one_image_a_call(ctx, case_list):
    cases, _, ptrs = case_list
    for k in range(0, len(cases), 29):
        assert device_counts(ctx, cases[k:k + 1], ptrs[k:k + 1]) == [cases[k]['want']], cases[k]['name']


def test_24_images_of_different_sizes_in_one_call(ctx):
    many = gray_cases.many(24)
    assert len({(c['w'], c['h']) for c in many}) >= 20
    dev, ptrs = upload(many)
    assert device_counts(ctx, many, ptrs) == [c['want'] for c in many]
    del dev


def test_an_image_above_the_grid_cap(ctx):
    """2301 x 1999 pixels are 1.15 million groups of four: more than 1024 workgroups x 256 lanes x 4, so the grid is capped and
    every lane strides; an odd padded pitch and an odd base, a window off every edge"""
    rng = np.random.default_rng(5)
    w, h = 2301, 1999
    pixels = rng.integers(0, 256, (h, w, 1)).astype(np.uint8).repeat(3, axis=2)
    pixels[..., 2] ^= (rng.integers(0, 4, (h, w)) == 0).astype(np.uint8)
    buffer, start, pitch = gray_cases.place(pixels, 3, 7, True)
    for window in [(0, 0, w, h), (3, 2, w - 4, h - 5)]:
        case = {'w': w, 'h': h, 'offset': start, 'pitch': pitch, 'window': window, 'buffer': buffer}
        dev, ptrs = upload([case])
        assert device_counts(ctx, [case], ptrs) == [gray_cases.count(pixels, window)]
        del dev


def test_refusals_leave_the_counters_untouched(ctx, case_list):
    import torch
    from megadetector_amd._lib import HipError
    cases, _, ptrs = case_list
    k = next(i for i, c in enumerate(cases) if c['window'] == (0, 0, 17, 2))
    c, p = cases[k], ptrs[k]
    size, pitch = (c['w'], c['h']), c['pitch']
    counts = np.full(3, 77, np.uint64)
    assert ctx.gray_count([p], [size], [pitch], [(0, 0, 17, 2)], counts=counts) == [c['want']] and counts.tolist() == [c['want'], 77, 77]
    counts[:] = 77
    for window in [(1, 0, 17, 2), (0, 1, 17, 2), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 17, 0), (17, 0, 1, 1), (0, 0, 2 ** 31 - 1, 1)]:
        with pytest.raises(HipError, match='window'):
            ctx.gray_count([p], [size], [pitch], [window], counts=counts)
    with pytest.raises(HipError, match='pitch'):
        ctx.gray_count([p], [size], [3 * 17 - 1], [(0, 0, 17, 2)], counts=counts)
    with pytest.raises(HipError):
        ctx.gray_count([p], [(0, 2)], [pitch], [(0, 0, 1, 1)], counts=counts)
    with pytest.raises(HipError):
        ctx.gray_count([0], [size], [pitch], [(0, 0, 17, 2)], counts=counts)
    # a host pointer, alone and behind a device image
    host = np.zeros((2, 17, 3), np.uint8)
    with pytest.raises(HipError, match='host pointer'):
        ctx.gray_count([host.ctypes.data], [size], [pitch], [(0, 0, 17, 2)], counts=counts)
    with pytest.raises(HipError, match='image 1: a host pointer'):
        ctx.gray_count([p, host.ctypes.data], [size, size], [pitch, pitch], [(0, 0, 17, 2)] * 2, counts=counts)
    # n outside 1 .. 65535 (the arrays are long enough for what is claimed)
    lib = ctx.lib
    for n in (0, -1, 65536):
        m = max(n, 1)
        rc = lib.mdhip_gray_count(ctx.h, C.cast((C.c_void_p * m)(*[p] * m), C.c_void_p), (C.c_int32 * m)(*[17] * m), (C.c_int32 * m)(*[2] * m),
                                  (C.c_int64 * m)(*[pitch] * m), (C.c_int32 * (4 * m))(*[0, 0, 17, 2] * m), n, counts.ctypes.data, None)
        assert rc != 0 and b'outside 1 .. 65535' in lib.mdhip_last_error(ctx.h)
    assert lib.mdhip_gray_count(ctx.h, None, None, None, None, None, 1, counts.ctypes.data, None) != 0
    assert counts.tolist() == [77, 77, 77]
    torch.cuda.synchronize()
    # and the context still works
    assert ctx.gray_count([p], [size], [pitch], [c['window']]) == [c['want']]


# ---- the tool -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'resize_reference.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def scene(tmp_path_factory, golden):
    folder = str(tmp_path_factory.mktemp('gray_scene'))
    files = S.build(folder)
    assert S.scene_hash(folder) == golden['scene'], 'the scene is not the one the fixture was recorded for'
    return folder, files


#: what the device leg leaves to the host leg: the progressive file and the truncated one (the GPU's decoder takes neither) and
#: the PNG; the 'L' JPEG and the palette PNG are answered from their headers
HOST_FILES = ('sub/prog.jpg', 'pic.png', 'truncated.jpg')
NO_DECODE = ('grey_l.jpg', 'palette.png')


@pytest.mark.parametrize('crop', S.CROPS)
def test_device_leg_equals_host_leg_and_reference(ctx, scene, golden, crop):
    from megadetector_amd import gray_scale as G
    _, files = scene
    counts = {}
    got = G.gray_scale_fractions(files, crop, backend='gpu', ctx=ctx, counts=counts)
    host = G.gray_scale_fractions(files, crop, backend='host')
    assert all(f is None or type(f) is float for f in got)
    assert [f.hex() for f in got] == [f.hex() for f in host]
    assert [f.hex() for f in got] == [golden['gray']['{},{}'.format(*crop)][name] for name, *_ in S.IMAGES]
    n = len(files)
    assert counts == {'files': n, 'gpu': n - len(HOST_FILES) - len(NO_DECODE), 'host': len(HOST_FILES), 'no_decode': len(NO_DECODE),
                      'unreadable': 0, 'files_decoded_gpu': n - len(HOST_FILES) - len(NO_DECODE), 'files_decoded_pil': len(HOST_FILES),
                      'decode_chunks': 1, 'gray_calls': 1}


def test_device_leg_one_call_a_chunk_and_files_that_do_not_open(ctx, scene, golden, monkeypatch):
    from megadetector_amd import device_render, gray_scale as G
    _, files = scene
    monkeypatch.setattr(device_render, 'DECODE_CHUNK_BYTES', 100000)       # two or three scene images a chunk
    listed = [files[0] + '.missing'] + files + files[:3]
    counts = {}
    got = G.gray_scale_fractions(listed, (0.1, 0.1), backend='gpu', device=0, counts=counts, profile=True)
    want = [golden['gray']['0.1,0.1'][name] for name, *_ in S.IMAGES]
    assert [None if f is None else f.hex() for f in got] == [None] + want + want[:3]
    assert counts['decode_chunks'] >= 4 and counts['gray_calls'] == counts['decode_chunks']
    assert counts['unreadable'] == 1 and counts['gpu'] == 13 and counts['host'] == 3 and counts['no_decode'] == 2
    assert set(counts['ms']) == {'decode', 'gray_count'}


def test_illegal_crop_on_the_gpu_backend(ctx, scene):
    """the reference's assertion, raised while the files are planned: nothing is decoded; an 'L' file answers before it"""
    from megadetector_amd import gray_scale as G
    _, files = scene
    counts = {}
    with pytest.raises(AssertionError, match='Illegal crop size'):
        G.gray_scale_fractions(files[:1], (0.5, 0.5), backend='gpu', ctx=ctx, counts=counts)
    assert counts['gray_calls'] == 0 and counts['decode_chunks'] == 0
    assert G.gray_scale_fractions([files[3]], (0.5, 0.5), backend='gpu', ctx=ctx) == [1.0]


def test_cli_on_the_device(scene, golden, tmp_path, capsys):
    from megadetector_amd import gray_scale as G
    folder, _ = scene
    out = str(tmp_path / 'gray.csv')
    assert G.main([folder, '--output_csv', out]) == 0
    with open(out, newline='') as f:
        rows = dict(line.split(',') for line in f.read().split('\n')[1:-1])
    assert {k: float(v).hex() for k, v in rows.items()} == golden['gray']['0.1,0.1']
    assert '15 files: 10 on the device, 3 on the host, 0 unreadable' in capsys.readouterr().err
