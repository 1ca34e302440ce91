"""
The gray-pixel share without a GPU (megadetector_amd/gray_scale.py, csrc/gray_count.h, mdjpeg_gray_count):

  * the host leg equals what the reference's own gray_scale_fraction returned for the scene of tests/resize_scene.py
    (tests/golden/resize_reference.json, written by tests/golden/gen_resize_reference.py), float for float, and direct numpy calls;
  * the device leg's steps on the host -- the pixels load_image gives (what a device image holds), the window window_of maps the
    reference's band of rows to, the host model's count, one division -- give the same floats, EXIF-rotated files included;
  * the host model, the plain loop and the kernel's walk of a row, equals numpy on every scene file and on the kernel's case
    list (tests/gray_cases.py), and refuses what the header says with the counters untouched;
  * `make asan-gray` runs clean.
"""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import gray_cases
import resize_scene as S
from conftest import GOLDEN, REPO


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(GOLDEN, 'resize_reference.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def scene(tmp_path_factory, golden):
    folder = str(tmp_path_factory.mktemp('gray_scene'))
    return folder, S.build(folder)


@pytest.fixture(scope='module')
def exact(scene, golden):
    """the recorded floats hold for the recorded Pillow version and scene; with another encoder the pixels differ, and the tests
    still assert everything else: the two legs against each other and against numpy, the shares that do not depend on pixels"""
    return S.is_exact(golden, scene[0])


def agrees(got_hexes, want_hexes, exact):
    """the recorded floats when exact; whatever the encoder, the same files answer and 1.0 stays 1.0"""
    if exact:
        return got_hexes == want_hexes
    one = (1.0).hex()
    return [g is None for g in got_hexes] == [w is None for w in want_hexes] and all(g == one for g, w in zip(got_hexes, want_hexes) if w == one)


def wanted(golden, crop):
    return [golden['gray']['{},{}'.format(*crop)][name] for name, *_ in S.IMAGES]


def hexes(fractions):
    return [None if f is None else float(f).hex() for f in fractions]


@pytest.fixture(scope='module', autouse=True)
def _built():
    import __graft_entry__ as G
    G.build()


def test_scene_has_the_shares_it_is_meant_to_have(golden):
    """the fixture itself: a share strictly between 0 and 1 that changes with the crop, 1.0 for 'L', one band and gray RGB, and a
    float for the truncated file (the reference loads truncated files)"""
    with_crop, without = golden['gray']['0.1,0.1'], golden['gray']['0,0']
    a, b = float.fromhex(with_crop['dusk420.jpg']), float.fromhex(without['dusk420.jpg'])
    assert 0.3 < a < 0.5 and 0.3 < b < 0.5 and a != b
    for name in ('grey_l.jpg', 'grey_rgb.jpg', 'palette.png'):
        assert float.fromhex(with_crop[name]) == 1.0
    assert with_crop['truncated.jpg'] is not None and not golden['gray_errors']['0.1,0.1']


@pytest.mark.parametrize('crop', S.CROPS)
def test_host_leg_equals_the_reference(scene, golden, exact, crop):
    from megadetector_amd import gray_scale as G
    _, files = scene
    counts = {}
    got = G.gray_scale_fractions(files, crop, backend='host', counts=counts)
    assert agrees(hexes(got), wanted(golden, crop), exact)
    assert all(type(f) is float for f in got)
    assert counts['files'] == counts['host'] == len(files) and counts['gpu'] == 0 and counts['gray_calls'] == 0
    # a file that does not open
    assert G.gray_scale_fractions([files[0] + '.missing', files[0]], crop, backend='host') == [None, got[0]]


def test_host_function_equals_direct_numpy_calls(scene):
    """gray_scale_fraction against slicing the decoded array: no PIL crop, no getchannel"""
    from PIL import ImageFile
    from megadetector_amd import gray_scale as G
    _, files = scene
    for (name, w, h, *_), path in zip(S.IMAGES, files):
        if name == 'truncated.jpg':
            continue
        im = Image.open(path)
        for crop in S.CROPS:
            got = G.gray_scale_fraction(path, crop)
            if len(im.getbands()) == 1:
                assert got == 1.0
                continue
            a = np.asarray(im.convert('RGB') if im.mode != 'RGB' else im).astype(np.int32)
            a = a[int(h * crop[0]):h - int(h * crop[1])]
            n = int(((a[..., 0] == a[..., 1]) & (a[..., 0] == a[..., 2])).sum())
            assert got == n / (a.shape[0] * a.shape[1]), (name, crop)
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False, 'the truncation rule leaked out of the call'
    # a PIL image instead of a name, and the assertion on the crop
    assert G.gray_scale_fraction(Image.open(files[0]), (0, 0)) == G.gray_scale_fraction(files[0], (0, 0))


def test_illegal_crop_is_the_reference_assertion(scene, golden):
    from megadetector_amd import gray_scale as G
    _, files = scene
    with pytest.raises(AssertionError) as e:
        G.gray_scale_fraction(files[0], (0.5, 0.5))
    assert str(e.value) == golden['illegal_crop']
    with pytest.raises(AssertionError, match='Illegal crop size'):
        G.gray_scale_fractions(files[:1], (0.5, 0.5), backend='host')
    with pytest.raises(AssertionError, match='Illegal crop size'):
        G.plan_file(files[0], (0.75, 0.25))
    # an 'L' file answers before the assertion, as in the reference
    assert G.gray_scale_fraction(files[3], (0.5, 0.5)) == 1.0 and G.plan_file(files[3], (0.5, 0.5)) == 1.0


@pytest.mark.parametrize('rotation', [0, 90, 180, 270])
def test_window_of_holds_the_stored_band(rotation):
    """the rectangle of the rotated image holds exactly the pixels of the stored rows the reference keeps"""
    from megadetector_amd.gray_scale import window_of
    rng = np.random.default_rng(rotation)
    for w, h, top, bottom in [(7, 5, 1, 2), (4, 9, 0, 3), (5, 5, 2, 0), (1, 3, 1, 1), (6, 1, 0, 0)]:
        stored = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        turned = np.asarray(Image.fromarray(stored).rotate(rotation, expand=True)) if rotation else stored
        x, y, ww, wh = window_of((w, h), rotation, top, bottom)
        assert 0 <= x and 0 <= y and x + ww <= turned.shape[1] and y + wh <= turned.shape[0]
        got = turned[y:y + wh, x:x + ww].reshape(-1, 3)
        want = stored[top:h - bottom].reshape(-1, 3)
        assert sorted(map(tuple, got)) == sorted(map(tuple, want))


@pytest.mark.parametrize('crop', S.CROPS)
def test_device_leg_steps_on_the_host_models(scene, golden, exact, crop):
    """plan_file -> the pixels a device image holds (load_image: after the EXIF rotation) -> mdjpeg_gray_count on the window,
    plainly and with the kernel's walk -> n_gray / n_pixels: the reference's float for every file the device leg plans, and the
    files it leaves to the host leg are the ones named here"""
    from megadetector_amd import gray_scale as G, jpeg_host
    from megadetector_amd.feed import load_image
    _, files = scene
    # (with another encoder than the recorded one the pixels differ: the host leg's float stands in for the recorded one)
    want = wanted(golden, crop) if exact else hexes(G.gray_scale_fractions(files, crop, backend='host'))
    kinds = {}
    for (name, *_), path, reference in zip(S.IMAGES, files, want):
        plan = G.plan_file(path, crop)
        kinds[name] = plan if not isinstance(plan, dict) else 'device'
        if not isinstance(plan, dict):
            continue
        pixels = np.ascontiguousarray(np.asarray(load_image(path)))
        assert (pixels.shape[1], pixels.shape[0]) == plan['size']
        for walk in (False, True):
            n_gray, = jpeg_host.gray_count([pixels], [plan['window']], walk=walk)
            assert (n_gray / plan['pixels']).hex() == reference, (name, walk)
    assert {k for k, v in kinds.items() if v == 'host'} == {'sub/prog.jpg', 'pic.png', 'truncated.jpg'}
    assert {k for k, v in kinds.items() if v == 1.0} == {'grey_l.jpg', 'palette.png'}
    assert sum(v == 'device' for v in kinds.values()) == 10
    assert G.plan_file(files[0] + '.missing', crop) is None
    assert G.plan_file(files[0], (-0.1, 0.2)) == 'host'                     # a negative crop pads in PIL: the host leg's


def test_host_model_equals_numpy_on_the_scene(scene):
    from megadetector_amd import jpeg_host
    _, files = scene
    images = []
    for (name, *_), path in zip(S.IMAGES, files):
        if name != 'truncated.jpg':
            images.append(np.ascontiguousarray(np.asarray(Image.open(path).convert('RGB'))))
    want = [gray_cases.count(a, (0, 0, a.shape[1], a.shape[0])) for a in images]
    assert jpeg_host.gray_count(images) == want
    assert jpeg_host.gray_count(images, walk=True) == want
    assert max(want) > 0 and any(v == a.shape[0] * a.shape[1] for v, a in zip(want, images))


def test_host_model_equals_numpy_on_the_kernel_cases():
    from megadetector_amd import jpeg_host
    cases = gray_cases.cases()
    assert len(cases) > 1000
    assert {c['w'] for c in cases} == set(gray_cases.WIDTHS) and {c['pitch'] % 2 for c in cases} == {0, 1}
    for walk in (False, True):
        got = jpeg_host.gray_count([gray_cases.view(c) for c in cases], [c['window'] for c in cases], walk=walk)
        wrong = [(c['name'], g, c['want']) for c, g in zip(cases, got) if g != c['want']]
        assert not wrong, wrong[:5]
    many = gray_cases.many()
    for walk in (False, True):
        assert jpeg_host.gray_count([gray_cases.view(c) for c in many], [c['window'] for c in many], walk=walk) == [c['want'] for c in many]


def test_host_model_refuses_with_nothing_written():
    import ctypes as C
    from megadetector_amd import jpeg_host
    lib = jpeg_host.load()
    px = np.zeros((4, 6, 3), np.uint8)

    def call(fn, window, n=1, width=6, height=4, pitch=18, image=px.ctypes.data):
        counts = np.full(2, 77, np.uint64)
        rc = fn((C.c_void_p * 1)(image), (C.c_int32 * 1)(width), (C.c_int32 * 1)(height), (C.c_int64 * 1)(pitch),
                (C.c_int32 * 4)(*window), n, counts.ctypes.data)
        return rc, counts.tolist()

    for fn in (lib.mdjpeg_gray_count, lib.mdjpeg_gray_count_walk):
        assert call(fn, (0, 0, 6, 4)) == (jpeg_host.MDJPEG_OK, [24, 77])
        assert call(fn, (5, 3, 1, 1)) == (jpeg_host.MDJPEG_OK, [1, 77])
        for window in [(1, 0, 6, 4), (0, 1, 6, 4), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 4), (0, 0, 6, 0), (6, 0, 1, 1), (0, 0, 2 ** 31 - 1, 1)]:
            assert call(fn, window) == (jpeg_host.MDJPEG_EINVAL, [77, 77]), window
        assert call(fn, (0, 0, 6, 4), n=0)[0] == jpeg_host.MDJPEG_EINVAL
        assert call(fn, (0, 0, 6, 4), n=65536)[0] == jpeg_host.MDJPEG_EINVAL
        assert call(fn, (0, 0, 6, 4), pitch=17) == (jpeg_host.MDJPEG_EINVAL, [77, 77])
        assert call(fn, (0, 0, 6, 4), width=0) == (jpeg_host.MDJPEG_EINVAL, [77, 77])
        assert call(fn, (0, 0, 6, 4), height=65536) == (jpeg_host.MDJPEG_EINVAL, [77, 77])
        assert call(fn, (0, 0, 6, 4), image=None) == (jpeg_host.MDJPEG_EINVAL, [77, 77])
    with pytest.raises(ValueError):
        jpeg_host.gray_count([px], [(1, 0, 6, 4)])
    with pytest.raises(ValueError):
        jpeg_host.gray_count([px[:, :, ::-1]])


def test_cli_writes_the_fractions(scene, golden, exact, tmp_path, capsys):
    from megadetector_amd import gray_scale as G
    folder, files = scene
    out = str(tmp_path / 'gray.csv')
    assert G.main([folder, '--output_csv', out, '--backend', 'host', '--crop_top', '0.25', '--crop_bottom', '0.05']) == 0
    with open(out, newline='') as f:
        lines = f.read().split('\n')
    assert lines[0] == 'image,gray_scale_fraction' and lines[-1] == ''
    rows = dict(line.split(',') for line in lines[1:-1])
    assert list(rows) == sorted(name for name, *_ in S.IMAGES)              # find_images: recursive, sorted, forward slashes
    names = sorted(rows)
    assert agrees([float(rows[n]).hex() for n in names], [golden['gray']['0.25,0.05'][n] for n in names], exact)
    assert [float(rows[n]) for n in names] == G.gray_scale_fractions([os.path.join(folder, n) for n in names], (0.25, 0.05), backend='host')
    assert '15 files: 0 on the device, 15 on the host, 0 unreadable' in capsys.readouterr().err
    assert G.main([folder, '--backend', 'host']) == 0
    assert capsys.readouterr().out.startswith('image,gray_scale_fraction\n')


def test_the_call_is_declared_and_bound():
    from megadetector_amd import _lib, jpeg_host
    assert 'mdhip_gray_count' in _lib.SYMBOLS and {'mdjpeg_gray_count', 'mdjpeg_gray_count_walk'} <= set(jpeg_host.SYMBOLS)
    for header, name in (('mdhip.h', 'mdhip_gray_count'), ('mdjpeg.h', 'mdjpeg_gray_count'), ('mdjpeg.h', 'mdjpeg_gray_count_walk')):
        assert name + '(' in open(os.path.join(REPO, 'include', header)).read()
    assert hasattr(_lib.load(), 'mdhip_gray_count')


def test_host_model_under_the_sanitizers(tmp_path):
    """`make asan-gray`: both host functions in a build with AddressSanitizer + UBSan, as a program of its own, on images that lie
    in heap blocks of exactly their bytes at every byte offset -- a read outside the rows is reported"""
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'gray_host_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-gray', 'GRAY_ASAN_OUT=' + exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert '2592 cases, 0 wrong' in r.stdout
