"""
The host half of the GPU JPEG feed, without a GPU: libmdjpeg.so (parser + Huffman decoder) and tests/jpeg_ref.py (the
NumPy restatement of what the GPU kernels compute) against Pillow, bit for bit; the files that must fall back to PIL;
damaged files; the loader processes.

Tolerance is zero everywhere and that is derived, not chosen: both sides run the same integer arithmetic.
"""

import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
import jpeg_fixtures as JF
from jpeg_ref import jpeg_ref, rotate

SIZES = [(1, 1), (8, 8), (17, 9), (16, 16), (333, 517), (640, 480), 'bundled']
# beyond the issue's list: at most two chroma columns (libjpeg replicates instead of interpolating), odd sizes around an MCU
EXTRA_SIZES = [(2, 2), (3, 3), (4, 4), (5, 2), (15, 17), (33, 31)]


@pytest.fixture(scope='module')
def J():
    return JF.ensure_libmdjpeg()


def _size(size):
    return JF.bundled_size() if size == 'bundled' else size


def _load(path):
    from megadetector_amd.feed import load_image
    return np.asarray(load_image(str(path)))


def _check_file(J, path, base=None):
    """the fast path takes the file and rebuilds load_image's pixels; returns (header, coef, unrotated rgb)"""
    from megadetector_amd import feed
    data = open(path, 'rb').read()
    hd = J.parse(data)
    assert hd.supported and hd.rc == 0, (str(path), hd.reason)
    rc, hd, coef = J.decode(data)
    assert rc == 0, (str(path), hd.reason)
    _, rotation = feed.open_for_coefficients(str(path))
    if base is not None and np.array_equal(base[1], coef) and hd.quant.tolist() == base[0].quant.tolist():
        rgb0 = base[2]                       # same coefficients and tables as the file without the EXIF tag: same pixels
    else:
        assert base is None, 'an EXIF tag changed the coefficients'
        rgb0 = jpeg_ref(hd, coef)
    np.testing.assert_array_equal(rotate(rgb0, rotation), _load(path), err_msg=str(path))
    return hd, coef, rgb0


@pytest.mark.parametrize('size', SIZES, ids=lambda s: s if isinstance(s, str) else '{}x{}'.format(*s))
@pytest.mark.parametrize('sampling', JF.SAMPLINGS)
def test_matrix_equals_pillow(J, tmp_path, sampling, size):
    """sampling x size (the test ids) x quality x optimize x restart markers x content x EXIF orientation: every file takes the
    fast path (supported, decode returns 0) and jpeg_ref(coefficients) == np.asarray(load_image(file)), tolerance zero"""
    w, h = _size(size)
    path = str(tmp_path / 'm.jpg')
    n = 0
    for kind in JF.CONTENTS:
        arr = JF.content(kind, w, h)
        for q, opt, rst in itertools.product(JF.QUALITIES, (False, True), JF.RESTARTS):
            base = None
            for orientation in JF.ORIENTATIONS:
                JF.write_jpeg(path, arr, sampling, q, opt, rst, orientation)
                got = _check_file(J, path, base)
                if base is None:
                    base = got
                n += 1
    assert n == 3 * 4 * 2 * 3 * 5


@pytest.mark.parametrize('sampling', JF.SAMPLINGS)
def test_small_and_odd_sizes_equal_pillow(J, tmp_path, sampling):
    path = str(tmp_path / 's.jpg')
    for (w, h), kind, q, rst in itertools.product(EXTRA_SIZES, ('noise', 'gradient'), (75, 100), JF.RESTARTS):
        JF.write_jpeg(path, JF.content(kind, w, h), sampling, q, False, rst)
        _check_file(J, path)


def test_rotation_angles_are_pils(J, tmp_path):
    """jpeg_ref's own rotation argument (what the kernels restate) for every orientation the loader maps to an angle"""
    from megadetector_amd import feed
    arr = JF.content('noise', 37, 21)
    for orientation, angle in [(None, 0), (1, 0), (3, 180), (6, 270), (8, 90), (2, 0)]:
        p = JF.write_jpeg(str(tmp_path / 'r.jpg'), arr, '420', 90, orientation=orientation)
        _, rotation = feed.open_for_coefficients(p)
        assert rotation == angle
        rc, hd, coef = J.decode(open(p, 'rb').read())
        assert rc == 0
        np.testing.assert_array_equal(jpeg_ref(hd, coef, rotation), _load(p))
    # a grayscale file: load_image converts first and the converted image carries no EXIF reader -- it is never rotated
    p = JF.write_jpeg(str(tmp_path / 'g.jpg'), arr, 'gray', 90, orientation=6)
    assert feed.open_for_coefficients(p)[1] == 0
    assert _load(p).shape == (21, 37, 3)


def test_files_that_fall_back(J, tmp_path):
    """unsupported with a reason; the PIL path then decodes them (the loader test below shows the same through the ring)"""
    from PIL import Image
    arr = JF.content('natural', 64, 48)
    prog = JF.write_jpeg(str(tmp_path / 'prog.jpg'), arr, '420', 80, progressive=True)
    cmyk = str(tmp_path / 'cmyk.jpg')
    Image.fromarray(arr).convert('CMYK').save(cmyk, 'JPEG')
    png = str(tmp_path / 'x.png')
    Image.fromarray(arr).save(png)
    # 4:4:0: a 4:2:2 file whose frame header says luma 1 x 2 (Pillow writes no such file; only the header is read here)
    d = bytearray(open(JF.write_jpeg(str(tmp_path / 's422.jpg'), arr, '422', 80), 'rb').read())
    k = d.index(b'\xff\xc0')
    assert d[k + 11] == 0x21
    d[k + 11] = 0x12
    s440 = str(tmp_path / 's440.jpg')
    open(s440, 'wb').write(bytes(d))
    for path, word in [(prog, 'progressive'), (cmyk, 'four components'), (png, 'not a JPEG'), (s440, 'sampling')]:
        hd = J.parse(open(path, 'rb').read())
        assert not hd.supported and hd.rc == J.MDJPEG_EUNSUPPORTED and word in hd.reason, (path, hd.reason)
        rc, hd2, _ = J.decode(open(path, 'rb').read())
        assert rc == J.MDJPEG_EUNSUPPORTED and hd2.reason == hd.reason
    np.testing.assert_array_equal(_load(prog).shape, (48, 64, 3))
    np.testing.assert_array_equal(_load(png), arr)
    with pytest.raises(AttributeError, match='unsupported mode'):
        _load(cmyk)
    for junk in (b'', b'\xff', b'\xff\xd8', b'\xff\xd8\xff', b'\xff\xd8\xff\xc0\x00', os.urandom(64)):
        hd = J.parse(junk)
        assert not hd.supported and hd.reason


def test_mirrored_orientation_stays_unrotated(J, tmp_path):
    """orientation 2: load_image's assert fails inside its own try and the image stays as decoded; so does the fast path"""
    from megadetector_amd import feed
    arr = JF.content('natural', 40, 24)
    p = JF.write_jpeg(str(tmp_path / 'm.jpg'), arr, '422', 85, orientation=2)
    assert feed.open_for_coefficients(p)[1] == 0
    rc, hd, coef = J.decode(open(p, 'rb').read())
    assert rc == 0
    np.testing.assert_array_equal(jpeg_ref(hd, coef, 0), _load(p))


GUARD = 4096


def _damaged_variants(tmp_path):
    """(name, bytes) of damaged files: truncated at 25 / 50 / 99 % of the scan, one byte flipped inside the scan at 10 seeded
    positions, a removed restart marker -- over the samplings, with and without restart markers"""
    out = []
    rng = np.random.default_rng(2024)
    for sampling, rst, kind in [('420', None, 'noise'), ('420', 'rows', 'natural'), ('444', 'blocks', 'noise'),
                                ('gray', None, 'natural'), ('422', 'rows', 'gradient')]:
        p = JF.write_jpeg(str(tmp_path / 'good.jpg'), JF.content(kind, 96, 64), sampling, 85, False, rst)
        data = open(p, 'rb').read()
        a, b = JF.scan_range(data)
        tag = '{}_{}'.format(sampling, rst)
        for pc in (25, 50, 99):
            out.append(('{}_trunc{}'.format(tag, pc), data[:a + (b - a) * pc // 100]))
        for pos in rng.integers(a, b, 10):
            d = bytearray(data)
            d[pos] ^= int(rng.integers(1, 256))
            out.append(('{}_flip{}'.format(tag, pos), bytes(d)))
        if rst is not None:
            k = data.index(b'\xff\xd0', a)
            out.append(('{}_norst'.format(tag), data[:k] + data[k + 2:]))
            k3 = data.index(b'\xff\xd1', a)
            out.append(('{}_rstseq'.format(tag), data[:k3 + 1] + b'\xd3' + data[k3 + 2:]))
    return out


def _pil_pixels(path):
    import warnings
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return _load(path)
    except Exception:
        return None


def test_damaged_files_error_or_equal_pillow(J, tmp_path):
    """mdjpeg_decode returns an error or coefficients whose pixels equal PIL's -- never different pixels, never a crash,
    never a write past `capacity` (a guard band behind the buffer keeps its pattern)"""
    variants = _damaged_variants(tmp_path)
    assert len(variants) >= 5 * 13
    n_err = n_ok = 0
    for name, data in variants:
        hd = J.parse(data)
        if not hd.supported:
            n_err += 1
            continue
        buf = np.full(hd.coef_count + GUARD, 0x5A5A, dtype=np.int16)
        rc, hd2, _ = J.decode(data, out=buf[:hd.coef_count])
        assert (buf[hd.coef_count:] == 0x5A5A).all(), name
        if rc != 0:
            assert rc == J.MDJPEG_ECORRUPT and hd2.reason, (name, rc)
            n_err += 1
            continue
        p = str(tmp_path / 'damaged.jpg')
        with open(p, 'wb') as f:
            f.write(data)
        want = _pil_pixels(p)
        assert want is not None, '{}: decoded cleanly here, PIL refuses the file'.format(name)
        np.testing.assert_array_equal(jpeg_ref(hd2, buf[:hd.coef_count]), want, err_msg=name)
        n_ok += 1
    print('damaged files: {} refused, {} decoded to PIL\'s pixels'.format(n_err, n_ok))
    assert n_err > 0
    # a capacity that is too small is refused before anything is written
    good = open(JF.write_jpeg(str(tmp_path / 'g.jpg'), JF.content('noise', 32, 32), '420'), 'rb').read()
    hd = J.parse(good)
    buf = np.full(hd.coef_count, 0x5A5A, dtype=np.int16)
    rc, _, _ = J.decode(good, out=buf[:hd.coef_count - 64])
    assert rc == J.MDJPEG_ECAPACITY and (buf == 0x5A5A).all()


def test_damaged_files_under_sanitizers(J, tmp_path):
    """the same files through host_asan_main.cpp, a program around jpeg_entropy.cpp (and the library's other sources) built with
    AddressSanitizer + UBSan (host code; `make asan-jpeg`): the buffers have their exact sizes there, so any read or write outside them, and any undefined arithmetic, ends the run"""
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'jpeg_entropy_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-jpeg', 'ASAN_OUT=' + exe])
    files = []
    for name, data in _damaged_variants(tmp_path):
        p = str(tmp_path / (name + '.jpg'))
        with open(p, 'wb') as f:
            f.write(data)
        files.append(p)
    files.append(JF.write_jpeg(str(tmp_path / 'fine.jpg'), JF.content('noise', 333, 517), '420', 95, True, 'rows'))
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(': rc ') == len(files)
    assert 'fine.jpg: rc 0' in r.stdout


def test_loader_coefficient_mode_mixed_folder(J, tmp_path):
    """ProcessLoader(decode='coefficients') yields 'jpeg' for the supported files and, for every other file, exactly what the
    default mode yields; the coefficient slots rebuild load_image's pixels; metadata is the rotated image's"""
    from PIL import Image
    from megadetector_amd import feed
    from megadetector_amd.jpeg_host import CoefficientImage
    arr = JF.content('natural', 80, 56)
    files = {
        'a420.jpg': JF.write_jpeg(str(tmp_path / 'a420.jpg'), arr, '420', 80),
        'b422_rot.jpg': JF.write_jpeg(str(tmp_path / 'b422_rot.jpg'), arr, '422', 90, orientation=6),
        'c_gray.jpg': JF.write_jpeg(str(tmp_path / 'c_gray.jpg'), arr, 'gray', 75, restart='rows'),
        'd_prog.jpg': JF.write_jpeg(str(tmp_path / 'd_prog.jpg'), arr, '420', 80, progressive=True),
        'g_big.jpg': JF.write_jpeg(str(tmp_path / 'g_big.jpg'), JF.content('noise', 400, 300), '444', 90),
    }
    Image.fromarray(arr).save(str(tmp_path / 'e.png'))
    files['e.png'] = str(tmp_path / 'e.png')
    with open(str(tmp_path / 'f_broken.jpg'), 'wb') as f:
        f.write(b'this is not an image')
    files['f_broken.jpg'] = str(tmp_path / 'f_broken.jpg')
    good = open(files['a420.jpg'], 'rb').read()
    a, b = JF.scan_range(good)
    with open(str(tmp_path / 'h_trunc.jpg'), 'wb') as f:
        f.write(good[:a + (b - a) // 2])
    files['h_trunc.jpg'] = str(tmp_path / 'h_trunc.jpg')
    paths = [files[k] for k in sorted(files)]
    # 400 x 300 x 3 = 360 000 bytes of pixels fit a slot, its 4:4:4 coefficients (2 bytes each, whole MCUs) do not
    slot_bytes = 400 * 1024

    def run(decode):
        loader = feed.ProcessLoader(paths, 2, 6, slot_bytes, want_meta=True, decode=decode)
        got = {}
        try:
            for kind, f, payload, shape, meta in loader:
                if kind == 'slot':
                    px = np.array(loader.ring.view(payload, shape))
                    loader.ring.release(payload)
                elif kind == 'jpeg':
                    ci = feed.coefficient_image(loader.ring, payload, shape)
                    assert isinstance(ci, CoefficientImage) and ci.shape == tuple(shape)
                    hd = J.parse(open(f, 'rb').read())
                    px = jpeg_ref(hd, np.array(ci.coef), ci.rotation)
                    assert np.array_equal(ci.quant, hd.quant)
                    loader.ring.release(payload)
                elif kind == 'array':
                    px = payload
                else:
                    px = None
                got[os.path.basename(f)] = (kind, None if shape is None else tuple(shape), meta, px)
        finally:
            loader.close()
        return got

    plain = run('pixels')
    coef = run('coefficients')
    assert sorted(plain) == sorted(coef) == sorted(files)
    assert {k: v[0] for k, v in coef.items()} == {
        'a420.jpg': 'jpeg', 'b422_rot.jpg': 'jpeg', 'c_gray.jpg': 'jpeg', 'd_prog.jpg': 'slot', 'e.png': 'slot',
        'f_broken.jpg': 'fail', 'g_big.jpg': 'slot', 'h_trunc.jpg': plain['h_trunc.jpg'][0]}
    assert {k: v[0] for k, v in plain.items() if k != 'h_trunc.jpg'} == {
        'a420.jpg': 'slot', 'b422_rot.jpg': 'slot', 'c_gray.jpg': 'slot', 'd_prog.jpg': 'slot', 'e.png': 'slot',
        'f_broken.jpg': 'fail', 'g_big.jpg': 'slot'}
    for k in files:
        assert coef[k][1] == plain[k][1], k
        assert coef[k][2] == plain[k][2], k
        if plain[k][3] is None:
            assert coef[k][3] is None
        else:
            np.testing.assert_array_equal(coef[k][3], plain[k][3], err_msg=k)
    assert plain['b422_rot.jpg'][1] == (80, 56, 3) and plain['b422_rot.jpg'][2]['width'] == 56


def test_loader_side_stays_off_the_gpu(J, tmp_path):
    """a fresh process that imports the binding and decodes a file maps neither the HIP nor the HSA runtime and never
    imports torch: a loader process does not count against the processes that have the GPU open"""
    p = JF.write_jpeg(str(tmp_path / 'x.jpg'), JF.content('natural', 64, 48), '420', 80)
    code = (
        'import sys, json\n'
        'sys.path.insert(0, {!r})\n'
        'from megadetector_amd import jpeg_host, feed\n'
        'rc, hd, coef = jpeg_host.decode(open({!r}, "rb").read())\n'
        'maps = open("/proc/self/maps").read()\n'
        'print(json.dumps(dict(rc=rc, n=int(hd.coef_count), hip="amdhip" in maps, hsa="hsa-runtime" in maps,\n'
        '                      torch="torch" in sys.modules, mdjpeg="libmdjpeg" in maps, mdhip="libmdhip" in maps)))\n'
    ).format(REPO, p)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == dict(rc=0, n=got['n'], hip=False, hsa=False, torch=False, mdjpeg=True, mdhip=False) and got['n'] > 0
