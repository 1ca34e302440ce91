"""
Entropy encoding of crops, host side: the host model of the GPU encoder (mdjpeg_encode_subsequences in libmdjpeg.so, compiled
from csrc/jpeg_encode.h like the kernels) and jpeg_host.jfif_file against Pillow, byte for byte.

For every quality x size x content: the coefficients of tests/jpeg_enc_ref.py (pinned against Pillow by
test_tile_jpeg_cpu.py) go through the host model, jfif_file puts the file around the scan, and the result must be the
bytes of Image.fromarray(rgb).save(f, 'JPEG', quality=q).  All contents of a (quality, size) travel in ONE call, as a batch
of crops does on the device, at the smallest stuffing chunks, so that stuffed bytes fall on and next to chunk boundaries.
"""

import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_enc_ref as E
from conftest import REPO
from megadetector_amd import jpeg_host as J
from test_tile_jpeg_cpu import CONTENTS, SIZES, make_content, pillow_file

QUALITIES = [1, 50, 75, 95, 100]
EXTRA_SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 17), (33, 15)]
ALL_SIZES = SIZES + [s for s in EXTRA_SIZES if s not in SIZES]
ZIGZAG = np.array(J._ZIGZAG)


def coefficients(rgb, quality):
    """flat int16 planes in the layout of mdjpeg_decode, from the NumPy restatement of the encoder's lossy half"""
    return np.concatenate([p.reshape(-1) for p in E.encode(rgb, quality).planes()])


def chunks_for(w, h):
    return (1, 2, 3, 64) if w * h <= 128 * 128 else (1, 64)


def scan_of(data):
    """the bytes between the SOS header and EOI of a file"""
    rc, sc, _ = J.scan(data)
    assert rc == J.MDJPEG_OK
    return data[int(sc.scan_begin):int(sc.scan_end)]


def zigzag_blocks(data):
    """every block of Pillow's file in zig-zag order, per component, read out of the file by libmdjpeg.so's decoder"""
    rc, header, coef = J.decode(data)
    assert rc == J.MDJPEG_OK, header.reason
    return [p.reshape(-1, 64)[:, ZIGZAG] for p in header.planes(coef)]


def has_zrl(blocks):
    """a run of 16 or more zeros in front of a non-zero AC coefficient"""
    for b in blocks:
        nz = b[:, 1:] != 0
        for row in nz[nz.any(axis=1)]:
            idx = np.flatnonzero(row)
            if (np.diff(np.concatenate([[-1], idx])) > 16).any():
                return True
    return False


def test_the_case_matrix_is_complete():
    assert set(EXTRA_SIZES) <= set(ALL_SIZES) and set(SIZES) <= set(ALL_SIZES) and len(CONTENTS) >= 13
    assert QUALITIES == [1, 50, 75, 95, 100]


@pytest.mark.parametrize('size', ALL_SIZES, ids=lambda s: '{}x{}'.format(*s))
@pytest.mark.parametrize('quality', QUALITIES)
def test_host_model_and_header_equal_pillow(quality, size):
    w, h = size
    images = [make_content(kind, w, h, seed=quality) for kind in CONTENTS]
    want = [pillow_file(rgb, quality) for rgb in images]
    coefs = [coefficients(rgb, quality) for rgb in images]
    for chunk in chunks_for(w, h):
        rc, scans, needed, _ = J.encode_subsequences(coefs, [size] * len(coefs), chunk)
        assert rc == J.MDJPEG_OK
        assert needed == sum(len(s) for s in scans) and needed <= len(coefs) * J.encode_bound(w, h)
        for kind, scan, file in zip(CONTENTS, scans, want):
            assert scan == scan_of(file), '{} at chunk {}: the scans differ'.format(kind, chunk)
            assert J.jfif_file(w, h, quality, scan) == file, '{} at chunk {}: the files differ'.format(kind, chunk)


def test_matrix_holds_zrl_large_dc_and_empty_chroma():
    """what the matrix has to contain, read out of Pillow's own bytes"""
    noise = zigzag_blocks(pillow_file(make_content('noise', 100, 75, seed=50), 50))
    assert has_zrl(noise), 'no ZRL symbol in noise at quality 50'
    white = zigzag_blocks(pillow_file(make_content('white', 16, 16, seed=100), 100))
    assert abs(int(white[0][0, 0])) >= 512, 'DC category below 10'
    for c in (1, 2):
        assert not white[c].any(), 'chroma of a white image is not all EOB'


def test_mixed_sizes_in_one_call_and_steps_of_the_dc():
    """crops of different sizes behind each other (segment boundaries of both prefix sums), and DC differences of category 11"""
    steps = np.zeros((16, 64, 3), np.uint8)
    steps[:, 8:16] = 255
    steps[:, 32:] = 255
    data = pillow_file(steps, 100)
    y = zigzag_blocks(data)[0][:, 0].astype(int)
    assert np.abs(np.diff(y)).max() >= 1024
    cases = [(steps, 100)] + [(make_content(k, w, h, seed=3), 100) for k, (w, h) in
                              zip(['noise', 'black', 'checkerboard', 'noise', 'gradient', 'noise'],
                                  [(1, 1), (33, 15), (17, 17), (100, 75), (7, 9), (16, 16)])]
    coefs = [coefficients(rgb, q) for rgb, q in cases]
    sizes = [(rgb.shape[1], rgb.shape[0]) for rgb, _ in cases]
    for chunk in (1, 2, 3, 5, 64, 4096):
        rc, scans, _, _ = J.encode_subsequences(coefs, sizes, chunk)
        assert rc == J.MDJPEG_OK
        for (rgb, q), scan, size in zip(cases, scans, sizes):
            assert J.jfif_file(size[0], size[1], q, scan) == pillow_file(rgb, q)


def _file_ending_in_a_stuffed_ff():
    """seeded search: a Pillow file whose last scan byte is FF, so that the file ends FF 00 FF D9"""
    for seed in range(20000):
        rgb = np.random.default_rng(seed).integers(0, 256, (8, 8, 3), dtype=np.uint8)
        data = pillow_file(rgb, 95)
        if data.endswith(b'\xff\x00\xff\xd9'):
            return seed, rgb, data
    raise AssertionError('no file ending in a stuffed FF among 20000 seeds')


def test_last_byte_stuffed():
    seed, rgb, data = _file_ending_in_a_stuffed_ff()
    print('seed', seed)
    assert data[-4:] == b'\xff\x00\xff\xd9'
    for chunk in (1, 2, 3, 64):
        rc, scans, _, _ = J.encode_subsequences([coefficients(rgb, 95)], [(8, 8)], chunk)
        assert rc == J.MDJPEG_OK and scans[0].endswith(b'\xff\x00')
        assert J.jfif_file(8, 8, 95, scans[0]) == data


def test_capacity_one_byte_short():
    rgb = make_content('noise', 33, 17, seed=5)
    coef = coefficients(rgb, 95)
    rc, scans, needed, _ = J.encode_subsequences([coef], [(33, 17)], 3)
    assert rc == J.MDJPEG_OK and needed == len(scans[0])
    rc, none, needed2, buf = J.encode_subsequences([coef], [(33, 17)], 3, capacity=needed - 1)     # (the wrapper checks the guard bytes)
    assert rc == J.MDJPEG_ECAPACITY and none is None and needed2 == needed
    assert buf.tobytes() == scans[0][:-1]
    rc, again, _, _ = J.encode_subsequences([coef], [(33, 17)], 3, capacity=needed2)
    assert rc == J.MDJPEG_OK and again == scans


def test_bad_arguments():
    coef = coefficients(make_content('noise', 8, 8), 95)
    assert J.encode_subsequences([coef], [(8, 8)], 0)[0] == J.MDJPEG_EINVAL
    assert J.encode_subsequences([coef], [(0, 8)], 64)[0] == J.MDJPEG_EINVAL
    assert J.encode_bound(0, 5) == -1 and J.encode_bound(1, 1) == 8 * 313
    with pytest.raises(ValueError):
        J.jfif_file(0, 1, 95, b'')
    with pytest.raises(ValueError, match='1 to 100'):
        J.jfif_file(8, 8, 0, b'')
    bad = coef.copy()
    bad[1] = 2000                                        # an AC coefficient of category 11
    assert J.encode_subsequences([bad], [(8, 8)], 64)[0] == J.MDJPEG_ECORRUPT


def test_host_model_under_sanitizers(tmp_path):
    """the encoder's host model, jpeg_encode_host.cpp, in the AddressSanitizer + UBSan build (`make asan-jpeg`): its program,
    host_asan_main.cpp, encodes every 4:2:0 file it decoded, at three chunk sizes, into buffers of exactly the size the call asked for"""
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
    _, stuffed, _ = _file_ending_in_a_stuffed_ff()
    for i, (rgb, q) in enumerate([(stuffed, 95), (make_content('noise', 1, 1), 100), (make_content('noise', 33, 15), 100),
                                  (make_content('checkerboard', 100, 75), 1), (make_content('noise', 333, 257), 75)]):
        p = str(tmp_path / '{}.jpg'.format(i))
        Image.fromarray(rgb).save(p, quality=q)
        files.append(p)
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(': rc 0') == len(files)
