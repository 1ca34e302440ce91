"""
The host side of GPU entropy decoding, without a GPU: mdjpeg_scan (the descriptor a decoder that starts anywhere needs) and
mdjpeg_decode_subsequences, the host model that runs the kernels' own per-subsequence decoder (csrc/jpeg_subseq.h) as loops
over lanes.  The yardstick is mdjpeg_decode; every comparison is equality.  All of these fail on a tree without the
feature (no symbol).
"""

import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import jpeg_fixtures as JF
from conftest import REPO
from test_jpeg_cpu import _damaged_variants

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (200, 150)]
SUBSEQ_BITS = (64, 128, 1024, 1 << 24)          # the last one is longer than any scan here: one lane per segment


@pytest.fixture(scope='module')
def J():
    return JF.ensure_libmdjpeg()


def _matrix(tmp_path):
    """(label, bytes) over sampling x quality x optimised tables x restart x size"""
    p = str(tmp_path / 'm.jpg')
    for sampling, q, opt, rst, (w, h) in itertools.product(JF.SAMPLINGS, (75, 95), (False, True), JF.RESTARTS, SIZES):
        kind = JF.CONTENTS[(w + h + q) % 3]
        JF.write_jpeg(p, JF.content(kind, w, h), sampling, q, opt, rst)
        yield (sampling, q, opt, rst, w, h, kind), open(p, 'rb').read()


def _info_fields(info):
    out = {}
    for name, _ in type(info)._fields_:
        v = getattr(info, name)
        out[name] = bytes(v) if name == 'reason' else np.ctypeslib.as_array(v).tolist() if hasattr(v, '_length_') else v
    return out


def test_descriptor_equals_the_decoders_view(J, tmp_path):
    """mdjpeg_scan's info is mdjpeg_parse's, the segment offsets sit behind the restart markers, the tables are the file's"""
    import ctypes as C
    n_rst = 0
    for label, data in _matrix(tmp_path):
        rc, sc, seg = J.scan(data)
        assert rc == J.MDJPEG_OK, (label, sc.info.reason)
        info = J.mdjpeg_info()
        assert J.load().mdjpeg_parse(np.frombuffer(data, np.uint8).ctypes.data, len(data), C.byref(info)) == 0
        assert _info_fields(sc.info) == _info_fields(info), label
        a, b = JF.scan_range(data)
        assert (sc.scan_begin, sc.scan_end) == (a, b), label
        mcus = info.mcus_x * info.mcus_y
        want = -(-mcus // info.restart_interval) if info.restart_interval else 1
        assert sc.n_segments == want, label
        assert seg[0] == 0
        for k in range(1, sc.n_segments):
            at = a + int(seg[k])
            assert data[at - 2] == 0xFF and data[at - 1] == 0xD0 + (k - 1) % 8, (label, k)
            n_rst += 1
        # no marker inside a segment: every FF in it is followed by 00
        ends = [a + int(seg[k]) - 2 for k in range(1, sc.n_segments)] + [b]
        for k, e in enumerate(ends):
            body = data[a + int(seg[k]):e]
            assert all(body[i + 1:i + 2] == b'\x00' for i in range(len(body)) if body[i] == 0xFF), (label, k)
        # the tables are those of the file's DHT segments
        assert 2 <= sc.n_tables <= (2 if info.components == 1 else 4), label
        for t in range(sc.n_tables):
            counts = bytes(sc.huff_counts[t])
            total = sum(counts)
            assert counts + bytes(sc.huff_vals[t])[:total] in data[:a], label
    assert n_rst > 1000


def test_host_model_equals_mdjpeg_decode(J, tmp_path):
    n = 0
    for label, data in _matrix(tmp_path):
        rc0, h0, c0 = J.decode(data)
        assert rc0 == J.MDJPEG_OK
        for bits in SUBSEQ_BITS:
            rc1, h1, c1 = J.decode_subsequences(data, bits)
            assert rc1 == rc0, (label, bits, h1.reason)
            np.testing.assert_array_equal(c1, c0, err_msg=str((label, bits)))
            n += 1
    assert n == 4 * 2 * 2 * 3 * 6 * 4
    rc, _, _ = J.decode_subsequences(data, 63, out=np.empty(c0.size, np.int16))
    assert rc == J.MDJPEG_EINVAL
    # not a multiple of 8; longer than a lane's 16-bit block count allows while the segment still needs several lanes
    big = open(JF.write_jpeg(str(tmp_path / 'big.jpg'), JF.content('noise', 200, 150), '444', 95), 'rb').read()
    for bits in (100, 65536 + 8):
        assert J.decode_subsequences(big, bits)[0] == J.MDJPEG_EINVAL, bits


def stuffed_file(tmp_path, sampling='420', restart=None, size=(96, 80)):
    """high-quality noise: the scan holds FF 00 pairs"""
    p = JF.write_jpeg(str(tmp_path / 'stuffed.jpg'), JF.content('noise', *size), sampling, 98, False, restart)
    return open(p, 'rb').read()


def test_stuffed_bytes_on_subsequence_boundaries(J, tmp_path):
    """64-bit subsequences over a scan with stuffed bytes: boundaries fall on the 00 of an FF 00 pair and a lane's end has
    to be carried over several neighbours"""
    for sampling, rst in [('420', None), ('444', 'rows'), ('gray', None), ('422', 'blocks')]:
        data = stuffed_file(tmp_path, sampling, rst)
        a, b = JF.scan_range(data)
        pairs = [i for i in range(a, b - 1) if data[i] == 0xFF and data[i + 1] == 0]
        assert len(pairs) >= 8, 'the fixture holds no stuffed bytes'
        if rst is None:
            assert any((i + 1 - a) % 8 == 0 for i in pairs), 'no stuffing byte begins a 64-bit subsequence'
        rc0, _, c0 = J.decode(data)
        assert rc0 == 0
        for bits in (64, 72, 128, 1000):                    # (multiples of 8: a subsequence begins on a byte)
            rc1, h1, c1 = J.decode_subsequences(data, bits)
            assert rc1 == 0, (sampling, rst, bits, h1.reason)
            np.testing.assert_array_equal(c1, c0)


def test_damaged_files_accept_exactly_what_mdjpeg_decode_accepts(J, tmp_path):
    """truncations, flipped bytes in the scan, a removed and a renumbered restart marker, trailing bytes: the same return
    code as mdjpeg_decode, the same coefficients where that is OK, nothing written behind the buffer"""
    variants = _damaged_variants(tmp_path)
    good = stuffed_file(tmp_path)
    a, b = JF.scan_range(good)
    variants += [('trailing_in_scan', good[:b] + b'\x12\x34' + good[b:]), ('trailing_zero', good[:b] + b'\x00' + good[b:]),
                 ('trailing_after_eoi', good + b'tail'), ('no_eoi', good[:b]), ('padding_byte', good[:b] + b'\x7f' + good[b:])]
    n_ok = n_err = 0
    for name, data in variants:
        hd = J.parse(data)
        if not hd.supported:
            rc, sc, _ = J.scan(data)
            assert rc == J.MDJPEG_EUNSUPPORTED, name
            continue
        rc0, h0, c0 = J.decode(data)
        rcs, sc, _ = J.scan(data)
        assert rcs in (J.MDJPEG_OK, J.MDJPEG_ECORRUPT), name
        if rcs == J.MDJPEG_ECORRUPT:
            assert rc0 == J.MDJPEG_ECORRUPT, name          # what the marker search refuses, the decoder refuses
        for bits in (64, 128, 1024):
            buf = np.full(hd.coef_count + 4096, 0x5A5A, dtype=np.int16)
            rc1, h1, _ = J.decode_subsequences(data, bits, out=buf[:hd.coef_count])
            assert (buf[hd.coef_count:] == 0x5A5A).all(), name
            assert rc1 == rc0, (name, bits, rc0, h0.reason, rc1, h1.reason)
            if rc0 == 0:
                np.testing.assert_array_equal(buf[:hd.coef_count], c0, err_msg=name)
        n_ok += rc0 == 0
        n_err += rc0 != 0
    print('damaged files: {} refused by both, {} decoded alike'.format(n_err, n_ok))
    assert n_err >= 40 and n_ok >= 1


def test_host_model_under_sanitizers(J, tmp_path):
    """the damaged files through the AddressSanitizer + UBSan build: its main runs mdjpeg_scan and the host model at 64 and
    1024 bits into buffers of exact size, next to mdjpeg_decode, and ends with an error when their codes differ"""
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'jpeg_entropy_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-jpeg', 'ASAN_OUT=' + exe])
    assert b'mdjpeg_decode_subsequences' in open(exe, 'rb').read()
    files = []
    for name, data in _damaged_variants(tmp_path) + [('stuffed', stuffed_file(tmp_path))]:
        p = str(tmp_path / (name + '.jpg'))
        with open(p, 'wb') as f:
            f.write(data)
        files.append(p)
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(': rc ') == len(files)
    assert 'stuffed.jpg: rc 0' in r.stdout


def test_loader_scan_mode_mixed_folder(J, tmp_path):
    """ProcessLoader(decode='scan') yields 'scan' where decode='coefficients' yields 'jpeg' and otherwise the same kinds,
    shapes and metadata -- except for a file whose damage only symbol decoding sees, which now arrives as 'scan'; a scan
    slot holds the descriptor and the file's bytes, from which the host model rebuilds mdjpeg_decode's coefficients"""
    from PIL import Image
    from megadetector_amd import feed
    from megadetector_amd.jpeg_host import ScanImage
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
    (tmp_path / 'f_broken.jpg').write_bytes(b'this is not an image')
    files['f_broken.jpg'] = str(tmp_path / 'f_broken.jpg')
    good = open(files['a420.jpg'], 'rb').read()
    a, b = JF.scan_range(good)
    (tmp_path / 'h_trunc.jpg').write_bytes(good[:a + (b - a) // 2])
    files['h_trunc.jpg'] = str(tmp_path / 'h_trunc.jpg')
    flipped = bytearray(good)
    flipped[a + (b - a) // 3] ^= 0x55                      # no marker appears or disappears: only the symbols are wrong
    assert J.scan(bytes(flipped))[0] == 0 and J.decode(bytes(flipped))[0] == J.MDJPEG_ECORRUPT
    (tmp_path / 'i_flip.jpg').write_bytes(bytes(flipped))
    files['i_flip.jpg'] = str(tmp_path / 'i_flip.jpg')
    paths = [files[k] for k in sorted(files)]
    slot_bytes = 400 * 1024

    def run(decode):
        loader = feed.ProcessLoader(paths, 2, 6, slot_bytes, want_meta=True, decode=decode)
        got = {}
        try:
            for kind, f, payload, shape, meta in loader:
                extra = None
                if kind == 'scan':
                    si = feed.scan_image(loader.ring, payload, shape)
                    assert isinstance(si, ScanImage) and si.shape == tuple(shape)
                    data = open(f, 'rb').read()
                    assert bytes(si.file) == data
                    rc, sc, seg = J.scan(data)
                    assert bytes(si.desc) == bytes(sc) and list(si.seg_offsets) == list(seg[:sc.n_segments])
                    assert bytes(si.scan_bytes) == data[sc.scan_begin:sc.scan_end]
                    extra = si.rotation
                if kind in ('slot', 'jpeg', 'scan'):
                    loader.ring.release(payload)
                got[os.path.basename(f)] = (kind, None if shape is None else tuple(shape), meta, extra)
        finally:
            loader.close()
        return got

    coef = run('coefficients')
    scan = run('scan')
    assert sorted(coef) == sorted(scan) == sorted(files)
    want = {k: {'jpeg': 'scan'}.get(v[0], v[0]) for k, v in coef.items()}
    assert coef['i_flip.jpg'][0] in ('slot', 'fail') and coef['a420.jpg'][0] == 'jpeg' and coef['g_big.jpg'][0] == 'slot'
    want['i_flip.jpg'] = 'scan'
    assert {k: v[0] for k, v in scan.items()} == want
    for k in files:
        if k != 'i_flip.jpg':
            assert scan[k][1:3] == coef[k][1:3], k
    assert scan['b422_rot.jpg'][3] == feed.EXIF_IMAGE_ROTATIONS[6] and scan['b422_rot.jpg'][1] == (80, 56, 3)
    with pytest.raises(ValueError, match='decode'):
        feed.ProcessLoader(paths, 1, 2, slot_bytes, decode='huffman')


def test_scan_loader_stays_off_the_gpu(J, tmp_path):
    """a fresh process that scans a file and fills a slot maps neither libmdhip.so nor the HIP / HSA runtime"""
    p = JF.write_jpeg(str(tmp_path / 'x.jpg'), JF.content('natural', 64, 48), '420', 80, restart='rows')      # 3 MCU rows: 3 segments
    code = (
        'import sys, json\n'
        'import numpy as np\n'
        'sys.path.insert(0, {!r})\n'
        'from megadetector_amd import jpeg_host, feed\n'
        'slot = np.zeros(1 << 16, np.uint8)\n'
        'rc = jpeg_host.scan_into_slot(open({!r}, "rb").read(), slot, 0)\n'
        'im = jpeg_host.ScanImage.from_slot(slot)\n'
        'maps = open("/proc/self/maps").read()\n'
        'print(json.dumps(dict(rc=rc, n=int(im.desc.n_segments), hip="amdhip" in maps, hsa="hsa-runtime" in maps,\n'
        '                      torch="torch" in sys.modules, mdjpeg="libmdjpeg" in maps, mdhip="libmdhip" in maps)))\n'
    ).format(REPO, p)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == dict(rc=0, n=3, hip=False, hsa=False, torch=False, mdjpeg=True, mdhip=False), got


class _StubDetector:
    """a detector without a GPU that takes scans: decode_scans follows HIPDetector's contract with mdjpeg_decode as the judge"""

    def __init__(self, J):
        self.J = J
        self.jpeg_images_reconstructed = self.jpeg_images_entropy_decoded = self.jpeg_entropy_fallbacks = 0
        self.seen = []

    def decode_scans(self, images):
        import io
        from megadetector_amd.feed import load_image
        from megadetector_amd.jpeg_host import ScanFailure, ScanImage
        out = []
        for im in images:
            if not isinstance(im, ScanImage):
                out.append(im)
                continue
            data = im.file.tobytes()
            if self.J.decode(data)[0] == 0:
                self.jpeg_images_entropy_decoded += 1
            else:
                self.jpeg_entropy_fallbacks += 1
            try:
                out.append(np.asarray(load_image(io.BytesIO(data))))
            except Exception as e:
                out.append(ScanFailure(e))
        return out

    def generate_detections_one_batch(self, images, names, **kw):
        self.seen += [(n, np.asarray(im).shape, int(np.asarray(im).sum())) for n, im in zip(names, images)]
        return [{'file': n, 'detections': [], 'max_detection_conf': 0.0} for n in names]

    def generate_detections_one_image(self, image, name, **kw):
        return self.generate_detections_one_batch([image], [name])[0]


@pytest.mark.parametrize('batch_size', [1, 3])
def test_driver_entropy_mode_with_a_stub_detector(J, tmp_path, batch_size):
    """run_detector_batch's shared-ring loop with gpu_jpeg='entropy': every file reaches the detector with the pixels of the
    plain run, a flagged file PIL refuses is reported as the loader reports it, and last_feed_counts gains 'scan' only here"""
    import warnings
    from PIL import Image
    from megadetector_amd import run_detector_batch as RDB
    arr = JF.content('natural', 80, 56)
    names = [JF.write_jpeg(str(tmp_path / 'a.jpg'), arr, '420', 80), JF.write_jpeg(str(tmp_path / 'b.jpg'), arr, '422', 90, orientation=6),
             JF.write_jpeg(str(tmp_path / 'c.jpg'), arr, 'gray', 75, restart='rows'),
             JF.write_jpeg(str(tmp_path / 'd_prog.jpg'), arr, '420', 80, progressive=True)]
    Image.fromarray(arr).save(str(tmp_path / 'e.png'))
    names.append(str(tmp_path / 'e.png'))
    (tmp_path / 'f.jpg').write_bytes(b'junk')
    names.append(str(tmp_path / 'f.jpg'))
    good = open(names[0], 'rb').read()
    a, b = JF.scan_range(good)
    n_flip = 0
    for k in range(3, 8):
        d = bytearray(good)
        d[a + (b - a) * k // 10] ^= 0x55
        if J.scan(bytes(d))[0] == 0 and J.decode(bytes(d))[0] == J.MDJPEG_ECORRUPT:
            (tmp_path / 'g_flip{}.jpg'.format(k)).write_bytes(bytes(d))
            names.append(str(tmp_path / 'g_flip{}.jpg'.format(k)))
            n_flip += 1
    assert n_flip >= 2

    def run(gpu_jpeg):
        det = _StubDetector(J)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = RDB.load_and_run_detector_batch('stub', names, quiet=True, detector=det, batch_size=batch_size, use_image_queue=True,
                                                  use_threads_for_queue=False, loader_workers=2, include_image_size=True,
                                                  gpu_jpeg=gpu_jpeg)
        return sorted(res, key=lambda r: r['file']), sorted(det.seen), det, dict(RDB.last_feed_counts)

    plain, seen0, _, c0 = run(False)
    fast, seen1, det, c1 = run('entropy')
    assert fast == plain and seen1 == seen0
    assert set(c0) == {'jpeg', 'slot', 'array', 'fail'}
    assert c1 == {'jpeg': 0, 'scan': 3 + n_flip, 'slot': 2, 'array': 0, 'fail': 1}
    assert (det.jpeg_images_entropy_decoded, det.jpeg_entropy_fallbacks) == (3, n_flip)
    assert sum(1 for r in plain if 'failure' in r) == c0['fail'] >= 1
