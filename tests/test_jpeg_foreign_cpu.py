"""
The host half of the GPU JPEG feed on files Pillow's encoder never writes (tests/jpeg_foreign.py): foreign anatomy around
the coefficients of Pillow files, and blocks no 8-bit image gives.  The contracts are those of test_jpeg_cpu.py and
test_jpeg_entropy_cpu.py -- mdjpeg_decode returns the file's coefficients, the host model of the GPU decoder returns
mdjpeg_decode's answer, jpeg_ref (what the kernels restate) gives Pillow's pixels, and a file that is not taken is refused
with a reason and left to Pillow -- and so is the tolerance: zero.
"""

import io
import warnings

import numpy as np
import pytest

import jpeg_fixtures as JF
import jpeg_foreign as F
import jpeg_ref as R

GUARD = 4096
SUBSEQ_BITS = (64, 128, 1024)


@pytest.fixture(scope='module')
def J():
    return JF.ensure_libmdjpeg()


@pytest.fixture(scope='module')
def corpus(J, tmp_path_factory):
    return F.structural_corpus(J, tmp_path_factory.mktemp('foreign'))


def _pil(data):
    """Pillow's own pixels, nothing of the project in between; None when Pillow refuses the bytes"""
    from PIL import Image
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
    except Exception:
        return None


def _load(data):
    """np.asarray(load_image(file)), or None when it raises"""
    from megadetector_amd.feed import load_image
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return np.asarray(load_image(io.BytesIO(data)))
    except Exception:
        return None


def _one_answer(J, name, data, want=None):
    """mdjpeg_decode, mdjpeg_scan and the host model at 64 / 128 / 1024 bits give ONE answer, and write nothing behind the
    planes.  Returns (rc, header, planes) of mdjpeg_decode; with `want`, asserts that the file is accepted with these planes."""
    hd = J.parse(data)
    assert hd.supported and hd.rc == 0, (name, hd.reason)
    buf = np.full(hd.coef_count + GUARD, 0x5A5A, dtype=np.int16)
    rc0, h0, _ = J.decode(data, out=buf[:hd.coef_count])
    assert (buf[hd.coef_count:] == 0x5A5A).all(), name
    c0 = buf[:hd.coef_count].copy()
    assert rc0 in (J.MDJPEG_OK, J.MDJPEG_ECORRUPT), (name, rc0)
    rcs, sc, _ = J.scan(data)
    assert rcs in (J.MDJPEG_OK, J.MDJPEG_ECORRUPT), name
    if rcs != 0:
        assert rc0 == J.MDJPEG_ECORRUPT, name                  # what the marker search refuses, the decoder refuses
    for bits in SUBSEQ_BITS:
        buf[:] = 0x5A5A
        rc1, h1, _ = J.decode_subsequences(data, bits, out=buf[:hd.coef_count])
        assert (buf[hd.coef_count:] == 0x5A5A).all(), (name, bits)
        assert rc1 == rc0, (name, bits, rc0, h0.reason, rc1, h1.reason)
        if rc0 == 0:
            np.testing.assert_array_equal(buf[:hd.coef_count], c0, err_msg='{} at {} bits'.format(name, bits))
    if want is not None:
        assert rc0 == 0, (name, h0.reason)
        np.testing.assert_array_equal(c0, want, err_msg=name)
    return rc0, h0, c0


# ---- the serialiser, judged by Pillow alone --------------------------------------------------------------------------------
def test_serialised_files_decode_in_pillow_to_the_source_files_pixels(J, tmp_path):
    """a foreign file holds the coefficients and tables of the Pillow file it was made from, so Pillow must decode both to
    the same pixels, whatever the anatomy; no project code takes part (foreign_file has walked the segments already)"""
    n = 0
    for sampling, (w, h) in F.BASES:
        p = JF.write_jpeg(str(tmp_path / 'base.jpg'), JF.content('noise', w, h), sampling, 95)
        src = open(p, 'rb').read()
        rc, header, coef = J.decode(src)
        assert rc == 0
        want = _pil(src)
        for name, knobs in F.variants(header):
            np.testing.assert_array_equal(_pil(F.foreign_file(header, coef, **knobs)), want, err_msg=name)
            n += 1
    assert n == len(F.BASES) * 28


def test_huffman_shapes():
    """flat(L): every code L bits long (longer where the symbols need it), ladder: every length it claims; canonical codes
    that are a prefix code with the all-ones code unused"""
    freq = {s: 1000 - s for s in range(162)}
    for shape, want in [(('flat', 1), {8}), (('flat', 9), {9}), (('flat', 16), {16}), ('ladder', {1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13, 16})]:
        counts, syms, codes = F.huffman_table(freq, shape)
        assert {ln for _, ln in codes.values()} == want and sum(counts) == 162
        words = sorted(format(c, '0{}b'.format(ln)) for c, ln in codes.values())
        assert all(not b.startswith(a) for a, b in zip(words, words[1:])), shape
        assert all('0' in w for w in words), shape
    assert [ln for _, ln in F.huffman_table({s: 12 - s for s in range(12)}, 'ladder')[2].values()] == list(range(1, 13))
    assert set(F._ladder_lengths(60)) >= {9, 13, 14, 15, 16}
    assert F.huffman_table(freq, 'ladder')[1][:3] == [0, 1, 2]            # the most frequent symbol takes the shortest code


# ---- structure -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('base', range(len(F.BASES)), ids=['{}_{}x{}'.format(s, w, h) for s, (w, h) in F.BASES])
def test_structural_corpus(J, corpus, base):
    """every knob alone and three camera-like combinations: parse, scan and decode accept the file, decode and the host model
    return the serialised planes, the descriptor holds the file's tables and segments, jpeg_ref gives load_image's pixels"""
    from megadetector_amd import feed
    sampling, (w, h) = F.BASES[base]
    mine = [e for e in corpus if e[0].startswith('{}_{}x{}_'.format(sampling, w, h))]
    assert len(mine) == 28
    for name, data, header, coef, knobs in mine:
        k = dict(F.PLAIN, **knobs)
        rc, hd, got = _one_answer(J, name, data, want=coef)
        assert (hd.width, hd.height, hd.components, hd.h_samp, hd.v_samp) == (w, h, header.components, header.h_samp, header.v_samp), name
        assert hd.restart_interval == k['dri'] and hd.quant.tolist() == header.quant.tolist(), name
        # the descriptor
        rcs, sc, seg = J.scan(data)
        assert rcs == 0, (name, sc.info.reason)
        file = F.walk(data)
        assert (sc.scan_begin, sc.scan_end) == (file['scan'], file['eoi']), name
        nc = header.components
        slots = [c if k['huff_per_component'] else min(c, 1) for c in range(nc)]
        assert sc.n_tables == 2 * len(set(slots)) and (not k['huff_per_component'] or nc == 1 or sc.n_tables == 6), name
        seen = []
        for c in range(nc):
            for cls, t in ((0, sc.dc_table[c]), (1, sc.ac_table[c])):
                counts = bytes(sc.huff_counts[t])
                assert counts + bytes(sc.huff_vals[t])[:sum(counts)] == file['huffman'][(cls, k['table_ids'][slots[c]])], (name, c, cls)
                if t not in seen:
                    seen.append(t)
        assert seen == list(range(sc.n_tables)), (name, 'tables are numbered in order of first use')
        mcus = hd.mcus_x * hd.mcus_y
        assert sc.n_segments == (-(-mcus // k['dri']) if k['dri'] else 1), name
        assert seg[0] == 0
        for i in range(1, sc.n_segments):
            at = file['scan'] + int(seg[i])
            assert data[at - 2] == 0xFF and data[at - 1] == 0xD0 + (i - 1) % 8, (name, i)
        # the pixels
        _, rotation = feed.open_for_coefficients(io.BytesIO(data))
        turned = {F.exif_orientation(6): 270, F.exif_orientation(8): 90}.get(k['exif'], 0)
        assert rotation == (0 if nc == 1 else turned), name       # (load_image never turns a grayscale file)
        want = _load(data)
        assert want is not None, name
        np.testing.assert_array_equal(R.jpeg_ref(hd, got, rotation), want, err_msg=name)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _patch_sof(data, offset, value):
    d = bytearray(data)
    k = d.index(b'\xff\xc0')
    d[k + offset] = value
    return bytes(d)


def _refused_files(J):
    """(name, bytes, key word of the reason)"""
    rng = np.random.default_rng(5)
    q = np.full(64, 3)

    def noise(header):
        coef = np.zeros(header.coef_count, np.int16)
        for p in header.planes(coef):
            p[..., :6] = rng.integers(-40, 41, p.shape[:2] + (6,))
        return coef

    h444 = F.Header(24, 16, '444', q)
    c444 = noise(h444)
    out = [('adobe0', F.foreign_file(h444, c444, jfif=False, adobe=0), 'Adobe'),
           ('adobe0_jfif', F.foreign_file(h444, c444, adobe=0), 'Adobe'),
           ('idsRGB_nojfif', F.foreign_file(h444, c444, jfif=False, ids=(82, 71, 66)), 'R, G, B')]
    for sampling in ('440', '411'):                            # real files of these samplings: Pillow decodes them
        hd = F.Header(40, 24, sampling, q)
        out.append((sampling, F.foreign_file(hd, noise(hd)), 'sampling'))
    plain = F.foreign_file(h444, c444)
    out.append(('440_header_only', _patch_sof(plain, 11, 0x12), 'sampling'))
    out.append(('411_header_only', _patch_sof(plain, 11, 0x41), 'sampling'))
    out.append(('12bit', _patch_sof(plain, 4, 12), 'precision'))
    k = plain.index(b'\xff\xda')
    assert plain[k + 2:k + 5] == b'\x00\x0c\x03'
    out.append(('one_of_three', plain[:k] + b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00' + plain[k + 14:], 'several scans'))
    d = bytearray(plain)
    d[k + 8] = 0x22                                            # Cb names the tables 2 / 2; 0 and 1 are defined
    out.append(('undefined_table', bytes(d), 'not defined'))
    d = bytearray(plain)
    k = d.index(b'\xff\xc4')                                   # the first DHT segment: the luma DC table, 12 codes of 4 bits
    assert d[k + 4] == 0x00 and list(d[k + 5:k + 21]) == [0, 0, 0, 12] + [0] * 12
    d[k + 5:k + 9] = bytes((0, 12, 0, 0))                      # ... now 12 codes of 2 bits
    out.append(('not_a_prefix_code', bytes(d), 'prefix'))
    return out


def test_refusals(J):
    """each is refused with its reason by parse, decode, scan and the host model alike, and goes to Pillow: load_image
    opens exactly what Pillow opens, to Pillow's pixels"""
    files = _refused_files(J)
    assert len(files) == 11
    n_open = 0
    for name, data, word in files:
        hd = J.parse(data)
        assert not hd.supported and hd.rc == J.MDJPEG_EUNSUPPORTED and word in hd.reason, (name, hd.reason)
        rc, h2, _ = J.decode(data)
        assert rc == J.MDJPEG_EUNSUPPORTED and h2.reason == hd.reason, name
        rc, sc, _ = J.scan(data)
        assert rc == J.MDJPEG_EUNSUPPORTED and word in sc.info.reason.decode(), name
        assert J.decode_subsequences(data, 64)[0] == J.MDJPEG_EUNSUPPORTED, name
        pil, got = _pil(data), _load(data)
        assert (pil is None) == (got is None), name
        if pil is not None:
            np.testing.assert_array_equal(got, pil, err_msg=name)
            n_open += 1
    assert n_open >= 5                                         # Adobe 0 (twice), R G B, the real 4:4:0 and 4:1:1 files


# ---- damage --------------------------------------------------------------------------------------------------------------
def damaged_foreign(corpus):
    """(name, bytes): the operations of test_jpeg_cpu._damaged_variants -- truncated at 25 / 50 / 99 % of the scan, one byte
    flipped inside the scan at 10 seeded positions, a removed and a renumbered restart marker -- on three foreign files:
    16-bit codes, one-MCU restart segments, and a camera-like combination"""
    out = []
    rng = np.random.default_rng(2025)
    by_name = {e[0]: e[1] for e in corpus}
    for tag in ('420_37x29_flat16', '422_40x24_dri1', 'gray_33x31_camera_b'):
        data = by_name[tag]
        file = F.walk(data)
        a, b = file['scan'], file['eoi']
        for pc in (25, 50, 99):
            out.append(('{}_trunc{}'.format(tag, pc), data[:a + (b - a) * pc // 100]))
        for pos in rng.integers(a, b, 10):
            d = bytearray(data)
            d[pos] ^= int(rng.integers(1, 256))
            out.append(('{}_flip{}'.format(tag, pos), bytes(d)))
        if file['dri']:
            k = data.index(b'\xff\xd0', a)
            out.append(('{}_norst'.format(tag), data[:k] + data[k + 2:]))
            k1 = data.index(b'\xff\xd1', a)
            out.append(('{}_rstseq'.format(tag), data[:k1 + 1] + b'\xd3' + data[k1 + 2:]))
    return out


def test_damaged_foreign_files_error_or_equal_pillow(J, corpus):
    """test_jpeg_cpu.test_damaged_files_error_or_equal_pillow and test_jpeg_entropy_cpu.test_damaged_files_accept_exactly_
    what_mdjpeg_decode_accepts on foreign anatomy: an error or Pillow's pixels, never different pixels; one answer from
    mdjpeg_decode and the host model; nothing written behind a buffer"""
    variants = damaged_foreign(corpus)
    assert len(variants) == 3 * 13 + 2 * 2
    n_err = n_ok = 0
    for name, data in variants:
        hd = J.parse(data)
        if not hd.supported:
            assert J.scan(data)[0] == J.MDJPEG_EUNSUPPORTED, name
            n_err += 1
            continue
        rc, h2, coef = _one_answer(J, name, data)
        if rc != 0:
            assert rc == J.MDJPEG_ECORRUPT and h2.reason, (name, rc)
            n_err += 1
            continue
        want = _load(data)
        assert want is not None, '{}: decoded cleanly here, PIL refuses the file'.format(name)
        np.testing.assert_array_equal(R.jpeg_ref(h2, coef), want, err_msg=name)
        n_ok += 1
    print('damaged foreign files: {} refused, {} decoded to PIL\'s pixels'.format(n_err, n_ok))
    assert n_err >= 20


# ---- blocks no 8-bit image gives -----------------------------------------------------------------------------------------
def test_range_limit_probe(J):
    """ONE block states which range limit the installed Pillow applies behind its inverse DCT: a one-pixel spike of height
    700 (norm 700, inside every energy bound) leaves [-512, 511].  This project saturates (jpeg_ref.range_limit, the
    kernels' range_limit), as libjpeg-turbo's SIMD inverse DCT does; libjpeg's C code indexes a table with (x & 1023) and
    wraps around.  A Pillow whose libjpeg does the latter fails HERE, with this text, and not in a pixel comparison."""
    header = F.Header(8, 8, 'gray', np.ones(64))
    coef = np.zeros(64, np.int16)
    coef[:] = F.spike_block(700, 3, 3, 1)
    data = F.foreign_file(header, coef)
    rc, hd, got = J.decode(data)
    assert rc == 0 and np.array_equal(got, coef)
    plane = hd.planes(got)[0]
    saturated = R.idct_plane(plane, hd.quant[0])
    table = R.idct_plane(plane, hd.quant[0], R.range_limit_table)
    assert saturated[3, 3] == 255 and table[3, 3] < 64, 'the probe block does not tell the two rules apart'
    pil = _pil(data)[..., 0]
    assert not np.array_equal(pil, table), \
        'the installed Pillow limits post-IDCT samples with libjpeg\'s table (wrap-around outside [-512, 511]); this project saturates'
    np.testing.assert_array_equal(pil, saturated, err_msg='the installed Pillow neither saturates nor applies libjpeg\'s range-limit table')


@pytest.mark.parametrize('sampling', ['444', 'gray'])
def test_extreme_blocks_are_refused_or_equal_pillow(J, sampling):
    """spikes of +-400 .. 1028 and single coefficients that de-quantise to 1900 .. 2799 (F.extreme_family): refused, or
    Pillow's pixels; one answer from scan, decode and the host model.  So that refusing everything is no way out, every
    member whose exact real-valued inverse DCT (float64, computed here) stays inside [-500, 500] must be accepted."""
    family = [m for m in F.extreme_family() if m[0].startswith(sampling)]
    n_spikes = len(F.SPIKE_HEIGHTS) * 2 * len(F.SPIKE_POSITIONS) * len(F.SPIKE_TABLES)
    n_singles = len(F.SINGLES) * (len(F.SINGLE_INDICES) + (2 if sampling == '444' else 0))
    assert len(family) == n_spikes + n_singles
    n_refused = n_equal = n_must = n_beyond_512 = 0
    wrong = []
    for name, header, coef, block, q, knobs in family:
        data = F.foreign_file(header, coef, **knobs)
        rc, hd, got = _one_answer(J, name, data)
        peak = float(np.abs(F.exact_idct(block, np.full(64, q))).max())
        n_must += peak <= 500
        n_beyond_512 += peak > 512
        if rc != 0:
            assert peak > 500, '{}: refused ({}), but its samples stay within +-{:.1f}'.format(name, hd.reason, peak)
            n_refused += 1
            continue
        np.testing.assert_array_equal(got, coef, err_msg=name)
        pil = _pil(data)
        if np.array_equal(R.jpeg_ref(hd, got), pil):
            n_equal += 1
        else:
            wrong.append((name, int(np.abs(R.jpeg_ref(hd, got).astype(int) - pil).max())))
    print('extreme blocks, {}: {} files, {} refused, {} equal to Pillow, {} different; {} had to be accepted, {} leave [-512, 511]'.format(
        sampling, len(family), n_refused, n_equal, len(wrong), n_must, n_beyond_512))
    assert not wrong, '{} files decode to pixels that are not Pillow\'s (name, largest difference): {}'.format(len(wrong), wrong[:12])
    assert n_must >= 100 and n_beyond_512 >= 100


def test_blocks_beyond_the_energy_bound_are_refused_alike(J):
    """single coefficients that de-quantise to more than any energy bound allows: mdjpeg_decode and the host model refuse
    them with one code; mdjpeg_scan, which decodes no symbol, passes them"""
    family = F.extreme_family(singles=F.BEYOND, spikes=False)
    assert len(family) == len(F.BEYOND) * (7 + 5)
    for name, header, coef, block, q, knobs in family:
        data = F.foreign_file(header, coef, **knobs)
        rc, hd, _ = _one_answer(J, name, data)
        assert rc == J.MDJPEG_ECORRUPT and 'energy' in hd.reason, (name, rc, hd.reason)
        assert J.scan(data)[0] == 0, name


def test_extreme_images_of_8_bits_are_accepted(J, tmp_path):
    """checkerboard, one-pixel spikes, their inverse and one-pixel stripes, written by Pillow in 4:4:4 / 4:2:0 / grayscale at
    qualities 1 .. 100: genuine extremes are all accepted and equal Pillow (the range limit sees nothing beyond +-512 here)"""
    files = F.pillow_extremes(tmp_path)
    assert len(files) == 60
    for name, path in files:
        data = open(path, 'rb').read()
        rc, hd, coef = _one_answer(J, name, data)
        assert rc == 0, (name, hd.reason)
        np.testing.assert_array_equal(R.jpeg_ref(hd, coef), _pil(data), err_msg=name)
