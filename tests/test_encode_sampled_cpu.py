"""
The encoder with a chroma sampling and a pair of quantisation tables per crop, host side: the host model
mdjpeg_encode_subsequences_sampled (libmdjpeg.so, compiled from csrc/jpeg_encode.h like the kernels) and
jpeg_host.sampled_file against Pillow, byte for byte.

Seeded random windows whose right and bottom edges fall at every kind of position within an MCU of each layout, at 4:4:4,
4:2:2 and 4:2:0, with the tables of quality 50, 91 and 100 and one pair no quality gives; a flat and a saturated window per
layout (long zero runs, FF stuffing).  The coefficients are those of tests/jpeg_enc_sampled_ref.py; Pillow's side is
Image.save(qtables=..., subsampling=...) without `optimize`.  All sizes of a (sampling, pair) travel in ONE call, and the
whole matrix once more in one mixed call, at small stuffing chunks.
"""

import io

import numpy as np
import pytest
from PIL import Image

import jpeg_enc_ref as E
import jpeg_enc_sampled_ref as S
from megadetector_amd import jpeg_host as J

PAIRS = S.table_pairs()


def _encode(cases, chunk):
    coefs = [S.coefficients(rgb, s, *PAIRS[pair]) for _, rgb, s, pair in cases]
    sizes = [(rgb.shape[1], rgb.shape[0]) for _, rgb, _, _ in cases]
    samplings = [s for _, _, s, _ in cases]
    rc, scans, needed, _ = J.encode_subsequences(coefs, sizes, chunk, samplings=samplings)
    assert rc == J.MDJPEG_OK
    assert needed == sum(len(x) for x in scans)
    for (w, h), s, scan in zip(sizes, samplings, scans):
        assert len(scan) <= J.encode_bound_sampled(w, h, s), 'the bound is exceeded'
    return scans


def test_the_case_matrix_is_complete():
    cases = S.matrix()
    assert S.SIZES == [(1, 1), (8, 8), (9, 8), (16, 8), (17, 9), (15, 17), (33, 31), (70, 50)]
    assert sorted(PAIRS) == ['odd', 'q100', 'q50', 'q91'] and len(cases) == 8 * 3 * 4 + 6
    assert {(rgb.shape[1], rgb.shape[0], s, p) for _, rgb, s, p in cases} >= {(w, h, s, p) for w, h in S.SIZES for s in S.SAMPLINGS for p in PAIRS}
    # the non-standard pair is no quality's
    assert not any(all((a == b).all() for a, b in zip(PAIRS['odd'], J.quant_tables(q))) for q in range(1, 101))


@pytest.mark.parametrize('pair', sorted(PAIRS))
@pytest.mark.parametrize('sampling', S.SAMPLINGS)
def test_host_model_and_file_equal_pillow(sampling, pair):
    cases = [c for c in S.matrix() if c[2] == sampling and c[3] == pair]
    assert len(cases) >= len(S.SIZES)
    ql, qc = PAIRS[pair]
    for chunk in (1, 3, 64):
        for (name, rgb, _, _), scan in zip(cases, _encode(cases, chunk)):
            want = S.pillow_file(rgb, sampling, ql, qc)
            assert scan == S.scan_of(want), '{} at chunk {}: the scans differ'.format(name, chunk)
            assert J.sampled_file(rgb.shape[1], rgb.shape[0], ql, qc, sampling, scan) == want, '{}: the files differ'.format(name)


def test_the_whole_matrix_in_one_mixed_call():
    cases = S.matrix()
    for (name, rgb, s, pair), scan in zip(cases, _encode(cases, 2)):
        assert scan == S.scan_of(S.pillow_file(rgb, s, *PAIRS[pair])), name


def test_flat_and_saturated_windows_hold_zero_runs_and_stuffed_bytes():
    """what the two special windows are there for, read out of Pillow's own bytes"""
    for s in S.SAMPLINGS:
        flat = S.pillow_file(S.window(70, 50, 0, 'flat'), s, *PAIRS['q50'])
        rc, header, coef = J.decode(flat)
        assert rc == J.MDJPEG_OK and all(not p[..., 1:].any() for p in header.planes(coef)), 'a flat window has AC coefficients'
        assert b'\xff\x00' in S.scan_of(S.pillow_file(S.window(70, 50, 7 + s, 'saturated'), s, *PAIRS['q100'])), 'no stuffed FF'


def test_the_old_export_is_the_h2v2_case_of_the_new_one():
    cases = [c for c in S.matrix() if c[2] == 2]
    coefs = [S.coefficients(rgb, 2, *PAIRS[pair]) for _, rgb, _, pair in cases]
    sizes = [(rgb.shape[1], rgb.shape[0]) for _, rgb, _, _ in cases]
    for chunk in (1, 64):
        old = J.encode_subsequences(coefs, sizes, chunk)
        new = J.encode_subsequences(coefs, sizes, chunk, samplings=[2] * len(cases))
        assert old[0] == new[0] == J.MDJPEG_OK and old[1] == new[1] and old[2] == new[2]
    for w, h in sizes + [(65535, 65535), (4000, 3000)]:
        assert J.encode_bound(w, h) == J.encode_bound_sampled(w, h, 2)
    # the same coefficients as jpeg_enc_ref's, which the old tests pin
    rgb = S.window(33, 31, 5)
    ql, qc = J.quant_tables(75)
    assert np.array_equal(S.coefficients(rgb, 2, ql, qc), np.concatenate([p.reshape(-1) for p in E.encode(rgb, 75).planes()]))


def test_the_bound_is_derived_per_layout():
    """8 x (52 x blocks + 1) bytes, blocks from the layout's MCUs"""
    for (w, h) in S.SIZES + [(4000, 3000)]:
        for s, (hs, vs) in J.SAMPLING_FACTORS.items():
            blocks = (hs * vs + 2) * (-(-w // (8 * hs))) * (-(-h // (8 * vs)))
            assert J.encode_bound_sampled(w, h, s) == 8 * (52 * blocks + 1)
    assert J.encode_bound_sampled(0, 5, 1) == -1 and J.encode_bound_sampled(5, 5, 3) == -1 and J.encode_bound_sampled(5, 5, -1) == -1


def test_capacity_one_byte_short_and_bad_arguments():
    rgb = S.window(33, 17, 5)
    coef = S.coefficients(rgb, 1, *PAIRS['q91'])
    rc, scans, needed, _ = J.encode_subsequences([coef], [(33, 17)], 3, samplings=[1])
    assert rc == J.MDJPEG_OK and needed == len(scans[0])
    rc, none, needed2, buf = J.encode_subsequences([coef], [(33, 17)], 3, capacity=needed - 1, samplings=[1])
    assert rc == J.MDJPEG_ECAPACITY and none is None and needed2 == needed and buf.tobytes() == scans[0][:-1]
    assert J.encode_subsequences([coef], [(33, 17)], 3, capacity=needed, samplings=[1])[1] == scans
    assert J.encode_subsequences([coef], [(33, 17)], 64, samplings=[3])[0] == J.MDJPEG_EINVAL
    assert J.encode_subsequences([coef], [(33, 17)], 64, samplings=[-1])[0] == J.MDJPEG_EINVAL
    with pytest.raises(ValueError):
        J.sampled_file(8, 8, PAIRS['q50'][0], PAIRS['q50'][1], 3, b'')
    with pytest.raises(ValueError):
        J.sampled_file(8, 8, np.zeros(64, np.uint16), PAIRS['q50'][1], 0, b'')


def _source(tmp_path, name, rgb, **kw):
    path = str(tmp_path / name)
    Image.fromarray(rgb).save(path, **kw)
    return path


@pytest.mark.parametrize('sampling', S.SAMPLINGS)
def test_keep_source_and_sampled_file_are_what_quality_keep_writes(tmp_path, sampling):
    """save(f, exif=image.getexif(), quality='keep') of an opened RGB JPEG: the source's tables, sampling, EXIF and COM"""
    rgb = S.window(70, 50, 40 + sampling)
    exif = Image.Exif()
    exif[271] = 'a camera'
    exif[306] = '2020:01:02 03:04:05'
    path = _source(tmp_path, 'a.jpg', rgb, quality=83, subsampling=sampling, exif=exif, comment=b'trap 7')
    with open(path, 'rb') as f:
        data = f.read()
    src = J.keep_source(path, data)
    assert src['keep'] and src['sampling'] == sampling and src['comment'] == b'trap 7' and src['size'] == (70, 50)
    assert all((a == b).all() for a, b in zip(src['quant'], J.quant_tables(83)))
    image = Image.open(path)
    image.load()
    pixels = np.asarray(image)
    bio = io.BytesIO()
    image.save(bio, 'JPEG', exif=image.getexif(), quality='keep')
    want = bio.getvalue()
    coef = S.coefficients(pixels, sampling, *src['quant'])
    rc, scans, _, _ = J.encode_subsequences([coef], [(70, 50)], 64, samplings=[sampling])
    assert rc == J.MDJPEG_OK
    assert J.sampled_file(70, 50, src['quant'][0], src['quant'][1], sampling, scans[0], src['exif'], src['comment']) == want


def test_keep_source_of_files_pillow_no_longer_calls_a_jpeg(tmp_path):
    rgb = S.window(40, 24, 3)
    exif = Image.Exif()
    exif[274] = 6
    turned = J.keep_source(_source(tmp_path, 'r.jpg', rgb, quality=90, exif=exif))
    assert not turned['keep'] and turned['rotation'] == 270 and turned['size'] == (24, 40) and turned['quant'] is None
    carried = Image.Exif()
    carried.load(turned['exif'])
    assert carried[274] == 6                                          # the saved copy still carries the orientation
    grey = J.keep_source(_source(tmp_path, 'g.jpg', rgb[..., 0], quality=90))
    assert not grey['keep'] and grey['format'] == 'JPEG'
    png = J.keep_source(_source(tmp_path, 'p.png', rgb))
    assert not png['keep'] and png['format'] == 'PNG'
