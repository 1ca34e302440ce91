"""
keep_source_blocks on the CPU: the host model of the merge (mdjpeg_keep_merge, jpeg_host.keep_merge) and the host leg of
separate_detections that is built on it, pinned against things that are not this project's encoder -- the source file's own
coefficients and Pillow's encode of the modified pixels with the source's tables and sampling.  The changed set of MCUs is
computed here in plain NumPy from the rule (clip, then overlap of half-open intervals), not through the library.

Sources: generated 83 x 61, 16 x 16 and 1 x 1 images at quality 90 in 4:4:4, 4:2:2 and 4:2:0.
"""

import io
import os

import numpy as np
import pytest
from PIL import Image, ImageDraw, ImageFilter

import jpeg_enc_sampled_ref as S
import separate_scene as SC
from megadetector_amd import jpeg_host as J
from megadetector_amd import separate_detections as SD

SIZES = [(83, 61), (16, 16), (1, 1)]
#: per size: a drawn rectangle (inclusive corners) and a blurred one (exclusive right / bottom)
EDITS = {(83, 61): ((10, 5, 30, 20), (40, 30, 70, 55)), (16, 16): ((3, 3, 9, 6), None), (1, 1): ((0, 0, 0, 0), None)}
CASES = [(w, h, s) for (w, h) in SIZES for s in (0, 1, 2)]
_STATE = {}


def _mcu(s):
    hs, vs = J.SAMPLING_FACTORS[s]
    return 8 * hs, 8 * vs


def changed_mcus(w, h, s, rects):
    """[mcus_y][mcus_x] bool, from the rule"""
    mw, mh = _mcu(s)
    out = np.zeros((-(-h // mh), -(-w // mw)), dtype=bool)
    for left, top, right, bottom in rects:
        left, top, right, bottom = max(left, 0), max(top, 0), min(right, w), min(bottom, h)
        if right <= left or bottom <= top:
            continue
        for my in range(out.shape[0]):
            for mx in range(out.shape[1]):
                if left < (mx + 1) * mw and right > mx * mw and top < (my + 1) * mh and bottom > my * mh:
                    out[my, mx] = True
    return out


def _source(tmp, w, h, s):
    rng = np.random.default_rng(1000 * w + 10 * h + s)
    rgb = SC._content(rng, max(w, 16), max(h, 16))[:h, :w]
    path = os.path.join(tmp, 'src_{}x{}_s{}.jpg'.format(w, h, s))
    Image.fromarray(np.ascontiguousarray(rgb)).save(path, quality=90, subsampling=s)
    return path


def _edit(image, w, h):
    """draws and blurs as the host leg does; -> the changed rectangles"""
    drawn, blurred = EDITS[(w, h)]
    rects = []
    if blurred is not None:
        region = image.crop(blurred)
        image.paste(region.filter(ImageFilter.GaussianBlur(radius=4)), (blurred[0], blurred[1]))
        rects.append(blurred)
    ImageDraw.Draw(image).rectangle([(drawn[0], drawn[1]), (drawn[2], drawn[3])], fill=(255, 20, 147))
    rects.append((drawn[0], drawn[1], drawn[2] + 1, drawn[3] + 1))
    return rects


def _case(tmp_path_factory, w, h, s):
    """source, the host leg's file for the edited image, and the planes of source, Pillow's encode and the file: made once"""
    key = (w, h, s)
    if key not in _STATE:
        tmp = str(tmp_path_factory.mktemp('keep_{}x{}_s{}'.format(w, h, s)))
        path = _source(tmp, w, h, s)
        with open(path, 'rb') as f:
            data = f.read()
        image = Image.open(path)
        image.load()
        rects = _edit(image, w, h)
        keep = SD.keep_source_record(path, os.path.join(tmp, 'out.jpg'))
        assert keep is not None and keep['src']['sampling'] == s and keep['size'] == (w, h)
        keep['changed'] = rects
        assert SD.save_kept_host(image, os.path.join(tmp, 'out.jpg'), keep) == 'kept'
        with open(os.path.join(tmp, 'out.jpg'), 'rb') as f:
            written = f.read()
        ql, qc = keep['src']['quant']
        pillow = S.pillow_file(np.asarray(image), s, ql, qc)
        planes = {}
        for name, blob in (('source', data), ('pillow', pillow), ('written', written)):
            rc, header, coef = J.decode(blob)
            assert rc == J.MDJPEG_OK, name
            planes[name] = header.planes(coef)
        _STATE[key] = dict(tmp=tmp, path=path, data=data, image=image, rects=rects, keep=keep, written=written, planes=planes,
                           changed=changed_mcus(w, h, s, rects))
    return _STATE[key]


def _block_mask(changed, s):
    """the changed set per block of each plane"""
    hs, vs = J.SAMPLING_FACTORS[s]
    return [np.repeat(np.repeat(changed, vs, axis=0), hs, axis=1), changed, changed]


@pytest.mark.parametrize('w,h,s', CASES)
def test_written_file_has_the_sources_blocks_where_nothing_changed_and_pillows_elsewhere(tmp_path_factory, w, h, s):
    c = _case(tmp_path_factory, w, h, s)
    n_changed = n_kept = 0
    for p, mask in enumerate(_block_mask(c['changed'], s)):
        got, src, pil = c['planes']['written'][p], c['planes']['source'][p], c['planes']['pillow'][p]
        assert got.shape == src.shape == pil.shape == mask.shape + (64,)
        assert np.array_equal(got[~mask], src[~mask]), 'plane {}: an unchanged block is not the source\'s'.format(p)
        assert np.array_equal(got[mask], pil[mask]), 'plane {}: a changed block is not Pillow\'s'.format(p)
        n_changed += int(mask.sum())
        n_kept += int((~mask).sum())
    assert n_changed > 0
    if (w, h) == (83, 61):
        assert n_kept >= 20                                                   # (the equality above is not over an empty set)
        src, pil = c['planes']['source'][0], c['planes']['pillow'][0]
        assert not np.array_equal(src[~_block_mask(c['changed'], s)[0]], pil[~_block_mask(c['changed'], s)[0]]), \
            'a full re-encode keeps every unchanged block here: the test shows nothing'


@pytest.mark.parametrize('w,h,s', CASES)
def test_pixels_outside_the_changed_mcus_and_their_ring_are_the_sources(tmp_path_factory, w, h, s):
    c = _case(tmp_path_factory, w, h, s)
    got = np.asarray(Image.open(io.BytesIO(c['written'])).convert('RGB'))
    src = np.asarray(Image.open(io.BytesIO(c['data'])).convert('RGB'))
    changed = c['changed']
    if s != 0:                                                                # one MCU around: fancy up-sampling reads the neighbour's edge
        padded = np.pad(changed, 1)
        changed = np.zeros_like(changed)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                changed |= padded[dy:dy + changed.shape[0], dx:dx + changed.shape[1]]
    mw, mh = _mcu(s)
    same = ~np.repeat(np.repeat(changed, mh, axis=0), mw, axis=1)[:h, :w]
    assert np.array_equal(got[same], src[same])
    if (w, h) == (83, 61):
        assert same.sum() > 0 and (s != 0 or same.sum() > w * h // 2)


@pytest.mark.parametrize('s', (0, 1, 2))
def test_boundaries_one_pixel_and_outside(s):
    w, h = 83, 61
    mw, mh = _mcu(s)
    hs, vs = J.SAMPLING_FACTORS[s]
    shape = (-(-h // mh), -(-w // mw))
    values = shape[0] * shape[1] * (hs * vs + 2) * 64
    source = np.full(values, 7, dtype=np.int16)

    def merged(rects):
        planes = np.zeros(values, dtype=np.int16)
        assert J.keep_merge(planes, source, (w, h), s, rects) == 0
        ny = shape[0] * vs * shape[1] * hs
        y = planes[:ny * 64].reshape(shape[0], vs, shape[1], hs, 64)
        cb = planes[ny * 64:(ny + shape[0] * shape[1]) * 64].reshape(shape + (64,))
        cr = planes[(ny + shape[0] * shape[1]) * 64:].reshape(shape + (64,))
        y_changed = (y == 0).all(axis=(1, 3, 4))
        assert np.array_equal(y_changed, ~(y == 7).all(axis=(1, 3, 4)))     # an MCU is kept or changed as a whole
        assert np.array_equal(y_changed, (cb == 0).all(axis=2)) and np.array_equal(y_changed, (cr == 0).all(axis=2))
        assert np.array_equal(~y_changed, (cb == 7).all(axis=2)) and np.array_equal(~y_changed, (cr == 7).all(axis=2))
        return y_changed

    only = lambda my, mx: np.array([[(y, x) == (my, mx) for x in range(shape[1])] for y in range(shape[0])])
    # the exclusive right / bottom edge exactly on an MCU boundary does not change the next MCU
    assert np.array_equal(merged([(0, 0, mw, mh)]), only(0, 0))
    assert np.array_equal(merged([(mw, mh, 2 * mw, 2 * mh)]), only(1, 1))
    assert merged([(0, 0, mw + 1, mh)]).sum() == 2 and merged([(0, 0, mw, mh + 1)]).sum() == 2
    # one pixel changes exactly one MCU, at every corner of it
    for x, y in ((mw, mh), (2 * mw - 1, mh), (mw, 2 * mh - 1), (2 * mw - 1, 2 * mh - 1)):
        assert np.array_equal(merged([(x, y, x + 1, y + 1)]), only(1, 1))
    # wholly outside the window: none, also where the last MCU reaches beyond the window
    assert w % mw and h % mh
    for rect in ((w, 0, w + 5, 5), (w + 1, 2, w + 9, 9), (0, h, 9, h + 3), (-9, -9, 0, 0), (-5, 3, 0, 9), (5, 5, 5, 9), (9, 9, 3, 3)):
        assert not merged([rect]).any(), rect
    # partly outside: clipped, not dropped
    assert np.array_equal(merged([(-5, -5, 1, 1)]), only(0, 0))
    assert np.array_equal(merged([(w - 1, h - 1, w + 50, h + 50)]), only(shape[0] - 1, shape[1] - 1))
    for rects in ([(3, 3, 20, 20), (18, 10, 40, 12)], [(0, 0, w, h)], []):
        assert np.array_equal(merged(rects), changed_mcus(w, h, s, rects))


@pytest.mark.parametrize('w,h,s', CASES)
def test_no_rectangle_gives_the_sources_scan_and_full_cover_todays_file(tmp_path_factory, w, h, s):
    c = _case(tmp_path_factory, w, h, s)
    keep = dict(c['keep'])
    target = os.path.join(c['tmp'], 'none.jpg')
    keep['changed'] = []
    assert SD.save_kept_host(c['image'], target, keep) == 'kept'
    with open(target, 'rb') as f:
        none = f.read()
    rc, header, coef = J.decode(none)
    assert rc == J.MDJPEG_OK
    for got, src in zip(header.planes(coef), c['planes']['source']):
        assert np.array_equal(got, src)
    assert S.scan_of(none) == S.scan_of(c['data'])                           # the source is Pillow's, without `optimize`
    keep['changed'] = [(0, 0, w, h)]
    full, today = os.path.join(c['tmp'], 'full.jpg'), os.path.join(c['tmp'], 'today.jpg')
    assert SD.save_kept_host(c['image'], full, keep) == 'kept'
    SD.exif_preserving_save(c['image'], today)
    with open(full, 'rb') as f, open(today, 'rb') as g:
        assert f.read() == g.read()


def test_uncodable_dc_difference_sets_the_status():
    """tables of ones: a source DC of +1500 beside a changed black MCU (DC -1024) differs by 2524 > 2047"""
    w, h, s = 16, 8, 0
    black = np.zeros((2, 3, 64), dtype=np.int16)                             # [mcu][Y, Cb, Cr] -> planes below
    black[:, 0, 0] = -1024
    source = np.zeros((2, 3, 64), dtype=np.int16)
    source[:, 0, 0] = 1500
    as_planes = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(-1)
    planes = as_planes(black)
    assert J.keep_merge(planes, as_planes(source), (w, h), s, [(0, 0, 8, 8)]) == 1
    assert planes[0] == -1024 and planes[64] == 1500                          # merged all the same
    assert J.encode_subsequences([planes], [(w, h)], samplings=[s])[0] == J.MDJPEG_ECORRUPT
    for rects in ([], [(0, 0, 16, 8)]):                                       # all source, all black: both codable
        planes = as_planes(black)
        assert J.keep_merge(planes, as_planes(source), (w, h), s, rects) == 0
        assert J.encode_subsequences([planes], [(w, h)], samplings=[s])[0] == J.MDJPEG_OK


def test_keep_merge_refuses_bad_arguments():
    good = np.zeros(3 * 64, dtype=np.int16)
    with pytest.raises(ValueError):
        J.keep_merge(good, good.copy(), (8, 8), 3, [])
    with pytest.raises(ValueError):
        J.keep_merge(good, np.zeros(64, dtype=np.int16), (8, 8), 0, [])
    with pytest.raises(ValueError):
        J.keep_merge(good, good.copy(), (9, 8), 0, [])
    lib = J.load()
    status = J.C.c_int32(5)
    assert lib.mdjpeg_keep_merge(good.ctypes.data, good.ctypes.data, 8, 8, 0, None, -1, J.C.byref(status)) == J.MDJPEG_EINVAL
    assert lib.mdjpeg_keep_merge(good.ctypes.data, None, 8, 8, 0, None, 0, J.C.byref(status)) == J.MDJPEG_EINVAL
    assert lib.mdjpeg_keep_merge(good.ctypes.data, good.ctypes.data, 0, 8, 0, None, 0, J.C.byref(status)) == J.MDJPEG_EINVAL
    assert status.value == 5


def _eligible(name, how):
    """an RGB JPEG that open_image returns as it is"""
    return name.endswith('.jpg') and how.get('mode') != 'L' and 274 not in how.get('exif', {})


@pytest.mark.parametrize('option_set', ['render_boxes', 'blur_and_boxes'])
def test_host_leg_over_the_scene_keeps_every_eligible_copy(tmp_path, option_set):
    image_folder, results_file = SC.build(str(tmp_path))
    sources = SC.source_hashes(image_folder)
    trees, counts = {}, {}
    for on in (False, True):
        out = str(tmp_path / ('on' if on else 'off'))
        options = SC.apply_options(SD.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out, SC.OPTION_SETS[option_set])
        assert options.keep_source_blocks is False
        options.keep_source_blocks = on
        counts[on] = SD.separate_detections_into_folders(options, backend='host')
        trees[on] = SC.describe_tree(out, sources)
    assert counts[False]['kept'] == 0 and counts[False]['kept_refused'] == 0
    assert sorted(trees[True]) == sorted(trees[False])
    how = {name: h for name, _, _, h, _ in SC.IMAGES}
    rendered = [rel for rel, e in trees[False].items() if not rel.endswith('/') and e['copy_of'] is None]
    eligible = [rel for rel in rendered if _eligible(rel, how[next(n for n in how if rel.endswith(n))])]
    assert len(rendered) == counts[True]['rendered'] == counts[False]['rendered']
    assert len(eligible) >= 5 and len(eligible) < len(rendered)
    assert counts[True]['kept'] == len(eligible) and counts[True]['kept_refused'] == 0
    # (a copy whose boxes touch every MCU, or whose source re-encodes to itself, is the same file either way)
    assert sum(trees[True][rel]['sha256'] != trees[False][rel]['sha256'] for rel in eligible) >= 3
    for rel in rendered:
        if rel in eligible:
            for k in ('size', 'quant', 'sampling', 'segments'):
                assert trees[True][rel][k] == trees[False][rel][k], (rel, k)
        else:
            assert trees[True][rel]['sha256'] == trees[False][rel]['sha256'], rel
    # and a kept copy of the scene really holds its source's blocks outside its boxes
    rel = next(r for r in eligible if r.endswith('a422.jpg'))
    with open(os.path.join(str(tmp_path / 'on'), rel), 'rb') as f, open(os.path.join(image_folder, 'a422.jpg'), 'rb') as g:
        (_, hk, ck), (_, hs_, cs) = J.decode(f.read()), J.decode(g.read())
    same = [(a == b).all(axis=2) for a, b in zip(hk.planes(ck), hs_.planes(cs))]
    assert 0 < same[1].sum() < same[1].size and same[1].sum() == same[2].sum()


def test_the_switch_reaches_the_options():
    seen = {}
    real = SD.separate_detections_into_folders
    SD.separate_detections_into_folders = lambda options, **kw: seen.update(options=options) or {'images': 0}
    try:
        SD.main(['r.json', 'in', 'out', '--keep_source_blocks', '--backend', 'host'])
        assert seen['options'].keep_source_blocks is True
        SD.main(['r.json', 'in', 'out', '--backend', 'host'])
        assert seen['options'].keep_source_blocks is False
    finally:
        SD.separate_detections_into_folders = real
