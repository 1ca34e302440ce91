"""
mdhip_jpeg_encode_kept (HipContext.jpeg_encode_kept) on the device against its host model (jpeg_host.keep_merge on the
coefficients of tests/jpeg_enc_sampled_ref.py and of jpeg_host.decode, then mdjpeg_encode_subsequences_sampled), byte for byte,
which tests/test_keep_blocks_cpu.py pins against Pillow and the source's own coefficients; then separate_detections with
keep_source_blocks on both legs over the scene of tests/separate_scene.py.

ONE batched call holds windows of 1 x 1, 16 x 16, 17 x 9, 33 x 35 and 83 x 61 in all three samplings with four table pairs, each
with each kind of rectangle list; the source planes are what mdhip_jpeg_entropy_decode leaves of Pillow's files.  The window
pixels are NOT the sources' pixels (another seed), so that a block taken from the wrong side cannot pass.
"""

import ctypes as C
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import jpeg_enc_sampled_ref as S
import separate_scene as SC
from megadetector_amd import _lib, jpeg_host as J
from megadetector_amd import separate_detections as SD
from megadetector_amd.hip_backend import HipContext

pytestmark = pytest.mark.gpu

CANARY = 256
SIZES = [(1, 1), (16, 16), (17, 9), (33, 35), (83, 61)]
PAIRS = S.table_pairs()
_STATE = {}


def _ctx():
    if 'ctx' not in _STATE:
        _STATE['ctx'] = HipContext.for_images(0)
    return _STATE['ctx']


def rect_lists(w, h, s):
    """name -> the rectangles of one window"""
    hs, vs = J.SAMPLING_FACTORS[s]
    mw, mh = 8 * hs, 8 * vs
    return {'none': [], 'full': [(0, 0, w, h)],
            'one pixel at an MCU corner': [(min(mw, w) - 1, min(mh, h) - 1, min(mw, w), min(mh, h))],
            'ends on an MCU boundary': [(0, 0, mw, mh)] if w > mw and h > mh else [(0, 0, min(mw, w), min(mh, h))],
            'two overlapping': [(1, 1, w // 2 + 2, h // 2 + 2), (w // 3, h // 3, w - 1, h // 2 + 3)],
            'partly outside': [(w - 2, h - 2, w + 9, h + 9), (-4, -3, 2, 1)]}


def _batch():
    """the windows, their sources on the device and the host model's scans: made once, shared, never changed"""
    if 'batch' in _STATE:
        return _STATE['batch']
    ctx = _ctx()
    bases = []
    for si, (w, h) in enumerate(SIZES):
        for s in S.SAMPLINGS:
            pair = list(PAIRS)[(si + s) % len(PAIRS)]
            ql, qc = PAIRS[pair]
            data = S.pillow_file(S.window(w, h, 400 + 10 * si + s), s, ql, qc)
            rc, scan, _ = J.ScanImage.from_bytes(data, 0)
            assert rc == J.MDJPEG_OK
            rc, header, coef = J.decode(data)
            assert rc == J.MDJPEG_OK
            bases.append(dict(w=w, h=h, s=s, pair=pair, scan=scan, coef=coef, header=header))
    # the sources' planes: one mdhip_jpeg_entropy_decode call
    scan_offs, coef_offs, nbytes, nvals = [], [], 0, 0
    for b in bases:
        scan_offs.append(nbytes)
        nbytes += (b['scan'].nbytes + 255) // 256 * 256 + 256
        coef_offs.append(nvals)
        nvals += (b['scan'].coef_count + 127) // 128 * 128
    host = np.zeros(nbytes, dtype=np.uint8)
    for b, off in zip(bases, scan_offs):
        host[off:off + b['scan'].nbytes] = b['scan'].scan_bytes
    compressed = torch.from_numpy(host).to('cuda:0')
    coefs = torch.empty(nvals, dtype=torch.int16, device='cuda:0')
    status = ctx.jpeg_entropy_decode([b['scan'] for b in bases], [compressed.data_ptr() + o for o in scan_offs],
                                     [coefs.data_ptr() + 2 * o for o in coef_offs])
    assert (status == 0).all()
    decoded = coefs.cpu().numpy()
    for b, off in zip(bases, coef_offs):
        assert np.array_equal(decoded[off:off + b['coef'].size], b['coef'])
        b['ptr'] = coefs.data_ptr() + 2 * off
    # the windows: every base with every rectangle list, in a seeded order, one below the other in a noisy parent
    wins = [(bi, name) for bi, b in enumerate(bases) for name in rect_lists(b['w'], b['h'], b['s'])]
    wins = [wins[i] for i in np.random.default_rng(11).permutation(len(wins))]
    parent_w = 97
    rows = sum(bases[bi]['h'] + 1 for bi, _ in wins) + 1
    parent = np.random.default_rng(12).integers(0, 256, (rows, parent_w, 3), dtype=np.uint8)
    records, y = [], 1
    for k, (bi, name) in enumerate(wins):
        b = bases[bi]
        x = 1 + k % 5
        rgb = parent[y:y + b['h'], x:x + b['w']]
        rects = rect_lists(b['w'], b['h'], b['s'])[name]
        planes = S.coefficients(rgb, b['s'], *PAIRS[b['pair']])
        assert J.keep_merge(planes, b['coef'], (b['w'], b['h']), b['s'], rects) == 0
        records.append(dict(base=b, name=name, x=x, y=y, rects=rects, planes=planes))
        y += b['h'] + 1
    rc, scans, needed, _ = J.encode_subsequences([r['planes'] for r in records], [(r['base']['w'], r['base']['h']) for r in records], 64,
                                                 samplings=[r['base']['s'] for r in records])
    assert rc == J.MDJPEG_OK
    device = torch.from_numpy(parent.reshape(-1).copy()).to('cuda:0')
    _STATE['batch'] = dict(records=records, scans=scans, needed=needed, device=device, parent=parent, pitch=parent_w * 3, keepalive=(coefs, compressed))
    return _STATE['batch']


def _encode(records, device, pitch, capacity):
    ctx = _ctx()
    buf = torch.full((capacity + 2 * CANARY,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    rect_image = [k for k, r in enumerate(records) for _ in r['rects']]
    fits, offs, lens, needed, status = ctx.jpeg_encode_kept(
        [device.data_ptr() + r['y'] * pitch + r['x'] * 3 for r in records], [(r['base']['w'], r['base']['h']) for r in records],
        [pitch] * len(records), [r['base']['s'] for r in records], [PAIRS[r['base']['pair']] for r in records],
        [r['base']['ptr'] for r in records], rect_image, [q for r in records for q in r['rects']], buf.data_ptr() + CANARY, capacity)
    host = buf.cpu().numpy()
    intact = bool((host[:CANARY] == 0xA5).all() and (host[CANARY + capacity:] == 0xA5).all())
    return fits, offs, lens, needed, status, host[CANARY:CANARY + capacity], intact


def test_mixed_batch_equals_the_host_model_and_a_short_buffer_is_refused_once():
    b = _batch()
    records, scans, needed = b['records'], b['scans'], b['needed']
    assert len(records) == 5 * 3 * 6
    assert {r['base']['s'] for r in records[:12]} == {0, 1, 2} and len({r['base']['pair'] for r in records}) == 4
    # the merged planes differ from both sides somewhere: the comparison below is about the merge
    assert any(not np.array_equal(r['planes'], r['base']['coef']) for r in records if r['name'] == 'one pixel at an MCU corner')
    capacity = sum(_ctx().jpeg_encode_sampled_bound(r['base']['w'], r['base']['h'], r['base']['s']) for r in records)
    fits, offs, lens, got_needed, status, body, intact = _encode(records, b['device'], b['pitch'], capacity)
    assert fits and intact and got_needed == needed and (status == 0).all()
    assert offs[0] == 0 and (offs[1:] == offs[:-1] + lens[:-1]).all() and offs[-1] + lens[-1] == needed
    assert (body[needed:] == 0xA5).all(), 'bytes behind the last scan were written'
    for r, o, n, want in zip(records, offs, lens, scans):
        got = body[o:o + n].tobytes()
        assert got == want, '{}x{} s{} {}: the kernel wrote {} bytes, the host model {}'.format(r['base']['w'], r['base']['h'], r['base']['s'],
                                                                                                 r['name'], len(got), len(want))
    # 'none' is the source's own scan (Pillow's, without optimize) and 'full' the scan of mdhip_jpeg_encode_sampled
    for r, want in zip(records, scans):
        if r['name'] == 'none':
            rc, again, _, _ = J.encode_subsequences([r['base']['coef']], [(r['base']['w'], r['base']['h'])], samplings=[r['base']['s']])
            assert rc == J.MDJPEG_OK and again[0] == want
    assert np.array_equal(b['device'].cpu().numpy(), b['parent'].reshape(-1)), 'the parent image was written to'
    # one byte short: refused with a valid `needed`, then success with it
    fits, offs, lens, got_needed, status, body, intact = _encode(records, b['device'], b['pitch'], needed - 1)
    assert not fits and intact and got_needed == needed and (status == 0).all()
    assert body.tobytes() == b''.join(scans)[:needed - 1] and offs[-1] + lens[-1] == needed
    fits, offs, lens, got_needed, status, body, intact = _encode(records, b['device'], b['pitch'], got_needed)
    assert fits and intact and body.tobytes() == b''.join(scans)


def test_bad_sources_and_rectangles_are_refused_with_nothing_written():
    b = _batch()
    ctx, pitch, device = _ctx(), b['pitch'], b['device']
    records = [r for r in b['records'] if r['base']['w'] == 33][:4]
    n = len(records)
    capacity = sum(ctx.jpeg_encode_sampled_bound(33, 35, r['base']['s']) for r in records)
    buf = torch.full((capacity,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    packed = np.stack([np.stack(PAIRS[r['base']['pair']]) for r in records]).astype(np.uint16)
    offs, lens, need, status = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int64(-7), (C.c_int32 * n)(*[9] * n)
    ptrs = (C.c_void_p * n)(*[device.data_ptr() + r['y'] * pitch + r['x'] * 3 for r in records])
    host_planes = np.zeros(records[1]['base']['coef'].size + 64, dtype=np.int16)
    host_ptr = (host_planes.ctypes.data + 15) // 16 * 16

    def call(coef_of=lambda k, r: r['base']['ptr'], grow=(0, 0, 0), rect_image=(0,), rects=(0, 0, 5, 5), n_rects=1):
        sources = (_lib.mdhip_jpeg_source * n)()
        for k, r in enumerate(records):
            h = r['base']['header']
            sources[k].coef = coef_of(k, r)
            sources[k].blocks_w[:] = list(h.blocks_w)
            sources[k].blocks_h[:] = list(h.blocks_h)
        sources[2].blocks_w[grow[0]] += grow[1]
        sources[2].blocks_h[grow[0]] += grow[2]
        return ctx.lib.mdhip_jpeg_encode_kept(
            ctx.h, C.cast(ptrs, C.POINTER(C.c_void_p)), (C.c_int32 * n)(*[33] * n), (C.c_int32 * n)(*[35] * n), (C.c_int64 * n)(*[pitch] * n),
            (C.c_int32 * n)(*[r['base']['s'] for r in records]), n, packed.ctypes.data_as(C.POINTER(C.c_uint16)), sources,
            (C.c_int32 * max(len(rect_image), 1))(*rect_image), (C.c_int32 * max(len(rects), 1))(*rects), n_rects,
            C.c_void_p(buf.data_ptr()), capacity, offs, lens, C.byref(need), status, None)

    assert call(coef_of=lambda k, r: host_ptr if k == 1 else r['base']['ptr']) == _lib.MDHIP_EINVAL       # planes in host memory
    assert call(coef_of=lambda k, r: r['base']['ptr'] + (2 if k == 3 else 0)) == _lib.MDHIP_EINVAL         # not 16-byte aligned
    assert call(coef_of=lambda k, r: 0 if k == 0 else r['base']['ptr']) == _lib.MDHIP_EINVAL
    for grow in ((0, 1, 0), (0, 0, -1), (1, 1, 0), (2, 0, 1)):                                             # not the window's whole MCUs
        assert call(grow=grow) == _lib.MDHIP_EINVAL, grow
    assert call(rect_image=(n,)) == _lib.MDHIP_EINVAL and call(rect_image=(-1,)) == _lib.MDHIP_EINVAL     # a rectangle of window n
    assert call(rect_image=(0, n), rects=(0, 0, 5, 5, 0, 0, 0, 0), n_rects=2) == _lib.MDHIP_EINVAL         # (even one without area)
    assert call(n_rects=-1) == _lib.MDHIP_EINVAL
    packed[1, 0, 7] = 0                                                                                    # and what encode_sampled refuses
    assert call() == _lib.MDHIP_EINVAL
    packed[1, 0, 7] = 9
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all() and need.value == -7 and list(status) == [9] * n
    assert call() == _lib.MDHIP_OK and need.value > 0 and list(status) == [0] * n                          # the same arguments, unspoilt


def test_an_uncodable_dc_difference_flags_its_window_only():
    """tables of ones, a source DC of +1500 beside a changed black MCU (-1024): category 12.  The flagged window comes FIRST,
    so the normal one's scan lies where the flagged one's would have begun."""
    b = _batch()
    ctx = _ctx()
    normal = next(r for r in b['records'] if r['base']['w'] == 33 and r['name'] == 'two overlapping')
    want = b['scans'][b['records'].index(normal)]
    w, h = 16, 8
    source = np.zeros((3, 2, 64), dtype=np.int16)
    source[0, :, 0] = 1500
    planes = torch.from_numpy(source.reshape(-1).copy()).to('cuda:0')
    black = torch.zeros(w * h * 3, dtype=torch.uint8, device='cuda:0')
    ones = (np.ones(64, dtype=np.uint16), np.ones(64, dtype=np.uint16))
    merged = np.zeros((3, 2, 64), dtype=np.int16)
    merged[0, :, 0] = -1024
    merged = merged.reshape(-1)
    assert J.keep_merge(merged, source.reshape(-1), (w, h), 0, [(0, 0, 8, 8)]) == 1                       # the host model says so too
    capacity = ctx.jpeg_encode_sampled_bound(w, h, 0) + ctx.jpeg_encode_sampled_bound(33, 35, normal['base']['s'])
    buf = torch.full((capacity,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()

    def run(rects_of_first):
        return ctx.jpeg_encode_kept([black.data_ptr(), b['device'].data_ptr() + normal['y'] * b['pitch'] + normal['x'] * 3],
                                    [(w, h), (33, 35)], [w * 3, b['pitch']], [0, normal['base']['s']], [ones, PAIRS[normal['base']['pair']]],
                                    [planes.data_ptr(), normal['base']['ptr']], [0] * len(rects_of_first) + [1] * len(normal['rects']),
                                    rects_of_first + normal['rects'], buf.data_ptr(), capacity)

    fits, offs, lens, needed, status = run([(0, 0, 8, 8)])
    assert fits and list(status) == [1, 0]
    assert lens[0] == 0 and offs[1] == 0 and lens[1] == len(want) and needed == len(want)
    assert buf[:needed].cpu().numpy().tobytes() == want
    fits, offs, lens, needed, status = run([])                            # all source: 1500, then a difference of 0
    assert fits and list(status) == [0, 0] and lens[0] > 0
    rc, scans, _, _ = J.encode_subsequences([source.reshape(-1)], [(w, h)], samplings=[0])
    assert rc == J.MDJPEG_OK and buf[:lens[0]].cpu().numpy().tobytes() == scans[0]
    assert buf[offs[1]:offs[1] + lens[1]].cpu().numpy().tobytes() == want


def _run(folder, backend):
    image_folder, results_file = SC.build(folder)
    sources = SC.source_hashes(image_folder)
    out = os.path.join(folder, 'out')
    options = SC.apply_options(SD.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out,
                               {'render_boxes': True, 'category_names_to_blur': 'person'})
    options.keep_source_blocks = True
    with redirect_stdout(io.StringIO()):
        counts = SD.separate_detections_into_folders(options, backend=backend)
    files = {}
    for root, _, names in os.walk(out):
        for n in names:
            with open(os.path.join(root, n), 'rb') as f:
                files[os.path.relpath(os.path.join(root, n), out).replace(os.sep, '/')] = f.read()
    return files, counts, SC.describe_tree(out, sources)


def test_device_leg_and_host_leg_write_the_same_kept_copies(tmp_path):
    (tmp_path / 'host').mkdir()
    (tmp_path / 'gpu').mkdir()
    host_files, host_counts, _ = _run(str(tmp_path / 'host'), 'host')
    gpu_files, counts, tree = _run(str(tmp_path / 'gpu'), 'gpu')
    print(counts)
    assert sorted(gpu_files) == sorted(host_files)
    for rel in sorted(host_files):
        assert gpu_files[rel] == host_files[rel], '{}: the device leg wrote {} bytes, the host leg {}'.format(rel, len(gpu_files[rel]), len(host_files[rel]))
    how = {name: h for name, _, _, h, _ in SC.IMAGES}
    rendered = [rel for rel, e in tree.items() if not rel.endswith('/') and e['copy_of'] is None]
    eligible = [rel for rel in rendered if rel.endswith('.jpg') and how[next(n for n in how if rel.endswith(n))].get('mode') != 'L'
                and 274 not in how[next(n for n in how if rel.endswith(n))].get('exif', {})]
    on_host = [rel for rel in rendered if rel.endswith('.png')]          # no JPEG name: the host leg's, and not eligible
    assert len(eligible) >= 8 and len(rendered) == counts['rendered'] == host_counts['rendered']
    assert counts['kept'] == host_counts['kept'] == len(eligible) and counts['kept_refused'] == host_counts['kept_refused'] == 0
    assert counts['host'] == len(on_host) == 1 and counts['gpu'] == len(rendered) - 1                    # no eligible copy fell back
    assert counts['files_decoded_pil'] == 0 and counts['decode_chunks'] == 1
    assert counts['encode_calls'] == 2                                    # ONE kept call, ONE sampled call for the rotated and the 'L' file
