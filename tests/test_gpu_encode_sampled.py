"""
mdhip_jpeg_encode_sampled (HipContext.jpeg_encode_sampled) on the device: the window matrix of test_encode_sampled_cpu.py in
ONE mixed batch -- 4:4:4, 4:2:2 and 4:2:0 windows and four pairs of quantisation tables interleaved in one call, the windows
cut out of a parent image with an odd pitch at odd origins -- against the host model (mdjpeg_encode_subsequences_sampled on the
coefficients of tests/jpeg_enc_sampled_ref.py, which the CPU suite pins against Pillow), byte for byte.  Canary bytes lie around
the output buffer.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_enc_sampled_ref as S
from megadetector_amd import _lib, jpeg_host as J
from megadetector_amd._lib import HipError
from megadetector_amd.hip_backend import HipContext

pytestmark = pytest.mark.gpu

CANARY = 256
PARENT_W = 97                                    # pixels a row of the parent: 291 bytes, an odd pitch
_STATE = {}
PAIRS = S.table_pairs()


def _ctx():
    if 'ctx' not in _STATE:
        _STATE['ctx'] = HipContext.for_images(0)
    return _STATE['ctx']


def _batch():
    """the matrix in a seeded random order, its windows one below the other in a noisy parent image on the device, and the
    host model's scans: computed once, shared by the tests, never changed"""
    if 'batch' not in _STATE:
        cases = S.matrix()
        order = np.random.default_rng(5).permutation(len(cases))
        cases = [cases[i] for i in order]
        rows = sum(c[1].shape[0] + 1 for c in cases) + 1
        parent = np.random.default_rng(6).integers(0, 256, (rows, PARENT_W, 3), dtype=np.uint8)
        wins, y = [], 1
        for k, (_, rgb, _, _) in enumerate(cases):
            h, w = rgb.shape[:2]
            x = 1 + k % 5 if w + 5 < PARENT_W else PARENT_W - w
            parent[y:y + h, x:x + w] = rgb
            wins.append((x, y, w, h))
            y += h + 1
        device = torch.from_numpy(parent.reshape(-1).copy()).to('cuda:0')
        coefs = [S.coefficients(rgb, s, *PAIRS[pair]) for _, rgb, s, pair in cases]
        rc, scans, needed, _ = J.encode_subsequences(coefs, [(w, h) for _, _, w, h in wins], 64, samplings=[c[2] for c in cases])
        assert rc == J.MDJPEG_OK
        _STATE['batch'] = (cases, wins, parent, device, scans, needed)
    return _STATE['batch']


def _encode(cases, wins, device, capacity, samplings=None, quants=None):
    """-> (fits, offsets, sizes, needed, the buffer's bytes, canaries intact)"""
    ctx = _ctx()
    pitch = PARENT_W * 3
    buf = torch.full((capacity + 2 * CANARY,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    fits, offs, lens, needed = ctx.jpeg_encode_sampled([device.data_ptr() + y * pitch + x * 3 for x, y, _, _ in wins],
                                                       [(w, h) for _, _, w, h in wins], [pitch] * len(wins),
                                                       samplings if samplings is not None else [c[2] for c in cases],
                                                       quants if quants is not None else [PAIRS[c[3]] for c in cases],
                                                       buf.data_ptr() + CANARY, capacity)
    host = buf.cpu().numpy()
    intact = bool((host[:CANARY] == 0xA5).all() and (host[CANARY + capacity:] == 0xA5).all())
    return fits, offs, lens, needed, host[CANARY:CANARY + capacity], intact


def test_the_batch_interleaves_layouts_and_tables():
    cases = _batch()[0]
    assert len(cases) == 8 * 3 * 4 + 6
    first = cases[:24]
    assert {c[2] for c in first} == {0, 1, 2} and {c[3] for c in first} == set(PAIRS)
    assert any(a[2] != b[2] for a, b in zip(cases, cases[1:])) and any(a[3] != b[3] for a, b in zip(cases, cases[1:]))


def test_mixed_batch_equals_the_host_model_and_pillow():
    cases, wins, parent, device, scans, needed = _batch()
    capacity = sum(_ctx().jpeg_encode_sampled_bound(w, h, c[2]) for c, (_, _, w, h) in zip(cases, wins))
    fits, offs, lens, got_needed, body, intact = _encode(cases, wins, device, capacity)
    assert fits and intact and got_needed == needed
    assert offs[0] == 0 and (offs[1:] == offs[:-1] + lens[:-1]).all() and offs[-1] + lens[-1] == needed
    assert (body[needed:] == 0xA5).all(), 'bytes behind the last scan were written'
    for (name, rgb, s, pair), o, n, want in zip(cases, offs, lens, scans):
        got = body[o:o + n].tobytes()
        assert got == want, '{}: the kernel wrote {} bytes, the host model {}'.format(name, len(got), len(want))
        assert n <= _ctx().jpeg_encode_sampled_bound(rgb.shape[1], rgb.shape[0], s)
    for k in range(0, len(cases), 7):                                     # and the files, against Pillow itself
        name, rgb, s, pair = cases[k]
        ql, qc = PAIRS[pair]
        assert J.sampled_file(rgb.shape[1], rgb.shape[0], ql, qc, s, body[offs[k]:offs[k] + lens[k]].tobytes()) == S.pillow_file(rgb, s, ql, qc), name
    assert np.array_equal(device.cpu().numpy(), parent.reshape(-1)), 'the parent image was written to'


def test_capacity_one_byte_short_is_refused_and_one_retry_succeeds():
    cases, wins, _, device, scans, needed = _batch()
    fits, offs, lens, got_needed, body, intact = _encode(cases, wins, device, needed - 1)
    assert not fits and intact and got_needed == needed
    assert body.tobytes() == b''.join(scans)[:needed - 1]
    assert offs[-1] + lens[-1] == needed
    fits, offs, lens, got_needed, body, intact = _encode(cases, wins, device, got_needed)
    assert fits and intact and body.tobytes() == b''.join(scans)


def test_invalid_tables_or_sampling_are_refused_with_nothing_launched():
    cases, wins, _, device, _, needed = _batch()
    cases, wins = cases[:6], wins[:6]
    good = [PAIRS[c[3]] for c in cases]
    for bad_value in (0, 256, 65535):
        luma = good[3][0].copy()
        luma[17] = bad_value
        quants = good[:3] + [(luma, good[3][1])] + good[4:]
        with pytest.raises(HipError, match='1 .. 255'):
            _encode(cases, wins, device, needed, quants=quants)
    chroma = good[5][1].copy()
    chroma[63] = 0
    with pytest.raises(HipError, match='1 .. 255'):
        _encode(cases, wins, device, needed, quants=good[:5] + [(good[5][0], chroma)])
    for bad_sampling in (3, -1, 4):
        with pytest.raises(HipError, match='sampling'):
            _encode(cases, wins, device, needed, samplings=[0, 1, 2, bad_sampling, 1, 0])
    # the output buffer is untouched by a refused call: the raw call, then the bytes
    ctx, pitch, n = _ctx(), PARENT_W * 3, len(wins)
    buf = torch.full((needed,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    packed = np.stack([np.stack(p) for p in good]).astype(np.uint16)
    packed[2, 1, 5] = 300
    offs, lens, need = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_int64(-7)
    ptrs = (C.c_void_p * n)(*[device.data_ptr() + y * pitch + x * 3 for x, y, _, _ in wins])
    args = lambda samplings: (ctx.h, C.cast(ptrs, C.POINTER(C.c_void_p)), (C.c_int32 * n)(*[a[2] for a in wins]),
                              (C.c_int32 * n)(*[a[3] for a in wins]), (C.c_int64 * n)(*[pitch] * n), (C.c_int32 * n)(*samplings), n,
                              packed.ctypes.data_as(C.POINTER(C.c_uint16)), C.c_void_p(buf.data_ptr()), needed, offs, lens, C.byref(need), None)
    assert ctx.lib.mdhip_jpeg_encode_sampled(*args([c[2] for c in cases])) == _lib.MDHIP_EINVAL
    packed[2, 1, 5] = 30
    assert ctx.lib.mdhip_jpeg_encode_sampled(*args([0, 1, 2, 2, 1, 7])) == _lib.MDHIP_EINVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all() and need.value == -7
    assert ctx.jpeg_encode_sampled_bound(8, 8, 3) == -1 and ctx.jpeg_encode_sampled_bound(0, 8, 1) == -1
    for (w, h) in S.SIZES:
        for s in S.SAMPLINGS:
            assert ctx.jpeg_encode_sampled_bound(w, h, s) == J.encode_bound_sampled(w, h, s)


def test_the_old_call_is_the_h2v2_one_pair_case_of_the_new_one():
    cases, wins, _, device, _, _ = _batch()
    keep = [k for k, c in enumerate(cases) if c[2] == 2]
    cases, wins = [cases[k] for k in keep], [wins[k] for k in keep]
    ctx, pitch = _ctx(), PARENT_W * 3
    capacity = sum(ctx.jpeg_encode_bound(w, h) for _, _, w, h in wins)
    assert capacity == sum(ctx.jpeg_encode_sampled_bound(w, h, 2) for _, _, w, h in wins)
    old = torch.full((capacity,), 0xA5, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    fits, offs, lens, needed = ctx.jpeg_encode([device.data_ptr() + y * pitch + x * 3 for x, y, _, _ in wins], [(w, h) for _, _, w, h in wins],
                                               [pitch] * len(wins), 91, old.data_ptr(), capacity)
    new = _encode(cases, wins, device, capacity, quants=[J.quant_tables(91)] * len(wins))
    assert fits and new[0] and new[5] and needed == new[3] and (offs == new[1]).all() and (lens == new[2]).all()
    assert np.array_equal(old.cpu().numpy(), new[4])
