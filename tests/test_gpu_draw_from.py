"""
The fan-out draw on the device: mdhip_draw_ops_from (HipContext.draw_ops_from) against its host model mdjpeg_draw_from, byte
for byte over whole allocations -- the destinations are filled with a sentinel first, so every byte beside the 3 * width
bytes of a row must still hold it -- and with the sources unchanged.  The cases (draw_from_cases.py) are the smallest at
which the 16-byte runs, the byte runs at a row's two ends and the alignments of a destination against its source can each go
wrong.
"""

import numpy as np
import pytest
import torch

import draw_from_cases as D
from megadetector_amd import _lib
from megadetector_amd import jpeg_host as J
from test_gpu_tile_jpeg import _ctx

pytestmark = pytest.mark.gpu


def _device(a):
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to('cuda:0')
    torch.cuda.synchronize()
    return t


def _run(ctx, c, check=True, **changes):
    """the case on the device -> (code, the destinations' allocations, the sources' allocations afterwards, the arguments)"""
    srcs = [_device(b) for b in D.source_buffers(c)]
    dsts = [_device(b) for b in D.dest_buffers(c)]
    assert all(t.data_ptr() % 16 == 0 for t in srcs + dsts)
    patches = _device(np.frombuffer(changes.pop('patches', c['patches']), np.uint8).copy())
    args = list(D.call_arguments(c, [t.data_ptr() for t in srcs], [t.data_ptr() for t in dsts]))
    names = ['src_ptrs', 'sizes', 'src_pitches', 'dst_ptrs', 'dst_src', 'dst_pitches', 'op_image', 'ops']
    for k, v in changes.items():
        args[names.index(k)] = v(args) if callable(v) else v
    rc = ctx.draw_ops_from(*args, patches.data_ptr(), patches.numel(), check=check)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in dsts], [t.cpu().numpy() for t in srcs]


def test_every_case_equals_the_host_model_padding_included():
    ctx = _ctx()
    for i, c in enumerate(D.all_cases()):
        rc, dsts, srcs = _run(ctx, c)
        hrc, want, _ = D.host_model(c)
        assert rc == 0 and hrc == J.MDJPEG_OK
        for m, (got, w) in enumerate(zip(dsts, want)):
            assert int((got != w).sum()) == 0, 'case {} ({}), destination {}: {} bytes differ'.format(
                i, c['sources'][0][0].shape, m, int((got != w).sum()))
        for got, w in zip(srcs, D.source_buffers(c)):
            np.testing.assert_array_equal(got, w, err_msg='case {}: a source changed'.format(i))


def test_bad_calls_return_einval_and_leave_the_sentinel():
    ctx = _ctx()
    c = D.case(33, 17, 5, 1)
    bad = {
        'a destination on its source': dict(dst_ptrs=lambda a: [a[0][0]] + a[3][1:]),
        'dst_src out of range': dict(dst_src=[0, 2, 0, 1]),
        'a patch beyond patches': dict(patches=c['patches'][:-1]),
    }
    for what, changes in bad.items():
        rc, dsts, srcs = _run(ctx, c, check=False, **changes)
        assert rc == _lib.MDHIP_EINVAL, what
        for got, w in zip(dsts, D.dest_buffers(c)):
            np.testing.assert_array_equal(got, w, err_msg=what)
        for got, w in zip(srcs, D.source_buffers(c)):
            np.testing.assert_array_equal(got, w, err_msg=what)
