"""
The host model of the fan-out draw, mdjpeg_draw_from (include/mdjpeg.h; the GPU call is mdhip_draw_ops_from): many
destinations made from shared sources in one call equal a copy of the source followed by mdjpeg_draw, byte for byte, with
nothing written beside the rows and no source changed; what it refuses, it refuses with nothing written.  The same code runs
under AddressSanitizer + UBSan as a program of its own (`make asan-jpeg`, the --draw-from mode of host_asan_main.cpp).
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

import draw_from_cases as D
from conftest import REPO
from megadetector_amd import jpeg_host as J


@pytest.mark.parametrize('index', range(len(D.all_cases())))
def test_equals_copy_then_draw_and_writes_nothing_else(index):
    c = D.all_cases()[index]
    rc, dsts, srcs = D.host_model(c)
    assert rc == J.MDJPEG_OK
    for m, (got, want) in enumerate(zip(dsts, D.copy_then_draw(c))):
        np.testing.assert_array_equal(got, want, err_msg='destination {}'.format(m))
    for got, want in zip(srcs, D.source_buffers(c)):
        np.testing.assert_array_equal(got, want)
    # the destination without an operation is its source, and the others are not
    changed = [not np.array_equal(a, b) for a, b in zip(D.copy_then_draw(c), D.copy_then_draw(dict(c, lists=[[]] * len(c['dests']))))]
    assert changed[0] and not changed[1] and changed[-1]


def test_the_operations_of_a_destination_keep_their_order():
    """two rectangles on one pixel: the later one wins, in either order, and the other destination of the source is untouched"""
    src = D.noise(5, 3, 1)
    red, blue = [0, 1, 1, 3, 1, 0x0000FF, 0, 0], [0, 2, 0, 2, 2, 0xFF0000, 0, 0]
    for ops, colour in (([red, blue], (0, 0, 255)), ([blue, red], (255, 0, 0))):
        a, b = np.zeros_like(src), np.zeros_like(src)
        assert J.draw_ops_from([src.ctypes.data], [(5, 3)], [15], [a.ctypes.data, b.ctypes.data], [0, 0], [15, 15], [0, 0], ops) == J.MDJPEG_OK
        assert tuple(a[1, 2]) == colour and tuple(a[0, 2]) == (0, 0, 255) and tuple(a[1, 1]) == (255, 0, 0)
        np.testing.assert_array_equal(b, src)


def _refused(c, srcs, dsts, **changes):
    args = list(D.call_arguments(c, [b.ctypes.data for b in srcs], [b.ctypes.data for b in dsts]))
    names = ['src_ptrs', 'sizes', 'src_pitches', 'dst_ptrs', 'dst_src', 'dst_pitches', 'op_image', 'ops']
    patches = changes.pop('patches', c['patches'])
    for k, v in changes.items():
        args[names.index(k)] = v
    return J.draw_ops_from(*args, patches)


def test_overlaps_and_bad_operations_are_refused_with_nothing_written():
    c = D.case(33, 17, 5, 1)
    srcs = [D.aligned_copy(b) for b in D.source_buffers(c)]
    dsts = [D.aligned_copy(b) for b in D.dest_buffers(c)]
    ptrs = D.call_arguments(c, [b.ctypes.data for b in srcs], [b.ctypes.data for b in dsts])[3]
    s0 = srcs[0].ctypes.data + D.LEAD
    last_row = s0 + (17 - 1) * (33 * 3 + 5)
    cases = {
        'a destination on its source': dict(dst_ptrs=[s0] + ptrs[1:]),
        'a destination that begins in the last row of a source': dict(dst_ptrs=[last_row + 98] + ptrs[1:]),
        'two destinations that share a byte': dict(dst_ptrs=[ptrs[0], ptrs[0] + D.extent(33, 17, 104) - 1] + ptrs[2:]),
        'dst_src out of range': dict(dst_src=[0, 2, 0, 1]),
        'dst_src negative': dict(dst_src=[-1, 0, 0, 1]),
        'an operation for a destination that is not there': dict(op_image=[4] + c['op_image'][1:]),
        'an unknown kind': dict(ops=[[2, 0, 0, 1, 1, 0, 0, 0]] + c['ops'][1:]),
        'a patch beyond patches': dict(patches=c['patches'][:-1]),
        'a destination pitch below a row': dict(dst_pitches=[98, 104, 104, 23]),
    }
    for what, changes in cases.items():
        assert _refused(c, srcs, dsts, **changes) == J.MDJPEG_EINVAL, what
        for got, want in zip(dsts, D.dest_buffers(c)):
            np.testing.assert_array_equal(got, want, err_msg=what)
        for got, want in zip(srcs, D.source_buffers(c)):
            np.testing.assert_array_equal(got, want, err_msg=what)
    # the same buffers with nothing changed are accepted, and so are two names for one source
    assert _refused(c, srcs, dsts) == J.MDJPEG_OK
    assert _refused(c, srcs, dsts, src_ptrs=[s0, s0, srcs[1].ctypes.data + D.LEAD], sizes=[(33, 17), (33, 17), (6, 2)],
                    src_pitches=[104, 104, 18], dst_src=[0, 1, 0, 2]) == J.MDJPEG_OK
    for got, want in zip(dsts, D.copy_then_draw(c)):
        np.testing.assert_array_equal(got, want)


def test_header_library_and_tables_name_the_call():
    from megadetector_amd import _lib
    assert 'mdhip_draw_ops_from' in _lib.SYMBOLS and 'mdjpeg_draw_from' in J.SYMBOLS
    for header, name in (('mdhip.h', 'mdhip_draw_ops_from'), ('mdjpeg.h', 'mdjpeg_draw_from')):
        assert name + '(' in open(os.path.join(REPO, 'include', header)).read()


def test_host_model_under_the_sanitizers(tmp_path):
    """mdjpeg_draw_from in a build of image_host.cpp with AddressSanitizer + UBSan, as a program of its own: the sizes, pitches,
    alignments and operations of the cases above on heap images of their exact sizes, and the refusals"""
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'jpeg_entropy_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-jpeg', 'ASAN_OUT=' + exe])
    r = subprocess.run([exe, '--draw-from'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'draw-from: 40 runs' in r.stdout
