"""
mdhip_set_option "pw_stream" on the CPU: the streaming body of the 160 -> 160 channel 1x1 convs is chosen inside the tile's
kernel family at launch, so nothing mdhip_launches_describe writes may depend on the switch -- the benchmark's forward is the
recorded text with it on and off, and so is the forward of the probe network tests/test_gpu_pw_stream.py runs, whose forced
tiles and in-place upsample that test relies on.
"""

import ctypes as C

import pytest

import test_launches_cpu as L

from megadetector_amd import _lib, hip_backend, weights_io


@pytest.mark.parametrize('case', ['bench_bf16_32x1280x1280', 'bench_fp16_32x1280x1280', 'x6_bf16_2x1280x1280'])
def test_the_described_forward_does_not_depend_on_the_switch(case):
    on, off = L._describe(case, pw_stream=True), L._describe(case, pw_stream=False)
    assert on == off
    assert on == L._recorded(case)
    # the launches the body is for are there, under the tiles they always had
    lines = [l for l in on.splitlines() if ' launch ' in l and ' m=' in l and ' n=160 k=160 ' in l]
    if case.startswith('bench'):
        assert len(lines) == 14, lines
    if case == 'bench_bf16_32x1280x1280':
        assert sorted({l.split('cfg=')[1].split()[0] for l in lines}) == ['v2:128x160/2x2', 'v2:320x160/4x2']


def test_the_probe_network_of_the_gpu_test():
    import test_gpu_pw_stream as G
    W = weights_io.synthetic_weights(G.NET_S, seed=5)
    shape = G.SHAPES[1]
    args = (W, 'bf16', G.CAPACITY, None) + shape
    plain = hip_backend.describe_launches(*args)
    rows = [l.split() for l in plain.splitlines()]
    pointwise = [int(r[1]) for r in rows if ' n=160 ' in ' '.join(r) + ' ' and (' k=160 ' in ' '.join(r) + ' ' or ' k=320 ' in ' '.join(r) + ' ')]
    up = [int(r[1]) for r in rows if 'upsample' in ' '.join(r)]
    assert len(pointwise) == 5 and len(up) == 1, plain
    forced = {op: G.TILE for op in pointwise}
    forced[max(pointwise)] = G.TILE_UP                       # the reader is the last of them
    texts = [hip_backend.describe_launches(*args, forced=forced, pw_stream=v) for v in (True, False)]
    assert texts[0] == texts[1]
    lines = texts[0].splitlines()
    assert sum('cfg=' + G.TILE + ' ' in l for l in lines) == 4 and sum('cfg=' + G.TILE_UP + ' ' in l for l in lines) == 1, texts[0]
    assert ' in_place ' in lines[up[0]], lines[up[0]]


def test_option_names_without_a_context():
    """no context: MDHIP_EINVAL for a known name and an unknown one alike, as before"""
    lib = _lib.load()
    for name in (b'pw_stream', b'fuse_decode', b'no_such_option'):
        assert lib.mdhip_set_option(None, name, 1) == lib.mdhip_set_option(None, b'letterbox_general', 1) < 0
    assert _lib.MDHIP_LAUNCHES_NO_PW_STREAM == 128
    assert 'variant' in [f for f, _ in _lib.mdhip_op_info._fields_]
    assert C.sizeof(_lib.mdhip_op_info) == 112
