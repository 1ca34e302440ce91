"""
tests/conv_probe.py without a GPU: the probe networks plan, the float64 reference of one conv op agrees with an independent
statement of it, a correct fp32 kernel (torch float32, in two summation orders) stays inside the bound on every element of
every layer of both networks in both storage types, and each planted mistake of MUTANTS is caught.  What the library itself
computes is tests/test_gpu_conv_probe.py's matter.
"""

import functools
import re

import numpy as np
import pytest

import conv_probe as P

DTYPES = ['bf16', 'fp16']

#: (name, m, n, k) of every op of a forward at the probe shape, as mdhip_launches_describe reports them (both storage types)
OPS = {
    'A': [
        ('L0 stem 6x6s2 (3x3 s2d)', 5760, 80, 108),
        ('L1 conv 3x3s1', 5760, 80, 720),
        ('L2 conv 1x1s1', 5760, 128, 80),
        ('L3 conv 3x3s2', 1440, 160, 1152),
        ('L4 conv 3x3s2', 1440, 160, 720),
        ('L6 conv 3x3s1', 1440, 320, 2880),
        ('L7 conv 1x1s1', 1440, 64, 320),
        ('L8 conv 3x3s2', 360, 160, 576),
        ('L9 conv 3x3s2', 360, 160, 2880),
        ('L10 conv 1x1s1', 1440, 72, 320),
        ('L11 conv 3x3s2', 360, 160, 648),
        ('L13 Detect.m0 1x1', 1440, 24, 320),
        ('L13 Detect.decode0', 0, 0, 0),
        ('L13 Detect.m1 1x1', 360, 24, 480),
        ('L13 Detect.decode1', 0, 0, 0),
    ],
    'B': [
        ('L0 stem 3x3s2 (3x3 s2d)', 5616, 32, 27),
        ('L1 conv 3x3s2', 1404, 64, 288),
        ('L2 conv 1x1s1', 1404, 72, 64),
        ('L3 conv 3x3s1', 1404, 200, 648),
        ('L4 conv 3x3s1', 1404, 24, 1800),
        ('L5 conv 1x1s1', 1404, 40, 200),
        ('L7 conv 3x3s2', 351, 160, 576),
        ('L8 conv 3x3s1', 351, 640, 1440),
        ('L9 conv 3x3s1', 351, 640, 5760),
        ('L10 conv 1x1s1', 351, 8, 640),
        ('L11 upsample x2', 0, 0, 0),
        ('L13 conv 1x1s1', 1404, 48, 840),
        ('L14 Detect.m0 1x1', 1404, 24, 64),
        ('L14 Detect.decode0', 0, 0, 0),
        ('L14 Detect.m1 1x1', 1404, 24, 48),
        ('L14 Detect.decode1', 0, 0, 0),
        ('L14 Detect.m2 1x1', 351, 24, 8),
        ('L14 Detect.decode2', 0, 0, 0),
    ],
}


@pytest.fixture(scope='module', autouse=True)
def _built():
    import __graft_entry__ as G
    G.build()


@functools.lru_cache(maxsize=None)
def _weights(net):
    return P.weights(net)


# ---- planning -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', list(P.NETS))
def test_probe_networks_plan_one_conv_op_per_layer(net, dtype):
    from megadetector_amd import hip_backend
    W = _weights(net)
    n, h, w = P.NETS[net]['shape']
    cap = P.NETS[net]['capacity']
    plan = hip_backend.describe_plan(W, dtype, *cap)
    assert 'fuse_groups 0' in plan                          # (no C3 block: nothing to fuse)
    text = hip_backend.describe_launches(W, dtype, cap, None, n, h, w)
    ops = [(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))
           for m in re.finditer(r'op \d+ "([^"]*)" \S+ cfg=\S+ table=\d decodes=\d m=(\d+) n=(\d+) k=(\d+)', text)]
    assert ops == OPS[net]
    # every Conv row is exactly one op (nothing pruned: each feeds a Detect level), named after its layer
    for i in P.conv_layers(W):
        assert sum(name.startswith('L{} '.format(i)) for name, *_ in ops) == 1, i
    # K as the bound counts it (c_in * kh * kw of the fp32 weights) is the K the library reports
    ck = P.Checker(W, dtype)
    for name, _, _, k in ops:
        layer = int(name.split()[0][1:])
        if ' conv ' in name or ' stem ' in name:
            assert ck.K(layer) == k, name
        elif 'Detect.m' in name:
            assert ck.K(layer, int(name.split('Detect.m')[1].split()[0])) == k, name


def test_every_configuration_name_is_of_a_known_family():
    """a new tile family must be added to the probe cases (PUBLIC_FAMILIES) before its name parses here"""
    from megadetector_amd import _lib
    lib = _lib.load()
    names = [lib.mdhip_conv_cfg_name(i).decode() for i in range(lib.mdhip_num_conv_cfgs())]
    fams = {P.family(n) for n in names}
    assert fams == set(P.PUBLIC_FAMILIES) | {'dev', 'f8'}, fams
    for n in names:
        bm, bn = P.tile_of(n)
        assert bm in (64, 96, 128, 160, 192, 256, 320) and bn in (32, 64, 80, 128, 160, 320), (n, bm, bn)


# ---- the reference and the bound ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('k,stride', [(3, 1), (3, 2), (1, 1)])
def test_reference_equals_explicit_loops(k, stride):
    rng = np.random.default_rng(3 + k + stride)
    n, c, h, w, o = 2, 8, 5, 7, 6
    a = rng.standard_normal((n, c, h, w)).astype(np.float32)
    wt = rng.standard_normal((o, c, k, k)).astype(np.float32)
    b = rng.standard_normal(o).astype(np.float32)
    pad = k // 2
    y, z, S = P.conv_reference(a, wt, b, stride, pad)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    assert z.shape == (n, o, ho, wo)
    zl, Sl = np.zeros(z.shape), np.zeros(z.shape)
    for i in range(n):
        for q in range(o):
            for oy in range(ho):
                for ox in range(wo):
                    acc, mag = float(b[q]), abs(float(b[q]))
                    for ch in range(c):
                        for dy in range(k):
                            for dx in range(k):
                                iy, ix = oy * stride + dy - pad, ox * stride + dx - pad
                                if 0 <= iy < h and 0 <= ix < w:                      # zero padding
                                    t = float(a[i, ch, iy, ix]) * float(wt[q, ch, dy, dx])
                                    acc += t
                                    mag += abs(t)
                    zl[i, q, oy, ox], Sl[i, q, oy, ox] = acc, mag
    np.testing.assert_allclose(z, zl, rtol=0, atol=1e-13 * Sl.max())
    np.testing.assert_allclose(S, Sl, rtol=1e-13)
    np.testing.assert_allclose(y, zl / (1 + np.exp(-zl)), rtol=0, atol=1e-13 * Sl.max())


def test_storage_ulps_and_tolerance():
    assert P.ulp_storage(1.0, 'bf16') == 2.0 ** -7 and P.ulp_storage(1.0, 'fp16') == 2.0 ** -10
    assert P.ulp_storage(1.99, 'bf16') == 2.0 ** -7 and P.ulp_storage(2.0, 'bf16') == 2.0 ** -6
    assert P.ulp_storage(0.75, 'fp16') == 2.0 ** -11
    assert P.ulp_storage(0.0, 'fp16') == 2.0 ** -24 and P.ulp_storage(2.0 ** -20, 'fp16') == 2.0 ** -24     # subnormal spacing
    assert P.ulp_storage(0.0, 'bf16') == 2.0 ** -133
    assert P.ulp_f32(1.0) == 2.0 ** -23
    # the storage rounding agrees with those spacings: rounding moves a value by at most half of one
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 3
    for dtype in DTYPES:
        assert (np.abs(P.round_storage(x, dtype).astype(np.float64) - x) <= P.ulp_storage(np.abs(x), dtype) / 2).all()
        assert P.is_storage(P.round_storage(x, dtype), dtype) and not P.is_storage(x, dtype)
    # an exact result leaves half a storage ulp and no more: z = 1.5, S = 2, K = 16 in bf16
    z = np.array([1.5])
    y = z / (1 + np.exp(-z))
    tol = P.conv_tolerance(y, z, np.array([2.0]), 16, 'bf16')
    E = 1.1 * 20 * 2.0 ** -24 * 2 + 11 * 2.0 ** -24 * y
    np.testing.assert_allclose(tol, E + 2.0 ** -8, rtol=1e-15)             # y = 1.226 lies in [1, 2): ulp 2^-7
    # a NaN or an infinity in the output is over every bound
    v = P.Verdict('x', 1, np.array([np.nan, 1.0, np.inf]), np.array([1.0, 1.0, 1.0]), np.array([0.1, 0.1, 0.1]))
    assert v.over == 2


# ---- a correct kernel passes --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _checker(net, dtype):
    return P.Checker(_weights(net), dtype)


@pytest.mark.parametrize('conv', [P.conv_f32, P.conv_f32_blocks], ids=['torch_f32', 'blocks_of_32_reversed'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', list(P.NETS))
def test_a_correct_fp32_kernel_is_inside_the_bound(net, dtype, conv):
    """(worst err / tol comes out just below 1 -- half a storage ulp is most of the bound -- so no ratio below 1 is asked)"""
    em = P.Emulated(_weights(net), dtype, P.input_tensor(net), conv=conv)
    verdicts = _checker(net, dtype).check(em, conv.__name__)
    assert len(verdicts) == len(P.conv_layers(_weights(net))) + len(_weights(net).strides)
    assert not P.failures(verdicts), '\n'.join(P.failures(verdicts))
    assert all(np.isfinite(v.worst) and v.worst > 0 for v in verdicts)
    worst = max(v.worst for v in verdicts if 'Detect' not in v.what)
    print('\n{} {} {}: worst err / tol {:.3f}'.format(net, dtype, conv.__name__, worst))


def test_the_two_summations_differ():
    """the second summation order is another kernel, not the first again: some layer's stored output differs"""
    W = _weights('B')
    a = P.Emulated(W, 'fp16', P.input_tensor('B'))
    b = P.Emulated(W, 'fp16', P.input_tensor('B'), conv=P.conv_f32_blocks)
    assert any(not np.array_equal(a.layer(i), b.layer(i)) for i in P.conv_layers(W))


# ---- planted mistakes are caught ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutant', P.MUTANTS)
def test_mutant_is_flagged(mutant, dtype):
    flagged, table = {}, []
    for net in P.NETS:
        W = _weights(net)
        em = P.Emulated(W, dtype, P.input_tensor(net), mutant=mutant)
        for v in _checker(net, dtype).check(em, mutant):
            flagged[net, v.key] = v
            if v.over:
                table.append('{} {}'.format(net, v))
    print('\n{} {}: {} of {} checks flag it'.format(mutant, dtype, len(table), len(flagged)))
    for line in table:
        print('  ' + line)
    assert table, 'no layer of either network flags {}'.format(mutant)
    if mutant == 'truncating_store':
        # The accumulation term of the bound grows with K: at K = 2880 it exceeds the half ulp that truncation adds, and
        # truncation is legitimately invisible there.  The rounding of an epilogue is therefore held sharply where
        # K <= SHARP_K only, and there it must be seen on every layer (the fp32 Detect outputs are not stored in 16 bits).
        sharp = [v for (net, key), v in flagged.items() if not isinstance(key, tuple) and v.K <= P.SHARP_K]
        assert len(sharp) >= 4, [str(v) for v in sharp]
        assert all(v.over for v in sharp), [str(v) for v in sharp if not v.over]
    if mutant == 'concat_slice_8_channels_off':
        # exactly the layers that write a slice of a concat buffer
        assert {k for k, v in flagged.items() if v.over and not isinstance(k[1], tuple)} == \
            {('A', 3), ('A', 4), ('A', 8), ('A', 9), ('A', 11), ('B', 4), ('B', 5), ('B', 3)}
    if mutant == 'n_tail_left_at_zero':
        assert {k for k, v in flagged.items() if v.over and not isinstance(k[1], tuple)} == \
            {('A', 10), ('B', 2), ('B', 3), ('B', 4), ('B', 5), ('B', 10)}
