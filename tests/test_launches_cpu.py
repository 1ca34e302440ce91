"""The executor's decisions on the CPU: what a forward launches (which tile each conv runs, which bottlenecks run fused, which
upsamples are read in place, which Detect convs decode in their epilogue, the statistics mdhip_get_op_info reports), against
records made by the executor of the commit BEFORE decisions and launches were separated in mdhip_exec.cpp.

hip_backend.describe_launches (mdhip_launches_describe) plans a context without a device, resolves one forward on it and writes
one line per op.  tests/golden/launches/ holds one text per case of CASES below (<case>.txt.gz: gzip, `zcat` shows it; a text
is one line per op, at most a few hundred lines, so every case is kept whole), for the synthetic weights of weights_io (seed 1;
values do not enter a decision).  A change of the executor that is meant to keep what runs must leave every one of them equal.
A change that is meant to alter a decision (a re-tune, a new kernel family, another heuristic) records them again:
`python tests/test_launches_cpu.py record` writes the files from the library that is built -- run it on a build of the commit
whose decisions are the reference (with mdhip_launches_describe available there), never to make a failing comparison pass.
tests/golden/bench_tiles.json, recorded on the GPU by tools/dump_bench_tiles.py, pins the nine benchmark workloads a second
time, independently of this file's records.
"""

import functools
import gzip
import json
import os
import re
import sys

import pytest

from conftest import GOLDEN

LAUNCHES = os.path.join(GOLDEN, 'launches')
SEED = 1
X6 = 'YOLOV5X6_MD'
BENCH = [('bf16', 32, 1280, 1280), ('bf16', 32, 768, 1280), ('bf16', 32, 960, 1280), ('bf16', 32, 896, 1280),
         ('fp16', 32, 1280, 1280), ('fp16', 32, 768, 1280), ('fp16', 32, 960, 1280), ('fp16', 32, 896, 1280),
         ('fp8', 64, 1280, 1280)]                 # tools/dump_bench_tiles.py WORKLOADS
TOYS = ['YOLOV5N6_TEST', 'YOLOV5N_P5_TEST', 'YOLOV5S6_TEST', 'YOLO11N_TEST', 'GELAN_TEST', 'YOLOV9_DUAL_TEST']
SMALL = (2, 256, 320)


def _case(model, dtype, cap, shape, table='own', forced=None, **options):
    """table: 'own' = the shipped table of the storage type, None = none (the heuristic alone); forced: a function of the
    unforced description giving {op: configuration name}"""
    return dict(model=model, dtype=dtype, cap=cap, shape=shape, table=table, forced=forced, options=options)


def _ops_named(text, *parts):
    return [int(line.split()[1]) for line in text.splitlines() if all(p in line.split('"')[1] for p in parts)]


def _strip_on_first_block(text):          # the 3x3s of the 80-channel C3 block: the block runs fused
    ops = _ops_named(text, 'L2 C3.m', 'cv2')
    assert len(ops) == 4
    return {op: 'v5:strip160x80/2x5' for op in ops}


def _v2_behind_upsample(text):            # the 1x1 conv behind the last upsample of the head: the upsample is read in place
    up = _ops_named(text, 'L21 upsample')
    assert len(up) == 1
    return {up[0] + 1: 'v2:160x160/2x2'}


def _strip_on_a_pointwise_conv(text):     # a configuration that does not support its op (a 1x1 conv)
    ops = _ops_named(text, 'L4 C3.cv3')
    assert len(ops) == 1
    return {ops[0]: 'v5:strip160x80/2x5'}


CASES = {}
for _d, _b, _h, _w in BENCH:
    CASES['bench_{}_{}x{}x{}'.format(_d, _b, _h, _w)] = _case(X6, _d, (_b, 1280, 1280), (_b, _h, _w))
for _d in ('bf16', 'fp16'):
    for _b in (1, 2, 4, 8, 16):
        CASES['x6_{}_{}x1280x1280'.format(_d, _b)] = _case(X6, _d, (32, 1280, 1280), (_b, 1280, 1280))
    for _b in (2, 32):
        CASES['x6_{}_{}x640x640'.format(_d, _b)] = _case(X6, _d, (32, 1280, 1280), (_b, 640, 640))
for _name, _opt in [('fuse_off', dict(fuse=False)), ('fuse_decode_off', dict(fuse_decode=False)), ('pair_off', dict(pair=False)),
                    ('isolated', dict(isolated=True))]:
    CASES['x6_bf16_32x1280x1280_' + _name] = _case(X6, 'bf16', (32, 1280, 1280), (32, 1280, 1280), **_opt)
for _s in (1088, 896):                        # the two scaled passes of mdhip_forward_tta on a 1280 x 1280 input
    CASES['x6_bf16_32x{0}x{0}_augmented'.format(_s)] = _case(X6, 'bf16', (32, 1280, 1280), (32, _s, _s), augmented=True)
CASES['x6_fp8_64x1280x1280_calibrating'] = _case(X6, 'fp8', (64, 1280, 1280), (64, 1280, 1280), calibrating=True)
for _m in ('YOLO11L_MD', 'YOLO11S_MD', 'YOLOV9C_MD'):        # (HipContext loads no table for these)
    for _b in (1, 32):
        CASES['{}_bf16_{}x1280x1280'.format(_m, _b)] = _case(_m, 'bf16', (32, 1280, 1280), (_b, 1280, 1280), table=None)
for _m in TOYS:
    for _d in ('bf16', 'fp16'):
        CASES['{}_{}_2x256x320'.format(_m, _d)] = _case(_m, _d, SMALL, SMALL, table=None if 'V5' not in _m else 'own')
CASES['YOLOV5N6_TEST_fp8_2x256x320'] = _case('YOLOV5N6_TEST', 'fp8', SMALL, SMALL)
CASES['x6_bf16_2x256x320_forced_strip'] = _case(X6, 'bf16', SMALL, SMALL, forced=_strip_on_first_block)
CASES['x6_bf16_2x256x320_forced_v2'] = _case(X6, 'bf16', SMALL, SMALL, forced=_v2_behind_upsample)
CASES['x6_bf16_2x256x320_forced_unsupported'] = _case(X6, 'bf16', SMALL, SMALL, forced=_strip_on_a_pointwise_conv)


@functools.lru_cache(maxsize=2)
def _weights(model):
    from megadetector_amd import weights_io, yolo_yaml
    return weights_io.synthetic_weights(getattr(yolo_yaml, model), seed=SEED)


def _describe(case, **more):
    from megadetector_amd import hip_backend
    c = CASES[case] if isinstance(case, str) else case
    table = hip_backend.table_entries(c['dtype']) if c['table'] == 'own' else None
    args = (_weights(c['model']), c['dtype'], c['cap'], table) + tuple(c['shape'])
    options = dict(c['options'], **more)
    if c['forced']:
        options['forced'] = c['forced'](hip_backend.describe_launches(*args, **options))
    return hip_backend.describe_launches(*args, **options)


def _recorded(case):
    return gzip.open(os.path.join(LAUNCHES, case + '.txt.gz'), 'rt').read()


LINE = re.compile(r'op (\d+) "([^"]*)" (launch|in_next|in_place|in_front|plain) cfg=(\S+) table=([01]) decodes=([01]) '
                  r'm=(\d+) n=(\d+) k=(\d+) flops=(\S+) bytes=(\S+)$')


def _lines(text):
    """[(op, name, how, cfg, table, decodes, m, n, k)]"""
    out = []
    for line in text.splitlines():
        g = LINE.match(line).groups()
        out.append((int(g[0]), g[1], g[2], g[3], int(g[4]), int(g[5]), int(g[6]), int(g[7]), int(g[8])))
    return out


def _assert_same(got, want, what):
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        pytest.fail('{}: {} lines against {}; first difference at line {}:\n  got  {}\n  want {}'.format(
            what, len(g), len(w), first + 1, g[first] if first < len(g) else '<end>', w[first] if first < len(w) else '<end>'))


# ---- the tests --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module', autouse=True)
def _built():
    import __graft_entry__ as G
    G.build()


@pytest.mark.parametrize('case', sorted(CASES, key=lambda c: (CASES[c]['model'], c)))
def test_launches_are_the_recorded_ones(case):
    _assert_same(_describe(case), _recorded(case), case)


@pytest.mark.parametrize('dtype,b,h,w', BENCH, ids=['{}:{}x{}x{}'.format(*t) for t in BENCH])
def test_benchmark_tiles_are_the_ones_recorded_on_the_gpu(dtype, b, h, w):
    """an independent pin: tests/golden/bench_tiles.json comes from mdhip_get_op_info after a forward on an MI355X.  A re-tune
    that forgets tools/dump_bench_tiles.py fails here."""
    want = json.load(open(os.path.join(GOLDEN, 'bench_tiles.json')))['{}:{}x{}x{}'.format(dtype, b, h, w)]
    convs = [l for l in _lines(_describe('bench_{}_{}x{}x{}'.format(dtype, b, h, w))) if l[2] in ('launch', 'in_next')]
    # (only conv ops are `launch` or `in_next`: every other kind has no tile)
    assert ['fused' if l[2] == 'in_next' else l[3] for l in convs] == want


HISTORY = ['bench_bf16_32x1280x1280', 'bench_fp16_32x768x1280', 'bench_fp8_64x1280x1280', 'x6_bf16_1x1280x1280',
           'x6_bf16_32x1280x1280_fuse_off', 'x6_bf16_32x1280x1280_fuse_decode_off', 'x6_bf16_32x1280x1280_isolated',
           'x6_bf16_32x1088x1088_augmented', 'x6_bf16_2x256x320_forced_strip', 'x6_bf16_2x256x320_forced_v2',
           'YOLO11S_MD_bf16_1x1280x1280', 'YOLOV5S6_TEST_bf16_2x256x320']


@pytest.mark.parametrize('case', HISTORY)
def test_launches_do_not_depend_on_what_the_context_resolved_before(case):
    """MDHIP_LAUNCHES_AFTER_OTHERS: the same context first resolves this and another shape as every kind of pass and with every
    setting flipped (through the setters) and flipped back, then describes: the text is the one of a fresh context"""
    _assert_same(_describe(case, after_others=True), _recorded(case), case + ' after others')


def test_records_cover_what_they_are_meant_to_cover():
    from megadetector_amd import hip_backend
    seen = dict(fused=0, absorbed=0, decoded=0, heuristic=0, nearest_m=0, e4m3=0)
    for case, c in CASES.items():
        lines = _lines(_recorded(case))
        seen['fused'] += sum(l[2] == 'in_next' for l in lines)
        assert all(lines[l[0] + 1][2] == 'launch' and lines[l[0] + 1][3].startswith('v5:strip') for l in lines if l[2] == 'in_next')
        seen['absorbed'] += sum(l[2] == 'in_place' for l in lines)
        assert sum(l[2] == 'in_front' for l in lines) == sum(l[5] for l in lines)   # one conv decodes per decode op without a launch
        seen['decoded'] += sum(l[2] == 'in_front' for l in lines)
        if c['table'] == 'own' and not c['forced']:
            seen['heuristic'] += sum(l[2] == 'launch' and not l[4] for l in lines)
        seen['e4m3'] += sum(l[2] == 'launch' and l[3].startswith('f8:') for l in lines)
        if c['table'] == 'own' and not c['forced']:
            # a table hit through the nearest-M rules: the table holds the layer's geometry (N, K), but at no such M.  (The
            # 768 x 1280 lists are exact hits since the table was measured at that shape too; the small batches, 640 x 640
            # and the augmented passes are not.)
            at = {(e['n'], e['k'], e['m']) for e in hip_backend.table_entries(c['dtype'])}
            seen['nearest_m'] += sum(l[2] == 'launch' and l[4] and (l[7], l[8], l[6]) not in at for l in lines)
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_describe_refuses_what_the_context_would_refuse():
    from megadetector_amd import hip_backend
    from megadetector_amd._lib import HipError
    W = _weights('YOLOV5N6_TEST')
    for shape, forced in (((3, 256, 320), None), ((2, 250, 320), None), ((2, 256, 320), {1: 10 ** 6}), ((2, 256, 320), {10 ** 6: 0})):
        with pytest.raises(HipError):
            hip_backend.describe_launches(W, 'bf16', SMALL, None, *shape, forced=forced)


def record():
    os.makedirs(LAUNCHES, exist_ok=True)
    for case in CASES:
        text = _describe(case)
        with open(os.path.join(LAUNCHES, case + '.txt.gz'), 'wb') as f:
            with gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0, compresslevel=9) as g:
                g.write(text.encode())
        print(case, len(text.splitlines()), 'ops')


if __name__ == '__main__' and sys.argv[1:] == ['record']:
    record()
