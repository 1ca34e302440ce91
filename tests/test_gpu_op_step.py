"""
A forward op by op on the GPU (tests/op_step.py; tests/test_op_step_cpu.py shows that the checker bites): the library steps its
own plan with mdhip_run_ops -- every op its own launch --, each op is read before and after (mdhip_read_op_tensor) and compared
with a float64 or exact evaluation of that ONE op on what it read, the weights it multiplied are read back from the device
(mdhip_read_op_weights).

  1. network C at seven shapes, which between them reach the four launches of launch_sppf_pool; then the stepped pass against a
     forward of the same context, bit for bit;
  2. the convs with a residual under every tile configuration that claims them;
  3. the small YOLO11 and YOLOv9 models: every op kind the anchor-free models add;
  4. the error returns of the three entry points.

The arenas are poisoned (MDHIP_ARENA_POISON=1), graph replay is off.  Figures (what ran, worst err / tol per op kind and storage
type) are recorded in profiles/op_step_tests.txt.
"""

import ctypes as C
import os

import numpy as np
import pytest

import op_step as S
import parity_util as PU

from megadetector_amd import _lib, weights_io, yolo_yaml
from megadetector_amd.hip_backend import HipContext, HipError

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']
RESIDUAL_SHAPES = [(3, 24, 40), (2, 88, 104)]
#: the models of test_yolo11n_layers and test_small_nets_layers, at the smaller of their two shapes, two images
ANCHOR_FREE = ['YOLO11N_TEST', 'GELAN_TEST', 'YOLOV9_DUAL_TEST']
ANCHOR_FREE_SHAPE = (2, 480, 640)


def _poisoned_context(W, dtype, capacity):
    before = os.environ.get('MDHIP_ARENA_POISON')
    os.environ['MDHIP_ARENA_POISON'] = '1'
    try:
        ctx = HipContext(W, dtype=dtype, max_batch=capacity[0], max_h=capacity[1], max_w=capacity[2])
    finally:
        if before is None:
            del os.environ['MDHIP_ARENA_POISON']
        else:
            os.environ['MDHIP_ARENA_POISON'] = before
    ctx.set_graph('off')
    return ctx


class Stepped:
    """one context of a model with its plan and checker"""

    def __init__(self, W, dtype, capacity):
        self.W, self.dtype = W, dtype
        self.plan = S.plan_of(W, dtype, capacity)
        self.checker = S.StepChecker(W, dtype)
        self.ctx = _poisoned_context(W, dtype, capacity)
        assert self.ctx.num_ops() == len(self.plan['ops'])

    def feed(self, imgs, shape):
        n, h, w = shape
        self.ctx.preprocess(imgs, [(h, w, h, w, 0, 0)] * n, h, w)

    def source(self, shape):
        return S.HipStepSource(self.ctx, shape, self.plan)


@pytest.fixture(scope='module')
def stepped():
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            if name == 'C':
                made[name, dtype] = Stepped(S.weights_c(), dtype, S.CAPACITY_C)
            else:
                made[name, dtype] = Stepped(weights_io.synthetic_weights(getattr(yolo_yaml, name), seed=0), dtype, ANCHOR_FREE_SHAPE)
        return made[name, dtype]
    yield get
    for s in made.values():
        s.ctx.close()


def _report(title, res):
    print('\n' + title)
    worst = res.worst()
    for kind in sorted(worst):
        print('  worst {}: {}'.format(kind, worst[kind]))
    for op, name, why in res.excluded:
        print('  excluded: op {} "{}": {}'.format(op, name, why))


def _shape_id(shape):
    return 'x'.join(str(v) for v in shape)


# ---------------------------------------------------------------------------------------------------------------------
# 1. network C, step by step
# ---------------------------------------------------------------------------------------------------------------------

def test_shapes_cover_the_four_pool_launches():
    # the rule of launch_sppf_pool (misc_kernels.cpp), from the map size alone -- the library is not asked which one ran: an
    # 8-channel chunk of an h x w map takes h * w * 32 bytes of LDS; four chunks a workgroup while they fit 64 KiB (h * w <= 512),
    # two of them when h * w is in 256 .. 512; one chunk while that fits (h * w <= 2048); else three chained launches
    launches = [S.sppf_launch(h // 2, w // 2) for _, h, w in S.SHAPES_C]
    assert launches == ['<4>', '<4>', '<2>', '<2>', '<1>', '<1>', 'chained']
    assert set(launches) == {'<4>', '<2>', '<1>', 'chained'}


@pytest.mark.parametrize('shape', S.SHAPES_C, ids=_shape_id)
@pytest.mark.parametrize('dtype', DTYPES)
def test_network_c_step_by_step(stepped, dtype, shape):
    p = stepped('C', dtype)
    ctx, n = p.ctx, shape[0]
    p.feed(S.images_c(shape), shape)
    res = p.checker.check_all(p.source(shape))
    _report('C {} {} (SPPF map {}x{}, launch {}):'.format(dtype, shape, shape[1] // 2, shape[2] // 2,
                                                            S.sppf_launch(shape[1] // 2, shape[2] // 2)), res)
    print(res.report())
    assert not res.failures(), '\n' + '\n'.join(res.failures())
    assert len(res.verdicts) + len(res.excluded) == ctx.num_ops()
    assert [name for _, name, _ in res.excluded] == ['L0 stem 6x6s2 (3x3 s2d)']
    exact = [v for v in res.verdicts if v.kind in ('pool', 'upsample', 'copy')]
    assert len(exact) == 3 and all(isinstance(v, S.Exact) and v.over == 0 for v in exact)
    assert len(res.pins) == 2 * sum(o['kind'] == S.CONV for o in p.plan['ops']) and not any(v.over for v in res.pins)
    pool = [o for o in p.plan['ops'] if o['kind'] == S.POOL][0]
    assert S.padding_shows(ctx.read_op_tensor(pool['op'], S.IN, n), pool['pool_k']), 'the pool input does not show the padding'
    # the stepped pass ran the forward's launches: the same context, fusion off, gives the same bits everywhere
    layers = [i for i, v in enumerate(p.plan['layers']) if v.valid]
    stepped_layers = {i: ctx.read_layer(i, n) for i in layers}
    stepped_pred = ctx.read_predictions(n)
    try:
        ctx.set_fuse(0)
        ctx.forward(*shape)
        for i in layers:
            assert np.array_equal(ctx.read_layer(i, n).view(np.uint32), stepped_layers[i].view(np.uint32)), ('layer', i)
        assert np.array_equal(ctx.read_predictions(n).view(np.uint32), stepped_pred.view(np.uint32))
    finally:
        ctx.set_fuse(1)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the convs with a residual under every configuration that claims them
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', RESIDUAL_SHAPES, ids=_shape_id)
@pytest.mark.parametrize('dtype', DTYPES)
def test_residual_convs_under_every_family(stepped, dtype, shape):
    p = stepped('C', dtype)
    ctx = p.ctx
    p.feed(S.images_c(shape), shape)
    ctx.run_ops(*shape, 0, ctx.num_ops())             # (op_supports_cfg evaluates at the last finished pass's shape: this one)
    convs = [o['op'] for o in p.plan['ops'] if o['kind'] == S.CONV]
    with_res = [o['op'] for o in p.plan['ops'] if o['kind'] == S.CONV and o['has_res']]
    assert len(with_res) == 5
    cfgs = {ctx.conv_cfg_name(c): c for c in range(ctx.num_conv_cfgs())}
    ran, worst = [], None
    try:
        for name, cfg in cfgs.items():
            switched = [op for op in with_res if ctx.op_supports_cfg(op, cfg)]
            if not switched:
                continue
            for op in convs:
                ctx.set_op_cfg(op, cfg if op in switched else -1)
            try:
                res = p.checker.check_all(p.source(shape), only=set(switched), what=name)
            except HipError as e:
                pytest.fail('{} claims {} but its launch fails: {}'.format(name, [p.plan['ops'][op]['name'] for op in switched], e))
            now = ctx.op_infos()
            wrong = [(now[op]['name'], ctx.conv_cfg_name(now[op]['cfg'])) for op in switched if now[op]['cfg'] != cfg]
            assert not wrong, (name, 'ops that did not run the forced configuration', wrong)
            assert [v.op for v in res.verdicts] == switched and all(v.kind == 'conv + residual' for v in res.verdicts)
            assert not res.failures(), '\n' + '\n'.join(res.failures())
            ran.append((name, switched))
            for v in res.verdicts:
                if worst is None or v.worst > worst.worst:
                    worst = v
    finally:
        for op in convs:
            ctx.set_op_cfg(op, -1)
    assert ran, 'no configuration claims a conv with a residual'
    print('\nC {} {}: {} configurations ran on the convs with a residual, {} forced launches'.format(
        dtype, shape, len(ran), sum(len(s) for _, s in ran)))
    for name, switched in ran:
        print('  {:28s} {}'.format(name, ' '.join(str(op) for op in switched)))
    print('  worst among the forced ops: {}'.format(worst))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the small anchor-free models
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ANCHOR_FREE)
@pytest.mark.parametrize('dtype', DTYPES)
def test_anchor_free_models_step_by_step(stepped, dtype, name):
    p = stepped(name, dtype)
    n, h, w = ANCHOR_FREE_SHAPE
    imgs = PU.structured_images(n, h, w, seed=4)
    x, infos = PU.oracle_input(imgs, 640, 32)
    assert x.shape == (n, 3, h, w)
    p.feed([np.ascontiguousarray(i['img_processed']) for i in infos], ANCHOR_FREE_SHAPE)
    res = p.checker.check_all(p.source(ANCHOR_FREE_SHAPE))
    _report('{} {} {}: {} ops'.format(name, dtype, ANCHOR_FREE_SHAPE, res.num_ops), res)
    kinds = {}
    for v in res.verdicts:
        kinds[v.kind] = kinds.get(v.kind, 0) + 1
    print('  verdicts: ' + ', '.join('{} {}'.format(kinds[k], k) for k in sorted(kinds)))
    assert not res.failures(), '\n' + '\n'.join(res.failures())
    assert len(res.verdicts) + len(res.excluded) == p.ctx.num_ops()
    assert res.excluded and all(p.plan['ops'][op]['stem'] for op, _, _ in res.excluded)
    # (the dual form lowers the auxiliary branch only: its SPPELAN and upsamples feed the head that does not run)
    need = {'conv', 'conv + residual', 'conv fp32 out', 'dfl decode'}
    need |= {'YOLO11N_TEST': {'pool', 'upsample', 'depthwise', 'attention'}, 'GELAN_TEST': {'pool', 'upsample', 'adown'},
             'YOLOV9_DUAL_TEST': {'adown', 'cbfuse'}}[name]
    assert need <= set(kinds), sorted(need - set(kinds))


# ---------------------------------------------------------------------------------------------------------------------
# 4. error returns
# ---------------------------------------------------------------------------------------------------------------------

def test_error_returns_do_not_poison_the_context(stepped):
    p = stepped('C', 'bf16')
    ctx, lib = p.ctx, p.ctx.lib
    shape = (3, 24, 40)
    n, h, w = shape
    p.feed(S.images_c(shape), shape)
    ctx.forward(*shape)
    want = ctx.read_predictions(n)
    ops = p.plan['ops']
    n_ops = len(ops)
    pool = [o['op'] for o in ops if o['kind'] == S.POOL][0]
    decode = [o['op'] for o in ops if o['kind'] == S.DECODE][0]
    plain = [o['op'] for o in ops if o['kind'] == S.CONV and not o['has_res'] and not o['stem']][0]
    c, hh, ww = C.c_int(), C.c_int(), C.c_int()
    dims = (C.byref(c), C.byref(hh), C.byref(ww))
    buf = np.empty(1 << 20, dtype=np.float32)
    EINVAL = _lib.MDHIP_EINVAL
    for first, count in ((-1, 1), (n_ops + 1, 0), (n_ops, 1), (0, n_ops + 1), (3, -1), (n_ops - 1, 2)):
        assert lib.mdhip_run_ops(ctx.h, n, h, w, first, count, None) == EINVAL, (first, count)
    assert lib.mdhip_run_ops(ctx.h, n, h + 1, w, 0, 1, None) == EINVAL              # the shape checks of the forwards
    assert lib.mdhip_run_ops(ctx.h, n + 1, h, w, 0, 1, None) == EINVAL
    assert lib.mdhip_run_ops(ctx.h, n, h, w, n_ops, 0, None) == 0                   # the empty range at the end is a range
    for op, which in ((-1, 0), (n_ops, 0), (plain, -1), (plain, 7), (plain, S.RES), (plain, S.OUT2), (plain, S.FSRC0),
                      (decode, S.IN), (decode, S.OUT)):
        assert lib.mdhip_read_op_tensor(ctx.h, op, which, n, _lib.np_ptr(buf), *dims, None) == EINVAL, (op, which)
    assert lib.mdhip_read_op_tensor(ctx.h, plain, S.OUT, n + 1, _lib.np_ptr(buf), *dims, None) == EINVAL
    for op in (-1, n_ops, pool, decode):
        assert lib.mdhip_read_op_weights(ctx.h, op, None, None, None, None, None, None) == EINVAL, op
    assert b'mdhip_read_op_weights' in lib.mdhip_last_error(ctx.h)
    # shape queries write nothing
    assert lib.mdhip_read_op_tensor(ctx.h, pool, S.OUT, n, None, *dims, None) == 0
    assert (c.value, hh.value, ww.value) == (96, h // 2, w // 2)
    ctx.forward(*shape)
    assert np.array_equal(ctx.read_predictions(n).view(np.uint32), want.view(np.uint32))
    res = p.checker.check_all(p.source(shape))
    assert not res.failures(), '\n' + '\n'.join(res.failures())
    assert np.array_equal(ctx.read_predictions(n).view(np.uint32), want.view(np.uint32))
