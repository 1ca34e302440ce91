"""
The op-by-op checker (tests/op_step.py) without a GPU: network C is planned by the library (mdhip_plan_describe needs no device)
and stepped by EmulatedSteps, a float32 restatement over a model of the arena.  Unmutated it passes every op at every shape, for
two summation orders; each planted mistake (op_step.MUTANTS) is caught, and only on the kind of op it was planted in.  Shown
here before tests/test_gpu_op_step.py is trusted.
"""

import numpy as np
import pytest

import conv_probe as P
import op_step as S

DTYPES = ['bf16', 'fp16']
MUTANT_SHAPES = [(3, 24, 40), (2, 88, 104)]
#: the kind of verdict (or 'pin') each mutant moves, and nothing else -- but for UNWRITTEN: the 8 channels the shifted copy leaves
#: unwritten are NaN in the poisoned arena, and so are the Detect logits and predictions computed from them
MUTANT_KINDS = {
    'residual_added_before_silu': 'conv + residual', 'residual_rounded_first': 'conv + residual',
    'residual_8_channels_off': 'conv + residual', 'residual_read_after_write': 'conv + residual',
    'pool_pads_with_zero': 'pool', 'pool_window_3': 'pool', 'pool_stage_reads_slice_0': 'pool', 'pool_swaps_h_w': 'pool',
    'upsample_transposed': 'upsample', 'copy_slice_8_channels_off': 'copy', 'merged_cv1_cv2_halves_swapped': 'pin',
}
UNWRITTEN = {'copy_slice_8_channels_off': {'conv fp32 out', 'decode'}}


@pytest.fixture(scope='module')
def net():
    import __graft_entry__ as G
    G.build()
    W = S.weights_c()
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = (W, S.plan_of(W, dtype, S.CAPACITY_C), S.StepChecker(W, dtype))
        return made[dtype]
    return get


def _step(net, dtype, shape, **kw):
    W, plan, checker = net(dtype)
    src = S.EmulatedSteps(W, dtype, plan, S.input_tensor_c(shape), **kw)
    return src, checker.check_all(src)


def test_network_c_is_what_it_is_for(net):
    """the rows the issue lists, as the planner lowered them"""
    W, plan, _ = net('bf16')
    ops = plan['ops']
    names = [o['name'] for o in ops]
    assert names[0] == 'L0 stem 6x6s2 (3x3 s2d)' and ops[0]['out'].c == 48 and ops[0]['stem']
    pool = [o for o in ops if o['kind'] == S.POOL]
    assert len(pool) == 1 and pool[0]['in'].c == 24 and pool[0]['in'].div == 2 and pool[0]['pool_k'] == 5      # three 8-channel chunks
    assert pool[0]['out'].off == pool[0]['in'].off and pool[0]['out'].c == 96
    res = {o['name']: o for o in ops if o['has_res']}
    assert sorted(res) == ['L2 C3.m0.cv2 3x3', 'L2 C3.m1.cv2 3x3', 'L5 C3.m0.cv2 3x3', 'L5 C3.m1.cv2 3x3', 'L5 C3.m2.cv2 3x3']
    assert all(o['res'] == o['out'] for o in res.values()), 'the residual is read from the view the op writes'
    assert {o['out'].c for o in res.values()} == {80, 40}
    assert [o['out'].c for o in ops if o['name'] in ('L4 C3.m0.cv2 3x3', 'L9 C3.m0.cv2 3x3')] == [32, 24]
    assert sum(o['stride'] == 2 and not o['stem'] for o in ops) == 2
    assert [o['kind'] for o in ops].count(S.UPSAMPLE) == 1 and [o['kind'] for o in ops].count(S.COPY) == 1
    assert [o['kind'] for o in ops].count(S.DECODE) == 2
    assert all(o['in'].c % 8 == 0 for o in ops if not o['stem'])
    for o in ops:
        if o['kind'] == S.CONV:
            for k in S.model_convs(o['name']):
                assert k + '.weight' in W.weights, (o['name'], k)


def test_shapes_reach_all_four_pool_launches():
    # launch_sppf_pool picks by h * w alone: < 256 four chunks a workgroup, 256 .. 512 two, 513 .. 2048 one (exactly 64 KiB of
    # LDS at 2048), above that three chained launches
    want = ['<4>', '<4>', '<2>', '<2>', '<1>', '<1>', 'chained']
    maps = [(h // 2, w // 2) for _, h, w in S.SHAPES_C]
    assert [S.sppf_launch(h, w) for h, w in maps] == want
    assert {S.sppf_launch(h, w) for h, w in maps} == {'<4>', '<2>', '<1>', 'chained'}
    assert maps[0][0] < 5, 'a map shorter than the window'
    assert [h * w for h, w in maps][2:4] == [256, 512] and maps[5][0] * maps[5][1] == 2048
    assert (S.sppf_launch(15, 17), S.sppf_launch(27, 19), S.sppf_launch(2049, 1)) == ('<4>', '<1>', 'chained')
    for n, h, w in S.SHAPES_C:
        assert n <= S.CAPACITY_C[0] and h % 8 == 0 and w % 8 == 0 and h * w <= S.CAPACITY_C[1] * S.CAPACITY_C[2]


@pytest.mark.parametrize('conv', [P.conv_f32, P.conv_f32_blocks], ids=['direct', 'blocks'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_unmutated_emulation_passes(net, dtype, conv):
    """every op of network C at the seven shapes: no element over its bound, pools / upsample / copy bit-exact, the packing pins
    hold; every op has a verdict or is the stem; and at every shape the pool's padding is visible in its input"""
    for shape in S.SHAPES_C:
        src, res = _step(net, dtype, shape, conv=conv)
        assert not res.failures(), '\n'.join([str(shape)] + res.failures())
        assert len(res.verdicts) + len(res.excluded) == res.num_ops
        assert [name for _, name, _ in res.excluded] == ['L0 stem 6x6s2 (3x3 s2d)']
        assert {v.kind for v in res.verdicts} == {'conv', 'conv + residual', 'conv fp32 out', 'pool', 'upsample', 'copy', 'decode'}
        assert len(res.pins) == 2 * sum(o['kind'] == S.CONV for o in src.plan['ops'])
        pool = [o for o in src.plan['ops'] if o['kind'] == S.POOL][0]
        x = src.tensor(pool['op'], S.IN)
        assert S.padding_shows(x, pool['pool_k']), (shape, 'a zero-padded pool equals the -inf-padded one')
        assert not np.isnan(src.predictions()).any()


@pytest.mark.parametrize('shape', MUTANT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mutant', S.MUTANTS)
def test_mutant_is_caught(net, mutant, dtype, shape):
    """residual_rounded_first (SiLU rounded to storage, added, rounded again) is within half a storage ulp of the reference
    wherever the first rounding is small against the last; it shows where the residual cancels most of the SiLU.  The synthetic
    C3 weights of network C (seed 5, default gains) give such elements at both storage types and both shapes: nothing was
    chosen for it."""
    _, res = _step(net, dtype, shape, mutant=mutant)
    bad = [v for v in res.verdicts + res.pins if v.over]
    assert bad, '{} is not caught'.format(mutant)
    kinds = {v.kind for v in bad}
    assert MUTANT_KINDS[mutant] in kinds and kinds <= {MUTANT_KINDS[mutant]} | UNWRITTEN.get(mutant, set()), [str(v) for v in bad]
    print('\n{} {} {}: caught on {} op(s), e.g. {}'.format(mutant, dtype, shape, len({v.op for v in bad}), bad[0]))


def test_decode_interval_holds_a_float32_decode_and_catches_a_shifted_grid(net):
    W, _, _ = net('bf16')
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((2, W.na * (W.nc + 5), 5, 7)) * 6).astype(np.float32)
    lo, hi = S.decode_interval(z, 1, W)
    s = 1 / (1 + np.exp(-z.reshape(2, W.na, W.nc + 5, 5, 7).transpose(0, 1, 3, 4, 2), dtype=np.float32))
    gx = np.arange(7, dtype=np.float32).reshape(1, 1, 1, 7) - np.float32(0.5)
    x = ((s[..., 0] * np.float32(2) + gx) * np.float32(W.strides[1])).reshape(2, -1)
    assert ((x >= lo[..., 0]) & (x <= hi[..., 0])).all()
    conf = s[..., 4].reshape(2, -1)
    assert ((conf >= lo[..., 4]) & (conf <= hi[..., 4])).all()
    shifted = ((s[..., 0] * np.float32(2) + gx + np.float32(0.5)) * np.float32(W.strides[1])).reshape(2, -1)
    assert not ((shifted >= lo[..., 0]) & (shifted <= hi[..., 0])).any()
