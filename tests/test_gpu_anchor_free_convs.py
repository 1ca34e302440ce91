"""
The conv stack of the anchor-free models (YOLO11: MDv1000-larch / -sorrel; YOLOv9-C: MDv1000-cedar) beyond the tiles the
heuristic picks at batch 1-2, through the C ABI, against the storage-emulating restatements tests/yolo11_ref.py and
tests/yolov9_ref.py:

  1. every tile configuration forced on every conv op it claims (supports()), on every anchor-free topology: the bitwise
     family bit-identical to the heuristic forward, the other K orders layer by layer within the layer bars;
  2. the in-place upsample read of conv_v2 configuration 0 (ConvArgs::in_up) on the Upsample -> Concat -> 1x1 heads,
     with a stale upsample buffer in the arena;
  3. MDHIP_ARENA_POISON on these topologies (channel slices, padded class rows, ADown halves, CBFuse sources, qkv);
  4. the launches of the published figures: batch 32 at the benchmark shapes against batch 1, bit for bit;
  5. the C2PSA attention kernel at the 16-query / 32-key block edges and with a peaked softmax.

Figures (coverage per family, worst layer errors, the batch-32 tiles) are recorded in profiles/anchor_free_conv_tests.txt.
"""

import numpy as np
import pytest
import torch

import parity_util as PU
import yolo11_ref as R11
import yolov9_ref as R9
from test_gpu_parity import LAYER_MAX_TOL, F16_LAYER_MAX_TOL
from test_gpu_headline import LAYER_MEAN_TOL, F16_LAYER_MEAN_TOL
from test_gpu_yolo11 import _bits, _from_bits, _unit_tol, _ctx as _y11_ctx
from test_gpu_yolov9 import _letterboxed, _reachable

from megadetector_amd import weights_io, yolo_yaml
from megadetector_amd import _lib
from megadetector_amd.hip_backend import HipContext, HipError
from megadetector_amd.yolo_model import MDHIP_SILENCE

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']

# network -> (letterbox size, source image h, w): batch 2 throughout, so that M tiles cross the image boundary
NETS = {
    'YOLO11N_TEST': (640, 480, 640),          # 16 / 32 / 48-channel slices of one concat buffer
    'GELAN_TEST': (640, 480, 640),
    'YOLOV9_DUAL_TEST': (640, 480, 640),
    'YOLO11L_MD': (640, 480, 640),            # larch: the shipped widths
    'YOLO11S_MD': (960, 720, 960),            # sorrel: a 4:3 source letterboxes to 736 x 960 -> odd P5 map 23 x 30, N = 690
    'GELAN_C_MD': (640, 480, 640),            # cedar, converted form: grouped head conv
    'YOLOV9C_MD': (640, 480, 640),            # cedar, training form: CBLinear / CBFuse
}
# the dual forms lower only the branch of the head that runs (the auxiliary one, tests/test_gpu_yolov9.py): it has no
# Upsample -> Concat -> 1x1 pattern, so section 2 has nothing to force there
UP_NETS = [n for n in NETS if n not in ('YOLOV9_DUAL_TEST', 'YOLOV9C_MD')]

KIND_CONV, KIND_UPSAMPLE = 0, 2
V2_UP_CFG = 'v2:160x160/2x2'          # conv_v2 configuration 0: the only one with the in-place upsample read


def _weights(name):
    return weights_io.synthetic_weights(getattr(yolo_yaml, name), seed=0)


def _ref_module(name):
    return R11 if yolo_yaml.is_yolo11(getattr(yolo_yaml, name)) else R9


def _bars(dtype):
    if dtype == 'fp16':
        return F16_LAYER_MAX_TOL, F16_LAYER_MEAN_TOL
    return LAYER_MAX_TOL, LAYER_MEAN_TOL


def _geoms(lb):
    return [(im.shape[0], im.shape[1], im.shape[0], im.shape[1], 0, 0) for im in lb]


def _family(cfg_name):
    """tile family of a configuration name: the first-generation tiles carry no prefix"""
    if ':' not in cfg_name:
        return 'v1'
    head = cfg_name.split(':')[0]
    if head == 'v5':
        return 'v5:strip' if cfg_name.startswith('v5:strip') else 'v5:run'
    return head


class Restated:
    """the storage-emulating restatement of one (network, dtype, input), computed once: every layer the library lowers and
    the predictions"""

    def __init__(self, name, W, x, dtype):
        self.keep = {}
        self.pred = _ref_module(name).Forward(W, emulate=dtype, keep=self.keep)(x)
        reach = _reachable(W)
        self.layers = [i for i in sorted(self.keep) if i in reach and W.specs[i].type != MDHIP_SILENCE]
        self.dtype = dtype

    def check(self, ctx, n, worst=None, what=''):
        """every lowered layer and the predictions of the context's last forward within the bars of test_gpu_yolo11._layers"""
        max_tol, mean_tol = _bars(self.dtype)
        for i in self.layers:
            emax, emean = PU.rel_err(ctx.read_layer(i, n), self.keep[i].numpy())
            if worst is not None:
                worst[0] = max(worst[0], emax)
                worst[1] = max(worst[1], emean)
            assert emax < max_tol and emean < mean_tol, (what, 'layer', i, emax, emean)
        pred = ctx.read_predictions(n)
        assert pred.shape == self.pred.shape, (what, pred.shape, self.pred.shape)
        e_box = PU.rel_err(pred[..., :4], self.pred[..., :4])
        e_cls = float(np.abs(pred[..., 4:] - self.pred[..., 4:]).max())
        assert e_box[0] < max_tol and e_box[1] < mean_tol and e_cls < max_tol, (what, e_box, e_cls)
        return pred


def _first_differing_layer(ctx, layers, n, hh, ww, convs):
    """the first layer whose output differs between the forced tiles (the current forward) and the heuristic ones"""
    forced = {i: ctx.read_layer(i, n) for i in layers}
    for op in convs:
        ctx.set_op_cfg(op, -1)
    ctx.forward(n, hh, ww)
    for i in layers:
        if not np.array_equal(ctx.read_layer(i, n), forced[i]):
            return i
    return None


# ---------------------------------------------------------------------------------------------------------------------
# 1. every conv configuration on every anchor-free topology
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(NETS))
def test_every_conv_configuration(name, dtype):
    size, sh, sw = NETS[name]
    W = _weights(name)
    x, lb = _letterboxed(2, sh, sw, size, 31)
    n, _, hh, ww = x.shape
    ref = Restated(name, W, x, dtype)
    ctx = HipContext(W, dtype=dtype, max_batch=2, max_h=size, max_w=size)
    convs = []
    try:
        ctx.set_graph('off')
        ctx.preprocess(lb, _geoms(lb), hh, ww)
        ctx.forward(n, hh, ww)
        worst = [0.0, 0.0]
        base = ref.check(ctx, n, worst, 'heuristic').copy()
        infos = ctx.op_infos()
        convs = [o['op'] for o in infos if o['kind'] == KIND_CONV]
        heur = {o['op']: o['cfg'] for o in infos if o['kind'] == KIND_CONV}
        assert all(ctx.cfg_is_bitwise(c) for c in heur.values()), 'the heuristic picks first-generation tiles only'
        took = {}                                  # cfg -> the conv ops it claimed
        for cfg in range(ctx.num_conv_cfgs()):
            cname = ctx.conv_cfg_name(cfg)
            # (op_supports_cfg evaluates at the last forward's shape: this one)
            switched = [op for op in convs if ctx.op_supports_cfg(op, cfg)]
            took[cfg] = switched
            if _family(cname) == 'v1':
                assert len(switched) == len(convs), (cname, 'the first-generation kernel takes every 16-bit op',
                                                     [infos[op]['name'] for op in convs if op not in switched])
            if not switched:
                continue
            for op in convs:
                ctx.set_op_cfg(op, cfg if op in switched else -1)
            try:
                ctx.forward(n, hh, ww)
            except HipError as e:
                pytest.fail('{} claims {} ops (first: {}) but its launch fails: {}'.format(
                    cname, len(switched), infos[switched[0]]['name'], e))
            # (no fused bottleneck here: these topologies have no C3 block, the only one conv_v5c.cpp fuses)
            ran = ctx.op_infos()
            wrong = [(ran[op]['name'], ran[op]['cfg']) for op in switched if ran[op]['cfg'] != cfg]
            assert not wrong, (cname, 'ops that did not run the forced configuration', wrong)
            if ctx.cfg_is_bitwise(cfg):
                got = ctx.read_predictions(n)
                if not np.array_equal(got, base):
                    first = _first_differing_layer(ctx, ref.layers, n, hh, ww, convs)
                    pytest.fail('{} (bitwise family) changes the predictions; first differing layer: {}'.format(cname, first))
            else:
                ref.check(ctx, n, worst, cname)
        # coverage table: per family, the configurations that took ops, the forced launches, the distinct ops
        fams = {}
        for cfg, ops in took.items():
            f = fams.setdefault(_family(ctx.conv_cfg_name(cfg)), [0, 0, 0, set()])
            f[0] += 1
            f[1] += len(ops) > 0
            f[2] += len(ops)
            f[3].update(ops)
        print('\n{} {} {}x{} b{}: {} conv ops; heuristic + non-bitwise worst layer max {:.2e} mean {:.2e}'.format(
            name, dtype, hh, ww, n, len(convs), worst[0], worst[1]))
        for fam in sorted(fams):
            c, t, k, ops = fams[fam]
            print('  {:9s} {:2d} configurations, {:2d} took ops, {:5d} forced launches, {:3d} / {} ops'.format(
                fam, c, t, k, len(ops), len(convs)))
    finally:
        for op in convs:
            ctx.set_op_cfg(op, -1)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the in-place upsample read (conv_v2 configuration 0 with ConvArgs::in_up) on the heads
# ---------------------------------------------------------------------------------------------------------------------

def _up_readers(ctx, W):
    """[(upsample op, its reader conv op, whether the in-place read is admitted)].  The reader is the cv1 of the
    C3k2 / RepNCSPELAN4 behind the Concat; absorb_upsample (mdhip_exec.cpp) admits the pair when the upsample's input
    has whole 64-channel slabs (the conv's map is twice the upsample input's, so even)"""
    infos = ctx.op_infos()
    out = []
    for o in infos:
        if o['kind'] != KIND_UPSAMPLE:
            continue
        layer = o['layer']
        assert W.specs[layer + 1].frm[0] == layer, 'the Concat behind the Upsample starts with it'
        prefix = 'L{} '.format(layer + 2)
        readers = [r for r in infos[o['op'] + 1:] if r['kind'] == KIND_CONV and r['name'].startswith(prefix)]
        assert readers and '.cv1 ' in readers[0]['name'] and readers[0]['ntaps'] == 1, (o['name'], readers[:1])
        up_c = W.specs[W.specs[layer].frm[0]].c_out
        out.append((o['op'], readers[0]['op'], up_c % 64 == 0))
    return out


def _force_up_readers(ctx, pairs, cfg):
    forced = []
    for _, rd, _ in pairs:
        if ctx.op_supports_cfg(rd, cfg):
            ctx.set_op_cfg(rd, cfg)
            forced.append(rd)
    return forced


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', UP_NETS)
def test_upsample_read_in_place_on_the_heads(name, dtype):
    size, sh, sw = NETS[name]
    W = _weights(name)
    xa, lba = _letterboxed(2, sh, sw, size, 41)
    _, lbb = _letterboxed(2, sh, sw, size, 42)
    n, _, hh, ww = xa.shape
    ctx = HipContext(W, dtype=dtype, max_batch=2, max_h=size, max_w=size)
    pairs = []
    try:
        ctx.set_graph('off')
        ctx.preprocess(lba, _geoms(lba), hh, ww)
        ctx.forward(n, hh, ww)
        base = ctx.read_predictions(n).copy()
        pairs = _up_readers(ctx, W)
        assert len(pairs) == 2, pairs
        infos = ctx.op_infos()
        assert all(infos[u]['bytes'] > 0 for u, _, _ in pairs), 'the heuristic tiles run the upsample launch'
        # images B with the heuristic tiles: the concat buffers now hold B's upsample, a stale value for A
        ctx.preprocess(lbb, _geoms(lbb), hh, ww)
        ctx.forward(n, hh, ww)
        cfg = {ctx.conv_cfg_name(c): c for c in range(ctx.num_conv_cfgs())}[V2_UP_CFG]
        forced = _force_up_readers(ctx, pairs, cfg)
        ctx.preprocess(lba, _geoms(lba), hh, ww)
        ctx.forward(n, hh, ww)
        np.testing.assert_array_equal(ctx.read_predictions(n), base)
        infos = ctx.op_infos()
        absorbed = []
        for u, rd, admitted in pairs:
            if rd in forced:
                assert infos[rd]['cfg'] == cfg, (infos[rd]['name'], infos[rd]['cfg'])
            admitted = admitted and rd in forced
            # mdhip_exec.cpp resolve: an upsample read in place by its consumer is not launched and reports no bytes
            assert (infos[u]['bytes'] == 0) == admitted, (infos[u]['name'], infos[rd]['name'], admitted, infos[u]['bytes'])
            if admitted:
                absorbed.append(infos[rd]['name'])
        # the path must really run here, or this test pins nothing: a head that admits no in-place read is a finding
        assert absorbed, 'no head of {} admits the in-place upsample read'.format(name)
        print('\n{} {}: in-place upsample read on {}'.format(name, dtype, absorbed))
    finally:
        for _, rd, _ in pairs:
            ctx.set_op_cfg(rd, -1)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a poisoned arena
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['YOLO11N_TEST', 'GELAN_TEST', 'YOLOV9_DUAL_TEST', 'YOLO11S_MD'])
def test_results_do_not_depend_on_unwritten_memory(name, dtype, monkeypatch):
    """MDHIP_ARENA_POISON=1 fills the arena with 0xFF bytes (NaN in both storage types): the channel slices under 64
    channels, the padded class rows, the qkv tensor read in place, ADown halves and CBFuse sources must never be read
    where nobody wrote.  The first forward of each context reads the upsamples in place where the heads admit it (the
    concatenated buffer's first part is then never written), then the heuristic tiles, then batch 1 in the same arena."""
    size, sh, sw = NETS[name]
    W = _weights(name)
    x, lb = _letterboxed(2, sh, sw, size, 51)
    n, _, hh, ww = x.shape
    out = {}
    for poison in ('0', '1'):
        monkeypatch.setenv('MDHIP_ARENA_POISON', poison)
        ctx = HipContext(W, dtype=dtype, max_batch=n, max_h=size, max_w=size)
        try:
            ctx.set_graph('off')
            pairs = _up_readers(ctx, W)
            cfg = {ctx.conv_cfg_name(c): c for c in range(ctx.num_conv_cfgs())}[V2_UP_CFG]
            # (a 1x1's support by conv_v2 does not depend on the map size: op_supports_cfg before the first forward is
            # the answer at this shape)
            forced = _force_up_readers(ctx, pairs, cfg)
            ctx.preprocess(lb, _geoms(lb), hh, ww)
            ctx.forward(n, hh, ww)
            up = ctx.read_predictions(n).copy()
            infos = ctx.op_infos()
            n_absorbed = sum(infos[u]['bytes'] == 0 for u, _, _ in pairs)
            for rd in forced:
                ctx.set_op_cfg(rd, -1)
            ctx.forward(n, hh, ww)
            plain = ctx.read_predictions(n).copy()
            ctx.preprocess(lb[:1], _geoms(lb[:1]), hh, ww)           # a smaller batch in the same arena: the rest stays poisoned
            ctx.forward(1, hh, ww)
            one = ctx.read_predictions(1).copy()
        finally:
            ctx.close()
        assert np.isfinite(up).all() and np.isfinite(plain).all() and np.isfinite(one).all(), \
            'NaN: a kernel read unwritten memory (poison {})'.format(poison)
        if name in UP_NETS:
            assert n_absorbed > 0, 'the in-place upsample read did not run'
        out[poison] = (up, plain, one)
    for a, b in zip(out['0'], out['1']):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(out['1'][0], out['1'][1])
    np.testing.assert_array_equal(out['1'][2][0], out['1'][1][0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the benchmarked launches: batch 32 at the benchmark shapes
# ---------------------------------------------------------------------------------------------------------------------

def _nms_rows(ctx, n, thr):
    d, c = ctx.nms(n, thr, 0.45, 300)
    return [d[i, :c[i]].copy() for i in range(n)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,size', [('YOLO11L_MD', 640), ('YOLO11S_MD', 960), ('YOLOV9C_MD', 640), ('GELAN_C_MD', 640)])
def test_batch32_benchmark_launches_equal_batch1(name, size, dtype):
    """the heuristic tiles at batch 32 (graph off, as bench.py runs them) are not those of batch 1 -- other tiles, other
    persistent-stream splits -- but of the same K order: 32 distinct images give bit for bit what each gives alone, and
    two of those batch-1 forwards are pinned layer by layer against the restatement"""
    W = _weights(name)
    B = 32
    imgs = PU.structured_images(B, size, size, seed=61)
    x, infos = PU.oracle_input(imgs, size, 32)
    lb = [np.ascontiguousarray(i['img_processed']) for i in infos]
    hh, ww = x.shape[2:]
    assert (hh, ww) == (size, size)
    ctx = HipContext(W, dtype=dtype, max_batch=B, max_h=size, max_w=size)
    try:
        ctx.set_graph('off')
        ctx.preprocess(lb, _geoms(lb), hh, ww)
        ctx.forward(B, hh, ww)
        ops = [o for o in ctx.op_infos() if o['kind'] == KIND_CONV]
        assert all(ctx.cfg_is_bitwise(o['cfg']) for o in ops), 'batch 32 runs one K order'
        tiles = {}
        for o in ops:
            tiles.setdefault(ctx.conv_cfg_name(o['cfg']), []).append(o['op'])
        p32 = ctx.read_predictions(B).copy()
        rows32 = {thr: _nms_rows(ctx, B, thr) for thr in (1e-5, 0.2)}
        assert np.isfinite(p32).all()
        assert all(len(r) > 0 for r in rows32[1e-5])        # (the synthetic weights leave few or no boxes above 0.2)
        for i in range(B):
            ctx.preprocess(lb[i:i + 1], _geoms(lb[i:i + 1]), hh, ww)
            ctx.forward(1, hh, ww)
            np.testing.assert_array_equal(ctx.read_predictions(1)[0], p32[i], err_msg='image {}'.format(i))
            for thr in (1e-5, 0.2):
                np.testing.assert_array_equal(_nms_rows(ctx, 1, thr)[0], rows32[thr][i], err_msg='image {} thr {}'.format(i, thr))
            if i in (0, B - 1):
                Restated(name, W, x[i:i + 1], dtype).check(ctx, 1, None, 'image {} at batch 1'.format(i))
        print('\n{} {} {}x{} b{}: tiles of the heuristic forward (configuration: conv ops)'.format(name, dtype, hh, ww, B))
        for t in sorted(tiles, key=lambda t: -len(tiles[t])):
            print('  {:20s} {:3d} ops: {}'.format(t, len(tiles[t]), ' '.join(str(op) for op in tiles[t])))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the attention kernel at the block edges and with a peaked softmax
# ---------------------------------------------------------------------------------------------------------------------

def _attention(ctx, qkv, n, N, heads, dtype):
    out = np.empty((n, N, heads * 64), dtype=np.uint16)
    rc = ctx.lib.mdhip_attention_on(ctx.h, _lib.np_ptr(_bits(qkv, dtype)), _lib.np_ptr(out), n, N, heads, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    h, w = qkv.shape[1:3]
    ref, _ = R11.Forward.attention_core(None, torch.from_numpy(qkv).permute(0, 3, 1, 2), heads)
    ref = ref.permute(0, 2, 3, 1).reshape(n, N, heads * 64).numpy()
    return _from_bits(out, dtype), ref


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('heads', [2, 4])
@pytest.mark.parametrize('hw', [(1, 1), (4, 4), (1, 17), (1, 31), (4, 8), (3, 11), (6, 8)])
def test_attention_kernel_block_edges(dtype, heads, hw):
    """N = 1, 16, 17, 31, 32, 33, 48: where the 16-query tile and the 32-key block masks (q >= N, key < N) change"""
    ctx, _ = _y11_ctx(dtype)
    h, w = hw
    n = 2
    rng = np.random.default_rng(1000 + h * w * heads)
    qkv = _from_bits(_bits(rng.standard_normal((n, h, w, heads * 128)) * 1.5, dtype), dtype)
    got, ref = _attention(ctx, qkv, n, h * w, heads, dtype)
    emax, emean = PU.rel_err(got, ref)
    assert emax < 2 * _unit_tol(dtype) and emean < _unit_tol(dtype) / 4, (emax, emean)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('heads', [2, 4])
@pytest.mark.parametrize('hw', [(3, 11), (6, 8), (23, 30)])
def test_attention_kernel_peaked_softmax(dtype, heads, hw):
    """q and k scaled x8: scores spread over several hundred.  Each query has one planted key in the LAST 32-key block
    whose score lies ~600 above every other, so the running max jumps by far more than the exp range after the earlier
    blocks: their partial sums only vanish if alpha rescales both the output and the row sum"""
    ctx, _ = _y11_ctx(dtype)
    h, w = hw
    n, N = 2, h * w
    rng = np.random.default_rng(77 + N * heads)
    raw = rng.standard_normal((n, N, heads, 128))
    q, k = raw[..., :32] * 8, raw[..., 32:64] * 8
    last = (N - 1) // 32 * 32
    assert last > 0, 'the planted keys must follow a full key block'
    planted = min(4, N - last)
    for c in range(planted):
        q[:, c::planted, :, :planted] = 0
        q[:, c::planted, :, c] = 40                  # query i aims at direction c = i % planted ...
        k[:, N - 1 - c, :, :] = 0
        k[:, N - 1 - c, :, c] = 120                  # ... which only key N - 1 - c carries: score 40 * 120 / sqrt(32) = 849
    raw[..., :32], raw[..., 32:64] = q, k
    qkv = _from_bits(_bits(raw.reshape(n, h, w, heads * 128), dtype), dtype)
    # the premise: the scores span several hundred and every query's maximum is its planted key, far above the rest
    qq = qkv.reshape(n, N, heads, 128)
    s = np.einsum('bqhc,bkhc->bhqk', qq[..., :32], qq[..., 32:64]) * 32 ** -0.5
    top = np.sort(s, axis=-1)
    assert s.max() - s.min() > 500 and (top[..., -1] - top[..., -2]).min() > 300
    assert (s.argmax(-1) >= last).all()
    got, ref = _attention(ctx, qkv, n, N, heads, dtype)
    emax, emean = PU.rel_err(got, ref)
    assert emax < 2 * _unit_tol(dtype) and emean < _unit_tol(dtype) / 4, (emax, emean)
