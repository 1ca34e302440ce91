"""
What a forward launched (mdhip_get_op_info) against the device-free description of the same settings
(hip_backend.describe_launches, pinned without a GPU by tests/test_launches_cpu.py), and its independence of what the context
did before: the executor resolves a pass once per shape, kind of pass and generation of the settings, so a forward behind
setters, a single timed op and a forward of another shape must launch what the first forward launched -- the same bits.
YOLOV5X6_MD at 2 x 256 x 320 in bf16, with the strip tile forced on the first C3 block's 3x3s (the block runs fused) and a
conv_v2 tile on the 1x1 behind the head's last upsample (read in place); the Detect convs decode in their epilogues by default.
"""

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

N, H, W = 2, 256, 320
DTYPE = 'bf16'


def _identity_geoms(imgs):
    return [(im.shape[0], im.shape[1], im.shape[0], im.shape[1], 0, 0) for im in imgs]


@pytest.fixture(scope='module')
def weights():
    from megadetector_amd import weights_io, yolo_yaml
    return weights_io.synthetic_weights(yolo_yaml.YOLOV5X6_MD, seed=0)


@pytest.fixture()
def ctx(weights):
    from megadetector_amd.hip_backend import HipContext
    c = HipContext(weights, device=0, dtype=DTYPE, max_batch=N, max_h=H, max_w=W)
    try:
        imgs = PU.random_images(N, H, W, seed=77)
        c.preprocess(imgs, _identity_geoms(imgs), H, W)
        yield c
    finally:
        c.close()


def _force(ctx):
    """{op: configuration name}: the forced tiles of this module, set on the context"""
    infos = ctx.op_infos()
    by_name = {ctx.conv_cfg_name(c): c for c in range(ctx.num_conv_cfgs())}
    forced = {o['op']: 'v5:strip160x80/2x5' for o in infos if 'L2 C3.m' in o['name'] and 'cv2' in o['name']}
    up = [o['op'] for o in infos if 'L21 upsample' in o['name']]
    assert len(forced) == 4 and len(up) == 1
    forced[up[0] + 1] = 'v2:160x160/2x2'
    for op, name in forced.items():
        ctx.set_op_cfg(op, by_name[name])
    return forced


def _ran(ctx):
    """what mdhip_get_op_info reports of the last forward, per op: (cfg name | -1 | -2, m, n, k, flops, bytes)"""
    return [(ctx.conv_cfg_name(o['cfg']) if o['cfg'] >= 0 else o['cfg'], o['m'], o['n'], o['k'], o['flops'], o['bytes'])
            for o in ctx.op_infos()]


def _described(weights, forced, **options):
    from megadetector_amd import hip_backend
    text = hip_backend.describe_launches(weights, DTYPE, (N, H, W), hip_backend.table_entries(DTYPE), N, H, W, forced=forced, **options)
    out = []
    for line in text.splitlines():
        f = dict(kv.split('=') for kv in line.rsplit('" ', 1)[1].split()[1:])
        how = line.rsplit('" ', 1)[1].split()[0]
        cfg = f['cfg'] if how == 'launch' else -2 if how == 'in_front' else -1
        out.append((cfg, int(f['m']), int(f['n']), int(f['k']), float(f['flops']), float(f['bytes'])))
    return out


def _assert_covers(ctx):
    """the ops that ran include a fused block, an absorbed upsample and an in-epilogue decode -- or the module proves nothing"""
    infos = ctx.op_infos()
    assert sum(o['kind'] == 0 and o['cfg'] < 0 for o in infos) == 4                               # the four 1x1s of the fused block
    assert sum(o['kind'] == 2 and o['bytes'] == 0 for o in infos) == 1                            # the upsample read in place
    assert sum(o['kind'] == 3 and o['cfg'] == -2 for o in infos) == 4                             # every level decoded in its conv


def test_op_infos_are_the_device_free_description(ctx, weights):
    forced = _force(ctx)
    ctx.forward(N, H, W)
    _assert_covers(ctx)
    assert _ran(ctx) == _described(weights, forced)
    ctx.set_fuse(False)
    ctx.set_option('fuse_decode', 0)
    ctx.forward(N, H, W)
    assert _ran(ctx) == _described(weights, forced, fuse=False, fuse_decode=False)


@pytest.mark.parametrize('graph', [0, 1], ids=['eager', 'graph'])
def test_a_forward_does_not_depend_on_the_calls_before_it(ctx, graph):
    _force(ctx)
    ctx.set_graph(graph)

    def forward():
        ctx.forward(N, H, W)
        return ctx.read_predictions(N).copy(), _ran(ctx)
    pred, ran = forward()
    _assert_covers(ctx)

    def same(with_infos=True):
        p, r = forward()
        np.testing.assert_array_equal(p, pred)
        assert not with_infos or r == ran
    for _ in range(5 if graph else 1):                 # with graphs: eager and captured for both prediction buffers, then replayed
        same()
    ctx.set_fuse(0)
    same(False)                                        # other launches, the same bits (tests/test_gpu_headline.py)
    assert sum(o['kind'] == 0 and o['cfg'] < 0 for o in ctx.op_infos()) == 0
    ctx.set_fuse(1)
    same()                                             # (with graphs: eager again behind a setter)
    ctx.set_option('fuse_decode', 0)
    same(False)
    assert sum(o['kind'] == 3 and o['cfg'] == -2 for o in ctx.op_infos()) == 0
    ctx.set_option('fuse_decode', 1)
    same()
    conv = [o['op'] for o in ctx.op_infos() if 'L2 C3.m1.cv2' in o['name']][0]
    assert ctx.time_op(conv, N, H, W, iters=2) > 0     # one 3x3 of the fused block on its own
    same()
    ctx.forward(1, 128, 192)                           # another shape (the input tensor stays as it is)
    same()
    same()
