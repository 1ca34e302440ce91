"""
The streaming body of the 160 -> 160 channel 1x1 convs (megadetector_amd/csrc/conv_v2_stream.h; mdhip_set_option "pw_stream"):
the same bits as the tiled instantiations of conv_v2.cpp, every element within the float64 bound of tests/conv_probe.py, and
taken by the ops it is for and by no other.

Network S is a probe network (one conv op per layer) whose 1x1 convs with 160 input and 160 output channels
  1  read a plain tensor and write channels 0 .. 159 of a 320-channel concat buffer (ld_out != N),
  2  read those channels (ld_in != C_in) and write channels 160 .. 319 of the SAME buffer (input and output interleave in
     memory without sharing a byte),
  5  read a channel slice and write a plain tensor,
  12 read a concat of an Upsample (64 channels) and a 96-channel tensor: with the upsample read in place (v2:160x160/2x2)
     the op has an in_up reader and is not streamed, without (mdhip_set_fuse 0) it is;
layer 4 has K = 320 and the Detect convs write fp32: never streamed.  Network R is a C3 block: its bottleneck's 1x1 is what
the benchmark streams (the hidden conv reading one half of the cv1|cv2 buffer), its 3x3 adds a residual.

The forward shapes give the 160-channel maps pixel counts that are no multiple of the 16 pixels of a group (22 x 20 and
10 x 6, one and three images), one that is (24 x 20), fewer pixels than a wave keeps in flight (4 x 4: one group, two empty
ones), and enough for every wave to go through its loop twice (3 images of 96 x 240: 4320 groups over 1024 waves).

"pw_stream" 1 takes the body only from the pixel count on at which it is the faster one; 2 takes it always, which is what
these shapes need.  The arenas are poisoned (MDHIP_ARENA_POISON=1), graph replay is off.
"""

import os

import numpy as np
import pytest

import conv_probe as P

from megadetector_amd import weights_io
from megadetector_amd.hip_backend import HipContext

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']
KIND_CONV = 0
V2_UP, V2_STREAM, KEY_DEC = 3, 6, 100          # mdhip_op_info::variant of conv_v2 tiles (include/mdhip.h)
TILE = 'v2:128x160/2x2'                         # the tile the benchmark's 819 200-pixel launches have
TILE_UP = 'v2:160x160/2x2'                      # the only one with the in-place upsample read

NET_S = P._yaml([
    [-1, 1, 'Conv', [160, 6, 2, 2]],               # 0  stem
    [-1, 1, 'Conv', [160, 1, 1]],                  # 1  streamed; writes concat slice 0
    [-1, 1, 'Conv', [160, 1, 1]],                  # 2  streamed; reads slice 0, writes slice 1 of the same buffer
    [[1, 2], 1, 'Concat', [1]],                    # 3
    [-1, 1, 'Conv', [160, 1, 1]],                  # 4  K = 320
    [1, 1, 'Conv', [160, 1, 1]],                   # 5  streamed; reads slice 0; Detect level 0
    [-1, 1, 'Conv', [160, 3, 2]],                  # 6
    [-1, 1, 'Conv', [64, 1, 1]],                   # 7
    [0, 1, 'Conv', [96, 1, 1]],                    # 8
    [7, 1, 'nn.Upsample', [None, 2, 'nearest']],   # 9
    [[-1, 8], 1, 'Concat', [1]],                   # 10 64 + 96 channels
    [4, 1, 'Conv', [24, 1, 1]],                    # 11 (keeps layer 4 alive)
    [10, 1, 'Conv', [160, 1, 1]],                  # 12 reader of the upsample; Detect level 1
], [5, 12])
STREAMED, READER, DETECT = (1, 2, 5), 12, 13
NET_R = P._yaml([
    [-1, 1, 'Conv', [160, 6, 2, 2]],
    [-1, 1, 'C3', [320]],
], [1])
CAPACITY = (3, 192, 480)
#: (images, height, width) of the forward; the 160-channel maps are half of it
SHAPES = [(1, 44, 40), (3, 44, 40), (1, 20, 12), (3, 20, 12), (3, 48, 40), (1, 8, 8), (3, 192, 480)]


def _images(shape, seed):
    n, h, w = shape
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(n):
        img = 127 + 100 * np.sin(xs / (7.0 + 3 * i) + i)[..., None] * np.cos(ys[..., None] / (5.0 + i) + np.arange(3))
        img = img + rng.normal(0, 30, (h, w, 3))
        out.append(np.clip(np.rint(img / 16 if i == 1 else img), 0, 255).astype(np.uint8))
    return out


class Net:
    """a context of one network over a poisoned arena, with the 160 -> 160 1x1 convs forced onto conv_v2 tiles"""

    def __init__(self, yaml, dtype):
        self.W = weights_io.synthetic_weights(yaml, seed=P.SEED)
        before = os.environ.get('MDHIP_ARENA_POISON')
        os.environ['MDHIP_ARENA_POISON'] = '1'
        try:
            self.ctx = HipContext(self.W, dtype=dtype, max_batch=CAPACITY[0], max_h=CAPACITY[1], max_w=CAPACITY[2])
        finally:
            if before is None:
                del os.environ['MDHIP_ARENA_POISON']
            else:
                os.environ['MDHIP_ARENA_POISON'] = before
        self.ctx.set_graph('off')
        self.cfgs = {self.ctx.conv_cfg_name(c): c for c in range(self.ctx.num_conv_cfgs())}
        self.forced = False

    def run(self, shape, pw_stream, seed=11):
        n, h, w = shape
        self.ctx.set_option('pw_stream', pw_stream)
        self.ctx.preprocess(_images(shape, seed), [(h, w, h, w, 0, 0)] * n, h, w)
        self.ctx.forward(n, h, w)
        if not self.forced:              # (the ops and their shapes are known after a forward)
            for o in self.ctx.op_infos():
                if o['kind'] == KIND_CONV and o['ntaps'] == 1 and o['n'] == 160 and o['k'] in (160, 320):
                    self.ctx.set_op_cfg(o['op'], self.cfgs[TILE_UP if o['layer'] == READER else TILE])
            self.forced = True
            self.ctx.forward(n, h, w)
        src = P.HipSource(self.ctx, shape)
        x = self.ctx.read_input(n, h, w)
        src.input = lambda: x
        return src

    def convs(self):
        return [o for o in self.ctx.op_infos() if o['kind'] == KIND_CONV]


@pytest.fixture(scope='module')
def nets():
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            made[name, dtype] = Net({'S': NET_S, 'R': NET_R}[name], dtype)
        return made[name, dtype]
    yield get
    for net in made.values():
        net.ctx.set_option('pw_stream', 1)
        net.ctx.close()


def _variants(net):
    return {(o['layer'], o['name']): o['variant'] for o in net.convs()}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '{}x{}x{}'.format(*s))
@pytest.mark.parametrize('dtype', DTYPES)
def test_same_bits_and_within_the_float64_bound(nets, dtype, shape):
    net = nets('S', dtype)
    checker = P.Checker(net.W, dtype)
    layers = P.conv_layers(net.W)
    got = {}
    for pw_stream in (0, 2):
        src = net.run(shape, pw_stream)
        by_layer = {o['layer']: o for o in net.convs() if o['layer'] in layers}
        took = sorted(l for l, o in by_layer.items() if o['variant'] == V2_STREAM)
        # (12 reads its upsample in place: an in_up reader keeps the tile's own instantiation)
        assert took == (list(STREAMED) if pw_stream else []), (pw_stream, took, _variants(net))
        assert by_layer[READER]['variant'] == V2_UP, _variants(net)
        assert all(net.ctx.conv_cfg_name(by_layer[l]['cfg']) == TILE for l in STREAMED), 'the tile keeps its name'
        got[pw_stream] = {l: src.layer(l) for l in layers}
        got[pw_stream]['pred'] = src.predictions()
        bad = P.failures(checker.check(src, 'pw_stream {}'.format(pw_stream)))
        assert not bad, '\n' + '\n'.join(bad)
    for key in got[0]:
        assert got[0][key].tobytes() == got[2][key].tobytes(), ('layer', key, 'differs between pw_stream 0 and 2')


@pytest.mark.parametrize('dtype', DTYPES)
def test_taken_by_the_ops_it_is_for(nets, dtype):
    net = nets('S', dtype)
    shape = SHAPES[1]
    ctx = net.ctx
    try:
        net.run(shape, 2)
        convs = net.convs()
        for o in convs:
            streamed = o['variant'] == V2_STREAM
            if o['layer'] == DETECT:
                assert not streamed, ('a Detect conv', o)
            elif o['layer'] == 4:
                assert o['k'] == 320 and ctx.conv_cfg_name(o['cfg']) == TILE and not streamed, ('K = 320', o)
            elif o['layer'] == READER:
                assert o['variant'] == V2_UP, ('the in_up reader', o)
            else:
                assert streamed == (o['layer'] in STREAMED), o
        # without the upsample read in place the reader is a plain 160 -> 160 1x1 over its concat buffer: streamed, same bits
        ctx.set_fuse(0)
        a = net.run(shape, 0).layer(READER)
        assert {o['layer']: o['variant'] for o in net.convs()}[READER] not in (V2_UP, V2_STREAM)
        b = net.run(shape, 2).layer(READER)
        assert {o['layer']: o['variant'] for o in net.convs()}[READER] == V2_STREAM
        assert a.tobytes() == b.tobytes()
        ctx.set_fuse(1)
        # the default takes the body where it is the faster one: not at these sizes
        net.run(shape, 1)
        assert not [o for o in net.convs() if o['variant'] == V2_STREAM]
    finally:
        ctx.set_fuse(1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bottleneck_of_a_c3_block(nets, dtype):
    """the benchmark's launches: the bottleneck's 1x1 reads one half of the cv1|cv2 buffer; the 3x3 behind it adds a residual"""
    net = nets('R', dtype)
    shape = (3, 44, 40)
    out = {}
    for pw_stream in (0, 2):
        net.run(shape, pw_stream)
        convs = net.convs()
        hidden = [o for o in convs if o['ntaps'] == 1 and o['n'] == 160 and o['k'] == 160]
        with_res = [o for o in convs if o['has_res']]
        assert len(hidden) == 1 and len(with_res) == 1, [o['name'] for o in convs]
        assert (hidden[0]['variant'] == V2_STREAM) == bool(pw_stream), hidden
        assert net.ctx.conv_cfg_name(hidden[0]['cfg']) == TILE
        assert [o['name'] for o in convs if o['variant'] == V2_STREAM] == ([hidden[0]['name']] if pw_stream else [])
        out[pw_stream] = (net.ctx.read_op_tensor(hidden[0]['op'], 1, shape[0]), net.ctx.read_layer(1, shape[0]),
                          net.ctx.read_predictions(shape[0]))
    for a, b in zip(out[0], out[2]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
