"""
Every conv op on its own, element by element against float64 (tests/conv_probe.py): the two probe networks run through the
C ABI, each conv layer's output (mdhip_read_layer) is compared with the float64 evaluation of that ONE op on the input it
really read (the producers' read_layer, read_input for the stem), every element within the derived bound -- no cascade, no
per-layer scalar.  The Detect convs (fp32, no activation) are held through the decoded predictions.

  1. the heuristic tiles, Detect decode in the conv epilogue and as its own launch;
  2. per tile family: every configuration forced on exactly the ops it claims (op_supports_cfg), nowhere else;
  3. the upsample read in place by its 1x1 reader (v2:160x160/2x2) over a stale concat buffer;
  4. the coverage predicates: what the families claim on the probe networks is what the networks were written for.

The arenas are poisoned (MDHIP_ARENA_POISON=1: padded K and N lanes hold NaN bytes), graph replay is off.  Figures (what ran,
worst err / tol per family and storage type) are recorded in profiles/conv_probe_tests.txt.
"""

import os

import pytest

import conv_probe as P

from megadetector_amd.hip_backend import HipContext, HipError

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']
KIND_CONV, KIND_UPSAMPLE = 0, 2
V2_UP_CFG = 'v2:160x160/2x2'          # conv_v2 configuration 0: the only one with the in-place upsample read
#: the families that ship, and one case for the configurations that do not (developer variants; e4m3 tiles, which claim
#: nothing in a 16-bit context): those that claim no op are passed over
CASES = list(P.PUBLIC_FAMILIES) + ['dev+f8']


class Probe:
    """one context of a probe network: created over a poisoned arena, its images preprocessed, one forward run"""

    def __init__(self, net, dtype):
        self.net, self.dtype = net, dtype
        self.W = P.weights(net)
        self.shape = P.NETS[net]['shape']
        self.checker = P.Checker(self.W, dtype)
        before = os.environ.get('MDHIP_ARENA_POISON')
        os.environ['MDHIP_ARENA_POISON'] = '1'
        try:
            cap = P.NETS[net]['capacity']
            self.ctx = HipContext(self.W, dtype=dtype, max_batch=cap[0], max_h=cap[1], max_w=cap[2])
        finally:
            if before is None:
                del os.environ['MDHIP_ARENA_POISON']
            else:
                os.environ['MDHIP_ARENA_POISON'] = before
        self.ctx.set_graph('off')
        self.cfgs = {self.ctx.conv_cfg_name(c): c for c in range(self.ctx.num_conv_cfgs())}
        self.feed(P.images(net))
        self.forward()
        self.infos = self.ctx.op_infos()
        self.convs = [o['op'] for o in self.infos if o['kind'] == KIND_CONV]
        self.shapes = P.op_shapes(net, self.W, self.infos)
        # (op_supports_cfg evaluates at the last forward's shape: this one)
        self.claims = {name: [op for op in self.convs if self.ctx.op_supports_cfg(op, c)] for name, c in self.cfgs.items()}

    def feed(self, imgs):
        n, h, w = self.shape
        self.ctx.preprocess(imgs, [(h, w, h, w, 0, 0)] * n, h, w)
        self.x = self.ctx.read_input(n, h, w)

    def forward(self):
        self.ctx.forward(*self.shape)
        src = P.HipSource(self.ctx, self.shape)
        src.input = lambda: self.x
        return src

    def unforce(self):
        for op in self.convs:
            self.ctx.set_op_cfg(op, -1)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope='module')
def probes():
    made = {}

    def get(net, dtype):
        if (net, dtype) not in made:
            made[net, dtype] = Probe(net, dtype)
        return made[net, dtype]
    yield get
    for p in made.values():
        p.close()


def _held(verdicts, worst=None, only=None):
    """no element over its bound; `worst` collects the largest err / tol per kind of check, over the checks `only` names
    (Verdict.key; None: all)"""
    for v in verdicts:
        if worst is not None and (only is None or v.key in only):
            key = 'detect' if 'Detect' in v.what else 'conv'
            if v.worst > worst.get(key, (0.0, ''))[0]:
                worst[key] = (v.worst, str(v))
    bad = P.failures(verdicts)
    assert not bad, '\n' + '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the heuristic tiles
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', list(P.NETS))
def test_heuristic_tiles(probes, net, dtype):
    p = probes(net, dtype)
    worst = {}
    try:
        for fuse_decode in (1, 0):
            p.ctx.set_option('fuse_decode', fuse_decode)
            src = p.forward()
            decoding = [o['name'] for o in p.ctx.op_infos() if 'Detect.decode' in o['name'] and o['bytes'] == 0]
            # (a decode done in the conv epilogue is not launched and reports no bytes)
            assert bool(decoding) == bool(fuse_decode), (fuse_decode, decoding)
            _held(p.checker.check(src, 'heuristic tiles, fuse_decode {}'.format(fuse_decode)), worst)
    finally:
        p.ctx.set_option('fuse_decode', 1)
    print('\n{} {} heuristic: {}'.format(net, dtype, ' '.join(
        '{}={}'.format(o['op'], p.ctx.conv_cfg_name(o['cfg'])) for o in p.infos if o['kind'] == KIND_CONV)))
    for key in sorted(worst):
        print('  worst {}: {}'.format(key, worst[key][1]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. every configuration of a family on the ops it claims
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('net', list(P.NETS))
def test_family_on_the_ops_it_claims(probes, net, dtype, case):
    p = probes(net, dtype)
    ctx = p.ctx
    worst = {}
    ran = []
    try:
        _held(p.checker.check(p.forward(), 'heuristic tiles'))
        for name, cfg in p.cfgs.items():
            fam = P.family(name)
            if (fam in ('dev', 'f8')) != (case == 'dev+f8') or (case != 'dev+f8' and fam != case):
                continue
            switched = p.claims[name]
            if not switched:
                continue
            for op in p.convs:
                ctx.set_op_cfg(op, cfg if op in switched else -1)
            try:
                src = p.forward()
            except HipError as e:
                pytest.fail('{} claims {} but its launch fails: {}'.format(name, [p.infos[op]['name'] for op in switched], e))
            now = ctx.op_infos()
            wrong = [(now[op]['name'], ctx.conv_cfg_name(now[op]['cfg'])) for op in switched if now[op]['cfg'] != cfg]
            assert not wrong, (name, 'ops that did not run the forced configuration', wrong)
            _held(p.checker.check(src, name), worst, only={p.shapes[net, op]['key'] for op in switched})
            ran.append((name, switched))
    finally:
        p.unforce()
    print('\n{} {} {}: {} configurations ran, {} forced launches, ops {}'.format(
        net, dtype, case, len(ran), sum(len(s) for _, s in ran), sorted({op for _, s in ran for op in s})))
    for name, switched in ran:
        print('  {:28s} {}'.format(name, ' '.join(str(op) for op in switched)))
    for key in sorted(worst):
        print('  worst {} among the forced ops: {}'.format(key, worst[key][1]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the upsample read in place
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_upsample_read_in_place(probes, dtype):
    """layer 13 of network B reads Upsample(9) ++ layer 3 through a Concat.  Forced to v2:160x160/2x2 it reads layer 9 in
    place: the upsample is not launched and the first 640 channels of the concat buffer are not written -- they hold the
    upsample of the images of the forward before (other images: a stale value).  The reference input is built from
    read_layer(9) repeated 2 x 2 and read_layer(3), never from the concat buffer."""
    p = probes('B', dtype)
    ctx = p.ctx
    imgs = P.images('B')
    up = [o for o in p.infos if o['kind'] == KIND_UPSAMPLE]
    reader = [o for o in p.infos if o['kind'] == KIND_CONV and o['layer'] == 13]
    assert len(up) == 1 and len(reader) == 1
    up, reader = up[0]['op'], reader[0]['op']
    cfg = p.cfgs[V2_UP_CFG]
    worst = {}
    try:
        p.forward()
        assert ctx.op_infos()[up]['bytes'] > 0, 'the heuristic tiles run the upsample launch'
        assert ctx.op_supports_cfg(reader, cfg)
        ctx.set_op_cfg(reader, cfg)
        p.feed(imgs[::-1])
        src = p.forward()
        now = ctx.op_infos()
        assert now[reader]['cfg'] == cfg, (now[reader]['name'], ctx.conv_cfg_name(now[reader]['cfg']))
        # mdhip_exec.cpp resolve: an upsample read in place by its consumer is not launched and reports no bytes
        assert now[up]['bytes'] == 0, (now[up]['name'], now[up]['bytes'])
        _held(p.checker.check(src, V2_UP_CFG + ' reading the upsample in place'), worst, only={13})
    finally:
        p.unforce()
        p.feed(imgs)
    for key in sorted(worst):
        print('\nB {} in place: worst {}: {}'.format(dtype, key, worst[key][1]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. what the probe networks reach
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
def test_probe_networks_reach_what_they_are_for(probes, dtype):
    claims, shapes = {}, {}
    for net in P.NETS:
        p = probes(net, dtype)
        shapes.update(p.shapes)
        for name, ops in p.claims.items():
            if P.family(name) in P.PUBLIC_FAMILIES:
                claims.setdefault(name, set()).update((net, op) for op in ops)
    unmet = P.unmet_coverage(claims, shapes)
    print('\n{}: claims (configuration: network.op ...)'.format(dtype))
    for name in claims:
        print('  {:28s} {}'.format(name, ' '.join('{}.{}'.format(*k) for k in sorted(claims[name]))))
    assert not unmet, '\n' + '\n'.join(unmet)
