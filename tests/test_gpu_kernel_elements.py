"""
attn_kernel, dwconv3x3_kernel and tta_scale_kernel on the GPU, every element against float64 (tests/kernel_elements.py holds the
references and the derivation of every bound; tests/test_kernel_elements_cpu.py shows that the checks bite).  The kernels run
through their hooks: mdhip_attention_on, mdhip_dwconv3x3_on and mdhip_tta_input_on.  The in-place, pitched views of the real
models are held to the same bounds by tests/test_gpu_op_step.py.

Every case prints one line per launch (prefix "KE|"): kernel, storage type, case, worst err / tol and where, elements over and in
all, and for attention and depthwise the old norm-wise figure max |d| / max |ref| of the same data.  profiles/kernel_element_tests.txt
is made of these lines.
"""

import numpy as np
import pytest
import torch

import conv_probe as P
import kernel_elements as KE

from megadetector_amd import _lib, weights_io, yolo_yaml
from megadetector_amd.hip_backend import HipContext

pytestmark = pytest.mark.gpu

DTYPES = ['bf16', 'fp16']


def _bits(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(P.TORCH_DTYPE[dtype])
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def _from_bits(u, dtype):
    return torch.from_numpy(np.ascontiguousarray(u).view(np.int16)).view(P.TORCH_DTYPE[dtype]).float().numpy()


@pytest.fixture(scope='module')
def contexts():
    made = {}

    def get(name, dtype, capacity):
        if (name, dtype) not in made:
            W = weights_io.synthetic_weights(getattr(yolo_yaml, name), seed=0)
            made[name, dtype] = HipContext(W, dtype=dtype, max_batch=capacity[0], max_h=capacity[1], max_w=capacity[2])
        return made[name, dtype]
    yield get
    for c in made.values():
        c.close()


def _line(kernel, dtype, case, v, old=None):
    print('KE| {} {} {} worst {:.3f} at {} over {} of {}{}'.format(kernel, dtype, case, v.worst, v.where, v.over, v.size,
                                                                  '' if old is None else ' old max|d|/max|ref| {:.3e}'.format(old)))


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------

def _attention(ctx, qkv, heads, dtype):
    n, N, _ = qkv.shape
    out = np.empty((n, N, heads * KE.HD), dtype=np.uint16)
    rc = ctx.lib.mdhip_attention_on(ctx.h, _lib.np_ptr(_bits(qkv, dtype)), _lib.np_ptr(out), n, N, heads, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    return _from_bits(out, dtype)


@pytest.mark.parametrize('N', KE.ATTN_TOKENS)
@pytest.mark.parametrize('cls', KE.ATTN_CLASSES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_attention_every_element(contexts, dtype, cls, N):
    ctx = contexts('YOLO11N_TEST', dtype, (2, 64, 64))
    print()
    for heads in KE.ATTN_HEADS:
        qkv = KE.attention_input(cls, KE.ATTN_IMAGES, N, heads, dtype)
        ref = KE.AttentionReference(qkv, heads, dtype)
        KE.assert_attention_class(cls, ref)               # the case exercises what it is in the set for
        got = _attention(ctx, qkv, heads, dtype)
        v = ref.verdict('attention {} {} N={} heads={}'.format(dtype, cls, N, heads), got)
        _line('attention', dtype, '{} N={} heads={}'.format(cls, N, heads), v, KE.norm_wise(got, ref.y)[0])
        assert v.size == KE.ATTN_IMAGES * N * heads * KE.HD
        assert v.over == 0, str(v)


# ---------------------------------------------------------------------------------------------------------------------
# depthwise 3x3
# ---------------------------------------------------------------------------------------------------------------------

def _depthwise(ctx, a, w, b, r, mapping, act, dtype):
    _, c, ld_in, grp, grp_stride, grp_off = mapping
    n, _, h, wd = a.shape
    out = np.empty((n, h, wd, c), dtype=np.uint16)
    a_bits = _bits(np.transpose(a, (0, 2, 3, 1)), dtype)
    r_bits = None if r is None else _bits(np.transpose(r, (0, 2, 3, 1)), dtype)
    rc = ctx.lib.mdhip_dwconv3x3_on(ctx.h, _lib.np_ptr(a_bits), ld_in, _lib.np_ptr(w), _lib.np_ptr(b),
                                    None if r is None else _lib.np_ptr(r_bits), _lib.np_ptr(out), n, h, wd, c, grp, grp_stride,
                                    grp_off, act, None)
    assert rc == 0, ctx.lib.mdhip_last_error(ctx.h)
    return np.ascontiguousarray(np.transpose(_from_bits(out, dtype), (0, 3, 1, 2)))


@pytest.mark.parametrize('mapping', KE.DW_MAPPINGS, ids=lambda m: m[0])
@pytest.mark.parametrize('dtype', DTYPES)
def test_depthwise_every_element(contexts, dtype, mapping):
    ctx = contexts('YOLO11N_TEST', dtype, (2, 64, 64))
    name, c, ld_in, grp, grp_stride, grp_off = mapping
    print()
    for hw in KE.DW_MAPS:
        a, w, b, r = KE.depthwise_case(hw, mapping, dtype)
        wr = P.round_storage(w, dtype)                   # the hook rounds the fp32 weights to storage: nearest even, as this does
        for act in (0, 1):
            for res in (0, 1):
                rr = r if res else None
                got = _depthwise(ctx, a, w, b, rr, mapping, act, dtype)
                y, tol = KE.depthwise_reference(a, wr, b, rr, grp, grp_stride, grp_off, act, dtype)
                v = P.Verdict('depthwise {} {} {} act={} res={}'.format(dtype, name, hw, act, res), 9, got, y, tol)
                _line('depthwise', dtype, '{} {}x{} act={} res={} threads={}'.format(name, hw[0], hw[1], act, res, KE.dw_threads(hw, mapping)),
                      v, KE.norm_wise(got, y)[0])
                assert v.size == KE.DW_IMAGES * c * hw[0] * hw[1]
                assert v.over == 0, str(v)


# ---------------------------------------------------------------------------------------------------------------------
# the TTA input
# ---------------------------------------------------------------------------------------------------------------------

TTA_MODELS = {64: 'YOLOV5N6_TEST', 32: 'YOLOV5N_P5_TEST'}


@pytest.mark.parametrize('case', KE.TTA_CASES, ids=lambda c: 's{}-{}x{}'.format(c[0], *c[1]))
@pytest.mark.parametrize('dtype', DTYPES)
def test_tta_input_every_element(contexts, dtype, case):
    stride, (h, w) = case
    ctx = contexts(TTA_MODELS[stride], dtype, (2, 192, 320))
    assert ctx.lib.mdhip_max_stride(ctx.h) == stride
    n = 2
    imgs = KE.tta_images(n, h, w)
    ctx.preprocess(imgs, [(h, w, h, w, 0, 0)] * n, h, w)
    x = ctx.read_input(n, h, w)
    assert P.is_storage(x, dtype)
    assert all(x[i, :, :, :w // 2].mean() + 0.05 < x[i, :, :, w // 2:].mean() for i in range(n)), 'no left-to-right asymmetry'
    ctx.forward(n, h, w)
    before = ctx.read_predictions(n).copy()
    print()
    for tta_pass in (1, 2):
        got = ctx.tta_input_on(n, h, w, tta_pass)
        ref = KE.TtaReference(x, tta_pass, dtype, stride)
        assert got.shape == ref.y.shape, (got.shape, ref.geometry)
        inner, pad = ref.verdicts('tta input {} stride {} {}x{} pass {}'.format(dtype, stride, h, w, tta_pass), got)
        _line('tta_input', dtype, 'stride={} {}x{} pass={} resized {}x{} of {}x{}'.format(stride, h, w, tta_pass, *ref.geometry[:4]), inner)
        print('KE| tta_input {} stride={} {}x{} pass={} pad: {} of {} differ'.format(dtype, stride, h, w, tta_pass, pad.over, pad.size))
        assert P.is_storage(got, dtype)
        assert inner.over == 0, str(inner)
        assert pad.size > 0 and pad.over == 0, str(pad)
        # `input` holds the batch again, bit for bit
        assert np.array_equal(ctx.read_input(n, h, w).view(np.uint32), x.view(np.uint32))
    ctx.forward(n, h, w)
    assert np.array_equal(ctx.read_predictions(n).view(np.uint32), before.view(np.uint32))


def test_tta_input_error_returns(contexts):
    ctx = contexts('YOLOV5N6_TEST', 'bf16', (2, 192, 320))
    imgs = KE.tta_images(2, 64, 64)
    ctx.preprocess(imgs, [(64, 64, 64, 64, 0, 0)] * 2, 64, 64)
    x = ctx.read_input(2, 64, 64)
    oh, ow = _lib.C.c_int(), _lib.C.c_int()
    buf = np.empty((2, 3, 64, 64), dtype=np.float32)
    call = lambda n, h, w, p: ctx.lib.mdhip_tta_input_on(ctx.h, n, h, w, p, _lib.np_ptr(buf), _lib.C.byref(oh), _lib.C.byref(ow), None)
    for p in (0, 3, -1):
        assert call(2, 64, 64, p) == _lib.MDHIP_EINVAL, p
    assert call(2, 128, 64, 1) == _lib.MDHIP_EINVAL                   # not the batch of the last preprocess
    assert call(2, 96, 64, 1) == _lib.MDHIP_EINVAL                    # no multiple of the stride
    assert call(3, 64, 64, 1) != 0                                     # more than the context's batch
    assert ctx.lib.mdhip_tta_input_on(ctx.h, 2, 64, 64, 2, None, _lib.C.byref(oh), _lib.C.byref(ow), None) == 0
    assert (oh.value, ow.value) == KE.tta_geometry(64, 64, 2)[2:4]
    assert np.array_equal(ctx.read_input(2, 64, 64), x)
    free = contexts('YOLO11N_TEST', 'bf16', (2, 64, 64))
    assert free.lib.mdhip_tta_input_on(free.h, 1, 64, 64, 1, _lib.np_ptr(buf), _lib.C.byref(oh), _lib.C.byref(ow), None) == _lib.MDHIP_EUNSUPPORTED
    assert b'anchor-free' in free.lib.mdhip_last_error(free.h)
