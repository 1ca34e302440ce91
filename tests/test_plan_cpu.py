"""The planner on the CPU: what mdhip_create would plan (ops, names, arena and weight-arena offsets, packed bytes) and what it
refuses, against records made by the planner of the commit BEFORE the planner moved to mdhip_plan.cpp.

hip_backend.describe_plan (mdhip_plan_describe) runs the host part of mdhip_create without a device and writes the plan as
text.  tests/golden/plans/ holds, for the synthetic weights of weights_io (seed 1):
  * the whole text for the toy models (<model>_<dtype>_<batch>x<h>x<w>.txt.gz: gzip, `zcat` shows it),
  * full_models.json: SHA-256 and line count of the text for the full-size models (the texts themselves are large) and the op
    names of each model,
  * errors.json: return code and message for malformed model descriptions.
A planner change that is meant to keep plans as they are must leave every one of them equal.  A change that is meant to alter
a plan records them again: `python tests/test_plan_cpu.py record` writes the files from the library that is built -- run it
on a build of the commit whose plans are the reference (with mdhip_plan_describe available there), never to make a failing
comparison pass.
"""

import functools
import gzip
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

PLANS = os.path.join(GOLDEN, 'plans')
SEED = 1

TOY = [(model, dtype, (2, 256, 320))
       for model, dtypes in [('YOLOV5N6_TEST', ('bf16', 'fp16', 'fp8')), ('YOLOV5N_P5_TEST', ('bf16', 'fp16', 'fp8')),
                             ('YOLOV5S6_TEST', ('bf16', 'fp16', 'fp8')), ('YOLO11N_TEST', ('bf16', 'fp16')),
                             ('GELAN_TEST', ('bf16', 'fp16')), ('YOLOV9_DUAL_TEST', ('bf16', 'fp16'))]
       for dtype in dtypes]
TOY.append(('YOLOV5N6_TEST', 'bf16', (3, 250, 300)))        # a capacity that is rounded up to the model stride

FULL = [(model, dtype, (32, 1280, 1280))
        for model, dtypes in [('YOLOV5X6_MD', ('bf16', 'fp16', 'fp8')), ('YOLO11L_MD', ('bf16', 'fp16')),
                              ('YOLO11S_MD', ('bf16', 'fp16')), ('YOLOV9C_MD', ('bf16', 'fp16'))]
        for dtype in dtypes]


def _key(model, dtype, cap):
    return '{}_{}_{}x{}x{}'.format(model, dtype, *cap)


@functools.lru_cache(maxsize=2)
def _weights(model):
    from megadetector_amd import weights_io, yolo_yaml
    return weights_io.synthetic_weights(getattr(yolo_yaml, model), seed=SEED)


def _describe(model, dtype, cap):
    from megadetector_amd import hip_backend
    return hip_backend.describe_plan(_weights(model), dtype, *cap)


def _op_names(text):
    return [line.split('"')[1] for line in text.splitlines() if line.startswith('op ')]


# ---- malformed descriptions -------------------------------------------------------------------------------------------------

def _spec(W, type_, nth=0, **attrs):
    """the nth layer of this type (and, with attrs, whose attributes equal them)"""
    hits = [s for s in W.specs if s.type == type_ and all(getattr(s, k) == v for k, v in attrs.items())]
    return hits[nth]


def _reshape_conv(W, name, shape):
    """the conv `name` with another shape (leading corner of the old weights, zeros beyond)"""
    old = W.weights[name + '.weight']
    new = np.zeros(shape, dtype=np.float32)
    common = tuple(slice(0, min(a, b)) for a, b in zip(old.shape, shape))
    new[common] = old[common]
    W.weights[name + '.weight'] = new
    W.weights[name + '.bias'] = np.ascontiguousarray(np.resize(W.weights[name + '.bias'], shape[0]), dtype=np.float32)


def _c3_hidden(W):
    s = _spec(W, M.MDHIP_C3)
    w = W.weights[s.conv_names[1] + '.weight']
    _reshape_conv(W, s.conv_names[1], (w.shape[0] + 8,) + w.shape[1:])


def _c3k2_short(W):
    k = _spec(W, M.MDHIP_C3K2).index
    del W.specs[k + 1:]
    W.specs[k].conv_names = W.specs[k].conv_names[:-1]


def _from_order(W):
    W.specs[5].frm = [7]


def _stem5(W):
    w = W.weights[W.specs[0].conv_names[0] + '.weight']
    _reshape_conv(W, W.specs[0].conv_names[0], (w.shape[0], 3, 5, 5))


def _detect_stride(W):
    W.strides = [2 * W.strides[0]] + list(W.strides[1:])


def _cbfuse_offset(W):
    _spec(W, M.MDHIP_CBFUSE).k = 4


def _upsample_input(W):
    _spec(W, M.MDHIP_UPSAMPLE).frm = [-1]


def _channels(W):
    W.specs[1].c_out = 12


def _detect_nl(W):
    W.nl -= 1


def _adown_input(W):
    _spec(W, M.MDHIP_ADOWN).frm = [-1]


def _unknown_type(W):
    W.specs[3].type = 99


def _detect_conv(W):
    W.nc += 1


def _c3_reads_input(W):
    _spec(W, M.MDHIP_C3).frm = [-1]


def _repncsp_kernel(W):
    s = _spec(W, M.MDHIP_ELAN4)
    w = W.weights[s.conv_names[4] + '.weight']          # cv2.0.m.0.cv1, a 3x3
    _reshape_conv(W, s.conv_names[4], w.shape[:2] + (1, 1))


def _c3k_kernel(W):
    s = _spec(W, M.MDHIP_C3K2, k=1)
    w = W.weights[s.conv_names[5] + '.weight']          # m.0.m.0.cv1, a 3x3
    _reshape_conv(W, s.conv_names[5], w.shape[:2] + (1, 1))


def _c3k_hidden(W):
    s = _spec(W, M.MDHIP_C3K2, k=1)
    w = W.weights[s.conv_names[3] + '.weight']          # m.0.cv2
    _reshape_conv(W, s.conv_names[3], (w.shape[0] + 8,) + w.shape[1:])


def _nothing(W):
    pass


#: name -> (model, dtype, capacity, what to break)
ERRORS = {
    'c3_hidden_widths_disagree': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _c3_hidden),
    'c3k2_conv_table_one_short': ('YOLO11N_TEST', 'bf16', (2, 256, 320), _c3k2_short),
    'from_index_out_of_order': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _from_order),
    'stem_5x5': ('YOLOV5N6_TEST', 'fp16', (2, 256, 320), _stem5),
    'detect_stride_contradicts_graph': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _detect_stride),
    'detect_stride_contradicts_graph_dfl': ('YOLO11N_TEST', 'bf16', (2, 256, 320), _detect_stride),
    'detect_stride_contradicts_graph_ddfl': ('GELAN_TEST', 'bf16', (2, 256, 320), _detect_stride),
    'cbfuse_offset_not_multiple_of_8': ('YOLOV9_DUAL_TEST', 'bf16', (2, 256, 320), _cbfuse_offset),
    'upsample_of_network_input': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _upsample_input),
    'channels_not_multiple_of_8': ('YOLOV5N6_TEST', 'fp8', (2, 256, 320), _channels),
    'anchor_free_fp8': ('YOLO11N_TEST', 'fp8', (2, 256, 320), _nothing),
    'anchor_free_fp8_yolov9': ('GELAN_TEST', 'fp8', (2, 256, 320), _nothing),
    'detect_inputs_not_nl': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _detect_nl),
    'adown_of_network_input': ('GELAN_TEST', 'bf16', (2, 256, 320), _adown_input),
    'unknown_layer_type': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _unknown_type),
    'detect_conv_shape': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _detect_conv),
    'c3_reads_network_input': ('YOLOV5N6_TEST', 'bf16', (2, 256, 320), _c3_reads_input),
    'repncsp_kernel_size': ('GELAN_TEST', 'bf16', (2, 256, 320), _repncsp_kernel),
    'c3k_kernel_size': ('YOLO11N_TEST', 'bf16', (2, 256, 320), _c3k_kernel),
    'c3k_hidden_widths_disagree': ('YOLO11N_TEST', 'bf16', (2, 256, 320), _c3k_hidden),
    'capacity_too_small': ('YOLOV5N6_TEST', 'bf16', (2, 32, 320), _nothing),
    'batch_zero': ('YOLOV5N6_TEST', 'bf16', (0, 256, 320), _nothing),
}


class _Lazy:
    """megadetector_amd.yolo_model, imported at first use (the module constants above need no package import)"""
    def __getattr__(self, name):
        from megadetector_amd import yolo_model
        return getattr(yolo_model, name)


M = _Lazy()


def _error_of(name):
    from megadetector_amd import hip_backend, weights_io, yolo_yaml
    from megadetector_amd._lib import HipError
    model, dtype, cap, breaker = ERRORS[name]
    W = weights_io.synthetic_weights(getattr(yolo_yaml, model), seed=SEED)       # (its own copy: the breaker edits it)
    breaker(W)
    try:
        hip_backend.describe_plan(W, dtype, *cap)
    except HipError as e:
        return {'code': e.code, 'message': str(e).split(': ', 1)[1]}
    return {'code': 0, 'message': ''}


# ---- the tests --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module', autouse=True)
def _built():
    import __graft_entry__ as G
    G.build()


@pytest.mark.parametrize('model,dtype,cap', TOY, ids=[_key(*t) for t in TOY])
def test_toy_plan_is_the_recorded_one(model, dtype, cap):
    want = gzip.open(os.path.join(PLANS, _key(model, dtype, cap) + '.txt.gz'), 'rt').read()
    got = _describe(model, dtype, cap)
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        pytest.fail('{}: {} lines against {} recorded; first difference at line {}:\n  got      {}\n  recorded {}'.format(
            _key(model, dtype, cap), len(g), len(w), first + 1, g[first] if first < len(g) else '<end>',
            w[first] if first < len(w) else '<end>'))


@pytest.mark.parametrize('model,dtype,cap', FULL, ids=[_key(*t) for t in FULL])
def test_full_model_plan_is_the_recorded_one(model, dtype, cap):
    recorded = json.load(open(os.path.join(PLANS, 'full_models.json')))
    want = dict(recorded['plans'][_key(model, dtype, cap)], ops=recorded['ops'][model])
    got = _describe(model, dtype, cap)
    names = _op_names(got)
    if names != want['ops']:
        first = next((i for i in range(min(len(names), len(want['ops']))) if names[i] != want['ops'][i]),
                     min(len(names), len(want['ops'])))
        pytest.fail('{}: {} ops against {} recorded; the first op whose name differs is op {}: got {!r}, recorded {!r}'.format(
            _key(model, dtype, cap), len(names), len(want['ops']), first, names[first] if first < len(names) else None,
            want['ops'][first] if first < len(want['ops']) else None))
    assert len(got.splitlines()) == want['lines']
    assert hashlib.sha256(got.encode()).hexdigest() == want['sha256'], (
        '{}: same ops and names, another digest: an offset, a field or packed bytes differ -- write the text with '
        'hip_backend.describe_plan on this build and on a build of the parent commit and diff the two'.format(_key(model, dtype, cap)))


@pytest.mark.parametrize('name', sorted(ERRORS))
def test_malformed_description_is_refused_as_recorded(name):
    want = json.load(open(os.path.join(PLANS, 'errors.json')))[name]
    assert want['code'] < 0 and want['message']
    assert _error_of(name) == want


def test_describe_reports_the_length_it_needs_and_truncates():
    import ctypes as C
    from megadetector_amd import _lib, hip_backend
    lib = _lib.load()
    m, keep = hip_backend.model_description(_weights('YOLOV5N6_TEST'))
    text = _describe('YOLOV5N6_TEST', 'bf16', (2, 256, 320))
    args = (C.byref(m), _lib.MDHIP_DTYPE_BF16, 2, 256, 320)
    assert lib.mdhip_plan_describe(*args, None, 0) == len(text)
    buf = C.create_string_buffer(b'\xff' * 64, 64)
    assert lib.mdhip_plan_describe(*args, buf, 32) == len(text)
    assert buf.raw[:32] == text.encode()[:31] + b'\0' and buf.raw[32:] == b'\xff' * 32
    assert lib.mdhip_plan_describe(None, _lib.MDHIP_DTYPE_BF16, 2, 256, 320, None, 0) < 0
    assert b'empty model description' in lib.mdhip_last_error(None)


def record():
    os.makedirs(PLANS, exist_ok=True)
    for model, dtype, cap in TOY:
        with open(os.path.join(PLANS, _key(model, dtype, cap) + '.txt.gz'), 'wb') as f:
            with gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0, compresslevel=9) as g:
                g.write(_describe(model, dtype, cap).encode())
    plans, ops = {}, {}
    for model, dtype, cap in FULL:
        text = _describe(model, dtype, cap)
        plans[_key(model, dtype, cap)] = {'sha256': hashlib.sha256(text.encode()).hexdigest(), 'lines': len(text.splitlines())}
        assert ops.setdefault(model, _op_names(text)) == _op_names(text)      # (a model's op names do not depend on the storage type)
        print(_key(model, dtype, cap), len(text), plans[_key(model, dtype, cap)]['sha256'])
    with open(os.path.join(PLANS, 'full_models.json'), 'w') as f:          # one plan, one model per line
        f.write('{"plans": {\n' + ',\n'.join(' {}: {}'.format(json.dumps(k), json.dumps(v)) for k, v in plans.items()))
        f.write('\n},\n"ops": {\n' + ',\n'.join(' {}: {}'.format(json.dumps(k), json.dumps(v)) for k, v in ops.items()) + '\n}}\n')
    errors = {name: _error_of(name) for name in sorted(ERRORS)}
    for name, e in errors.items():
        print(name, e)
    json.dump(errors, open(os.path.join(PLANS, 'errors.json'), 'w'), indent=1, sort_keys=True)


if __name__ == '__main__' and sys.argv[1:] == ['record']:
    record()
