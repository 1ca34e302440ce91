"""The device-free description of a plan (hip_backend.describe_plan, pinned on the CPU by tests/test_plan_cpu.py) is the plan
of the context that runs: same ops, same names, in order; and that context's forward runs."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('model', ['YOLOV5N6_TEST', 'YOLO11N_TEST', 'GELAN_TEST'])
def test_described_plan_is_the_plan_of_the_context(model):
    from megadetector_amd import hip_backend, weights_io, yolo_yaml
    W = weights_io.synthetic_weights(getattr(yolo_yaml, model), seed=1)
    text = hip_backend.describe_plan(W, 'bf16', 2, 256, 320)
    described = [line.split('"')[1] for line in text.splitlines() if line.startswith('op ')]
    ctx = hip_backend.HipContext(W, dtype='bf16', max_batch=2, max_h=256, max_w=320)
    try:
        assert ctx.num_ops() == len(described)
        # (mdhip_op_info.name holds 47 characters)
        assert [o['name'] for o in ctx.op_infos()] == [name[:47] for name in described]
        ctx.forward(2, 256, 320)
        pred = ctx.read_predictions(2)
        assert pred.shape == (2, ctx.num_anchors(256, 320), ctx.no) and np.isfinite(pred).all()
    finally:
        ctx.close()
