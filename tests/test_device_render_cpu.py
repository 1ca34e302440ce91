"""
device_render without a GPU: the pure parts of the shared device render path -- the packing of the label patches of a batch,
RenderPlan.extend, the encoder's two-try loop (on a CPU tensor with a stand-in for the encoder), the greedy chunker against the
chunk lists the loops it replaced cut the test scenes into (tests/golden/device_render_chunks.json), the profiling clock, the
chunk driver of the results-file tools, its resample stage and its encode tail on stand-ins for torch, the context and the
encoders, the host leg's pool, device_decode.plan_source on files Pillow writes -- and preview.stacked_labels for one string
against the single-label arithmetic it replaced.
"""

import ctypes
import json
import os
from contextlib import contextmanager

import numpy as np
import pytest

import rde_review_scene as RS
import separate_scene as SS
from megadetector_amd import device_decode as DD
from megadetector_amd import device_render as DR
from megadetector_amd import jpeg_host as J
from megadetector_amd import preview as PV
from megadetector_amd._lib import HipError

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'device_render_chunks.json')) as _f:
    CHUNKS = json.load(_f)


# ---- pack_ops --------------------------------------------------------------------------------------------------------------------

def _plan(rows):
    """a RenderPlan of ('rect', x0, y0, x1, y1, colour) and ('patch', x, y, w, h, bytes) rows"""
    plan = PV.RenderPlan()
    for kind, a, b, c, d, e in rows:
        if kind == 'rect':
            plan.ops.append([PV.OP_RECT, a, b, c, d, e, 0, 0])
        else:
            plan.ops.append([PV.OP_PATCH, a, b, c, d, plan.add_patch(e), 0, 0])
    return plan


def test_pack_ops_stores_a_shared_patch_once_and_keeps_the_order():
    shared, other = bytes(range(2 * 3 * 3)), bytes(range(100, 100 + 1 * 2 * 3))
    first = _plan([('rect', 1, 2, 3, 4, 0x0000FF), ('patch', 5, 6, 2, 3, shared), ('patch', 0, 0, 1, 2, other), ('patch', 9, 9, 2, 3, shared)])
    second = _plan([('patch', 7, 1, 2, 3, shared), ('rect', 0, 0, 9, 9, 0x00FF00)])
    plans = [first, PV.RenderPlan(), second]
    assert first.patches == shared + other                                # (the plan itself holds a repeated patch once)
    op_image, ops, packed = DR.pack_ops(plans)
    assert op_image == [0, 0, 0, 0, 2, 2]                                 # the empty plan contributes nothing
    assert bytes(packed) == shared + other                                # each patch once, in the order of first use
    flat = [(k, op) for k, plan in enumerate(plans) for op in plan.ops]
    assert len(ops) == len(flat)
    for image, row, (k, op) in zip(op_image, ops, flat):
        assert image == k and len(row) == 8
        if op[0] == PV.OP_RECT:
            assert row == op                                              # untouched
        else:
            assert row[:5] == op[:5] and row[6:] == op[6:]
            assert bytes(packed[row[5]:row[5] + row[3] * row[4] * 3]) == plans[k].patch_of(op)
    assert [row[5] for row in ops if row[0] == PV.OP_PATCH] == [0, len(shared), 0, 0]
    assert first.ops[3][5] == 0 and second.ops[0][5] == 0                 # (the plans are not changed)
    assert DR.pack_ops([]) == ([], [], bytearray()) and DR.pack_ops([PV.RenderPlan()]) == ([], [], bytearray())


# ---- RenderPlan.extend ------------------------------------------------------------------------------------------------------------

def _category_plan(detections, category, width, height):
    """the render_plan of one category pass of separate_detections with show_box_labels, at the thickness of 'blur_and_boxes'"""
    o = PV.PreviewOptions(confidence_threshold=0.2, output_image_width=None, box_thickness=3, box_expansion=0)
    return PV.render_plan([d for d in detections if d['category'] == category], width, height, o, SS.DETECTION_CATEGORIES, True)


def test_extend_draws_what_the_two_plans_draw_one_after_the_other():
    """Two category passes over all3.jpg of the separate scene at its own 96 x 64.  The patch bytes come from the installed
    font, so nothing recorded is compared: the extended plan must draw, by the host model of mdhip_draw_ops, exactly what the
    two plans draw one after the other, and its rows must be theirs with only the patch offsets rewritten."""
    name, width, height, _, detections = next(im for im in SS.IMAGES if im[0] == 'all3.jpg')
    animal, person = _category_plan(detections, '1', width, height), _category_plan(detections, '2', width, height)
    for plan in (animal, person):
        assert sum(op[0] == PV.OP_RECT for op in plan.ops) == 4 and sum(op[0] == PV.OP_PATCH for op in plan.ops) == 1
    both = PV.RenderPlan().extend(animal).extend(person)
    assert len(both.ops) == len(animal.ops) + len(person.ops)
    for row, (plan, op) in zip(both.ops, [(animal, op) for op in animal.ops] + [(person, op) for op in person.ops]):
        if op[0] == PV.OP_RECT:
            assert row == op
        else:
            assert row[:5] == op[:5] and row[6:] == op[6:] and both.patch_of(row) == plan.patch_of(op)
    assert bytes(both.patches) == bytes(animal.patches) + bytes(person.patches)        # different labels: two patches
    assert both.labels == animal.labels + person.labels and both.order == animal.order + person.order
    one_by_one = np.full((height, width, 3), 77, dtype=np.uint8)
    for plan in (animal, person):
        assert J.draw_ops(one_by_one, plan.ops, bytes(plan.patches)) == J.MDJPEG_OK
    together = np.full((height, width, 3), 77, dtype=np.uint8)
    assert J.draw_ops(together, both.ops, bytes(both.patches)) == J.MDJPEG_OK
    assert np.array_equal(together, one_by_one) and (together != 77).any()
    # a patch both plans hold is kept once, and the rows of both point at it
    twice = PV.RenderPlan().extend(animal).extend(animal)
    assert bytes(twice.patches) == bytes(animal.patches) and twice.ops == animal.ops + animal.ops
    assert len(animal.ops) == 5 and len(person.ops) == 5                   # (extend leaves the other plan alone)


# ---- read_encoded -----------------------------------------------------------------------------------------------------------------

class _Encoder:
    """stands in for an encoder call: writes `scan` when the buffer holds it, else asks for len(scan) + slack bytes"""

    def __init__(self, scan, refuse=0, extra=()):
        self.scan, self.refuse, self.extra, self.calls = scan, refuse, tuple(extra), []

    def __call__(self, out_ptr, capacity):
        self.calls.append(capacity)
        if len(self.calls) <= self.refuse or capacity < len(self.scan):
            return (False, [], [], len(self.scan)) + self.extra
        ctypes.memmove(out_ptr, self.scan, len(self.scan))
        return (True, [0, 4], [4, len(self.scan) - 4], len(self.scan)) + self.extra


def test_read_encoded_makes_one_call_when_the_guess_holds():
    scan = bytes(range(10, 30))
    call = _Encoder(scan, extra=([0, 1],))
    host, offs, lens, rest = DR.read_encoded(call, 64, 'cpu', 'mdhip_test')
    assert call.calls == [64]
    assert host.tobytes() == scan and (offs, lens, rest) == ([0, 4], [4, 16], [[0, 1]])


def test_read_encoded_calls_once_more_with_the_size_asked_for():
    scan = bytes(range(40))
    call = _Encoder(scan)
    host, offs, lens, rest = DR.read_encoded(call, 8, 'cpu', 'mdhip_test')
    assert call.calls == [8, len(scan)]
    assert host.tobytes() == scan and rest == []
    assert [host[o:o + n].tobytes() for o, n in zip(offs, lens)] == [scan[:4], scan[4:]]


def test_read_encoded_raises_when_the_size_asked_for_is_refused_too():
    call = _Encoder(bytes(40), refuse=2)
    with pytest.raises(RuntimeError, match=r'^mdhip_test asked for 40 bytes and refused a buffer of that size$'):
        DR.read_encoded(call, 8, 'cpu', 'mdhip_test')
    assert call.calls == [8, 40]


# ---- chunked ----------------------------------------------------------------------------------------------------------------------

def test_chunked_cuts_greedily():
    size = lambda item: item[1]
    items = [('a', 5), ('b', 5), ('c', 11), ('d', 1), ('e', 9), ('f', 1)]
    assert DR.chunked(items, size, 10) == [[('a', 5), ('b', 5)], [('c', 11)], [('d', 1), ('e', 9)], [('f', 1)]]
    assert DR.chunked([('c', 11)], size, 10) == [[('c', 11)]] and DR.chunked([], size, 10) == []
    assert DR.chunked([('x', 0)] * 3, size, 0) == [[('x', 0)] * 3]
    same_name = lambda chunk, item: any(c[0] == item[0] for c in chunk)
    assert DR.chunked([('a', 1), ('b', 1), ('a', 1), ('a', 1)], size, 10, same_name) == [[('a', 1), ('b', 1)], [('a', 1)], [('a', 1)]]
    rng = np.random.default_rng(3)
    for _ in range(50):
        items = [(int(k), int(s)) for k, s in zip(rng.integers(0, 4, 12), rng.integers(0, 30, 12))]
        chunks = DR.chunked(items, size, 40, same_name)
        assert all(chunks) and [i for c in chunks for i in c] == items
        for c in chunks:
            assert len(c) == 1 or (sum(s for _, s in c) <= 40 and len({k for k, _ in c}) == len(c))


def test_chunked_cuts_the_scenes_as_the_loops_it_replaced():
    """the planned copies of separate_detections over the separate scene ('blur_and_boxes'; with keep_source_blocks the
    coefficients count too; `twice`: a422.jpg a second time in the results) and the files each location of the RDE review
    scene needs, at several limits: the chunks the tools' own loops made before they shared this one"""
    same_file = lambda chunk, item: any(c[0] == item[0] for c in chunk)
    pixels = {name: w * h * 3 for name, w, h, _, _ in SS.IMAGES}
    assert len(CHUNKS['separate']) == 4 and len(CHUNKS['rde_review']) == len(RS.CAMERAS)
    n = 0
    for case in CHUNKS['separate']:
        items = [tuple(item) for item in case['items']]
        assert all(size >= pixels[f] and (case['keep_source_blocks'] or size == pixels[f]) for f, size in items)
        assert (len(items) != len({f for f, _ in items})) == case['twice']
        for limit, chunks in case['chunks'].items():
            assert [[f for f, _ in c] for c in DR.chunked(items, lambda item: item[1], int(limit), same_file)] == chunks, (case, limit)
            n += 1
    for camera, case in zip(RS.CAMERAS, CHUNKS['rde_review']):
        items = [tuple(item) for item in case['items']]
        assert all(f.startswith(camera + '/') for f, _ in items)
        for limit, chunks in case['chunks'].items():
            assert [[f for f, _ in c] for c in DR.chunked(items, lambda item: item[1], int(limit))] == chunks, (camera, limit)
            n += 1
    assert n == 4 * 5 + 2 * 4
    assert any(len(c) > 1 for case in CHUNKS['separate'] for chunks in case['chunks'].values() for c in chunks)
    assert DR.DECODE_CHUNK_BYTES == 256 << 20 and str(DR.DECODE_CHUNK_BYTES) in CHUNKS['separate'][0]['chunks']


# ---- Clock ------------------------------------------------------------------------------------------------------------------------

class _NoTorch:
    def __getattr__(self, name):
        raise AssertionError('torch.{} was touched'.format(name))


class _Torch:
    def __init__(self):
        self.synced = []
        self.cuda = self

    def synchronize(self, device):
        self.synced.append(device)


def test_clock_without_a_dict_touches_nothing():
    clock = DR.Clock(_NoTorch(), 'cuda:0', None)
    ran = []
    with clock('decode'):
        ran.append(1)
    assert ran == [1]


def test_clock_adds_to_its_key_and_waits_for_the_device_around_the_block():
    torch, ms = _Torch(), {'draw': 1.0}
    clock = DR.Clock(torch, 'cuda:1', ms)
    with clock('decode'):
        assert torch.synced == ['cuda:1']
    first = ms['decode']
    with clock('decode'):
        pass
    with clock('draw'):
        pass
    assert torch.synced == ['cuda:1'] * 6
    assert first >= 0.0 and ms['decode'] >= first and ms['draw'] >= 1.0 and set(ms) == {'decode', 'draw'}


# ---- run_chunks -------------------------------------------------------------------------------------------------------------------

class _Cuda:
    def __init__(self):
        self.synced, self.entered = [], []

    def synchronize(self, device):
        self.synced.append(device)

    @contextmanager
    def device(self, device):
        self.entered.append(device)
        yield


class _Tensor:
    def __init__(self, n, ptr):
        self.n, self.ptr = n, ptr

    def data_ptr(self):
        return self.ptr


class _DeviceTorch:
    """what run_chunks and resample_stage touch of torch: device, empty, cuda.device and cuda.synchronize"""
    uint8 = 'uint8'

    def __init__(self):
        self.cuda, self.made = _Cuda(), []

    def device(self, name):
        return name

    def empty(self, n, dtype, device):
        assert dtype == self.uint8
        self.made.append(_Tensor(n, 0x1000 * (len(self.made) + 1)))
        return self.made[-1]


class _Context:
    device = 1

    def __init__(self):
        self.resample_calls = []

    def resample_lanczos(self, *args):
        self.resample_calls.append(args)


MB = 1 << 20
JOBS = [{'file': f, 'bytes': n * MB} for f, n in (('a', 100), ('b', 100), ('c', 100), ('a', 1), ('d', 300), ('e', 1))]
JOB_CHUNKS = [['a', 'b'], ['c', 'a'], ['d'], ['e']]                      # under 256 MiB; the second 'a' would break the first chunk anyway


def _drive(render_chunk, profile=False, items=JOBS, **kw):
    torch, ctx, counts = _DeviceTorch(), _Context(), {'decode_chunks': 0, 'ms': {}}
    seen = []

    def wrapped(*args):
        seen.append(args)
        return render_chunk(args[3])

    try:
        host = DR.run_chunks(ctx, torch, items, lambda j: j['bytes'], wrapped, counts, profile, **kw)
    finally:
        counts['seen'], counts['torch'], counts['ctx'] = seen, torch, ctx
    return host, counts


def test_run_chunks_renders_each_chunk_of_chunked_once():
    assert [[j['file'] for j in c] for c in DR.chunked(JOBS, lambda j: j['bytes'], DR.DECODE_CHUNK_BYTES, DR.file_twice)] == JOB_CHUNKS
    for profile in (False, True):
        host, counts = _drive(lambda chunk: [], profile, also_break=DR.file_twice)
        assert host == [] and counts['decode_chunks'] == len(JOB_CHUNKS) == len(counts['seen'])
        assert [c for _, _, _, c, _ in counts['seen']] == DR.chunked(JOBS, lambda j: j['bytes'], DR.DECODE_CHUNK_BYTES, DR.file_twice)
        for ctx, torch, device, _, clock in counts['seen']:
            assert ctx is counts['ctx'] and torch is counts['torch'] and device == 'cuda:1'
            assert isinstance(clock, DR.Clock) and clock.device == 'cuda:1' and clock.ms is (counts['ms'] if profile else None)
        assert counts['torch'].cuda.entered == ['cuda:1'] and counts['torch'].cuda.synced == ['cuda:1']
    # without the rule for a file listed twice only the bytes cut
    _, counts = _drive(lambda chunk: [])
    assert [[j['file'] for j in c] for _, _, _, c, _ in counts['seen']] == [['a', 'b'], ['c', 'a'], ['d'], ['e']]
    _, counts = _drive(lambda chunk: [], items=JOBS[:2] + JOBS[3:4])
    assert [[j['file'] for j in c] for _, _, _, c, _ in counts['seen']] == [['a', 'b', 'a']]
    host, counts = _drive(lambda chunk: [], items=[])
    assert host == [] and counts['decode_chunks'] == 0 and counts['torch'].cuda.synced == ['cuda:1']


def test_run_chunks_gives_the_refused_jobs_back_in_the_order_of_the_input():
    unplanned = [{'file': 'x', 'place': 2.5}, {'file': 'y', 'place': 9}]
    for k, job in enumerate(JOBS):
        job['place'] = k
    refuse = lambda chunk: [j for j in reversed(chunk) if j['file'] in ('a', 'd')]
    host, _ = _drive(refuse, host=unplanned, also_break=DR.file_twice, order=lambda j: j['place'])
    assert [(j['file'], j['place']) for j in host] == [('a', 0), ('x', 2.5), ('a', 3), ('d', 4), ('y', 9)]
    # without an order: what could not be planned, then what each chunk gave back, as it gave it back
    host, _ = _drive(refuse, host=unplanned, also_break=DR.file_twice)
    assert [(j['file'], j['place']) for j in host] == [('x', 2.5), ('y', 9), ('a', 0), ('a', 3), ('d', 4)]
    assert unplanned == [{'file': 'x', 'place': 2.5}, {'file': 'y', 'place': 9}]         # (the caller's list is not changed)


def test_run_chunks_hands_a_chunk_that_fails_on_the_device_to_the_host_leg(capsys):
    def render(chunk):
        if chunk[0]['file'] == 'c':
            raise HipError('mdhip_draw_ops failed (7)')
        return [j for j in chunk if j['file'] == 'e']

    host, counts = _drive(render, also_break=DR.file_twice)
    assert [j['file'] for j in host] == ['c', 'a', 'e'] and host[0] is JOBS[2] and host[1] is JOBS[3]
    assert capsys.readouterr().out == 'Warning: rendering 2 images on the device failed (mdhip_draw_ops failed (7)); PIL renders them\n'
    assert counts['decode_chunks'] == 4 and [c[0]['file'] for _, _, _, c, _ in counts['seen']] == ['a', 'c', 'd', 'e']
    assert counts['torch'].cuda.synced == ['cuda:1']                     # the wait at the end, once, failed chunk or not


def test_run_chunks_counts_and_flattens_the_jobs_of_grouped_items(capsys):
    groups = [[{'file': 'a', 'n': 0}, {'file': 'a', 'n': 1}, {'file': 'a', 'n': 2}], [{'file': 'b', 'n': 3}], [{'file': 'c', 'n': 4}]]

    def render(chunk):
        if len(chunk) == 2:
            raise HipError('out of memory')
        return []

    torch, counts = _DeviceTorch(), {'decode_chunks': 0}
    host = DR.run_chunks(_Context(), torch, groups, lambda g: (100 if g[0]['file'] != 'c' else 200) * MB,
                         lambda ctx, torch, device, chunk, clock: render(chunk), counts, False, [{'file': 'z', 'n': 2.5}], jobs_of=list,
                         order=lambda j: j['n'])
    assert [j['n'] for j in host] == [0, 1, 2, 2.5, 3] and counts['decode_chunks'] == 2
    assert capsys.readouterr().out == 'Warning: rendering 4 images on the device failed (out of memory); PIL renders them\n'


def test_run_chunks_lets_every_other_exception_through():
    def render(chunk):
        if chunk[0]['file'] == 'c':
            raise ValueError('not the device')
        return []

    with pytest.raises(ValueError, match='^not the device$'):
        _drive(render)


# ---- resample_stage ---------------------------------------------------------------------------------------------------------------

def test_resample_stage_returns_the_sources_themselves_where_no_size_changes():
    torch, ctx, clock = _DeviceTorch(), _Context(), DR.Clock(_NoTorch(), 'cuda:1', None)
    sources = [_Tensor(12 * 8 * 3, 0x10), _Tensor(5 * 7 * 3, 0x20)]
    out, made = DR.resample_stage(ctx, torch, 'cuda:1', sources, [(12, 8), (5, 7)], [(12, 8), (5, 7)], clock)
    assert made is False and len(out) == 2 and all(o is s for o, s in zip(out, sources))
    assert ctx.resample_calls == [] and torch.made == []
    assert DR.resample_stage(ctx, torch, 'cuda:1', [], [], [], clock) == ([], False)


def test_resample_stage_makes_one_call_for_the_images_whose_size_changes():
    torch, ctx, ms = _DeviceTorch(), _Context(), {}
    clock = DR.Clock(_Torch(), 'cuda:1', ms)
    sources = [_Tensor(12 * 8 * 3, 0x10), _Tensor(5 * 7 * 3, 0x20), _Tensor(9 * 9 * 3, 0x30), _Tensor(4 * 2 * 3, 0x40)]
    source_sizes, sizes = [(12, 8), (5, 7), (9, 9), (4, 2)], [(6, 4), (5, 7), (9, 9), (40, 20)]
    out, made = DR.resample_stage(ctx, torch, 'cuda:1', sources, source_sizes, sizes, clock)
    assert made is True and out[1] is sources[1] and out[2] is sources[2]
    assert [t.n for t in torch.made] == [6 * 4 * 3, 40 * 20 * 3] and out[0] is torch.made[0] and out[3] is torch.made[1]
    assert ctx.resample_calls == [([0x10, 0x40], [(12, 8), (4, 2)], [36, 12], [0x1000, 0x2000], [(6, 4), (40, 20)], [18, 120])]
    assert set(ms) == {'resample'}


# ---- encode_copies ----------------------------------------------------------------------------------------------------------------

def _encoders(monkeypatch, flag):
    """encode_kept and encode_sampled stood in for: -> the calls, as (encoder, the jobs' names); the kept call flags `flag`"""
    calls = []

    def kept(ctx, device, tensors, jobs, source_ptrs, stream=0):
        assert source_ptrs == [j['ptr'] for j in jobs] and tensors == [j['name'].upper() for j in jobs]
        calls.append(('kept', [j['name'] for j in jobs]))
        return [None if j['name'] in flag else 'kept ' + j['name'] for j in jobs]

    def sampled(ctx, device, tensors, jobs, stream=0):
        assert tensors == [j['name'].upper() for j in jobs]
        calls.append(('sampled', [j['name'] for j in jobs]))
        return ['sampled ' + j['name'] for j in jobs]

    monkeypatch.setattr(DR, 'encode_kept', kept)
    monkeypatch.setattr(DR, 'encode_sampled', sampled)
    return calls


@pytest.mark.parametrize('reencode_flagged', [True, False])
def test_encode_copies_makes_one_call_of_each_encoder_the_jobs_need(monkeypatch, reencode_flagged):
    """separate_detections (reencode_flagged) encodes a copy the kept call flagged whole, in the SAME sampled call as the copies
    without 'keep'; visualize_video_output leaves it to the host leg.  Either way at most one call of each encoder per chunk."""
    clock = DR.Clock(_NoTorch(), 'cuda:0', None)
    jobs = [{'name': n, 'keep': k, 'ptr': p} for n, k, p in (('a', True, 1), ('b', False, None), ('c', True, 3), ('d', False, None))]

    def run(jobs, flag=()):
        calls = _encoders(monkeypatch, flag)
        return DR.encode_copies(None, 'cuda:0', [j['name'].upper() for j in jobs], jobs, [j['ptr'] for j in jobs], clock, reencode_flagged), calls

    (files, n, flagged), calls = run(jobs)
    assert files == ['kept a', 'sampled b', 'kept c', 'sampled d'] and (n, flagged) == (2, 0)
    assert calls == [('kept', ['a', 'c']), ('sampled', ['b', 'd'])]
    (files, n, flagged), calls = run(jobs, flag=('c',))
    assert (n, flagged) == (2, 1)
    if reencode_flagged:
        assert files == ['kept a', 'sampled b', 'sampled c', 'sampled d'] and calls == [('kept', ['a', 'c']), ('sampled', ['b', 'c', 'd'])]
    else:
        assert files == ['kept a', 'sampled b', None, 'sampled d'] and calls == [('kept', ['a', 'c']), ('sampled', ['b', 'd'])]
    # only copies that keep their blocks: a second call only for a flagged one that is encoded whole
    (files, n, flagged), calls = run(jobs[0::2], flag=('a',))
    assert (files, n, flagged) == ((['sampled a', 'kept c'], 2, 1) if reencode_flagged else ([None, 'kept c'], 1, 1))
    (files, n, flagged), calls = run(jobs[0::2])
    assert (files, n, flagged) == (['kept a', 'kept c'], 1, 0) and calls == [('kept', ['a', 'c'])]
    (files, n, flagged), calls = run(jobs[1::2])
    assert (files, n, flagged) == (['sampled b', 'sampled d'], 1, 0) and calls == [('sampled', ['b', 'd'])]
    assert run([]) == (([], 0, 0), [])


# ---- pool_map ---------------------------------------------------------------------------------------------------------------------

def test_pool_map_keeps_the_order_of_the_items():
    assert DR.pool_map(abs, [-3, 2, -1, 0], 2, True) == [3, 2, 1, 0]
    assert DR.pool_map(abs, [-3, 2], None, True) == [3, 2] and DR.pool_map(abs, [], 3, True) == []


# ---- device_decode.plan_source ----------------------------------------------------------------------------------------------------

def test_plan_source_raises_each_message_for_its_condition(tmp_path, monkeypatch):
    from PIL import Image
    rng = np.random.default_rng(5)
    image = Image.fromarray(rng.integers(0, 255, (8, 16, 3), dtype=np.uint8))
    baseline, png, progressive, gone = (str(tmp_path / n) for n in ('base.jpg', 'image.png', 'prog.jpg', 'gone.jpg'))
    image.save(baseline)
    image.save(png)
    image.save(progressive, progressive=True)
    probed = []
    real = DD.probe
    monkeypatch.setattr(DD, 'probe', lambda path, keep_data=False: probed.append(path) or real(path, keep_data))

    def message(*args, **kw):
        with pytest.raises(PV.HostLeg) as e:
            DD.plan_source(*args, **kw)
        return str(e.value)

    p, size = DD.plan_source(baseline, 'out/copy.JPG')
    assert p['size'] == size == (16, 8) and p['scan'] is not None and 'data' not in p
    p, size = DD.plan_source(baseline, 'copy.jpeg', 40, keep_data=True)
    assert size == (40, 20) and p['size'] == (16, 8) and p['data'] == open(baseline, 'rb').read()
    assert DD.plan_source(baseline, 'copy.jpg', 16)[1] == DD.plan_source(baseline, 'copy.jpg', -1)[1] == (16, 8)
    assert message(png, 'copy.jpg') == message(progressive, 'copy.jpg') == 'a file the device does not decode'
    assert message(png, 'copy.png') == 'a file the device does not decode'             # (the file is looked at before the name)
    assert message(baseline, 'copy.png') == message(baseline, 'copy') == 'not a JPEG name'
    assert message(baseline, 'copy.jpg', 65536) == message(baseline, 'copy.jpg', 131072) == 'a side above 65535 pixels'
    assert DD.plan_source(baseline, 'copy.jpg', 65535)[1] == (65535, 32767)
    assert message(gone, 'copy.jpg') == 'a file that does not open: PIL raises what the reference raises'
    with pytest.raises(AssertionError, match='^Invalid image resize target 0,0$'):
        DD.plan_source(baseline, 'copy.jpg', 0)
    # a dict of probes: every file is probed once, whatever it gave
    del probed[:]
    probes = {}
    for _ in range(2):
        assert DD.plan_source(baseline, 'copy.jpg', 40, probes=probes)[1] == (40, 20)
        assert message(png, 'copy.jpg', probes=probes) == 'a file the device does not decode'
        assert message(gone, 'copy.jpg', probes=probes) == 'a file that does not open: PIL raises what the reference raises'
    assert probed == [baseline, png, gone] and set(probes) == {baseline, png, gone}
    assert probes[png]['scan'] is None and isinstance(probes[gone], Exception)


# ---- stacked_labels ---------------------------------------------------------------------------------------------------------------

def _label_box_before(font, s, left, top, bottom, im_height):
    """preview.label_box as it was before stacked_labels took its place: draw_bounding_box_on_image :1052-1131 for ONE label"""
    total_height = (1 + 2 * 0.05) * PV.text_size(font, s)[1]
    padded = ' ' + s + ' '
    text_width, text_height = PV.text_size(font, padded)
    margin = int(np.ceil(0.05 * text_height))
    text_bottom = top
    if (text_bottom - total_height) < 0:
        text_bottom = bottom + total_height
        if text_bottom > im_height:
            text_bottom = top + total_height
    text_bottom = int(text_bottom)
    text_left = int(left)
    return padded, margin, (text_left, (text_bottom - text_height) - (2 * margin), text_left + text_width, text_bottom)


@pytest.mark.parametrize('where,top,bottom', [('above', 120.0, 180.5), ('below', 3.0, 100.25), ('inside', 2.5, 239.0)])
def test_stacked_labels_of_one_string_is_the_single_label(where, top, bottom):
    font = PV.load_font(PV.DEFAULT_LABEL_FONT, PV.DEFAULT_LABEL_FONT_SIZE)
    im_height, left, s = 240, 17.75, 'animal: 87%'
    want = _label_box_before(font, s, left, top, bottom, im_height)
    padded, margin, (x0, y0, x1, y1) = want
    assert {'above': y1 == int(top), 'below': y1 > int(bottom), 'inside': int(top) < y1 < int(bottom)}[where]
    lines = list(PV.stacked_labels(font, [s], left, top, bottom, im_height))
    assert lines == [(padded, margin, (x0, y0), (x1, y1), (x0 + margin, y0 + margin))]
    assert PV.label_box(font, s, left, top, bottom, im_height) == want
    assert list(PV.stacked_labels(font, [''], left, top, bottom, im_height)) == []
