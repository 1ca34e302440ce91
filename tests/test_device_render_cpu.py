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


# ---- the chunk body: plan_each, decode_front, render_jobs ----------------------------------------------------------------------------

def test_plan_each_sends_what_raises_to_the_host_leg_in_order():
    def plan(item):
        if item % 3 == 0:
            raise PV.HostLeg('a file the device does not decode') if item else ZeroDivisionError()
        return {'item': item}

    assert DR.plan_each(range(8), plan) == ([{'item': k} for k in (1, 2, 4, 5, 7)], [0, 3, 6])
    assert DR.plan_each([], plan) == ([], [])
    with pytest.raises(KeyboardInterrupt):                                 # (not an Exception: not the host leg's)
        DR.plan_each([1], lambda item: (_ for _ in ()).throw(KeyboardInterrupt()))


def test_job_bytes_counts_the_resized_pixels_only_where_the_size_changes():
    assert DR.job_bytes({'source_size': (12, 8), 'size': (12, 8)}) == 12 * 8 * 3
    assert DR.job_bytes({'source_size': (12, 8), 'size': (6, 4)}) == 12 * 8 * 3 + 6 * 4 * 3


class _Chunk:
    """One chunk on stand-ins: decode_stage refuses `refused` and gives every other file one _Tensor, under clock('decode');
    draw_plans, draw_plans_from and blur_rects record instead of calling the device; `log` holds every call in its order."""

    def __init__(self, monkeypatch, refused=(), profile=True):
        self.torch, self.ctx, self.log, self.ms = _DeviceTorch(), _Context(), [], ({} if profile else None)
        self.clock = DR.Clock(_Torch(), 'cuda:1', self.ms)
        self.counts = {k: 0 for k in ('gpu', 'files_decoded_gpu', 'files_decoded_pil', 'resample_calls', 'draw_calls', 'encode_calls')}
        self.pixels = {}
        self.ctx.resample_lanczos = lambda *args: self.log.append(('resample', list(args[0]), list(args[4])))

        def decode_stage(ctx, torch, device, image_base, files, probes, counts, clock, keep_coefficients=False):
            assert ctx is self.ctx and torch is self.torch and device == 'cuda:1' and counts is self.counts
            assert list(probes) == list(files) and all(probes[f] == 'probe of ' + f for f in files)
            self.log.append(('decode', image_base, list(files), keep_coefficients))
            with clock('decode'):
                for k, f in enumerate(f for f in files if f not in refused):
                    self.pixels[f] = _Tensor(0, 0x10 * (k + 1))
            counts['files_decoded_gpu'] += len(self.pixels)
            return dict(self.pixels), set(refused), ({f: (7, None) for f in self.pixels} if keep_coefficients else None)

        def draw_plans(ctx, ptrs, sizes, plans, device, stream=0, clock=None):
            if not any(p.ops for p in plans):
                return False
            with clock('draw'):
                self.log.append(('draw', list(ptrs), list(sizes)))
            return True

        def draw_plans_from(ctx, src_ptrs, sizes, dst_ptrs, dst_src, plans, device, stream=0, clock=None):
            with clock('draw'):
                self.log.append(('draw', list(dst_ptrs), [sizes[k] for k in dst_src]))
            return True

        def blur_rects(ctx, ptrs, sizes, rects_per_image, radius, stream=0):
            self.log.append(('blur', list(ptrs), [list(r) for r in rects_per_image]))
            return True

        monkeypatch.setattr(DD, 'decode_stage', decode_stage)
        monkeypatch.setattr(DR, 'draw_plans', draw_plans)
        monkeypatch.setattr(DR, 'draw_plans_from', draw_plans_from)
        monkeypatch.setattr(DR, 'blur_rects', blur_rects)

    def args(self):
        return self.ctx, self.torch, 'cuda:1'

    def encode(self, tensors, jobs):
        with self.clock('encode'):
            self.log.append(('encode', [t.data_ptr() for t in tensors], [j['name'] for j in jobs]))
        return ['file of ' + j['name'] for j in jobs], 1

    def write(self, job, data):
        self.log.append(('write', job['name'], data))

    def kinds(self):
        return [entry[0] for entry in self.log]


def _job(name, file, source_size=(12, 8), size=None, ops=True, **more):
    plan = _plan([('rect', 1, 2, 3, 4, 0x0000FF)]) if ops else PV.RenderPlan()
    return dict({'name': name, 'file': file, 'probe': 'probe of ' + file, 'source_size': source_size, 'size': size or source_size,
                 'plan': plan}, **more)


def test_decode_front_decodes_each_distinct_file_once_and_gives_the_jobs_of_a_refused_file_to_the_host(monkeypatch):
    """one file refused, two jobs on one file (compare_batch_results): the file is decoded once, its jobs share the tensor, and
    all jobs of the refused file come back for the host leg, in their order"""
    chunk = _Chunk(monkeypatch, refused={'b.jpg'})
    jobs = [_job('a1', 'a.jpg'), _job('b1', 'b.jpg'), _job('c1', 'c.jpg'), _job('a2', 'a.jpg'), _job('b2', 'b.jpg')]
    taken, tensors, host, coefficients = DR.decode_front(*chunk.args(), jobs, 'base', chunk.counts, chunk.clock)
    assert chunk.log == [('decode', 'base', ['a.jpg', 'b.jpg', 'c.jpg'], False)] and coefficients is None
    assert [j['name'] for j in taken] == ['a1', 'c1', 'a2'] and [j['name'] for j in host] == ['b1', 'b2']
    assert all(t is j for t, j in zip(taken + host, [jobs[0], jobs[2], jobs[3], jobs[1], jobs[4]]))
    assert tensors[0] is tensors[2] is chunk.pixels['a.jpg'] and tensors[1] is chunk.pixels['c.jpg']
    assert set(chunk.ms) == {'decode'} and chunk.counts['files_decoded_gpu'] == 2
    # the sources' planes are asked for, and handed on, only on request (separate_detections with keep_source_blocks)
    chunk = _Chunk(monkeypatch)
    taken, _, host, coefficients = DR.decode_front(*chunk.args(), jobs[:1], '', chunk.counts, chunk.clock, True)
    assert chunk.log == [('decode', '', ['a.jpg'], True)] and coefficients == {'a.jpg': (7, None)} and host == []


def test_render_jobs_resamples_draws_encodes_and_only_then_writes(monkeypatch):
    """sizes that change for some jobs and not for others: ONE resample call, the source tensors reused where the size stays;
    ONE draw call on the images at their final sizes; ONE encoder call; every file written after it, in the jobs' order"""
    chunk = _Chunk(monkeypatch)
    jobs = [_job('a', 'a.jpg', (12, 8), (6, 4)), _job('b', 'b.jpg', (5, 7)), _job('c', 'c.jpg', (9, 9), (18, 18), ops=False), _job('d', 'd.jpg')]
    jobs, tensors, host, _ = DR.decode_front(*chunk.args(), jobs, '', chunk.counts, chunk.clock)
    DR.render_jobs(*chunk.args(), jobs, tensors, chunk.counts, chunk.clock, chunk.encode, chunk.write)
    a, b, c, d = (t.data_ptr() for t in tensors)
    new_a, new_c = (t.data_ptr() for t in chunk.torch.made)
    assert [t.n for t in chunk.torch.made] == [6 * 4 * 3, 18 * 18 * 3] and host == []
    assert chunk.log[1:] == [('resample', [a, c], [(6, 4), (18, 18)]),
                             ('draw', [new_a, b, new_c, d], [(6, 4), (5, 7), (18, 18), (12, 8)]),
                             ('encode', [new_a, b, new_c, d], ['a', 'b', 'c', 'd']),
                             ('write', 'a', 'file of a'), ('write', 'b', 'file of b'), ('write', 'c', 'file of c'), ('write', 'd', 'file of d')]
    assert chunk.counts == {'gpu': 4, 'files_decoded_gpu': 4, 'files_decoded_pil': 0, 'resample_calls': 1, 'draw_calls': 1, 'encode_calls': 1}
    assert set(chunk.ms) == {'decode', 'resample', 'draw', 'encode'}       # postprocess_batch_results, visualize_db


def test_render_jobs_makes_no_draw_call_for_plans_without_operations(monkeypatch):
    chunk = _Chunk(monkeypatch)
    jobs = [_job('a', 'a.jpg', ops=False), _job('b', 'b.jpg', ops=False)]
    jobs, tensors, _, _ = DR.decode_front(*chunk.args(), jobs, '', chunk.counts, chunk.clock)
    DR.render_jobs(*chunk.args(), jobs, tensors, chunk.counts, chunk.clock, chunk.encode, chunk.write)
    assert chunk.kinds() == ['decode', 'encode', 'write', 'write'] and chunk.torch.made == []
    assert chunk.counts['draw_calls'] == 0 and chunk.counts['resample_calls'] == 0 and chunk.counts['encode_calls'] == 1
    assert set(chunk.ms) == {'decode', 'encode'}
    # and none at all, whatever the plans hold, for a tool that does not draw (the resize tools)
    chunk = _Chunk(monkeypatch)
    jobs = [_job('a', 'a.jpg', (12, 8), (6, 4))]
    del jobs[0]['plan']
    jobs, tensors, _, _ = DR.decode_front(*chunk.args(), jobs, '', chunk.counts, chunk.clock)
    DR.render_jobs(*chunk.args(), jobs, tensors, chunk.counts, chunk.clock, chunk.encode, chunk.write, draw=False)
    assert chunk.kinds() == ['decode', 'resample', 'encode', 'write'] and set(chunk.ms) == {'decode', 'resample', 'encode'}


def test_render_jobs_needs_every_counter_it_moves(monkeypatch):
    """a counter the tool's counts lack is an error, not a silent miss (separate_detections, which counts neither resample nor
    draw calls, does not go through render_jobs)"""
    for missing in ('resample_calls', 'draw_calls', 'encode_calls', 'gpu'):
        chunk = _Chunk(monkeypatch)
        del chunk.counts[missing]
        jobs, tensors, _, _ = DR.decode_front(*chunk.args(), [_job('a', 'a.jpg', (12, 8), (6, 4))], '', chunk.counts, chunk.clock)
        with pytest.raises(KeyError, match=missing):
            DR.render_jobs(*chunk.args(), jobs, tensors, chunk.counts, chunk.clock, chunk.encode, chunk.write)


def _tool_chunks(monkeypatch, tmp_path, chunk):
    """the chunk bodies of the five tools on the stand-ins of `chunk`, each writing below tmp_path: name -> (run(jobs) -> what
    the body returns for the host leg, the jobs of a chunk over a.jpg, b.jpg and c.jpg)"""
    from types import SimpleNamespace
    from megadetector_amd import compare_batch_results as C
    from megadetector_amd import crops
    from megadetector_amd import postprocess_batch_results as PB
    from megadetector_amd import resize_images as R
    from megadetector_amd import separate_detections as SD
    from megadetector_amd import visualize_db as VD

    def encode_windows(ctx, ptrs, pitches, rects, quality, stream=0, comments=None):
        chunk.log.append(('encode', list(ptrs), quality))
        return [b'window %d' % k for k in range(len(ptrs))]

    def encode_copies(ctx, device, tensors, jobs, source_ptrs, clock, reencode_flagged, stream=0):
        with clock('encode_kept'):
            chunk.log.append(('encode', [t.data_ptr() for t in tensors], source_ptrs))
        return [b'copy'] * len(jobs), 1, 1

    def encode_sampled(ctx, device, tensors, jobs, stream=0):
        chunk.log.append(('encode', [t.data_ptr() for t in tensors], 'sampled'))
        return [b'sampled'] * len(jobs)

    def decode_scans(ctx, torch, device, scans, keep_coefficients=False):
        chunk.log.append(('decode', list(scans)))
        return [None if s == 'scan of b.jpg' else _Tensor(0, 0x10 * (k + 1)) for k, s in enumerate(scans)], [None] * len(scans)

    monkeypatch.setattr(crops, 'encode_windows', encode_windows)
    monkeypatch.setattr(DR, 'encode_copies', encode_copies)
    monkeypatch.setattr(DR, 'encode_sampled', encode_sampled)
    monkeypatch.setattr(DD, 'decode_scans', decode_scans)
    out = str(tmp_path)
    os.makedirs(os.path.join(out, 'rendered_images'))
    os.makedirs(os.path.join(out, 'detections'))
    chunk.counts.update(kept=0, kept_refused=0)
    files = ('a.jpg', 'b.jpg', 'c.jpg')
    path = lambda tool, f: os.path.join(out, tool + '_' + f)
    plain = lambda tool, **more: [_job(f[0], f, (12, 8), (6, 4) if f == 'c.jpg' else None, **dict({k: v(f) for k, v in more.items()})) for f in files]
    options = SimpleNamespace(image_base_dir='base', output_dir=out, base_input_folder='base', image_folder='base')
    args, done = chunk.args() + (None, chunk.clock), []
    return {
        'postprocess': (lambda jobs: PB._render_chunk_device(*args[:3], jobs, chunk.clock, options, chunk.counts),
                        plain('postprocess', decision=lambda f: {'category_string': 'detections', 'file': f}, sample_name=lambda f: 'detections_' + f)),
        'visualize_db': (lambda jobs: VD._render_chunk_device(*args[:3], jobs, chunk.clock, out, chunk.counts),
                         plain('visualize_db', info=lambda f: {'output_file_name': 'visualize_db_' + f}, quality=lambda f: 75, comment=lambda f: None)),
        'separate': (lambda jobs: SD._render_chunk_device(*args[:3], jobs, chunk.clock, options, chunk.counts),
                     [dict(j, size=j['source_size']) for j in plain('separate', target=lambda f: path('separate', f), rects=lambda f: [(0, 0, 2, 2)],
                                                                   keep=lambda f: f == 'a.jpg')]),
        'compare': (lambda jobs: C._render_chunk_device(*args[:3], C.group_by_file(jobs), chunk.clock, options, chunk.counts),
                    plain('compare', output_path=lambda f: path('compare', f)) + [_job('a2', 'a.jpg', ops=False, output_path=path('compare', 'a2.jpg'))]),
        'resize': (lambda jobs: R.render_chunk(*args[:3], jobs, chunk.clock, lambda j: dict(j, probe={'scan': 'scan of ' + j['file']}), chunk.counts,
                                               done.append),
                   plain('resize', output=lambda f: path('resize', f))),
    }


CLOCK_KEYS = {'postprocess': {'decode', 'resample', 'draw', 'encode'}, 'visualize_db': {'decode', 'resample', 'draw', 'encode'},
              'compare': {'decode', 'resample', 'draw', 'encode'}, 'separate': {'decode', 'blur', 'draw', 'encode_kept'},
              'resize': {'decode', 'resample', 'encode'}}


@pytest.mark.parametrize('tool', sorted(CLOCK_KEYS))
def test_the_tools_chunk_bodies_refuse_one_file_and_render_the_rest(monkeypatch, tmp_path, tool):
    """b.jpg is refused by the decoder: its jobs come back for the host leg, a.jpg and c.jpg (which is resized, except by
    separate_detections) are rendered in ONE call of each kind under the clock keys the tool has always had, and their files
    are on disk only after the encoder call"""
    chunk = _Chunk(monkeypatch, refused={'b.jpg'})
    run, jobs = _tool_chunks(monkeypatch, tmp_path, chunk)[tool]
    if tool == 'separate':                                                # (it keeps neither counter)
        del chunk.counts['resample_calls'], chunk.counts['draw_calls']
    written = lambda: sorted(n for _, _, names in os.walk(str(tmp_path)) for n in names)
    real = chunk.log.append
    seen = []
    chunk.log = type('Log', (list,), {'append': lambda self, entry: (seen.append((entry[0], written())), real(entry), list.append(self, entry))})()
    host = run(jobs)
    b = [j for j in jobs if j['file'] == 'b.jpg']
    # what the host leg gets is what the tool's run_chunks orders and its host leg renders: the decision, the entry, else the job
    assert len(host) == len(b) == 1
    if tool in ('postprocess', 'visualize_db'):
        assert host[0] is b[0]['decision' if tool == 'postprocess' else 'info']
    elif tool == 'resize':                                                # (its plan stand-in returns a copy of the job)
        assert host[0]['name'] == 'b' and host[0]['output'] == b[0]['output']
    else:
        assert host[0] is b[0]
    kinds = [k for k, _ in seen]
    assert kinds == {'separate': ['decode', 'blur', 'draw', 'encode'], 'resize': ['decode', 'resample', 'encode']}.get(
        tool, ['decode', 'resample', 'draw', 'encode'])
    assert all(files == [] for _, files in seen)                           # nothing is written before the last device call returned
    n = 3 if tool == 'compare' else 2
    assert len(written()) == n and chunk.counts['gpu'] == n and chunk.counts['encode_calls'] == 1
    assert chunk.counts.get('resample_calls') == (None if tool == 'separate' else 1)
    assert chunk.counts.get('draw_calls') == {'separate': None, 'resize': 0}.get(tool, 1)
    assert set(chunk.ms) == CLOCK_KEYS[tool]
    if tool == 'separate':
        assert (chunk.counts['kept'], chunk.counts['kept_refused']) == (0, 1)          # one copy keeps, and the stand-in flags one
        assert [e for e in chunk.log if e[0] == 'decode'][0][3] is True and chunk.log[-1][2] == [7, None]
    if tool == 'compare':                                                 # a.jpg decoded once; its job without operations is the shared image
        assert [e for e in chunk.log if e[0] == 'decode'][0][2] == ['a.jpg', 'b.jpg', 'c.jpg']
        a, c = chunk.pixels['a.jpg'].data_ptr(), chunk.pixels['c.jpg'].data_ptr()
        assert [e for e in chunk.log if e[0] == 'resample'] == [('resample', [c], [(6, 4)])]
        ptrs = chunk.log[-1][1]                                           # the jobs by file: a, a2, c
        assert ptrs[1] == a and a not in (ptrs[0], ptrs[2]) and c not in ptrs


def test_visualize_db_gives_the_entry_of_a_refused_file_to_the_host_leg_in_its_place(monkeypatch, tmp_path):
    """the whole device leg (_render_device, run_chunks with the tool's order) around a file the decoder refuses: the entries
    come back -- not the jobs, which the order does not know -- in the order of to_render, after the entry that was not planned"""
    from megadetector_amd import crops
    from megadetector_amd import visualize_db as VD
    chunk = _Chunk(monkeypatch, refused={'b.jpg'})
    monkeypatch.setattr(crops, 'encode_windows', lambda ctx, ptrs, *args, **kw: [b'window'] * len(ptrs))
    os.makedirs(str(tmp_path / 'rendered_images'))
    infos = [{'img_path': f, 'output_file_name': f} for f in ('x.png', 'a.jpg', 'b.jpg', 'c.jpg')]

    def plan_job(info, options, label_map, thin_outlines):
        if info['img_path'] == 'x.png':
            raise PV.HostLeg('a file the device does not decode')
        return _job(info['img_path'][0], info['img_path'], info=info, quality=75, comment=None)

    monkeypatch.setattr(VD, 'plan_job', plan_job)
    monkeypatch.setitem(__import__('sys').modules, 'torch', chunk.torch)   # (_render_device imports it for run_chunks)
    chunk.counts['decode_chunks'] = 0
    host = VD._render_device(list(reversed(infos)), str(tmp_path), None, None, chunk.ctx, chunk.counts, False, True)
    assert len(host) == 2 and host[0] is infos[2] and host[1] is infos[0]
    assert sorted(os.listdir(str(tmp_path / 'rendered_images'))) == ['a.jpg', 'c.jpg'] and chunk.counts['gpu'] == 2


@pytest.mark.parametrize('tool', sorted(CLOCK_KEYS))
def test_the_tools_chunk_bodies_stop_after_the_decode_when_every_file_is_refused(monkeypatch, tmp_path, tool):
    chunk = _Chunk(monkeypatch, refused={'a.jpg', 'b.jpg', 'c.jpg'})
    run, jobs = _tool_chunks(monkeypatch, tmp_path, chunk)[tool]
    if tool == 'resize':                                                  # (its decoder stand-in flags b.jpg only)
        jobs = [j for j in jobs if j['file'] == 'b.jpg']
    before = dict(chunk.counts)
    host = run(jobs)
    assert len(host) == len(jobs) and chunk.kinds() == ['decode'] and chunk.torch.made == []
    assert chunk.counts == before and chunk.counts['gpu'] == 0
    assert [n for _, _, names in os.walk(str(tmp_path)) for n in names] == []


def test_encode_windows_writes_a_window_with_a_comment_through_sampled_file(monkeypatch):
    """visualize_db: Pillow carries a source's COM segment into the file it saves, so such a window is written by sampled_file
    with the quality's standard tables at 4:2:0 (sampling 2) around the same scan; every other window by jfif_file"""
    from types import SimpleNamespace
    from megadetector_amd import crops
    scans = [bytes([k]) * (k + 3) for k in range(3)]
    calls = []

    def read_encoded(call, capacity, device, what):
        assert what == 'mdhip_jpeg_encode' and device == 'cuda:1'
        blob = b''.join(scans)
        offs = [0, len(scans[0]), len(scans[0]) + len(scans[1])]
        return np.frombuffer(blob, np.uint8), offs, [len(s) for s in scans], []

    monkeypatch.setattr(DR, 'read_encoded', read_encoded)
    for name in ('sampled_file', 'jfif_file'):
        real = getattr(J, name)
        monkeypatch.setattr(J, name, lambda *args, name=name, real=real: calls.append((name, args)) or real(*args))
    ctx = SimpleNamespace(device=1)
    rects, comments = [(0, 0, 16, 8), (2, 1, 10, 9), (0, 0, 24, 16)], [None, b'a comment', b'']
    files = crops.encode_windows(ctx, [0x100, 0x200, 0x300], [48, 48, 72], rects, 60, comments=comments)
    ql, qc = J.quant_tables(60)
    assert [name for name, _ in calls] == ['jfif_file', 'sampled_file', 'jfif_file']
    assert calls[0][1] == (16, 8, 60, scans[0]) and calls[2][1] == (24, 16, 60, scans[2])
    w, h, got_ql, got_qc, sampling, scan, exif, comment = calls[1][1]
    assert (w, h, sampling, scan, exif, comment) == (8, 8, 2, scans[1], b'', b'a comment')
    assert np.array_equal(got_ql, ql) and np.array_equal(got_qc, qc)
    assert files == [J.jfif_file(16, 8, 60, scans[0]), J.sampled_file(8, 8, ql, qc, 2, scans[1], b'', b'a comment'), J.jfif_file(24, 16, 60, scans[2])]
    assert b'a comment' in files[1] and files[1] != J.jfif_file(8, 8, 60, scans[1])
    # without comments: as it always was
    del calls[:]
    assert crops.encode_windows(ctx, [0x100, 0x200, 0x300], [48, 48, 72], rects, 60) == [J.jfif_file(w, h, 60, s) for (w, h), s in
                                                                                         zip([(16, 8), (8, 8), (24, 16)], scans)]
    assert [name for name, _ in calls] == ['jfif_file'] * 6


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
