"""
Records what the host side of the hot path DOES, mode by mode, and writes it to tests/golden/batch_driver_traces.json:
tests/test_batch_driver_cpu.py records the same traces and compares.  The fixture was written by this script on the commit
before the batch driver was folded into one loop, so it pins that every mode kept its calls, their order and their text.

A trace of load_and_run_detector_batch holds
  events    in the order they happened in the consumer thread:
              ['call', method, [file names], [type of every image], {keyword: value}]    every detector call
              ['on_results', n, [file names]]                                            every results.extend of the driver
              ['checkpoint', n]                                                          write_checkpoint with n results
              ['release', slot]                                                          SharedImageRing.release
  printed   the lines the run printed in this process, the folder taken out of them; sorted in the modes whose producer
            threads print (their place among the consumer's lines is a race)
  results   per result: file, failure, number of detections, width, height, datetime
  feed      last_feed_counts (the ring modes)
and of run_detector_on_frames: the calls, ['take', [file names]] for every renderer.take, and the exception that left it.

No GPU, no reference: a stub detector.  Run:  python tests/golden/gen_batch_driver_traces.py
"""

import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from megadetector_amd import feed, process_video  # noqa: E402
from megadetector_amd import run_detector_batch as RDB  # noqa: E402
from stub_detector import StubDetector  # noqa: E402

FIXTURE = os.path.join(HERE, 'batch_driver_traces.json')

# seven files: five readable images of three sizes, an unreadable file in the middle, a readable one the detector fails on
FILES = [('a0.png', 40), ('a1.png', 43), ('a2.png', 46), ('a3_broken.png', None), ('a4.png', 40), ('a5_fails.png', 43),
         ('a6.png', 46)]
WIDTH = 64
ARRAY_SLOT_BYTES = 45 * WIDTH * 3           # ring_slot_bytes of the 'array' case: the 46-row images do not fit a slot


def write_files(folder):
    from PIL import Image
    names = []
    for i, (name, h) in enumerate(FILES):
        p = os.path.join(folder, name)
        if h is None:
            with open(p, 'wb') as f:
                f.write(b'not an image')
        else:
            rng = np.random.default_rng(500 + i)
            exif = Image.Exif()
            if i % 2 == 0:
                exif[306] = '2024:05:0{} 10:11:12'.format(i + 1)          # DateTime: the timestamp of every other image
            Image.fromarray(rng.integers(0, 256, (h, WIDTH, 3), dtype=np.uint8)).save(p, exif=exif)
        names.append(p)
    return names


def _plain(v):
    return v if isinstance(v, (bool, int, float, str, type(None))) else '<{}>'.format(type(v).__name__)


class RecordingStub(StubDetector):
    """StubDetector that writes every call into `events` and, unlike it, also fails the per-image call on a fail_on file"""

    def __init__(self, events, fail_on=()):
        super().__init__(fail_on=set(fail_on))
        self.events = events

    def record(self, method, imgs, names, kw):
        self.events.append(['call', method, [os.path.basename(n) for n in names], [type(i).__name__ for i in imgs],
                            {k: _plain(kw[k]) for k in sorted(kw)}])

    def generate_detections_one_batch(self, imgs, names, **kw):
        self.record('generate_detections_one_batch', imgs, names, kw)
        kw.pop('render', None)
        return super().generate_detections_one_batch(imgs, names, **kw)

    def generate_detections_one_image(self, img, name='unknown', **kw):
        self.record('generate_detections_one_image', [img], [name], kw)
        kw.pop('render', None)
        if name in self.fail_on:
            raise RuntimeError('simulated device failure')
        return super().generate_detections_one_image(img, name, **kw)


class RecordingTicketStub(RecordingStub):
    """with the start_batch / finish_batch pair; a fail_on file fails the batch in finish_batch, or (fail_in_start) in
    start_batch"""

    def __init__(self, events, fail_on=(), fail_in_start=False):
        super().__init__(events, fail_on)
        self.fail_in_start = fail_in_start
        self.outstanding = self.max_outstanding = 0

    def start_batch(self, imgs, names, **kw):
        self.record('start_batch', imgs, names, kw)
        if self.fail_in_start and any(n in self.fail_on for n in names):
            raise RuntimeError('simulated device failure')
        self.outstanding += 1
        self.max_outstanding = max(self.max_outstanding, self.outstanding)
        return {'imgs': imgs, 'names': names}

    def finish_batch(self, ticket):
        self.record('finish_batch', ticket['imgs'], ticket['names'], {})
        self.outstanding -= 1
        return StubDetector.generate_detections_one_batch(self, ticket['imgs'], ticket['names'])


class RecordingResults(list):
    """passed as results=: the driver hands every group of results on with one extend"""

    def __init__(self, events):
        super().__init__()
        self.events = events

    def extend(self, new):
        new = list(new)
        self.events.append(['on_results', len(new), [os.path.basename(r['file']) for r in new]])
        super().extend(new)


@contextlib.contextmanager
def patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


THREADS = dict(use_image_queue=True, use_threads_for_queue=True, loader_workers=1)
RING = dict(use_image_queue=True, use_threads_for_queue=False, loader_workers=1)

#: case -> (keywords of load_and_run_detector_batch, ticket stub?, what is patched, are the printed lines sorted)
BATCH_CASES = {
    'inline_b1': (dict(batch_size=1), False, None, False),
    'inline_b3': (dict(batch_size=3), False, None, False),
    'threads_b1': (dict(batch_size=1, **THREADS), False, None, True),
    'threads_b3': (dict(batch_size=3, **THREADS), False, None, True),
    'threads_b3_tickets': (dict(batch_size=3, **THREADS), True, None, True),
    'threads_b3_preprocess': (dict(batch_size=3, preprocess_on_image_queue=True, **THREADS), False, None, True),
    'ring_b1': (dict(batch_size=1, **RING), False, None, False),
    'ring_b3_tickets': (dict(batch_size=3, **RING), True, None, False),
    'ring_b3_tickets_start_fails': (dict(batch_size=3, **RING), 'start', None, False),
    'ring_b3_array': (dict(batch_size=3, **RING), False, 'small_slots', False),
    'ring_fallback': (dict(batch_size=3, **RING), False, 'no_shared_memory', True),
}


def record_batch_case(case, folder):
    """-> (the trace, the slots that were handed out and not released exactly once: must be empty)"""
    kw, tickets, patch, sort_printed = BATCH_CASES[case]
    names = write_files(folder)
    fail_on = [n for n in names if n.endswith('_fails.png')]
    events = []
    det = RecordingTicketStub(events, fail_on, fail_in_start=(tickets == 'start')) if tickets else RecordingStub(events, fail_on)
    outstanding, slot_errors = set(), []

    real_checkpoint, real_release, real_iter = RDB.write_checkpoint, feed.SharedImageRing.release, feed.ProcessLoader.__iter__

    def write_checkpoint(path, results):
        events.append(['checkpoint', len(results)])
        real_checkpoint(path, results)

    def release(ring, slot):
        events.append(['release', slot])
        if slot in outstanding:
            outstanding.remove(slot)
        else:
            slot_errors.append(('released but not held', slot))
        real_release(ring, slot)

    def iterate(loader):
        for item in real_iter(loader):
            if item[0] in ('slot', 'jpeg', 'scan'):
                if item[2] in outstanding:
                    slot_errors.append(('handed out while held', item[2]))
                outstanding.add(item[2])
            yield item

    def no_shared_memory(*a, **k):
        raise OSError(28, 'No space left on device')

    out = io.StringIO()
    with contextlib.ExitStack() as stack:
        stack.enter_context(patched(RDB, 'write_checkpoint', write_checkpoint))
        stack.enter_context(patched(feed.SharedImageRing, 'release', release))
        stack.enter_context(patched(feed.ProcessLoader, '__iter__', iterate))
        if patch == 'small_slots':
            stack.enter_context(patched(RDB, 'ring_slot_bytes', ARRAY_SLOT_BYTES))
        if patch == 'no_shared_memory':
            stack.enter_context(patched(feed, 'ProcessLoader', no_shared_memory))
        stack.enter_context(patched(RDB, 'last_feed_counts', {}))
        stack.enter_context(contextlib.redirect_stdout(out))
        results = RDB.load_and_run_detector_batch(
            'stub', names, detector=det, results=RecordingResults(events), confidence_threshold=0.4, image_size=640,
            include_image_size=True, include_image_timestamp=True, checkpoint_frequency=2,
            checkpoint_path=os.path.join(folder, 'checkpoint.json'), **kw)
        feed_counts = dict(RDB.last_feed_counts)
    printed = [ln.replace(folder + os.sep, '') for ln in out.getvalue().splitlines()]
    trace = {'events': events, 'printed': sorted(printed) if sort_printed else printed,
             'results': [[os.path.basename(r['file']), r.get('failure'),
                          None if r.get('detections') is None else len(r['detections']),
                          r.get('width'), r.get('height'), r.get('datetime', 'absent')] for r in results]}
    if kw.get('use_threads_for_queue') is False and patch != 'no_shared_memory':
        trace['feed'] = feed_counts
    if tickets:
        trace['max_outstanding'] = det.max_outstanding
    slot_errors += [('never released', s) for s in sorted(outstanding)]
    return json.loads(json.dumps(trace)), slot_errors


class RecordingRenderer:
    """what run_detector_on_frames needs of visualize_video_output.InPassRenderer"""

    on_device = True

    def __init__(self, events):
        self.events = events

    def take(self, results):
        self.events.append(['take', [r['file'] for r in results]])


#: case -> (batch size, ticket stub?, the frame whose batch fails)
VIDEO_CASES = {
    'video_b1': (1, False, None),
    'video_b3': (3, False, None),
    'video_b3_tickets': (3, True, None),
    'video_b3_tickets_second_finish_raises': (3, True, 'frame000006.jpg'),
}


def record_video_case(case):
    batch_size, tickets, failing = VIDEO_CASES[case]
    rng = np.random.default_rng(77)
    frames = [rng.integers(0, 256, (32, 48, 3), dtype=np.uint8) for _ in range(7)]
    events = []
    det = (RecordingTicketStub if tickets else RecordingStub)(events, [failing] if failing else [])
    trace = {'events': events, 'raised': None}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        try:
            r = process_video.run_detector_on_frames(det, process_video.ArrayFrameSource(frames), every_n_frames=2,
                                                     batch_size=batch_size, detection_threshold=0.4, image_size=640,
                                                     renderer=RecordingRenderer(events))
            trace['results'] = [[x['file'], len(x['detections'])] for x in r['results']]
            trace['frame_filenames'] = r['frame_filenames']
        except Exception as e:
            trace['raised'] = '{}: {}'.format(type(e).__name__, e)
    trace['printed'] = out.getvalue().splitlines()
    if tickets:
        trace['max_outstanding'] = det.max_outstanding
    return json.loads(json.dumps(trace))


def record_all():
    traces = {}
    for case in BATCH_CASES:
        with tempfile.TemporaryDirectory() as folder:
            traces[case], slot_errors = record_batch_case(case, folder)
        assert not slot_errors, (case, slot_errors)
    for case in VIDEO_CASES:
        traces[case] = record_video_case(case)
    return traces


def dump(traces):
    return json.dumps(traces, indent=0, sort_keys=True) + '\n'


if __name__ == '__main__':
    text = dump(record_all())
    with open(FIXTURE, 'w') as f:
        f.write(text)
    print('wrote {} ({} bytes, {} cases)'.format(FIXTURE, len(text), len(BATCH_CASES) + len(VIDEO_CASES)))
