"""
Batch driver: the image loop of the reference (megadetector/detection/run_detector_batch.py) on
top of the HIP detector, emitting the same MegaDetector JSON.

Mirrored entry points (same names, argument meaning and failure conventions):
  load_and_run_detector_batch   reference :1062-1439
  write_checkpoint / load_checkpoint   reference :1465 / :1497
  write_results_to_file         reference :1546-1662
  main (CLI)                    reference :1763-2186 (the options that touch this path)
The reference's loop bodies -- per image (:937-1056: threshold, image_size and augment forwarded :988-994), batched (:680-831:
none of them forwarded, the threshold applied afterwards :766) and the queue consumer (:203-455) -- are one loop here: a feed per way images arrive (_inline_feed, _thread_feed, _ring_feed) delivers groups
of loaded images and load failures, _BatchDriver does everything else with a group, and DetectorWindow holds every detector
call, for this file and for process_video.
New here (spec = reference notebooks/manage_local_batch.py:496-964):
  run_sharded                   one spawned worker process per GPU, balanced `i % G` sharding of the
                                image list, host-side merge with duplicate/missing checks -- no
                                collectives; output identical to the 1-GPU result.

Loader workers are threads (`use_threads_for_queue=True`, reference :1814) or *spawned* processes that
decode into a page-locked shared-memory ring (`use_threads_for_queue=False`; feed.py, SURVEY.md 8(f)
N1) -- never forked processes: a forked child of a process that has touched HIP is undefined behaviour
(the reference forks before loading the model, run_detector_batch.py:545-557).  In both queue modes the
batches go through the detector's pipelined start_batch / finish_batch when it has them (the GPU works
on batch i while the host formats batch i-1 and assembles batch i+1); results are identical to the
plain loop.
"""

import argparse
import contextlib
import copy
import json
import os
import queue
import shutil
import sys
import threading
import time
from datetime import datetime
from functools import partial

import numpy as np

from . import feed, placement, run_detector
from .feed import load_image, EXIF_IMAGE_ROTATIONS          # noqa: F401  (re-exported)
from .constants import FAILURE_IMAGE_OPEN, FAILURE_INFER, DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD
from .constants import DEFAULT_DETECTOR_LABEL_MAP
from . import classify as classify_mod
from . import crops as crops_mod
from . import blur as blur_mod
from . import preview as preview_mod
from .jpeg_host import ScanFailure
from .ref_utils import write_json as _write_json

# reference run_detector_batch.py:86-119
default_loaders = 4
default_preprocess_on_image_queue = False
max_queue_size = 10
current_format_version = '1.6'
verbose = False

image_extensions = ('.jpg', '.jpeg', '.gif', '.png')           # reference ct_utils.py:30


# --------------------------------------------------------------------------------------------
# host I/O helpers
# --------------------------------------------------------------------------------------------
def is_image_file(s):
    return os.path.splitext(s)[1].lower() in image_extensions


def find_images(dirname, recursive=False):
    """reference path_utils.py:525 (sorted list of image files)"""
    found = []
    if recursive:
        for root, _, files in os.walk(dirname):
            found += [os.path.join(root, f) for f in files if is_image_file(f)]
    else:
        found = [os.path.join(dirname, f) for f in os.listdir(dirname) if is_image_file(f)]
    return sorted(found)


def parse_kvp_list(items, kv_separator='='):
    """reference ct_utils.py:921: ['a=b','c=d'] (or 'a=b,c=d') -> {'a':'b','c':'d'}"""
    if items is None:
        return {}
    if isinstance(items, str):
        items = [s for s in items.split(',') if s]
    d = {}
    for item in items:
        if kv_separator not in item:
            raise ValueError('Illegal key-value pair: {}'.format(item))
        k, v = item.split(kv_separator, 1)
        d[k.strip()] = v.strip()
    return d


write_json = partial(_write_json, force_str=True)               # reference ct_utils.py:210-251 with force_str=True


def _sort_by_key(items, key, reverse=False):
    """reference ct_utils.py:509 (None sorts as smallest)"""
    return sorted(items, key=lambda d: (d[key] is not None, d[key]), reverse=reverse)


# --------------------------------------------------------------------------------------------
# per-batch / per-image processing
# --------------------------------------------------------------------------------------------
def _group_into_batches(items, batch_size):
    """reference :657"""
    if batch_size <= 0:
        raise ValueError('Batch size must be positive')
    return [items[i:i + batch_size] for i in range(0, len(items), batch_size)]


def _add_image_metadata(result, image, include_image_size, include_image_timestamp):
    if isinstance(image, dict):
        image = image['img_original_pil']
    if image is None:
        return
    if include_image_size:
        result['width'] = image.width
        result['height'] = image.height
    if include_image_timestamp:
        dt = None
        try:
            exif = image.getexif()
            dt = exif.get(36867) or exif.get(306)       # DateTimeOriginal / DateTime
        except Exception:
            pass
        result['datetime'] = dt


def _filter_batch_output(dets, names, images, confidence_threshold, include_image_size, include_image_timestamp):
    """reference :760-792: the batched detector call gets no threshold; it is applied to its output"""
    assert len(dets) == len(names)
    out = []
    for i, r in enumerate(dets):
        assert names[i] == r['file']
        if 'failure' not in r:
            r['detections'] = [d for d in r['detections'] if d['conf'] >= confidence_threshold]
            if include_image_size or include_image_timestamp:
                _add_image_metadata(r, images[i], include_image_size, include_image_timestamp)
        else:
            print('Warning: within-batch processing failure for image {}'.format(r['file']))
        out.append(r)
    return out


# --------------------------------------------------------------------------------------------
# written products, made while the images are at hand: detection crops (reference postprocessing/create_crop_folder.py),
# blurred copies (postprocessing/separate_detections_into_folders.py --category_names_to_blur) and annotated previews
# (visualization/visualize_detector_output.py)
# --------------------------------------------------------------------------------------------
#: crops of the most recent run in this process: 'files' written, of them 'gpu' = JPEG names encoded by the detector on
#: the device, 'host_jpeg' = JPEG names saved by PIL here (a detector without crops=), 'host_other' = other extensions,
#: saved by PIL as the reference does; 'skipped' = rectangles without area
last_crop_counts = {}

#: blurred copies of the most recent run in this process: 'files' written, of them 'gpu' = made by the detector from the
#: image in device memory (blur=), 'host' = blurred and saved here (a detector without blur=)
last_blur_counts = {}

#: previews of the most recent run in this process: 'files' written, of them 'gpu' = made by the detector from the image in
#: device memory (preview=), 'host' = rendered or saved by PIL (a detector without preview=, pixels that never were in device
#: memory, an extension that is not JPEG, drawing the plan does not restate); 'skipped' = images without a file (failed,
#: below the threshold with detections_only, a resize target that is not positive, drawing that raises)
last_preview_counts = {}

#: classifications of the most recent run in this process (--classifier): {image file: [(detection index, [[class id,
#: conf], ...])]}, the index counting the detections as the results file holds them; and the crops counted: 'gpu' = by a
#: detector with classify= (its own classify_counts tell its kernel and its host leg apart), 'host' = made by PIL here (a
#: detector without classify=), 'skipped' = detections without a crop
last_classifications = {}
last_classify_counts = {}
last_detector = None        # the detector of the last load_and_run_detector_batch of this process (--rde_review_folder works on its context)


def _relative_name(file, base):
    """the name an image's products are derived from: relative to the image folder (a lone file: its base name)"""
    if os.path.isabs(file):
        file = os.path.relpath(file, start=base) if base else os.path.basename(file)
    return file.replace('\\', '/')


class _Writer:
    """writes an image's product below the product's folder BEFORE its result is handed on, so that a result a checkpoint
    holds has its files on disk and a resumed run leaves no gaps.  A detector that has the product's keyword makes it and
    the result carries it; for any other detector the host leg makes it here.  The per-product part: `keyword`, `count_keys`
    and files(result, relative name, pixels) -> [(name below the folder, bytes, the count it adds to)]."""

    def __init__(self, folder, options, base):
        self.folder, self.options, self.base = folder, options, base
        # (a category name the label map does not hold ends the run here)
        self.category_ids = options.category_ids() if hasattr(options, 'category_ids') else None
        self.counts = dict.fromkeys(('files',) + self.count_keys, 0)

    def detector_kw(self, detector):
        return {self.keyword: self.options} if getattr(detector, 'supports_' + self.keyword, False) else {}

    @staticmethod
    def _pixels(image, file):
        if isinstance(image, dict):
            image = image.get('img_original')
        a = None if image is None or hasattr(image, 'coef') or hasattr(image, 'desc') else np.asarray(image)
        if a is None or a.ndim != 3 or a.dtype != np.uint8:
            a = np.asarray(load_image(file))                 # the reference's second pass: the file once more
        return a

    def write(self, results, images):
        for i, r in enumerate(results):
            pixels = lambda: self._pixels(images[i] if images else None, r['file'])
            for name, data, kind in self.files(r, _relative_name(r['file'], self.base), pixels):
                crops_mod.write_file(self.folder, name, data)
                self.counts['files'] += 1
                self.counts[kind] += 1


class _CropWriter(_Writer):
    """<crop folder>/<crop_filename of the relative path>, one file for every detection that is cropped"""

    keyword, count_keys = 'crops', ('gpu', 'host_jpeg', 'host_other', 'skipped')

    def files(self, r, rel, pixels):
        crops, jpeg_kind = r.pop('crops', None), 'gpu'
        if r.get('detections') is None:
            return []
        if crops is None:                                    # a detector without crops=: PIL on the host, as the reference
            jpeg_kind = 'host_jpeg'
            if crops_mod.select_crops(crops_mod.output_order(r['detections'], self.options.output_threshold), self.options, self.category_ids):
                crops, skipped = crops_mod.crops_of_host_image(pixels(), r['file'], r['detections'], self.options, self.category_ids)
                self.counts['skipped'] += skipped
        named = [(crops_mod.crop_filename(rel, cid), data) for cid, _, data in crops or []]
        return [(name, data, jpeg_kind if crops_mod.is_jpeg_name(name) else 'host_other') for name, data in named]


class _BlurWriter(_Writer):
    """<blur folder>/<relative path>, for an image that has something to blur; no other image is written"""

    keyword, count_keys = 'blur', ('gpu', 'host')

    def files(self, r, rel, pixels):
        from_detector = 'blurred' in r
        data = r.pop('blurred', None)
        if r.get('detections') is None:
            return []
        if not from_detector and blur_mod.select_detections(r['detections'], self.options, self.category_ids):
            # a detector without blur=, or pixels that never were in device memory: the host leg
            data = blur_mod.blurred_file_of_host_image(pixels(), rel, r['detections'], self.options, self.category_ids)
        return [] if data is None else [(rel, data, 'gpu' if from_detector else 'host')]


class _PreviewWriter(_Writer):
    """<preview folder>/anno_<name> (or <relative path>); an image without a file counts as 'skipped'"""

    keyword, count_keys = 'preview', ('gpu', 'host', 'skipped')

    def files(self, r, rel, pixels):
        data, leg = r.pop('preview', (None, None))
        if leg is None and preview_mod.is_rendered(r, self.options):
            # a detector without preview=: the host leg
            data, leg = preview_mod.preview_file_of_host_image(pixels(), rel, r['detections'], self.options), 'host'
        if data is None:
            self.counts['skipped'] += 1
            return []
        return [(preview_mod.output_name(rel, self.options), data, leg)]


class _ClassifyWriter(_Writer):
    """no folder and no files: takes an image's classifications off its result, so that the results and the checkpoints are
    what they are without the classifier, and keeps them for the classified results file"""

    keyword, count_keys = 'classify', ('gpu', 'host', 'skipped')

    def __init__(self, options):
        super().__init__(None, options, None)
        self.collected = {}

    def files(self, r, rel, pixels):
        from_detector = 'classifications' in r
        value = r.pop('classifications', None)
        if r.get('detections') is None:
            return []
        if from_detector:
            self.counts['gpu'] += len(value)
        elif crops_mod.select_crops(crops_mod.output_order(r['detections'], self.options.output_threshold), self.options, self.category_ids):
            # a detector without classify=: the host leg
            value, skipped = classify_mod.classifications_of_host_image(pixels(), r['file'], r['detections'], self.options, self.category_ids)
            self.counts['host'] += len(value)
            self.counts['skipped'] += skipped
        if value:
            self.collected[r['file']] = value
        return []


def write_classified_results(final_output, classifications, options, path, relative_path_base=None):
    """the results with 'classifications' on every classified detection, 'classification_categories' and the classifier in
    'info' (merge_classification_detection_output.py:307-335), as a copy: the results themselves are not changed"""
    def name(f):
        if relative_path_base is not None:
            f = os.path.relpath(f, start=relative_path_base)
        return f.replace('\\', '/')
    classified = copy.deepcopy(final_output)
    classify_mod.annotate_results(classified, {name(f): v for f, v in classifications.items()}, options,
                                  datetime.now().strftime('%Y-%m-%d %H:%M:%S'))
    write_json(path, classified)
    print('Classified results saved at {}'.format(path))
    return classified


def _detector_kw(writers, detector):
    """the product keywords this detector takes; a duck-typed detector without the flag never receives the keyword"""
    kw = {}
    for w in writers:
        kw.update(w.detector_kw(detector))
    return kw


def _write_products(writers, results, images):
    """outside the callers' try blocks: a folder that cannot be written ends the run, it is no inference failure"""
    for w in writers:
        w.write(results, images)


def _crop_options(confidence_threshold, expansion, quality, categories, output_threshold=None):
    """crops.CropOptions from the crop arguments of load_and_run_detector_batch and of the command line; categories: a list of
    names, or a string of names separated by commas or blanks"""
    if isinstance(categories, str):
        categories = [v for v in categories.replace(',', ' ').split() if v]
    return crops_mod.CropOptions(confidence_threshold=confidence_threshold, expansion=expansion, quality=quality,
                                 category_names_to_include=categories or None, output_threshold=output_threshold)


def write_crop_result_files(final_output, options, base, crop_results_file=None, crops_output_file=None):
    """the two files create_crop_folder writes next to the crops: the results with 'crop_id' and 'crop_filename_relative'
    added (its output_file), and one entry per crop (its crops_output_file, create_crop_folder.py:485-521)"""
    annotated = copy.deepcopy(final_output)
    records = crops_mod.annotate_results(annotated['images'], options, options.category_ids(),
                                         name_of=lambda f: _relative_name(f, base))
    if crop_results_file is not None:
        write_json(crop_results_file, annotated)
    if crops_output_file is not None:
        per_crop = dict(annotated)
        per_crop['images'] = records
        write_json(crops_output_file, per_crop)


class DetectorWindow:
    """
    Every call of the detector, for this driver and for process_video.run_detector_on_frames: which entry point a batch
    goes through, and the window of batches in flight.
      batch size 1                          generate_detections_one_image with image_kw
      pipelined, a detector with the pair   start_batch with batch_kw at once; finish_batch of its ticket when a second ticket
                                            is outstanding, oldest first, and at drain(): the GPU works on one batch while
                                            the host formats the one before it and assembles the next
      otherwise                             generate_detections_one_batch with batch_kw
    deliver(context, results, error, entry) gets what every call returned, `entry` naming the call.  The caller says what an
    exception means: one of the classes in `catch` is delivered as `error` with no results -- from start_batch at once, ahead of
    the ticket in flight -- and any other leaves submit() or drain().
    """

    def __init__(self, detector, batch_size, pipelined, image_kw, batch_kw, deliver, catch=()):
        self.det, self.image_kw, self.batch_kw, self.deliver, self.catch = detector, image_kw, batch_kw, deliver, catch
        if batch_size == 1:
            self.entry = 'one_image'
        elif pipelined and hasattr(detector, 'start_batch') and hasattr(detector, 'finish_batch'):
            self.entry = 'start_batch'
        else:
            self.entry = 'one_batch'
        self.inflight = []

    def _awaited(self, entry, context, call):
        results = error = None
        try:
            results = call()
        except self.catch as e:
            error = e
        self.deliver(context, results, error, entry)

    def submit(self, images, names, context=None):
        if self.entry == 'one_image':
            self._awaited('one_image', context,
                          lambda: [self.det.generate_detections_one_image(images[0], names[0], **self.image_kw)])
        elif self.entry == 'one_batch':
            self._awaited('one_batch', context, lambda: self.det.generate_detections_one_batch(images, names, **self.batch_kw))
        else:
            try:
                ticket = self.det.start_batch(images, names, **self.batch_kw)
            except self.catch as e:
                self.deliver(context, None, e, 'start_batch')
                return
            self.inflight.append((ticket, context, images))         # (the pixels stay alive until finish_batch has read them)
            while len(self.inflight) >= 2:
                self._finish_oldest()

    def _finish_oldest(self):
        ticket, context, _ = self.inflight.pop(0)
        self._awaited('finish_batch', context, lambda: self.det.finish_batch(ticket))

    def drain(self):
        while self.inflight:
            self._finish_oldest()


class _BatchDriver:
    """
    The loop body, once, for every feed.  A group is (items, failures): an item is (file, image, meta, release) -- meta the
    object its size and timestamp are read from (None: the image), release (or None) frees what holds the pixels -- and a
    failure a finished {'file', 'failure'} record.  A group's images go to the detector through one DetectorWindow; an
    exception becomes FAILURE_INFER records; the batched call gets no threshold, it is applied to its output (reference
    :751-767), the per-image call gets threshold, image_size and augment (:988-994); then metadata, the written products, the
    releases -- after the call that read the pixels has returned, also when it raised -- and on_results, the group's failures
    in front.  fed: the queue modes, whose batches go through the ticket pair.
    """

    def __init__(self, detector, batch_size, fed, confidence_threshold, quiet, image_size, include_image_size,
                 include_image_timestamp, augment, writers, on_results):
        self.batch_size, self.thr, self.quiet = batch_size, confidence_threshold, quiet
        self.inc_size, self.inc_time = include_image_size, include_image_timestamp
        self.writers, self.on_results = writers, on_results
        products = _detector_kw(writers, detector)
        self.window = DetectorWindow(
            detector, batch_size, fed,
            dict(detection_threshold=confidence_threshold, image_size=image_size, augment=augment, verbose=verbose, **products),
            dict(verbose=verbose, **products), self._deliver, catch=Exception)
        self.drain = self.window.drain

    def submit(self, group):
        items, failures = group
        if not items:
            self.on_results(failures)
            return
        if self.batch_size == 1 and not self.quiet:
            print('Processing image {}'.format(items[0][0]))
        self.window.submit([it[1] for it in items], [it[0] for it in items], group)

    def _deliver(self, group, results, error, entry):
        items, failures = group
        names, images = [it[0] for it in items], [it[1] for it in items]
        metas = [it[1] if it[2] is None else it[2] for it in items]
        if error is None and entry == 'one_image':
            if results[0].get('failure') is None:
                _add_image_metadata(results[0], metas[0], self.inc_size, self.inc_time)
        elif error is None:
            try:
                results = _filter_batch_output(results, names, metas, self.thr, self.inc_size, self.inc_time)
            except Exception as e:
                error = e
        if error is not None:
            if entry != 'one_image':
                print('Batch processing failure for {} images: {}'.format(len(names), str(error)))
            elif not self.quiet:
                print('Image {} cannot be processed: {}'.format(names[0], str(error)))
            results = [{'file': n, 'failure': FAILURE_INFER} for n in names]
        if error is None or entry in ('one_batch', 'finish_batch'):
            # (outside the try blocks: a folder that cannot be written ends the run, it is no inference failure)
            _write_products(self.writers, results, images)
        for it in items:
            if it[3] is not None:
                it[3]()
        self.on_results(failures + results)


def _inline_feed(image_files, batch_size, quiet):
    """the files grouped before they are loaded (reference :1297): a file that cannot be loaded takes its place in its group"""
    for group in _group_into_batches(image_files, batch_size):
        items, failures = [], []
        for im_file in group:
            try:
                items.append((im_file, load_image(im_file), None, None))
            except Exception as e:
                if batch_size == 1 and not quiet:           # (the per-image path announces a file before it loads it)
                    print('Processing image {}'.format(im_file))
                if batch_size > 1 or not quiet:
                    print('Image {} cannot be loaded: {}'.format(im_file, str(e)))
                failures.append({'file': im_file, 'failure': FAILURE_IMAGE_OPEN})
        yield items, failures


def _accumulate(arrivals, batch_size, groups_of=None):
    """the fed modes: valid items up to the batch size; a failure record travels as a group of its own the moment it arrives.
    groups_of(items): the groups a full batch becomes (default: itself)"""
    groups_of = groups_of or (lambda items: [(items, [])])
    pending = []
    for arrival in arrivals:
        if isinstance(arrival, dict):
            yield [], [arrival]
            continue
        pending.append(arrival)
        if len(pending) >= batch_size:
            yield from groups_of(pending)
            pending = []
    if pending:
        yield from groups_of(pending)


# --------------------------------------------------------------------------------------------
# checkpoints (reference :1465-1520)
# --------------------------------------------------------------------------------------------
def write_checkpoint(checkpoint_path, results):
    assert checkpoint_path is not None
    tmp = None
    if os.path.isfile(checkpoint_path):
        tmp = checkpoint_path + '_tmp'
        shutil.copyfile(checkpoint_path, tmp)
    write_json(checkpoint_path, {'checkpoint': results})
    if tmp is not None:
        try:
            os.remove(tmp)
        except Exception as e:
            print('Warning: error removing backup checkpoint file {}:\n{}'.format(tmp, str(e)))


def load_checkpoint(checkpoint_path):
    print('Loading previous results from checkpoint file {}'.format(checkpoint_path))
    with open(checkpoint_path, 'r') as f:
        data = json.load(f)
    if 'checkpoint' not in data:
        raise ValueError('Checkpoint file {} is missing "checkpoint" field'.format(checkpoint_path))
    print('Restored {} entries from the checkpoint {}'.format(len(data['checkpoint']), checkpoint_path))
    return data['checkpoint']


# --------------------------------------------------------------------------------------------
# image queue (threads) -- reference :124-200 producers, :203-455 consumer, :461-650 driver
# --------------------------------------------------------------------------------------------
def _producer(q, file_q, preprocessor, image_size, producer_id):
    while True:
        try:
            im_file = file_q.get_nowait()
        except queue.Empty:
            break
        try:
            image = load_image(im_file)
            if preprocessor is not None:
                image = preprocessor.preprocess_image(image, image_id=im_file, image_size=image_size)
        except Exception as e:
            print('Producer process: image {} cannot be loaded:\n{}'.format(im_file, str(e)))
            image = FAILURE_IMAGE_OPEN
        q.put((im_file, image, producer_id))
    q.put(None)


def _make_preprocessor(detector, detector_options):
    """A weight-free, HIP-free twin of `detector` for the producer side: same options, same geometry attributes."""
    from .detector import HIPDetector
    opts = copy.deepcopy(dict(detector_options or {}))
    if getattr(detector, 'compatibility_mode', None) is not None:
        opts['compatibility_mode'] = detector.compatibility_mode
    opts['preprocess_only'] = True
    pre = HIPDetector('synthetic', opts)
    for attr in ('default_image_size', 'letterbox_stride', 'compatibility_mode'):
        if hasattr(detector, attr):
            setattr(pre, attr, getattr(detector, attr))
    return pre


def _thread_feed(image_files, detector, image_size, loader_workers, batch_size, preprocess_on_image_queue=False,
                 detector_options=None):
    q = queue.Queue(max_queue_size)
    file_q = queue.Queue()
    for f in image_files:
        file_q.put(f)
    preprocessor = None
    if preprocess_on_image_queue:
        # reference _producer_func (:143-152): load_detector(..., deepcopy(detector_options) + preprocess_only), so the
        # producers letterbox in the consumer's compatibility mode
        preprocessor = _make_preprocessor(detector, detector_options)
    n_workers = max(1, min(loader_workers, len(image_files)))
    threads = [threading.Thread(target=_producer, args=(q, file_q, preprocessor, image_size, i), daemon=True)
               for i in range(n_workers)]
    for t in threads:
        t.start()

    def arrivals():
        finished = 0
        while finished < n_workers:
            item = q.get()
            if item is None:
                finished += 1
            elif isinstance(item[1], str):
                yield {'file': item[0], 'failure': item[1]}
            else:
                yield item[0], item[1], None, None

    yield from _accumulate(arrivals(), batch_size)
    for t in threads:
        t.join()


# the shared-memory ring: slot size (bytes) and slots per image of the batch size
ring_slot_bytes = 48 * 1024 * 1024              # a 16-megapixel RGB frame; larger images travel through the queue
ring_slots_per_batch_image = 3                  # one batch being filled, two in flight


#: how the files of the most recent shared-ring run reached the detector: 'jpeg' = as DCT coefficients (gpu_jpeg), 'slot' /
#: 'array' = as PIL pixels, 'fail' = could not be opened; with gpu_jpeg='entropy' also 'scan' = as the compressed scan
last_feed_counts = {}


@contextlib.contextmanager
def _ring_feed(image_files, detector, image_size, want_meta, loader_workers, batch_size, gpu_jpeg=False):
    """
    SURVEY.md 8(f) N1 (feed.py): spawned loader processes decode into a page-locked shared-memory ring.  A context: the
    groups inside it, the ring open until the last batch in flight has been finished and its slots released.
    gpu_jpeg: the loaders only entropy-decode baseline JPEGs and the detector rebuilds their pixels on the GPU
    (feed.py decode='coefficients'); needs a detector that takes coefficient images (HIPDetector).
    gpu_jpeg='entropy': the loaders only parse the headers and the GPU Huffman-decodes too (feed.py decode='scan',
    HIPDetector.decode_scans); a file the GPU flags is decoded with PIL in this process from the bytes it holds.
    """
    global last_feed_counts
    last_feed_counts = {'jpeg': 0, 'slot': 0, 'array': 0, 'fail': 0}
    if gpu_jpeg and not hasattr(detector, 'jpeg_images_reconstructed'):
        print('Warning: gpu_jpeg is ignored: this detector does not take JPEG coefficients')
        gpu_jpeg = False
    if gpu_jpeg == 'entropy' and not hasattr(detector, 'decode_scans'):
        print('Warning: gpu_jpeg="entropy" is ignored: this detector does not take JPEG scans')
        gpu_jpeg = False
    entropy = gpu_jpeg == 'entropy'
    if entropy:
        last_feed_counts['scan'] = 0
    n_workers = max(1, min(loader_workers, len(image_files)))
    n_slots = ring_slots_per_batch_image * batch_size + n_workers
    try:
        loader = feed.ProcessLoader(image_files, n_workers, n_slots, ring_slot_bytes, want_meta=want_meta,
                                    decode='scan' if entropy else 'coefficients' if gpu_jpeg else 'pixels')
    except (OSError, MemoryError) as e:
        # e.g. a container whose /dev/shm is smaller than the ring: the thread queue needs no shared memory
        print('Warning: cannot create the shared-memory ring ({} slots of {} MB: {}); using loader threads'.format(
            n_slots, ring_slot_bytes >> 20, str(e)))
        loader = None
    if loader is None:
        yield _thread_feed(image_files, detector, image_size, loader_workers, batch_size)
        return
    ring = loader.ring
    in_slot = {'slot': ring.view, 'jpeg': partial(feed.coefficient_image, ring), 'scan': partial(feed.scan_image, ring)}

    def arrivals():
        for kind, im_file, payload, shape, meta in loader:
            last_feed_counts[kind] = last_feed_counts.get(kind, 0) + 1
            meta_img = feed.ImageMeta(meta) if meta is not None else None
            if kind == 'fail':
                yield {'file': im_file, 'failure': FAILURE_IMAGE_OPEN}
            elif kind in in_slot:
                yield im_file, in_slot[kind](payload, shape), meta_img, partial(ring.release, payload)
            else:
                yield im_file, payload, meta_img, None

    def decoded(pending):
        """gpu_jpeg='entropy': the batch's scans become device coefficient images, or what PIL makes of a flagged file --
        pixels, or the failure the loader would have reported, which goes ahead of the batch"""
        kept = []
        for (f, _, meta_img, release), im in zip(pending, detector.decode_scans([it[1] for it in pending])):
            if isinstance(im, ScanFailure):
                print('Image {} cannot be loaded:\n{}'.format(f, str(im.error)))
                if release is not None:
                    release()
                yield [], [{'file': f, 'failure': FAILURE_IMAGE_OPEN}]
            elif isinstance(im, np.ndarray) and release is not None:
                release()                                # PIL's pixels are an array of this process: the slot is free
                kept.append((f, im, meta_img, None))
            else:
                kept.append((f, im, meta_img, release))
        if kept:
            yield kept, []

    try:
        if hasattr(detector, 'start_batch'):
            ring.pin()
        yield _accumulate(arrivals(), batch_size, decoded if entropy else None)
    finally:
        loader.close()


# --------------------------------------------------------------------------------------------
# main entry point
# --------------------------------------------------------------------------------------------
def _resolve_image_list(image_file_names):
    """reference :1150-1190: list | single image | folder | .json / .txt list file"""
    if isinstance(image_file_names, str):
        s = image_file_names
        if os.path.isdir(s):
            return find_images(s, recursive=True)
        if is_image_file(s):
            return [s]
        if s.lower().endswith('.json'):
            with open(s, 'r') as f:
                return list(json.load(f))
        if s.lower().endswith('.txt'):
            with open(s, 'r') as f:
                return [ln.strip() for ln in f if ln.strip()]
        raise ValueError('Illegal image_file_names value {}'.format(s))
    return list(image_file_names)


def load_and_run_detector_batch(model_file, image_file_names, checkpoint_path=None,
                                confidence_threshold=DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD,
                                checkpoint_frequency=-1, results=None, n_cores=1, use_image_queue=False,
                                quiet=False, image_size=None, class_mapping_filename=None,
                                include_image_size=False, include_image_timestamp=False,
                                include_exif_tags=None, augment=False, force_model_download=False,
                                detector_options=None, loader_workers=default_loaders,
                                preprocess_on_image_queue=default_preprocess_on_image_queue, batch_size=1,
                                verbose_output=False, use_threads_for_queue=True, detector=None, gpu_jpeg=False,
                                crop_folder=None, crop_confidence_threshold=0.1, crop_expansion=0, crop_quality=95,
                                crop_categories=None, crop_base=None,
                                blur_folder=None, blur_categories=('person',), blur_confidence_threshold=None, blur_radius=40,
                                blur_quality=85, blur_base=None,
                                preview_folder=None, preview_width=1000, preview_confidence_threshold=0.15,
                                preview_detections_only=False, preview_preserve_paths=False, preview_box_thickness=4,
                                preview_box_expansion=0, preview_label_font_size=16, preview_label_font='arial.ttf',
                                preview_blur_categories=None, preview_quality=75, preview_base=None, classify_options=None):
    """
    reference :1062-1439.  `detector` (extra, optional) injects an already constructed detector
    object -- used by run_sharded and by the CPU tests of the loop with a stub detector.
    `gpu_jpeg` (extra, default off): in the shared-ring mode (use_image_queue with loader processes) baseline JPEGs travel
    as DCT coefficients and are rebuilt on the GPU, bit for bit what PIL decodes; every other file, and every other mode,
    runs as without it.  gpu_jpeg='entropy' (--gpu_jpeg_entropy): they travel as their compressed scan and the GPU
    Huffman-decodes them too; a file the GPU flags is decoded with PIL here from its bytes.  Same results either way.
    `crop_folder` (extra, default None = off): every detection at or above crop_confidence_threshold (of the categories
    named in crop_categories, if any) is written below it as create_crop_folder.py names and cuts it, at crop_quality,
    crop_expansion pixels on every side; names are relative to crop_base (the image folder).  A detector with crops=
    (HIPDetector) encodes JPEG crops on the GPU from the resident image; other extensions, and other detectors, go through
    PIL here.  An image's crops are on disk before its result can reach a checkpoint.  The results are the same objects
    as without it.
    `blur_folder` (extra, default None = off): every image with a detection of blur_categories at or above
    blur_confidence_threshold (None: blur.DEFAULT_BLUR_CONFIDENCE_THRESHOLD, the reference script's default) is written to
    <blur_folder>/<path relative to blur_base> with those boxes blurred as visualization_utils.blur_detections blurs them
    (Gaussian, blur_radius) and saved at blur_quality; no other image is written.  A detector with blur= (HIPDetector)
    blurs and encodes a copy of the image on the GPU; other detectors, and pixels that are not in device memory, go
    through libmdjpeg.so and PIL here.  The results are the same objects as without it.
    `preview_folder` (extra, default None = off): every image is written to <preview_folder>/anno_<name> as
    visualization/visualize_detector_output.py writes it -- resized to preview_width with Pillow's LANCZOS filter, the boxes at
    or above preview_confidence_threshold drawn with their labels, people blurred first with preview_blur_categories -- the
    name relative to preview_base with slashes, backslashes and colons replaced by ~ (preview_preserve_paths: the relative path itself).  A detector
    with preview= (HIPDetector) does all of it on the GPU from the resident image; other detectors, and pixels that are not in
    device memory, go through PIL here.  The results are the same objects as without it.
    `classify_options` (extra, default None = off; a classify.ClassifyOptions): every detection at or above its confidence
    threshold is classified as classification/run_classifier.py classifies the reference's crop files.  A detector with
    classify= (HIPDetector) makes the classifier's input on the GPU from the resident image and runs the model there; other
    detectors go through PIL here.  The classifications are kept in last_classifications (write_classified_results writes
    them); the results, and the checkpoints, are what they are without it.
    Returns the list of per-image result dicts.
    """
    global verbose, last_crop_counts, last_blur_counts, last_preview_counts, last_classifications, last_classify_counts, last_detector
    verbose = bool(verbose_output)
    output_threshold = DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD if confidence_threshold is None else confidence_threshold
    writers = []
    if crop_folder is not None:
        writers.append(_CropWriter(crop_folder, _crop_options(crop_confidence_threshold, crop_expansion, crop_quality, crop_categories,
                                                              output_threshold), crop_base))
        last_crop_counts = writers[-1].counts         # (of the most recent call, for reporting; the writer itself is local)
    if blur_folder is not None:
        writers.append(_BlurWriter(blur_folder, blur_mod.BlurOptions(
            category_names=blur_categories,
            confidence_threshold=blur_mod.DEFAULT_BLUR_CONFIDENCE_THRESHOLD if blur_confidence_threshold is None else blur_confidence_threshold,
            radius=blur_radius, quality=blur_quality, output_threshold=output_threshold), blur_base))
        last_blur_counts = writers[-1].counts
    if preview_folder is not None:
        writers.append(_PreviewWriter(preview_folder, preview_mod.PreviewOptions(
            confidence_threshold=preview_confidence_threshold, output_image_width=preview_width,
            detections_only=preview_detections_only, preserve_path_structure=preview_preserve_paths,
            box_thickness=preview_box_thickness, box_expansion=preview_box_expansion, label_font_size=preview_label_font_size,
            label_font=preview_label_font, blur_categories=preview_blur_categories, quality=preview_quality,
            output_threshold=output_threshold), preview_base))
        last_preview_counts = writers[-1].counts
    if classify_options is not None:
        classify_options.output_threshold = output_threshold
        writers.append(_ClassifyWriter(classify_options))
        last_classifications, last_classify_counts = writers[-1].collected, writers[-1].counts
    if detector_options is None:
        detector_options = {}
    elif isinstance(detector_options, (list, str)):
        detector_options = parse_kvp_list(detector_options)
    else:
        detector_options = dict(detector_options)
    if class_mapping_filename is not None or include_exif_tags is not None:
        raise NotImplementedError('class_mapping_filename / include_exif_tags are not part of the HIP hot path')
    if n_cores is not None and n_cores > 1:
        print('Warning: n_cores is ignored when running on a GPU (reference :1204)')
    if confidence_threshold is None:
        confidence_threshold = DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD
    if checkpoint_frequency is None or checkpoint_path is None:
        checkpoint_frequency = -1
    if results is None:
        results = []
    already_processed = set(r['file'] for r in results)
    image_files = [f for f in _resolve_image_list(image_file_names) if f not in already_processed]
    batch_size = max(1, int(batch_size))
    if batch_size > 1:
        detector_options['batch_size'] = batch_size           # reference :1227-1228
    if image_size is not None and int(image_size) > int(detector_options.get('max_image_size', 1280) or 1280):
        # the device arena is planned at construction (default: the model's own size, 1280): a user-supplied size
        # above it (the reference accepts any, :988-994) must be known there, or every image would come back as an
        # inference failure
        detector_options['max_image_size'] = int(image_size)

    if detector is None:
        t0 = time.time()
        detector = run_detector.load_detector(model_file, force_model_download=force_model_download,
                                              detector_options=detector_options, verbose=verbose)
        print('Loaded model in {:.2f} seconds'.format(time.time() - t0))
    last_detector = detector
    # Building the per-image result dicts allocates tens of thousands of containers per batch; every full pass of
    # the cyclic collector they trigger walks the start-up heap (torch, numpy, the model).  Freezing that heap once
    # (the collector stays on) is worth ~7 % of the loop at MI355X speeds.
    import gc
    gc.collect()
    gc.freeze()

    # Checkpoint cadence, as the reference has it: the in-line loops write when the number of images handed to the
    # detector in THIS run is a multiple of the frequency (:1314, :1338 -- with batches, only when a batch boundary
    # lands on a multiple); the queue consumer writes whenever a multiple has been crossed (:272-288).
    counts = {'images': 0, 'last_checkpoint': 0}
    crossing_rule = bool(use_image_queue)

    def on_results(new_results):
        results.extend(new_results)
        counts['images'] += len(new_results)
        if checkpoint_path is None or checkpoint_frequency is None or checkpoint_frequency <= 0:
            return
        if crossing_rule:
            due = counts['images'] // checkpoint_frequency > counts['last_checkpoint'] // checkpoint_frequency
        else:
            due = counts['images'] % checkpoint_frequency == 0
        if due:
            print('Writing a new checkpoint after having processed {} images since last restart'.format(
                counts['images']))
            write_checkpoint(checkpoint_path, results)
            counts['last_checkpoint'] = counts['images']

    if gpu_jpeg and not (use_image_queue and not use_threads_for_queue):
        print('gpu_jpeg is ignored: it takes effect with --use_image_queue and loader processes only')
    if use_image_queue and not use_threads_for_queue and len(image_files) > 0:
        groups_in = _ring_feed(image_files, detector, image_size, include_image_size or include_image_timestamp, loader_workers,
                               batch_size, gpu_jpeg='entropy' if gpu_jpeg == 'entropy' else bool(gpu_jpeg))
    elif use_image_queue:
        groups_in = contextlib.nullcontext(_thread_feed(image_files, detector, image_size, loader_workers, batch_size,
                                                        preprocess_on_image_queue, detector_options))
    else:
        groups_in = contextlib.nullcontext(_inline_feed(image_files, batch_size, quiet))
    driver = _BatchDriver(detector, batch_size, bool(use_image_queue), confidence_threshold, quiet, image_size, include_image_size,
                          include_image_timestamp, augment, writers, on_results)
    with groups_in as groups:
        for group in groups:
            driver.submit(group)
            del group                   # (its images go before the feed loads the next group's)
        driver.drain()
    # a loader process that died mid-list, or a result dropped anywhere above, must not pass silently
    have = set(r['file'] for r in results)
    missing = [f for f in image_files if f not in have]
    if missing:
        raise RuntimeError('{} images have no result (first: {})'.format(len(missing), missing[0]))
    return results


def write_results_to_file(results, output_file, relative_path_base=None, detector_file=None, info=None,
                          include_max_conf=False, custom_metadata=None, force_forward_slashes=True):
    """reference :1546-1662: MegaDetector batch output format 1.6"""
    out = []
    for r in results:
        r = copy.copy(r)
        if relative_path_base is not None:
            r['file'] = os.path.relpath(r['file'], start=relative_path_base)
        if force_forward_slashes:
            r['file'] = r['file'].replace('\\', '/')
        if not include_max_conf:
            r.pop('max_detection_conf', None)
        out.append(r)
    if info is None:
        info = {'detection_completion_time': datetime.now().strftime('%Y-%m-%d %H:%M:%S'),
                'format_version': current_format_version}
        if detector_file is not None:
            name = os.path.basename(detector_file)
            info['detector'] = name
            info['detector_metadata'] = run_detector.get_detector_metadata_from_version_string(
                run_detector.get_detector_version_from_filename(name, verbose=True))
        else:
            info['detector'] = 'unknown'
            info['detector_metadata'] = run_detector.get_detector_metadata_from_version_string('unknown')
    elif detector_file is not None:
        print('Warning (write_results_to_file): info struct and detector file supplied, ignoring detector file')
    if custom_metadata is not None:
        info['custom_metadata'] = custom_metadata
    out = _sort_by_key(out, 'file')
    for im in out:
        if im.get('detections') is not None:
            im['detections'] = _sort_by_key(im['detections'], 'conf', reverse=True)
        if 'failure' in im:
            assert im.get('detections') is None, 'Illegal failure/detection combination'
            im['detections'] = None
    final_output = {'images': out, 'detection_categories': DEFAULT_DETECTOR_LABEL_MAP, 'info': info}
    write_json(output_file, final_output)
    print('Output file saved at {}'.format(output_file))
    return final_output


# --------------------------------------------------------------------------------------------
# multi-GPU: shard the image queue, one process per GPU, no collectives
# --------------------------------------------------------------------------------------------
def shard_image_list(image_files, n_shards):
    """balanced split (reference ct_utils.py:499-503 'balanced' strategy: shard i gets files i, i+n, ...)"""
    return [list(image_files[i::n_shards]) for i in range(n_shards)]


def merge_shard_results(shard_results, expected_files=None):
    """reference notebooks/manage_local_batch.py:930-964: concatenate, reject duplicates / omissions"""
    merged, seen = [], set()
    for res in shard_results:
        for r in res:
            if r['file'] in seen:
                raise ValueError('duplicate result for {}'.format(r['file']))
            seen.add(r['file'])
            merged.append(r)
    if expected_files is not None:
        missing = [f for f in expected_files if f not in seen]
        if missing:
            raise ValueError('{} images have no result (first: {})'.format(len(missing), missing[0]))
    return merged


def shard_checkpoint_path(checkpoint_path, gpu):
    """every shard process writes its own checkpoint file: G processes must not rewrite one file"""
    return None if checkpoint_path is None else '{}.shard{}'.format(checkpoint_path, gpu)


def _shard_worker(gpu, model_file, files, kwargs, out_q):
    try:
        n_gpus = kwargs.pop('_n_gpus', 1)
        # CPUs of this GPU's NUMA node, disjoint from the other shards'; the loader processes spawned below inherit
        # the mask and are sized to it (placement.py)
        cpus = placement.pin_worker(gpu, n_gpus)
        if cpus and kwargs.get('use_image_queue'):
            kwargs['loader_workers'] = placement.loader_workers_for(kwargs.get('loader_workers', default_loaders), len(cpus))
        opts = dict(kwargs.pop('detector_options', None) or {})
        opts['device'] = 'cuda:{}'.format(gpu)
        kwargs['checkpoint_path'] = shard_checkpoint_path(kwargs.get('checkpoint_path'), gpu)
        res = load_and_run_detector_batch(model_file, files, detector_options=opts, **kwargs)
        out_q.put((gpu, res, None))
    except Exception as e:        # the parent reports it; a dead shard must not hang the join
        out_q.put((gpu, None, repr(e)))


def run_spawned_shards(target, shard_args, n_shards):
    """
    One *spawned* process per shard (a forked child of a process that has touched HIP is undefined behaviour):
    `target(g, *shard_args[g], out_q)` posts (g, result, error-or-None) on out_q.  Returns [result of shard 0, ...];
    raises when a shard reports an error or dies without a result (its exit code is polled: a process killed by a
    signal -- HIP fault, OOM killer -- never posts).  Shared by the image path (run_sharded) and the video path
    (process_video.process_videos).
    """
    import multiprocessing as mp
    ctx = mp.get_context('spawn')
    out_q = ctx.Queue()
    procs = []
    for g in range(n_shards):
        p = ctx.Process(target=target, args=(g,) + tuple(shard_args[g]) + (out_q,))
        p.start()
        procs.append(p)
    got = {}
    try:
        while len(got) < n_shards:
            try:
                g, res, err = out_q.get(timeout=2.0)
            except queue.Empty:
                dead = [g for g, p in enumerate(procs) if g not in got and not p.is_alive()]
                if dead and out_q.empty():
                    time.sleep(0.5)                  # its last message may still be in the pipe
                    if out_q.empty():
                        raise RuntimeError('shard {} exited with code {} without a result'.format(
                            dead[0], procs[dead[0]].exitcode))
                continue
            if err is not None:
                raise RuntimeError('shard {} failed: {}'.format(g, err))
            got[g] = res
    except BaseException:
        for p in procs:
            if p.is_alive():
                p.terminate()
        raise
    for p in procs:
        p.join()
    return [got[g] for g in range(n_shards)]


def require_saved_fp8_scales_for_shards(detector_options):
    """A multi-GPU run (image shards here, video shards in process_video.py) in the fp8 mode must start from SAVED
    activation scales: with fp8_calibrate_on_first_batch every shard would calibrate its e4m3 scales on its own first
    batch (and race to write the same fp8_scales_file), so the same image would get different detections depending
    on n_gpus and the shard it lands in."""
    dopts = detector_options or {}
    if str(dopts.get('dtype', '')).lower() == 'fp8' and not dopts.get('fp8_scales') and not (
            dopts.get('fp8_scales_file') and os.path.isfile(dopts['fp8_scales_file'])):
        raise ValueError("dtype 'fp8' on several GPUs needs saved scales (detector_options fp8_scales or an existing "
                         "fp8_scales_file): calibrate once on one GPU first")


def run_sharded(model_file, image_file_names, n_gpus, results=None, worker=None, **kwargs):
    """
    Runs load_and_run_detector_batch on n_gpus GPUs of one node: the image list is split
    `i % n_gpus`, each shard runs in its own *spawned* process pinned to one GPU
    (detector_options['device'] = 'cuda:g', reference pytorch_detector.py:853-858) and to that GPU's share of the
    CPUs (placement.py), results are merged on the host.  There is no inter-GPU traffic.

    Checkpoints: shard g writes `<checkpoint_path>.shard<g>` (shard_checkpoint_path).  `results` (restored from a
    checkpoint, single-GPU or merged from shard files by load_sharded_checkpoints) are kept as they are; only the
    files without a result are sharded, so a resumed run recomputes nothing.
    `worker` replaces _shard_worker in the CPU tests.
    """
    files = _resolve_image_list(image_file_names)
    results = list(results) if results else []
    done = set(r['file'] for r in results)
    todo = [f for f in files if f not in done]
    if n_gpus <= 1:
        return load_and_run_detector_batch(model_file, files, results=results, **kwargs)
    dopts = kwargs.get('detector_options') or {}
    if isinstance(dopts, (list, str)):
        dopts = parse_kvp_list(dopts)
    require_saved_fp8_scales_for_shards(dopts)
    ck = kwargs.get('checkpoint_path')
    if ck is not None and results and (kwargs.get('checkpoint_frequency') or -1) > 0:
        # The shards only know their own new results, and their `<ck>.shard<g>` files are about to be overwritten by
        # this run's first checkpoints (a resumed run is split i % n again): keep everything restored so far in the
        # plain file, which load_sharded_checkpoints unions with the shard files -- a second crash loses nothing.
        write_checkpoint(ck, results)
    shards = shard_image_list(todo, n_gpus)
    shard_kwargs = dict(kwargs)
    if worker is None:
        shard_kwargs['_n_gpus'] = n_gpus
    got = run_spawned_shards(worker or _shard_worker, [(model_file, shards[g], dict(shard_kwargs)) for g in range(n_gpus)],
                             n_gpus)
    return merge_shard_results([results] + got, expected_files=files)


def load_sharded_checkpoints(checkpoint_path, n_gpus):
    """what a sharded run left behind: the union of `<checkpoint_path>.shard<g>` (and of the plain file, if any)"""
    results, seen = [], set()
    paths = [checkpoint_path] + [shard_checkpoint_path(checkpoint_path, g) for g in range(max(1, n_gpus))]
    for p in paths:
        if p and os.path.isfile(p):
            for r in load_checkpoint(p):
                if r['file'] not in seen:
                    seen.add(r['file'])
                    results.append(r)
    return results


def load_previous_results(previous_results_file, image_folder):
    """
    reference :2056-2096: results of an earlier pass over the same folder (relative paths), made absolute the way
    the final output stage expects them.  Returns the list of image entries.
    """
    assert os.path.isfile(previous_results_file), 'Could not find previous results file {}'.format(previous_results_file)
    with open(previous_results_file, 'r') as f:
        previous = json.load(f)
    assert previous['detection_categories'] == DEFAULT_DETECTOR_LABEL_MAP, \
        "Can't merge previous results when those results use a different set of detection categories"
    print('Loaded previous results for {} images from {}'.format(len(previous['images']), previous_results_file))
    assert os.path.isdir(image_folder)
    for im in previous['images']:
        assert not os.path.isabs(im['file']), 'When processing previous results, relative paths are required'
        im['file'] = os.path.join(image_folder, im['file']).replace('\\', '/')
    return previous['images']


# --------------------------------------------------------------------------------------------
# CLI (reference :1763-2186, the options that concern this path)
# --------------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description='Run MegaDetector (HIP / MI355X path) on a batch of images')
    ap.add_argument('detector_file', help='.pt checkpoint, known model name (MDV5A ...; resolved through the '
                                          'environment variable of the same name) or "synthetic"')
    ap.add_argument('image_file', help='image file, folder, or .json/.txt list of image paths')
    ap.add_argument('output_file', help='output .json')
    ap.add_argument('--recursive', action='store_true', default=True)
    ap.add_argument('--output_relative_filenames', action='store_true')
    ap.add_argument('--quiet', action='store_true')
    ap.add_argument('--image_size', type=int, default=None)
    ap.add_argument('--augment', action='store_true')
    ap.add_argument('--use_image_queue', action='store_true')
    ap.add_argument('--preprocess_on_image_queue', action='store_true')
    ap.add_argument('--use_threads_for_queue', action='store_true',
                    help='loader threads instead of loader processes (reference :1814); without it the image queue '
                         'uses spawned processes and the page-locked shared-memory ring (feed.py)')
    ap.add_argument('--loader_workers', type=int, default=default_loaders)
    ap.add_argument('--batch_size', type=int, default=1)
    ap.add_argument('--threshold', type=float, default=DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD)
    ap.add_argument('--checkpoint_frequency', type=int, default=-1)
    ap.add_argument('--checkpoint_path', type=str, default=None)
    ap.add_argument('--resume_from_checkpoint', type=str, default=None)
    ap.add_argument('--include_max_conf', action='store_true')
    ap.add_argument('--include_image_size', action='store_true')
    ap.add_argument('--include_image_timestamp', action='store_true')
    ap.add_argument('--detector_options', nargs='*', metavar='KEY=VALUE', default='')
    ap.add_argument('--previous_results_file', type=str, default=None,
                    help='results of a previous run over the same folder: images in it are skipped and its entries '
                         'are merged into the output (needs a folder and --output_relative_filenames; reference :1894)')
    ap.add_argument('--overwrite_handling', type=str, default='overwrite', choices=['skip', 'overwrite', 'error'])
    ap.add_argument('--n_gpus', type=int, default=1, help='shard the image list over this many GPUs')
    ap.add_argument('--gpu_jpeg', action='store_true',
                    help='with --use_image_queue and loader processes: the loaders only entropy-decode baseline JPEGs, the GPU '
                         'rebuilds the pixels PIL would have decoded (bit for bit); other files are decoded with PIL as usual')
    ap.add_argument('--gpu_jpeg_entropy', action='store_true',
                    help='as --gpu_jpeg, and the GPU Huffman-decodes too: the loaders only parse the headers and ship the '
                         'compressed scan; a file the GPU flags is decoded with PIL in the detector process')
    ap.add_argument('--crop_folder', type=str, default=None,
                    help='write every detection at or above --crop_confidence_threshold below this folder, named and cut as '
                         'create_crop_folder.py does; JPEG crops are encoded on the GPU from the image that is resident there')
    ap.add_argument('--crop_confidence_threshold', type=float, default=0.1)
    ap.add_argument('--crop_expansion', type=int, default=0, help='pixels added on every side of a crop')
    ap.add_argument('--crop_quality', type=int, default=95)
    ap.add_argument('--crop_categories', type=str, default=None, help='comma-separated category names; default: all')
    ap.add_argument('--crop_results_file', type=str, default=None,
                    help='the results with crop_id and crop_filename_relative added (create_crop_folder output_file)')
    ap.add_argument('--crops_output_file', type=str, default=None,
                    help='one entry per crop (create_crop_folder crops_output_file)')
    ap.add_argument('--blur_folder', type=str, default=None,
                    help='write a copy of every image with a detection of --blur_categories at or above '
                         '--blur_confidence_threshold to this folder (same relative path), those boxes blurred as '
                         'separate_detections_into_folders.py --category_names_to_blur blurs them; the copy is blurred and '
                         'encoded on the GPU from the image that is resident there.  No other image is written')
    ap.add_argument('--blur_categories', type=str, default=None, help='comma-separated category names; default: person')
    ap.add_argument('--blur_confidence_threshold', type=float, default=None,
                    help='default: {} (the typical detection threshold the reference script falls back to)'.format(
                        blur_mod.DEFAULT_BLUR_CONFIDENCE_THRESHOLD))
    ap.add_argument('--blur_radius', type=float, default=None, help='radius of the Gaussian; default 40, as the reference')
    ap.add_argument('--blur_quality', type=int, default=None, help='JPEG quality of the copies; default 85, as the reference')
    ap.add_argument('--preview_folder', type=str, default=None,
                    help='write an annotated copy of every image to this folder as anno_<name>, as '
                         'visualize_detector_output.py does: resized to --preview_width with the LANCZOS filter, boxes and '
                         'labels drawn; resized, drawn and encoded on the GPU from the image that is resident there')
    ap.add_argument('--preview_width', type=int, default=None, help='width of the previews; default 1000, -1: no resize')
    ap.add_argument('--preview_confidence_threshold', type=float, default=None, help='boxes at or above it are drawn; default 0.15')
    ap.add_argument('--preview_detections_only', action='store_true', help='no preview of an image without such a box')
    ap.add_argument('--preview_preserve_paths', action='store_true', help='<folder>/<relative path> instead of anno_<name>')
    ap.add_argument('--preview_box_thickness', type=float, default=None, help='default 4; below 1: a fraction of the width')
    ap.add_argument('--preview_box_expansion', type=float, default=None, help='default 0; below 1: a fraction of the width')
    ap.add_argument('--preview_label_font_size', type=float, default=None, help='default 16; below 1: a fraction of the width')
    ap.add_argument('--preview_label_font', type=str, default=None, help="default arial.ttf; Pillow's default font if not found")
    ap.add_argument('--preview_blur_categories', type=str, default=None, help='comma-separated category names blurred before drawing')
    ap.add_argument('--preview_quality', type=int, default=None, help="JPEG quality; default 75, Pillow's own, as the reference")
    ap.add_argument('--classifier', type=str, default=None, metavar='MODEL',
                    help='a TorchScript classifier (torch.jit.load): every detection at or above --classify_confidence_threshold is '
                         'classified as classification/run_classifier.py classifies crop files; the crops go from the image that is '
                         'resident on the GPU to the model in one kernel.  Results go to --classification_results_file')
    ap.add_argument('--classifier_categories', type=str, default=None, metavar='FILE', help='JSON {"0": name, ...}; default: the index')
    ap.add_argument('--classifier_image_size', type=int, default=None, help='default 224')
    ap.add_argument('--classifier_no_square_crops', action='store_true', help='crop the box itself, not the square around it')
    ap.add_argument('--classifier_interpolation', type=str, default=None, choices=sorted(classify_mod.FILTERS), help='default bicubic')
    ap.add_argument('--classify_confidence_threshold', type=float, default=None, help='detections at or above it are classified; default 0.1')
    ap.add_argument('--classify_categories', type=str, default=None, help='comma-separated detection category names; default: all')
    ap.add_argument('--classification_threshold', type=float, default=None, help='classes at or above it are written; default 0.1')
    ap.add_argument('--classifier_batch_size', type=int, default=None, help='crops per run of the model; default 64')
    ap.add_argument('--classifier_jpeg_quality', type=int, default=None, metavar='Q',
                    help='give every crop the JPEG file round trip of the reference (75 there) on the GPU; default: the source pixels')
    ap.add_argument('--classification_results_file', type=str, default=None, metavar='F',
                    help='the results with classifications; default <output>.classified.json')
    ap.add_argument('--rde_results_file', type=str, default=None, metavar='F',
                    help='after the run, mark the repeat detections of the results (repeat_detections.find_repeat_detections: a box a '
                         'camera was given --rde_occurrence_threshold times gets a negative confidence) and write them to F and '
                         'F.rde_index.json; the output file and the checkpoints are what they are without it')
    ap.add_argument('--rde_review_folder', type=str, default=None, metavar='DIR',
                    help='with --rde_results_file: also write the review folder DIR/filtering_<date>/ (rde_review.write_review_folder: one '
                         'sample image per suspicious candidate; after a review, python -m megadetector_amd.rde_review remove un-marks '
                         'the candidates whose samples were deleted); the images are read from the image folder of the run')
    ap.add_argument('--rde_occurrence_threshold', type=int, default=None, help='default 20, as the reference')
    ap.add_argument('--rde_iou_threshold', type=float, default=None, help='default 0.9, as the reference')
    ap.add_argument('--rde_backend', type=str, default=None, choices=('gpu', 'host'),
                    help="default gpu; 'host': the host model of the kernels")
    ap.add_argument('--verbose', action='store_true')
    args = ap.parse_args(argv)
    if args.rde_results_file is None:
        assert args.rde_occurrence_threshold is None and args.rde_iou_threshold is None and args.rde_backend is None, \
            '--rde_occurrence_threshold / --rde_iou_threshold / --rde_backend need --rde_results_file'
        assert args.rde_review_folder is None, '--rde_review_folder needs --rde_results_file'
    if args.rde_review_folder is not None:
        assert os.path.isdir(args.image_file), '--rde_review_folder needs a folder of images as the input'
    classify_sub = {k: getattr(args, k) for k in ('classifier_categories', 'classifier_image_size', 'classifier_interpolation',
                                                  'classify_confidence_threshold', 'classify_categories', 'classification_threshold',
                                                  'classifier_batch_size', 'classifier_jpeg_quality', 'classification_results_file')}
    if args.classifier is None:
        assert all(v is None for v in classify_sub.values()) and not args.classifier_no_square_crops, \
            '--classifier_* / --classify_* / --classification_* need --classifier'
    else:
        # the classifications live in this process until the run ends: neither a checkpoint nor a shard carries them
        assert args.n_gpus <= 1 and not args.resume_from_checkpoint, '--classifier runs on one GPU and does not resume from a checkpoint'
    preview_sub = {k: getattr(args, k) for k in ('preview_width', 'preview_confidence_threshold', 'preview_box_thickness',
                                                 'preview_box_expansion', 'preview_label_font_size', 'preview_label_font',
                                                 'preview_blur_categories', 'preview_quality')}
    if args.preview_folder is None:
        assert all(v is None for v in preview_sub.values()) and not args.preview_detections_only and not args.preview_preserve_paths, \
            '--preview_width / --preview_confidence_threshold / --preview_detections_only / --preview_preserve_paths / ' \
            '--preview_box_thickness / --preview_box_expansion / --preview_label_font_size / --preview_label_font / ' \
            '--preview_blur_categories / --preview_quality need --preview_folder'
    if args.blur_folder is None:
        assert args.blur_categories is None and args.blur_confidence_threshold is None and args.blur_radius is None \
            and args.blur_quality is None, '--blur_categories / --blur_confidence_threshold / --blur_radius / --blur_quality need --blur_folder'
    if args.crop_folder is None:
        assert args.crop_results_file is None and args.crops_output_file is None, \
            '--crop_results_file / --crops_output_file need --crop_folder'

    assert 0.0 <= args.threshold <= 1.0, 'Confidence threshold needs to be between 0 and 1'
    assert args.output_file.endswith('.json'), 'output_file specified needs to end with .json'
    if args.checkpoint_frequency != -1:
        assert args.checkpoint_frequency > 0, 'Checkpoint_frequency needs to be > 0 or == -1'
    if args.output_relative_filenames:
        assert os.path.isdir(args.image_file), \
            'Could not find folder {}, must supply a folder when --output_relative_filenames is set'.format(args.image_file)
    if args.previous_results_file is not None:
        assert os.path.isdir(args.image_file) and args.output_relative_filenames, \
            'Can only process previous results when using relative paths'
    if os.path.exists(args.output_file):
        if args.overwrite_handling == 'overwrite':
            print('Warning: output file {} already exists and will be overwritten'.format(args.output_file))
        elif args.overwrite_handling == 'skip':
            print('Output file {} exists, returning'.format(args.output_file))
            return
        else:
            raise Exception('Output file {} exists'.format(args.output_file))
    results = None
    checkpoint_path = args.checkpoint_path
    if args.checkpoint_frequency > 0 and checkpoint_path is None:
        checkpoint_path = os.path.join(os.path.dirname(os.path.abspath(args.output_file)),
                                       'md_checkpoint_{}.json'.format(datetime.now().strftime('%Y%m%d%H%M%S')))
    if args.resume_from_checkpoint:
        results = load_sharded_checkpoints(args.resume_from_checkpoint, args.n_gpus) if args.n_gpus > 1 \
            else load_checkpoint(args.resume_from_checkpoint)
    files = _resolve_image_list(args.image_file)
    print('{} image files found in the input'.format(len(files)))
    previous_images = None
    if args.previous_results_file is not None:
        previous_images = load_previous_results(args.previous_results_file, args.image_file)
        previous_set = set(im['file'] for im in previous_images)
        keep = [f for f in files if f.replace('\\', '/') not in previous_set]
        print('Based on previous results file, processing {} of {} images'.format(len(keep), len(files)))
        files = keep
    kwargs = dict(checkpoint_path=checkpoint_path, confidence_threshold=args.threshold,
                  checkpoint_frequency=args.checkpoint_frequency, use_image_queue=args.use_image_queue,
                  quiet=args.quiet, image_size=args.image_size, include_image_size=args.include_image_size,
                  include_image_timestamp=args.include_image_timestamp, augment=args.augment,
                  detector_options=parse_kvp_list(args.detector_options), loader_workers=args.loader_workers,
                  preprocess_on_image_queue=args.preprocess_on_image_queue, batch_size=args.batch_size,
                  verbose_output=args.verbose, use_threads_for_queue=args.use_threads_for_queue,
                  gpu_jpeg='entropy' if args.gpu_jpeg_entropy else args.gpu_jpeg)
    crop_base = os.path.abspath(args.image_file) if os.path.isdir(args.image_file) else None
    if args.crop_folder is not None:
        kwargs.update(crop_folder=args.crop_folder, crop_confidence_threshold=args.crop_confidence_threshold,
                      crop_expansion=args.crop_expansion, crop_quality=args.crop_quality, crop_categories=args.crop_categories,
                      crop_base=crop_base)
    if args.blur_folder is not None:
        kwargs.update(blur_folder=args.blur_folder, blur_categories=args.blur_categories or 'person',
                      blur_confidence_threshold=args.blur_confidence_threshold,
                      blur_radius=blur_mod.DEFAULT_BLUR_RADIUS if args.blur_radius is None else args.blur_radius,
                      blur_quality=blur_mod.DEFAULT_BLUR_QUALITY if args.blur_quality is None else args.blur_quality,
                      blur_base=crop_base)
    if args.preview_folder is not None:
        whole = lambda v: int(v) if v is not None and v >= 1 else v     # (pixels are whole numbers; a fraction stays one)
        kwargs.update(preview_folder=args.preview_folder, preview_detections_only=args.preview_detections_only,
                      preview_preserve_paths=args.preview_preserve_paths, preview_base=crop_base,
                      **{k: v for k, v in preview_sub.items() if v is not None})
        for k in ('preview_box_thickness', 'preview_box_expansion', 'preview_label_font_size'):
            if k in kwargs:
                kwargs[k] = whole(kwargs[k])
    classify_options = None
    if args.classifier is not None:
        names = [v for v in (args.classify_categories or '').replace(',', ' ').split() if v]
        given = {'categories': args.classifier_categories, 'image_size': args.classifier_image_size,
                 'interpolation': args.classifier_interpolation, 'confidence_threshold': args.classify_confidence_threshold,
                 'classification_threshold': args.classification_threshold, 'batch_size': args.classifier_batch_size,
                 'jpeg_quality': args.classifier_jpeg_quality}
        classify_options = classify_mod.ClassifyOptions(args.classifier, square_crops=not args.classifier_no_square_crops,
                                                        category_names_to_include=names or None,
                                                        **{k: v for k, v in given.items() if v is not None})
        classify_options.category_ids()                      # (a category name the label map does not hold ends the run here)
        kwargs.update(classify_options=classify_options)
    t0 = time.time()
    if args.n_gpus > 1:
        results = run_sharded(args.detector_file, files, args.n_gpus, results=results, **kwargs)
    else:
        results = load_and_run_detector_batch(args.detector_file, files, results=results, **kwargs)
    elapsed = time.time() - t0
    print('Finished inference for {} images in {:.1f} s ({:.2f} images per second)'.format(
        len(results), elapsed, len(results) / max(elapsed, 1e-9)))
    base = os.path.abspath(args.image_file) if (args.output_relative_filenames and os.path.isdir(args.image_file)) else None
    if previous_images is not None:                      # reference :2166-2171
        previous_set = set(im['file'] for im in previous_images)
        assert not previous_set.intersection(r['file'] for r in results), \
            'Previous results handling error: redundant image filenames'
        results.extend(previous_images)
    final_output = write_results_to_file(results, args.output_file, relative_path_base=base, detector_file=args.detector_file,
                                         include_max_conf=args.include_max_conf)
    if args.crop_folder is not None and (args.crop_results_file or args.crops_output_file):
        write_crop_result_files(final_output, _crop_options(args.crop_confidence_threshold, args.crop_expansion, args.crop_quality,
                                                            args.crop_categories), crop_base, args.crop_results_file, args.crops_output_file)
    if classify_options is not None:
        write_classified_results(final_output, last_classifications, classify_options,
                                 args.classification_results_file or os.path.splitext(args.output_file)[0] + '.classified.json', base)
        print('Classified {} detections ({} skipped)'.format(last_classify_counts['gpu'] + last_classify_counts['host'],
                                                             last_classify_counts['skipped']))
    if args.rde_results_file is not None:
        from megadetector_amd import repeat_detections as rde_mod
        rde_options = rde_mod.RepeatDetectionOptions()
        if args.rde_occurrence_threshold is not None:
            rde_options.occurrenceThreshold = args.rde_occurrence_threshold
        if args.rde_iou_threshold is not None:
            rde_options.iouThreshold = args.rde_iou_threshold
        marked = rde_mod.mark_repeat_detections(copy.deepcopy(final_output), rde_options, backend=args.rde_backend or 'gpu')
        rde_mod.write_outputs(marked, rde_options, args.rde_results_file)
        print('Marked {} repeat detections; results saved at {}'.format(marked.n_bbox_changes, args.rde_results_file))
        if args.rde_review_folder is not None:
            from megadetector_amd import rde_review
            review_options = rde_review.ReviewFolderOptions()
            review_options.imageBase, review_options.outputBase = os.path.abspath(args.image_file), args.rde_review_folder
            # on the detector's own context where this process has one (a sharded run has none here: a context without a model)
            counts = rde_review.write_review_folder(marked, review_options, backend=args.rde_backend or 'gpu',
                                                    ctx=getattr(last_detector, '_ctx', None), rde_options=rde_options)
            print('Wrote {} review samples to {} ({} on the GPU, {} by PIL)'.format(counts['sheets'], counts['folder'], counts['gpu'], counts['host']))
    for cp in [checkpoint_path] + [shard_checkpoint_path(checkpoint_path, g) for g in range(max(1, args.n_gpus))]:
        if cp and os.path.isfile(cp):
            os.remove(cp)
            print('Deleted checkpoint file {}'.format(cp))


if __name__ == '__main__':
    main()
