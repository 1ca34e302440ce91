"""
Sorting the images of a results file into folders, as the reference does it (postprocessing/
separate_detections_into_folders.py): animals/, people/, vehicles/, animals_people/ ..., empty/, processing_failure/ and, with
classification thresholds, animals/deer/ and so on -- by copying or moving the files, or, with render_boxes or
category_names_to_blur, by writing a MANIPULATED copy: people blurred, one set of boxes per category above its threshold, saved
by exif_preserving_save(quality='keep').

What is restated statement for statement (separate_detections_into_folders.py:230-696): the validation, the thresholds and the
folder map (resolve_options), the decision per image (decide: a pure function of the image's entry and the options) and the
file handling (_dispose).  What a manipulated copy is has two legs that write the same bytes:

  backend='host'   exactly the reference's PIL calls: load_image, blur_detections, one render_detection_bounding_boxes per
                   category above threshold in sorted name order, exif_preserving_save(quality='keep').
  backend='gpu'    the device render path (device_render.py; DESIGN.md, "the device render path"), per chunk of images
                   (device_render.run_chunks): every file decoded once on the device (device_decode.decode_stage), ONE
                   mdhip_blur_regions call, ONE mdhip_draw_ops call with the preview.render_plan of the categories one behind
                   the other (RenderPlan.extend), ONE mdhip_jpeg_encode_sampled call for all images of the chunk -- each
                   with the sampling and the quantisation tables Pillow's quality='keep' takes from its source file
                   (device_render.encode_copies) -- and jpeg_host.sampled_file around each scan.

For a plain RGB JPEG, which is what a camera trap writes, quality='keep' re-encodes with the SOURCE file's quantisation tables
and chroma sampling and writes an EXIF APP1 segment and the source's COM segment.  A file open_image makes a new image of (an
EXIF rotation, an 'L' file) is no JPEG to Pillow any more and is saved at quality 85 with 4:2:0: both forms are made on the
device.  A file goes to the host leg as a whole, and is counted as 'host' in what separate_detections_into_folders returns, when
the device does not decode it (a progressive file; also a file Pillow calls 'MPO', which device_decode.probe leaves to PIL,
though its saved form would be the quality-85 one), when its name is not a JPEG's, when its saved form is not one the device restates (not exactly
two 8-bit tables, a sampling other than 4:4:4 / 4:2:2 / 4:2:0, a box thinner than its outline, classification labels on the
boxes) or when its rendering fails on the device.

keep_source_blocks (not in the reference, off by default): a manipulated copy of a plain RGB JPEG keeps the SOURCE file's
quantised coefficients in every MCU that no blur rectangle and no drawing operation touches, and only the touched MCUs are
re-encoded (device_render.encode_kept on the device leg, device_render.kept_file_host on the host leg: the same bytes).  Every
other copy, and one whose merged blocks no baseline scan holds, is written exactly as without the option; the counts say how
many of each ('kept', 'kept_refused').

Not restated: nothing of run_detector_batch changes, there is no multi-GPU sharding, and n_threads applies to the host leg.

Command line:  python -m megadetector_amd.separate_detections RESULTS INPUT_DIR OUTPUT_DIR [the reference's flags]
               [--backend gpu|host] [--device 0] [--keep_source_blocks]
"""

import argparse
import itertools
import json
import os
import shutil
import sys
from functools import partial

from . import device_render as DR
from . import preview as PV
from .blur import DEFAULT_BLUR_QUALITY, blur_rectangle
from .ref_utils import exif_preserving_save, path_is_abs

friendly_folder_names = {'animal': 'animals', 'person': 'people', 'vehicle': 'vehicles'}
default_line_thickness = 8
default_box_expansion = 3
fallback_detection_threshold = 0.2               # detection/run_detector.py:83


class SeparateDetectionsIntoFoldersOptions:
    """The reference's options, under its names and with its defaults."""

    def __init__(self, threshold=None):
        self.threshold = None                            #: default threshold (None: the detector's typical one)
        self.category_name_to_threshold = {'animal': self.threshold, 'person': self.threshold, 'vehicle': self.threshold}
        self.n_threads = 1                               #: workers of the host leg; <= 1: none
        self.rendering_pool_type = 'threads'             #: 'threads' or 'processes'
        self.allow_existing_directory = False
        self.allow_missing_files = False
        self.overwrite = True
        self.skip_empty_images = False
        self.results_file = None
        self.base_input_folder = None
        self.base_output_folder = None
        self.move_images = False
        self.render_boxes = False
        self.show_box_labels = False
        self.line_thickness = default_line_thickness
        self.box_expansion = default_box_expansion
        self.classification_thresholds = None            #: a dict, or 'deer=0.75,cow=0.75'
        self.unlisted_category_threshold = 0.5
        self.classification_category_id_to_name = None   # (set from the results)
        self.classification_categories = None            # (set from the results)
        self.debug_max_images = None
        self.category_name_to_folder = None              # (set from the results)
        self.category_id_to_category_name = None         # (set from the results)
        self.category_names_to_blur = None               #: a list, or 'person,vehicle'
        self.remove_empty_folders = False
        self.verbose = False
        self.keep_source_blocks = False                  #: (not the reference's) manipulated copies keep the source's JPEG blocks


def is_float(s):
    """utils/string_utils.py is_float"""
    if s is None:
        return False
    try:
        _ = float(s)
    except ValueError:
        return False
    return True


def get_typical_confidence_threshold_from_results(results):
    """detection/run_detector.py:504-551"""
    from .run_detector import get_detector_metadata_from_version_string, get_detector_version_from_filename
    default_threshold = None
    if 'detector_metadata' in results['info'] and 'typical_detection_threshold' in results['info']['detector_metadata']:
        default_threshold = results['info']['detector_metadata']['typical_detection_threshold']
    elif ('detector' not in results['info']) or (results['info']['detector'] is None):
        print('Warning: detector version not available in results file, using MDv5 defaults')
        default_threshold = get_detector_metadata_from_version_string('v5a.0.0')['typical_detection_threshold']
    else:
        print('Warning: detector metadata not available in results file, inferring from MD version')
        try:
            detector_version = get_detector_version_from_filename(results['info']['detector'])
            detector_metadata = get_detector_metadata_from_version_string(detector_version)
            if 'typical_detection_threshold' in detector_metadata:
                default_threshold = detector_metadata['typical_detection_threshold']
        except Exception:
            pass
    if default_threshold is None:
        print('Could not determine threshold, using fallback threshold of {}'.format(fallback_detection_threshold))
        default_threshold = fallback_detection_threshold
    return default_threshold


def remove_empty_folders(path, remove_root=False):
    """utils/path_utils.py remove_empty_folders"""
    if not os.path.isdir(path):
        return False
    is_empty = True
    for item in os.listdir(path):
        item_path = os.path.join(path, item)
        if os.path.isdir(item_path):
            if not remove_empty_folders(item_path, True):
                is_empty = False
        else:
            is_empty = False
    if is_empty and remove_root:
        try:
            os.rmdir(path)
        except Exception as e:
            print('Error removing directory {}: {}'.format(path, str(e)))
            is_empty = False
    return is_empty


# ---- options and the decision per image --------------------------------------------------------------------------------------

def check_options(options):
    """separate_detections_into_folders.py:524-533"""
    assert not (options.render_boxes and options.move_images), 'Cannot specify both render_boxes and move_images'
    assert not ((options.category_names_to_blur is not None) and options.move_images), \
        'Cannot specify both category_names_to_blur and move_images'
    if (options.debug_max_images is not None) and (options.debug_max_images < 0):
        options.debug_max_images = None


def resolve_options(options, results):
    """
    separate_detections_into_folders.py:549-657 without the file system: the check for absolute paths, the default and the
    per-category thresholds, the folder of every category, of every combination of categories, of 'empty' and of 'failure',
    and the classification thresholds, all written into `options` as the reference writes them.  -> the folders to create
    """
    images = results['images']
    for im in images:
        assert not path_is_abs(im['file'], leading_backslash=False), 'Cannot process results with absolute image paths'
    default_threshold = options.threshold
    if default_threshold is None:
        default_threshold = get_typical_confidence_threshold_from_results(results)
    detection_categories = results['detection_categories']
    options.detection_categories = detection_categories
    options.category_id_to_category_name = detection_categories
    options.category_name_to_folder = {}
    options.category_name_to_folder['empty'] = os.path.join(options.base_output_folder, 'empty')
    options.category_name_to_folder['failure'] = os.path.join(options.base_output_folder, 'processing_failure')
    category_names = list(detection_categories.values())
    category_names.sort()
    for category_name in category_names:
        if category_name not in options.category_name_to_threshold:
            print('Warning: category {} in detection file, but not in threshold mapping'.format(category_name))
            options.category_name_to_threshold[category_name] = None
        if options.category_name_to_threshold[category_name] is None:
            options.category_name_to_threshold[category_name] = default_threshold
        print('Processing category {} at threshold {}'.format(category_name, options.category_name_to_threshold[category_name]))
    target_category_names = list(category_names)
    for combination_length in range(2, len(category_names) + 1):
        for combination in itertools.combinations(category_names, combination_length):
            target_category_names.append('_'.join(combination))
    for category_name in target_category_names:
        folder_name = friendly_folder_names.get(category_name, category_name)
        options.category_name_to_folder[category_name] = os.path.join(options.base_output_folder, folder_name)
    if options.classification_thresholds is not None:
        assert 'classification_categories' in results and results['classification_categories'] is not None, \
            'Classification thresholds specified, but no classification results available'
        classification_categories = results['classification_categories']
        classification_category_name_to_id = {v: k for k, v in classification_categories.items()}
        options.classification_category_id_to_name = {k: v for k, v in classification_categories.items()}
        options.classification_categories = classification_categories
        if isinstance(options.classification_thresholds, str):
            classification_thresholds = {}
            for token in options.classification_thresholds.split(','):
                subtokens = token.split('=')
                assert (len(subtokens) == 2) and (is_float(subtokens[1])), 'Illegal classification threshold {}'.format(token)
                classification_thresholds[subtokens[0]] = float(subtokens[1])
            options.classification_thresholds = classification_thresholds
        for class_name in options.classification_thresholds.keys():
            assert class_name in classification_category_name_to_id, \
                'Category {} specified at the command line, but is not available in the results file'.format(class_name)
    return list(options.category_name_to_folder.values())


def using_classification_folders(options):
    return (options.classification_thresholds is not None) and (len(options.classification_thresholds) > 0)


def decide(im, options):
    """
    _process_detections :239-393: (target folder, categories above threshold) of one image entry -- the categories sorted, None
    for an image that failed.  A pure function of the entry and the resolved options: no file is touched.
    """
    relative_filename = im['file']
    detections = None
    if 'detections' in im:
        detections = im['detections']
    if detections is None:
        assert im['failure'] is not None and len(im['failure']) > 0
        return options.category_name_to_folder['failure'], None
    category_name_to_max_confidence = {}
    category_names = options.category_id_to_category_name.values()
    for category_name in category_names:
        category_name_to_max_confidence[category_name] = 0.0
    for det in detections:
        category_id = det['category']
        if category_id not in options.category_id_to_category_name:
            print('Warning: unrecognized category {} in file {}'.format(category_id, relative_filename))
            continue
        category_name = options.category_id_to_category_name[category_id]
        if det['conf'] > category_name_to_max_confidence[category_name]:
            category_name_to_max_confidence[category_name] = det['conf']
    categories_above_threshold = []
    for category_name in category_names:
        threshold = options.category_name_to_threshold[category_name]
        assert threshold is not None
        if category_name_to_max_confidence[category_name] >= threshold:
            categories_above_threshold.append(category_name)
    categories_above_threshold.sort()
    if len(categories_above_threshold) > 1:
        target_folder = options.category_name_to_folder['_'.join(categories_above_threshold)]
    elif len(categories_above_threshold) == 0:
        target_folder = options.category_name_to_folder['empty']
    else:
        target_folder = options.category_name_to_folder[categories_above_threshold[0]]
        if ('animal' in categories_above_threshold) and using_classification_folders(options):
            category_name_to_id = {v: k for k, v in options.category_id_to_category_name.items()}
            animal_category_id = category_name_to_id['animal']
            valid_animal_detections = [d for d in detections if (d['category'] == animal_category_id and
                                                                 d['conf'] >= options.category_name_to_threshold['animal'])]
            listed, unlisted = set(), set()
            for d in valid_animal_detections:
                if 'classifications' not in d or d['classifications'] is None:
                    continue
                for classification in d['classifications']:
                    classification_category_id = classification[0]
                    classification_confidence = classification[1]
                    assert options.classification_category_id_to_name is not None
                    name = options.classification_category_id_to_name[classification_category_id]
                    if name in options.classification_thresholds:
                        if classification_confidence > options.classification_thresholds[name]:
                            listed.add(name)
                    elif classification_confidence > options.unlisted_category_threshold:
                        unlisted.add(name)
            if len(listed) == 0:
                classification_folder_name = 'unclassified'
            elif (len(listed) > 1) or (len(unlisted) > 1):
                classification_folder_name = 'multiple'
            else:
                assert len(listed) == 1
                classification_folder_name = list(listed)[0]
            target_folder = os.path.join(target_folder, classification_folder_name)
    return target_folder, categories_above_threshold


# ---- what a manipulated copy is ------------------------------------------------------------------------------------------------

def names_to_blur(options):
    """:436-442: None, or the list of category names"""
    names = options.category_names_to_blur
    if names is not None and isinstance(names, str):
        names = [s.strip() for s in names.split(',')]
    return names


def detections_to_blur(detections, options):
    """:444-449, in the order of the file (the order matters where boxes overlap); an unknown category raises KeyError as there"""
    names = names_to_blur(options)
    if names is None:
        return []
    out = []
    for d in detections:
        category_name = options.category_id_to_category_name[d['category']]
        if (d['conf'] >= options.category_name_to_threshold[category_name]) and (category_name in names):
            out.append(d)
    return out


def category_passes(detections, categories_above_threshold, options):
    """
    :456-493: one (detections, PreviewOptions, label map, labels) per category above threshold, in the order of the list, as
    preview.render_plan and preview.render_with_pil take them.  The classifications stay on a detection only where the
    reference keeps them: with classification folders AND show_box_labels.
    """
    category_name_to_id = {v: k for k, v in options.category_id_to_category_name.items()}
    assert len(category_name_to_id) == len(options.category_id_to_category_name)
    keep_classifications = using_classification_folders(options) and options.show_box_labels
    passes = []
    for category_name in categories_above_threshold:
        category_id = category_name_to_id[category_name]
        category_threshold = options.category_name_to_threshold[category_name]
        assert category_threshold is not None
        category_detections = [d for d in detections if d['category'] == category_id]
        if not keep_classifications:
            category_detections = [{k: v for k, v in d.items() if k != 'classifications'} for d in category_detections]
        o = PV.PreviewOptions(confidence_threshold=0, output_image_width=None, box_thickness=options.line_thickness,
                              box_expansion=options.box_expansion)
        o.confidence_threshold = category_threshold
        passes.append((category_detections, o, options.detection_categories if options.show_box_labels else None,
                       bool(options.show_box_labels)))
    return passes


def rectangles_to_blur(detections, options, width, height):
    """the rectangles with area of detections_to_blur, in the order they are applied"""
    rects = [blur_rectangle(d['bbox'], width, height) for d in detections_to_blur(detections, options)]
    return [r for r in rects if r is not None]


def _plan(detections, categories_above_threshold, options, width, height):
    """what is drawn on a copy as ONE preview.RenderPlan: the render_plan of every category pass, one behind the other.  Raises
    preview.HostLeg, also where the reference's own drawing raises (the host leg then raises it as the reference does)."""
    plan = PV.RenderPlan()
    try:
        for category_detections, o, label_map, labels in category_passes(detections, categories_above_threshold, options):
            plan.extend(PV.render_plan(category_detections, width, height, o, label_map, labels))
    except PV.RenderFailure as e:
        raise PV.HostLeg(str(e))
    return plan


def keep_source_record(source_path, target_path):
    """What the host leg needs of a source file to keep its blocks in a copy -- {'src': jpeg_host.keep_source's record, 'coef':
    its quantised planes (jpeg_host.decode), 'size'} -- or None when a copy of it at target_path is not eligible: the name is
    no JPEG's, the source is not an RGB JPEG that open_image returns as it is with two 8-bit tables at 4:4:4 / 4:2:2 / 4:2:0,
    or the coefficient decoder does not take it."""
    from PIL import Image
    from . import jpeg_host
    if Image.registered_extensions().get(os.path.splitext(target_path)[1].lower()) != 'JPEG':
        return None
    try:
        with open(source_path, 'rb') as f:
            data = f.read()
        src = jpeg_host.keep_source(source_path, data)
        if not src['keep'] or src['quant'] is None or len(src['exif']) > 65533 or len(src['comment'] or b'') > 65533:
            return None
        rc, _, coef = jpeg_host.decode(data)
    except Exception:
        return None
    if rc != jpeg_host.MDJPEG_OK or max(src['size']) > 65535:
        return None
    return {'src': src, 'coef': coef, 'size': tuple(src['size'])}


def _keep_plan_host(source_path, target_path, detections, categories_above_threshold, options):
    """keep_source_record with 'changed', the rectangles the copy's plan changes; None also when its drawing is not one the
    plan restates (the device leg sends such a copy to the host leg as a whole)"""
    keep = keep_source_record(source_path, target_path)
    if keep is None:
        return None
    width, height = keep['size']
    try:
        plan = _plan(detections, categories_above_threshold, options, width, height)
    except Exception:
        return None
    keep['changed'] = DR.changed_rectangles(rectangles_to_blur(detections, options, width, height), plan.ops)
    return keep


def save_kept_host(pil_image, target_path, keep):
    """The host leg of a kept copy (device_render.kept_file_host, with the source's EXIF block).  -> 'kept', or 'kept_refused'
    when no baseline scan holds the merged blocks (nothing is written; the caller saves the copy as without the option)"""
    data = DR.kept_file_host(pil_image, keep, keep['src']['exif'])
    if data is None:
        return 'kept_refused'
    with open(target_path, 'wb') as f:
        f.write(data)
    return 'kept'


def render_host(source_path, target_path, detections, categories_above_threshold, options):
    """:432-500 by the reference's own PIL calls: the host leg of one manipulated copy.  -> None, or with keep_source_blocks
    'kept' / 'kept_refused' for an eligible copy"""
    from .feed import load_image
    keep = None
    if getattr(options, 'keep_source_blocks', False):
        keep = _keep_plan_host(source_path, target_path, detections, categories_above_threshold, options)
    pil_image = load_image(source_path)
    DR.blur_with_pil(pil_image, rectangles_to_blur(detections, options, pil_image.size[0], pil_image.size[1]))
    # (the classifications are on the boxes only with classification folders and show_box_labels: category_passes)
    classification_label_map = options.classification_categories if using_classification_folders(options) else None
    for category_detections, o, label_map, labels in category_passes(detections, categories_above_threshold, options):
        PV.render_with_pil(pil_image, category_detections, o, label_map=label_map, labels=labels,
                           classification_label_map=classification_label_map,
                           classification_confidence_threshold=PV.DEFAULT_CLASSIFICATION_CONFIDENCE_THRESHOLD)
    kept = save_kept_host(pil_image, target_path, keep) if keep is not None else None
    if kept != 'kept':
        exif_preserving_save(pil_image, target_path)
    return kept


# ---- file handling ---------------------------------------------------------------------------------------------------------------

printed_missing_file_warning = False


def _dispose(im, options, manipulate=None):
    """
    _process_detections :395-500 for one image entry: returns what was done -- 'missing', 'exists', 'skipped', 'copied', 'moved',
    'rendered' -- after doing it.  manipulate: called with (source, target, detections, categories above threshold) for a
    manipulated copy instead of the host leg (the device leg queues it); None: render_host.
    """
    global printed_missing_file_warning
    target_folder, categories_above_threshold = decide(im, options)
    relative_filename = im['file']
    source_path = os.path.join(options.base_input_folder, relative_filename)
    if not os.path.isfile(source_path):
        if not options.allow_missing_files:
            raise ValueError('Cannot find file {}'.format(source_path))
        if not printed_missing_file_warning:
            print('Warning: cannot find at least one file ({})'.format(source_path))
            printed_missing_file_warning = True
        return 'missing'
    target_path = os.path.join(target_folder, relative_filename)
    if (not options.overwrite) and (os.path.isfile(target_path)):
        return 'exists'
    os.makedirs(os.path.dirname(target_path), exist_ok=True)
    nothing_above = (categories_above_threshold is None) or (len(categories_above_threshold) == 0)
    if nothing_above and options.skip_empty_images:
        return 'skipped'
    if (not options.render_boxes and (options.category_names_to_blur is None)) or nothing_above:
        if options.move_images:
            shutil.move(source_path, target_path)
            return 'moved'
        shutil.copyfile(source_path, target_path)
        return 'copied'
    (manipulate or render_host)(source_path, target_path, im['detections'], categories_above_threshold, options)
    return 'rendered'


def _map(function, items, options):
    """the reference's loop: serial, or its pool of threads or processes"""
    if options.n_threads <= 1:
        return [function(item) for item in items]
    return DR.pool_map(function, items, options.n_threads, options.rendering_pool_type == 'threads')


def _dispose_host(im, options):
    """-> (what _dispose did, what render_host returned for a manipulated copy)"""
    kept = []
    done = _dispose(im, options, manipulate=lambda *args: kept.append(render_host(*args)))
    return done, (kept[0] if kept else None)


def _render_job_host(job, options):
    return render_host(job['source'], job['target'], job['detections'], job['categories'], options)


# ---- the device leg ----------------------------------------------------------------------------------------------------------------

def _plan_job(job, options):
    """What the device needs for one manipulated copy, before any pixel is decoded: fills the job and returns it; raises
    preview.HostLeg (the host leg then raises what the reference raises)."""
    from . import jpeg_host
    from .device_decode import plan_source
    p, (width, height) = plan_source(job['source'], job['target'], keep_data=True)
    src = jpeg_host.keep_source(job['source'], p['data'])
    if src['keep'] and src['quant'] is None:
        raise PV.HostLeg('tables or a sampling the device does not restate')
    if len(src['exif']) > 65533 or len(src['comment'] or b'') > 65533:
        raise PV.HostLeg('an EXIF block or a comment Pillow refuses')
    if src['keep']:
        job['sampling'], job['quant'] = src['sampling'], src['quant']
    else:
        job['sampling'], job['quant'] = 2, list(jpeg_host.quant_tables(DEFAULT_BLUR_QUALITY))
    job['exif'], job['comment'], job['size'], job['probe'] = src['exif'], src['comment'], (width, height), p
    job['rects'] = rectangles_to_blur(job['detections'], options, width, height)
    job['plan'] = _plan(job['detections'], job['categories'], options, width, height)
    # eligible for keep_source_blocks: an RGB JPEG saved with its own tables and sampling (the decoder's verdict comes with the chunk)
    job['keep'] = bool(getattr(options, 'keep_source_blocks', False) and src['keep'])
    if job['keep']:
        job['changed'] = DR.changed_rectangles(job['rects'], job['plan'].ops)
    return job


def _job_bytes(job):
    """device bytes of a planned copy in its decode chunk: its pixels and, when it keeps its source's blocks, the coefficients
    that stay on the device with them"""
    return job['size'][0] * job['size'][1] * 3 + (2 * int(job['probe']['scan'].coef_count) if job['keep'] else 0)


def _render_chunk_device(ctx, torch, device, jobs, clock, options, counts):
    """The manipulated copies of one chunk, by the device render path (device_render).  -> the jobs the host leg has to make"""
    # (with copies that keep their blocks the sources' planes stay until the chunk is written)
    jobs, tensors, host, coefficients = DR.decode_front(ctx, torch, device, jobs, options.base_input_folder, counts, clock,
                                                        any(j['keep'] for j in jobs))

    def encode(tensors, jobs):
        # (a copy the kept call flagged is re-encoded whole)
        files, calls, flagged = DR.encode_copies(ctx, device, tensors, jobs, [coefficients[j['file']][0] if j['keep'] else None for j in jobs],
                                                 clock, True)
        counts['kept'] += sum(j['keep'] for j in jobs) - flagged
        counts['kept_refused'] += flagged
        return files, calls

    if jobs:                                                              # (a copy is never resized: no resample_jobs)
        DR.blur_and_draw(ctx, device, tensors, jobs, clock)
        DR.encode_and_write(jobs, tensors, counts, encode, lambda job, data: DR.write_bytes(job['target'], data))
    return host


def _render_device(jobs, options, ctx, counts, profile):
    """-> the jobs that go to the host leg: those that could not be planned, then those the chunks gave back (run_chunks
    without an order)"""
    import torch
    planned, host = DR.plan_each(jobs, partial(_plan_job, options=options))
    return DR.run_chunks(ctx, torch, planned, _job_bytes, partial(_render_chunk_device, options=options, counts=counts), counts,
                         profile, host, DR.file_twice)


# ---- the entry function ------------------------------------------------------------------------------------------------------------

def separate_detections_into_folders(options, backend='gpu', device=0, ctx=None, profile=False):
    """
    The reference's separate_detections_into_folders(options).  backend 'host': PIL, no GPU; 'gpu': the manipulated copies on
    HIP device `device`, on `ctx` (a HipContext) or on a context without a model made for the call; without render_boxes and
    category_names_to_blur nothing touches a GPU whatever the backend.  profile: also counts['ms'], the milliseconds around
    the decode, blur, draw and encode calls (the device is waited for around each: slower).
    Returns counts: 'images', and of these 'missing', 'exists', 'skipped', 'copied', 'moved' and 'rendered'; of the rendered
    ones those made on the 'gpu' and by the 'host' leg; 'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks', 'encode_calls';
    with options.keep_source_blocks 'kept', the eligible copies that kept their source's blocks, and 'kept_refused', those the
    merge refused and that were written as without the option (both 0 without it).
    """
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    check_options(options)
    if (os.path.isdir(options.base_output_folder)) and (len(os.listdir(options.base_output_folder)) > 0):
        if options.allow_existing_directory:
            print('Warning: target folder exists and is not empty... did you mean to delete an old version?')
        else:
            raise ValueError('Target folder exists and is not empty')
    os.makedirs(options.base_output_folder, exist_ok=True)
    print('Loading detection results')
    with open(options.results_file, 'r') as f:
        results = json.load(f)
    images = results['images']
    print('Processing detections for {} images'.format(len(images)))
    for folder in resolve_options(options, results):
        os.makedirs(folder, exist_ok=True)
    if (options.debug_max_images is not None) and (options.debug_max_images < len(images)):
        print('Debug: clipping list to {} images'.format(options.debug_max_images))
        images = images[0:options.debug_max_images]
    counts = {k: 0 for k in ('missing', 'exists', 'skipped', 'copied', 'moved', 'rendered', 'gpu', 'host', 'files_decoded_gpu',
                             'files_decoded_pil', 'decode_chunks', 'encode_calls', 'kept', 'kept_refused')}
    counts['images'] = len(images)
    if profile:
        counts['ms'] = {}
    manipulating = options.render_boxes or (options.category_names_to_blur is not None)
    if backend == 'host' or not manipulating:
        for done, kept in _map(partial(_dispose_host, options=options), images, options):
            counts[done] += 1
            if kept:
                counts[kept] += 1
        counts['host'] = counts['rendered']
    else:
        jobs = []

        def queue(source, target, detections, categories, _options):
            jobs.append({'file': os.path.relpath(source, options.base_input_folder), 'source': source, 'target': target,
                         'detections': detections, 'categories': categories})

        for im in images:
            counts[_dispose(im, options, manipulate=queue)] += 1
        if jobs:
            from .hip_backend import HipContext
            with HipContext.images_or(ctx, device) as ctx:
                host = _render_device(jobs, options, ctx, counts, profile)
            for kept in _map(partial(_render_job_host, options=options), host, options):
                if kept:
                    counts[kept] += 1
            counts['host'] = len(host)
    if options.remove_empty_folders:
        print('Removing empty folders from {}'.format(options.base_output_folder))
        remove_empty_folders(options.base_output_folder)
    return counts


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    parser = argparse.ArgumentParser(description='Sort the images of a results file into folders by what was detected in them')
    parser.add_argument('results_file', type=str, help='Input .json filename')
    parser.add_argument('base_input_folder', type=str, help='Input image folder')
    parser.add_argument('base_output_folder', type=str, help='Output image folder')
    parser.add_argument('--threshold', type=float, default=None, help='Default confidence threshold for all categories '
                        '(defaults to selection based on model version; other options may override it for specific categories)')
    parser.add_argument('--animal_threshold', type=float, default=None, help='Confidence threshold for the animal category')
    parser.add_argument('--human_threshold', type=float, default=None, help='Confidence threshold for the human category')
    parser.add_argument('--vehicle_threshold', type=float, default=None, help='Confidence threshold for vehicle category')
    parser.add_argument('--classification_thresholds', type=str, default=None,
                        help='Classification thresholds for species-based folder separation, e.g. "deer=0.75,cow=0.75"')
    parser.add_argument('--n_threads', type=int, default=1, help='Number of threads of the host leg (default=1)')
    parser.add_argument('--allow_existing_directory', action='store_true', help='Proceed even if the target directory exists and is not empty')
    parser.add_argument('--no_overwrite', action='store_true',
                        help='Skip images that already exist in the target folder, must also specify --allow_existing_directory')
    parser.add_argument('--skip_empty_images', action='store_true', help='Do not copy empty images to the output folder')
    parser.add_argument('--move_images', action='store_true', help='Move images (rather than copying)')
    parser.add_argument('--render_boxes', action='store_true', help='Render bounding boxes on output images')
    parser.add_argument('--line_thickness', type=int, default=default_line_thickness,
                        help='Line thickness (in pixels) for rendering (defaults to {})'.format(default_line_thickness))
    parser.add_argument('--box_expansion', type=int, default=default_box_expansion,
                        help='Box expansion (in pixels) for rendering (defaults to {})'.format(default_box_expansion))
    parser.add_argument('--category_names_to_blur', type=str, default=None,
                        help='Comma-separated list of category names to blur (or a single category name, e.g. "person")')
    parser.add_argument('--remove_empty_folders', action='store_true', help='Remove all empty folders from the target folder at the end')
    parser.add_argument('--backend', choices=('host', 'gpu'), default='gpu', help="'host': the reference's PIL calls, no GPU needed")
    parser.add_argument('--device', type=int, default=0, help='HIP device of the gpu backend')
    parser.add_argument('--keep_source_blocks', action='store_true',
                        help="Manipulated copies of RGB JPEGs keep the source file's JPEG blocks outside the boxes (not in the reference)")
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    options = SeparateDetectionsIntoFoldersOptions()
    for name in ('results_file', 'base_input_folder', 'base_output_folder', 'threshold', 'classification_thresholds', 'n_threads',
                 'allow_existing_directory', 'skip_empty_images', 'move_images', 'render_boxes', 'line_thickness', 'box_expansion',
                 'category_names_to_blur', 'remove_empty_folders', 'keep_source_blocks'):
        setattr(options, name, getattr(args, name))

    def validate_threshold(v, name):
        if v is not None:
            assert v >= 0.0 and v <= 1.0, 'Illegal {} threshold {}'.format(name, v)

    validate_threshold(args.threshold, 'default')
    validate_threshold(args.animal_threshold, 'animal')
    validate_threshold(args.vehicle_threshold, 'vehicle')
    validate_threshold(args.human_threshold, 'human')
    if args.threshold is not None:
        if args.animal_threshold is not None and args.human_threshold is not None and args.vehicle_threshold is not None:
            raise ValueError("Default threshold specified, but all category thresholds also specified... not exactly wrong, "
                             "but it's likely that you meant something else.")
    options.category_name_to_threshold['animal'] = args.animal_threshold
    options.category_name_to_threshold['person'] = args.human_threshold
    options.category_name_to_threshold['vehicle'] = args.vehicle_threshold
    options.overwrite = (not args.no_overwrite)
    counts = separate_detections_into_folders(options, backend=args.backend, device=args.device)
    print('Separated {} images ({})'.format(counts['images'], ', '.join('{} {}'.format(k, v) for k, v in counts.items() if k != 'images')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
