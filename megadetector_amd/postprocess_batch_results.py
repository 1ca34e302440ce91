"""
The HTML preview of a results file, as the reference makes it (postprocessing/postprocess_batch_results.py, the path without
ground truth): sample images from the file, sort them into result sets -- non_detections, detections_animal,
detections_animal_person ..., almost_detections, class_deer ... --, render every sampled image (open, LANCZOS to
viz_target_width, boxes and labels, saved under <set>/<set>_<flattened path>), write one HTML page per result set and an
index.html.

Restated statement for statement (:1118-1253, :1701-2127 and their helpers :441-947, utils/write_html_image_list.py,
postprocessing/load_api_results.py): loading (load_api_results, without pandas: a field an image lacks reads as MISSING, the
DataFrame's NaN, and a numeric field some images lack reads as a float, as a DataFrame column does), the failure count, the
thresholds (None, a float, a dict by category name with 'default'), the sample (sample_indices: DataFrame.sample as
numpy.random.RandomState(seed).choice), the result sets, the decision per image (decide_image: a pure function of the entry
and the options), the file names, the sub-pages (prepare_html_subpages, write_html_image_list) and the text of index.html.

What rendering one image is has two legs that write the same bytes:

  backend='host'   exactly the reference's PIL calls (_render_bounding_boxes): open_image, resize_image,
                   render_detection_bounding_boxes, Image.save; parallelize_rendering, parallelize_rendering_n_cores and
                   parallelize_rendering_with_threads size its pool.
  backend='gpu'    the device render path (device_render.py) on a context without a model: the sampled images that are not
                   bypassed, in order, cut into decode chunks (device_render.run_chunks); per chunk every file decoded once
                   on the device (device_decode.decode_stage), ONE mdhip_resample_lanczos call, ONE mdhip_draw_ops call with the
                   preview.render_plan of every image, ONE mdhip_jpeg_encode call (Pillow's quality 75 with 4:2:0) and
                   jpeg_host.jfif_file around each scan.

An image goes to the host leg as a whole, and is counted as 'host', when the device does not decode its file, when Pillow
does not map its output name to JPEG, when the plan hands its drawing to the host (preview.HostLeg) or when its rendering
fails on the device.  As for the previews, a device-made file does not carry the source file's COM segment, which Pillow
copies through Image.info.

Not restated (NotImplementedError before anything is read or written): ground_truth_json_file and what belongs to it, an
image_base_dir that is a URL, api_detection_results / api_other_fields.  A SpeciesNet predictions file is not converted.
Video entries are out of scope, as in the reference.  With backend='gpu' the host leg's pool is one of threads whatever
parallelize_rendering_with_threads says: a process that has opened the GPU is not forked.

Command line:  python -m megadetector_amd.postprocess_batch_results MD_RESULTS OUTPUT_DIR [the reference's arguments]
               [--backend gpu|host] [--device 0]
"""

import argparse
import collections
import copy
import errno
import json
import math
import os
import random
import sys
import urllib.parse
import uuid
from collections import defaultdict
from functools import partial

import numpy as np

from . import device_render as DR
from . import preview as PV
from .preview import resized_size
from .ref_utils import clean_filename, flatten_path, insert_before_extension, open_image  # noqa: F401  (compare_batch_results' too)
from .separate_detections import get_typical_confidence_threshold_from_results

DEFAULT_NEGATIVE_CLASSES = ['empty']
DEFAULT_UNKNOWN_CLASSES = ['unknown', 'unlabeled', 'ambiguous']
SAVE_QUALITY = 75                                # Image.save(path) of a JPEG: Pillow's default, with 4:2:0

MISSING = float('nan')                           # what a DataFrame holds where an image lacks a field


class PostProcessingOptions:
    """The reference's options, under its names and with its defaults (:78-261)."""

    def __init__(self):
        self.md_results_file = ''
        self.output_dir = ''
        self.image_base_dir = ''
        self.ground_truth_json_file = ''                         # (not restated)
        self.negative_classes = DEFAULT_NEGATIVE_CLASSES         # (ground truth: not restated)
        self.unlabeled_classes = DEFAULT_UNKNOWN_CLASSES         # (ground truth: not restated)
        self.rendering_bypass_sets = []                          #: result sets that are counted and listed, but not rendered
        self.confidence_threshold = None                         #: None (the detector's typical one), a float, or name -> float
        self.classification_confidence_threshold = 0.5
        self.target_recall = 0.9                                 # (ground truth: not restated)
        self.num_images_to_sample = 1000                         #: None or <= 0: all images
        self.sample_seed = 0                                     #: None: unseeded
        self.viz_target_width = 1200                             #: None: the images keep their size
        self.line_thickness = 4
        self.box_expansion = 0
        self.job_name_string = None
        self.model_version_string = None
        self.html_sort_order = 'filename'                        #: 'filename', 'confidence' or 'random'
        self.link_images_to_originals = True
        self.separate_detections_by_category = True
        self.api_output_filename_replacements = {}
        self.ground_truth_filename_replacements = {}             # (ground truth: not restated)
        self.api_detection_results = None                        # (a DataFrame: not restated)
        self.api_other_fields = None                             # (not restated)
        self.include_almost_detections = False
        self.almost_detection_confidence_threshold = None        #: None: confidence_threshold - 0.05, floored at 0
        self.parallelize_rendering = True
        self.parallelize_rendering_n_cores = 8
        self.parallelize_rendering_with_threads = True
        self.sort_classification_results_by_count = False
        self.category_name_to_sort_weight = {}
        self.max_figures_per_html_file = 1000
        self.footer_text = ''
        self.output_html_encoding = None
        self.additional_image_fields_to_display = None           #: a list of fields, or field -> display name
        self.include_classification_category_report = True
        self.include_category_descriptions_with_global_counts = False
        self.include_size_range = False


class PostProcessingResults:
    """What process_batch_results returns: output_html_file, and counts (process_batch_results says which)."""

    def __init__(self):
        self.output_html_file = ''
        self.counts = {}
        self.api_detection_results = None                        # (the reference's DataFrame: never set here)
        self.api_other_fields = None                             #: what the results file holds beside 'images'


DS_NEGATIVE, DS_POSITIVE, DS_ALMOST = 0, 1, 5                    # DetectionStatus :285-310, the values this path uses


# ---- the reference's small helpers -----------------------------------------------------------------------------------------------

def get_max_conf(im):
    """utils/ct_utils.py get_max_conf"""
    max_conf = 0.0
    if 'detections' in im and im['detections'] is not None and len(im['detections']) > 0:
        max_conf = max([det['conf'] for det in im['detections']])
    return max_conf


def is_missing(value):
    """what DataFrame.isna says of a cell"""
    return value is None or (isinstance(value, float) and math.isnan(value))


def is_url(s):
    return isinstance(s, str) and s.startswith(('http://', 'https://'))


# ---- loading ---------------------------------------------------------------------------------------------------------------------

_ABSENT = object()


def _as_column(values):
    """The values of one field over all images (_ABSENT where an image lacks it) as a DataFrame column holds them: where every
    value that is there is a number and one of them is a float, or some image lacks the field or holds None, the column is
    one of floats -- 3 reads as 3.0 -- and a missing cell is NaN; any other column keeps its objects, a missing cell being
    NaN too and a None staying None."""
    present = [v for v in values if v is not _ABSENT and v is not None]
    numeric = len(present) > 0 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in present)
    if numeric and (len(present) < len(values) or any(isinstance(v, float) for v in present)):
        return [MISSING if (v is _ABSENT or v is None) else float(v) for v in values]
    return [MISSING if v is _ABSENT else v for v in values]


def load_api_results(api_output_path, filename_replacements=None):
    """
    postprocessing/load_api_results.py load_api_results(path, force_forward_slashes=True, filename_replacements=...) without
    the DataFrame.  -> (rows, other_fields): rows, the image entries in file order as dicts that all hold every field any
    image holds (a field an image lacks reads as MISSING); other_fields, what the file holds beside 'images'.
    """
    print('Loading results from {}'.format(api_output_path))
    with open(api_output_path, 'r') as f:
        detection_results = json.load(f)
    if 'predictions' in detection_results:
        raise NotImplementedError('a SpeciesNet predictions file is not converted')
    assert 'images' in detection_results, 'Detector output file should be a json file with an "images" field.'
    for s in ['info', 'detection_categories', 'images']:
        assert s in detection_results, 'Missing field {} in detection results'.format(s)
    other_fields = {k: v for k, v in detection_results.items() if k != 'images'}
    images = detection_results['images']
    for image in images:
        image['file'] = os.path.normpath(image['file'])
    for image in images:
        image['file'] = image['file'].replace('\\', '/')
    if filename_replacements is not None:
        for string_to_replace in filename_replacements.keys():
            replacement_string = filename_replacements[string_to_replace]
            for im in images:
                im['file'] = im['file'].replace(string_to_replace, replacement_string)
    print('Converting results to dataframe')
    for im in images:
        if 'max_detection_conf' not in im:
            im['max_detection_conf'] = get_max_conf(im)
    fields = []
    for im in images:
        for k in im:
            if k not in fields:
                fields.append(k)
    columns = {k: _as_column([im.get(k, _ABSENT) for im in images]) for k in fields}
    rows = [{k: columns[k][i] for k in fields} for i in range(len(images))]
    print('Finished loading MegaDetector results for {} images from {}'.format(len(rows), api_output_path))
    return rows, other_fields


# ---- thresholds ------------------------------------------------------------------------------------------------------------------

def get_threshold_for_category_name(category_name, options):
    """:666-685"""
    if isinstance(options.confidence_threshold, float):
        return options.confidence_threshold
    else:
        assert isinstance(options.confidence_threshold, dict), 'confidence_threshold must either be a float or a dict'
    if category_name in options.confidence_threshold:
        return options.confidence_threshold[category_name]
    else:
        assert 'default' in options.confidence_threshold, \
            'category {} not in confidence_threshold dict, and no default supplied'.format(category_name)
        return options.confidence_threshold['default']


def get_threshold_for_category_id(category_id, options, detection_categories):
    """:688-703"""
    if isinstance(options.confidence_threshold, float):
        return options.confidence_threshold
    assert category_id in detection_categories, 'Invalid category ID {}'.format(category_id)
    return get_threshold_for_category_name(detection_categories[category_id], options)


def get_positive_detections(detections, options, detection_categories):
    """:721-731"""
    return [d for d in detections if d['conf'] >= get_threshold_for_category_id(d['category'], options, detection_categories)]


def get_positive_categories(detections, options, detection_categories):
    """:706-718: the sorted category ids above their thresholds"""
    return sorted(set(d['category'] for d in get_positive_detections(detections, options, detection_categories)))


def has_positive_detection(detections, options, detection_categories):
    """:734-746"""
    for d in detections:
        if d['conf'] >= get_threshold_for_category_id(d['category'], options, detection_categories):
            return True
    return False


def resolve_thresholds(options, other_fields):
    """:1134-1148, written into `options` as the reference writes them"""
    if options.confidence_threshold is None:
        options.confidence_threshold = get_typical_confidence_threshold_from_results(other_fields)
        print('Choosing default confidence threshold of {} based on MD version'.format(options.confidence_threshold))
    if options.almost_detection_confidence_threshold is None and options.include_almost_detections:
        assert isinstance(options.confidence_threshold, float), \
            'If you are using a dictionary of confidence thresholds and almost-detections are enabled, ' + \
            'you need to supply a threshold for almost detections.'
        options.almost_detection_confidence_threshold = options.confidence_threshold - 0.05
        if options.almost_detection_confidence_threshold < 0:
            options.almost_detection_confidence_threshold = 0


def rendering_confidence_threshold(detections, options, detection_categories):
    """:527-537: the float, or category id -> threshold for the categories the image's detections have"""
    if isinstance(options.confidence_threshold, float):
        return options.confidence_threshold
    category_ids = set()
    for d in detections:
        category_ids.add(d['category'])
    return {category_id: get_threshold_for_category_id(category_id, options, detection_categories) for category_id in category_ids}


# ---- the sample and the result sets ------------------------------------------------------------------------------------------------

def sample_indices(n_rows, num_images_to_sample, sample_seed):
    """:1239-1242: the rows DataFrame.sample(n=min(n, N), random_state=seed) takes, in its order; every row in file order
    for a number that is None or not positive"""
    if (num_images_to_sample is not None) and (num_images_to_sample > 0):
        n = min(num_images_to_sample, n_rows)
        return [int(i) for i in np.random.RandomState(sample_seed).choice(n_rows, size=n, replace=False)]
    return list(range(n_rows))


def result_sets(sample, options, detection_categories):
    """
    :1707-1760: -> (images_html, detection_categories_to_results_name, detection_categories_to_category_count): the result
    sets in the order the reference creates them (a defaultdict of lists), the set of every combination of category ids the
    SAMPLE uses, and how many categories each set stands for.
    """
    images_html = collections.defaultdict(list)
    detection_categories_to_results_name = {}
    detection_categories_to_category_count = {}
    images_html['non_detections']
    detection_categories_to_category_count['non_detections'] = 0
    if not options.separate_detections_by_category:
        images_html['detections']
        detection_categories_to_category_count['detections'] = 0
    else:
        used_combinations = []                                   # (a set there: only the order of creation depends on it)
        for row in sample:
            above = set()
            for detection in row['detections']:
                threshold = get_threshold_for_category_id(detection['category'], options, detection_categories)
                if detection['conf'] >= threshold:
                    above.add(detection['category'])
            if len(above) == 0:
                continue
            combination = tuple(sorted(above))
            if combination not in used_combinations:
                used_combinations.append(combination)
        for sorted_subset in used_combinations:
            results_name = 'detections'
            for category_id in sorted_subset:
                results_name = results_name + '_' + detection_categories[category_id]
            images_html[results_name]
            detection_categories_to_results_name[sorted_subset] = results_name
            detection_categories_to_category_count[results_name] = len(sorted_subset)
    if options.include_almost_detections:
        images_html['almost_detections']
        detection_categories_to_category_count['almost_detections'] = 0
    return images_html, detection_categories_to_results_name, detection_categories_to_category_count


# ---- the decision per image --------------------------------------------------------------------------------------------------------

def decide_image(file_info, detection_categories_to_results_name, detection_categories, classification_categories, options):
    """
    _render_image_no_gt :778-947 without the rendering, a pure function of the entry and the options: -> {'file',
    'detections', 'status', 'category_string', 'title', 'rendering_options' (the options with the almost-detection threshold
    as confidence_threshold for an almost-detection), 'class_strings' (the class pages the image is listed on, each once, in
    the order of its detections) and 'max_conf' of its entry}.
    """
    image_relative_path = file_info['file']
    max_conf = file_info['max_detection_conf']
    detections = file_info['detections']
    found_positive_detection = has_positive_detection(detections, options, detection_categories)
    if found_positive_detection:
        detection_status = DS_POSITIVE
    else:
        if options.include_almost_detections:
            if max_conf >= options.almost_detection_confidence_threshold:
                detection_status = DS_ALMOST
            else:
                detection_status = DS_NEGATIVE
        else:
            detection_status = DS_NEGATIVE
    if detection_status == DS_POSITIVE:
        if options.separate_detections_by_category:
            positive_categories = tuple(get_positive_categories(detections, options, detection_categories))
            if positive_categories not in detection_categories_to_results_name:
                raise ValueError('Error: {} not in category mapping (file {})'.format(str(positive_categories), image_relative_path))
            category_string = detection_categories_to_results_name[positive_categories]
        else:
            category_string = 'detections'
    elif detection_status == DS_NEGATIVE:
        category_string = 'non_detections'
    else:
        category_string = 'almost_detections'
    display_name = '<b>Result type</b>: {}, <b>image</b>: {}, <b>max conf</b>: {:0.2f}'.format(
        category_string, image_relative_path, max_conf)
    if options.include_size_range:
        min_size = None
        max_size = None
        for d in get_positive_detections(detections, options, detection_categories):
            assert 'bbox' in d
            assert len(d['bbox']) >= 4
            assert d['bbox'][2] > 0
            assert d['bbox'][3] > 0
            normalized_size = d['bbox'][2] * d['bbox'][3]
            if (min_size is None) or (normalized_size < min_size):
                min_size = normalized_size
            if (max_size is None) or (normalized_size > max_size):
                max_size = normalized_size
        if min_size is None:
            display_name += ' (no size range)'
        else:
            display_name += ' (size min/max: {:0.4f},{:0.4f})'.format(min_size, max_size)
    if options.additional_image_fields_to_display is not None:
        for field_name in options.additional_image_fields_to_display:
            if field_name in file_info:
                field_value = file_info[field_name]
                if is_missing(field_value):
                    continue
                if isinstance(options.additional_image_fields_to_display, dict):
                    field_display_name = options.additional_image_fields_to_display[field_name]
                else:
                    field_display_name = field_name
                display_name += ', {}'.format('<b>{}</b>: {}'.format(field_display_name, field_value))
    rendering_options = copy.copy(options)
    if detection_status == DS_ALMOST:
        rendering_options.confidence_threshold = rendering_options.almost_detection_confidence_threshold
    # :896-943 (what follows the rendering there; nothing of it depends on the rendered file)
    class_strings = []
    entry_max_conf = 0
    for det in detections:
        if det['conf'] > entry_max_conf:
            entry_max_conf = det['conf']
        detection_threshold = get_threshold_for_category_id(det['category'], options, detection_categories)
        if det['conf'] < detection_threshold:
            continue
        if ('classifications' in det) and (len(det['classifications']) > 0) and (category_string != 'non_detections'):
            classifications = det['classifications']
            top1_class_id = classifications[0][0]
            if str(top1_class_id) in classification_categories:
                top1_class_id = str(top1_class_id)
            if top1_class_id not in classification_categories:
                print('Warning: no classification category for ID {}'.format(top1_class_id))
                top1_class_name = str(top1_class_id)
            else:
                top1_class_name = str(classification_categories[top1_class_id])
            top1_class_score = classifications[0][1]
            if (options.classification_confidence_threshold < 0) or (top1_class_score >= options.classification_confidence_threshold):
                class_string = 'class_{}'.format(top1_class_name)
            else:
                class_string = 'class_unreliable'
            if class_string not in class_strings:
                class_strings.append(class_string)
    return {'file': image_relative_path, 'detections': detections, 'status': detection_status, 'category_string': category_string,
            'title': display_name, 'rendering_options': rendering_options, 'class_strings': class_strings, 'max_conf': entry_max_conf}


TEXT_STYLE = 'font-family:verdana,arial,calibri;font-size:80%;text-align:left;margin-top:20;margin-bottom:5'


def sample_name_of(decision):
    """:485/:504: the flat file name of an image within its result set's folder"""
    return decision['category_string'] + '_' + flatten_path(decision['file'])


def html_info(decision, sample_name, options):
    """:563-584: the entry of one image for write_html_image_list"""
    bypassed = decision['category_string'] in options.rendering_bypass_sets
    info = {'filename': '{}/{}'.format(decision['category_string'], sample_name), 'title': decision['title'], 'textStyle': TEXT_STYLE}
    if options.link_images_to_originals and not bypassed:
        info['linkTarget'] = os.path.join(options.image_base_dir, decision['file'])
    return info


# ---- rendering: the host leg -------------------------------------------------------------------------------------------------------

def draw_arguments(decision, detection_categories, classification_categories):
    """What render_detection_bounding_boxes is called with at :540-547, as preview.render_plan and preview.render_with_pil
    take it: -> (PreviewOptions, keyword arguments)"""
    options = decision['rendering_options']
    threshold = rendering_confidence_threshold(decision['detections'], options, detection_categories)
    o = PV.PreviewOptions(confidence_threshold=0, output_image_width=None, box_thickness=options.line_thickness,
                          box_expansion=options.box_expansion)
    by_category = None
    if isinstance(threshold, dict):
        by_category = threshold
    else:
        o.confidence_threshold = threshold
    return o, dict(label_map=detection_categories, labels=True, classification_label_map=classification_categories,
                   classification_confidence_threshold=options.classification_confidence_threshold, category_thresholds=by_category)


def _save(save, output_dir, category_string, sample_name):
    """:549-559: save(path), and once more under a uuid4 name where the name is too long.  -> the name used"""
    fullpath = os.path.join(output_dir, category_string, sample_name)
    try:
        save(fullpath)
    except OSError as e:
        if (e.errno == errno.ENAMETOOLONG) or (len(fullpath) >= 259):
            extension = os.path.splitext(sample_name)[1]
            sample_name = category_string + '_' + str(uuid.uuid4()) + extension
            save(os.path.join(output_dir, category_string, sample_name))
        else:
            raise
    return sample_name


def render_host(decision, detection_categories, classification_categories, options):
    """_render_bounding_boxes :489-559 by the reference's own PIL calls: the host leg of one image that is not bypassed.
    -> (the sample name, whether the image opened)"""
    image_full_path = os.path.join(options.image_base_dir, decision['file'])
    try:
        image = open_image(image_full_path)
    except Exception as e:
        print('Warning: could not open image file {}: {}'.format(image_full_path, str(e)))
        image = None
    sample_name = sample_name_of(decision)
    if image is None:
        return sample_name, False
    rendering_options = decision['rendering_options']
    if rendering_options.viz_target_width is not None:
        from PIL import Image
        size = resized_size(image.size[0], image.size[1], rendering_options.viz_target_width)
        if size != tuple(image.size):
            image = image.resize(size, Image.Resampling.LANCZOS)
    o, kw = draw_arguments(decision, detection_categories, classification_categories)
    PV.render_with_pil(image, decision['detections'], o, **kw)
    return _save(image.save, options.output_dir, decision['category_string'], sample_name), True


def _map(function, items, options, threads_only=False):
    """the reference's loop :1785-1825: serial, or its pool of threads or processes"""
    if not options.parallelize_rendering:
        return [function(item) for item in items]
    threads = options.parallelize_rendering_with_threads or threads_only
    n = options.parallelize_rendering_n_cores
    if n is not None:
        print('Rendering images with {} {}'.format(n, 'threads' if threads else 'processes'))
    return DR.pool_map(function, items, n, threads)


# ---- rendering: the device leg -----------------------------------------------------------------------------------------------------

def _plan_job(decision, detection_categories, classification_categories, options):
    """What the device needs for one image before any pixel is decoded: -> the job; raises preview.HostLeg, or whatever
    planning raises (the host leg then does what the reference does with it)."""
    from .device_decode import plan_source
    sample_name = sample_name_of(decision)
    p, target = plan_source(os.path.join(options.image_base_dir, decision['file']), sample_name,
                            decision['rendering_options'].viz_target_width)
    o, kw = draw_arguments(decision, detection_categories, classification_categories)
    try:
        plan = PV.render_plan(decision['detections'], target[0], target[1], o, **kw)
    except PV.RenderFailure as e:
        raise PV.HostLeg(str(e))
    return {'decision': decision, 'file': decision['file'], 'sample_name': sample_name, 'probe': p, 'source_size': p['size'],
            'size': target, 'plan': plan}


def _render_chunk_device(ctx, torch, device, jobs, clock, options, counts):
    """The images of one chunk, by the device render path.  -> the decisions the host leg has to render"""
    jobs, tensors, host, _ = DR.decode_front(ctx, torch, device, jobs, options.image_base_dir, counts, clock)

    def write(job, data):
        decision = job['decision']
        decision['sample_name'] = _save(partial(DR.write_bytes, data=data), options.output_dir, decision['category_string'], job['sample_name'])

    if jobs:
        DR.render_jobs(ctx, torch, device, jobs, tensors, counts, clock, partial(DR.encode_whole, ctx, clock, SAVE_QUALITY), write)
    return [j['decision'] for j in host]


def _render_device(decisions, detection_categories, classification_categories, options, ctx, counts, profile):
    """-> the decisions that go to the host leg, in their order"""
    import torch
    planned, host = DR.plan_each(decisions, lambda d: _plan_job(d, detection_categories, classification_categories, options))
    place = {id(d): i for i, d in enumerate(decisions)}
    return DR.run_chunks(ctx, torch, planned, DR.job_bytes, partial(_render_chunk_device, options=options, counts=counts), counts,
                         profile, host, DR.file_twice, lambda job: [job['decision']], lambda d: place[id(d)])


# ---- the HTML ----------------------------------------------------------------------------------------------------------------------

def write_html_image_list(filename, images, options):
    """utils/write_html_image_list.py with the options it is given here (pageTitle, headerHtml, maxFiguresPerHtmlFile):
    one page, or -- above maxFiguresPerHtmlFile images -- a table of links to pages of that many images each"""
    options = dict(options)
    options.setdefault('subPageHeaderHtml', '')
    options.setdefault('trailerHtml', '')
    default_text_style = 'font-family:calibri,verdana,arial;font-weight:bold;font-size:150%;text-align:left;margin:0px;'
    default_image_style = 'margin:0px;margin-top:5px;margin-bottom:5px;'
    if options.get('maxFiguresPerHtmlFile') is None:
        options['maxFiguresPerHtmlFile'] = math.inf
    for i_image, image_info in enumerate(images):
        if isinstance(image_info, str):
            image_info = {'filename': image_info}
        image_info.setdefault('filename', '')
        image_info.setdefault('imageStyle', default_image_style)
        image_info.setdefault('title', '')
        image_info.setdefault('linkTarget', '')
        image_info.setdefault('textStyle', default_text_style)
        images[i_image] = image_info
    n_images = len(images)
    if n_images > options['maxFiguresPerHtmlFile']:
        starts = list(range(0, n_images, options['maxFiguresPerHtmlFile']))
        assert len(starts) > 1
        with open(filename, 'w') as f_meta:
            title_string = '<title>Index page</title>'
            if len(options['pageTitle']) > 0:
                title_string = '<title>Index page for: {}</title>'.format(options['pageTitle'])
            f_meta.write('<html><head>{}</head><body>\n'.format(title_string))
            f_meta.write(options['headerHtml'])
            f_meta.write('<table border = 0 cellpadding = 2>\n')
            for i_start in starts:
                i_end = i_start + options['maxFiguresPerHtmlFile'] - 1
                if i_end >= n_images:
                    i_end = n_images - 1
                local_filename = insert_before_extension(filename, 'image_{:05d}_{:05d}'.format(i_start, i_end))
                f_meta.write('<tr><td>\n')
                f_meta.write('<p style="padding-bottom:0px;margin-bottom:0px;text-align:left;font-family:segoe ui,calibri,arial;'
                             'font-size:100%;text-decoration:none;font-weight:bold;">')
                f_meta.write('<a href="{}">Figures for images {} through {}</a></p></td></tr>\n'.format(
                    os.path.basename(local_filename), i_start, i_end))
                local_options = dict(options)
                local_options['headerHtml'] = options['subPageHeaderHtml']
                local_options['trailerHtml'] = ''
                write_html_image_list(local_filename, images[i_start:i_end + 1], local_options)
            f_meta.write('</table></body>\n')
            f_meta.write(options['trailerHtml'])
            f_meta.write('</html>\n')
        return
    with open(filename, 'w') as f_html:
        title_string = ''
        if len(options['pageTitle']) > 0:
            title_string = '<title>{}</title>'.format(options['pageTitle'])
        f_html.write('<html><head>{}</head><body>\n'.format(title_string))
        f_html.write(options['headerHtml'])
        for i_image, image in enumerate(images):
            title = image['title'].encode('ascii', 'ignore').decode('ascii')
            name = image['filename'].encode('ascii', 'ignore').decode('ascii')
            name = urllib.parse.quote(name.replace('\\', '/'))
            if len(title) > 0:
                f_html.write('<p style="{}">{}</p>\n'.format(image['textStyle'], title))
            link_target = urllib.parse.quote(image['linkTarget'].replace('\\', '/'), safe=':/')
            if len(link_target) > 0:
                f_html.write('<a href="{}">'.format(link_target))
            f_html.write('<img src="{}" style="{}">\n'.format(name, image['imageStyle']))
            if len(link_target) > 0:
                f_html.write('</a>')
            if i_image != len(images) - 1:
                f_html.write('<br/>')
        f_html.write(options['trailerHtml'])
        f_html.write('</body></html>\n')


def prepare_html_subpages(images_html, output_dir, options):
    """_prepare_html_subpages :589-661: sorts every result set's entries and writes its page.  -> set -> number of images"""
    image_counts = {}
    for category_string, images_this_category in images_html.items():
        image_counts[category_string] = len(images_this_category)
    if options.html_sort_order == 'filename':
        images_html = {k: sorted(v, key=lambda x: x['filename']) for k, v in images_html.items()}
    elif options.html_sort_order == 'confidence':
        images_html_sorted = {}
        rebound = images_html
        for category_string, images_this_category in images_html.items():
            if not all(['max_conf' in d for d in images_this_category]):
                print("Warning: some elements in the {} page don't have confidence values, can't sort by confidence".format(
                    category_string))
            else:
                images_html_sorted[category_string] = sorted(images_this_category, key=lambda x: x['max_conf'], reverse=True)
                rebound = images_html_sorted                     # (as there: only the sets that could be sorted are written)
        images_html = rebound
    else:
        assert options.html_sort_order == 'random', 'Unrecognized sort order {}'.format(options.html_sort_order)
        images_html = {k: random.sample(v, len(v)) for k, v in images_html.items()}
    for category_string, images_this_category in images_html.items():
        if len(images_this_category) == 0:
            continue
        html_image_list_options = {'maxFiguresPerHtmlFile': options.max_figures_per_html_file,
                                   'headerHtml': '<h1>{}</h1>'.format(category_string.upper()),
                                   'pageTitle': '{}'.format(category_string.lower())}
        html_filename_base = clean_filename(category_string, replace_whitespace='_')
        write_html_image_list(os.path.join(output_dir, '{}.html'.format(html_filename_base)), images_this_category,
                              html_image_list_options)
    return image_counts


STYLE_HEADER = """<head>
        <title>Detection results preview</title>
        <style type="text/css">
        a { text-decoration: none; }
        body { font-family: segoe ui, calibri, "trebuchet ms", verdana, arial, sans-serif; }
        div.contentdiv { margin-left: 20px; }
        </style>
        </head>"""


def result_set_name_to_friendly_name(result_set_name):
    friendly_name = result_set_name.replace('_', '-')
    if friendly_name.startswith('detections-'):
        friendly_name = friendly_name.replace('detections-', 'detections: ')
    return friendly_name.capitalize()


def category_count_report(options):
    """:2042-2101: the counts of top-1 classifications over the WHOLE results file, read once more"""
    with open(options.md_results_file, 'r') as f:
        d = json.load(f)
    category_name_to_count = {}
    include_descriptions = options.include_category_descriptions_with_global_counts
    if 'classification_category_descriptions' not in d:
        include_descriptions = False
    else:
        category_name_to_id = {v: k for k, v in d['classification_categories'].items()}
        category_id_to_description = d['classification_category_descriptions']
    for im in d['images']:
        if 'detections' in im and im['detections'] is not None:
            for det in im['detections']:
                if ('classifications' in det) and (len(det['classifications']) > 0):
                    class_id = det['classifications'][0][0]
                    class_conf = det['classifications'][0][1]
                    if class_conf < options.classification_confidence_threshold:
                        continue
                    if str(class_id) in d['classification_categories']:
                        class_id = str(class_id)
                    if class_id not in d['classification_categories']:
                        print('Warning: no category name for ID {}'.format(class_id))
                        category_name = str(class_id)
                    else:
                        category_name = d['classification_categories'][class_id]
                    category_name_to_count[category_name] = category_name_to_count.get(category_name, 0) + 1
    category_name_to_count = {k: v for k, v in sorted(category_name_to_count.items(), key=lambda item: item[1], reverse=True)}
    footer = ''
    footer += '<br/>\n'
    footer += '<h3>Category counts (for the whole dataset, not just the sample used for this page)</h3>\n'
    footer += '<div class="contentdiv">\n'
    for category_name in category_name_to_count.keys():
        category_count_html = '{}: {}'.format(category_name, category_name_to_count[category_name])
        if include_descriptions:
            category_count_html += ' ({})'.format(category_id_to_description[category_name_to_id[category_name]])
        category_count_html += '<br/>\n'
        footer += category_count_html
    footer += '</div>\n'
    return footer


def index_page_text(options, images_html, image_counts, detection_categories_to_category_count, classification_categories,
                    has_classification_info, image_count, n_rows, n_failures, job_name_string, model_version_string):
    """:1856-2115: the text of index.html, character for character"""
    total_images = 0
    for k in image_counts.keys():
        v = image_counts[k]
        if has_classification_info and k.startswith('class_'):
            continue
        total_images += v
    if total_images != image_count:
        print('Warning, missing images: image_count is {}, total_images is {}'.format(total_images, image_count))
    almost_detection_string = ''
    if options.include_almost_detections:
        almost_detection_string = ' (&ldquo;almost detection&rdquo; threshold at {:.1%})'.format(
            options.almost_detection_confidence_threshold)
    if isinstance(options.confidence_threshold, float):
        confidence_threshold_string = '{:.2%}'.format(options.confidence_threshold)
    else:
        confidence_threshold_string = str(options.confidence_threshold)
    index_page = """<html>\n{}\n<body>\n
        <h2>Visualization of results for {}</h2>\n
        <p>A sample of {} images (of {} total)FAILURE_PLACEHOLDER, annotated with detections above confidence {}{}.</p>\n

        <div class="contentdiv">
        <p>Model version: {}</p>
        </div>

        <h3>Detection results</h3>\n
        <div class="contentdiv">\n""".format(
        STYLE_HEADER, job_name_string, image_count, n_rows, confidence_threshold_string, almost_detection_string, model_version_string)
    failure_string = ''
    if n_failures is not None:
        failure_string = ' ({} failures)'.format(n_failures)
    index_page = index_page.replace('FAILURE_PLACEHOLDER', failure_string)
    sorted_result_set_names = sorted(list(images_html.keys()))
    result_set_name_to_count = {name: image_counts[name] for name in sorted_result_set_names}
    sorted_result_set_names = sorted(sorted_result_set_names, key=lambda x: result_set_name_to_count[x], reverse=True)
    for result_set_name in sorted_result_set_names:
        if has_classification_info and result_set_name.lower().startswith('class_'):
            continue
        filename = result_set_name + '.html'
        label = result_set_name_to_friendly_name(result_set_name)
        image_count = image_counts[result_set_name]
        if image_count == 0 and detection_categories_to_category_count[result_set_name] > 1:
            continue
        if total_images == 0:
            image_fraction = -1
        else:
            image_fraction = image_count / total_images
        if image_count == 0:
            index_page += '{} ({}, {:.1%})<br/>\n'.format(label, image_count, image_fraction)
        else:
            index_page += '<a href="{}">{}</a> ({}, {:.1%})<br/>\n'.format(filename, label, image_count, image_fraction)
    index_page += '</div>\n'
    category_count_footer = None
    if has_classification_info:
        index_page += '<h3>Species classification results</h3>'
        index_page += '<p>The same image might appear under multiple classes ' + 'if multiple species were detected.</p>\n'
        index_page += '<p>Classifications with confidence less than {:.1%} confidence are considered "unreliable".</p>\n'.format(
            options.classification_confidence_threshold)
        index_page += '<div class="contentdiv">\n'
        class_names = sorted(classification_categories.values())
        if 'class_unreliable' in images_html.keys():
            class_names.append('unreliable')
        if options.sort_classification_results_by_count:
            class_name_to_count = {}
            for cname in class_names:
                class_name_to_count[cname] = len(images_html['class_{}'.format(cname)])
            class_names = sorted(class_names, key=lambda x: class_name_to_count[x], reverse=True)
        # :1976-1983 as it is written there: the weights are checked to be integers only when the option is None -- and then
        # the loop over None raises TypeError; a dict that is given is used below without that check
        if options.category_name_to_sort_weight is not None:
            category_name_to_sort_weight = {}
        else:
            category_name_to_sort_weight = options.category_name_to_sort_weight
            for category_name in category_name_to_sort_weight:
                assert isinstance(category_name_to_sort_weight[category_name], int), \
                    'Illegal sort weight {} for category {}'.format(category_name_to_sort_weight[category_name], category_name)
        sort_weight_to_class_names = defaultdict(list)
        for class_name in class_names:
            if class_name in options.category_name_to_sort_weight:
                sort_weight_to_class_names[options.category_name_to_sort_weight[class_name]].append(class_name)
            else:
                sort_weight_to_class_names[0].append(class_name)
        sort_weight_to_class_names = dict(sorted(sort_weight_to_class_names.items()))
        category_names_printed = set()
        for i_weight, sort_weight in enumerate(sort_weight_to_class_names):
            for cname in sort_weight_to_class_names[sort_weight]:
                if cname in category_names_printed:
                    continue
                category_names_printed.add(cname)
                ccount = len(images_html['class_{}'.format(cname)])
                if ccount > 0:
                    html_filename_base = clean_filename('class_{}'.format(cname), replace_whitespace='_')
                    cname_print_string = cname.lower()
                    if len(cname_print_string) == 0:
                        cname_print_string = '[no name available]'
                    index_page += '<a href="{}.html">{}</a> ({})<br/>\n'.format(html_filename_base, cname_print_string, ccount)
            if i_weight != (len(sort_weight_to_class_names) - 1):
                index_page += '<br/>\n'
        index_page += '</div>\n'
        if options.include_classification_category_report:
            print('Generating classification category report')
            category_count_footer = category_count_report(options)
    if category_count_footer is not None:
        index_page += category_count_footer + '\n'
    if (options.footer_text is not None) and (len(options.footer_text) > 0):
        index_page += options.footer_text + '\n'
    index_page += '\n</body></html>\n'
    return index_page


# ---- the entry function ------------------------------------------------------------------------------------------------------------

COUNT_KEYS = ('sampled', 'rendered', 'gpu', 'host', 'unopened', 'bypassed', 'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks',
              'resample_calls', 'draw_calls', 'encode_calls')


def check_restated(options):
    """what this module does not restate: NotImplementedError, before anything is read or written"""
    if (options.ground_truth_json_file is not None) and (len(options.ground_truth_json_file) > 0):
        raise NotImplementedError('ground truth (ground_truth_json_file, the tp/fp/tn/fn sets, the precision-recall figures) is not restated')
    if is_url(options.image_base_dir):
        raise NotImplementedError('an image_base_dir that is a URL is not restated')
    if (options.api_detection_results is not None) or (options.api_other_fields is not None):
        raise NotImplementedError('api_detection_results and api_other_fields (DataFrames) are not restated')


def decide_sample(options):
    """
    :1118-1242 and :1707-1760, and decide_image for every sampled image: everything process_batch_results decides before a
    pixel is touched, as a dict -- 'rows' (the images that did not fail), 'other_fields', 'n_failures', the category maps, the
    'sample' in its order, the result sets ('images_html', 'results_names', 'category_counts'), the header strings and the
    'decisions'.  Writes the thresholds into `options` as the reference does; touches no file but the results file.
    """
    rows, other_fields = load_api_results(options.md_results_file, filename_replacements=options.api_output_filename_replacements)
    resolve_thresholds(options, other_fields)
    n_failures = 0
    if rows and 'failure' in rows[0]:
        n_failures = sum(1 for row in rows if not is_missing(row['failure']))
        print('Ignoring {} failed images'.format(n_failures))
        rows = [row for row in rows if is_missing(row['failure'])]
    detection_categories = other_fields['detection_categories']
    classification_categories = other_fields.get('classification_categories', {})
    if classification_categories is not None:
        classification_categories = {k.lower(): v.lower() for k, v in classification_categories.items()}
    n_positives = 0
    n_almosts = 0
    print('Assigning images to rendering categories')
    for row in rows:
        if has_positive_detection(row['detections'], options, detection_categories):
            n_positives += 1
        elif (options.almost_detection_confidence_threshold is not None) and \
                (row['max_detection_conf'] >= options.almost_detection_confidence_threshold):
            n_almosts += 1
    print('Finished loading and preprocessing {} rows from detector output, predicted {} positives.'.format(len(rows), n_positives))
    if options.include_almost_detections:
        print('...and {} almost-positives'.format(n_almosts))
    if options.job_name_string is not None:
        job_name_string = options.job_name_string
    else:
        job_name_string = 'unknown' if options.md_results_file is None else os.path.basename(options.md_results_file)
    if options.model_version_string is not None:
        model_version_string = options.model_version_string
    elif 'info' not in other_fields or 'detector' not in other_fields['info']:
        print('No model metadata supplied, assuming MDv5a')
        model_version_string = 'MDv5a (assumed)'
    else:
        model_version_string = other_fields['info']['detector']
    sample = [rows[i] for i in sample_indices(len(rows), options.num_images_to_sample, options.sample_seed)]
    images_html, results_names, category_counts = result_sets(sample, options, detection_categories)
    for row in sample:
        assert isinstance(row['detections'], list)
    decisions = [decide_image(row, results_names, detection_categories, classification_categories, options) for row in sample]
    return {'rows': rows, 'other_fields': other_fields, 'n_failures': n_failures, 'detection_categories': detection_categories,
            'classification_categories': classification_categories, 'sample': sample, 'images_html': images_html,
            'results_names': results_names, 'category_counts': category_counts, 'job_name_string': job_name_string,
            'model_version_string': model_version_string, 'decisions': decisions}


def process_batch_results(options, backend='gpu', device=0, profile=False):
    """
    The reference's process_batch_results(options) without ground truth.  backend 'host': PIL, no GPU; 'gpu': the rendering on
    HIP device `device`, on a context without a model made for the call.  profile: also counts['ms'], the milliseconds around
    the decode, resample, draw and encode calls (the device is waited for around each: slower).
    Returns PostProcessingResults: output_html_file, and counts -- 'sampled' images, of which 'rendered' (a file was written:
    'gpu' on the device, 'host' by PIL), 'unopened' (a warning, no file, listed all the same) and 'bypassed'
    (rendering_bypass_sets); 'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks', 'resample_calls', 'draw_calls',
    'encode_calls' of the device leg.
    """
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    check_restated(options)
    ppresults = PostProcessingResults()
    output_dir = options.output_dir
    os.makedirs(output_dir, exist_ok=True)
    d = decide_sample(options)
    ppresults.api_other_fields = d['other_fields']
    rows, sample, decisions, images_html = d['rows'], d['sample'], d['decisions'], d['images_html']
    detection_categories, classification_categories = d['detection_categories'], d['classification_categories']
    for res in images_html.keys():
        os.makedirs(os.path.join(output_dir, res), exist_ok=True)
    image_count = len(sample)
    counts = {k: 0 for k in COUNT_KEYS}
    counts['sampled'] = image_count
    if profile:
        counts['ms'] = {}
    to_render = []
    for decision in decisions:
        decision['sample_name'] = sample_name_of(decision)
        if decision['category_string'] in options.rendering_bypass_sets:
            counts['bypassed'] += 1
        else:
            to_render.append(decision)
    host = to_render
    if backend == 'gpu' and to_render:
        from .hip_backend import HipContext
        with HipContext.images_or(None, device) as ctx:
            host = _render_device(to_render, detection_categories, classification_categories, options, ctx, counts, profile)
    render = partial(render_host, detection_categories=detection_categories,
                     classification_categories=classification_categories, options=options)
    for decision, (sample_name, opened) in zip(host, _map(render, host, options, threads_only=backend == 'gpu')):
        decision['sample_name'] = sample_name
        counts['host' if opened else 'unopened'] += 1
    counts['rendered'] = counts['gpu'] + counts['host']
    has_classification_info = False
    image_rendered_count = 0
    for decision in decisions:
        info = html_info(decision, decision['sample_name'], options)
        image_rendered_count += 1
        info['max_conf'] = decision['max_conf']
        for result_set in [decision['category_string']] + decision['class_strings']:
            if 'class' in result_set:
                has_classification_info = True
            images_html[result_set].append(info)
    image_counts = prepare_html_subpages(images_html, output_dir, options)
    print('Rendered {} images (of {})'.format(image_rendered_count, image_count))
    index_page = index_page_text(options, images_html, image_counts, d['category_counts'], classification_categories,
                                 has_classification_info, image_count, len(rows), d['n_failures'], d['job_name_string'],
                                 d['model_version_string'])
    output_html_file = os.path.join(output_dir, 'index.html')
    with open(output_html_file, 'w', encoding=options.output_html_encoding) as f:
        f.write(index_page)
    print('Finished writing html to {}'.format(output_html_file))
    ppresults.output_html_file = output_html_file
    ppresults.counts = counts
    return ppresults


# ---- command line --------------------------------------------------------------------------------------------------------------------

def options_from_arguments(argv):
    """main() :2153-2235: the arguments as the reference maps them onto the options (every argument becomes an attribute of
    that name, as args_to_object does it).  -> (options, backend, device)"""
    options = PostProcessingOptions()
    parser = argparse.ArgumentParser(description='Sample images from a results file and render them to HTML pages')
    parser.add_argument('md_results_file', help='path to .json file containing MegaDetector results')
    parser.add_argument('output_dir', help='base directory for output')
    parser.add_argument('--image_base_dir', default=options.image_base_dir, help='base directory for images')
    parser.add_argument('--ground_truth_json_file', default=options.ground_truth_json_file, help='ground truth labels (not restated)')
    parser.add_argument('--confidence_threshold', type=float, default=options.confidence_threshold,
                        help='Confidence threshold for statistics and visualization')
    parser.add_argument('--almost_detection_confidence_threshold', type=float, default=options.almost_detection_confidence_threshold,
                        help='Almost-detection confidence threshold for statistics and visualization')
    parser.add_argument('--target_recall', type=float, default=options.target_recall, help='Target recall (for statistics only)')
    parser.add_argument('--num_images_to_sample', type=int, default=options.num_images_to_sample,
                        help='number of images to visualize, -1 for all images')
    parser.add_argument('--viz_target_width', type=int, default=options.viz_target_width, help='Output image width')
    parser.add_argument('--include_almost_detections', action='store_true',
                        help='Include a separate category for images just above a second confidence threshold')
    parser.add_argument('--html_sort_order', type=str, default='filename',
                        help='Sort order for output pages, should be one of [filename,confidence,random] (defaults to filename)')
    parser.add_argument('--sort_by_confidence', action='store_true',
                        help='(accepted as by the reference, which does not read it: use --html_sort_order confidence)')
    parser.add_argument('--n_cores', type=int, default=4, help='Number of threads to use for rendering (default: 4)')
    parser.add_argument('--parallelize_rendering_with_processes', action='store_true',
                        help='Should we use processes (instead of threads) for parallelization?')
    parser.add_argument('--no_separate_detections_by_category', action='store_true',
                        help='Collapse all categories into just "detections" and "non-detections"')
    parser.add_argument('--open_output_file', action='store_true', help='(accepted and ignored)')
    parser.add_argument('--max_figures_per_html_file', type=int, default=None, help='Maximum number of images to put on a single HTML page')
    parser.add_argument('--backend', choices=('host', 'gpu'), default='gpu', help="'host': the reference's PIL calls, no GPU needed")
    parser.add_argument('--device', type=int, default=0, help='HIP device of the gpu backend')
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    backend, device = args.backend, args.device
    del args.backend, args.device
    if args.n_cores != 1:
        assert (args.n_cores > 1), 'Illegal number of cores: {}'.format(args.n_cores)
        if args.parallelize_rendering_with_processes:
            args.parallelize_rendering_with_threads = False
        args.parallelize_rendering = True
        args.parallelize_rendering_n_cores = args.n_cores
    for n, v in vars(args).items():
        if not n.startswith('_'):
            setattr(options, n, v)
    if args.no_separate_detections_by_category:
        options.separate_detections_by_category = False
    return options, backend, device


def main(argv=None):
    options, backend, device = options_from_arguments(sys.argv[1:] if argv is None else argv)
    ppresults = process_batch_results(options, backend=backend, device=device)
    if options.open_output_file:
        print('--open_output_file is ignored: open {} in a browser'.format(ppresults.output_html_file))
    c = ppresults.counts
    print('Sampled {} images ({})'.format(c['sampled'], ', '.join('{} {}'.format(k, v) for k, v in c.items() if k != 'sampled')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
