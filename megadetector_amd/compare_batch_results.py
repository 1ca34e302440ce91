"""
Compare results files, as the reference's postprocessing/compare_batch_results.py does without ground truth: every pairwise
comparison of the files sorts the images into common_detections, common_non_detections, detections_a_only, detections_b_only
and class_transitions, samples each category, renders every sampled image with the boxes of both files (A: thickness 4,
labels on top; B: thickness 2, labels below) and writes a page per category and an index.html.  Names, defaults, the
sampling (random.seed(options.random_seed) once per comparison, random.sample per category in dict order), the output names
(cmp_000/<category>/<flatten_path(file)>) and the HTML are the reference's, statement for statement.

What is ours is WHERE the images are rendered.  The reference opens, decodes and LANCZOS-resizes a file again for every
comparison it is sampled in.  Here every comparison is decided and sampled first (planning, on the host), which gives a list
of jobs; then

  backend='host'   makes the reference's PIL calls per job (open_image, resize_image, render_detection_bounding_boxes twice,
                   Image.save), on its pool of n_rendering_workers threads or processes;
  backend='gpu'    groups the jobs by source file and renders a decode chunk (device_render.run_chunks) with ONE decode of each
                   file (device_decode.decode_stage), ONE mdhip_resample_lanczos call that makes one resampled image per
                   distinct file, ONE mdhip_draw_ops_from call that makes every job's image from its file's shared image
                   (the plan is A's preview.render_plan, then B's), and ONE mdhip_jpeg_encode call.  A job without any
                   operation needs no image of its own: the encoder reads the shared one.  The host leg takes, per job and
                   counted, a file the device does not decode, an output name Pillow does not map to JPEG, a plan that raises
                   preview.HostLeg (a box thinner than twice its outline: 8 pixels for A, 4 for B) and a chunk whose
                   rendering fails on the device.  Both legs write the same bytes.

Not restated (NotImplementedError before anything is read or written): ground_truth_file and what belongs to it
(gt_iou_threshold, gt_empty_categories, include_clean_categories, the tp/fp/tn/fn categories, the rotated GT labels);
find_equivalent_threshold and find_image_level_detections_above_threshold are not part of this module.

One deliberate difference: with category_names_to_include the reference compares two LISTS built by iterating over sets,
so whether an image with the same categories on both sides is a common detection or a class transition can depend on
string hashing; here the two are compared as sets.
"""

import argparse
import copy
import itertools
import json
import os
import random
import re
import sys
import textwrap
import urllib.parse
from functools import partial

from . import device_render as DR
from . import preview as PV
from .postprocess_batch_results import SAVE_QUALITY, flatten_path, open_image, resized_size, write_html_image_list

THICKNESS_A, THICKNESS_B = 4, 2                  # _render_image_pair: thickness=4 for A, 2 for B
COUNT_KEYS = ('jobs', 'gpu', 'host', 'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks', 'resample_calls', 'draw_calls',
              'encode_calls')


def _maxempty(L):  # noqa
    return 0 if len(L) == 0 else max(L)


class PairwiseBatchComparisonOptions:
    """The options of one pairwise comparison, under the reference's names and with its defaults."""

    def __init__(self):
        self.results_filename_a = None
        self.results_filename_b = None
        self.results_description_a = None
        self.results_description_b = None
        self.detection_thresholds_a = {'animal': 0.15, 'person': 0.15, 'vehicle': 0.15, 'default': 0.15}
        self.detection_thresholds_b = {'animal': 0.15, 'person': 0.15, 'vehicle': 0.15, 'default': 0.15}
        self.rendering_confidence_threshold_a = 0.1
        self.rendering_confidence_threshold_b = 0.1
        self.classification_confidence_threshold_a = 0.3
        self.classification_confidence_threshold_b = 0.3


class BatchComparisonOptions:
    """The options of a set of pairwise comparisons, under the reference's names and with its defaults."""

    def __init__(self):
        self.output_folder = None
        self.image_folder = None
        self.job_name = ''
        self.max_images_per_category = 1000
        self.max_images_per_page = None
        self.colormap_a = ['Red']
        self.colormap_b = ['RoyalBlue']
        self.parallelize_rendering_with_threads = True
        self.filenames_to_include = None
        self.category_names_to_include = None
        self.class_agnostic_comparison = False
        self.target_width = 800
        self.n_rendering_workers = 10
        self.random_seed = 0
        self.sort_by_confidence = False
        self.error_on_non_matching_lists = True
        self.ground_truth_file = None
        self.gt_iou_threshold = 0.5
        self.gt_empty_categories = ['empty', 'blank', 'misfire']
        self.show_labels_for_image_level_gt = True
        self.show_category_names_on_gt_boxes = True
        self.show_category_names_on_detected_boxes = True
        self.show_classification_categories = True
        self.pairwise_options = []
        self.required_token = None
        self.verbose = False
        self.include_clean_categories = True
        self.fn_to_display_fn = None
        self.parse_link_paths = True
        self.include_toc = True
        self.return_images_by_category = False


class PairwiseBatchComparisonResults:
    """The results of one pairwise comparison."""

    def __init__(self):
        self.html_content = None
        self.pairwise_options = None
        self.categories_to_image_pairs = None
        self.comparison_short_name = None
        self.comparison_friendly_name = None


class BatchComparisonResults:
    """The results of a set of pairwise comparisons; counts: the jobs and the legs that rendered them (module docstring)."""

    def __init__(self):
        self.html_output_file = None
        self.pairwise_results = None
        self.counts = None


main_page_style_header = """<head><title>Results comparison</title>
    <style type="text/css">
    a { text-decoration: none; }
    body { font-family: segoe ui, calibri, "trebuchet ms", verdana, arial, sans-serif; }
    div.contentdiv { margin-left: 20px; }
    </style>
    </head>"""

main_page_header = '<html>\n{}\n<body>\n'.format(main_page_style_header)
main_page_footer = '<br/><br/><br/></body></html>\n'

CATEGORIES_TO_PAGE_TITLES = {
    'common_detections': 'Detections common to both models',
    'common_non_detections': 'Non-detections common to both models',
    'detections_a_only': 'Detections reported by model A only',
    'detections_b_only': 'Detections reported by model B only',
    'class_transitions': 'Detections reported as different classes by models A and B'
}


def check_restated(options):
    """what this module does not restate: NotImplementedError, before anything is read or written"""
    if options.ground_truth_file is not None:
        raise NotImplementedError('ground truth (ground_truth_file, gt_iou_threshold, gt_empty_categories, include_clean_categories, '
                                  'the tp/fp/tn/fn categories, the rotated GT labels) is not restated')


# ---- planning: what the reference decides before it renders -----------------------------------------------------------------------

def _subset_md_results(results, options):
    if options.required_token is None:
        return results
    images_to_keep = []
    for im in results['images']:
        if isinstance(options.required_token, str):
            if options.required_token in im['file']:
                images_to_keep.append(im)
        else:
            assert callable(options.required_token), 'Illegal value for required_token'
            if options.required_token(im['file']):
                images_to_keep.append(im)
    if options.verbose:
        print('Keeping {} of {} images in MD results'.format(len(images_to_keep), len(results['images'])))
    results['images'] = images_to_keep
    return results


def _category_thresholds(detection_categories, detection_thresholds):
    out = {}
    for category_id in detection_categories:
        category_name = detection_categories[category_id]
        if category_name in detection_thresholds:
            out[category_id] = detection_thresholds[category_name]
        else:
            out[category_id] = detection_thresholds['default']
    return out


def _categories_above_threshold(im, thresholds, side, fn):
    """the categories with a detection at or above their threshold (>=); None for a detection of an unknown category"""
    above = set()
    for det in im['detections']:
        category_id = det['category']
        if category_id not in thresholds:
            print('Warning: unexpected category {} for model {} on file {}'.format(category_id, side, fn))
            return None
        if det['conf'] >= thresholds[category_id]:
            above.add(category_id)
    return above


def _plan_pairwise(options, output_index, pairwise_options):
    """_pairwise_compare_batch_results up to the rendering: loads, checks, sorts the images into the categories and samples
    them.  -> the plan of the comparison: what its pages and its block of the index need, and its rendering jobs"""
    assert options.pairwise_options is None
    if options.random_seed is not None:
        random.seed(options.random_seed)
    if isinstance(pairwise_options.detection_thresholds_a, float):
        pairwise_options.detection_thresholds_a = {'default': pairwise_options.detection_thresholds_a}
    if isinstance(pairwise_options.detection_thresholds_b, float):
        pairwise_options.detection_thresholds_b = {'default': pairwise_options.detection_thresholds_b}
    max_detection_threshold_a = max(list(pairwise_options.detection_thresholds_a.values()))
    max_detection_threshold_b = max(list(pairwise_options.detection_thresholds_b.values()))
    if pairwise_options.rendering_confidence_threshold_a > max_detection_threshold_a:
        print('*** Warning: rendering threshold A ({}) is higher than max confidence threshold A ({}) ***'.format(
            pairwise_options.rendering_confidence_threshold_a, max_detection_threshold_a))
    if pairwise_options.rendering_confidence_threshold_b > max_detection_threshold_b:
        print('*** Warning: rendering threshold B ({}) is higher than max confidence threshold B ({}) ***'.format(
            pairwise_options.rendering_confidence_threshold_b, max_detection_threshold_b))

    assert os.path.isfile(pairwise_options.results_filename_a), "Can't find results file {}".format(pairwise_options.results_filename_a)
    assert os.path.isfile(pairwise_options.results_filename_b), "Can't find results file {}".format(pairwise_options.results_filename_b)
    assert os.path.isdir(options.image_folder), "Can't find image folder {}".format(options.image_folder)
    os.makedirs(options.output_folder, exist_ok=True)
    if options.category_names_to_include is not None:
        if isinstance(options.category_names_to_include, str):
            options.category_names_to_include = [options.category_names_to_include]

    if options.verbose:
        print('Loading {}'.format(pairwise_options.results_filename_a))
    with open(pairwise_options.results_filename_a, 'r') as f:
        results_a = json.load(f)
    if options.verbose:
        print('Loading {}'.format(pairwise_options.results_filename_b))
    with open(pairwise_options.results_filename_b, 'r') as f:
        results_b = json.load(f)
    for results in (results_a, results_b):
        for im in results['images']:
            if 'file' in im:
                im['file'] = im['file'].replace('\\', '/')
    if not options.class_agnostic_comparison:
        assert results_a['detection_categories'] == results_b['detection_categories'], \
            'Cannot perform a class-sensitive comparison across results with different categories'
    detection_categories_a = results_a['detection_categories']
    detection_categories_b = results_b['detection_categories']
    classification_categories_a = results_a.get('classification_categories', None)
    classification_categories_b = results_b.get('classification_categories', None)
    name_to_id_a = {v: k for k, v in detection_categories_a.items()}
    name_to_id_b = {v: k for k, v in detection_categories_b.items()}
    if options.category_names_to_include is None:
        category_ids_to_include_a = sorted(list(name_to_id_a.values()))
        category_ids_to_include_b = sorted(list(name_to_id_b.values()))
    else:
        category_ids_to_include_a = [name_to_id_a[n] for n in options.category_names_to_include if n in name_to_id_a]
        category_ids_to_include_b = [name_to_id_b[n] for n in options.category_names_to_include if n in name_to_id_b]
    if pairwise_options.results_description_a is None:
        if 'detector' not in results_a['info']:
            print('No model metadata supplied for results-A, assuming MDv4')
            pairwise_options.results_description_a = 'MDv4 (assumed)'
        else:
            pairwise_options.results_description_a = results_a['info']['detector']
    if pairwise_options.results_description_b is None:
        if 'detector' not in results_b['info']:
            print('No model metadata supplied for results-B, assuming MDv4')
            pairwise_options.results_description_b = 'MDv4 (assumed)'
        else:
            pairwise_options.results_description_b = results_b['info']['detector']
    results_a = _subset_md_results(results_a, options)
    results_b = _subset_md_results(results_b, options)
    images_a = results_a['images']
    images_b = results_b['images']
    filename_to_image_a = {im['file']: im for im in images_a}
    filename_to_image_b = {im['file']: im for im in images_b}

    filenames_a = [im['file'] for im in images_a]
    filenames_b_set = set([im['file'] for im in images_b])
    if len(images_a) != len(images_b):
        s = 'set A has {} images, set B has {}'.format(len(images_a), len(images_b))
        if options.error_on_non_matching_lists:
            raise ValueError(s)
        else:
            print('Warning: ' + s)
    else:
        if options.error_on_non_matching_lists:
            for fn in filenames_a:
                assert fn in filenames_b_set
    assert len(filenames_a) == len(images_a)
    assert len(filenames_b_set) == len(images_b)
    if options.filenames_to_include is None:
        filenames_to_compare = filenames_a
    else:
        filenames_to_compare = options.filenames_to_include

    categories_to_image_pairs = {category: {} for category in CATEGORIES_TO_PAGE_TITLES}
    category_id_to_threshold_a = _category_thresholds(detection_categories_a, pairwise_options.detection_thresholds_a)
    category_id_to_threshold_b = _category_thresholds(detection_categories_b, pairwise_options.detection_thresholds_b)
    for fn in filenames_to_compare:
        if fn not in filename_to_image_b:
            assert not options.error_on_non_matching_lists
            print('Skipping filename {}, not in image set B'.format(fn))
            continue
        im_a = filename_to_image_a[fn]
        im_b = filename_to_image_b[fn]
        im_pair = {'im_a': im_a, 'im_b': im_b, 'im_gt': None, 'annotations_gt': None}
        if 'detections' not in im_a or im_a['detections'] is None:
            assert 'failure' in im_a and im_a['failure'] is not None
            continue
        if 'detections' not in im_b or im_b['detections'] is None:
            assert 'failure' in im_b and im_b['failure'] is not None
            continue
        categories_above_threshold_a = _categories_above_threshold(im_a, category_id_to_threshold_a, 'A', fn)
        if categories_above_threshold_a is None:
            continue
        categories_above_threshold_b = _categories_above_threshold(im_b, category_id_to_threshold_b, 'B', fn)
        if categories_above_threshold_b is None:
            continue
        if options.category_names_to_include is not None:
            # (sets, where the reference makes lists in the sets' iteration order: the module docstring)
            categories_above_threshold_a = {c for c in categories_above_threshold_a if c in category_ids_to_include_a}
            categories_above_threshold_b = {c for c in categories_above_threshold_b if c in category_ids_to_include_b}
        detection_a = (len(categories_above_threshold_a) > 0)
        detection_b = (len(categories_above_threshold_b) > 0)
        if detection_a and detection_b:
            if (categories_above_threshold_a == categories_above_threshold_b) or options.class_agnostic_comparison:
                comparison_category = 'common_detections'
            else:
                comparison_category = 'class_transitions'
        elif (not detection_a) and (not detection_b):
            comparison_category = 'common_non_detections'
        elif detection_a and (not detection_b):
            comparison_category = 'detections_a_only'
        else:
            assert detection_b and (not detection_a)
            comparison_category = 'detections_b_only'
        max_conf_a = _maxempty([det['conf'] for det in im_a['detections']])
        max_conf_b = _maxempty([det['conf'] for det in im_b['detections']])
        if comparison_category == 'detections_a_only':
            sort_conf = max_conf_a
        elif comparison_category == 'detections_b_only':
            sort_conf = max_conf_b
        else:
            sort_conf = max(max_conf_a, max_conf_b)
        categories_to_image_pairs[comparison_category][fn] = im_pair
        im_pair['sort_conf'] = sort_conf

    if options.n_rendering_workers > 1:
        print('Rendering images with {} {}'.format(options.n_rendering_workers,
                                                   'threads' if options.parallelize_rendering_with_threads else 'processes'))
    local_output_folder = os.path.join(options.output_folder, 'cmp_' + str(output_index).zfill(3))
    label_map = classification_label_map_a = classification_label_map_b = None
    if options.show_category_names_on_detected_boxes:
        label_map = detection_categories_a
        if options.show_classification_categories:
            classification_label_map_a = classification_categories_a
            classification_label_map_b = classification_categories_b
    sampled, jobs = {}, []
    for category in categories_to_image_pairs.keys():
        image_pairs = categories_to_image_pairs[category]
        image_filenames = list(image_pairs.keys())
        if options.max_images_per_category is not None and options.max_images_per_category > 0:
            if len(image_filenames) > options.max_images_per_category:
                print('Sampling {} of {} image pairs for category {}'.format(options.max_images_per_category, len(image_filenames), category))
                image_filenames = random.sample(image_filenames, options.max_images_per_category)
            assert len(image_filenames) <= options.max_images_per_category
        sampled[category] = image_filenames
        category_folder = os.path.join(local_output_folder, category)
        for fn in image_filenames:
            image_pair = image_pairs[fn]
            jobs.append({
                'comparison': output_index, 'category': category, 'file': fn, 'input_path': os.path.join(options.image_folder, fn),
                'output_path': os.path.join(category_folder, flatten_path(fn)), 'target_width': options.target_width,
                'sides': [_side(image_pair['im_a']['detections'], pairwise_options.rendering_confidence_threshold_a,
                                pairwise_options.classification_confidence_threshold_a, THICKNESS_A, label_map,
                                classification_label_map_a, options.colormap_a, 'top'),
                          _side(image_pair['im_b']['detections'], pairwise_options.rendering_confidence_threshold_b,
                                pairwise_options.classification_confidence_threshold_b, THICKNESS_B, label_map,
                                classification_label_map_b, options.colormap_b, 'bottom')]})
    return {'output_index': output_index, 'pairwise_options': pairwise_options, 'categories_to_image_pairs': categories_to_image_pairs,
            'sampled': sampled, 'jobs': jobs, 'local_output_folder': local_output_folder, 'n_files': len(filenames_to_compare)}


def _side(detections, rendering_threshold, classification_threshold, thickness, label_map, classification_label_map, colormap,
          vtextalign):
    """What render_detection_bounding_boxes is called with for one file's detections in _render_image_pair, as
    preview.render_plan and preview.render_with_pil take it: (detections, PreviewOptions, keyword arguments)"""
    custom_strings = [''] * len(detections)
    for i_det, det in enumerate(detections):
        if 'transferred_from' in det:
            custom_strings[i_det] = '({})'.format(det['transferred_from'].split('.')[0])
    o = PV.PreviewOptions(confidence_threshold=0, output_image_width=None, box_thickness=thickness, box_expansion=0)
    by_category = None
    if isinstance(rendering_threshold, dict):
        by_category = rendering_threshold
    else:
        o.confidence_threshold = rendering_threshold
    return detections, o, dict(label_map=label_map, labels=label_map is not None, classification_label_map=classification_label_map,
                               classification_confidence_threshold=classification_threshold, category_thresholds=by_category,
                               colormap=colormap, vtextalign=vtextalign, custom_strings=custom_strings,
                               unlabelled_classifications=True)


# ---- rendering: the host leg ------------------------------------------------------------------------------------------------------

def render_job_host(job):
    """_render_image_pair by the reference's own PIL calls.  -> the output path"""
    assert os.path.isfile(job['input_path']), 'Image {} does not exist'.format(job['input_path'])
    im = open_image(job['input_path'])
    if job['target_width'] is not None:
        from PIL import Image
        size = resized_size(im.size[0], im.size[1], job['target_width'])
        if size != tuple(im.size):
            im = im.resize(size, Image.Resampling.LANCZOS)
    for detections, o, kw in job['sides']:
        PV.render_with_pil(im, detections, o, **kw)
    im.save(job['output_path'])
    return job['output_path']


def _render_host(jobs, options, threads_only=False):
    """the reference's loop over the images of a category, for all jobs: serial, or its pool of threads or processes"""
    if options.n_rendering_workers <= 1 or not jobs:
        return [render_job_host(job) for job in jobs]
    return DR.pool_map(render_job_host, jobs, options.n_rendering_workers, options.parallelize_rendering_with_threads or threads_only)


# ---- rendering: the device leg ----------------------------------------------------------------------------------------------------

def job_plan(job, size):
    """the drawing of one job on an image of `size` as ONE preview.RenderPlan: A's plan, then B's.  Raises preview.HostLeg"""
    plan = PV.RenderPlan()
    for detections, o, kw in job['sides']:
        try:
            plan.extend(PV.render_plan(detections, size[0], size[1], o, **kw))
        except PV.RenderFailure as e:
            raise PV.HostLeg(str(e))
    return plan


def plan_device_jobs(jobs, probes=None):
    """Which jobs the device leg renders, decided before any pixel is decoded.  -> (planned, host, undecodable): the jobs
    with their 'probe', 'source_size', 'size' and 'plan'; the jobs the host leg takes, in their order; the distinct files
    among those that the device does not decode.  A missing file is the reference's AssertionError.  probes: a dict that
    keeps device_decode.plan_source's probe per input path (a file is probed once however many jobs draw on it)."""
    from .device_decode import plan_source
    probes = {} if probes is None else probes
    planned, host, undecodable = [], [], []
    for job in jobs:
        assert os.path.isfile(job['input_path']), 'Image {} does not exist'.format(job['input_path'])
        try:
            p, size = plan_source(job['input_path'], job['output_path'], job['target_width'], probes=probes)
            plan = job_plan(job, size)
        except Exception:                                            # (not a HostLeg: the host leg raises it as the reference does)
            host.append(job)
            probed = probes[job['input_path']]                       # (what plan_source kept: the file is counted whatever fails after it)
            if isinstance(probed, dict) and probed['scan'] is None and job['file'] not in undecodable:
                undecodable.append(job['file'])
            continue
        planned.append(dict(job, probe=p, source_size=p['size'], size=size, plan=plan))
    return planned, host, undecodable


def group_by_file(planned):
    """the planned jobs grouped by source file, in order of first use"""
    groups = {}
    for job in planned:
        groups.setdefault(job['file'], []).append(job)
    return list(groups.values())


def group_bytes(group):
    """device bytes of the jobs of one file in their decode chunk: the decoded pixels, the resampled image when the size
    changes, and one destination per job that draws anything"""
    (w, h), (tw, th) = group[0]['source_size'], group[0]['size']
    return w * h * 3 + (tw * th * 3 if (tw, th) != (w, h) else 0) + tw * th * 3 * sum(1 for j in group if j['plan'].ops)


def _render_chunk_device(ctx, torch, device, groups, clock, options, counts):
    """The jobs of one chunk of files, by the device render path.  -> the jobs the host leg has to make"""
    heads, pixels, refused, _ = DR.decode_front(ctx, torch, device, [g[0] for g in groups], options.image_folder, counts, clock)
    refused = {j['file'] for j in refused}
    host = [j for g in groups for j in g if j['file'] in refused]    # the device did not decode it
    groups = [g for g in groups if g[0]['file'] not in refused]
    if not groups:
        return host
    # ONE shared image per distinct file: its decoded pixels, or their resampled form
    sizes = [j['size'] for j in heads]
    shared = DR.resample_jobs(ctx, torch, device, heads, pixels, counts, clock)
    jobs = [j for g in groups for j in g]
    # ONE fan-out draw: every job that draws anything gets an image of its own, made from its file's shared image
    drawn = [(k, j) for k, g in enumerate(groups) for j in g if j['plan'].ops]
    dests = [torch.empty(sizes[k][0] * sizes[k][1] * 3, dtype=torch.uint8, device=device) for k, _ in drawn]
    if DR.draw_plans_from(ctx, [t.data_ptr() for t in shared], sizes, [t.data_ptr() for t in dests], [k for k, _ in drawn],
                          [j['plan'] for _, j in drawn], device, clock=clock):
        counts['draw_calls'] += 1
    image_of = {id(j): t for (_, j), t in zip(drawn, dests)}
    rendered = [image_of.get(id(j), shared[k]) for k, g in enumerate(groups) for j in g]      # (no operation: the shared image itself)
    DR.encode_and_write(jobs, rendered, counts, partial(DR.encode_whole, ctx, clock, SAVE_QUALITY),
                        lambda job, data: DR.write_bytes(job['output_path'], data))
    return host


def _render_device(jobs, options, ctx, counts, profile):
    """-> the jobs that go to the host leg, in their order"""
    import torch
    planned, host, undecodable = plan_device_jobs(jobs)
    counts['files_decoded_pil'] += len(undecodable)
    place = {(j['comparison'], j['category'], j['file']): i for i, j in enumerate(jobs)}
    return DR.run_chunks(ctx, torch, group_by_file(planned), group_bytes, partial(_render_chunk_device, options=options, counts=counts),
                         counts, profile, host, jobs_of=list, order=lambda j: place[(j['comparison'], j['category'], j['file'])])


# ---- the pages --------------------------------------------------------------------------------------------------------------------

def _sanitize_id_name(s, lower=True):
    s = re.sub(r'[^a-zA-Z0-9_-]', '', s)
    s = re.sub(r'^[^a-zA-Z]*', '', s)
    if lower:
        s = s.lower()
    return s


def _write_pages(plan, options):
    """_pairwise_compare_batch_results behind the rendering: the page of every category, and the comparison's block of the
    index.  -> PairwiseBatchComparisonResults"""
    pairwise_options = plan['pairwise_options']
    categories_to_image_pairs = plan['categories_to_image_pairs']
    local_output_folder = plan['local_output_folder']
    color_string_a = str(options.colormap_a) if len(options.colormap_a) > 1 else options.colormap_a[0]
    color_string_b = str(options.colormap_b) if len(options.colormap_b) > 1 else options.colormap_b[0]
    for category in categories_to_image_pairs.keys():
        image_pairs = categories_to_image_pairs[category]
        image_filenames = plan['sampled'][category]
        input_image_absolute_paths = [os.path.join(options.image_folder, fn) for fn in image_filenames]
        category_image_output_paths = [os.path.join(local_output_folder, category, flatten_path(fn)) for fn in image_filenames]
        category_html_filename = os.path.join(local_output_folder, category + '.html')
        category_image_output_paths_relative = [os.path.relpath(s, local_output_folder) for s in category_image_output_paths]
        image_info = []
        assert len(category_image_output_paths_relative) == len(input_image_absolute_paths)
        for i_fn, fn in enumerate(category_image_output_paths_relative):
            input_path_relative = image_filenames[i_fn]
            image_pair = image_pairs[input_path_relative]
            image_a = image_pair['im_a']
            image_b = image_pair['im_b']
            if options.fn_to_display_fn is not None:
                assert input_path_relative in options.fn_to_display_fn, \
                    'fn_to_display_fn provided, but {} is not mapped'.format(input_path_relative)
                display_path = options.fn_to_display_fn[input_path_relative]
            else:
                display_path = input_path_relative
            sort_conf = image_pair['sort_conf']
            max_conf_a = _maxempty([det['conf'] for det in image_a['detections']])
            max_conf_b = _maxempty([det['conf'] for det in image_b['detections']])
            title = display_path + ' (max conf {:.2f},{:.2f})'.format(max_conf_a, max_conf_b)
            if options.parse_link_paths:
                link_target_string = urllib.parse.quote(input_image_absolute_paths[i_fn])
            else:
                link_target_string = input_image_absolute_paths[i_fn]
            image_info.append({
                'filename': fn,
                'title': title,
                'textStyle': 'font-family:verdana,arial,calibri;font-size:' + '80%;text-align:left;margin-top:20;margin-bottom:5',
                'linkTarget': link_target_string,
                'sort_conf': sort_conf
            })
        category_page_header_string = '<h1>{}</h1>\n'.format(CATEGORIES_TO_PAGE_TITLES[category])
        category_page_header_string += '<p style="font-weight:bold;">\n'
        category_page_header_string += 'Model A: {} ({})<br/>\n'.format(pairwise_options.results_description_a, color_string_a)
        category_page_header_string += 'Model B: {} ({})'.format(pairwise_options.results_description_b, color_string_b)
        category_page_header_string += '</p>\n'
        category_page_header_string += '<p>\n'
        category_page_header_string += 'Detection thresholds for A ({}):\n{}<br/>'.format(
            pairwise_options.results_description_a, str(pairwise_options.detection_thresholds_a))
        category_page_header_string += 'Detection thresholds for B ({}):\n{}<br/>'.format(
            pairwise_options.results_description_b, str(pairwise_options.detection_thresholds_b))
        category_page_header_string += 'Rendering threshold for A ({}):\n{}<br/>'.format(
            pairwise_options.results_description_a, str(pairwise_options.rendering_confidence_threshold_a))
        category_page_header_string += 'Rendering threshold for B ({}):\n{}<br/>'.format(
            pairwise_options.results_description_b, str(pairwise_options.rendering_confidence_threshold_b))
        category_page_header_string += '</p>\n'
        subpage_header_string = '\n'.join(category_page_header_string.split('\n')[1:])
        if options.sort_by_confidence:
            image_info = sorted(image_info, key=lambda d: d['sort_conf'], reverse=True)
        else:
            image_info = sorted(image_info, key=lambda d: d['filename'])
        write_html_image_list(category_html_filename, images=image_info, options={
            'pageTitle': '', 'headerHtml': category_page_header_string, 'subPageHeaderHtml': subpage_header_string,
            'maxFiguresPerHtmlFile': options.max_images_per_page})

    html_output_string = ''
    comparison_short_name = '{}_vs_{}'.format(_sanitize_id_name(pairwise_options.results_description_a),
                                              _sanitize_id_name(pairwise_options.results_description_b))
    comparison_friendly_name = '{} vs {}'.format(pairwise_options.results_description_a, pairwise_options.results_description_b)
    html_output_string += '<p id="{}">Comparing <b>{}</b> (A, {}) to <b>{}</b> (B, {})</p>'.format(
        comparison_short_name, pairwise_options.results_description_a, color_string_a.lower(),
        pairwise_options.results_description_b, color_string_b.lower())
    html_output_string += '<div class="contentdiv">\n'
    html_output_string += 'Detection thresholds for {}:\n{}<br/>'.format(
        pairwise_options.results_description_a, str(pairwise_options.detection_thresholds_a))
    html_output_string += 'Detection thresholds for {}:\n{}<br/>'.format(
        pairwise_options.results_description_b, str(pairwise_options.detection_thresholds_b))
    html_output_string += 'Rendering threshold for {}:\n{}<br/>'.format(
        pairwise_options.results_description_a, str(pairwise_options.rendering_confidence_threshold_a))
    html_output_string += 'Rendering threshold for {}:\n{}<br/>'.format(
        pairwise_options.results_description_b, str(pairwise_options.rendering_confidence_threshold_b))
    html_output_string += '<br/>'
    html_output_string += 'Rendering a maximum of {} images per category<br/>'.format(options.max_images_per_category)
    html_output_string += '<br/>'
    category_summary = ''
    for i_category, category_name in enumerate(categories_to_image_pairs):
        if i_category > 0:
            category_summary += '<br/>'
        category_summary += '{} {}'.format(len(categories_to_image_pairs[category_name]), category_name.replace('_', ' '))
    category_summary = 'Of {} total files:<br/><br/><div style="margin-left:15px;">{}</div><br/>'.format(
        plan['n_files'], category_summary)
    html_output_string += category_summary
    html_output_string += 'Comparison pages:<br/><br/>\n'
    html_output_string += '<div style="margin-left:15px;">\n'
    comparison_path_relative = os.path.relpath(local_output_folder, options.output_folder)
    for category in categories_to_image_pairs.keys():
        category_html_filename = os.path.join(comparison_path_relative, category + '.html')
        html_output_string += '<a href="{}">{}</a><br/>\n'.format(category_html_filename, category)
    html_output_string += '</div>\n'
    html_output_string += '</div>\n'

    pairwise_results = PairwiseBatchComparisonResults()
    pairwise_results.comparison_short_name = comparison_short_name
    pairwise_results.comparison_friendly_name = comparison_friendly_name
    pairwise_results.html_content = html_output_string
    pairwise_results.pairwise_options = pairwise_options
    pairwise_results.categories_to_image_pairs = categories_to_image_pairs
    return pairwise_results


# ---- the entry points -------------------------------------------------------------------------------------------------------------

def plan_comparisons(options):
    """compare_batch_results up to the rendering, on the deep copy of the options it works on: -> (that copy, the plan of every
    pairwise comparison); the category folders exist afterwards"""
    assert options.output_folder is not None
    assert options.image_folder is not None
    assert options.pairwise_options is not None
    check_restated(options)
    options = copy.deepcopy(options)
    if not isinstance(options.pairwise_options, list):
        options.pairwise_options = [options.pairwise_options]
    pairwise_options_list = options.pairwise_options
    n_comparisons = len(pairwise_options_list)
    options.pairwise_options = None
    plans = []
    for i_comparison, pairwise_options in enumerate(pairwise_options_list):
        print('Running comparison {} of {}'.format(i_comparison, n_comparisons))
        pairwise_options.verbose = options.verbose
        plans.append(_plan_pairwise(options, i_comparison, pairwise_options))
    for plan in plans:
        for category in plan['categories_to_image_pairs'].keys():
            print('Rendering detections for category {}'.format(category))
            os.makedirs(os.path.join(plan['local_output_folder'], category), exist_ok=True)
    return options, plans


def compare_batch_results(options, backend='gpu', device=0, profile=False):
    """
    The reference's compare_batch_results(options) without ground truth.  backend 'host': PIL, no GPU; 'gpu': the rendering on
    HIP device `device`, on a context without a model made for the call.  profile: also counts['ms'], the milliseconds around
    the decode, resample, draw and encode calls (the device is waited for around each: slower).
    Returns BatchComparisonResults: html_output_file, pairwise_results, and counts -- 'jobs' (one per sampled image of a
    comparison), of which 'gpu' were rendered on the device and 'host' by PIL; 'files_decoded_gpu' (distinct files: a file is
    decoded once per chunk however many comparisons draw on it), 'files_decoded_pil' (distinct files the device does not
    decode), 'decode_chunks', 'resample_calls', 'draw_calls', 'encode_calls' of the device leg.
    """
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    options, plans = plan_comparisons(options)
    jobs = [job for plan in plans for job in plan['jobs']]
    counts = {k: 0 for k in COUNT_KEYS}
    counts['jobs'] = len(jobs)
    if profile:
        counts['ms'] = {}
    host = jobs
    if backend == 'gpu' and jobs:
        from .hip_backend import HipContext
        with HipContext.images_or(None, device) as ctx:
            host = _render_device(jobs, options, ctx, counts, profile)
    _render_host(host, options, threads_only=backend == 'gpu')
    counts['host'] = len(host)

    html_content = ''
    all_pairwise_results = []
    for plan in plans:
        pairwise_results = _write_pages(plan, options)
        if not options.return_images_by_category:
            pairwise_results.categories_to_image_pairs = None
        html_content += pairwise_results.html_content
        all_pairwise_results.append(pairwise_results)
    html_output_string = main_page_header
    job_name_string = ''
    if len(options.job_name) > 0:
        job_name_string = ' for {}'.format(options.job_name)
    html_output_string += '<h2>Comparison of results{}</h2>\n'.format(job_name_string)
    if options.include_toc and (len(plans) > 2):
        toc_string = '<p><b>Contents</b></p>\n'
        toc_string += '<div class="contentdiv">\n'
        for r in all_pairwise_results:
            toc_string += '<a href="#{}">{}</a><br/>'.format(r.comparison_short_name, r.comparison_friendly_name)
        toc_string += '</div>\n'
        html_output_string += toc_string
    html_output_string += html_content
    html_output_string += main_page_footer
    html_output_file = os.path.join(options.output_folder, 'index.html')
    with open(html_output_file, 'w') as f:
        f.write(html_output_string)
    results = BatchComparisonResults()
    results.html_output_file = html_output_file
    results.pairwise_results = all_pairwise_results
    results.counts = counts
    return results


def n_way_comparison(filenames, options, detection_thresholds=None, rendering_thresholds=None, model_names=None, backend='gpu',
                     device=0):
    """The reference's n_way_comparison: every pairwise comparison of the results files in `filenames`."""
    if detection_thresholds is None:
        detection_thresholds = [0.15] * len(filenames)
    assert len(detection_thresholds) == len(filenames), '[detection_thresholds] should be the same length as [filenames]'
    if rendering_thresholds is not None:
        assert len(rendering_thresholds) == len(filenames), '[rendering_thresholds] should be the same length as [filenames]'
    else:
        rendering_thresholds = [(x * 0.6666) for x in detection_thresholds]
    if model_names is not None:
        assert len(model_names) == len(filenames), '[model_names] should be the same length as [filenames]'
    options.pairwise_options = []
    for i, j in itertools.combinations(list(range(0, len(filenames))), 2):
        pairwise_options = PairwiseBatchComparisonOptions()
        pairwise_options.results_filename_a = filenames[i]
        pairwise_options.results_filename_b = filenames[j]
        pairwise_options.rendering_confidence_threshold_a = rendering_thresholds[i]
        pairwise_options.rendering_confidence_threshold_b = rendering_thresholds[j]
        pairwise_options.detection_thresholds_a = {'default': detection_thresholds[i]}
        pairwise_options.detection_thresholds_b = {'default': detection_thresholds[j]}
        if model_names is not None:
            pairwise_options.results_description_a = model_names[i]
            pairwise_options.results_description_b = model_names[j]
        options.pairwise_options.append(pairwise_options)
    return compare_batch_results(options, backend=backend, device=device)


def main(argv=None):  # noqa
    options = BatchComparisonOptions()
    parser = argparse.ArgumentParser(
        prog='python -m megadetector_amd.compare_batch_results', formatter_class=argparse.RawDescriptionHelpFormatter,
        epilog=textwrap.dedent('''\
           Example:

           python -m megadetector_amd.compare_batch_results output_folder image_folder mdv5a.json mdv5b.json mdv4.json --detection_thresholds 0.15 0.15 0.7
           '''))
    parser.add_argument('output_folder', type=str, help='folder to which to write html results')
    parser.add_argument('image_folder', type=str, help='image source folder')
    parser.add_argument('results_files', nargs='*', type=str, help='list of .json files to be compared')
    parser.add_argument('--detection_thresholds', nargs='*', type=float,
                        help='list of detection thresholds, same length as the number of .json files, defaults to 0.15 for all files')
    parser.add_argument('--rendering_thresholds', nargs='*', type=float,
                        help='list of rendering thresholds, same length as the number of .json files, defaults to 0.10 for all files')
    parser.add_argument('--max_images_per_category', type=int, default=options.max_images_per_category,
                        help='number of images to sample for each agreement category (common detections, etc.)')
    parser.add_argument('--target_width', type=int, default=options.target_width,
                        help='output image width, defaults to {}'.format(options.target_width))
    parser.add_argument('--use_processes', action='store_true',
                        help='use processes rather than threads for parallelization (the host leg)')
    parser.add_argument('--open_results', action='store_true', help='accepted; the output html file is not opened')
    parser.add_argument('--n_rendering_workers', type=int, default=options.n_rendering_workers,
                        help='number of workers of the host leg, defaults to {}'.format(options.n_rendering_workers))
    parser.add_argument('--backend', choices=('gpu', 'host'), default='gpu', help='where the images are rendered')
    parser.add_argument('--device', type=int, default=0, help='the HIP device of the gpu backend')
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    print('Output folder:')
    print(args.output_folder)
    print('\nResults files:')
    print(args.results_files)
    print('\nDetection thresholds:')
    print(args.detection_thresholds)
    print('\nRendering thresholds:')
    print(args.rendering_thresholds)
    options = BatchComparisonOptions()
    options.output_folder = args.output_folder
    options.image_folder = args.image_folder
    options.target_width = args.target_width
    options.n_rendering_workers = args.n_rendering_workers
    options.max_images_per_category = args.max_images_per_category
    if args.use_processes:
        options.parallelize_rendering_with_threads = False
    results = n_way_comparison(args.results_files, options, args.detection_thresholds, args.rendering_thresholds,
                               backend=args.backend, device=args.device)
    if args.open_results:
        print('Note: --open_results is accepted and ignored; open {} yourself'.format(results.html_output_file))
    print('Wrote results to {}'.format(results.html_output_file))
    return results


if __name__ == '__main__':
    main()
