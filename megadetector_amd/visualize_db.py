"""
The page one looks at before trusting or publishing a COCO Camera Traps file: the reference's visualization/visualize_db.py,
with its option names and defaults, on two legs that write the same bytes.  Images are sampled from the database, each is
resized (1000 pixels wide by default) and gets its ground-truth boxes, class names and scores drawn, and one HTML page is
written, or one page per category and an index.

Restated statement for statement (no pandas, no humanfriendly): the option clean-ups (a string becomes a list; the process-pool
warning), db_path as a file name or a loaded dict, trim_to_images_with_bboxes with its assertions, classes_to_include /
classes_to_exclude with '*multiple*' under IndexedJsonDb.get_classes_for_image's rule (the names of the sorted set of category
ids) -- and what building IndexedJsonDb does to the database it is handed: with a class filter the class names are lowered and
the file names get forward slashes, in place, so titles, labels and category pages are then in lower case --,
random.seed(random_seed) and random.sample only where the reference calls them, the sequence-friends pass for
max_sequence_length (None, <= 0, > 0) with its duplicate assertion, and the per-image annotation loop: confidence_threshold
with its assertion, sequence_level_annotation -> image / sequence / mixed, add_search_links, bbox against bbox_relative and
the three assertions, the NaN-float box, the '(93%)' tag, the output name <id lowercased, extension stripped>_gt.jpg with the
seven replaced characters; the title with frame, flags and extra image / annotation fields, the sequence header, linkTarget,
the three sort orders, create_category_pages with both page orders, 'no_categories' and clean_filename, index.html and every
page through postprocess_batch_results.write_html_image_list.  force_rendering=False skips existing files; a missing or
unopenable image gets no file but keeps its HTML entry; custom_category_mapping, colormap and quality are the reference's.
render_db_bounding_boxes is restated as written: y / img_height, then ymin + h / img_height, in floats, on the ORIGINAL size,
the result through draw_bounding_box_on_image's own multiplications (preview.corner_edges).

One deliberate difference: the reference joins a Python set of class names, so a title with several classes depends on string
hashing; here the names appear in first-seen order.  Not restated: an image_base_dir that is a URL (NotImplementedError before
anything is read or written), process pools (which the reference itself refuses), and html_options other than pageTitle,
headerHtml, subPageHeaderHtml, trailerHtml and maxFiguresPerHtmlFile.

backend='host' makes exactly the reference's PIL calls, in the reference's thread pool.  backend='gpu' works on a context
without a model, through device_render.run_chunks: the images in rendering order in decode chunks, each file decoded once; per
chunk ONE mdhip_resample_lanczos call (resize_images.resize_target with no_enlarge_width; none when nothing is resized), ONE
mdhip_draw_ops call and ONE mdhip_jpeg_encode call (quality 75, or options.quality, at 4:2:0).  Planning reuses preview.py, with
thin_outlines: ground-truth boxes are often smaller than twice their outline once the image is reduced, and
preview.thin_outline_ops keeps those on the device.  Pillow carries a source's COM segment through convert, rotate and resize
into the file it saves; the device leg writes it where Pillow does (jpeg_host.sampled_file).  The host leg takes, per image and
counted: a file the device does not decode, a drawing the plan hands over, a quality whose tables quant_tables does not give, a
chunk that fails on the device, and every image whose planning raises -- so whatever the reference raises, PIL raises here.

CLI: python -m megadetector_amd.visualize_db DB OUTPUT_DIR IMAGE_BASE_DIR [--num_to_visualize N --random_sort
         --trim_to_images_with_bboxes --random_seed S --backend gpu|host --device 0]
"""

import argparse
import json
import math
import os
import random
import sys
from collections import defaultdict
from copy import deepcopy
from functools import partial
from itertools import compress
from types import SimpleNamespace

from . import device_render as DR
from . import preview as PV
from .ref_utils import clean_filename, open_image
from .resize_images import resize_target

COUNT_KEYS = ('sampled', 'rendered', 'skipped', 'unopened', 'gpu', 'host', 'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks',
              'resample_calls', 'draw_calls', 'encode_calls')
RENDERED, SKIPPED, UNOPENED = 'rendered', 'skipped', 'unopened'


def default_html_options():
    """write_html_image_list() without arguments: the reference's options dict"""
    return {'f_html': -1, 'pageTitle': '', 'headerHtml': '', 'subPageHeaderHtml': '', 'trailerHtml': '',
            'defaultTextStyle': 'font-family:calibri,verdana,arial;font-weight:bold;font-size:150%;text-align:left;margin:0px;',
            'defaultImageStyle': 'margin:0px;margin-top:5px;margin-bottom:5px;', 'urlEncodeFilenames': True,
            'urlEncodeLinkTargets': True, 'maxFiguresPerHtmlFile': math.inf}


class DbVizOptions:
    """Parameters controlling the behavior of visualize_db(): the reference's names and defaults (visualize_db.py:40-170)"""

    def __init__(self):
        self.num_to_visualize = None                    # None: every image
        self.viz_size = (1000, -1)                      # -1 preserves the aspect ratio; None or (-1, -1): the original size
        self.html_options = default_html_options()
        self.sort_by_filename = True                    # False: random; ignored with max_sequence_length
        self.trim_to_images_with_bboxes = False
        self.random_seed = 0
        self.add_search_links = False
        self.include_image_links = False
        self.include_filename_links = False
        self.box_thickness = 4
        self.box_expansion = 0
        self.classes_to_include = None
        self.classes_to_exclude = None
        self.multiple_categories_tag = '*multiple*'
        self.parallelize_rendering = True
        self.parallelize_rendering_with_threads = True
        self.parallelize_rendering_n_cores = 12
        self.show_full_paths = False
        self.extra_image_fields_to_print = None
        self.extra_annotation_fields_to_print = None
        self.force_rendering = True
        self.verbose = False
        self.confidence_field_name = 'score'
        self.confidence_threshold = None
        self.custom_category_mapping = None
        self.quality = None                             # None: Pillow's default, 75
        self.colormap = None
        self.create_category_pages = False
        self.category_page_sort_order = 'alphabetical'  # or 'image_count'
        self.max_sequence_length = None


# ---- the reference's small helpers -------------------------------------------------------------------------------------------------

def is_empty(v):
    """utils/ct_utils.py is_empty: None, '', blanks, NaN"""
    if v is None:
        return True
    if isinstance(v, str) and len(v.strip()) == 0:
        return True
    if isinstance(v, float) and math.isnan(v):
        return True
    return False


def classes_for_image(image, image_id_to_annotations, cat_id_to_name):
    """IndexedJsonDb.get_classes_for_image: the names of the image's category ids, as a sorted set of ids"""
    if image['id'] not in image_id_to_annotations:
        return []
    class_ids = sorted(set(ann['category_id'] for ann in image_id_to_annotations[image['id']]))
    return [cat_id_to_name[x] for x in class_ids]


def category_page_name(category_name):
    """clean_filename(category_name, force_lower=True, replace_whitespace='_') + '.html'"""
    return clean_filename(category_name, force_lower=True, replace_whitespace='_') + '.html'


def check_restated(options, image_base_dir):
    if image_base_dir.startswith('http'):
        raise NotImplementedError('an image_base_dir that is a URL is not restated')
    defaults = default_html_options()
    for key in ('f_html', 'defaultTextStyle', 'defaultImageStyle', 'urlEncodeFilenames', 'urlEncodeLinkTargets'):
        if options.html_options.get(key, defaults[key]) not in (None, defaults[key]):
            raise NotImplementedError('html_options[{!r}] is not restated'.format(key))


# ---- which images, and what is said and drawn for each ----------------------------------------------------------------------------

def select_images(image_db, options):
    """visualize_db.py:225-397: trimming, the class filters, the sample and the sequence friends.
    -> (the images in rendering order, image id -> annotations, the label map)"""
    annotations, images, categories = image_db['annotations'], image_db['images'], image_db['categories']
    if options.trim_to_images_with_bboxes:
        b_has_bbox = [False] * len(annotations)
        for i_ann, ann in enumerate(annotations):
            if 'bbox' in ann or 'bbox_relative' in ann:
                if 'bbox' in ann:
                    assert isinstance(ann['bbox'], list)
                else:
                    assert isinstance(ann['bbox_relative'], list)
                b_has_bbox[i_ann] = True
        image_ids_with_boxes = set(x['image_id'] for x in compress(annotations, b_has_bbox))
        images = [image for image in images if image['id'] in image_ids_with_boxes]
    assert not ((options.classes_to_exclude is not None) and (options.classes_to_include is not None)), \
        'Cannot specify an inclusion and exclusion list'
    if options.classes_to_exclude is not None:
        assert isinstance(options.classes_to_exclude, list), 'If supplied, classes_to_exclude should be a list'
    if options.classes_to_include is not None:
        assert isinstance(options.classes_to_include, list), 'If supplied, classes_to_include should be a list'
    if (options.classes_to_exclude is not None) or (options.classes_to_include is not None):
        print('Indexing database')
        # IndexedJsonDb(image_db) changes the database it is given: class names in lower case -- so the label map below, the
        # titles and the labels are in lower case whenever a class filter is set -- and file names with forward slashes
        assert 'images' in image_db
        for c in image_db['categories']:
            c['name'] = c['name'].lower()
        for im in image_db['images']:
            im['file_name'] = im['file_name'].replace('\\', '/')
        indexed = defaultdict(list)
        for ann in image_db['annotations']:
            indexed[ann['image_id']].append(ann)
        cat_id_to_name = {cat['id']: cat['name'] for cat in image_db['categories']}
        b_valid_class = [True] * len(images)
        for i_image, image in enumerate(images):
            classes = classes_for_image(image, indexed, cat_id_to_name)
            if options.classes_to_exclude is not None:
                for excluded_class in options.classes_to_exclude:
                    if excluded_class in classes:
                        b_valid_class[i_image] = False
                        break
            else:
                b_valid_class[i_image] = False
                if options.multiple_categories_tag in options.classes_to_include:
                    if len(classes) > 1:
                        b_valid_class[i_image] = True
                if not b_valid_class[i_image]:
                    for c in classes:
                        if c in options.classes_to_include:
                            b_valid_class[i_image] = True
                            break
        images = list(compress(images, b_valid_class))
    label_map = {}
    for cat in categories:
        label_map[int(cat['id'])] = cat['name']
    sequence_id_to_images = defaultdict(list)
    if options.max_sequence_length is not None:
        for im in images:
            if 'seq_id' in im:
                sequence_id_to_images[im['seq_id']].append(im)
    if options.num_to_visualize is not None:
        if options.num_to_visualize > len(images):
            print('Warning: asked to visualize {} images, but only {} are available, keeping them all'.format(
                options.num_to_visualize, len(images)))
        else:
            random.seed(options.random_seed)
            images = random.sample(images, options.num_to_visualize)
    image_id_to_annotations = defaultdict(list)
    for ann in annotations:
        image_id_to_annotations[ann['image_id']].append(ann)
    if options.max_sequence_length is not None:
        print('Preparing sequence friends')
        seq_id_to_images_rendered = defaultdict(int)
        image_ids_already_sampled = set()
        for im in images:
            image_ids_already_sampled.add(im['id'])
            if 'seq_id' in im:
                seq_id_to_images_rendered[im['seq_id']] += 1
        images_to_add = []
        for im in images:
            if 'seq_id' not in im:
                continue
            seq_id = im['seq_id']
            for candidate_im in sequence_id_to_images[seq_id]:
                if (options.max_sequence_length > 0) and (seq_id_to_images_rendered[seq_id] >= options.max_sequence_length):
                    if options.verbose:
                        print('Already rendered {} images from sequence {}'.format(options.max_sequence_length, seq_id))
                    break
                assert candidate_im['seq_id'] == seq_id
                if candidate_im['id'] not in image_ids_already_sampled:
                    images_to_add.append(candidate_im)
                    image_ids_already_sampled.add(candidate_im['id'])
                    seq_id_to_images_rendered[seq_id] += 1
        print('Adding {} new images ({} initially) as sequence friends'.format(len(images_to_add), len(images)))
        images.extend(images_to_add)                                         # (in place, as there: without a trim, a filter or a
        all_image_ids = [im['id'] for im in images]                          # sample this is the database's own list)
        assert len(all_image_ids) == len(set(all_image_ids))
    return images, image_id_to_annotations, label_map


def output_file_name(img_id):
    """visualize_db.py:504-511"""
    file_name = '{}_gt.jpg'.format(os.path.splitext(str(img_id).lower())[0])
    for c in ['/', '\\', ':', '\t', '#', ' ', '%']:
        file_name = file_name.replace(c, '~')
    return file_name


def describe_image(img, annotations_this_image, image_base_dir, label_map, options):
    """visualize_db.py:401-585 for one image: -> (what is rendered -- 'bboxes', 'box_classes', 'tags', 'img_path',
    'output_file_name', 'boxes_are_normalized' --, its entry of the HTML page)"""
    img_id = img['id']
    assert img_id is not None
    img_relative_path = img['file_name']
    img_path = os.path.join(image_base_dir, img_relative_path).replace('\\', '/')
    bboxes, box_classes, box_score_strings = [], [], []
    image_categories = []                                                    # first-seen order (the reference: a set)
    extra_annotation_field_string = ''
    annotation_level_for_image = ''
    boxes_are_normalized = None
    for ann in annotations_this_image:
        if options.extra_annotation_fields_to_print is not None:
            for field_name in ann.keys():
                if field_name in options.extra_annotation_fields_to_print:
                    field_value = ann[field_name]
                    if not is_empty(field_value):
                        extra_annotation_field_string += ' ({}:{})'.format(field_name, field_value)
        if options.confidence_threshold is not None:
            assert options.confidence_field_name in ann, \
                'Error: confidence thresholding requested, ' + \
                'but at least one annotation does not have the {} field'.format(options.confidence_field_name)
            if ann[options.confidence_field_name] < options.confidence_threshold:
                continue
        if 'sequence_level_annotation' in ann:
            annotation_level = 'sequence' if ann['sequence_level_annotation'] else 'image'
            if annotation_level_for_image == '':
                annotation_level_for_image = annotation_level
            elif annotation_level_for_image != annotation_level:
                annotation_level_for_image = 'mixed'
        category_id = ann['category_id']
        category_name = label_map[category_id]
        if options.add_search_links:
            category_name = category_name.replace('"', '')
            category_name = '<a href="https://www.google.com/search?tbm=isch&q={}">{}</a>'.format(category_name, category_name)
        if category_name not in image_categories:
            image_categories.append(category_name)
        assert not ('bbox' in ann and 'bbox_relative' in ann), \
            "An annotation can't have both an absolute and a relative bounding box"
        box_field = 'bbox'
        if 'bbox_relative' in ann:
            box_field = 'bbox_relative'
            assert (boxes_are_normalized is None) or (boxes_are_normalized), \
                "An image can't have both absolute and relative bounding boxes"
            boxes_are_normalized = True
        elif 'bbox' in ann:
            assert (boxes_are_normalized is None) or (not boxes_are_normalized), \
                "An image can't have both absolute and relative bounding boxes"
            boxes_are_normalized = False
        if box_field in ann:
            bbox = ann[box_field]
            if isinstance(bbox, float):
                assert math.isnan(bbox), "I shouldn't see a bbox that's neither a box nor NaN"
                continue
            bboxes.append(bbox)
            box_classes.append(ann['category_id'])
            box_score_string = ''
            if options.confidence_field_name is not None and options.confidence_field_name in ann:
                box_score_string = '({}%)'.format(round(100 * ann[options.confidence_field_name]))
            box_score_strings.append(box_score_string)
    image_classes = ', '.join(image_categories)
    file_name = output_file_name(img_id)
    rendering_info = {'bboxes': bboxes, 'box_classes': box_classes, 'tags': box_score_strings, 'img_path': img_path,
                      'output_file_name': file_name, 'boxes_are_normalized': boxes_are_normalized}
    label_level_string = ''
    if len(annotation_level_for_image) > 0:
        label_level_string = ' (annotation level: {})'.format(annotation_level_for_image)
    if 'frame_num' in img and 'seq_num_frames' in img:
        frame_string = ' frame: {} of {},'.format(img['frame_num'], img['seq_num_frames'])
    elif 'frame_num' in img:
        frame_string = ' frame: {},'.format(img['frame_num'])
    else:
        frame_string = ''
    filename_text = img_path if options.show_full_paths else img_relative_path
    if options.include_filename_links:
        filename_text = '<a href="{}">{}</a>'.format(img_path, filename_text)
    flag_string = ''
    if ('flags' in img) and (not is_empty(img['flags'])):
        flag_string = ', flags: {}'.format(str(img['flags']))
    extra_field_string = ''
    if options.extra_image_fields_to_print is not None:
        for field_name in options.extra_image_fields_to_print:
            if field_name in img:
                extra_field_string += ', {}: {}'.format(field_name, str(img[field_name]))
    image_dict = {
        'filename': '{}/{}'.format('rendered_images', file_name),
        'title': '{}<br/>{}, num boxes: {},{} class labels: {}{}{}{}{}'.format(
            filename_text, img_id, len(bboxes), frame_string, image_classes, label_level_string, flag_string, extra_field_string,
            extra_annotation_field_string),
        'textStyle': 'font-family:verdana,arial,calibri;font-size:80%;text-align:left;margin-top:20;margin-bottom:5;',
        'imageStyle': 'max-width:95%;',
        'image_categories': image_categories,
    }
    if (options.max_sequence_length is not None) and ('frame_num' in img) and ('seq_id' in img) and \
       (img['frame_num'] is not None) and (img['frame_num'] in (0, -1)):
        sequence_header = '<span style="font-weight:bold;font-size:120%">Sequence {}</span><br/><br/>'.format(img['seq_id'])
        image_dict['title'] = sequence_header + image_dict['title']
    if options.include_image_links:
        image_dict['linkTarget'] = img_path
    for field_name in ('seq_id', 'frame_num'):
        if field_name in img:
            image_dict[field_name] = img[field_name]
    return rendering_info, image_dict


def display_boxes(info, original_size, label_map):
    """render_db_bounding_boxes :1240-1285: per box ((ymin, xmin, ymax, xmax) normalised on the ORIGINAL size, its class, its
    one label line)"""
    img_width, img_height = original_size
    tags = info.get('tags')
    out = []
    for i_box, (box, clss) in enumerate(zip(info['bboxes'], info['box_classes'])):
        x_min_abs, y_min_abs, width_abs, height_abs = box[0:4]
        if info['boxes_are_normalized']:
            xmin, xmax = x_min_abs, x_min_abs + width_abs
            ymin, ymax = y_min_abs, y_min_abs + height_abs
        else:
            ymin = y_min_abs / img_height
            ymax = ymin + height_abs / img_height
            xmin = x_min_abs / img_width
            xmax = xmin + width_abs / img_width
        name = label_map[int(clss)] if (label_map is not None) and (int(clss) in label_map) else clss
        display_str = str(name)
        if tags is not None and tags[i_box] is not None and len(tags[i_box]) > 0:
            display_str += ' ' + tags[i_box]
        out.append(((ymin, xmin, ymax, xmax), clss, display_str))
    return out


def _draw_sizes(options, width):
    # draw_bounding_box_on_image :996-1013 (asserted only where a box is drawn, as there)
    assert options.box_thickness != 0.0, 'thickness cannot be zero'
    return PV.resolve_sizes(SimpleNamespace(box_thickness=options.box_thickness, box_expansion=options.box_expansion,
                                            label_font_size=PV.DEFAULT_LABEL_FONT_SIZE), width)


def rendering_label_map(label_map, options):
    return label_map if options.custom_category_mapping is None else options.custom_category_mapping


def db_render_plan(info, original_size, size, options, label_map, thin_outlines=True):
    """render_db_bounding_boxes for an image of `size` (the resized size) as a preview.RenderPlan: per box its outline
    (preview.box_outline_ops), then the patch of its label line.  Raises preview.HostLeg or preview.RenderFailure."""
    width, height = size
    plan = PV.RenderPlan()
    for (ymin, xmin, ymax, xmax), clss, display_str in display_boxes(info, original_size, rendering_label_map(label_map, options)):
        color_name, rgb = PV.box_color(clss, options.colormap)
        thickness, expansion, font_size = _draw_sizes(options, width)
        left, top, right, bottom = PV.corner_edges(ymin, xmin, ymax, xmax, width, height, expansion)
        plan.ops += PV.box_outline_ops(left, top, right, bottom, thickness, rgb, thin_outlines)
        plan.labels.append(display_str)
        if len(display_str) == 0:
            continue
        font = PV.load_font(PV.DEFAULT_LABEL_FONT, font_size)
        PV.add_label_ops(plan, font, (PV.DEFAULT_LABEL_FONT, font_size), [display_str], left, top, bottom, height, 'top', color_name)
    return plan


def render_db_with_pil(image, info, original_size, options, label_map):
    """render_db_bounding_boxes by PIL's own calls in the reference's order (draw_bounding_box_on_image :978-1137), IN PLACE"""
    from PIL import ImageDraw
    for (ymin, xmin, ymax, xmax), clss, display_str in display_boxes(info, original_size, rendering_label_map(label_map, options)):
        color_name, _ = PV.box_color(clss, options.colormap)
        draw = ImageDraw.Draw(image)
        width, height = image.size
        thickness, expansion, font_size = _draw_sizes(options, width)
        left, top, right, bottom = PV.corner_edges(ymin, xmin, ymax, xmax, width, height, expansion)
        draw.rectangle([(left, top), (right, bottom)], outline=color_name, width=thickness)
        font = PV.load_font(PV.DEFAULT_LABEL_FONT, font_size)
        for padded, _, corner0, corner1, text_at in PV.stacked_labels(font, [display_str], left, top, bottom, height):
            draw.rectangle([corner0, corner1], fill=color_name)
            draw.text(text_at, padded, fill='black', font=font)
    return image


def viz_target(source_size, viz_size):
    """:628-635 with resize_image's decision: -> (the size the image is rendered at, whether it is resized); the reference's
    assertion for a target that is not positive"""
    if (viz_size is None) or (viz_size[0] == -1 and viz_size[1] == -1):
        return tuple(source_size), False
    width, height, resized = resize_target(source_size, viz_size[0], viz_size[1], no_enlarge_width=True)
    if not resized:
        return tuple(source_size), False
    assert width > 0 and height > 0, 'Invalid image resize target {},{}'.format(width, height)
    return (width, height), True


# ---- rendering: the host leg ------------------------------------------------------------------------------------------------------

def _output_path(info, output_dir):
    return os.path.join(output_dir, 'rendered_images', info['output_file_name'])


def render_host(info, output_dir, options, label_map):
    """_render_image_info :589-660 by the reference's own PIL calls.  -> RENDERED, SKIPPED (an existing file without
    force_rendering) or UNOPENED (no file)"""
    from PIL import Image
    img_path = info['img_path']
    output_full_path = _output_path(info, output_dir)
    if (os.path.isfile(output_full_path)) and (not options.force_rendering):
        if options.verbose:
            print('Skipping existing image {}'.format(output_full_path))
        return SKIPPED
    if not os.path.exists(img_path):
        print('Image {} cannot be found'.format(img_path))
        return UNOPENED
    try:
        original_image = open_image(img_path)
        original_size = original_image.size
        size, resized = viz_target(original_size, options.viz_size)
        image = original_image.resize(size, Image.Resampling.LANCZOS) if resized else original_image
    except Exception as e:
        print('Image {} failed to open, error: {}'.format(img_path, e))
        return UNOPENED
    render_db_with_pil(image, info, original_size, options, label_map)
    if options.quality is None:
        image.save(output_full_path)
    else:
        image.save(output_full_path, quality=options.quality)
    return RENDERED


def _map(function, items, options):
    """:667-700: serial, or the reference's pool of threads"""
    if not options.parallelize_rendering:
        return [function(item) for item in items]
    n = options.parallelize_rendering_n_cores
    if n is not None:
        print('Rendering images with {} {}'.format(n, 'threads'))
    try:
        return DR.pool_map(function, items, n, True)
    finally:
        print('Pool closed and joined for DB visualization')


# ---- rendering: the device leg ----------------------------------------------------------------------------------------------------

def plan_job(info, options, label_map, thin_outlines=True):
    """What the device needs for one image before any pixel is decoded: -> the job; raises preview.HostLeg, or whatever the
    planning raises (the host leg then does what the reference does with it)."""
    from . import jpeg_host
    from .device_decode import plan_source
    p, source_size = plan_source(info['img_path'], info['output_file_name'], keep_data=True)
    comment = jpeg_host.keep_source(info['img_path'], p.pop('data', None))['comment']
    if len(comment or b'') > 65533:
        raise PV.HostLeg('a comment Pillow refuses')
    size, _ = viz_target(source_size, options.viz_size)
    if max(size) > 65535:
        raise PV.HostLeg('a side above 65535 pixels')
    quality = PV.DEFAULT_PREVIEW_QUALITY if options.quality is None else options.quality
    try:
        jpeg_host.quant_tables(quality)
    except ValueError:
        raise PV.HostLeg('a quality whose tables quant_tables does not give')
    plan = db_render_plan(info, source_size, size, options, label_map, thin_outlines)
    return {'info': info, 'file': info['img_path'], 'probe': p, 'source_size': tuple(source_size), 'size': size, 'plan': plan,
            'quality': quality, 'comment': comment}


def _render_chunk_device(ctx, torch, device, jobs, clock, output_dir, counts):
    """The images of one chunk, by the device render path.  -> the entries the host leg has to render"""
    jobs, tensors, host, _ = DR.decode_front(ctx, torch, device, jobs, '', counts, clock)
    if jobs:
        DR.render_jobs(ctx, torch, device, jobs, tensors, counts, clock, partial(DR.encode_whole, ctx, clock, jobs[0]['quality']),
                       lambda job, data: DR.write_bytes(_output_path(job['info'], output_dir), data))
    return [j['info'] for j in host]


def _render_device(to_render, output_dir, options, label_map, ctx, counts, profile, thin_outlines):
    """-> the entries of to_render that go to the host leg, in their order"""
    import torch
    planned, host = DR.plan_each(to_render, lambda info: plan_job(info, options, label_map, thin_outlines))
    place = {id(info): i for i, info in enumerate(to_render)}
    return DR.run_chunks(ctx, torch, planned, DR.job_bytes, partial(_render_chunk_device, output_dir=output_dir, counts=counts), counts,
                         profile, host, DR.file_twice, lambda job: [job['info']], lambda info: place[id(info)])


def render_images(rendering_info, output_dir, options, label_map, backend, device, counts, profile, thin_outlines=True):
    """Renders every entry of rendering_info on `backend`; fills counts"""
    host = rendering_info
    if backend == 'gpu':
        to_render = []
        for info in rendering_info:
            if (os.path.isfile(_output_path(info, output_dir))) and (not options.force_rendering):
                if options.verbose:
                    print('Skipping existing image {}'.format(_output_path(info, output_dir)))
                counts['skipped'] += 1
            elif not os.path.exists(info['img_path']):
                print('Image {} cannot be found'.format(info['img_path']))
                counts['unopened'] += 1
            else:
                to_render.append(info)
        host = to_render
        if to_render:
            from .hip_backend import HipContext
            with HipContext.images_or(None, device) as ctx:
                host = _render_device(to_render, output_dir, options, label_map, ctx, counts, profile, thin_outlines)
    render = partial(render_host, output_dir=output_dir, options=options, label_map=label_map)
    for status in _map(render, host, options):
        counts['host' if status == RENDERED else status] += 1
    counts['rendered'] = counts['gpu'] + counts['host']


# ---- the pages --------------------------------------------------------------------------------------------------------------------

def write_pages(images_html, db_path, output_dir, options):
    """visualize_db.py:707-835: sorts the entries and writes index.html, or one page per category and the index.  -> index.html"""
    from .postprocess_batch_results import write_html_image_list
    if options.max_sequence_length is not None:
        for im in images_html:
            if 'seq_id' not in im:
                im['seq_id'] = 'no_sequence_id'
            if 'frame_num' not in im:
                im['frame_num'] = -1
        images_html = sorted(images_html, key=lambda x: (x['seq_id'], x['frame_num'], x['filename']))
    elif options.sort_by_filename:
        images_html = sorted(images_html, key=lambda x: x['filename'])
    else:
        random.shuffle(images_html)
    html_output_file = os.path.join(output_dir, 'index.html')
    if isinstance(db_path, str):
        title_string = '<h1>Sample annotations from {}</h1>'.format(db_path)
    else:
        title_string = '<h1>Sample annotations</h1>'
    if not options.create_category_pages:
        html_options = options.html_options
        html_options['headerHtml'] = title_string
        write_html_image_list(html_output_file, images_html, html_options)
        print('Visualized {} images, wrote results to {}'.format(len(images_html), html_output_file))
        return html_output_file
    category_name_to_count = defaultdict(int)
    for im in images_html:
        for category_name in im['image_categories']:
            category_name_to_count[category_name] += 1
    if options.category_page_sort_order == 'image_count':
        all_categories = [k for k, _ in sorted(category_name_to_count.items(), key=lambda item: item[1], reverse=True)]
    else:
        if options.category_page_sort_order != 'alphabetical':
            print('Warning: unrecognized category sort order: {}'.format(options.category_page_sort_order))
        all_categories = sorted(list(category_name_to_count.keys()))
    no_category_token = 'no_categories'
    all_categories.append(no_category_token)
    category_name_to_relative_filename = {}
    category_name_to_count = {}
    for category_name in all_categories:
        category_filename_relative = category_page_name(category_name)
        category_name_to_relative_filename[category_name] = category_filename_relative
        if category_name == no_category_token:
            images_this_category = [im for im in images_html if len(im['image_categories']) == 0]
        else:
            images_this_category = [im for im in images_html if category_name in im['image_categories']]
        category_name_to_count[category_name] = len(images_this_category)
        html_options = deepcopy(options.html_options)
        html_options['headerHtml'] = '<h1>Sample annotations for category {}</h1>'.format(category_name)
        write_html_image_list(os.path.join(output_dir, category_filename_relative), images_this_category, html_options)
    with open(html_output_file, 'w') as f:
        f.write('<html><head>{}</head><body>\n'.format(title_string))
        for category_name in category_name_to_relative_filename:
            s = '<p style="padding:0px;margin:0px;margin-left:15px;text-align:left;'
            s += 'font-family:segoe ui,calibri,arial;font-size:100%;text-decoration:none;font-weight:normal;">'
            f.write(s)
            f.write('<a href="{}">{}</a> ({} images)</p>\n'.format(
                category_name_to_relative_filename[category_name], category_name, category_name_to_count[category_name]))
        f.write('</body></html>\n')
    return html_output_file


# ---- the tool ---------------------------------------------------------------------------------------------------------------------

def visualize_db(db_path, output_dir, image_base_dir, options=None, backend='gpu', device=0, counts=None, profile=False,
                 thin_outlines=True):
    """
    Writes images and HTML to output_dir to visualize the images and annotations of a COCO-formatted .json file (a file name
    or a loaded dict); the file names of the database are relative to image_base_dir.  backend 'host': PIL, no GPU; 'gpu': the
    rendering on HIP device `device`, on a context without a model made for the call.  counts: a dict that is filled in place
    with COUNT_KEYS -- 'sampled' images, of which 'rendered' (a file was written: 'gpu' on the device, 'host' by PIL), 'skipped'
    (an existing file without force_rendering) and 'unopened' (no file, listed all the same), and the device leg's
    'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks', 'resample_calls', 'draw_calls', 'encode_calls' -- and, with
    profile, 'ms' per kind of device call (the device is waited for around each: slower).  thin_outlines False: a box thinner
    than twice its outline sends its image to the host leg, as in the other tools (for measuring what the option saves).
    -> (the html file name, the loaded database)
    """
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    if options is None:
        options = DbVizOptions()
    if isinstance(options.extra_image_fields_to_print, str):
        options.extra_image_fields_to_print = [options.extra_image_fields_to_print]
    if isinstance(options.extra_annotation_fields_to_print, str):
        options.extra_annotation_fields_to_print = [options.extra_annotation_fields_to_print]
    if not options.parallelize_rendering_with_threads:
        print('Warning: process-based parallelization is not yet supported by visualize_db')
        options.parallelize_rendering_with_threads = True
    check_restated(options, image_base_dir)
    assert (os.path.isdir(image_base_dir))
    os.makedirs(os.path.join(output_dir, 'rendered_images'), exist_ok=True)
    if isinstance(db_path, str):
        assert (os.path.isfile(db_path))
        print('Loading database from {}...'.format(db_path))
        with open(db_path) as f:
            image_db = json.load(f)
        print('...done, loaded {} images'.format(len(image_db['images'])))
    elif isinstance(db_path, dict):
        print('Using previously-loaded DB')
        image_db = db_path
    else:
        raise ValueError('Illegal dictionary or filename')
    images, image_id_to_annotations, label_map = select_images(image_db, options)
    print('Preparing rendering list')
    images_html, rendering_info = [], []
    for img in images:
        annotations_this_image = image_id_to_annotations[img['id']] if img['id'] in image_id_to_annotations else []
        info, image_dict = describe_image(img, annotations_this_image, image_base_dir, label_map, options)
        rendering_info.append(info)
        images_html.append(image_dict)
    counts = {} if counts is None else counts
    counts.update({k: 0 for k in COUNT_KEYS})
    counts['sampled'] = len(images)
    if profile:
        counts['ms'] = {}
    print('Rendering images')
    render_images(rendering_info, output_dir, options, label_map, backend, device, counts, profile, thin_outlines)
    print('Rendered {} images ({} successful)'.format(len(rendering_info), counts['rendered'] + counts['skipped']))
    return write_pages(images_html, db_path, output_dir, options), image_db


def main(argv=None):
    parser = argparse.ArgumentParser(description='Render a sample of a COCO Camera Traps database to an HTML page')
    parser.add_argument('db_path', type=str, help='.json file to visualize')
    parser.add_argument('output_dir', type=str, help='Output directory for html and rendered images')
    parser.add_argument('image_base_dir', type=str, help='Base directory for input images')
    parser.add_argument('--num_to_visualize', type=int, default=None, help='Number of images to visualize (randomly drawn) (defaults to all)')
    parser.add_argument('--random_sort', action='store_true', help='Sort randomly (rather than by filename) in output html')
    parser.add_argument('--trim_to_images_with_bboxes', action='store_true', help='Only include images with bounding boxes')
    parser.add_argument('--random_seed', type=int, default=None, help='Random seed for image selection')
    parser.add_argument('--backend', choices=('gpu', 'host'), default='gpu', help="'host': the reference's PIL calls, no GPU needed")
    parser.add_argument('--device', type=int, default=0, help='HIP device of the gpu backend')
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    backend, device = args.backend, args.device
    del args.backend, args.device
    options = DbVizOptions()
    for n, v in vars(args).items():                                          # (_args_to_object)
        if not n.startswith('_'):
            setattr(options, n, v)
    if options.random_sort:
        options.sort_by_filename = False
    counts = {}
    visualize_db(options.db_path, options.output_dir, options.image_base_dir, options, backend=backend, device=device, counts=counts)
    print('Sampled {} images ({})'.format(counts['sampled'], ', '.join('{} {}'.format(k, v) for k, v in counts.items() if k != 'sampled')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
