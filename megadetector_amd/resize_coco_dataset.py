"""
Resizing a COCO dataset as training preparation: the reference's data_management/resize_coco_dataset.py -- every image of a
COCO file resized (or copied, or rewritten) into an output folder, its boxes scaled, a new COCO file written -- with the
reference's argument names, defaults, return value and command line, on two legs that write the same bytes.

Restated statement for statement (process_single_image): the per-image decision -- a missing file; open_image is lazy, so a
file opens although its pixels do not decode; already the target size; no_enlarge_width and input_w < target_w; both
dimensions -1 --, 'copy' as shutil.copyfile unless source and target are one path, 'rewrite' as exif_preserving_save(pil_im,
out), the resized save with tags_to_exclude=('Orientation',), the three exception texts under 'error', the prints and the
omission under 'omit', width and height of the image record from the saved image, the box scaling (four multiplications by
output_w / input_w and output_h / input_h, only for annotations with a 'bbox', only when a side changed), images without
annotations, the order of the lists, and the text write_json writes (json.dump with indent 1, newline '\\n').  The reference
loads files that end early (visualization_utils sets ImageFile.LOAD_TRUNCATED_IMAGES when imported), so such a file is resized
like any other; both legs do the same for the length of a call (gray_scale._reference_truncation_rule: while a call runs,
other threads of the process load truncated files too).

backend='host' makes the reference's PIL calls in the reference's pool.  backend='gpu' is the device leg of resize_images.py
(render_chunk: per decode chunk one decode, ONE mdhip_resample_lanczos call, ONE mdhip_jpeg_encode_sampled call): it plans
every image from device_decode.probe and hands everything that raises, every copy, and every file the device does not decode
or write to the host leg, so every message is the reference's.  pool_type and n_workers size the host leg's pool; with the
gpu backend that pool is one of threads.

CLI (the reference's, plus --backend and --device):
    python -m megadetector_amd.resize_coco_dataset INPUT_FOLDER INPUT_FILENAME OUTPUT_FOLDER OUTPUT_FILENAME
        [--target_size "W,H" --correct_size_image_handling copy|rewrite --n_workers N --pool_type thread|process
         --backend gpu|host --device 0]
"""

import argparse
import json
import os
import shutil
import sys
from collections import defaultdict
from functools import partial

from . import device_render as DR
from .gray_scale import _reference_truncation_rule
from .preview import HostLeg
from .ref_utils import DEFAULT_SAVE_QUALITY as DEFAULT_QUALITY
from .ref_utils import ORIENTATION, exif_preserving_save, exif_without, open_image, write_json
from .resize_images import _resize_image, render_chunk, resize_target

COUNT_KEYS = ('files', 'omitted', 'gpu', 'host', 'files_decoded_gpu', 'decode_chunks', 'resample_calls', 'encode_calls')


def finish_image(im, annotations_this_image, input_size, output_size):
    """the end of the reference's per-image function: the record's size and the scaled boxes"""
    (input_w, input_h), (output_w, output_h) = input_size, output_size
    im['width'] = output_w
    im['height'] = output_h
    for ann in annotations_this_image:
        if 'bbox' in ann:
            bbox = ann['bbox']
            if (output_w != input_w) or (output_h != input_h):
                width_scale = output_w / input_w
                height_scale = output_h / input_h
                bbox = [bbox[0] * width_scale, bbox[1] * height_scale, bbox[2] * width_scale, bbox[3] * height_scale]
            ann['bbox'] = bbox
    return im, annotations_this_image


def correct_size(input_size, target_size, no_enlarge_width):
    """whether the reference writes the image at its own size: already the target size, no_enlarge_width and narrower than the
    target, or both dimensions -1"""
    input_w, input_h = input_size
    image_is_already_target_size = (input_w == target_size[0]) and (input_h == target_size[1])
    if no_enlarge_width and (input_w < target_size[0]):
        image_is_already_target_size = True
    preserve_original_size = (target_size[0] == -1) and (target_size[1] == -1)
    return image_is_already_target_size or preserve_original_size


def process_single_image(image_data, input_folder, output_folder, target_size, correct_size_image_handling, unavailable_image_handling,
                         no_enlarge_width, verbose):
    """_process_single_image_for_resize: image_data is (image record, its annotations) -> (the new record, the new
    annotations), or (None, None) for an image that is omitted"""
    assert unavailable_image_handling in ('error', 'omit'), 'Illegal unavailable_image_handling {}'.format(unavailable_image_handling)
    assert isinstance(image_data, tuple) and len(image_data) == 2
    assert isinstance(image_data[0], dict)
    assert isinstance(image_data[1], list)
    im = image_data[0].copy()
    annotations_this_image = [ann.copy() for ann in image_data[1]]
    input_fn_relative = im['file_name']
    input_fn_abs = os.path.join(input_folder, input_fn_relative)
    if not os.path.isfile(input_fn_abs):
        if unavailable_image_handling == 'error':
            raise FileNotFoundError('Could not find file {}'.format(input_fn_abs))
        print("Can't find image {}, skipping".format(input_fn_relative))
        return None, None
    output_fn_abs = os.path.join(output_folder, input_fn_relative)
    output_dir = os.path.dirname(output_fn_abs)
    if len(output_dir) > 0:
        os.makedirs(output_dir, exist_ok=True)
    if verbose:
        print('Resizing {} to {}'.format(input_fn_abs, output_fn_abs))
    with _reference_truncation_rule():
        try:
            pil_im = open_image(input_fn_abs)
            input_w = pil_im.width
            input_h = pil_im.height
        except Exception as e:
            if unavailable_image_handling == 'error':
                raise Exception('Could not open image {}: {}'.format(input_fn_relative, str(e)))
            print("Can't open image {}, skipping".format(input_fn_relative))
            return None, None
        if correct_size((input_w, input_h), target_size, no_enlarge_width):
            output_w = input_w
            output_h = input_h
            if correct_size_image_handling == 'copy':
                if input_fn_abs != output_fn_abs:
                    shutil.copyfile(input_fn_abs, output_fn_abs)
            elif correct_size_image_handling == 'rewrite':
                exif_preserving_save(pil_im, output_fn_abs)
            else:
                raise ValueError('Unrecognized value {} for correct_size_image_handling'.format(correct_size_image_handling))
        else:
            try:
                pil_im, _ = _resize_image(pil_im, target_size[0], target_size[1], None, no_enlarge_width, False, 'keep')
                output_w = pil_im.width
                output_h = pil_im.height
                exif_preserving_save(pil_im, output_fn_abs, tags_to_exclude=(ORIENTATION,))
            except Exception as e:
                if unavailable_image_handling == 'error':
                    raise Exception('Could not resize image {}: {}'.format(input_fn_relative, str(e)))
                print("Can't resize image {}, skipping".format(input_fn_relative))
                return None, None
    return finish_image(im, annotations_this_image, (input_w, input_h), (output_w, output_h))


# ---- the device leg ----------------------------------------------------------------------------------------------------------------

def plan_job(job, target_size, correct_size_image_handling, no_enlarge_width):
    """What the device needs for one image, before any pixel is decoded (the fields of resize_images.plan_job).  Raises for
    everything the host leg takes: a copy, and whatever the reference would raise for."""
    from PIL import Image
    from . import jpeg_host
    from .device_decode import plan_source
    p, source_size = plan_source(job['input'], job['output'], keep_data=True)
    src = jpeg_host.keep_source(job['input'], p['data'])
    p.pop('data', None)
    own = src['keep']                       # Pillow still calls the image a JPEG: quality 'keep' is its own tables and sampling
    if correct_size(source_size, target_size, no_enlarge_width):
        if correct_size_image_handling != 'rewrite':
            raise HostLeg('a copy, or a value the reference refuses')
        width, height, resized, exif = source_size[0], source_size[1], False, src['exif']
    else:
        width, height, resized = resize_target(source_size, target_size[0], target_size[1], no_enlarge_width)
        if resized:
            assert width > 0 and height > 0, 'Invalid image resize target {},{}'.format(width, height)
            if max(width, height) > 65535:
                raise HostLeg('a side above 65535 pixels')
        else:
            width, height = source_size
        exif = exif_without(Image.open(job['input']), (ORIENTATION,)).tobytes()
    if len(exif) > 65533 or len(src['comment'] or b'') > 65533:
        raise HostLeg('an EXIF block or a comment Pillow refuses')
    if own and not resized:
        if src['quant'] is None:
            raise HostLeg('tables or a sampling the device does not restate')
        job['sampling'], job['quant'] = src['sampling'], src['quant']
    else:
        job['sampling'], job['quant'] = 2, list(jpeg_host.quant_tables(DEFAULT_QUALITY))
    job['probe'], job['source_size'], job['size'], job['resized'] = p, tuple(source_size), (width, height), resized
    job['exif'], job['comment'] = exif, src['comment']
    return job


def _light_job(index, image_data, input_folder, output_folder):
    """an image the device leg may take: its file exists and its header opens; None: the host leg's"""
    from .feed import open_for_coefficients
    relative = image_data[0]['file_name']
    path = os.path.join(input_folder, relative)
    try:
        if not os.path.isfile(path):
            return None
        image, _ = open_for_coefficients(path)
    except Exception:
        return None
    output = os.path.join(output_folder, relative)
    if len(os.path.dirname(output)) > 0:
        os.makedirs(os.path.dirname(output), exist_ok=True)
    return {'index': index, 'input': path, 'output': output, 'bytes': image.size[0] * image.size[1] * 3}


def resize_coco_dataset(input_folder, input_filename, output_folder, output_filename=None, target_size=(-1, -1),
                        correct_size_image_handling='copy', unavailable_image_handling='error', n_workers=1, pool_type='thread',
                        no_enlarge_width=True, verbose=False, backend='gpu', device=0, ctx=None, profile=False, counts=None):
    """resize_coco_dataset of the reference: -> the COCO dict with the resized images, which is what output_filename holds.
    counts: a dict filled in place with COUNT_KEYS (and, with profile, 'ms' per kind of device call)."""
    assert unavailable_image_handling in ('error', 'omit'), 'Illegal unavailable_image_handling {}'.format(unavailable_image_handling)
    assert backend in ('gpu', 'host'), 'Illegal backend: {}'.format(backend)
    with open(input_filename, 'r') as f:
        d = json.load(f)
    image_id_to_annotations = defaultdict(list)
    for ann in d['annotations']:
        image_id_to_annotations[ann['image_id']].append(ann)
    image_annotation_tuples = []
    for im in d['images']:
        annotations_this_image = image_id_to_annotations[im['id']] if im['id'] in image_id_to_annotations else []
        image_annotation_tuples.append((im, annotations_this_image))
    counts = {} if counts is None else counts
    counts.update({k: 0 for k in COUNT_KEYS})
    counts['files'] = len(image_annotation_tuples)
    if profile:
        counts['ms'] = {}
    processed_results = [None] * len(image_annotation_tuples)
    host = list(range(len(image_annotation_tuples)))
    if backend == 'gpu':
        items = [_light_job(i, t, input_folder, output_folder) for i, t in enumerate(image_annotation_tuples)]
        host = [i for i, item in enumerate(items) if item is None]
        items = [item for item in items if item is not None]

        def done(j):
            im, annotations = image_annotation_tuples[j['index']]
            processed_results[j['index']] = finish_image(im.copy(), [ann.copy() for ann in annotations], j['source_size'], j['size'])

        if items:
            import torch
            from .hip_backend import HipContext
            plan = partial(plan_job, target_size=target_size, correct_size_image_handling=correct_size_image_handling,
                           no_enlarge_width=no_enlarge_width)
            with HipContext.images_or(ctx, device) as ctx:
                left = DR.run_chunks(ctx, torch, items, lambda j: j['bytes'], partial(render_chunk, plan=plan, counts=counts, done=done),
                                     counts, profile)
            host = sorted(host + [j['index'] for j in left])
    function = partial(process_single_image, input_folder=input_folder, output_folder=output_folder, target_size=target_size,
                       correct_size_image_handling=correct_size_image_handling, unavailable_image_handling=unavailable_image_handling,
                       no_enlarge_width=no_enlarge_width, verbose=verbose)
    if n_workers <= 1 or not host:
        made = [function(image_annotation_tuples[i]) for i in host]
    else:
        assert pool_type in ('process', 'thread'), 'Illegal pool type {}'.format(pool_type)
        threads = pool_type == 'thread' or backend == 'gpu'
        print('Starting a {} pool of {} workers for image resizing'.format('thread' if threads else 'process', n_workers))
        try:
            made = DR.pool_map(function, [image_annotation_tuples[i] for i in host], n_workers, threads)
        finally:
            print('Pool closed and joined for COCO dataset resizing')
    for i, result in zip(host, made):
        processed_results[i] = result
        counts['host'] += 1
        counts['omitted'] += result[0] is None
    new_images_list = []
    new_annotations_list = []
    for res_im_data, res_annotations in processed_results:
        if res_im_data is None or res_annotations is None:
            assert res_annotations is None and res_im_data is None
            assert unavailable_image_handling == 'omit'
            continue
        new_images_list.append(res_im_data)
        new_annotations_list.extend(res_annotations)
    d['images'] = new_images_list
    d['annotations'] = new_annotations_list
    if output_filename is not None:
        write_json(output_filename, d)
    return d


def main(argv=None):
    parser = argparse.ArgumentParser(description='Resize images in a COCO dataset and scale annotations')
    parser.add_argument('input_folder', type=str, help='Path to the folder containing original images')
    parser.add_argument('input_filename', type=str, help='Path to the input COCO .json file')
    parser.add_argument('output_folder', type=str, help='Path to the folder where resized images will be saved')
    parser.add_argument('output_filename', type=str, help='Path to the output COCO .json file for resized data')
    parser.add_argument('--target_size', type=str, default='-1,-1',
                        help='Target size as "width,height". Use -1 to preserve aspect ratio for a dimension. E.g., "800,600" or "1024,-1".')
    parser.add_argument('--correct_size_image_handling', type=str, default='copy', choices=['copy', 'rewrite'],
                        help='How to handle images already at target size')
    parser.add_argument('--n_workers', type=int, default=1, help='Number of workers for parallel processing. <=1 for sequential')
    parser.add_argument('--pool_type', type=str, default='thread', choices=['thread', 'process'], help='Type of multiprocessing pool if n_workers > 1')
    parser.add_argument('--backend', choices=('gpu', 'host'), default='gpu')
    parser.add_argument('--device', type=int, default=0)
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    try:
        target_size_parts = args.target_size.split(',')
        if len(target_size_parts) != 2:
            raise ValueError('target_size must have two comma-separated parts (width,height).')
        parsed_target_size = (int(target_size_parts[0]), int(target_size_parts[1]))
    except ValueError as e:
        print('Error parsing target_size: {}'.format(e))
        parser.print_help()
        parser.exit()
    resize_coco_dataset(args.input_folder, args.input_filename, args.output_folder, args.output_filename, target_size=parsed_target_size,
                        correct_size_image_handling=args.correct_size_image_handling, n_workers=args.n_workers, pool_type=args.pool_type,
                        backend=args.backend, device=args.device)
    print('Dataset resizing complete')
    return 0


if __name__ == '__main__':
    sys.exit(main())
