"""
Tiled inference for images much larger than the network input (aerial / drone surveys, high-resolution camera traps
with small animals): the counterpart of the reference's detection/run_tiled_inference.py.

Every image is split into tiles of tile_size_x x tile_size_y pixels with a fractional overlap, the detector runs on the
tiles, tile detections are mapped back to the image and de-duplicated across overlapping tiles (class-agnostic NMS at
IoU 0.45).  Parameter names, defaults, output JSON and the intermediate JSON files are the reference's.

What differs: the reference crops every tile with PIL, writes it as a quality-95 JPEG into the tiling folder and runs the
batch driver on that folder.  Here an image is decoded and uploaded to the GPU once; every tile is cut out of the device
image by the windowed letterbox kernels (HIPDetector.generate_detections_for_tiles).  No tile file is ever written, so
  * BY DEFAULT the detector sees the SOURCE pixels, not pixels that went through a JPEG encode / decode;
  * with tile_jpeg_quality=95 (--tile_jpeg_quality 95; extra, off by default) every tile goes through that JPEG round
    trip on the GPU (mdhip_jpeg_recompress: libjpeg's integer arithmetic, no file, no entropy coder) and the detector
    sees the reference's tile pixels, bit for bit what PIL reads back from the tile file it would have written.  PINNED:
    tests/test_tile_jpeg_cpu.py (the arithmetic against Pillow, coefficient by coefficient) and
    tests/test_gpu_tile_jpeg.py (the kernels, the network input, and a run against tile files written with PIL);
  * what the default's difference does to detections of the real weights remains NOT PINNED (no real weights here);
  * `patch_fn` in <folder>_patch_info.json is the path the tile WOULD have.

Parameters of the reference that have no meaning without tile files:
  accepted and ignored:   remove_tiles, overwrite_tiles, load_cached_tiles_if_available, n_patch_extraction_workers,
                          pool_type (validated), use_image_queue, preprocess_on_image_queue
  raise ValueError:       yolo_inference_options (run_inference_with_yolov5_val is not part of this package),
                          create_tiles_only (there are no tiles to create)
Multi-GPU sharding by image is not implemented here.

  python -m megadetector_amd.run_tiled_inference MODEL IMAGE_FOLDER TILING_FOLDER OUTPUT.json [--tile_overlap 0.5] ...
"""

import argparse
import json
import os
import sys
import tempfile
import uuid
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import run_detector
from .constants import CONF_DIGITS, COORD_DIGITS, DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD
from .feed import load_image
from .jpeg_host import check_quality
from .ref_utils import clean_filename
from .run_detector_batch import (default_loaders, find_images, load_checkpoint, parse_kvp_list, write_checkpoint,
                                 write_json, write_results_to_file)

default_patch_overlap = 0.5
nms_iou_threshold = 0.45            # de-duplication of detections from overlapping tiles, not the model's own NMS
default_tile_size = [1280, 1280]
default_n_patch_extraction_workers = 1
default_pool_type = 'thread'

def get_patch_boundaries(image_size, patch_size, patch_stride=None):
    """
    Upper-left corners [x, y] of the tiles of a (w, h) image, row by row.  Tiles advance by the stride; the last tile of
    a row / column is moved back so that it ends flush with the image (a 15 px wide image, 10 px tiles, stride 10:
    x = 0 and x = 5).  patch_stride: (x, y), or a float = fraction of the tile size; default half a tile.
    """
    if patch_stride is None:
        patch_stride = (round(patch_size[0] * (1.0 - default_patch_overlap)),
                        round(patch_size[1] * (1.0 - default_patch_overlap)))
    elif isinstance(patch_stride, float):
        patch_stride = (round(patch_size[0] * patch_stride), round(patch_size[1] * patch_stride))
    for axis, name in ((0, 'width'), (1, 'height')):
        assert patch_size[axis] <= image_size[axis], 'Patch {} {} is larger than image {} {}'.format(
            name, patch_size[axis], name, image_size[axis])

    def starts(length, size, stride):
        out, s = [], 0
        while True:
            out.append(s)
            if s + size == length:
                return out
            s += stride
            if s + size > length:
                out.append(length - size)
                return out

    xs = starts(image_size[0], patch_size[0], patch_stride[0])
    ys = starts(image_size[1], patch_size[1], patch_stride[1])
    positions = [[x, y] for y in ys for x in xs]
    assert len(set(tuple(p) for p in positions)) == len(positions), 'Patch generation error (duplicate start position)'
    return positions


def patch_info_to_patch_name(image_name, patch_x_min, patch_y_min):
    """("a.jpg", 10, 20) -> "a.jpg_0010_0020" """
    return image_name + '_' + str(patch_x_min).zfill(4) + '_' + str(patch_y_min).zfill(4)


def tiles_for_image(fn_relative, image_size, tiling_folder, patch_size, patch_stride):
    """The reference's per-image patch record (without writing the tiles): {'patches', 'image_fn', 'error'}"""
    image_name = clean_filename(fn_relative, char_limit=None, force_lower=True)
    patches, error = [], None
    try:
        for x, y in get_patch_boundaries(image_size, patch_size, patch_stride):
            patches.append({'xmin': x, 'xmax': x + patch_size[0] - 1, 'ymin': y, 'ymax': y + patch_size[1] - 1,
                            'patch_fn': os.path.join(tiling_folder, patch_info_to_patch_name(image_name, x, y) + '.jpg'),
                            'source_fn': fn_relative})
    except Exception as e:
        error = 'Patch generation error for {}: \n{}'.format(fn_relative, str(e))
        print(error)
    return {'patches': patches, 'image_fn': fn_relative, 'error': error}


def merge_tile_results(image_fn_relative, image_size, patches, tile_results, patch_size):
    """
    Tile-level results -> one image-level record (before the cross-tile NMS).  tile_results[i] belongs to patches[i] and
    is an entry of the tile-level results file (detections sorted by descending conf).  Tile-normalised boxes go to
    pixels, get the tile origin added and are divided by the image size, in float64 and in the reference's operation
    order; one failed tile makes the image a failure carrying that tile's failure string.
    """
    image_w, image_h = image_size
    output_im = {'file': image_fn_relative, 'detections': []}
    for patch_info, patch_results in zip(patches, tile_results):
        patch_w = (patch_info['xmax'] - patch_info['xmin']) + 1
        patch_h = (patch_info['ymax'] - patch_info['ymin']) + 1
        assert patch_w == patch_size[0] and patch_h == patch_size[1]
        if patch_results.get('detections') is None:
            assert 'failure' in patch_results
            output_im['detections'] = None
            output_im['failure'] = patch_results['failure']
            break
        for det in patch_results['detections']:
            bx, by, bw, bh = det['bbox']
            w_pixels = bw * patch_w
            h_pixels = bh * patch_h
            xmin_image_pixels = patch_info['xmin'] + bx * patch_w
            ymin_image_pixels = patch_info['ymin'] + by * patch_h
            bbox = [xmin_image_pixels / image_w, ymin_image_pixels / image_h, w_pixels / image_w, h_pixels / image_h]
            output_im['detections'].append({'bbox': [round(v, COORD_DIGITS) for v in bbox],
                                            'conf': round(det['conf'], CONF_DIGITS),
                                            'category': det['category']})
    return output_im


def greedy_nms(boxes, scores, iou_thres):
    """torchvision.ops.nms on the host: float32 [x1, y1, x2, y2] boxes, stable descending score order, a box goes when its
    IoU with a kept box is ABOVE the threshold; returns the kept indices in kept order"""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32)
    order = np.argsort(-scores, kind='stable')
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    suppressed = np.zeros(len(boxes), dtype=bool)
    keep = []
    for pos, i in enumerate(order):
        if suppressed[i]:
            continue
        keep.append(int(i))
        rest = order[pos + 1:]
        if len(rest) == 0:
            break
        xx1 = np.maximum(boxes[i, 0], boxes[rest, 0])
        yy1 = np.maximum(boxes[i, 1], boxes[rest, 1])
        xx2 = np.minimum(boxes[i, 2], boxes[rest, 2])
        yy2 = np.minimum(boxes[i, 3], boxes[rest, 3])
        w = np.maximum(np.float32(0), xx2 - xx1)
        h = np.maximum(np.float32(0), yy2 - yy1)
        inter = w * h
        iou = inter / (areas[i] + areas[rest] - inter)
        suppressed[rest[iou > np.float32(iou_thres)]] = True
    return keep


def in_place_nms(md_results, iou_thres=nms_iou_threshold, verbose=True):
    """class-agnostic de-duplication of every image's detections, in place; survivors in kept (descending conf) order"""
    before = after = 0
    for im in md_results['images']:
        if im['detections'] is None or len(im['detections']) == 0:
            continue
        before += len(im['detections'])
        boxes = [[d['bbox'][0], d['bbox'][1], d['bbox'][0] + d['bbox'][2], d['bbox'][1] + d['bbox'][3]]
                 for d in im['detections']]
        keep = greedy_nms(boxes, [d['conf'] for d in im['detections']], iou_thres)
        im['detections'] = [im['detections'][i] for i in keep]
        after += len(im['detections'])
    if verbose:
        print('NMS removed {} of {} detections'.format(before - after, before))


def _resolve_image_files(image_folder, image_list):
    if image_list is None:
        print('Enumerating images in {}'.format(image_folder))
        files = [os.path.relpath(f, image_folder) for f in find_images(image_folder, recursive=True)]
        assert len(files) > 0, 'No images found in folder {}'.format(image_folder)
        return files
    print('Loading image list from {}'.format(image_list))
    with open(image_list, 'r') as f:
        files = json.load(f)
    n_absolute = 0
    for i, fn in enumerate(files):
        if os.path.isabs(fn):
            n_absolute += 1
            rel = os.path.relpath(fn, image_folder)
            if rel.startswith('..'):
                raise ValueError('Illegal absolute path supplied to run_tiled_inference, {} is outside of {}'.format(
                    fn, image_folder))
            files[i] = rel
    if n_absolute not in (0, len(files)):
        raise ValueError('Illegal file list: converted {} of {} paths to relative'.format(n_absolute, len(files)))
    return files


def _tile_level_results(detector, image, patches, confidence_threshold, inference_size, augment, tile_jpeg_quality=None):
    """runs the detector on the tiles of one image; returns the per-tile result dicts (file = the tile's would-be path)"""
    names = [p['patch_fn'] for p in patches]
    origins = [(p['xmin'], p['ymin']) for p in patches]
    size = (patches[0]['xmax'] - patches[0]['xmin'] + 1, patches[0]['ymax'] - patches[0]['ymin'] + 1)
    extra = {} if tile_jpeg_quality is None else {'jpeg_quality': tile_jpeg_quality}
    try:
        results = detector.generate_detections_for_tiles(image, origins, size, tile_ids=names, image_size=inference_size,
                                                         augment=augment, **extra)
    except Exception as e:
        print('Warning: tile inference failed for an image: {}'.format(str(e)))
        return [{'file': n, 'failure': run_detector.FAILURE_INFER} for n in names]
    out = []
    for r in results:
        if r.get('failure') is not None:
            out.append({'file': r['file'], 'failure': r['failure']})
            continue
        # (the batched detector call gets no threshold: it is applied to its output, as the batch driver does)
        r['detections'] = [d for d in r['detections'] if d['conf'] >= confidence_threshold]
        out.append(r)
    return out


def run_tiled_inference(model_file, image_folder, tiling_folder, output_file, tile_size_x=1280, tile_size_y=1280,
                        tile_overlap=0.5, checkpoint_path=None, checkpoint_frequency=-1, remove_tiles=False,
                        yolo_inference_options=None, n_patch_extraction_workers=default_n_patch_extraction_workers,
                        overwrite_tiles=True, image_list=None, augment=False, detector_options=None,
                        use_image_queue=True, preprocess_on_image_queue=True, loader_workers=default_loaders,
                        inference_size=None, verbose=False, pool_type=None, load_cached_tiles_if_available=False,
                        create_tiles_only=False, detector=None, tile_jpeg_quality=None):
    """
    See the module docstring.  `detector` (extra, optional) injects an already constructed detector object.
    `tile_jpeg_quality` (extra, 1 .. 100, default None = off): tiles go through a JPEG round trip at that quality on the
    GPU before the detector sees them; 95 is the reference's patch_jpeg_quality.
    Checkpoints hold one record per finished IMAGE ({'file', 'size', 'tiles': tile-level results, files relative to
    the tiling folder}, and 'tile_jpeg_quality' when that switch is on); a checkpoint made with another setting of the
    switch is refused.
    Returns the image-level results dict that is written to output_file.
    """
    assert 0 <= tile_overlap < 1, 'Illegal tile overlap value {}'.format(tile_overlap)
    if yolo_inference_options is not None:
        raise ValueError('yolo_inference_options: run_inference_with_yolov5_val is not part of this package')
    if create_tiles_only:
        raise ValueError('create_tiles_only: tiles are cut on the GPU and never written, there is nothing to create')
    if tile_jpeg_quality is not None:
        tile_jpeg_quality = check_quality(tile_jpeg_quality)
    if tile_size_x == -1:
        tile_size_x = default_tile_size[0]
    if tile_size_y == -1:
        tile_size_y = default_tile_size[1]
    patch_size = [tile_size_x, tile_size_y]
    patch_stride = (round(patch_size[0] * (1.0 - tile_overlap)), round(patch_size[1] * (1.0 - tile_overlap)))
    assert (pool_type or default_pool_type) in ('thread', 'process'), 'Illegal pool type {}'.format(pool_type)
    write_intermediates = tiling_folder is not None
    if tiling_folder is None:
        tiling_folder = os.path.join(tempfile.gettempdir(), 'md-tiling', str(uuid.uuid1()))    # names only: never created
    else:
        os.makedirs(tiling_folder, exist_ok=True)
    if isinstance(detector_options, (list, str)):
        detector_options = parse_kvp_list(detector_options)
    detector_options = dict(detector_options or {})
    if checkpoint_path is None or checkpoint_frequency is None:
        checkpoint_frequency = -1

    image_files_relative = _resolve_image_files(image_folder, image_list)
    folder_name = clean_filename(image_folder, force_lower=True)
    if folder_name.startswith('_'):
        folder_name = folder_name[1:]

    if detector is None:
        size = max(int(inference_size or 0), int(detector_options.get('max_image_size', 0) or 0))
        if size:
            detector_options['max_image_size'] = size
        detector_options.setdefault('max_batch', 32)
        detector = run_detector.load_detector(model_file, detector_options=detector_options, verbose=verbose)

    done = {}
    if checkpoint_path is not None and os.path.isfile(checkpoint_path):
        done = {r['file']: r for r in load_checkpoint(checkpoint_path)}
        other = sorted({str(r.get('tile_jpeg_quality')) for r in done.values() if r.get('tile_jpeg_quality') != tile_jpeg_quality})
        if other:
            raise ValueError('checkpoint {} holds records made with tile_jpeg_quality {}, this run uses {}: results of two '
                             'settings are not mixed'.format(checkpoint_path, ', '.join(other), tile_jpeg_quality))
    records = []                                   # per image, in input order: {'file', 'size', 'tiles' | 'load_failure'}

    def load(fn_relative):
        try:
            image = load_image(os.path.join(image_folder, fn_relative))
            return image, None
        except Exception as e:
            return None, str(e)

    n_new = 0
    todo = [fn for fn in image_files_relative if fn not in done]
    pool = ThreadPoolExecutor(max_workers=1) if (loader_workers or 0) > 0 and len(todo) > 1 else None
    try:
        pending = pool.submit(load, todo[0]) if pool is not None and todo else None     # image i + 1 decodes while image i runs
        i_todo = 0
        for fn_relative in image_files_relative:
            if fn_relative in done:
                records.append(done[fn_relative])
                continue
            image, load_error = pending.result() if pending is not None else load(fn_relative)
            i_todo += 1
            if pool is not None:
                pending = pool.submit(load, todo[i_todo]) if i_todo < len(todo) else None
            rec = {'file': fn_relative}
            if tile_jpeg_quality is not None:
                rec['tile_jpeg_quality'] = tile_jpeg_quality
            if image is None:
                rec['size'] = None
                rec['load_failure'] = load_error
            else:
                rec['size'] = [image.width, image.height]
                info = tiles_for_image(fn_relative, rec['size'], tiling_folder, patch_size, patch_stride)
                rec['tiles'] = [] if info['error'] is not None else _tile_level_results(
                    detector, image, info['patches'], DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD, inference_size, augment,
                    tile_jpeg_quality)
                for t in rec['tiles']:              # (a checkpoint may be resumed with another tiling folder)
                    t['file'] = os.path.relpath(t['file'], tiling_folder)
            records.append(rec)
            n_new += 1
            if checkpoint_frequency > 0 and n_new % checkpoint_frequency == 0:
                print('Writing a new checkpoint after having processed {} images since last restart'.format(n_new))
                write_checkpoint(checkpoint_path, records)
    finally:
        if pool is not None:
            pool.shutdown(wait=True)

    # patch records and tile-level results, as the reference writes them
    all_image_patch_info, tile_level = [], []
    for rec in records:
        if rec['size'] is None:
            info = {'patches': [], 'image_fn': rec['file'],
                    'error': 'Patch generation error for {}: \n{}'.format(rec['file'], rec['load_failure'])}
        else:
            info = tiles_for_image(rec['file'], rec['size'], tiling_folder, patch_size, patch_stride)
            tile_level.extend(dict(t, file=os.path.join(tiling_folder, t['file'])) for t in rec['tiles'])
        all_image_patch_info.append(info)
    job_guid = str(uuid.uuid1())
    prefix = os.path.join(tiling_folder, folder_name + '_')
    if write_intermediates:
        write_json(prefix + 'patch_info.json', all_image_patch_info)
        patch_level_file = prefix + job_guid + '_patch_level_results.json'
    else:
        patch_level_file = os.path.join(tempfile.gettempdir(), 'md_tiled_{}_patch_level_results.json'.format(job_guid))
    patch_level_results = write_results_to_file(tile_level, patch_level_file, relative_path_base=tiling_folder,
                                                detector_file=model_file)
    if not write_intermediates:
        os.remove(patch_level_file)
    by_file = {im['file']: im for im in patch_level_results['images']}

    image_level_results = {'info': patch_level_results['info'],
                           'detection_categories': patch_level_results['detection_categories'], 'images': []}
    for rec, info in zip(records, all_image_patch_info):
        if info['error'] is not None:
            image_level_results['images'].append({'file': rec['file'], 'detections': None,
                                                  'failure': 'Patch generation error', 'failure_details': info['error']})
            continue
        tiles = [by_file[os.path.relpath(p['patch_fn'], tiling_folder).replace('\\', '/')] for p in info['patches']]
        image_level_results['images'].append(merge_tile_results(rec['file'], rec['size'], info['patches'], tiles, patch_size))
    if write_intermediates:
        with open(prefix + job_guid + '_image_level_results_pre_nms.json', 'w') as f:
            json.dump(image_level_results, f, indent=1)

    in_place_nms(image_level_results, iou_thres=nms_iou_threshold)

    print('Saving image-level results (after NMS) to {}'.format(output_file))
    parent_dir = os.path.dirname(output_file)
    if len(parent_dir) > 0:
        os.makedirs(parent_dir, exist_ok=True)
    with open(output_file, 'w') as f:
        json.dump(image_level_results, f, indent=1)
    return image_level_results


def main(argv=None):
    parser = argparse.ArgumentParser(
        description='Chop a folder of images up into tiles, run MD on the tiles, and stitch the results together')
    parser.add_argument('model_file', help='Path to detector model file (.pt)')
    parser.add_argument('image_folder', help='Folder containing images for inference (always recursive, unless image_list is supplied)')
    parser.add_argument('tiling_folder', help='Folder where intermediate results will be stored (no tile images are written)')
    parser.add_argument('output_file', help='Path to output JSON results file, should end with a .json extension')
    parser.add_argument('--no_remove_tiles', action='store_true', help='Accepted for compatibility: there are no tile files to remove')
    parser.add_argument('--augment', action='store_true', help='Enable test-time augmentation')
    parser.add_argument('--verbose', action='store_true', help='Enable additional debug output')
    parser.add_argument('--tile_size_x', type=int, default=default_tile_size[0], help='Tile width (defaults to {})'.format(default_tile_size[0]))
    parser.add_argument('--tile_size_y', type=int, default=default_tile_size[1], help='Tile height (defaults to {})'.format(default_tile_size[1]))
    parser.add_argument('--tile_overlap', type=float, default=default_patch_overlap, help='Overlap between tiles [0,1] (defaults to {})'.format(default_patch_overlap))
    parser.add_argument('--overwrite_handling', type=str, default='skip', help='Behavior when the target file exists (skip/overwrite/error) (default skip)')
    parser.add_argument('--image_list', type=str, default=None, help='A .json list of relative filenames (or absolute paths contained within image_folder) to include')
    parser.add_argument('--detector_options', nargs='*', metavar='KEY=VALUE', default=None, help='A list of detector options (key-value pairs)')
    parser.add_argument('--inference_size', type=int, default=None, help='Run inference at a non-default size')
    parser.add_argument('--n_patch_extraction_workers', type=int, default=1, help='Accepted for compatibility (tiles are cut on the GPU)')
    parser.add_argument('--loader_workers', type=int, default=default_loaders, help='0 disables decoding the next image while the current one is on the GPU')
    parser.add_argument('--tile_jpeg_quality', type=int, default=None, metavar='Q',
                        help='Pass every tile through a JPEG round trip at quality Q (1-100) on the GPU before detection: the pixels of '
                             'the tile files the reference writes.  The reference\'s value is 95.  Default: off, detect on the source pixels')
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    model_file = run_detector.try_download_known_detector(args.model_file)
    if os.path.exists(args.output_file):
        if args.overwrite_handling == 'skip':
            print('Warning: output file {} exists, skipping'.format(args.output_file))
            return
        elif args.overwrite_handling == 'overwrite':
            print('Warning: output file {} exists, overwriting'.format(args.output_file))
        elif args.overwrite_handling == 'error':
            raise ValueError('Output file {} exists'.format(args.output_file))
        else:
            raise ValueError('Unknown output handling method {}'.format(args.overwrite_handling))
    run_tiled_inference(model_file, args.image_folder, args.tiling_folder, args.output_file,
                        tile_size_x=args.tile_size_x, tile_size_y=args.tile_size_y, tile_overlap=args.tile_overlap,
                        remove_tiles=not args.no_remove_tiles, image_list=args.image_list, augment=args.augment,
                        detector_options=parse_kvp_list(args.detector_options), inference_size=args.inference_size,
                        verbose=args.verbose, n_patch_extraction_workers=args.n_patch_extraction_workers,
                        loader_workers=args.loader_workers, use_image_queue=args.loader_workers > 0,
                        tile_jpeg_quality=args.tile_jpeg_quality)


if __name__ == '__main__':
    main()
