"""
Change detection between consecutive camera images (reference: megadetector/detection/change_detection.py), for time-lapse and
burst series whose background is stable: per camera folder every image is compared with the one before it -- gray, blur,
absolute difference, threshold, dilation, connected regions -- and gets one CSV row.

    python -m megadetector_amd.change_detection --root_dir D [--output_csv F ... --backend gpu|host --device 0]

RESTATED statement for statement: the image list of a camera (path_utils.find_images: a recursive glob, extension filter,
sorted), the first image's row, the pair loop, the unreadable-image rule (such a pair gets the empty result, and so does the
next pair, whose previous image it is), the `regions` string, the seven columns, the CSV text of DataFrame.to_csv(index=False)
(written without pandas), the summary lines, the previews' sampling.

OURS: the arithmetic.  OpenCV is not available to this project, so every numeric step is defined in integers by
csrc/change_detect.h and computed either by mdhip_change_detect on the GPU (backend='gpu') or by its host model
mdjpeg_change_detect (backend='host'); both give the same rows.  NOT VERIFIED AGAINST OPENCV: the gray constants, the blur
coefficients (OpenCV's rounding of a Gaussian kernel could not be read), and whether cv2.imread gives the pixels Pillow gives
(ours are the project's decode: Pillow's, after EXIF rotation).  Two DELIBERATE DIFFERENCES: a region's area is its PIXEL
COUNT, where cv2.contourArea is the area of the polygon through the border pixels' centres (smaller by about half the border
length, so min_area bites a little earlier in the reference); and regions are listed by ascending label (the smallest raster index
of their pixels), where the order of cv2.findContours is not known to this project.  Also ours: a pair of images of different
sizes gets the empty result and a warning (in the reference cv2.absdiff raises and the camera folder is lost); `workers` sizes
the host leg's pool and is ignored by the gpu leg; results are lists of row dicts, not DataFrames; options outside the ranges
of csrc/change_detect.h are a ValueError.

NOT RESTATED, NotImplementedError before anything is read: DetectionMethod.MOG2 / KNN / MOTION_HISTORY, ThresholdType.ADAPTIVE,
verbose's debug_images, stop_at_token, and create_change_previews (the reference draws with OpenCV's Hershey font).

The gpu leg walks the images of all cameras in decode chunks (device_render.chunked, device_decode.decode_chunk), makes ONE
mdhip_change_detect call per chunk for all its pairs, and carries each camera's last blurred plane into the next chunk, so
every image is decoded, converted and blurred once.  A pair with more significant regions than REGION_CAP is done again by the
host model and counted in 'host_pairs'.
"""

import argparse
import csv
import io
import os
import random
import sys
from dataclasses import dataclass
from enum import Enum, auto
from pathlib import Path
from typing import Optional

from .ref_utils import find_images

#: significant regions a pair's device result has room for; a pair with more goes to the host model
REGION_CAP = 256
COLUMNS = ('camera', 'image', 'prev_image', 'motion_detected', 'diff_percentage', 'num_regions', 'regions')


class DetectionMethod(Enum):
    FRAME_DIFF = auto()
    MOG2 = auto()
    KNN = auto()
    MOTION_HISTORY = auto()


class ThresholdType(Enum):
    GLOBAL = auto()
    ADAPTIVE = auto()
    OTSU = auto()


@dataclass
class ChangeDetectionOptions:
    """the reference's options, with its defaults"""
    min_area: int = 500
    threshold: int = 25
    detection_method: DetectionMethod = DetectionMethod.FRAME_DIFF
    threshold_type: ThresholdType = ThresholdType.GLOBAL
    blur_kernel_size: int = 21
    dilate_kernel_size: int = 5
    history: int = 25
    var_threshold: float = 16
    detect_shadows: bool = False
    adaptive_block_size: int = 11
    adaptive_c: int = 2
    mhi_duration: float = 10.0
    mhi_threshold: int = 30
    mhi_buffer_size: int = 20
    ignore_fraction: Optional[float] = None
    dilate_iterations: int = 2
    workers: int = 4
    verbose: bool = False
    stop_at_token: str = None


def check_options(options, backend='host'):
    """NotImplementedError for what is not restated, ValueError for values the arithmetic is not defined for; -> the option
    record of the two entry points"""
    from . import jpeg_host
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    if options.detection_method != DetectionMethod.FRAME_DIFF:
        raise NotImplementedError('detection_method {}: only FRAME_DIFF is restated'.format(options.detection_method.name))
    if options.threshold_type == ThresholdType.ADAPTIVE:
        raise NotImplementedError('ThresholdType.ADAPTIVE is not restated')
    if options.verbose:
        raise NotImplementedError("verbose: the reference's debug_images are not restated")
    if options.stop_at_token is not None:
        raise NotImplementedError('stop_at_token is not restated')
    k, d = options.blur_kernel_size, options.dilate_kernel_size
    if not (isinstance(k, int) and 1 <= k <= 127 and k % 2 == 1):
        raise ValueError('blur_kernel_size must be odd and 1 .. 127')
    if not (1 <= d <= 33 and 0 <= options.dilate_iterations <= 64):
        raise ValueError('dilate_kernel_size must be 1 .. 33 and dilate_iterations 0 .. 64')
    if not (0 <= options.threshold <= 255 and options.min_area >= 0):
        raise ValueError('threshold must be 0 .. 255 and min_area >= 0')
    if options.ignore_fraction is not None and not -1.0 <= options.ignore_fraction <= 1.0:
        raise ValueError('ignore_fraction must be between -1.0 and 1.0')
    return jpeg_host.change_options(k, 1 if options.threshold_type == ThresholdType.OTSU else 0, options.threshold, d,
                                    options.dilate_iterations, options.min_area, options.ignore_fraction, REGION_CAP)


def empty_result():
    return {'motion_detected': False, 'motion_regions': [], 'diff_percentage': 0.0, 'debug_images': {}}


def pair_result(size, count, regions, options):
    """detect_motion's return value from a pair's integers: size (width, height), the thresholded count, the significant
    regions (x, y, w, h, ...) in order"""
    w, h = size
    if options.ignore_fraction is not None:
        ignore_rows = int(abs(options.ignore_fraction) * h)
        roi_area = (h - ignore_rows) * w if options.ignore_fraction != 0 else h * w
        diff_percentage = (int(count) / roi_area) * 100 if roi_area > 0 else 0
    else:
        diff_percentage = (int(count) / (h * w)) * 100
    out = empty_result()
    out['motion_detected'] = len(regions) > 0
    out['motion_regions'] = [tuple(int(v) for v in r[:4]) for r in regions]
    out['diff_percentage'] = diff_percentage
    return out


def _load_rgb(path):
    """the project's decode (Pillow's pixels after EXIF rotation) as an (h, w, 3) array, or None for a file that cannot be read"""
    import numpy as np
    from .feed import load_image
    try:
        return np.ascontiguousarray(np.asarray(load_image(str(path))))
    except Exception:
        return None


def _host_pair(prev, curr, record):
    """the host model on one pair of arrays, with room for every region"""
    from . import jpeg_host
    from copy import copy
    rec = copy(record)
    while True:
        res = jpeg_host.change_detect([prev, curr], [(0, 1)], rec)
        if not res['overflow'][0]:
            n = int(res['n_regions'][0])
            return int(res['counts'][0]), res['regions'][0][:n]
        rec.region_cap = min(65536, max(int(res['n_regions'][0]), 2 * rec.region_cap))
        if rec.region_cap == 65536 and int(res['n_regions'][0]) > 65536:
            raise RuntimeError('more than 65536 significant regions in one pair')


def _detect_arrays(prev, curr, prev_path, curr_path, options, record):
    """detect_motion's result for two decoded images (None: unreadable), host model"""
    if curr is None:
        print('Could not read image: {}'.format(curr_path))
        return empty_result()
    if prev is None:
        print('Could not read image: {}'.format(prev_path))
        return empty_result()
    if prev.shape != curr.shape:
        print('Warning: {} and {} differ in size, no change is reported'.format(prev_path, curr_path))
        return empty_result()
    count, regions = _host_pair(prev, curr, record)
    return pair_result((curr.shape[1], curr.shape[0]), count, regions, options)


def detect_motion(prev_image_path, curr_image_path, options=None, backend='host', device=0):
    """Motion between two images -> {'motion_detected', 'motion_regions': [(x, y, w, h)], 'diff_percentage', 'debug_images': {}}.
    (The reference returns (result, motion_state); there is no motion state here.)"""
    if options is None:
        options = ChangeDetectionOptions()
    record = check_options(options, backend)
    if prev_image_path is None:                     # FRAME_DIFF without a previous image: the current one is read, nothing else
        if _load_rgb(curr_image_path) is None:
            print('Could not read image: {}'.format(curr_image_path))
        return empty_result()
    if backend == 'gpu':
        rows, _ = _gpu_rows([('', [str(prev_image_path), str(curr_image_path)])], options, record, device)
        row = rows[1]
        regions = [tuple(int(v) for v in r.split(',')) for r in row['regions'].split(';') if r]
        return {'motion_detected': row['motion_detected'], 'motion_regions': regions, 'diff_percentage': row['diff_percentage'],
                'debug_images': {}}
    return _detect_arrays(_load_rgb(prev_image_path), _load_rgb(curr_image_path), prev_image_path, curr_image_path, options, record)


def first_row(camera_name, first_image):
    return {'camera': camera_name, 'image': str(first_image), 'prev_image': None, 'motion_detected': False, 'diff_percentage': 0.0,
            'num_regions': 0, 'regions': ''}


def result_row(camera_name, prev_image, curr_image, motion_result):
    regions = motion_result['motion_regions']
    return {'camera': camera_name, 'image': str(curr_image), 'prev_image': str(prev_image),
            'motion_detected': motion_result['motion_detected'], 'diff_percentage': motion_result['diff_percentage'],
            'num_regions': len(regions), 'regions': ';'.join(['{},{},{},{}'.format(x, y, w, h) for x, y, w, h in regions])}


def _camera_images(folder_path):
    folder_path = Path(folder_path)
    camera_name = folder_path.name
    image_files = find_images(folder_path, recursive=True)
    if len(image_files) == 0:
        print('No images found in {}'.format(folder_path))
    else:
        print('Processing {} images in {}'.format(len(image_files), camera_name))
    return camera_name, image_files


def _host_camera(camera_name, image_files, options, record):
    """the reference's loop over one camera, every image decoded once"""
    results = []
    if len(image_files) > 0:
        results.append(first_row(camera_name, image_files[0]))
    prev = _load_rgb(image_files[0]) if len(image_files) > 1 else None
    for i_image in range(1, len(image_files)):
        prev_image, curr_image = image_files[i_image - 1], image_files[i_image]
        curr = _load_rgb(curr_image)
        results.append(result_row(camera_name, prev_image, curr_image, _detect_arrays(prev, curr, prev_image, curr_image, options, record)))
        prev = curr
    return results


def _host_camera_job(args):
    return _host_camera(*args)


def process_camera_folder(folder_path, options=None, backend='host', device=0):
    """All images of one camera folder -> its rows (the reference returns them as a DataFrame)"""
    if options is None:
        options = ChangeDetectionOptions()
    record = check_options(options, backend)
    camera_name, image_files = _camera_images(folder_path)
    if backend == 'gpu':
        return _gpu_rows([(camera_name, image_files)], options, record, device)[0]
    return _host_camera(camera_name, image_files, options, record)


def _gpu_rows(cameras, options, record, device=0, counts=None, clock_ms=None):
    """The gpu leg: cameras [(name, files)] -> (rows in the cameras' order, counts)"""
    import numpy as np
    import torch
    from . import device_decode, device_render
    from .hip_backend import HipContext
    counts = counts if counts is not None else {}
    for key in ('gpu_pairs', 'host_pairs', 'pil_decodes'):
        counts.setdefault(key, 0)
    ctx = HipContext.for_images(device)
    dev = torch.device('cuda', device)
    clock = device_render.Clock(torch, dev, clock_ms)
    # every image once, in the cameras' order: (camera index, index in its camera, file)
    items, probes = [], {}
    for c, (_, files) in enumerate(cameras):
        for k, f in enumerate(files):
            if len(files) < 2:
                continue                            # a single image is never read
            try:
                probes[f] = device_decode.probe(f)
            except Exception:
                probes[f] = None
            items.append((c, k, f))
    size_of = lambda it: 3 * probes[it[2]]['size'][0] * probes[it[2]]['size'][1] if probes[it[2]] else 0
    results = {}                                    # (camera, k) -> detect_motion's result for the pair (k - 1, k)
    carried = {}                                    # camera -> (k, size, blurred plane) of its last readable image so far, or (k, None, None)
    try:
        for chunk in device_render.chunked(items, size_of, device_render.DECODE_CHUNK_BYTES):
            readable = [it[2] for it in chunk if probes[it[2]] is not None]
            dec = {'files_decoded_gpu': 0, 'files_decoded_pil': 0}
            with clock('decode'):
                pixels, _ = device_decode.decode_chunk(ctx, torch, dev, '', readable, probes, dec)
            counts['pil_decodes'] += dec['files_decoded_pil']
            # the call's images: this chunk's decoded ones, and the carried planes of the cameras it continues
            ptrs, sizes, planes, ready, index_of = [], [], [], [], {}
            for c, k, f in chunk:
                if k > 0 and (c, k - 1) not in index_of and c in carried and carried[c][0] == k - 1 and carried[c][1] is not None:
                    index_of[(c, k - 1)] = len(ptrs)
                    ptrs.append(0), sizes.append(carried[c][1]), planes.append(carried[c][2]), ready.append(1)
                if f in pixels:
                    w, h = probes[f]['size']
                    index_of[(c, k)] = len(ptrs)
                    ptrs.append(pixels[f].data_ptr()), sizes.append((w, h)), ready.append(0)
                    planes.append(torch.empty(w * h, dtype=torch.uint8, device=dev))
            pairs, pair_keys = [], []
            for c, k, f in chunk:
                if k == 0:
                    continue
                files = cameras[c][1]
                if (c, k) not in index_of:
                    print('Could not read image: {}'.format(f))
                    results[(c, k)] = empty_result()
                elif (c, k - 1) not in index_of:
                    print('Could not read image: {}'.format(files[k - 1]))
                    results[(c, k)] = empty_result()
                elif sizes[index_of[(c, k - 1)]] != sizes[index_of[(c, k)]]:
                    print('Warning: {} and {} differ in size, no change is reported'.format(files[k - 1], f))
                    results[(c, k)] = empty_result()
                else:
                    pairs.append((index_of[(c, k - 1)], index_of[(c, k)]))
                    pair_keys.append((c, k))
            if ptrs:
                with clock('change_detect'):
                    res = ctx.change_detect(ptrs, sizes, [p.data_ptr() for p in planes], ready, pairs, record)
                for j, (c, k) in enumerate(pair_keys):
                    size = sizes[pairs[j][1]]
                    if res['overflow'][j]:
                        files = cameras[c][1]
                        count, regions = _host_pair(_load_rgb(files[k - 1]), _load_rgb(files[k]), record)
                        counts['host_pairs'] += 1
                    else:
                        count, regions = int(res['counts'][j]), res['regions'][j][:int(res['n_regions'][j])]
                        counts['gpu_pairs'] += 1
                    results[(c, k)] = pair_result(size, count, regions, options)
            for c, k, f in chunk:                   # what the next chunk may need of this one
                i = index_of.get((c, k))
                carried[c] = (k, sizes[i], planes[i]) if i is not None else (k, None, None)
            del pixels
        torch.cuda.synchronize(dev)
    finally:
        ctx.close()
    rows = []
    for c, (name, files) in enumerate(cameras):
        if files:
            rows.append(first_row(name, files[0]))
        for k in range(1, len(files)):
            rows.append(result_row(name, files[k - 1], files[k], results[(c, k)]))
    return rows, counts


def csv_text(rows):
    """the rows as DataFrame.to_csv(index=False) writes them: None as an empty field, True / False, a float's repr, a field
    quoted only where it must be; no row at all: the line pandas writes for an empty frame"""
    if not rows:
        return os.linesep
    out = io.StringIO()
    writer = csv.writer(out, lineterminator=os.linesep, quoting=csv.QUOTE_MINIMAL)
    writer.writerow(COLUMNS)
    def field(key, value):
        if value is None:
            return ''
        return repr(float(value)) if key == 'diff_percentage' else str(value)

    for row in rows:
        writer.writerow([field(key, row[key]) for key in COLUMNS])
    return out.getvalue()


def process_folders(folders, options=None, output_csv=None, backend='gpu', device=0, profile=None):
    """Several camera folders -> (rows, counts): the rows of all folders in their order, written to output_csv when given;
    counts {'gpu_pairs', 'host_pairs', 'pil_decodes'}.  profile: a dict that receives the waited-for milliseconds per kind of
    device call (gpu leg; slows the run)."""
    if options is None:
        options = ChangeDetectionOptions()
    record = check_options(options, backend)
    if isinstance(folders, (str, Path)):
        folders = [folders]
    folders = [Path(folder) for folder in folders]
    counts = {'gpu_pairs': 0, 'host_pairs': 0, 'pil_decodes': 0}
    cameras = [_camera_images(folder) for folder in folders]
    if backend == 'gpu':
        rows, counts = _gpu_rows(cameras, options, record, device, counts, profile)
    else:
        jobs = [(name, files, options, record) for name, files in cameras]
        if options.workers == 1 or len(jobs) < 2:
            per_camera = [_host_camera(*job) for job in jobs]
        else:
            import multiprocessing
            from concurrent.futures import ProcessPoolExecutor
            # (spawned, not forked: a worker must not inherit a GPU the calling process may have open)
            with ProcessPoolExecutor(max_workers=options.workers, mp_context=multiprocessing.get_context('spawn')) as executor:
                per_camera = list(executor.map(_host_camera_job, jobs))
        rows = [row for camera_rows in per_camera for row in camera_rows]
        counts['host_pairs'] = sum(1 for row in rows if row['prev_image'] is not None)
    if output_csv:
        with open(output_csv, 'w', newline='') as f:
            f.write(csv_text(rows))
        print('Results saved to {}'.format(output_csv))
    return rows, counts


def sample_previews(rows, num_samples=10, random_seed=None):
    """the rows create_change_previews draws, as the reference picks them: those with motion_detected, random.sample over
    their positions after random.seed(random_seed), all of them for num_samples None"""
    motion_detected = [row for row in rows if row['motion_detected'] == True]  # noqa
    if len(motion_detected) == 0:
        print('No motion detected in any images')
        return []
    if random_seed is not None:
        random.seed(random_seed)
    if num_samples is None:
        return motion_detected
    sample_size = min(num_samples, len(motion_detected))
    return [motion_detected[i] for i in random.sample(range(len(motion_detected)), sample_size)]


def preview_name(row):
    return 'preview_{}_{}'.format(Path(row['image']).parent.name, Path(row['image']).name)


def create_change_previews(rows, output_folder, num_samples=10, random_seed=None, backend='gpu'):
    """Side-by-side previews of sampled rows with motion.  The sampling (sample_previews) and the file names (preview_name) are
    the reference's; the picture is not restated yet."""
    raise NotImplementedError('create_change_previews: the preview picture is not restated (sample_previews and preview_name are)')


def build_parser():
    parser = argparse.ArgumentParser(description='Detect motion in timelapse camera images')
    parser.add_argument('--root_dir', required=True, help='Root directory containing camera folders')
    parser.add_argument('--output_csv', default=None, help='Optional output CSV file')
    parser.add_argument('--min_area', type=int, default=500, help='Minimum region area (pixels) to consider as significant motion')
    parser.add_argument('--threshold', type=int, default=25, help='Threshold for binary image creation')
    parser.add_argument('--detection_method', type=str, default='frame_diff', choices=['frame_diff', 'mog2', 'knn', 'motion_history'],
                        help='Method to use for change detection (only frame_diff is implemented)')
    parser.add_argument('--threshold_type', type=str, default='global', choices=['global', 'adaptive', 'otsu'],
                        help='Type of thresholding to apply (adaptive is not implemented)')
    parser.add_argument('--history', type=int, default=500, help='Number of frames used to build the background model')
    parser.add_argument('--var_threshold', type=float, default=16, help='Threshold for MOG2/KNN background subtraction')
    parser.add_argument('--detect_shadows', action='store_true', help='Detect and mark shadows in background subtraction')
    parser.add_argument('--adaptive_block_size', type=int, default=11, help='Block size for adaptive thresholding')
    parser.add_argument('--adaptive_c', type=int, default=2, help='Constant subtracted from the mean for adaptive thresholding')
    parser.add_argument('--mhi_duration', type=float, default=1.0, help='Duration in seconds for the motion history image')
    parser.add_argument('--mhi_threshold', type=int, default=30, help='Threshold for motion detection in the motion history image')
    parser.add_argument('--mhi_buffer_size', type=int, default=10, help='Number of frames to keep in motion history buffer')
    parser.add_argument('--ignore_fraction', type=float, default=None,
                        help='Fraction of image to ignore: negative = top, positive = bottom, range [-1.0, 1.0]')
    parser.add_argument('--workers', type=int, default=4, help='Number of parallel workers (host backend)')
    parser.add_argument('--verbose', action='store_true', help='Enable additional debug output (not implemented)')
    parser.add_argument('--create_previews', action='store_true', help='Create side-by-side previews of detected motion')
    parser.add_argument('--preview_folder', default='change_previews', help='Folder to save preview images')
    parser.add_argument('--num_previews', type=int, default=10, help='Number of random preview images to create')
    parser.add_argument('--backend', default='gpu', choices=['gpu', 'host'], help='mdhip_change_detect on the GPU, or its host model')
    parser.add_argument('--device', type=int, default=0, help='GPU index')
    return parser


def options_from_args(args):
    return ChangeDetectionOptions(
        min_area=args.min_area, threshold=args.threshold, detection_method=getattr(DetectionMethod, args.detection_method.upper()),
        threshold_type=getattr(ThresholdType, args.threshold_type.upper()), history=args.history, var_threshold=args.var_threshold,
        detect_shadows=args.detect_shadows, adaptive_block_size=args.adaptive_block_size, adaptive_c=args.adaptive_c,
        mhi_duration=args.mhi_duration, mhi_threshold=args.mhi_threshold, mhi_buffer_size=args.mhi_buffer_size,
        ignore_fraction=args.ignore_fraction, workers=args.workers, verbose=args.verbose)


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        parser.exit()
    args = parser.parse_args(argv)
    if args.ignore_fraction is not None and (args.ignore_fraction < -1.0 or args.ignore_fraction > 1.0):
        print('Error: ignore_fraction must be between -1.0 and 1.0')
        return
    options = options_from_args(args)
    camera_folders = [f for f in Path(args.root_dir).iterdir() if f.is_dir()]
    print('Found {} camera folders'.format(len(camera_folders)))
    results, _ = process_folders(camera_folders, options=options, output_csv=args.output_csv, backend=args.backend, device=args.device)
    if args.create_previews:
        preview_paths = create_change_previews(results, args.preview_folder, num_samples=args.num_previews, backend=args.backend)
        print('Created {} preview images in {}'.format(len(preview_paths), args.preview_folder))
    print('Motion detection completed')
    motion_detected_count = sum(1 for row in results if row['motion_detected'])
    total_images = len(results)
    if total_images > 0:
        print('Motion detected in {} out of {} images ({:.2f}%)'.format(motion_detected_count, total_images,
                                                                       motion_detected_count / total_images * 100))
    else:
        print('No images were processed')


if __name__ == '__main__':
    main()
