"""
Repeat-detection elimination (RDE): find the boxes a camera was given again and again -- a rock, a branch -- and make their
confidences negative.  The reference: postprocessing/repeat_detection_elimination/repeat_detections_core.py
(find_repeat_detections, _find_matches_in_directory, _update_detection_table, _sort_detections_for_directory 'xsort') and
find_repeat_detections.py, its command line.

What is restated, statement for statement: loading and path handling of load_api_results, the grouping of images into
locations, the filters a detection has to pass, the greedy matching rule (a detection is appended to EVERY earlier candidate
of its location it matches, and opens a new candidate when it matches none), the occurrence threshold, the 'xsort' order and
the marking.  The comparison of every detection with the candidates before it -- the part that grows with (detections per
camera)^2 -- runs on the GPU (mdhip_repeat_detections, csrc/rde_kernels.cpp) or, with backend='host', in its host model
(mdjpeg_repeat_detections); both decide a pair with the same doubles, operation for operation, as ct_utils.get_iou.

What is not, in THIS module: the review folder (sample images, remove_repeat_detections after a manual review,
filterFileToLoad) -- it has entry points of its own in rde_review.py (write_review_folder, find_and_write,
remove_repeat_detections), which take what find_repeat_detections returns -- and, anywhere, the HTML page,
smartSort='clustersort', the CSV and intermediate-file paths.  Here they raise NotImplementedError.  So bWriteFilteringFolder
defaults to False HERE (True in the reference).

The output file differs from the reference's write_api_results in two deliberate ways: values are NOT rounded (the reference's
writer rounds every float of the file to 3 decimals, a side effect of DataFrame.to_json(double_precision=3)), and images do
not gain keys they did not have (the reference's table gives a failed image "detections": null).  A second file,
<output>.rde_index.json, lists the suspicious candidates with their instances in a plain layout of our own; the review folder's
detectionIndex.json extends it.

No pandas on this path.

Command line:  python -m megadetector_amd.repeat_detections INPUT --outputFile OUT [--backend host|gpu] [...]
"""

import argparse
import copy
import ctypes as C
import json
import os
import sys

import numpy as np

from .ref_utils import IMG_EXTENSIONS, write_json

#: layout of mdhip_rde_box / mdjpeg_rde_box
BOX_DTYPE = np.dtype([('x', '<f8'), ('y', '<f8'), ('w', '<f8'), ('h', '<f8'), ('group', '<i4'), ('category', '<i4')])

#: options of the reference that only the review folder reads: setting one is a request for it
REVIEW_FOLDER_OPTIONS = ('imageBase', 'outputBase', 'filteredFileListToLoad', 'bRenderOtherDetections', 'bRenderDetectionTiles',
                         'maxOutputImageWidth', 'lineThickness', 'boxExpansion', 'otherDetectionsThreshold', 'otherDetectionsLineWidth',
                         'detectionTilesPrimaryImageWidth', 'detectionTilesCroppedGridWidth', 'detectionTilesPrimaryImageLocation',
                         'detectionTilesMaxCrops', 'otherDetectionsColors', 'bFailOnRenderError', 'bParallelizeRendering',
                         'debugMaxRenderDir', 'debugMaxRenderDetection', 'debugMaxRenderInstance')


class RepeatDetectionOptions:
    """The reference's RepeatDetectionOptions, under its attribute names and with its defaults -- except bWriteFilteringFolder,
    which is False here: the review folder is written by rde_review.write_review_folder, not by this function."""

    def __init__(self):
        self.confidenceMin = 0.1                 #: detections below it are not considered
        self.confidenceMax = 1.0                 #: detections above it are not considered
        self.iouThreshold = 0.9                  #: two boxes are the same place at or above this IoU
        self.occurrenceThreshold = 20            #: instances that make a candidate suspicious
        self.minSuspiciousDetectionSize = 0.0    #: w * h below it: not considered
        self.maxSuspiciousDetectionSize = 0.2    #: w * h above it: not considered (an animal that fills the frame)
        self.maxImagesPerFolder = None           #: locations with more images are left alone
        self.excludeClasses = []                 #: category ids (ints) that are not considered
        self.categoryAgnosticComparisons = False
        self.nDirLevelsFromLeaf = 0              #: how many folders above an image's folder a camera is
        self.customDirNameFunction = None        #: file name -> location, instead of the folder
        self.includeFolders = None
        self.excludeFolders = None
        self.filenameReplacements = {}
        self.smartSort = 'xsort'                 #: 'xsort': suspicious candidates from left to right; None: in order of creation
        self.bWriteFilteringFolder = False       #: the reference's default is True; True is NotImplementedError here (rde_review.py)
        self.filterFileToLoad = ''


class IndexedDetection:
    """one instance of a candidate (reference IndexedDetection)"""

    def __init__(self, i_detection, filename, bbox, confidence, category):
        self.i_detection = i_detection
        self.filename = filename
        self.bbox = bbox
        self.confidence = confidence
        self.category = category


class DetectionLocation:
    """a candidate: a box that matched no candidate before it, and everything that matched it (reference DetectionLocation)"""

    def __init__(self, instance, relative_dir, id):
        self.instances = [instance]
        self.category = instance.category
        self.bbox = instance.bbox
        self.relativeDir = relative_dir
        self.id = id                 #: index of the candidate's image among the images of its location


class RepeatDetectionResults:
    def __init__(self):
        self.detectionResults = None         #: the marked results: the dict of the file, 'images' included
        self.otherFields = None              #: its fields other than 'images'
        self.dirs = None                     #: the locations, in order of first appearance
        self.suspicious_detections = None    #: per location, its suspicious DetectionLocations
        self.n_boxes = 0                     #: detections that took part
        self.n_bbox_changes = 0              #: confidences made negative


def check_options(options):
    if options.smartSort == 'clustersort':
        raise NotImplementedError("smartSort='clustersort' is not restated here; use 'xsort' or None")
    if options.smartSort not in (None, 'xsort'):
        raise ValueError('Unrecognized sort method {}'.format(options.smartSort))
    if getattr(options, 'bWriteFilteringFolder', False):
        raise NotImplementedError('the review folder is not written by find_repeat_detections: bWriteFilteringFolder must stay False '
                                  '(rde_review.write_review_folder takes what this function returns)')
    if getattr(options, 'filterFileToLoad', ''):
        raise NotImplementedError('filterFileToLoad belongs to the review folder: rde_review.remove_repeat_detections loads its index')
    given = [k for k in REVIEW_FOLDER_OPTIONS if k in vars(options) and vars(options)[k] not in (None, '', False)]
    if given:
        raise NotImplementedError('{} belong(s) to the review folder: see rde_review.ReviewFolderOptions'.format(', '.join(given)))
    if options.customDirNameFunction is not None and options.nDirLevelsFromLeaf != 0:
        raise ValueError('Cannot mix custom dir name functions with nDirLevelsFromLeaf')
    if options.includeFolders is not None and options.excludeFolders is not None:
        raise ValueError('Cannot specify include and exclude folder lists')


def prepare_results(results, options):
    """reference load_api_results(normalize_paths=True, force_forward_slashes=True, filename_replacements=...) on a loaded file"""
    for s in ('info', 'detection_categories', 'images'):
        if s not in results:
            raise ValueError('Missing field {} in detection results'.format(s))
    for im in results['images']:
        im['file'] = os.path.normpath(im['file']).replace('\\', '/')
    for old, new in (options.filenameReplacements or {}).items():
        for im in results['images']:
            im['file'] = im['file'].replace(old, new)
    for im in results['images']:
        if 'max_detection_conf' not in im:
            dets = im.get('detections')
            im['max_detection_conf'] = max(d['conf'] for d in dets) if dets else 0.0
    return results


def group_images(images, options):
    """location name -> indices of its images, in order of first appearance (reference 'Separate files into locations')"""
    rows_by_directory = {}
    seen = set()
    for i, im in enumerate(images):
        relative_path = im['file']
        if options.customDirNameFunction is not None:
            dir_name = options.customDirNameFunction(relative_path)
        else:
            dir_name = os.path.dirname(relative_path)
        if len(dir_name) == 0:
            if options.nDirLevelsFromLeaf != 0:
                raise ValueError("Can't use the dirLevelsFromLeaf option with flat filenames")
        else:
            for _ in range(max(0, options.nDirLevelsFromLeaf)):
                dir_name = os.path.dirname(dir_name)
            if len(dir_name) == 0:
                raise ValueError('nDirLevelsFromLeaf leaves no folder name for {}'.format(relative_path))
        rows_by_directory.setdefault(dir_name, []).append(i)
        if relative_path in seen:
            raise ValueError('{} occurs twice in the results'.format(relative_path))
        seen.add(relative_path)
    return rows_by_directory


def collect_boxes(images, rows_by_directory, options):
    """The detections that take part, of all locations in processing order: the box records the kernels take, and per box
    (location index, index of the image in its location, index of the image in the file, index of the detection)."""
    columns, where = ([], [], [], [], [], []), []
    xs, ys, ws, hs, groups, categories = columns
    category_index = {}
    exclude = set(options.excludeClasses or [])
    for i_dir, (dir_name, rows) in enumerate(rows_by_directory.items()):
        if options.maxImagesPerFolder is not None and len(rows) > options.maxImagesPerFolder:
            continue
        if options.includeFolders is not None and dir_name not in options.includeFolders:
            continue
        if options.excludeFolders is not None and dir_name in options.excludeFolders:
            continue
        for i_iteration, i_image in enumerate(rows):
            im = images[i_image]
            if os.path.splitext(im['file'])[1].lower() not in IMG_EXTENSIONS:
                continue
            detections = im.get('detections')
            if detections is None:                       # a failed image
                continue
            if float(im['max_detection_conf']) < options.confidenceMin:
                continue
            for i_detection, detection in enumerate(detections):
                if detection is None:
                    continue
                confidence = detection['conf']
                if not (-1.0 <= confidence <= 1.0):
                    raise ValueError('Illegal confidence {} in image {}'.format(confidence, im['file']))
                if confidence < options.confidenceMin or confidence > options.confidenceMax:
                    continue
                if exclude and int(detection['category']) in exclude:
                    continue
                bbox = detection['bbox']
                w, h = bbox[2], bbox[3]
                if w == 0 or h == 0:
                    continue
                area = h * w
                if area < 0:
                    area = abs(area)
                if not (0.0 <= area <= 1.0):
                    raise ValueError('Illegal bounding box area {} in image {}'.format(area, im['file']))
                if area < options.minSuspiciousDetectionSize or area > options.maxSuspiciousDetectionSize:
                    continue
                category = category_index.setdefault(detection['category'], len(category_index))    # categories compare as strings
                xs.append(bbox[0])
                ys.append(bbox[1])
                ws.append(w)
                hs.append(h)
                groups.append(i_dir)
                categories.append(category)
                where.append((i_dir, i_iteration, i_image, i_detection))
    boxes = np.zeros(len(where), dtype=BOX_DTYPE)
    for name, column in zip(BOX_DTYPE.names, columns):
        boxes[name] = column
    return boxes, where


def match_boxes(boxes, iou_threshold, category_agnostic, occurrence_threshold, backend='gpu', device=0, chunk=0, capacity=None):
    """mdhip_repeat_detections (backend 'gpu') or its host model mdjpeg_repeat_detections ('host') on a BOX_DTYPE array:
    (is_candidate uint8 [n], n_instances int32 [n], pairs int64 [k, 2] of (instance, candidate)).  Too small a `capacity` is
    answered with the capacity the call needs, and the call is made once more."""
    boxes = np.ascontiguousarray(boxes, dtype=BOX_DTYPE)
    n = len(boxes)
    is_candidate = np.zeros(max(n, 1), np.uint8)
    n_instances = np.zeros(max(n, 1), np.int32)
    if backend == 'host':
        from megadetector_amd import jpeg_host
        lib, ecapacity = jpeg_host.load(), jpeg_host.MDJPEG_ECAPACITY

        def call(pairs, cap, needed):
            return lib.mdjpeg_repeat_detections(boxes.ctypes.data, n, iou_threshold, int(bool(category_agnostic)), int(occurrence_threshold),
                                                int(chunk), is_candidate.ctypes.data, n_instances.ctypes.data, pairs.ctypes.data, cap,
                                                C.byref(needed))

        def error(rc):
            return ValueError('mdjpeg_repeat_detections: bad argument (n < 0, a decreasing group, a NaN threshold or a chunk out of range)')
    elif backend == 'gpu':
        from megadetector_amd import _lib
        lib, ecapacity = _lib.load(), _lib.MDHIP_ECAPACITY

        def call(pairs, cap, needed):
            return lib.mdhip_repeat_detections(int(device), boxes.ctypes.data, n, iou_threshold, int(bool(category_agnostic)),
                                               int(occurrence_threshold), int(chunk), is_candidate.ctypes.data, n_instances.ctypes.data,
                                               pairs.ctypes.data, cap, C.byref(needed))

        def error(rc):
            text = (lib.mdhip_last_error(None) or b'').decode()
            return (ValueError if rc == -1 else _lib.HipError)('mdhip_repeat_detections failed ({}): {}'.format(rc, text))
    else:
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    cap = n if capacity is None else int(capacity)
    for _ in range(2):
        pairs = np.zeros((max(cap, 1), 2), np.int64)
        needed = C.c_int64(0)
        rc = call(pairs, cap, needed)
        if rc != ecapacity:
            break
        cap = needed.value
    if rc != 0:
        raise error(rc)
    return is_candidate[:n], n_instances[:n], pairs[:needed.value]


def mark_repeat_detections(results, options=None, backend='gpu', device=0):
    """find_repeat_detections on results that are in memory (the dict of a results file): marks `results` in place."""
    options = options or RepeatDetectionOptions()
    check_options(options)
    results = prepare_results(results, options)
    images = results['images']
    rows_by_directory = group_images(images, options)
    dirs = list(rows_by_directory.keys())
    boxes, where = collect_boxes(images, rows_by_directory, options)
    _, n_instances, pairs = match_boxes(boxes, options.iouThreshold, options.categoryAgnosticComparisons, options.occurrenceThreshold,
                                        backend=backend, device=device)

    def instance_of(b):
        _, _, i_image, i_detection = where[b]
        d = images[i_image]['detections'][i_detection]
        return IndexedDetection(i_detection, images[i_image]['file'], d['bbox'], d['conf'], d['category'])

    # the suspicious candidates with their instance lists: `pairs` is sorted by candidate, then by instance
    suspicious = [[] for _ in dirs]
    current = -1
    for b, c in pairs.tolist():
        if c != current:
            current = c
            i_dir, i_iteration, _, _ = where[c]
            assert b == c, 'the first instance of a candidate is the candidate'
            location = DetectionLocation(instance_of(c), dirs[i_dir], i_iteration)
            suspicious[i_dir].append(location)
        else:
            location.instances.append(instance_of(b))
    for location_list in suspicious:
        for location in location_list:
            assert len(location.instances) >= options.occurrenceThreshold
    if options.smartSort == 'xsort':
        suspicious = [sorted(s, key=lambda x: x.bbox[0] + x.bbox[2] / 2.0) for s in suspicious]

    # marking (reference _update_detection_table)
    n_bbox_changes = 0
    for b in pairs[:, 0].tolist():
        _, _, i_image, i_detection = where[b]
        d = images[i_image]['detections'][i_detection]
        if d['conf'] >= 0:
            d['conf'] = -1 * d['conf']
            n_bbox_changes += 1
    for im in images:
        if im.get('detections'):
            im['max_detection_conf'] = max(d['conf'] for d in im['detections'])

    out = RepeatDetectionResults()
    out.detectionResults = results
    out.otherFields = {k: v for k, v in results.items() if k != 'images'}
    out.dirs = dirs
    out.suspicious_detections = suspicious
    out.n_boxes = len(where)
    out.n_bbox_changes = n_bbox_changes
    return out


def results_for_file(results):
    """what the reference's write_api_results writes of marked results -- without its rounding and without the keys its table
    adds: 'failure' dropped where it is None, format_version a string, max_detection_conf dropped for format >= 1.3"""
    out = {k: copy.deepcopy(v) for k, v in results.items() if k != 'images'}
    images = [dict(im) for im in results['images']]
    for im in images:
        if 'failure' in im and im['failure'] is None:
            del im['failure']
    try:
        if not isinstance(out['info']['format_version'], str):
            out['info']['format_version'] = str(out['info']['format_version'])
        if float(out['info']['format_version']) >= 1.3:
            for im in images:
                im.pop('max_detection_conf', None)
    except Exception:
        print('Warning: error determining format version')
    out['images'] = images
    return out


def index_for_file(rde_results, options):
    """the suspicious candidates and their instances, per location: the layout of <output>.rde_index.json"""
    names = ('confidenceMin', 'confidenceMax', 'iouThreshold', 'occurrenceThreshold', 'minSuspiciousDetectionSize',
             'maxSuspiciousDetectionSize', 'maxImagesPerFolder', 'excludeClasses', 'categoryAgnosticComparisons', 'nDirLevelsFromLeaf',
             'includeFolders', 'excludeFolders', 'filenameReplacements', 'smartSort')
    return {'options': {k: getattr(options, k) for k in names},
            'dirs': rde_results.dirs,
            'suspicious_detections': [
                [{'bbox': loc.bbox, 'category': loc.category, 'id': loc.id, 'relativeDir': loc.relativeDir,
                  'instances': [{'filename': i.filename, 'i_detection': i.i_detection, 'bbox': i.bbox, 'confidence': i.confidence}
                                for i in loc.instances]} for loc in locs]
                for locs in rde_results.suspicious_detections]}


def write_outputs(rde_results, options, output_file_name):
    write_json(output_file_name, results_for_file(rde_results.detectionResults), force_str=True)
    write_json(output_file_name + '.rde_index.json', index_for_file(rde_results, options), force_str=True)


def find_repeat_detections(input_filename, output_file_name=None, options=None, backend='gpu', device=0):
    """The reference's find_repeat_detections without the review folder: loads a results file, marks its repeat detections
    (negative `conf`) and, when output_file_name is given, writes it and <output_file_name>.rde_index.json.  backend='gpu'
    compares the boxes on HIP device `device`; backend='host' runs the host model of the kernels and needs no GPU."""
    options = options or RepeatDetectionOptions()
    check_options(options)
    with open(input_filename, 'r') as f:
        results = json.load(f)
    out = mark_repeat_detections(results, options, backend=backend, device=device)
    print('Found {} suspicious detections on {} boxes in {} locations; changed {} confidences'.format(
        sum(len(s) for s in out.suspicious_detections), out.n_boxes, len(out.dirs), out.n_bbox_changes))
    if output_file_name:
        write_outputs(out, options, output_file_name)
    return out


def main(argv=None):
    d = RepeatDetectionOptions()
    ap = argparse.ArgumentParser(description='Mark repeat detections of a MegaDetector results file (negative confidences)')
    ap.add_argument('inputFile', type=str, help='MD results .json file to process')
    ap.add_argument('--outputFile', type=str, default=None, help='.json file to write the marked results to')
    ap.add_argument('--confidenceMin', type=float, default=d.confidenceMin)
    ap.add_argument('--confidenceMax', type=float, default=d.confidenceMax)
    ap.add_argument('--iouThreshold', type=float, default=d.iouThreshold)
    ap.add_argument('--occurrenceThreshold', type=int, default=d.occurrenceThreshold)
    ap.add_argument('--minSuspiciousDetectionSize', type=float, default=d.minSuspiciousDetectionSize)
    ap.add_argument('--maxSuspiciousDetectionSize', type=float, default=d.maxSuspiciousDetectionSize)
    ap.add_argument('--maxImagesPerFolder', type=int, default=d.maxImagesPerFolder)
    ap.add_argument('--excludeClasses', nargs='+', type=int, default=None)
    ap.add_argument('--nDirLevelsFromLeaf', type=int, default=d.nDirLevelsFromLeaf)
    ap.add_argument('--backend', choices=('host', 'gpu'), default='gpu', help="'host': the host model of the kernels, no GPU needed")
    ap.add_argument('--device', type=int, default=0, help='HIP device of the gpu backend')
    args = ap.parse_args(argv)
    for k in ('confidenceMin', 'confidenceMax', 'iouThreshold', 'occurrenceThreshold', 'minSuspiciousDetectionSize',
              'maxSuspiciousDetectionSize', 'maxImagesPerFolder', 'nDirLevelsFromLeaf'):
        setattr(d, k, getattr(args, k))
    if args.excludeClasses is not None:
        d.excludeClasses = args.excludeClasses
    find_repeat_detections(args.inputFile, args.outputFile, d, backend=args.backend, device=args.device)
    return 0


if __name__ == '__main__':
    sys.exit(main())
