"""
Privacy blurring of detections in written image copies, as the reference does it
(postprocessing/separate_detections_into_folders.py --category_names_to_blur person: vis_utils.load_image, then
visualization_utils.blur_detections -- per box crop, ImageFilter.GaussianBlur(40), paste -- then exif_preserving_save),
from an image that is in device memory already: the GPU blurs a copy of it (HipContext.blur_regions, Pillow's arithmetic
bit for bit), encodes the whole copy (HipContext.jpeg_encode) and the host puts the file around the scan
(jpeg_host.jfif_file).  No second read or decode of the source file, no blur and no encode on the host.

The files equal, byte for byte, what Image.save(name, quality=q) writes for Pillow's blurred pixels.  That is what the
reference's exif_preserving_save(quality='keep') writes only where open_image made a NEW image -- an 'L' or 'RGBA' file, a
file with an EXIF rotation -- and then with the source's EXIF block and COM segment, which are not written here.  For a plain
RGB JPEG, which is what a camera trap writes, the opened image is still a JPEG to Pillow, and quality='keep' re-encodes with
the source file's own quantisation tables and its own chroma sampling (4:4:4, 4:2:2 or 4:2:0), again with an EXIF APP1 segment
and the source's COM segment: these files do NOT equal the reference's.  separate_detections.py reproduces them, on the
device too (HipContext.jpeg_encode_sampled, jpeg_host.sampled_file); blur= keeps its behaviour.
"""

from . import jpeg_host
from .crops import Product, device_stream, files_of_device_images, output_order, write_file, _pil_file

#: the reference script's own default: its --threshold is None (separate_detections_into_folders.py:708), so it takes
#: get_typical_confidence_threshold_from_results (separate_detections_into_folders.py:557-560), which is
#: 'typical_detection_threshold' of the detector -- 0.2 for MDv5a / MDv5b (detection/run_detector.py:180, :190) and for a
#: detector it does not know (run_detector.py:293)
DEFAULT_BLUR_CONFIDENCE_THRESHOLD = 0.2
DEFAULT_BLUR_RADIUS = 40            # visualization_utils.py:497 blur_detections(image, detections, blur_radius=40)
DEFAULT_BLUR_QUALITY = 85           # visualization_utils.py:199 exif_preserving_save(..., default_quality=85)


class BlurOptions:
    """which detections are blurred and how the copy is saved (defaults: what the reference script does for `person`)"""

    def __init__(self, category_names=('person',), confidence_threshold=DEFAULT_BLUR_CONFIDENCE_THRESHOLD,
                 radius=DEFAULT_BLUR_RADIUS, quality=DEFAULT_BLUR_QUALITY, output_threshold=None):
        if isinstance(category_names, str):
            category_names = [s.strip() for s in category_names.split(',')]          # separate_detections_into_folders.py:440-442
        self.category_names = tuple(category_names)
        if not self.category_names:
            raise ValueError('no category to blur')
        self.confidence_threshold = float(confidence_threshold)
        self.radius = float(radius)
        if not 0.0 <= self.radius <= 512.0:
            raise ValueError('blur radius {!r} is outside 0 .. 512'.format(radius))
        self.quality = jpeg_host.check_quality(quality)
        # the confidence threshold of the results file, as for crops.CropOptions: the reference blurs what that file holds
        self.output_threshold = output_threshold

    def category_ids(self, detection_categories=None):
        """the ids of category_names in the results' category map (id -> name)"""
        if detection_categories is None:
            from .constants import DEFAULT_DETECTOR_LABEL_MAP
            detection_categories = DEFAULT_DETECTOR_LABEL_MAP
        name_to_id = {v: k for k, v in detection_categories.items()}
        for name in self.category_names:
            if name not in name_to_id:
                raise ValueError('category {!r} is not one of {}'.format(name, sorted(name_to_id)))
        return {name_to_id[name] for name in self.category_names}


def select_detections(detections, options, category_ids):
    """separate_detections_into_folders.py:444-449: the detections of the categories to blur at or above the threshold, in
    the order of the results file (crops.output_order: confidence descending) -- the order matters where boxes overlap"""
    return [d for d in output_order(detections, options.output_threshold)
            if d['conf'] >= options.confidence_threshold and d['category'] in category_ids]


def blur_rectangle(bbox, width, height):
    """
    visualization_utils.py:513-526 for a normalised [x, y, w, h] box of a width x height image: (left, top, right, bottom),
    right / bottom exclusive, or None for a box that leaves nothing to blur.  right == left (or bottom == top) is a crop
    without pixels, for which Pillow pastes nothing.  Deviation: for right < left or bottom < top -- a box that begins
    beyond the right or bottom border, ends in front of the left or top one, or has a negative size; no detector writes
    one -- Image.crop raises and the reference's run stops; here it is None too.
    """
    x_norm, y_norm, width_norm, height_norm = bbox
    x = int(x_norm * width)
    y = int(y_norm * height)
    w = int(width_norm * width)
    h = int(height_norm * height)
    left, top = max(0, x), max(0, y)
    right, bottom = min(width, x + w), min(height, y + h)
    if right <= left or bottom <= top:
        return None
    return left, top, right, bottom


def rectangles_to_blur(detections, width, height, options, category_ids):
    """the rectangles with area of an image's detections to blur, in the order they are applied"""
    rects = [blur_rectangle(d['bbox'], width, height) for d in select_detections(detections, options, category_ids)]
    return [r for r in rects if r is not None]


def blurred_file_of_host_image(pixels, name, detections, options, category_ids):
    """
    The host leg, for an image whose pixels are not in device memory: mdjpeg_blur_regions (libmdjpeg.so; Pillow's blur,
    compiled from the header the kernels are compiled from) on a copy of the H x W x 3 uint8 array, saved by PIL in the
    format of `name` at options.quality.  None when nothing in the image is to be blurred.
    """
    import numpy as np
    rects = rectangles_to_blur(detections, pixels.shape[1], pixels.shape[0], options, category_ids)
    if not rects:
        return None
    copy = np.array(pixels, dtype=np.uint8, order='C')
    rc = jpeg_host.blur_regions(copy, rects, options.radius)
    if rc != jpeg_host.MDJPEG_OK:
        raise RuntimeError('mdjpeg_blur_regions returned {}'.format(rc))
    return _pil_file(copy, name, options.quality)


def blurred_of_device_images(ctx, entries, options, category_ids, stream=0):
    """
    The blurred copies of a batch of images that lie in device memory.  entries: [(tensor, width, height, file, detections)],
    tensor a flat uint8 torch tensor of height * width * 3 bytes, which is NOT changed: an image with something to blur is
    copied on the device, and only such an image is.  Returns ([bytes or None per entry], counts): ONE blur call and, for
    the names Pillow maps to JPEG, ONE encoder call for all copies (counts['gpu']); for any other extension the blurred
    pixels are copied back and PIL saves them in the format of the name (counts['host']).
    """
    import torch
    from .device_render import blur_rects
    counts = {'gpu': 0, 'host': 0}
    out = [None] * len(entries)
    jobs = []                                                    # (entry, rectangles)
    for e, (tensor, width, height, image_file, detections) in enumerate(entries):
        rects = rectangles_to_blur(detections, width, height, options, category_ids)
        if rects:
            jobs.append((e, rects))
    if not jobs:
        return out, counts
    ext = device_stream(stream, entries[0][0].device)
    with torch.cuda.stream(ext):
        copies = [entries[e][0].clone() for e, _ in jobs]
    sizes = [(entries[e][1], entries[e][2]) for e, _ in jobs]
    blur_rects(ctx, [c.data_ptr() for c in copies], sizes, [rects for _, rects in jobs], options.radius, ext.cuda_stream)
    files = files_of_device_images(ctx, [(c, w, h, entries[e][3]) for c, (w, h), (e, _) in zip(copies, sizes, jobs)], options.quality, ext)
    for (e, _), (data, leg) in zip(jobs, files):
        out[e] = data
        counts[leg] += 1
    return out, counts


def write_blurred(blur_folder, relative_name, data):
    """writes one blurred copy below blur_folder; returns the path"""
    return write_file(blur_folder, relative_name, data)


class BlurProduct(Product):
    """blur=: result['blurred'] = bytes, or None when nothing in the image is to be blurred; counted in HIPDetector.blur_counts"""

    key = 'blurred'

    def nothing(self):
        return None

    def _host(self, pixels, name, detections):
        data = blurred_file_of_host_image(pixels, name, detections, self.options, self.options.category_ids())
        return data, None if data is None else 'host'

    def _device(self, ctx, entries, stream):
        return blurred_of_device_images(ctx, entries, self.options, self.options.category_ids(), stream=stream)


__all__ = ['BlurOptions', 'DEFAULT_BLUR_CONFIDENCE_THRESHOLD', 'blur_rectangle', 'blurred_file_of_host_image',
           'blurred_of_device_images', 'rectangles_to_blur', 'select_detections', 'write_blurred']
