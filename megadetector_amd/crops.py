"""
Detection crops as the reference cuts and names them (postprocessing/create_crop_folder.py, visualization_utils.crop_image),
written from an image that is in device memory already: the GPU encodes the JPEG scans (HipContext.jpeg_encode), the host
puts the file around each (jpeg_host.jfif_file).  No second read or decode of the source file, and no pixels of the whole
image come back to the host.

The files equal, byte for byte, what Image.crop(...).save(name, quality=q) writes for the same pixels, with one stated
difference: Pillow copies a COM segment of the source file (info['comment']) into the crop it saves; these files carry none.
"""

import os

from . import jpeg_host


class CropOptions:
    """which detections become crops and how they are saved (defaults: CreateCropFolderOptions of the reference)"""

    def __init__(self, confidence_threshold=0.1, expansion=0, quality=95, category_names_to_include=None,
                 output_threshold=None):
        self.confidence_threshold = confidence_threshold
        self.expansion = expansion
        self.quality = jpeg_host.check_quality(quality)
        self.category_names_to_include = category_names_to_include
        # the confidence threshold of the results file (the batch driver filters with it behind the detector): crop ids
        # count the detections that file holds.  None = every detection the detector returns
        self.output_threshold = output_threshold

    def category_ids(self):
        from .constants import DEFAULT_DETECTOR_LABEL_MAP
        return category_ids_to_include(self, DEFAULT_DETECTOR_LABEL_MAP)


def output_order(detections, output_threshold=None):
    """the detections as the results file holds them: at or above its threshold, sorted by confidence descending (the
    sort of write_results_to_file: stable, None smallest)"""
    dets = [d for d in detections or [] if output_threshold is None or d['conf'] >= output_threshold]
    return sorted(dets, key=lambda d: (d['conf'] is not None, d['conf']), reverse=True)


def category_ids_to_include(options, detection_categories):
    """the ids of options.category_names_to_include in the results' category map (id -> name); None = every category"""
    if options.category_names_to_include is None:
        return None
    name_to_id = {v: k for k, v in detection_categories.items()}
    ids = set()
    for name in options.category_names_to_include:
        if name not in name_to_id:
            raise ValueError('category {!r} is not one of {}'.format(name, sorted(name_to_id)))
        ids.add(name_to_id[name])
    return ids


def crop_filename(image_file, crop_id):
    """_get_crop_filename: insert_before_extension(file, 'crop_' + the id with three digits)"""
    if isinstance(crop_id, int):
        crop_id = str(crop_id).zfill(3)
    name, ext = os.path.splitext(image_file)
    return '{}.crop_{}{}'.format(name, crop_id, ext)


def select_crops(detections, options, category_ids=None):
    """
    create_crop_folder.py:392-425 for one image: [(crop_id, detection)] of the detections at or above the threshold and in
    the categories asked for.  The id is the detection's index in the list as the output JSON holds it.
    """
    out = []
    for i, det in enumerate(detections or []):
        if det['conf'] < options.confidence_threshold:
            continue
        if category_ids is not None and det['category'] not in category_ids:
            continue
        out.append((det.get('crop_id', i), det))
    return out


def crop_rectangle(bbox, width, height, expansion=0):
    """
    The pixels visualization_utils.crop_image cuts for a normalised [x, y, w, h] box of a width x height image:
    box -> pixels, `expansion` pixels on every side, clamped to [0, width - 1] x [0, height - 1], then what Image.crop does
    with the float box: Python's round (half to even) and int.  Returns (left, top, right, bottom), right / bottom
    exclusive, or None for a rectangle without area, which PIL cannot save either.  Deviation: a box of NEGATIVE width or
    height (no detector writes one) is None too, where Image.crop raises and the reference's second pass stops.
    """
    x1, y1, w_box, h_box = bbox
    left, right, top, bottom = x1 * width, (x1 + w_box) * width, y1 * height, (y1 + h_box) * height
    if expansion > 0:
        left -= expansion
        right += expansion
        top -= expansion
        bottom += expansion
    left, right, top, bottom = max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)
    left, right = min(left, width - 1), min(right, width - 1)
    top, bottom = min(top, height - 1), min(bottom, height - 1)
    x0, y0, x1, y1 = (int(round(v)) for v in (left, top, right, bottom))
    if x1 <= x0 or y1 <= y0:
        return None
    return x0, y0, x1, y1


_JPEG_EXTENSIONS = None


def is_jpeg_name(name):
    """whether Pillow saves a file of this name as JPEG (it picks the format from the extension)"""
    global _JPEG_EXTENSIONS
    if _JPEG_EXTENSIONS is None:
        from PIL import Image
        _JPEG_EXTENSIONS = {e for e, f in Image.registered_extensions().items() if f == 'JPEG'}
    return os.path.splitext(name)[1].lower() in _JPEG_EXTENSIONS


def encode_windows(ctx, ptrs, pitches, rects, quality, stream=0, comments=None):
    """
    JPEG files of windows of device images: ptrs[i] the first pixel of the image rects[i] (from crop_rectangle) lies in,
    pitches[i] its bytes a row.  ONE call of the encoder for all of them and one read-back; a second call with the size
    the first reported when the guess at the output was too small.  comments: per window None or the bytes of the COM
    segment Pillow carries over from a source; a window with one is written by jpeg_host.sampled_file, not jfif_file.
    """
    from .device_render import read_encoded
    if not rects:
        return []
    wins = [int(p) + y0 * pitch + x0 * 3 for p, pitch, (x0, y0, _, _) in zip(ptrs, pitches, rects)]
    sizes = [(x1 - x0, y1 - y0) for x0, y0, x1, y1 in rects]
    # a guess far below the bound (ctx.jpeg_encode_bound): half a byte a sample and the 16 x 16 blocks' fixed cost
    capacity = sum(w * h * 3 // 2 + 64 * ((w + 15) // 16) * ((h + 15) // 16) + 64 for w, h in sizes)
    host, offs, lens, _ = read_encoded(
        lambda out_ptr, capacity: ctx.jpeg_encode(wins, sizes, list(pitches), quality, out_ptr, capacity, stream),
        capacity, 'cuda:{}'.format(ctx.device), 'mdhip_jpeg_encode')
    scans = [host[o:o + n].tobytes() for o, n in zip(offs, lens)]
    if not comments or not any(comments):
        return [jpeg_host.jfif_file(w, h, quality, scan) for (w, h), scan in zip(sizes, scans)]
    ql, qc = jpeg_host.quant_tables(quality)
    return [jpeg_host.sampled_file(w, h, ql, qc, 2, scan, b'', comment) if comment else jpeg_host.jfif_file(w, h, quality, scan)
            for (w, h), scan, comment in zip(sizes, scans, comments)]


def _pick(image_file, width, height, detections, options, category_ids, warn):
    """-> ([(crop_id, name, rectangle)], skipped) of one image"""
    picked, skipped = [], 0
    for crop_id, det in select_crops(output_order(detections, options.output_threshold), options, category_ids):
        r = crop_rectangle(det['bbox'], width, height, options.expansion)
        if r is None:
            skipped += 1
            warn('Warning: no crop for detection {} of {}: its box {} has no area in a {} x {} image'.format(
                crop_id, image_file, det['bbox'], width, height))
            continue
        picked.append((crop_id, crop_filename(image_file, crop_id), r))
    return picked, skipped


def _pil_file(pixels, name, quality):
    import io
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(pixels).save(bio, format=Image.registered_extensions().get(os.path.splitext(name)[1].lower()), quality=quality)
    return bio.getvalue()


def device_stream(stream, device):
    """the torch stream work for a raw stream handle goes on: an ExternalStream around the handle, the current stream for 0"""
    import torch
    return torch.cuda.ExternalStream(stream, device=device) if stream else torch.cuda.current_stream(device)


def files_of_device_images(ctx, images, quality, ext):
    """
    Whole images in device memory saved under names.  images: [(tensor, width, height, name)], ext the torch stream they were
    made on.  Returns [(bytes, leg)]: the names Pillow maps to JPEG are encoded on the device, all in ONE encoder call
    ('gpu'); for any other extension the pixels are copied back and PIL saves them in the format of the name ('host').
    """
    import torch
    out = [None] * len(images)
    jpeg = [k for k, image in enumerate(images) if is_jpeg_name(image[3])]
    if jpeg:
        files = encode_windows(ctx, [images[k][0].data_ptr() for k in jpeg], [images[k][1] * 3 for k in jpeg],
                               [(0, 0, images[k][1], images[k][2]) for k in jpeg], quality, ext.cuda_stream)
        for k, data in zip(jpeg, files):
            out[k] = (data, 'gpu')
    for k, (tensor, width, height, name) in enumerate(images):
        if out[k] is None:
            with torch.cuda.stream(ext):
                pixels = tensor.cpu().numpy().reshape(height, width, 3)
            out[k] = (_pil_file(pixels, name, quality), 'host')
    return out


def crops_of_host_image(pixels, image_file, detections, options, category_ids=None, warn=print):
    """the reference's way, from an H x W x 3 uint8 array on the host: PIL saves every crop.  -> (crops, skipped)"""
    picked, skipped = _pick(image_file, pixels.shape[1], pixels.shape[0], detections, options, category_ids, warn)
    return [(i, name, _pil_file(pixels[y0:y1, x0:x1], name, options.quality)) for i, name, (x0, y0, x1, y1) in picked], skipped


def crops_of_device_images(ctx, entries, options, category_ids=None, stream=0, warn=print):
    """
    The crops of a batch of images that lie in device memory.  entries: [(tensor, width, height, file, detections)], tensor a
    flat uint8 torch tensor of height * width * 3 bytes.  Returns ([[(crop_id, crop_filename_relative, bytes)] per entry],
    counts): crops whose name Pillow maps to JPEG are encoded on the device, all images' in ONE encoder call
    (counts['gpu']); for any other extension the crop's pixels alone are copied back and PIL saves them in the format of the
    name, as the reference's second pass does (counts['host']).  A rectangle without area gets no file, one warning and a
    count (counts['skipped']).
    """
    counts = {'gpu': 0, 'host': 0, 'skipped': 0}
    picked_all, jobs = [], []
    for e, (tensor, width, height, image_file, detections) in enumerate(entries):
        picked, skipped = _pick(image_file, width, height, detections, options, category_ids, warn)
        counts['skipped'] += skipped
        picked_all.append(picked)
        jobs += [(e, k) for k, (_, name, _) in enumerate(picked) if is_jpeg_name(name)]
    files = dict(zip(jobs, encode_windows(ctx, [entries[e][0].data_ptr() for e, _ in jobs], [entries[e][1] * 3 for e, _ in jobs],
                                          [picked_all[e][k][2] for e, k in jobs], options.quality, stream)))
    counts['gpu'] = len(jobs)
    out = []
    for e, picked in enumerate(picked_all):
        tensor, width, height = entries[e][:3]
        crops = []
        for k, (crop_id, name, (x0, y0, x1, y1)) in enumerate(picked):
            data = files.get((e, k))
            if data is None:
                pixels = tensor.view(height, width * 3)[y0:y1, x0 * 3:x1 * 3].contiguous().cpu().numpy().reshape(y1 - y0, x1 - x0, 3)
                data = _pil_file(pixels, name, options.quality)
                counts['host'] += 1
            crops.append((crop_id, name, data))
        out.append(crops)
    return out, counts


def crops_of_device_image(ctx, tensor, width, height, image_file, detections, options, category_ids=None, stream=0, warn=print):
    """crops_of_device_images for one image -> (crops, skipped)"""
    out, counts = crops_of_device_images(ctx, [(tensor, width, height, image_file, detections)], options, category_ids, stream, warn)
    return out[0], counts['skipped']


def write_file(folder, relative_name, data):
    """writes the bytes of one file below folder under its relative name; returns the path"""
    path = os.path.join(folder, relative_name).replace('\\', '/')
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)
    return path


def write_crops(crop_folder, crops):
    """writes [(crop_id, crop_filename_relative, bytes)] below crop_folder; returns the paths"""
    return [write_file(crop_folder, name, data) for _, name, data in crops]


class Product:
    """
    What HIPDetector needs to know about a product it makes from the image in device memory (crops=, blur=, preview=): `key`
    of the result dict, nothing() for an image that has none, the dict `counts` feeds, selects(result), and how the product
    is made -- _device(ctx, entries, stream) -> (values, counts) for a batch of [(tensor, width, height, name, detections)]
    and, unless `letterboxed_on_device`, _host(pixels, name, detections) -> (value, the count it adds to or None).
    """

    #: an input that came already letterboxed: True = the product is made on the device from the letterboxed pixels, False =
    #: by the host leg from 'img_original', which for such an input is on the host only
    letterboxed_on_device = False

    def __init__(self, options, counts):
        self.options, self.counts = options, counts

    def selects(self, result):
        return result.get('detections') is not None

    def of_host_image(self, pixels, name, detections):
        value, leg = self._host(pixels, name, detections)
        if leg is not None:
            self.counts[leg] += 1
        return value

    def of_device_images(self, ctx, entries, stream=0):
        out, counts = self._device(ctx, entries, stream)
        for key, n in counts.items():
            self.counts[key] += n
        return out


class CropProduct(Product):
    """crops=: result['crops'] = [(crop_id, crop_filename_relative, bytes)], counted in HIPDetector.crop_counts"""

    key = 'crops'
    letterboxed_on_device = True

    def nothing(self):
        return []

    def _device(self, ctx, entries, stream):
        return crops_of_device_images(ctx, entries, self.options, self.options.category_ids(), stream=stream)


def annotate_results(images, options, category_ids=None, name_of=None):
    """
    What create_crop_folder adds to the results it was given (output_file): 'crop_id' and 'crop_filename_relative' on every
    detection that is cropped.  Returns the per-crop records of crops_output_file (create_crop_folder.py:485-521).
    name_of: maps an image's 'file' to the name its crops are derived from (default: the file itself).
    """
    records = []
    for im in images:
        for crop_id, det in select_crops(im.get('detections'), options, category_ids):
            det['crop_id'] = crop_id
            det['crop_filename_relative'] = crop_filename(name_of(im['file']) if name_of else im['file'], crop_id)
        for det in im.get('detections') or []:
            if 'crop_id' in det:
                records.append({'file': det['crop_filename_relative'],
                                'detections': [{'category': det['category'], 'conf': det['conf'], 'bbox': [0, 0, 1, 1],
                                                'crop_id': det['crop_id']}]})
    return records


__all__ = ['CropOptions', 'annotate_results', 'category_ids_to_include', 'crop_filename', 'crop_rectangle', 'crops_of_device_image', 'crops_of_device_images', 'crops_of_host_image', 'output_order',
           'encode_windows', 'is_jpeg_name', 'select_crops', 'write_crops']
