"""
Species classification of detections in the same pass, as the reference's second stage does it from crop files
(classification/crop_detections.py save_crop -> classification/run_classifier.py -> merge_classification_detection_output.py),
from an image that is in device memory already: ONE kernel launch takes the crops of a batch from their images to the
normalised tensor the classifier reads (HipContext.classifier_input), the TorchScript model runs on that tensor on the same
stream, and only the probabilities come back.  No crop file is written, read, decoded or resized on the host.

The rules are restated here once.  crop_canvas says which pixels a detection's crop holds; classifier_input_host makes the
tensor with PIL and numpy -- it is the host leg (pixels that are not in device memory, crops the kernel refuses) and the
reference the tests compare the kernel with; classification_list formats a row of probabilities.

Deliberate differences from the reference scripts: no crop files and no CSV between the stages (the `jpeg_quality` option
restores the pixels of the file round trip); ground-truth features of the merge script (label_pos, relative_conf) are not
restated; a box wider AND higher than its image (no detector writes one), which ImageOps.pad would enlarge, is skipped.
This module imports neither torch nor the HIP library at module level.
"""

import json

from .crops import Product, category_ids_to_include, device_stream, output_order, select_crops

DEFAULT_CLASSIFIER_IMAGE_SIZE = 224             # run_classifier.py --image-size default
IMAGENET_MEAN = (0.485, 0.456, 0.406)           # train_classifier.MEANS
IMAGENET_STD = (0.229, 0.224, 0.225)            # train_classifier.STDS
FILTERS = {'bicubic': 0, 'bilinear': 1, 'lanczos': 2}       # csrc/resample.h MD_FILTER_*


class ClassifyOptions:
    """which detections are classified, how their crops are cut and transformed, and by which model (defaults: the
    reference's crop_detections.py / run_classifier.py / merge_classification_detection_output.py)"""

    def __init__(self, model, categories=None, image_size=DEFAULT_CLASSIFIER_IMAGE_SIZE, square_crops=True, interpolation='bicubic',
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, confidence_threshold=0.1, category_names_to_include=None,
                 classification_threshold=0.1, batch_size=64, jpeg_quality=None, output_threshold=None):
        if model is None:
            raise ValueError('a classifier model is needed: a TorchScript file, a torch.nn.Module or a callable')
        self.model = model
        self.categories = categories
        self.image_size = int(image_size)
        if not 1 <= self.image_size <= 4096:
            raise ValueError('image size {!r} is outside 1 .. 4096'.format(image_size))
        self.square_crops = bool(square_crops)
        if interpolation not in FILTERS:
            raise ValueError('interpolation {!r} is not one of {}'.format(interpolation, sorted(FILTERS)))
        self.interpolation = interpolation
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or any(v == 0 for v in self.std):
            raise ValueError('mean and std need three values each, and no std may be 0')
        self.confidence_threshold = confidence_threshold
        self.category_names_to_include = category_names_to_include
        self.classification_threshold = classification_threshold
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError('batch size must be positive')
        if jpeg_quality is not None:
            from . import jpeg_host
            jpeg_quality = jpeg_host.check_quality(jpeg_quality)
        self.jpeg_quality = jpeg_quality
        # the confidence threshold of the results file, as for crops.CropOptions: a detection's index counts that file's list
        self.output_threshold = output_threshold
        self._models = {}
        self.n_classes = None                                       # of the model, known once it has run

    def category_ids(self):
        from .constants import DEFAULT_DETECTOR_LABEL_MAP
        return category_ids_to_include(self, DEFAULT_DETECTOR_LABEL_MAP)

    @property
    def filter(self):
        return FILTERS[self.interpolation]

    def model_on(self, device=None):
        """the model ready to run (eval mode) on `device` (None: the host).  A path is loaded with torch.jit.load
        (run_classifier.py:186); a Module handed in stays where it is, and a copy of it goes to a device"""
        key = str(device)
        if key not in self._models:
            import copy
            import torch
            model = self.model
            if isinstance(model, (str, bytes)) or hasattr(model, '__fspath__'):
                model = torch.jit.load(model, map_location=device or 'cpu')
            elif isinstance(model, torch.nn.Module) and device is not None:
                model = copy.deepcopy(model).to(device)
            if isinstance(model, torch.nn.Module):
                model.eval()
            self._models[key] = model
        return self._models[key]

    def model_name(self):
        import os
        return os.path.basename(str(self.model)) if isinstance(self.model, (str, bytes)) or hasattr(self.model, '__fspath__') \
            else type(self.model).__name__


# ---- which pixels ----------------------------------------------------------------------------------------------------------

def crop_canvas(bbox, width, height, square=True):
    """
    crop_detections.py:422-449 (save_crop) for a normalised [x, y, w, h] box of a width x height image, as a CANVAS:
    (canvas_w, canvas_h, off_x, off_y, (x0, y0, x1, y1)) -- the canvas is 0 except for the rectangle of x1 - x0 by y1 - y0
    pixels at (off_x, off_y), which holds the image's pixels x0 .. x1 - 1, y0 .. y1 - 1; the rectangle is None when no image
    pixel lies in the canvas.  None for a crop with a side of 0, which the reference skips (:440), and for a box wider and
    higher than its image (see the module's text).
    """
    xmin, ymin = int(bbox[0] * width), int(bbox[1] * height)            # :423-424
    box_w, box_h = int(bbox[2] * width), int(bbox[3] * height)          # :425-426
    box_size = None
    if square:                                                          # :428-438
        box_size = max(box_w, box_h)
        xmin = max(0, min(xmin - int((box_size - box_w) / 2), width - box_w))
        ymin = max(0, min(ymin - int((box_size - box_h) / 2), height - box_h))
        box_w, box_h = min(width, box_size), min(height, box_size)
    if box_w <= 0 or box_h <= 0:                                        # :440 (a negative side: Image.crop raises)
        return None
    # Image.crop(box=[xmin, ymin, xmin + box_w, ymin + box_h]) (:445): what lies outside the image is 0
    x0, y0, x1, y1 = max(xmin, 0), max(ymin, 0), min(xmin + box_w, width), min(ymin + box_h, height)
    rect = (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None
    off_x, off_y = max(-xmin, 0), max(-ymin, 0)
    canvas_w, canvas_h = box_w, box_h
    if square and box_w != box_h:                                       # :447-449 ImageOps.pad(crop, (box_size, box_size), color=0)
        if box_w != box_size and box_h != box_size:
            return None                                                 # (pad would resize the crop first)
        # ImageOps.pad pastes at round((size - side) * 0.5) along the axis that is short, Python's round
        if box_w != box_size:
            off_x += int(round((box_size - box_w) * 0.5))
        else:
            off_y += int(round((box_size - box_h) * 0.5))
        canvas_w = canvas_h = box_size
    return canvas_w, canvas_h, off_x, off_y, rect


def pick_crops(detections, width, height, options, category_ids=None, name='', warn=print):
    """-> ([(detection_index, canvas)], skipped) of one image: the detections at or above the threshold and in the categories
    asked for, their index the position in the list as the results file holds it
    (merge_classification_detection_output.py:329-331)"""
    picked, skipped = [], 0
    for index, det in select_crops(output_order(detections, options.output_threshold), options, category_ids):
        canvas = crop_canvas(det['bbox'], width, height, options.square_crops)
        if canvas is None:
            skipped += 1
            warn('Warning: no classification for detection {} of {}: its box {} gives no crop in a {} x {} image'.format(
                index, name, det['bbox'], width, height))
            continue
        picked.append((index, canvas))
    return picked, skipped


def canvas_pixels(pixels, canvas):
    """the canvas as an H x W x 3 uint8 array; pixels: the image the canvas's rectangle indexes"""
    import numpy as np
    canvas_w, canvas_h, off_x, off_y, rect = canvas
    out = np.zeros((canvas_h, canvas_w, 3), np.uint8)
    if rect is not None:
        x0, y0, x1, y1 = rect
        out[off_y:off_y + y1 - y0, off_x:off_x + x1 - x0] = pixels[y0:y1, x0:x1]
    return out


def resized_geometry(canvas_w, canvas_h, size):
    """[3P] torchvision Resize(size) and CenterCrop(size) of a canvas: (resized_w, resized_h, left, top)"""
    short, long = (canvas_w, canvas_h) if canvas_w <= canvas_h else (canvas_h, canvas_w)
    new_long = int(size * long / short)
    w, h = (size, new_long) if canvas_w <= canvas_h else (new_long, size)
    return w, h, int(round((w - size) / 2.0)), int(round((h - size) / 2.0))


def classifier_input_host(pixels, canvas, options):
    """
    run_classifier.py:134-141 for one crop, with PIL and numpy: the canvas (optionally through the JPEG file round trip of
    crop.save(path) / Image.open at options.jpeg_quality), [3P] Resize(S, interpolation), CenterCrop(S), ToTensor (/ 255 in
    float32), Normalize ((x - mean) / std in float32).  -> float32 [3][S][S].  The host leg and the tests' reference.
    """
    import numpy as np
    from PIL import Image
    size = options.image_size
    image = Image.fromarray(canvas_pixels(pixels, canvas))
    if options.jpeg_quality is not None:
        import io
        bio = io.BytesIO()
        image.save(bio, format='JPEG', quality=options.jpeg_quality)
        image = Image.open(io.BytesIO(bio.getvalue())).convert('RGB')
    w, h, left, top = resized_geometry(image.width, image.height, size)
    if (w, h) != image.size:
        image = image.resize((w, h), {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR, 'lanczos': Image.LANCZOS}[options.interpolation])
    a = np.asarray(image)[top:top + size, left:left + size].astype(np.float32) / np.float32(255)
    a = (a - np.array(options.mean, np.float32)) / np.array(options.std, np.float32)
    return np.ascontiguousarray(a.transpose(2, 0, 1))


# ---- the model and its output -------------------------------------------------------------------------------------------------

def run_model(model, x, batch_size):
    """run_classifier.py:217-221: the model under no_grad on chunks of batch_size crops, softmax(dim=1) -> a tensor where x is"""
    import torch
    with torch.no_grad():
        return torch.cat([torch.nn.functional.softmax(model(x[i:i + batch_size]), dim=1) for i in range(0, len(x), batch_size)])


def classification_list(probs, threshold):
    """
    merge_classification_detection_output.py:119-133 for one row of probabilities: [[str(class), conf], ...] of the classes
    at or above the threshold, conf rounded to 4 digits (ct_utils.round_float: Python's round), sorted by the rounded value,
    descending and stable.  The reference carries the row from run_classifier.py to the merge script in a CSV: a value is
    float(str(numpy.float32(p))) here, the shortest decimal of the fp32 probability, which is the reading of that CSV leg.
    """
    import numpy as np
    result = [[str(i), float(str(np.float32(p)))] for i, p in enumerate(probs)]
    result = [[k, round(conf, 4)] for k, conf in result if conf >= threshold]
    return sorted(result, key=lambda x: x[1], reverse=True)


def load_categories(categories, n_classes=None):
    """run_classifier.py:178-182, 223-224: {"0": name, ...} from a JSON file (or a dict), or str(i) for every class"""
    if categories is None:
        return None if n_classes is None else {str(i): str(i) for i in range(n_classes)}
    if not isinstance(categories, dict):
        with open(categories, 'r') as f:
            categories = json.load(f)
    return {str(i): categories[str(i)] for i in range(len(categories))}


# ---- the two legs ---------------------------------------------------------------------------------------------------------------

def _lists(probs, options):
    options.n_classes = int(probs.shape[1])
    return [classification_list(row, options.classification_threshold) for row in probs]


def classifications_of_host_image(pixels, name, detections, options, category_ids=None, warn=print):
    """the host leg for one image, from an H x W x 3 uint8 array: -> ([(detection_index, list)], skipped)"""
    import numpy as np
    import torch
    picked, skipped = pick_crops(detections, pixels.shape[1], pixels.shape[0], options, category_ids, name, warn)
    if not picked:
        return [], skipped
    x = torch.from_numpy(np.stack([classifier_input_host(pixels, canvas, options) for _, canvas in picked]))
    probs = run_model(options.model_on(None), x, options.batch_size).numpy()
    return [(index, lst) for (index, _), lst in zip(picked, _lists(probs, options))], skipped


def classifier_inputs_of_device_images(ctx, jobs, options, ext):
    """
    The tensor of crops of images in device memory: jobs = [(tensor, width, canvas)], tensor a flat uint8 torch tensor of the
    image's height * width * 3 bytes, every canvas with a rectangle and a plan (jpeg_host.classifier_plan).  ONE
    mdhip_classifier_input for all of them; with options.jpeg_quality the canvases are materialised and go through
    mdhip_jpeg_recompress first.  -> float32 [n][3][S][S] on the device, made on the torch stream `ext`.
    """
    import torch
    size, device = options.image_size, jobs[0][0].device
    keep = []
    if options.jpeg_quality is None:
        recs = [(t.data_ptr() + y0 * w * 3 + x0 * 3, w * 3, x1 - x0, y1 - y0, cw, ch, ox, oy) for t, w, (cw, ch, ox, oy, (x0, y0, x1, y1)) in jobs]
    else:
        with torch.cuda.stream(ext):
            for t, w, (cw, ch, ox, oy, (x0, y0, x1, y1)) in jobs:
                canvas = torch.zeros(ch * cw * 3, dtype=torch.uint8, device=device)
                canvas.view(ch, cw * 3)[oy:oy + y1 - y0, ox * 3:(ox + x1 - x0) * 3] = t.view(-1, w * 3)[y0:y1, x0 * 3:x1 * 3]
                keep.append((canvas, torch.empty_like(canvas)))
        sizes = [(job[2][0], job[2][1]) for job in jobs]
        ctx.jpeg_recompress([a.data_ptr() for a, _ in keep], sizes, [cw * 3 for cw, _ in sizes], options.jpeg_quality,
                            [b.data_ptr() for _, b in keep], stream=ext.cuda_stream)
        recs = [(b.data_ptr(), cw * 3, cw, ch, cw, ch, 0, 0) for (_, b), (cw, ch) in zip(keep, sizes)]
    with torch.cuda.stream(ext):
        x = torch.empty((len(jobs), 3, size, size), dtype=torch.float32, device=device)
    if not ctx.classifier_input(recs, size, x.data_ptr(), options.filter, options.mean, options.std, stream=ext.cuda_stream):
        raise RuntimeError('mdhip_classifier_input refused a crop its plan accepts')
    for pair in keep:
        for t in pair:
            t.record_stream(ext)
    return x


def classifications_of_device_images(ctx, entries, options, category_ids=None, stream=0, warn=print):
    """
    The classifications of a batch of images that lie in device memory.  entries: [(tensor, width, height, name, detections)],
    tensor a flat uint8 torch tensor of height * width * 3 bytes, which is not changed.  Returns ([[(detection_index, list)]
    per entry], counts): per chunk of options.batch_size crops, across all images, ONE kernel launch makes the model's input,
    the model runs on it on the same stream, and the probabilities come back in one copy (counts['gpu']).  A crop the kernel
    refuses (reduced more than fits on chip) or without an image pixel goes through the host leg, from its own pixels alone
    (counts['host']); a crop with a side of 0 is counted as 'skipped'.
    """
    import numpy as np
    import torch
    from . import jpeg_host
    counts = {'gpu': 0, 'host': 0, 'skipped': 0}
    out = [[] for _ in entries]
    gpu, host = [], []                                                  # (entry, detection index, canvas)
    for e, (tensor, width, height, name, detections) in enumerate(entries):
        picked, skipped = pick_crops(detections, width, height, options, category_ids, name, warn)
        counts['skipped'] += skipped
        for index, canvas in picked:
            on_device = canvas[4] is not None and jpeg_host.classifier_plan(canvas[0], canvas[1], options.image_size, options.filter) is not None
            (gpu if on_device else host).append((e, index, canvas))
    if not gpu and not host:
        return out, counts
    device = entries[0][0].device
    ext = device_stream(stream, device)
    results = {}
    if gpu:
        model = options.model_on(device)
        parts = []
        for start in range(0, len(gpu), options.batch_size):
            chunk = gpu[start:start + options.batch_size]
            x = classifier_inputs_of_device_images(ctx, [(entries[e][0], entries[e][1], canvas) for e, _, canvas in chunk], options, ext)
            with torch.cuda.stream(ext):
                parts.append(run_model(model, x, options.batch_size))
        with torch.cuda.stream(ext):
            probs = torch.cat(parts).cpu().numpy()                       # (one copy back; it waits for the stream)
        for (e, index, _), lst in zip(gpu, _lists(probs, options)):
            results[(e, index)] = lst
        counts['gpu'] = len(gpu)
    if host:
        xs = []
        for e, _, (cw, ch, ox, oy, rect) in host:
            tensor, width = entries[e][0], entries[e][1]
            pixels = None
            if rect is not None:
                x0, y0, x1, y1 = rect
                with torch.cuda.stream(ext):
                    pixels = tensor.view(-1, width * 3)[y0:y1, x0 * 3:x1 * 3].contiguous().cpu().numpy().reshape(y1 - y0, x1 - x0, 3)
                rect = (0, 0, x1 - x0, y1 - y0)
            xs.append(classifier_input_host(pixels, (cw, ch, ox, oy, rect), options))
        probs = run_model(options.model_on(None), torch.from_numpy(np.stack(xs)), options.batch_size).numpy()
        for (e, index, _), lst in zip(host, _lists(probs, options)):
            results[(e, index)] = lst
        counts['host'] = len(host)
    for (e, index), lst in sorted(results.items()):
        out[e].append((index, lst))
    return out, counts


class ClassifyProduct(Product):
    """classify=: result['classifications'] = [(detection_index, [[class_id, conf], ...])], counted per crop in
    HIPDetector.classify_counts"""

    key = 'classifications'

    def nothing(self):
        return []

    def of_host_image(self, pixels, name, detections):
        value, skipped = classifications_of_host_image(pixels, name, detections, self.options, self.options.category_ids())
        self.counts['host'] += len(value)
        self.counts['skipped'] += skipped
        return value

    def _device(self, ctx, entries, stream):
        return classifications_of_device_images(ctx, entries, self.options, self.options.category_ids(), stream=stream)


def annotate_results(output, classifications, options, completion_time, n_classes=None):
    """
    merge_classification_detection_output.py:307-335 on a results dict IN PLACE: 'classifications' on every classified
    detection -- classifications: {file as the results hold it: [(detection_index, list)]} -- 'classification_categories' at
    the top level, info['classifier'] and info['classification_completion_time'].
    """
    output['info'].update({'classifier': options.model_name(), 'classification_completion_time': completion_time})
    output['classification_categories'] = load_categories(options.categories, n_classes or options.n_classes or 0)
    for im in output['images']:
        for index, lst in classifications.get(im['file'], []):
            im['detections'][index]['classifications'] = lst
    return output


__all__ = ['ClassifyOptions', 'ClassifyProduct', 'FILTERS', 'annotate_results', 'canvas_pixels', 'classification_list',
           'classifications_of_device_images', 'classifications_of_host_image', 'classifier_input_host',
           'classifier_inputs_of_device_images', 'crop_canvas', 'load_categories', 'pick_crops', 'resized_geometry', 'run_model']
