"""
Annotated preview copies, as the reference writes them (visualization/visualize_detector_output.py _render_image: open the
file again, optionally blur_detections, visualization_utils.resize_image to 1000 pixels wide with Pillow's LANCZOS filter,
render_detection_bounding_boxes, Image.save to anno_<name>), from an image that is in device memory already: the GPU blurs a
copy (HipContext.blur_regions), resamples it (HipContext.resample_lanczos, Pillow's arithmetic bit for bit), draws the boxes
and their labels (HipContext.draw_ops) and encodes the result (HipContext.jpeg_encode); the host puts the file around the
scan (jpeg_host.jfif_file).  No second read or decode of the source file, no resample and no encode on the host.

What the reference draws is restated here as a PLAN (render_plan): an ordered list of solid rectangles and of small label
patches that PIL rasterises on the host, once per distinct label.  Whatever the plan does not restate -- a box thinner than
its own outline, ink that may leave a label's patch, a confidence of None -- sends the image to the HOST LEG
(preview_file_of_host_image), which draws with PIL's own calls in the reference's order, so a run writes the same files
either way.  A caller that asks by name (render_plan(thin_outlines=True): visualize_db.py, whose ground-truth boxes are often
tiny) keeps a box thinner than its outline on the device: thin_outline_ops takes its pixels from Pillow, once per box size.

Two deliberate differences from the reference script: the HTML index is not written, and an image whose resize target is not
positive is skipped and counted (the reference asserts, which its caller reports as a rendering failure of that image: no
file either).  Image.save(path) copies no EXIF block, and neither do these files; what Pillow does carry from the opened
file into the saved one through Image.info -- a JPEG's COM segment, a PNG's ICC profile -- is not written, as for the crops.
"""

import os

from . import jpeg_host
from .crops import Product, device_stream, files_of_device_images, output_order, write_file, _pil_file

DEFAULT_PREVIEW_CONFIDENCE_THRESHOLD = 0.15     # visualize_detector_output.py:177 confidence_threshold=0.15
DEFAULT_PREVIEW_WIDTH = 1000                    # visualize_detector_output.py:179 output_image_width=1000
DEFAULT_BOX_THICKNESS = 4                       # visualization_utils.py:64
DEFAULT_LABEL_FONT_SIZE = 16                    # visualization_utils.py:65
DEFAULT_LABEL_FONT = 'arial.ttf'                # visualization_utils.py:66
DEFAULT_PREVIEW_QUALITY = 75                    # visualize_detector_output.py:159 image.save(path): Pillow's JPEG default

# visualization_utils.py:72-96 DEFAULT_COLORS: the colour of a box is entry int(category) % 126, so the order is behaviour
PREVIEW_COLORS = (
    'AliceBlue Red RoyalBlue Gold Chartreuse Aqua Azure Beige Bisque BlanchedAlmond BlueViolet BurlyWood CadetBlue AntiqueWhite '
    'Chocolate Coral CornflowerBlue Cornsilk Crimson Cyan DarkCyan DarkGoldenRod DarkGrey DarkKhaki DarkOrange DarkOrchid '
    'DarkSalmon DarkSeaGreen DarkTurquoise DarkViolet DeepPink DeepSkyBlue DodgerBlue FireBrick FloralWhite ForestGreen Fuchsia '
    'Gainsboro GhostWhite GoldenRod Salmon Tan HoneyDew HotPink IndianRed Ivory Khaki Lavender LavenderBlush LawnGreen '
    'LemonChiffon LightBlue LightCoral LightCyan LightGoldenRodYellow LightGray LightGrey LightGreen LightPink LightSalmon '
    'LightSeaGreen LightSkyBlue LightSlateGray LightSlateGrey LightSteelBlue LightYellow Lime LimeGreen Linen Magenta '
    'MediumAquaMarine MediumOrchid MediumPurple MediumSeaGreen MediumSlateBlue MediumSpringGreen MediumTurquoise '
    'MediumVioletRed MintCream MistyRose Moccasin NavajoWhite OldLace Olive OliveDrab Orange OrangeRed Orchid PaleGoldenRod '
    'PaleGreen PaleTurquoise PaleVioletRed PapayaWhip PeachPuff Peru Pink Plum PowderBlue Purple RosyBrown Aquamarine '
    'SaddleBrown Green SandyBrown SeaGreen SeaShell Sienna Silver SkyBlue SlateBlue SlateGray SlateGrey Snow SpringGreen '
    'SteelBlue GreenYellow Teal Thistle Tomato Turquoise Violet Wheat White WhiteSmoke Yellow YellowGreen').split()

NUM_DETECTOR_CATEGORIES = 3                     # data_management/annotation_constants.py: animal, person, vehicle
DEFAULT_CLASSIFICATION_CONFIDENCE_THRESHOLD = 0.3       # render_detection_bounding_boxes' defaults
MAX_CLASSIFICATIONS = 3

OP_RECT, OP_PATCH = 0, 1                        # csrc/resample.h MD_DRAW_RECT / MD_DRAW_PATCH
_COORD_LIMIT = 1 << 30                          # operations carry int32 coordinates


class PreviewOptions:
    """which images are rendered and how (defaults: visualize_detector_output's own)"""

    def __init__(self, confidence_threshold=DEFAULT_PREVIEW_CONFIDENCE_THRESHOLD, output_image_width=DEFAULT_PREVIEW_WIDTH,
                 detections_only=False, preserve_path_structure=False, box_thickness=DEFAULT_BOX_THICKNESS, box_expansion=0,
                 label_font_size=DEFAULT_LABEL_FONT_SIZE, label_font=DEFAULT_LABEL_FONT, box_sort_order='confidence',
                 blur_categories=None, quality=DEFAULT_PREVIEW_QUALITY, output_threshold=None):
        # visualize_detector_output.py:279-280
        if not 0 <= confidence_threshold <= 1:
            raise ValueError('confidence threshold {!r} is outside 0 .. 1'.format(confidence_threshold))
        self.confidence_threshold = confidence_threshold
        self.output_image_width = -1 if output_image_width is None else int(output_image_width)
        self.detections_only = bool(detections_only)
        self.preserve_path_structure = bool(preserve_path_structure)
        label_font_size = DEFAULT_LABEL_FONT_SIZE if label_font_size is None else label_font_size      # visualization_utils.py:645-646
        # visualization_utils.py:996-997
        if box_thickness == 0 or label_font_size == 0:
            raise ValueError('box thickness and label font size cannot be zero')
        if box_thickness < 0 or box_expansion < 0 or label_font_size < 0:
            raise ValueError('box thickness, box expansion and label font size cannot be negative')
        self.box_thickness, self.box_expansion = box_thickness, box_expansion
        self.label_font_size = label_font_size
        self.label_font = DEFAULT_LABEL_FONT if label_font is None else label_font
        if box_sort_order not in (None, 'confidence', 'reverse_confidence'):
            raise ValueError('Unrecognized sorting scheme {}'.format(box_sort_order))    # visualization_utils.py:671
        self.box_sort_order = box_sort_order
        if isinstance(blur_categories, str):
            blur_categories = [s.strip() for s in blur_categories.split(',') if s.strip()]
        self.blur_categories = tuple(blur_categories) if blur_categories else None
        self.quality = jpeg_host.check_quality(quality)
        # the confidence threshold of the results file, as for blur.BlurOptions: the reference renders what that file holds
        self.output_threshold = output_threshold

    def blur_category_ids(self, label_map=None):
        """visualize_detector_output.py:118-124: the ids whose NAME is one to blur (a name no category has selects nothing)"""
        if self.blur_categories is None:
            return set()
        return {k for k, v in _label_map(label_map).items() if v in self.blur_categories}


def _label_map(label_map):
    if label_map is None:
        from .constants import DEFAULT_DETECTOR_LABEL_MAP
        return DEFAULT_DETECTOR_LABEL_MAP
    return label_map


NO_LABELS = 'no_detection_labels'               # visualize_detector_output.py:282-285: boxes without labels


# ---- which images, which size, which name ----------------------------------------------------------------------------------

def target_size(width, height, target_width):
    """
    visualization_utils.resize_image(image, target_width) (:367-417): the size the image is resized to, (width, height) itself
    when there is nothing to resize, None for a target that is not positive (the reference asserts).
    """
    if target_width is None or target_width == -1:
        return width, height
    aspect_ratio = width / height                                   # :385
    target_height = int(target_width / aspect_ratio)                # :389
    if target_width == width and target_height == height:           # :403
        return width, height
    if not (target_width > 0 and target_height > 0):                # :416
        return None
    return target_width, target_height


def resized_size(width, height, target_width):
    """the size resize_image(image, target_width) gives (target_size); the reference's assertion for a target that is not
    positive"""
    size = target_size(width, height, target_width)
    assert size is not None, 'Invalid image resize target {},{}'.format(target_width, int(target_width / (width / height)))
    return size


def output_name(image_file, options):
    """visualize_detector_output.py:150-156: the path below the output folder; image_file is relative to the image folder"""
    if options.preserve_path_structure:
        if os.path.isabs(image_file):
            raise ValueError("Can't preserve paths when operating on absolute paths")
        return image_file
    for char in ['/', '\\', ':']:
        image_file = image_file.replace(char, '~')
    return 'anno_' + image_file


def file_detections(detections, options):
    """the detections as the results file holds them (crops.output_order): what the reference script reads"""
    return output_order(detections, options.output_threshold)


def is_rendered(result, options):
    """visualize_detector_output.py:79-90: not an image that failed, and not one below the threshold with detections_only"""
    if result.get('failure') is not None or result.get('detections') is None:
        return False
    confs = [d['conf'] for d in file_detections(result['detections'], options)]
    max_conf = max(confs) if confs else 0.0                          # ct_utils.get_max_conf
    return not (max_conf < options.confidence_threshold and options.detections_only)


def rectangles_to_blur(detections, width, height, options, label_map=None):
    """visualize_detector_output.py:126-131: blur_detections' rectangles for the boxes of the categories to blur at or above
    the threshold, in the order of the file"""
    from .blur import blur_rectangle
    ids = options.blur_category_ids(label_map)
    rects = [blur_rectangle(d['bbox'], width, height) for d in file_detections(detections, options)
             if d['conf'] >= options.confidence_threshold and d['category'] in ids]
    return [r for r in rects if r is not None]


# ---- what is drawn ---------------------------------------------------------------------------------------------------------

def resolve_sizes(options, im_width):
    """visualization_utils.py:1002-1013: thickness, expansion and font size in pixels; a value in (0, 1) is a fraction of the
    image width"""
    thickness, expansion, font_size = options.box_thickness, options.box_expansion, options.label_font_size
    if 0 < thickness < 1:
        thickness = max(1, round(thickness * im_width))
    if 0 < expansion < 1:
        expansion = round(expansion * im_width)
    if 0 < font_size < 1:
        font_size = max(1, round(font_size * im_width))
    return int(thickness), int(expansion), int(font_size)


_FONTS = {}


def load_font(label_font, label_font_size):
    """visualization_utils._load_font (:895-915): the named font, else Pillow's default at that size, else its default"""
    key = (label_font, label_font_size)
    if key not in _FONTS:
        from PIL import ImageFont
        font = None
        try:
            font = ImageFont.truetype(label_font, label_font_size)
        except Exception:
            font = None
        if font is None:
            try:
                font = ImageFont.load_default(label_font_size)
            except Exception:
                font = None
        if font is None:
            font = ImageFont.load_default()
        _FONTS[key] = font
    return _FONTS[key]


def text_size(font, s):
    """visualization_utils.get_text_size (:865-892): right and bottom of the text's box, NOT its width and height"""
    try:
        _, _, w, h = font.getbbox(s)
    except Exception:
        w, h = font.getsize(s)
    return w, h


def box_color(category, colormap=None):
    """visualization_utils.py:978-988 (name, (r, g, b)); colormap: None for DEFAULT_COLORS, or a list of colour names -- the
    class index is taken % len(colormap), and a class of None takes colormap[1] as there (IndexError for a list of one)"""
    from PIL import ImageColor
    colors = PREVIEW_COLORS if colormap is None else colormap
    name = colors[1] if category is None else colors[int(category) % len(colors)]
    return name, ImageColor.getrgb(name)[:3]


def drawn_detections(detections, options, category_thresholds=None):
    """render_detection_bounding_boxes :664-684: the order the boxes are drawn in -- ascending confidence, so that the most
    confident box lands on top (a stable sort: equal confidences keep the file's order) -- and only those at or above the
    threshold (a confidence of None is always drawn).  category_thresholds: None, or the reference's confidence_threshold as
    a dict (:677-680) -- category id -> threshold, consulted instead of options.confidence_threshold; a category it lacks is
    KeyError as there, and a threshold of None draws every box of the category"""
    return [d for _, d in _drawn_with_positions(detections, options, category_thresholds)]


def _drawn_with_positions(detections, options, category_thresholds=None):
    """drawn_detections with, for every drawn detection, the reference's i_detection (:673): its position in the list the
    loop runs over, which is the SORTED list when there is a sort order"""
    dets = list(file_detections(detections, options))
    if options.box_sort_order is not None:
        dets = sorted(dets, key=lambda d: (d['conf'] is not None, d['conf']), reverse=options.box_sort_order == 'reverse_confidence')
    if category_thresholds is None:
        return [(i, d) for i, d in enumerate(dets) if d['conf'] is None or d['conf'] >= options.confidence_threshold]
    drawn = []
    for i, d in enumerate(dets):
        threshold = category_thresholds[d['category']]
        if d['conf'] is None or threshold is None or d['conf'] >= threshold:
            drawn.append((i, d))
    return drawn


def label_string(det, label_map):
    """render_detection_bounding_boxes :696-703; label_map None: no label"""
    if label_map is None:
        return ''
    label = label_map[det['category']] if det['category'] in label_map else det['category']
    if det['conf'] is None:
        return '{}'.format(label)
    return '{}: {}%'.format(label, round(100 * det['conf']))


def box_edges(bbox, width, height, expansion):
    """draw_bounding_box_on_image :1015-1042: (left, top, right, bottom) of a normalised [x, y, w, h] box as floats, expanded
    and, only then, clamped to the image"""
    x1, y1, w_box, h_box = bbox
    ymin, xmin, ymax, xmax = y1, x1, y1 + h_box, x1 + w_box          # render_detection_bounding_boxes :686-687
    return corner_edges(ymin, xmin, ymax, xmax, width, height, expansion)


def corner_edges(ymin, xmin, ymax, xmax, width, height, expansion):
    """box_edges for a box that is given as draw_bounding_box_on_image takes it: normalised (ymin, xmin, ymax, xmax)"""
    left, right, top, bottom = xmin * width, xmax * width, ymin * height, ymax * height
    if expansion > 0:
        left -= expansion
        right += expansion
        top -= expansion
        bottom += expansion
        left, right, top, bottom = max(left, 0), max(right, 0), max(top, 0), max(bottom, 0)
        left, right = min(left, width - 1), min(right, width - 1)
        top, bottom = min(top, height - 1), min(bottom, height - 1)
    return left, top, right, bottom


def classified_label_lines(det, label_map, classification_label_map,
                           classification_confidence_threshold=DEFAULT_CLASSIFICATION_CONFIDENCE_THRESHOLD):
    """render_detection_bounding_boxes :691-769 for one drawn detection: (its label lines -- the detection's, then one per
    classification at or above the threshold, at most MAX_CLASSIFICATIONS looked at --, the class its colour is of: the
    detection's category, or NUM_DETECTOR_CATEGORIES + the best classification's)"""
    clss = det['category']
    strings = [label_string(det, label_map)]
    if ('classifications' in det) and len(det['classifications']) > 0:
        classifications = det['classifications']
        if len(classifications) > MAX_CLASSIFICATIONS:
            classifications = classifications[0:MAX_CLASSIFICATIONS]
        max_category, max_conf = 0, -100
        if classification_label_map is not None:
            for class_key, conf in (c[:2] for c in classifications):
                if conf is None or conf < classification_confidence_threshold:
                    continue
                if conf > max_conf:
                    max_conf, max_category = conf, int(class_key)
                if class_key in classification_label_map:
                    class_name = classification_label_map[class_key]
                elif str(class_key) in classification_label_map:
                    class_name = classification_label_map[str(class_key)]
                else:
                    class_name = str(class_key)
                strings += ['{}: {}%'.format(class_name.lower(), str(round(100.0 * conf, 1)))]
        clss = NUM_DETECTOR_CATEGORIES + max_category
    return strings, clss


def stacked_labels(font, strings, left, top, bottom, im_height, vtextalign='top'):
    """draw_bounding_box_on_image :1052-1131 for the label lines of one box, left-aligned, in the order they are drawn:
    the last line first, at the bottom, every further line int(text_height + 2 * margin) higher.  vtextalign 'top'
    (VTEXTALIGN_TOP): above the box, below it when that leaves the image at the top, inside it at the top when below leaves
    the image too.  'bottom' (VTEXTALIGN_BOTTOM, :1112-1116): below the box, above it when that leaves the image at the
    bottom, inside it at the bottom when above leaves the image too.  Yields (the padded string, its margin, the corners
    (x0, y0), (x1, y1) of its filled rectangle (inclusive), where its text goes)."""
    import numpy as np
    if vtextalign not in ('top', 'bottom'):
        raise ValueError('Unrecognized vertical text alignment {}'.format(vtextalign))
    total_height = (1 + 2 * 0.05) * sum(text_size(font, s)[1] for s in strings)     # :1055 (of the strings WITHOUT their padding)
    for i_str, s in enumerate(strings[::-1]):
        if len(s) == 0:                                                              # :1061
            continue
        s = ' ' + s + ' '
        text_width, text_height = text_size(font, s)
        margin = int(np.ceil(0.05 * text_height))
        if vtextalign == 'top':
            text_bottom = top
            if (text_bottom - total_height) < 0:
                text_bottom = bottom + total_height
                if text_bottom > im_height:
                    text_bottom = top + total_height
        else:
            text_bottom = bottom + total_height
            if text_bottom > im_height:
                text_bottom = top
                if (text_bottom - total_height) < 0:
                    text_bottom = bottom
        text_bottom = int(text_bottom) - i_str * (int(text_height + (2 * margin)))
        text_left = int(left)
        yield (s, margin, (text_left, (text_bottom - text_height) - (2 * margin)), (text_left + text_width, text_bottom),
               (text_left + margin, text_bottom - text_height - margin))


def label_box(font, s, left, top, bottom, im_height):
    """stacked_labels for ONE label that is not empty: the padded string, its margin and the filled rectangle (x0, y0, x1, y1
    inclusive) the text is drawn into at (x0 + margin, y0 + margin)"""
    padded, margin, (x0, y0), (x1, y1), _ = next(stacked_labels(font, [s], left, top, bottom, im_height))
    return padded, margin, (x0, y0, x1, y1)


class HostLeg(Exception):
    """the plan does not restate what the reference draws for this image: PIL draws it (preview_file_of_host_image)"""


class RenderFailure(Exception):
    """the reference's own drawing raises for this image: it gets no file (visualize_detector_output.py:162-165)"""


def _check_rectangle(left, top, right, bottom):
    # ImageDraw.rectangle refuses reversed corners (Pillow's _draw_rectangle, on the floats)
    if right < left:
        raise RenderFailure('x1 must be greater than or equal to x0')
    if bottom < top:
        raise RenderFailure('y1 must be greater than or equal to y0')
    if not all(abs(v) < _COORD_LIMIT for v in (left, top, right, bottom)):
        raise HostLeg('a box edge beyond 2^30 pixels')


def outline_ops(left, top, right, bottom, thickness, rgb):
    """
    ImageDraw.rectangle([(left, top), (right, bottom)], outline=color, width=thickness) as four solid rectangles, inward from
    int(left), int(top), int(right), int(bottom) inclusive: the top and bottom bars over the whole width, the side bars
    between them.  Pinned against Pillow for thicknesses 1 .. 5 (tests/test_preview_cpu.py): equal for every box at least
    2 * thickness pixels wide and high, in and out of the image; a thinner box Pillow draws otherwise -> HostLeg.
    """
    _check_rectangle(left, top, right, bottom)
    x0, y0, x1, y1 = int(left), int(top), int(right), int(bottom)
    t = thickness
    if x1 - x0 + 1 < 2 * t or y1 - y0 + 1 < 2 * t:
        raise HostLeg('a box of {} x {} pixels with an outline of {}'.format(x1 - x0 + 1, y1 - y0 + 1, t))
    c = rgb[0] | rgb[1] << 8 | rgb[2] << 16
    return [[OP_RECT, x0, y0, x1, y0 + t - 1, c, 0, 0], [OP_RECT, x0, y1 - t + 1, x1, y1, c, 0, 0],
            [OP_RECT, x0, y0 + t, x0 + t - 1, y1 - t, c, 0, 0], [OP_RECT, x1 - t + 1, y0 + t, x1, y1 - t, c, 0, 0]]


def is_thin(left, top, right, bottom, thickness):
    """whether outline_ops hands this box over: narrower or lower than twice its outline"""
    return int(right) - int(left) + 1 < 2 * thickness or int(bottom) - int(top) + 1 < 2 * thickness


_THIN_OUTLINES = {}


def _thin_outline_rectangles(width, height, thickness):
    """What ImageDraw.rectangle(outline=, width=thickness) sets for a box of width x height pixels, rasterised by Pillow once on
    a scratch canvas with room for what spills (its bars are as long as the outline is thick, whatever the box): ->
    [(dx0, dy0, dx1, dy1)] inclusive, relative to the box's top left corner -- the runs of every row, equal runs of consecutive
    rows as one rectangle"""
    key = (width, height, thickness)
    if key not in _THIN_OUTLINES:
        import numpy as np
        from PIL import Image, ImageDraw
        if len(_THIN_OUTLINES) > 4096:
            _THIN_OUTLINES.clear()
        m = 2 * thickness + 2
        canvas = Image.new('L', (width + 2 * m, height + 2 * m), 0)
        ImageDraw.Draw(canvas).rectangle([(m, m), (m + width - 1, m + height - 1)], outline=255, width=thickness)
        ink = np.asarray(canvas) != 0
        assert not (ink[0].any() or ink[-1].any() or ink[:, 0].any() or ink[:, -1].any()), 'the outline reaches the scratch canvas edge'
        rectangles, open_runs = [], {}                                    # (x0, x1) -> the row the rectangle began in
        for y in range(ink.shape[0] + 1):
            runs = []
            if y < ink.shape[0] and ink[y].any():
                steps = np.diff(np.concatenate(([0], ink[y].astype(np.int8), [0])))
                runs = list(zip(np.flatnonzero(steps == 1).tolist(), (np.flatnonzero(steps == -1) - 1).tolist()))
            for run in [r for r in open_runs if r not in runs]:
                rectangles.append((run[0] - m, open_runs.pop(run) - m, run[1] - m, y - 1 - m))
            for run in runs:
                open_runs.setdefault(run, y)
        _THIN_OUTLINES[key] = sorted(rectangles, key=lambda r: (r[1], r[0]))
    return _THIN_OUTLINES[key]


def thin_outline_ops(left, top, right, bottom, thickness, rgb):
    """
    ImageDraw.rectangle([(left, top), (right, bottom)], outline=color, width=thickness) for a box outline_ops hands over, one
    narrower or lower than 2 * thickness pixels: there Pillow's bars overlap, are not solid and leave the box, so the pixels
    are Pillow's own -- rasterised once per (width, height, thickness) and kept, as label_patch keeps its labels -- as solid
    rectangles offset to int(left), int(top).  Pinned against Pillow for thicknesses 1 .. 8, in the image and across its edge
    (tests/test_visualize_db_cpu.py).  Any box is drawn right; only a thin one is worth a scratch canvas.
    """
    _check_rectangle(left, top, right, bottom)
    x0, y0, x1, y1 = int(left), int(top), int(right), int(bottom)
    c = rgb[0] | rgb[1] << 8 | rgb[2] << 16
    return [[OP_RECT, x0 + a, y0 + b, x0 + p, y0 + q, c, 0, 0] for a, b, p, q in _thin_outline_rectangles(x1 - x0 + 1, y1 - y0 + 1, thickness)]


_PATCHES = {}


def label_patch(font, font_key, padded, margin, size, color_name):
    """the label as pixels: an RGB image of `size` filled with the colour, the text in black at (margin, margin) -- what the
    reference's filled rectangle and draw.text leave in the image.  -> bytes (R G B, 3 * width a row)"""
    key = (font_key, padded, margin, size, color_name)
    if key not in _PATCHES:
        from PIL import Image, ImageDraw
        if len(_PATCHES) > 4096:
            _PATCHES.clear()
        patch = Image.new('RGB', size, color_name)
        ImageDraw.Draw(patch).text((margin, margin), padded, fill='black', font=font)
        _PATCHES[key] = patch.tobytes()
    return _PATCHES[key]


class RenderPlan:
    """ops: rows of 8 int32 in drawing order (include/mdhip.h mdhip_draw_ops), patch offsets into `patches`; labels and
    order: the label string and the index in the file's list of every drawn detection, in drawing order"""

    def __init__(self):
        self.ops, self.patches, self.labels, self.order = [], bytearray(), [], []
        self._offsets = {}

    def add_patch(self, data):
        if data not in self._offsets:
            self._offsets[data] = len(self.patches)
            self.patches += data
        return self._offsets[data]

    def patch_of(self, op):
        """the pixels a PATCH row pastes"""
        return bytes(self.patches[op[5]:op[5] + op[3] * op[4] * 3])

    def extend(self, other):
        """appends what another plan draws (for the same image) behind what this one draws; a patch both hold is kept once"""
        for op in other.ops:
            if op[0] == OP_PATCH:
                op = op[:5] + [self.add_patch(other.patch_of(op))] + op[6:]
            self.ops.append(op)
        self.labels += other.labels
        self.order += other.order
        return self


def box_outline_ops(left, top, right, bottom, thickness, rgb, thin_outlines=False):
    """outline_ops, and with thin_outlines thin_outline_ops for the boxes outline_ops hands over"""
    if thin_outlines:
        _check_rectangle(left, top, right, bottom)
        if is_thin(left, top, right, bottom, thickness):
            return thin_outline_ops(left, top, right, bottom, thickness, rgb)
    return outline_ops(left, top, right, bottom, thickness, rgb)


def add_label_ops(plan, font, font_key, strings, left, top, bottom, height, vtextalign, color_name):
    """appends to `plan` one patch per label line of a box in the order PIL draws them (stacked_labels); raises HostLeg for a
    label the patches do not restate"""
    for padded, margin, (x0, y0), (x1, y1), _ in stacked_labels(font, strings, left, top, bottom, height, vtextalign):
        bbox = font.getbbox(padded)
        if bbox[0] < 0 or bbox[1] < 0:
            raise HostLeg('ink of {!r} may leave its label'.format(padded))
        if not all(isinstance(v, int) or float(v).is_integer() for v in (x0, y0, x1, y1)):
            raise HostLeg('a label of a fractional size')
        x0, y0, x1, y1 = int(x0), int(y0), int(x1), int(y1)
        w, h = x1 - x0 + 1, y1 - y0 + 1
        if w < 1 or h < 1 or w > 32767 or h > 32767:
            raise HostLeg('a label of {} x {} pixels'.format(w, h))
        data = label_patch(font, font_key, padded, margin, (w, h), color_name)
        plan.ops.append([OP_PATCH, x0, y0, w, h, plan.add_patch(data), 0, 0])


def _label_lines(det, label_map, classification_label_map, classification_confidence_threshold, custom_string=None,
                 unlabelled_classifications=False):
    """(the label lines of one drawn detection, the class its colour is of); None for a detection with classifications when
    they are not asked for (no threshold) or cannot be labelled (no label map) -- unless unlabelled_classifications, which
    then does what the reference does without a label map: no classification line, and the colour of the best
    classification it looked at.  custom_string: render_detection_bounding_boxes :705-709, appended to the first line with
    a blank when it is not empty"""
    if classification_confidence_threshold is None or (label_map is None and not unlabelled_classifications):
        if 'classifications' in det and len(det['classifications']) > 0:
            return None
        strings, clss = [label_string(det, label_map)], det['category']
    else:
        strings, clss = classified_label_lines(det, label_map, classification_label_map, classification_confidence_threshold)
    if custom_string is not None and len(custom_string) > 0:
        strings[0] += ' ' + custom_string
    return strings, clss


def _check_custom_strings(custom_strings, listed):
    # render_detection_bounding_boxes :651-654
    if custom_strings is not None:
        assert len(custom_strings) == len(listed), \
            '{} custom strings provided for {} detections'.format(len(custom_strings), len(listed))


def render_plan(detections, width, height, options, label_map=None, labels=True, classification_label_map=None,
                classification_confidence_threshold=None, *, colormap=None, vtextalign='top', custom_strings=None,
                unlabelled_classifications=False, thin_outlines=False, category_thresholds=None):
    """
    render_detection_bounding_boxes(detections, image, label_map=..., confidence_threshold, thickness, expansion,
    label_font_size, label_font, box_sort_order) for an image of width x height (the RESIZED size) as a RenderPlan: per box
    outline_ops, then one patch per label line in the order PIL draws them (stacked_labels).
    labels False: label_map=None of the reference (boxes only).  classification_confidence_threshold None: a box that carries
    classifications is a HostLeg; a number: its classification_label_map=, classification_confidence_threshold= are the
    reference's, and such a box gets a label line per classification and the colour of the best one (classified_label_lines).
    category_thresholds: drawn_detections' (the reference's confidence_threshold as a dict by category id).
    colormap: box_color's; vtextalign: stacked_labels'; custom_strings: None, or one string per detection of the list, indexed
    as the reference indexes it -- by the position in the list its loop runs over, which is the list sorted by confidence
    when there is a sort order, not the file's; unlabelled_classifications: _label_lines'.  What follows
    classification_confidence_threshold is given by name (category_thresholds stays the last argument).  thin_outlines: a box
    thinner than twice its outline is drawn by thin_outline_ops; without it such a box is a HostLeg.
    Raises HostLeg or RenderFailure.
    """
    thickness, expansion, font_size = resolve_sizes(options, width)
    label_map = _label_map(label_map) if labels else None
    font = None
    plan = RenderPlan()
    listed = file_detections(detections, options)
    _check_custom_strings(custom_strings, listed)
    for position, det in _drawn_with_positions(detections, options, category_thresholds):
        if det['conf'] is None:
            raise HostLeg('a detection without a confidence')
        try:
            lines = _label_lines(det, label_map, classification_label_map, classification_confidence_threshold,
                                 None if custom_strings is None else custom_strings[position], unlabelled_classifications)
            if lines is None:
                raise HostLeg('classification labels')
            strings, clss = lines
            color_name, rgb = box_color(clss, colormap)
        except (TypeError, ValueError) as e:
            raise RenderFailure(str(e))
        left, top, right, bottom = box_edges(det['bbox'], width, height, expansion)
        plan.ops += box_outline_ops(left, top, right, bottom, thickness, rgb, thin_outlines)
        plan.labels.append(strings[0])
        plan.order.append(next(i for i, d in enumerate(listed) if d is det))
        if not any(strings):                                                     # :1061
            continue
        if font is None:
            font = load_font(options.label_font, font_size)
        add_label_ops(plan, font, (options.label_font, font_size), strings, left, top, bottom, height, vtextalign, color_name)
    return plan


def render_with_pil(image, detections, options, label_map=None, labels=True, classification_label_map=None,
                    classification_confidence_threshold=None, *, colormap=None, vtextalign='top', custom_strings=None,
                    unlabelled_classifications=False, category_thresholds=None):
    """the same drawing by PIL's own calls in the reference's order (render_detection_bounding_boxes :673-796,
    draw_bounding_box_on_image :990-1137), IN PLACE on a PIL image of the resized size: the host leg.  The arguments are
    render_plan's; a box with classifications that are not asked for is NotImplementedError.  Raises what PIL raises."""
    from PIL import ImageDraw
    width, height = image.size
    thickness, expansion, font_size = resolve_sizes(options, width)
    label_map = _label_map(label_map) if labels else None
    _check_custom_strings(custom_strings, file_detections(detections, options))
    for position, det in _drawn_with_positions(detections, options, category_thresholds):
        lines = _label_lines(det, label_map, classification_label_map, classification_confidence_threshold,
                             None if custom_strings is None else custom_strings[position], unlabelled_classifications)
        if lines is None:
            raise NotImplementedError('classification labels are not rendered')
        strings, clss = lines
        color_name, _ = box_color(clss, colormap)
        draw = ImageDraw.Draw(image)
        left, top, right, bottom = box_edges(det['bbox'], width, height, expansion)
        draw.rectangle([(left, top), (right, bottom)], outline=color_name, width=thickness)
        font = load_font(options.label_font, font_size)
        if not any(strings):
            continue
        for padded, _, corner0, corner1, text_at in stacked_labels(font, strings, left, top, bottom, height, vtextalign):
            draw.rectangle([corner0, corner1], fill=color_name)
            draw.text(text_at, padded, fill='black', font=font)
    return image


# ---- the two legs -----------------------------------------------------------------------------------------------------------

def preview_file_of_host_image(pixels, name, detections, options, label_map=None):
    """
    The host leg, for an image whose pixels are not in device memory or whose drawing the plan does not restate: the
    reference's steps on a copy of the H x W x 3 uint8 array -- blur (libmdjpeg.so: Pillow's blur), Image.resize(LANCZOS),
    PIL's drawing -- saved by PIL in the format of `name` at options.quality.  None for an image that gets no file: a resize
    target that is not positive, or drawing that raises.
    """
    import numpy as np
    from PIL import Image
    height, width = pixels.shape[:2]
    size = target_size(width, height, options.output_image_width)
    if size is None:
        return None
    labels = label_map != NO_LABELS
    label_map = None if not labels else label_map
    copy = np.array(pixels, dtype=np.uint8, order='C')
    rects = rectangles_to_blur(detections, width, height, options, label_map)
    if rects:
        rc = jpeg_host.blur_regions(copy, rects, 40)                 # visualization_utils.py:497 blur_radius=40
        if rc != jpeg_host.MDJPEG_OK:
            raise RuntimeError('mdjpeg_blur_regions returned {}'.format(rc))
    image = Image.fromarray(copy)
    if size != (width, height):
        image = image.resize(size, Image.LANCZOS)
    try:
        render_with_pil(image, detections, options, label_map, labels)
    except Exception as e:
        print('Warning: error rendering {}: {}'.format(name, str(e)))
        return None
    return _pil_file(np.asarray(image), name, options.quality)


def previews_of_device_images(ctx, entries, options, label_map=None, stream=0):
    """
    The previews of a batch of images that lie in device memory.  entries: [(tensor, width, height, name, detections)],
    tensor a flat uint8 torch tensor of height * width * 3 bytes, which is NOT changed; name the output name (its extension
    picks the format).  Returns ([(bytes or None, leg) per entry], counts), leg 'gpu', 'host' or 'skipped': for all images
    together at most ONE blur call (on copies of the images with something to blur), ONE resample call, ONE drawing call and,
    for the names Pillow maps to JPEG, ONE encoder call (counts['gpu']); for any other extension the rendered pixels are
    copied back and PIL saves them (counts['host']).  An image the plan hands to the host leg is copied back as it is and
    PIL renders it (counts['host'] too); one without a file counts as 'skipped'.
    """
    import torch
    from .device_render import blur_rects, draw_plans
    counts = {'gpu': 0, 'host': 0, 'skipped': 0}
    out = [(None, 'skipped')] * len(entries)
    labels = label_map != NO_LABELS
    plan_map = None if not labels else label_map
    jobs, host = [], []                                              # (entry, size, plan, rectangles to blur)
    for e, (tensor, width, height, name, detections) in enumerate(entries):
        size = target_size(width, height, options.output_image_width)
        if size is None:
            continue
        try:
            plan = render_plan(detections, size[0], size[1], options, plan_map, labels)
        except RenderFailure as err:
            print('Warning: error rendering {}: {}'.format(name, str(err)))
            continue
        except HostLeg:
            host.append(e)
            continue
        jobs.append((e, size, plan, rectangles_to_blur(detections, width, height, options, plan_map)))
    if not entries:
        return out, counts
    device = entries[0][0].device
    ext = device_stream(stream, device)
    for e in host:
        tensor, width, height, name, detections = entries[e]
        with torch.cuda.stream(ext):
            pixels = tensor.cpu().numpy().reshape(height, width, 3)
        data = preview_file_of_host_image(pixels, name, detections, options, label_map)
        out[e] = (data, 'host' if data is not None else 'skipped')
    if jobs:
        sizes = [(entries[e][1], entries[e][2]) for e, _, _, _ in jobs]
        with torch.cuda.stream(ext):
            # a copy only where the source would be changed: something to blur, or nothing to resize (drawn in place)
            sources = [entries[e][0].clone() if rects or size == sizes[k] else entries[e][0] for k, (e, size, _, rects) in enumerate(jobs)]
        blurred = [k for k, job in enumerate(jobs) if job[3]]
        blur_rects(ctx, [sources[k].data_ptr() for k in blurred], [sizes[k] for k in blurred], [jobs[k][3] for k in blurred], 40,
                   ext.cuda_stream)
        with torch.cuda.stream(ext):
            rendered = [sources[k] if size == sizes[k] else torch.empty(size[0] * size[1] * 3, dtype=torch.uint8, device=device)
                        for k, (_, size, _, _) in enumerate(jobs)]
        resized = [k for k, job in enumerate(jobs) if job[1] != sizes[k]]
        if resized:
            ctx.resample_lanczos([sources[k].data_ptr() for k in resized], [sizes[k] for k in resized], [sizes[k][0] * 3 for k in resized],
                                 [rendered[k].data_ptr() for k in resized], [jobs[k][1] for k in resized], [jobs[k][1][0] * 3 for k in resized],
                                 stream=ext.cuda_stream)
        with torch.cuda.stream(ext):
            draw_plans(ctx, [t.data_ptr() for t in rendered], [job[1] for job in jobs], [job[2] for job in jobs], device, ext.cuda_stream)
        files = files_of_device_images(ctx, [(t, size[0], size[1], entries[e][3]) for t, (e, size, _, _) in zip(rendered, jobs)],
                                       options.quality, ext)
        for (e, _, _, _), pair in zip(jobs, files):
            out[e] = pair
    for _, leg in out:
        counts[leg] += 1
    return out, counts


def write_preview(preview_folder, relative_name, data):
    """writes one preview below preview_folder; returns the path"""
    return write_file(preview_folder, relative_name, data)


class PreviewProduct(Product):
    """preview=: result['preview'] = (bytes or None, leg); counted in HIPDetector.preview_counts, the images that are not
    rendered (is_rendered) as 'skipped'"""

    key = 'preview'

    def nothing(self):
        return None, 'skipped'

    def selects(self, result):
        if is_rendered(result, self.options):
            return True
        result[self.key] = self.nothing()
        self.counts['skipped'] += 1
        return False

    def _host(self, pixels, name, detections):
        data = preview_file_of_host_image(pixels, name, detections, self.options)
        leg = 'host' if data is not None else 'skipped'
        return (data, leg), leg

    def _device(self, ctx, entries, stream):
        return previews_of_device_images(ctx, entries, self.options, stream=stream)


__all__ = ['HostLeg', 'NO_LABELS', 'PreviewOptions', 'RenderFailure', 'RenderPlan', 'box_edges', 'classified_label_lines',
           'corner_edges', 'drawn_detections', 'is_rendered', 'label_box', 'label_string', 'output_name', 'outline_ops',
           'preview_file_of_host_image', 'previews_of_device_images', 'rectangles_to_blur', 'render_plan', 'render_with_pil',
           'resolve_sizes', 'stacked_labels', 'target_size', 'thin_outline_ops', 'write_preview']
