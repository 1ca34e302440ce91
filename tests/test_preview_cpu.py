"""
Annotated previews, host side: the host models of the GPU calls (mdjpeg_resample, mdjpeg_draw in libmdjpeg.so, compiled from
csrc/resample.h like the kernels) against Pillow's Image.resize(LANCZOS) and ImageDraw, bit for bit; the target sizes, names,
selection and drawing plan of megadetector_amd.preview against the reference's statements (restated here) and against what
the reference itself computed (tests/golden/preview_reference.json); the written file; the driver's options.  The shapes,
scenes and the restated renderer defined here are what tests/test_gpu_preview.py runs on the device.
"""

import hashlib
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageColor, ImageDraw

from conftest import GOLDEN, REPO
from megadetector_amd import jpeg_host as J
from megadetector_amd import preview as P

# (width, height) -> (width, height); the last: the source is a view with pitch 64
RESAMPLE_SHAPES = [((97, 61), (40, 25)), ((333, 500), (166, 249)), ((50, 40), (120, 96)), ((1000, 37), (70, 2)), ((1, 1), (5, 5)),
                   ((640, 480), (640, 479))]
LABEL_MAP = {'1': 'animal', '2': 'person', '3': 'vehicle'}


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pillow_resize(rgb, size):
    return np.asarray(Image.fromarray(np.ascontiguousarray(rgb)).resize(size, Image.LANCZOS))


def pitched(rgb, pitch, fill=0xA5):
    """rgb as a view with `pitch` bytes a row of a larger array filled with a sentinel: (backing array, view)"""
    h, w = rgb.shape[:2]
    backing = np.full((h + 2, pitch), fill, dtype=np.uint8)
    view = backing[1:1 + h, 4:4 + w * 3].reshape(h, w, 3)
    view[...] = rgb
    assert view.strides == (pitch, 3, 1)
    return backing, view


# ---- the reference, restated ------------------------------------------------------------------------------------------------

def reference_target_size(width, height, target_width):
    """visualization_utils.resize_image(image, target_width) :367-417, statement for statement; None where it asserts"""
    target_height = -1
    if target_width is None:
        target_width = -1
    resize_required = True
    if target_width == -1 and target_height == -1:
        resize_required = False
    elif target_width == -1 or target_height == -1:
        aspect_ratio = width / height
        if target_width != -1:
            target_height = int(target_width / aspect_ratio)
        else:
            target_width = int(aspect_ratio * target_height)
    if (target_width == width) and (target_height == height):
        resize_required = False
    if not resize_required:
        return width, height
    if not (target_width > 0 and target_height > 0):
        return None
    return target_width, target_height


def reference_draw_box(image, ymin, xmin, ymax, xmax, clss, thickness, expansion, display_str_list, label_font_size, font):
    """visualization_utils.draw_bounding_box_on_image :978-1137 for left / top aligned, unrotated text, statement for
    statement; `font` stands for _load_font's result, so that a test draws with one font object"""
    colormap = P.PREVIEW_COLORS
    color = colormap[1] if clss is None else colormap[int(clss) % len(colormap)]
    draw = ImageDraw.Draw(image)
    im_width, im_height = image.size
    if 0 < thickness < 1:
        thickness = max(1, round(thickness * im_width))
    if 0 < expansion < 1:
        expansion = round(expansion * im_width)
    if 0 < label_font_size < 1:
        label_font_size = max(1, round(label_font_size * im_width))
    thickness, expansion, label_font_size = int(thickness), int(expansion), int(label_font_size)
    (left, right, top, bottom) = (xmin * im_width, xmax * im_width, ymin * im_height, ymax * im_height)
    if expansion > 0:
        left -= expansion
        right += expansion
        top -= expansion
        bottom += expansion
        left = max(left, 0); right = max(right, 0)                           # noqa: E702
        top = max(top, 0); bottom = max(bottom, 0)                           # noqa: E702
        left = min(left, im_width - 1); right = min(right, im_width - 1)     # noqa: E702
        top = min(top, im_height - 1); bottom = min(bottom, im_height - 1)   # noqa: E702
    draw.rectangle([(left, top), (right, bottom)], outline=color, width=thickness)
    font = font(label_font_size)
    display_str_heights = [font.getbbox(ds)[3] for ds in display_str_list]
    total_display_str_height = (1 + 2 * 0.05) * sum(display_str_heights)
    for i_str, display_str in enumerate(display_str_list[::-1]):
        if len(display_str) == 0:
            continue
        display_str = ' ' + display_str + ' '
        _, _, text_width, text_height = font.getbbox(display_str)
        margin = int(np.ceil(0.05 * text_height))
        text_bottom = top
        if (text_bottom - total_display_str_height) < 0:
            text_bottom = bottom + total_display_str_height
            if text_bottom > im_height:
                text_bottom = top + total_display_str_height
        text_bottom = int(text_bottom) - i_str * (int(text_height + (2 * margin)))
        text_left = int(left)
        draw.rectangle([(text_left, (text_bottom - text_height) - (2 * margin)), (text_left + text_width, text_bottom)], fill=color)
        draw.text((text_left + margin, text_bottom - text_height - margin), display_str, fill='black', font=font)


def reference_render(detections, image, label_map, confidence_threshold, thickness=4, expansion=0, label_font_size=16,
                     label_font='arial.ttf'):
    """visualization_utils.render_detection_bounding_boxes :642-796 without classifications and custom strings, sort order
    'confidence', statement for statement; IN PLACE on a PIL image"""
    if (label_map is not None) and isinstance(label_map, str) and (label_map == 'show_categories'):
        label_map = {}
    display_boxes, display_strs, classes = [], [], []
    detections = sorted(detections, key=lambda d: (d['conf'] is not None, d['conf']), reverse=False)
    for detection in detections:
        score = detection['conf']
        if (score is None) or (score >= confidence_threshold):
            x1, y1, w_box, h_box = detection['bbox']
            display_boxes.append([y1, x1, y1 + h_box, x1 + w_box])
            clss = detection['category']
            if label_map is not None:
                label = label_map[clss] if clss in label_map else clss
                displayed_label = ['{}: {}%'.format(label, round(100 * score))]
            else:
                displayed_label = ['']
            display_strs.append(displayed_label)
            classes.append(clss)
    display_boxes = np.array(display_boxes)
    if len(display_boxes.shape) != 2 or display_boxes.shape[1] != 4:
        return image
    for i in range(display_boxes.shape[0]):
        reference_draw_box(image, display_boxes[i, 0], display_boxes[i, 1], display_boxes[i, 2], display_boxes[i, 3], classes[i],
                           thickness, expansion, display_strs[i], label_font_size, lambda size: P.load_font(label_font, size))
    return image


def reference_preview_pixels(rgb, detections, options, label_map=LABEL_MAP):
    """visualize_detector_output._render_image :115-148 on an array: blur, resize, render; None where resize_image asserts"""
    from test_blur_cpu import reference_blur_detections
    im = Image.fromarray(rgb.copy())
    dets = P.output_order(detections, options.output_threshold)
    ids = [k for k, v in LABEL_MAP.items() if options.blur_categories and v in options.blur_categories]
    to_blur = [d for d in dets if d['conf'] >= options.confidence_threshold and d['category'] in ids]
    if to_blur:
        reference_blur_detections(im, to_blur)
    size = reference_target_size(im.size[0], im.size[1], options.output_image_width)
    if size is None:
        return None
    if size != im.size:
        im = im.resize(size, Image.LANCZOS)
    reference_render(dets, im, label_map, options.confidence_threshold, options.box_thickness, options.box_expansion,
                     options.label_font_size, options.label_font)
    return np.asarray(im)


def planned_pixels(rgb, detections, options, labels=True):
    """the plan of megadetector_amd.preview applied by the host model of the drawing kernel, on a copy of rgb"""
    plan = P.render_plan(detections, rgb.shape[1], rgb.shape[0], options, LABEL_MAP, labels)
    out = rgb.copy()
    assert J.draw_ops(out, plan.ops, bytes(plan.patches)) == J.MDJPEG_OK
    return out, plan


# the 500 x 375 scene: a label above its box, one forced below, one forced inside, one clipped at the right border, two
# overlapping boxes, a box that leaves the image on every side, one below the default threshold
SCENE_SIZE = (500, 375)
SCENE = [{'category': '1', 'conf': 0.93, 'bbox': [0.1, 0.3, 0.2, 0.25]}, {'category': '2', 'conf': 0.5, 'bbox': [0.5, 0.01, 0.2, 0.3]},
         {'category': '3', 'conf': 0.8, 'bbox': [0.02, 0.0, 0.3, 0.99]}, {'category': '1', 'conf': 0.3, 'bbox': [0.9, 0.5, 0.09, 0.2]},
         {'category': '2', 'conf': 0.31, 'bbox': [0.15, 0.35, 0.3, 0.3]}, {'category': '1', 'conf': 0.1, 'bbox': [0.4, 0.4, 0.1, 0.1]}]
OUTSIDE = [{'category': '1', 'conf': 0.6, 'bbox': [-0.1, -0.1, 1.3, 1.3]}, {'category': '2', 'conf': 0.7, 'bbox': [-0.2, 0.3, 0.5, 0.2]},
           {'category': '3', 'conf': 0.8, 'bbox': [0.8, 0.7, 0.5, 0.6]}]
EQUAL = [{'category': '2', 'conf': 0.6, 'bbox': [0.2, 0.2, 0.5, 0.6]}, {'category': '1', 'conf': 0.6, 'bbox': [0.3, 0.1, 0.5, 0.6]},
         {'category': '3', 'conf': 0.6, 'bbox': [0.25, 0.15, 0.5, 0.6]}]
THIN = [{'category': '1', 'conf': 0.9, 'bbox': [0.4, 0.4, 0.005, 0.005]}, {'category': '2', 'conf': 0.5, 'bbox': [0.1, 0.1, 0.3, 0.3]}]
DRAW_CASES = {
    'scene': (SCENE, {}),
    'outside': (OUTSIDE, {}),
    'expansion_10': (SCENE + OUTSIDE, {'box_expansion': 10}),
    'fractions': (SCENE, {'box_thickness': 0.01, 'label_font_size': 0.03, 'box_expansion': 0.004}),
    'threshold': (SCENE, {'confidence_threshold': 0.4}),
    'equal_confidence': (EQUAL, {}),
}


# ---- resampling -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['noise', 'white'])
@pytest.mark.parametrize('src,dst', RESAMPLE_SHAPES)
def test_host_model_equals_pillow_lanczos(src, dst, kind):
    rgb = noise(src[0], src[1], 11) if kind == 'noise' else np.full((src[1], src[0], 3), 255, np.uint8)
    got = J.resample_lanczos(rgb, dst)
    assert got.shape == (dst[1], dst[0], 3)
    assert int((got != pillow_resize(rgb, dst)).sum()) == 0


@pytest.mark.parametrize('kind', ['noise', 'white'])
def test_host_model_with_a_pitch_of_64_touches_nothing_beside_the_rows(kind):
    rgb = noise(17, 9, 12) if kind == 'noise' else np.full((9, 17, 3), 255, np.uint8)
    _, view = pitched(rgb, 64)
    backing, out = pitched(np.zeros((4, 8, 3), np.uint8), 29, fill=0x5A)
    J.resample_lanczos(view, (8, 4), out=out)
    assert int((out != pillow_resize(rgb, (8, 4))).sum()) == 0
    guard = backing.copy()
    guard[1:5, 4:4 + 24] = 0x5A
    assert (guard == 0x5A).all()


def test_target_sizes_follow_resize_image():
    table = [(2048, 1536, 1000), (1920, 1080, 1000), (1000, 750, 1000), (1000, 751, 1000), (333, 500, 166), (3, 7, 1000), (4000, 3, 1000),
             (5000, 2, 1000), (1333, 1001, 1000), (999, 1000, 1000), (640, 480, -1), (640, 480, None), (3001, 17, 1000), (720, 1280, 1000),
             (1000, 3, 1000), (7, 7, 3), (4999, 5, 1000), (5001, 5, 1000), (1366, 768, 1000), (1001, 1000, 1000)]
    for w, h, tw in table:
        assert P.target_size(w, h, tw) == reference_target_size(w, h, tw), (w, h, tw)
    assert P.target_size(1920, 1080, 1000) == (1000, 562)                        # int() truncates 562.5
    assert P.target_size(4000, 3, 1000) is None and P.target_size(1000, 750, 1000) == (1000, 750)


# ---- drawing ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('thickness', [1, 2, 3, 4, 5])
def test_outline_rectangles_equal_pillows_outline(thickness):
    """every box from 2 t to 2 t + 9 pixels wide and high, inside the image and across each of its corners; a thinner box is
    handed to the host leg"""
    W, H = 40, 36
    for bw in range(0, 2 * thickness + 9):
        for bh in range(0, 2 * thickness + 9):
            for x0, y0 in ((10.7, 9.2), (-3.5, -2.0), (W - 5.0, H - 4.5)):
                box = (x0, y0, x0 + bw, y0 + bh)
                try:
                    ops = P.outline_ops(*box, thickness, (255, 0, 0))
                except P.HostLeg:
                    assert int(box[2]) - int(box[0]) + 1 < 2 * thickness or int(box[3]) - int(box[1]) + 1 < 2 * thickness
                    continue
                assert int(box[2]) - int(box[0]) + 1 >= 2 * thickness and int(box[3]) - int(box[1]) + 1 >= 2 * thickness
                ref = Image.new('RGB', (W, H))
                ImageDraw.Draw(ref).rectangle([box[:2], box[2:]], outline='Red', width=thickness)
                got = np.zeros((H, W, 3), np.uint8)
                assert J.draw_ops(got, ops) == J.MDJPEG_OK
                assert np.array_equal(got, np.asarray(ref)), (box, thickness)


@pytest.mark.parametrize('labels', [True, False])
@pytest.mark.parametrize('case', sorted(DRAW_CASES))
def test_the_plan_draws_what_the_reference_draws(case, labels):
    dets, kw = DRAW_CASES[case]
    opt = P.PreviewOptions(**kw)
    base = noise(SCENE_SIZE[0], SCENE_SIZE[1], 21)
    got, plan = planned_pixels(base, dets, opt, labels)
    want = np.asarray(reference_render(dets, Image.fromarray(base.copy()), LABEL_MAP if labels else None, opt.confidence_threshold,
                                       opt.box_thickness, opt.box_expansion, opt.label_font_size, opt.label_font))
    assert int((got != want).any(axis=2).sum()) == 0
    assert not np.array_equal(got, base)
    drawn = [d for d in sorted(dets, key=lambda d: d['conf']) if d['conf'] >= opt.confidence_threshold]
    assert len(plan.labels) == len(drawn) and all((s == '') == (not labels) for s in plan.labels)
    # the host leg draws the same pixels with PIL's own calls
    assert np.array_equal(np.asarray(P.render_with_pil(Image.fromarray(base.copy()), dets, opt, LABEL_MAP, labels)), want)


def test_equal_confidences_keep_the_order_of_the_file():
    plan = P.render_plan(EQUAL, 500, 375, P.PreviewOptions(), LABEL_MAP)
    assert plan.labels == ['person: 60%', 'animal: 60%', 'vehicle: 60%'] and plan.order == [0, 1, 2]
    base = noise(500, 375, 22)
    a, _ = planned_pixels(base, EQUAL, P.PreviewOptions())
    b, _ = planned_pixels(base, EQUAL[::-1], P.PreviewOptions())
    assert not np.array_equal(a, b)                                          # the last one drawn lies on top


def test_a_box_thinner_than_its_outline_goes_to_the_host_leg():
    opt = P.PreviewOptions()
    with pytest.raises(P.HostLeg):
        P.render_plan(THIN, 500, 375, opt, LABEL_MAP)
    base = noise(500, 375, 23)
    want = reference_preview_pixels(base, THIN, P.PreviewOptions(output_image_width=-1))
    data = P.preview_file_of_host_image(base, 'thin.png', THIN, P.PreviewOptions(output_image_width=-1), LABEL_MAP)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), want)


def test_what_the_plan_does_not_restate_goes_to_the_host_leg_or_fails_as_the_reference():
    opt = P.PreviewOptions()
    with pytest.raises(P.HostLeg):
        P.render_plan([{'category': '1', 'conf': None, 'bbox': [0.1, 0.1, 0.5, 0.5]}], 500, 375, opt, LABEL_MAP)
    with pytest.raises(P.HostLeg):
        P.render_plan([{'category': '1', 'conf': 0.9, 'bbox': [0.1, 0.1, 0.5, 0.5], 'classifications': [['3', 0.9]]}], 500, 375, opt, LABEL_MAP)
    reversed_box = [{'category': '1', 'conf': 0.9, 'bbox': [0.5, 0.5, -0.2, 0.2]}]
    with pytest.raises(P.RenderFailure):
        P.render_plan(reversed_box, 500, 375, opt, LABEL_MAP)
    with pytest.raises(ValueError):                                           # Pillow itself refuses it
        reference_render(reversed_box, Image.new('RGB', (500, 375)), LABEL_MAP, 0.15)
    assert P.preview_file_of_host_image(noise(50, 40, 1), 'r.png', reversed_box, P.PreviewOptions(output_image_width=-1)) is None


def test_operations_that_leave_the_image_and_bad_operations():
    img = np.full((20, 30, 3), 7, np.uint8)
    patch = bytes(range(4 * 3 * 3))
    ops = [[0, -5, -5, 2, 2, 0x0000FF, 0, 0], [0, 25, 15, 100, 100, 0x00FF00, 0, 0], [1, 28, 18, 4, 3, 0, 0, 0], [1, -2, -1, 4, 3, 0, 0, 0],
           [0, 10, 10, 9, 12, 0xFFFFFF, 0, 0], [1, 100, 100, 4, 3, 0, 0, 0]]
    assert J.draw_ops(img, ops, patch) == J.MDJPEG_OK
    want = np.full((20, 30, 3), 7, np.uint8)
    want[0:3, 0:3] = (255, 0, 0)
    want[15:, 25:] = (0, 255, 0)
    p = np.frombuffer(patch, np.uint8).reshape(3, 4, 3)
    want[18:20, 28:30] = p[:2, :2]
    want[0:2, 0:2] = p[1:, 2:]
    assert np.array_equal(img, want)
    before = img.copy()
    assert J.draw_ops(img, [[0, 0, 0, 5, 5, 1, 0, 0], [1, 0, 0, 4, 3, 1, 0, 0]], patch) == J.MDJPEG_EINVAL      # a patch past its buffer
    assert J.draw_ops(img, [[2, 0, 0, 5, 5, 1, 0, 0]], patch) == J.MDJPEG_EINVAL
    assert np.array_equal(img, before)


# ---- the reference's own results ---------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def golden():
    return json.load(open(os.path.join(GOLDEN, 'preview_reference.json')))


def _golden_images():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_preview_golden', os.path.join(GOLDEN, 'gen_preview_golden_from_reference.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_golden_target_sizes(golden):
    assert len(golden['target_sizes']) >= 20
    for t in golden['target_sizes']:
        size = P.target_size(t['width'], t['height'], t['target_width'])
        assert (None if size is None else list(size)) == t['size'], t


def test_golden_draw_order_and_labels(golden):
    gen = _golden_images()
    assert len(golden['draw_order']) == 6
    for key, rec in golden['draw_order'].items():
        name, threshold = key.rsplit('@', 1)
        w, h, _, dets = gen.IMAGES[name]
        opt = P.PreviewOptions(confidence_threshold=float(threshold), output_image_width=-1)
        drawn = P.drawn_detections(dets, opt)
        assert [[d['bbox'][1], d['bbox'][0], d['bbox'][1] + d['bbox'][3], d['bbox'][0] + d['bbox'][2]] for d in drawn] == rec['boxes']
        assert [d['category'] for d in drawn] == rec['classes']
        assert [[P.label_string(d, LABEL_MAP)] for d in drawn] == rec['labels']


def test_golden_names_selection_and_label_free_renders(golden):
    """every run of the reference script: the same images get a file, under the same name, with the same pixels -- from the
    host leg (PIL) and from the plan applied by the host models of the two kernels"""
    gen = _golden_images()
    translate = {'render_detections_only': 'detections_only', 'preserve_path_structure': 'preserve_path_structure',
                 'confidence_threshold': 'confidence_threshold', 'output_image_width': 'output_image_width', 'box_thickness': 'box_thickness',
                 'box_expansion': 'box_expansion', 'category_names_to_blur': 'blur_categories'}
    assert len(golden['runs']) == 6
    for key, run in golden['runs'].items():
        opt = P.PreviewOptions(**{translate[k]: v for k, v in run['options'].items()})
        files = {}
        for name, (w, h, seed, dets) in gen.IMAGES.items():
            r = {'file': name, 'detections': dets} if dets is not None else {'file': name, 'failure': 'Failure image access'}
            if not P.is_rendered(r, opt):
                continue
            rgb = gen.seeded_image(w, h, seed)
            out_name = P.output_name(name, opt)
            data = P.preview_file_of_host_image(rgb, out_name, dets, opt, P.NO_LABELS)
            host = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
            files[out_name] = {'size': [host.shape[1], host.shape[0]], 'sha256': hashlib.sha256(host.tobytes()).hexdigest()}
            # the device's way on the host: blur, mdjpeg_resample, the plan through mdjpeg_draw
            copy = rgb.copy()
            rects = P.rectangles_to_blur(dets, w, h, opt)
            if rects:
                assert J.blur_regions(copy, rects, 40) == J.MDJPEG_OK
            size = P.target_size(w, h, opt.output_image_width)
            model = J.resample_lanczos(copy, size) if size != (w, h) else copy
            plan = P.render_plan(dets, size[0], size[1], opt, None, labels=False)
            assert J.draw_ops(model, plan.ops, bytes(plan.patches)) == J.MDJPEG_OK
            assert np.array_equal(model, host), (key, name)
        assert files == run['files'], key


# ---- files and the driver ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['a.jpg', 'sub/b.JPEG', 'c.png'])
def test_the_host_leg_writes_the_file_pillow_saves(name):
    rgb = noise(320, 240, 31)
    dets = [{'category': '2', 'conf': 0.9, 'bbox': [0.1, 0.2, 0.4, 0.6]}, {'category': '1', 'conf': 0.5, 'bbox': [0.0, 0.0, 0.3, 0.3]},
            {'category': '2', 'conf': 0.1, 'bbox': [0.6, 0.0, 0.2, 0.2]}]
    for opt in (P.PreviewOptions(output_image_width=200), P.PreviewOptions(output_image_width=200, blur_categories='person')):
        source = rgb.copy()
        got = P.preview_file_of_host_image(rgb, name, dets, opt, LABEL_MAP)
        np.testing.assert_array_equal(rgb, source)                                  # the caller's pixels are not touched
        bio = io.BytesIO()
        save_kw = {} if name.endswith('.png') else {'quality': 75}
        Image.fromarray(reference_preview_pixels(source, dets, opt)).save(bio, format='PNG' if name.endswith('.png') else 'JPEG', **save_kw)
        assert got == bio.getvalue()
        plain = io.BytesIO()
        Image.fromarray(reference_preview_pixels(source, dets, opt)).save(plain, format='PNG' if name.endswith('.png') else 'JPEG')
        assert got == plain.getvalue()                                              # Image.save(path): quality 75 IS Pillow's default
    assert P.preview_file_of_host_image(noise(4000, 3, 1), name, [], P.PreviewOptions()) is None


def test_options_and_names():
    opt = P.PreviewOptions()
    assert (opt.confidence_threshold, opt.output_image_width, opt.detections_only, opt.preserve_path_structure, opt.box_thickness,
            opt.box_expansion, opt.label_font_size, opt.label_font, opt.box_sort_order, opt.blur_categories, opt.quality) == \
        (0.15, 1000, False, False, 4, 0, 16, 'arial.ttf', 'confidence', None, 75)
    assert P.PreviewOptions(output_image_width=None).output_image_width == -1
    assert P.output_name('a/b\\c:d.jpg', opt) == 'anno_a~b~c~d.jpg'
    assert P.output_name('a/b.jpg', P.PreviewOptions(preserve_path_structure=True)) == 'a/b.jpg'
    with pytest.raises(ValueError):
        P.output_name('/abs/b.jpg', P.PreviewOptions(preserve_path_structure=True))
    for bad in ({'box_thickness': 0}, {'label_font_size': 0}, {'confidence_threshold': 1.5}, {'box_sort_order': 'size'}, {'quality': 0}):
        with pytest.raises(ValueError):
            P.PreviewOptions(**bad)
    assert P.resolve_sizes(P.PreviewOptions(box_thickness=0.01, box_expansion=0.004, label_font_size=0.03), 500) == (5, 2, 15)
    assert P.resolve_sizes(P.PreviewOptions(box_thickness=0.0001), 500) == (1, 0, 16)
    assert [ImageColor.getrgb(P.PREVIEW_COLORS[i]) for i in (1, 2, 3)] == [(255, 0, 0), (65, 105, 225), (255, 215, 0)]
    assert len(P.PREVIEW_COLORS) == 126
    below = {'file': 'x', 'detections': [{'category': '1', 'conf': 0.1, 'bbox': [0, 0, 1, 1]}]}
    assert P.is_rendered(below, opt) and not P.is_rendered(below, P.PreviewOptions(detections_only=True))
    assert not P.is_rendered({'file': 'x', 'failure': 'f'}, opt) and not P.is_rendered({'file': 'x', 'detections': None, 'failure': 'f'}, opt)
    assert P.is_rendered({'file': 'x', 'detections': []}, opt) and not P.is_rendered({'file': 'x', 'detections': []}, P.PreviewOptions(detections_only=True))


def _without_clock(path):
    """the bytes of a results file with the one value that is the time of writing blanked"""
    import re
    text = open(path, 'rb').read()
    assert text.count(b'"detection_completion_time"') == 1
    return re.sub(rb'("detection_completion_time": ")[^"]*(")', rb'\1\2', text)


def _tree(folder):
    return sorted(os.path.relpath(os.path.join(d, f), str(folder)).replace('\\', '/') for d, _, fs in os.walk(str(folder)) for f in fs)


def test_the_driver_writes_a_preview_of_every_image_that_rendered(tmp_path):
    """run_detector_batch's loop with the stub detector (no preview= of its own) over the bundled images: the host leg"""
    from megadetector_amd import run_detector_batch as RDB
    from stub_detector import StubDetector
    img_dir = str(tmp_path / 'bundled')
    shutil.copytree(os.path.join(GOLDEN, 'bundled_images'), img_dir)
    files = RDB.find_images(img_dir, recursive=True)
    assert len(files) >= 6 and any(f.endswith('.png') for f in files)
    failing = files[1]
    plain_json = str(tmp_path / 'plain.json')
    plain = RDB.load_and_run_detector_batch('stub', list(files), quiet=True, detector=StubDetector(), batch_size=4)
    RDB.write_results_to_file(plain, plain_json, relative_path_base=img_dir, detector_file='stub')
    for k, kw in enumerate([{}, {'batch_size': 4}, {'use_image_queue': True, 'batch_size': 2}]):
        out = tmp_path / 'preview{}'.format(k)
        res = RDB.load_and_run_detector_batch('stub', list(files), quiet=True, detector=StubDetector(), preview_folder=str(out),
                                              preview_base=img_dir, preview_width=120, **kw)
        assert all('preview' not in r for r in res)
        res_json = str(tmp_path / 'with{}.json'.format(k))
        RDB.write_results_to_file(res, res_json, relative_path_base=img_dir, detector_file='stub')
        assert _without_clock(res_json) == _without_clock(plain_json)
        rels = [os.path.relpath(f, img_dir).replace('\\', '/') for f in files]
        assert _tree(out) == sorted('anno_' + r.replace('/', '~') for r in rels)
        assert RDB.last_preview_counts == {'files': len(files), 'gpu': 0, 'host': len(files), 'skipped': 0}
        opt = P.PreviewOptions(output_image_width=120, output_threshold=RDB.DEFAULT_OUTPUT_CONFIDENCE_THRESHOLD)
        by_file = {r['file']: r for r in res}
        for f, rel in zip(files, rels):
            want = reference_preview_pixels(np.asarray(RDB.load_image(f)), by_file[f]['detections'], opt)
            bio = io.BytesIO()
            Image.fromarray(want).save(bio, format='PNG' if rel.endswith('.png') else 'JPEG', quality=75)
            assert open(os.path.join(str(out), 'anno_' + rel.replace('/', '~')), 'rb').read() == bio.getvalue(), rel
    # an image that failed and images below the threshold are skipped; the relative paths can be kept
    class Failing(StubDetector):
        def _one(self, img, name):
            if name == failing:
                return {'file': name, 'detections': None, 'failure': 'image access failure'}
            return super()._one(img, name)
    out = tmp_path / 'kept'
    maxes = sorted(max([d['conf'] for d in r['detections']] or [0.0]) for r in plain if r['file'] != failing)
    cut = maxes[len(maxes) // 2]                                             # (of the stub's confidences: half of the images stay below)
    assert maxes[0] < cut <= 1
    res = RDB.load_and_run_detector_batch('stub', list(files), quiet=True, detector=Failing(), preview_folder=str(out), preview_base=img_dir,
                                          preview_width=-1, preview_detections_only=True, preview_confidence_threshold=cut,
                                          preview_preserve_paths=True)
    want = sorted(os.path.relpath(r['file'], img_dir).replace('\\', '/') for r in res
                  if r.get('detections') is not None and max([d['conf'] for d in r['detections']] or [0.0]) >= cut)
    assert 0 < len(want) < len(files) - 1                                     # some rendered, one failed, some below the threshold
    assert _tree(out) == want and os.path.relpath(failing, img_dir).replace('\\', '/') not in want
    assert RDB.last_preview_counts == {'files': len(want), 'gpu': 0, 'host': len(want), 'skipped': len(files) - len(want)}


def test_the_cli_refuses_preview_options_without_a_preview_folder(tmp_path):
    from megadetector_amd import run_detector_batch as RDB
    out = str(tmp_path / 'o.json')
    for extra in (['--preview_width', '500'], ['--preview_confidence_threshold', '0.3'], ['--preview_detections_only'],
                  ['--preview_preserve_paths'], ['--preview_box_thickness', '2'], ['--preview_box_expansion', '3'],
                  ['--preview_label_font_size', '12'], ['--preview_label_font', 'x.ttf'], ['--preview_blur_categories', 'person'],
                  ['--preview_quality', '90']):
        with pytest.raises(AssertionError, match='--preview_folder'):
            RDB.main(['synthetic:YOLOV5N6_TEST:1', str(tmp_path), out] + extra)
    assert not os.path.exists(out)


# ---- the C ABI and the sanitizers --------------------------------------------------------------------------------------------

def test_the_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as G
    G.build()
    from megadetector_amd import _lib
    header = open(os.path.join(REPO, 'include', 'mdhip.h')).read()
    lib = _lib.load()
    for name in ('mdhip_resample_lanczos', 'mdhip_draw_ops'):
        assert 'int {}('.format(name) in header and name in _lib.SYMBOLS and hasattr(lib, name)
    from megadetector_amd.hip_backend import HipContext
    from megadetector_amd.detector import HIPDetector
    assert callable(HipContext.resample_lanczos) and callable(HipContext.draw_ops) and HIPDetector.supports_preview
    jheader = open(os.path.join(REPO, 'include', 'mdjpeg.h')).read()
    for name in ('mdjpeg_resample', 'mdjpeg_draw'):
        assert 'int {}('.format(name) in jheader and name in J.SYMBOLS and hasattr(J.load(), name)


def test_host_models_under_sanitizers(tmp_path):
    """mdjpeg_resample and mdjpeg_draw in a build of image_host.cpp with AddressSanitizer + UBSan (host code; `make asan-jpeg`,
    the --preview mode of host_asan_main.cpp): images of their exact sizes at every alignment, a pitch above 3 x width, operations that leave the
    image -- any access outside an image, and any undefined arithmetic, ends the run"""
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'jpeg_entropy_asan')
    subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), 'asan-jpeg', 'ASAN_OUT=' + exe])
    r = subprocess.run([exe, '--preview'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'preview: 10 shapes x 4 alignments' in r.stdout
