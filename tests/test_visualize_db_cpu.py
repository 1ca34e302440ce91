"""
megadetector_amd.visualize_db against the reference's visualize_db, host side: the selection of the images, the titles, the
pages and the host leg of the rendering, on the scene of tests/visualize_db_scene.py, against
tests/golden/visualize_db_reference.json (written by tests/golden/gen_visualize_db_reference.py from the reference's own run).
The rendering order, the tree and the HTML texts are compared always; the hashes of the rendered files when Pillow is the
recorded version and writes the recorded scene.  Independently of the fixture every rendered file is compared with what direct
Pillow calls write for its image, the device leg's steps are run on the host models of its kernels, and
preview.thin_outline_ops is compared with Pillow pixel by pixel.
"""

import io
import json
import math
import os
from contextlib import redirect_stdout

import numpy as np
import PIL
import pytest
from PIL import Image, ImageDraw

import visualize_db_scene as S
from conftest import REPO
from megadetector_amd import jpeg_host
from megadetector_amd import preview as PV
from megadetector_amd import visualize_db as VD

GOLDEN = json.load(open(os.path.join(REPO, 'tests', 'golden', 'visualize_db_reference.json')))


def run_set(tmp, name, backend='host', extra=None, **kw):
    """-> (what the run wrote (visualize_db_scene.describe_output), counts, options, whether the same bytes are expected, the
    output names in rendering order, what is rendered per image)"""
    tmp = str(tmp)
    attributes = dict(S.OPTION_SETS[name], **(extra or {}))
    image_folder, db_file = S.build(tmp, attributes.get('variant'))
    out = os.path.join(tmp, 'out')
    options = S.apply_options(VD.DbVizOptions(), out, attributes)
    counts, seen = {}, []
    render_images = VD.render_images

    def noted(rendering_info, *args, **kwargs):
        seen[:] = rendering_info
        return render_images(rendering_info, *args, **kwargs)

    VD.render_images = noted
    try:
        with redirect_stdout(io.StringIO()):
            html_file, image_db = VD.visualize_db(db_file, out, image_folder, options, backend=backend, counts=counts, **kw)
    finally:
        VD.render_images = render_images
    assert html_file == os.path.join(out, 'index.html') and len(image_db['annotations']) >= 20
    exact = PIL.__version__ == GOLDEN['pillow'] and S.scene_hash(image_folder) == GOLDEN['scene']
    return S.describe_output(out, tmp), counts, options, exact, [i['output_file_name'] for i in seen], list(seen)


def compare_output(got, want, exact):
    assert got['tree'] == want['tree']
    assert sorted(got['html']) == sorted(want['html'])
    for name, text in want['html'].items():
        assert got['html'][name] == text, '{}: the text differs'.format(name)
    assert sorted(got['sha256']) == sorted(want['sha256'])
    if exact:
        for name, sha in want['sha256'].items():
            assert got['sha256'][name] == sha, '{}: the bytes differ'.format(name)


def rendered_names(want):
    """the files of a set's tree that a run rendered (not the pre-filled ones)"""
    import hashlib
    prefilled = hashlib.sha256(S.PREFILL_BYTES).hexdigest()
    return [rel for rel, sha in want['sha256'].items() if sha != prefilled]


def test_the_scene_and_the_option_sets_cover_what_the_issue_lists():
    assert len(S.OPTION_SETS) >= 15 and sorted(GOLDEN['sets']) == sorted(S.OPTION_SETS) and sorted(GOLDEN['errors']) == sorted(S.ERROR_CASES)
    written = [spec for spec in S.FILES.values() if isinstance(spec, tuple)]
    sizes = [(w, h) for w, h, _ in written]
    assert (64, 48) in sizes and (640, 480) in sizes and (333, 251) in sizes and 10 <= len(S.FILES) <= 14
    assert {how.get('subsampling', 2) for _, _, how in written if how and how.get('mode') != 'L'} == {0, 1, 2}
    assert sum('exif' in how for _, _, how in written) == 1 and sum(how.get('mode') == 'L' for _, _, how in written) == 1
    assert sum('comment' in how for _, _, how in written) == 1 and sum(f.endswith('.png') for f in S.FILES) == 1
    assert S.FILES[S.MISSING] is None and isinstance(S.FILES[S.BROKEN], str)
    by_image = {}
    for a in S.ANNOTATIONS:
        by_image.setdefault(a['image_id'], []).append(a)
    assert any(all('bbox' in a for a in anns) for anns in by_image.values())
    assert any(all('bbox_relative' in a for a in anns) for anns in by_image.values())
    assert any(all('bbox' not in a and 'bbox_relative' not in a for a in anns) for anns in by_image.values())
    assert any(isinstance(a.get('bbox'), float) and math.isnan(a['bbox']) for a in S.ANNOTATIONS)
    assert any('score' in a for a in S.ANNOTATIONS) and not all('score' in a for a in S.ANNOTATIONS)
    assert any(im['id'] not in by_image for im in S.IMAGES)
    assert any(len({a['category_id'] for a in anns}) == 2 for anns in by_image.values())
    assert any({'seq_id', 'frame_num', 'seq_num_frames'} <= set(im) for im in S.IMAGES) and any('flags' in im for im in S.IMAGES)
    assert any('/' in str(im['id']) and ' ' in str(im['id']) and '#' in str(im['id']) for im in S.IMAGES)
    boxes = [a['bbox'] for a in S.ANNOTATIONS if isinstance(a.get('bbox'), list) and a['image_id'] == 'cam1/a444']
    drawn = {(int(x + w) - int(x) + 1, int(y + h) - int(y) + 1) for x, y, w, h in boxes}
    assert {(1, 1), (3, 2), (7, 20)} <= drawn
    assert any(a['bbox'][0] < 0 for a in S.ANNOTATIONS if isinstance(a.get('bbox'), list))
    defaults = GOLDEN['sets']['defaults']
    assert 'rendered_images/cam3~deer~one~1_gt.jpg' in defaults['tree'] and 'rendered_images/broken~_gt.jpg' not in defaults['tree']
    assert 'rendered_images/gone_gt.jpg' not in defaults['tree'] and 'gone_gt.jpg' in defaults['order']
    assert 'broken~_gt.jpg' in defaults['html']['index.html'] and 'Deer, red fox' in defaults['html']['index.html']
    assert len(GOLDEN['sets']['sample_6_seed_3']['order']) == 6 and len(GOLDEN['sets']['sequences_unlimited']['order']) > 3
    assert 'deer, red fox' in GOLDEN['sets']['multiple']['html']['index.html']           # a class filter lowers the names
    pages = GOLDEN['sets']['category_pages']['html']
    assert {'deer.html', 'red_fox.html', 'empty.html', 'bird_small.html', 'no_categories.html', 'index.html'} == set(pages)
    by_count = GOLDEN['sets']['category_pages_by_count']['html']['index.html']
    assert by_count.index('deer.html') < by_count.index('red_fox.html') < by_count.index('empty.html') < by_count.index('bird_small.html')
    assert any('image_00000_00004' in t for t in GOLDEN['sets']['extra_fields']['tree'])
    assert '(q:0.6) (note:small)' in ''.join(GOLDEN['sets']['extra_fields']['html'].values())
    assert all('Sequence s1' in GOLDEN['sets'][n]['html']['index.html'] for n in ('sequences_unlimited', 'sequences_of_2'))
    assert 'Sequence s2' in GOLDEN['sets']['sequences_of_2']['html']['index.html'] and len(GOLDEN['sets']['sequences_of_2']['order']) == 4
    assert GOLDEN['sets']['no_force_rendering']['sha256']['rendered_images/cam1~a444_gt.jpg'] != defaults['sha256']['rendered_images/cam1~a444_gt.jpg']


@pytest.mark.parametrize('name', sorted(S.OPTION_SETS))
def test_host_backend_writes_what_the_reference_writes(tmp_path, name):
    got, counts, options, exact, order, _ = run_set(tmp_path, name, extra={'parallelize_rendering_n_cores': 2})
    want = GOLDEN['sets'][name]
    print('exact bytes compared:', exact, counts)
    compare_output(got, want, exact)
    assert order == want['order']
    rendered = rendered_names(want)
    assert counts['sampled'] == len(want['order']) and counts['rendered'] == counts['host'] == len(rendered) and counts['gpu'] == 0
    assert counts['sampled'] == counts['rendered'] + counts['unopened'] + counts['skipped']
    assert counts['skipped'] == len(S.OPTION_SETS[name].get('prefill', []))
    assert counts['decode_chunks'] == counts['resample_calls'] == counts['draw_calls'] == counts['encode_calls'] == 0


@pytest.mark.parametrize('name', sorted(S.ERROR_CASES))
def test_the_reference_s_assertions_are_raised_with_its_messages(tmp_path, name):
    attributes, variant = S.ERROR_CASES[name]
    image_folder, db_file = S.build(str(tmp_path), variant)
    options = S.apply_options(VD.DbVizOptions(), str(tmp_path / 'out'), attributes)
    want = GOLDEN['errors'][name]
    with pytest.raises(AssertionError) as e, redirect_stdout(io.StringIO()):
        VD.visualize_db(db_file, str(tmp_path / 'out'), image_folder, options, backend='host')
    assert type(e.value).__name__ == want['type'] and str(e.value) == want['message']


def test_what_is_not_restated_raises_before_anything_is_read_or_written(tmp_path):
    out = str(tmp_path / 'out')
    for backend in ('host', 'gpu'):
        with pytest.raises(NotImplementedError):
            VD.visualize_db(str(tmp_path / 'no such file.json'), out, 'https://example.com/images', backend=backend)
        assert not os.path.exists(out)
    options = VD.DbVizOptions()
    options.html_options['urlEncodeFilenames'] = False
    with pytest.raises(NotImplementedError):
        VD.visualize_db({}, out, str(tmp_path), options, backend='host')
    assert not os.path.exists(out)
    with pytest.raises(ValueError, match='backend'):
        VD.visualize_db({}, out, str(tmp_path), backend='cuda')
    with pytest.raises(ValueError, match='Illegal dictionary or filename'), redirect_stdout(io.StringIO()):
        VD.visualize_db(['a list'], out, str(tmp_path), backend='host')


def test_the_options_are_the_reference_s_and_the_command_line_maps_them_as_main_does(tmp_path, monkeypatch):
    o = VD.DbVizOptions()
    assert o.num_to_visualize is None and o.viz_size == (1000, -1) and o.sort_by_filename and o.random_seed == 0 and o.box_thickness == 4
    assert o.parallelize_rendering_n_cores == 12 and o.force_rendering and o.confidence_field_name == 'score' and o.quality is None
    assert o.multiple_categories_tag == '*multiple*' and o.category_page_sort_order == 'alphabetical' and o.max_sequence_length is None
    assert o.html_options['maxFiguresPerHtmlFile'] == math.inf and o.html_options['headerHtml'] == ''
    calls = []
    monkeypatch.setattr(VD, 'visualize_db', lambda *a, **kw: calls.append((a, kw)) or kw['counts'].update(sampled=0))
    with redirect_stdout(io.StringIO()):
        VD.main(['db.json', 'out', 'images', '--num_to_visualize', '7', '--random_sort', '--trim_to_images_with_bboxes', '--random_seed', '5',
                 '--backend', 'host', '--device', '2'])
        VD.main(['db.json', 'out', 'images'])
    (a, kw), (a2, kw2) = calls
    assert a[:3] == ('db.json', 'out', 'images') and (kw['backend'], kw['device']) == ('host', 2)
    assert a[3].num_to_visualize == 7 and a[3].sort_by_filename is False and a[3].trim_to_images_with_bboxes and a[3].random_seed == 5
    assert (kw2['backend'], kw2['device']) == ('gpu', 0) and a2[3].num_to_visualize is None and a2[3].sort_by_filename
    assert a2[3].random_seed is None and not a2[3].trim_to_images_with_bboxes           # (the command line's default seed is None)


def test_a_loaded_database_and_string_options(tmp_path):
    image_folder, db_file = S.build(str(tmp_path))
    options = VD.DbVizOptions()
    options.extra_image_fields_to_print, options.extra_annotation_fields_to_print = 'location', 'note'
    options.parallelize_rendering_with_threads, options.parallelize_rendering = False, False
    db = S.database()
    with redirect_stdout(io.StringIO()) as said:
        html_file, image_db = VD.visualize_db(db, str(tmp_path / 'out'), image_folder, options, backend='host')
    assert image_db is db and options.extra_image_fields_to_print == ['location'] and options.extra_annotation_fields_to_print == ['note']
    assert options.parallelize_rendering_with_threads and 'process-based parallelization is not yet supported' in said.getvalue()
    text = open(html_file).read()
    assert '<h1>Sample annotations</h1>' in text and ', location: ridge' in text and ' (note:small)' in text
    assert db['categories'][0]['name'] == 'Deer'
    options = VD.DbVizOptions()
    options.classes_to_exclude = ['empty']
    with redirect_stdout(io.StringIO()):
        VD.visualize_db(db, str(tmp_path / 'out2'), image_folder, options, backend='host')
    assert db['categories'][0]['name'] == 'deer' and db['images'][4]['file_name'] == 'cam2/grey.jpg'     # as IndexedJsonDb leaves it


# ---- the rendering -----------------------------------------------------------------------------------------------------------------

def _direct_pillow(path, info, viz_size, names, thickness, expansion, colormap, quality, out_path):
    """open_image's steps, resize_image's, render_db_bounding_boxes' and the save, written out with Pillow alone"""
    image = Image.open(path)
    if image.mode in ('RGBA', 'L'):
        image = image.convert('RGB')
    exif = image.getexif() if hasattr(image, 'getexif') else {}
    if exif.get(274) == 6:
        image = image.rotate(270, expand=True)
    original_width, original_height = image.size
    if viz_size is not None and tuple(viz_size) != (-1, -1):
        target_width, target_height = viz_size
        if target_height == -1:
            target_height = int(target_width / (original_width / original_height))
        if target_width <= original_width and (target_width, target_height) != image.size:
            image = image.resize((target_width, target_height), Image.Resampling.LANCZOS)
    width, height = image.size
    font = PV.load_font('arial.ttf', 16)
    colors = PV.PREVIEW_COLORS if colormap is None else colormap
    for box, clss, tag in zip(info['bboxes'], info['box_classes'], info['tags']):
        x, y, w, h = box
        if info['boxes_are_normalized']:
            xmin, xmax, ymin, ymax = x, x + w, y, y + h
        else:
            ymin = y / original_height
            ymax = ymin + h / original_height
            xmin = x / original_width
            xmax = xmin + w / original_width
        left, right, top, bottom = xmin * width, xmax * width, ymin * height, ymax * height
        if expansion > 0:
            left, right, top, bottom = left - expansion, right + expansion, top - expansion, bottom + expansion
            left, right = min(max(left, 0), width - 1), min(max(right, 0), width - 1)
            top, bottom = min(max(top, 0), height - 1), min(max(bottom, 0), height - 1)
        color = colors[clss % len(colors)]
        draw = ImageDraw.Draw(image)
        draw.rectangle([(left, top), (right, bottom)], outline=color, width=thickness)
        label = str(names.get(clss, clss)) + (' ' + tag if tag else '')
        # (where the label goes is preview.stacked_labels, pinned against the reference by tests/test_preview_cpu.py)
        for padded, _, corner0, corner1, text_at in PV.stacked_labels(font, [label], left, top, bottom, height):
            draw.rectangle([corner0, corner1], fill=color)
            draw.text(text_at, padded, fill='black', font=font)
    if quality is None:
        image.save(out_path)
    else:
        image.save(out_path, quality=quality)


RENDERING_SETS = ['defaults', 'size_400_300', 'size_110', 'confidence_threshold', 'quality_colormap', 'custom_mapping', 'include']


@pytest.mark.parametrize('name', RENDERING_SETS)
def test_every_rendered_file_is_what_direct_pillow_calls_write(tmp_path, name):
    got, counts, options, _, _, infos = run_set(tmp_path / 'run', name)
    names = {c['id']: c['name'].lower() if name == 'include' else c['name'] for c in S.CATEGORIES}
    if options.custom_category_mapping is not None:
        names = options.custom_category_mapping
    checked = 0
    for info in infos:
        written = os.path.join(str(tmp_path / 'run'), 'out', 'rendered_images', info['output_file_name'])
        if not os.path.isfile(written):
            continue
        direct = str(tmp_path / 'direct.jpg')
        _direct_pillow(info['img_path'], info, options.viz_size, names, options.box_thickness, options.box_expansion, options.colormap,
                       options.quality, direct)
        assert open(written, 'rb').read() == open(direct, 'rb').read(), info['output_file_name']
        checked += 1
    assert checked == counts['rendered'] >= 3
    if name == 'defaults':
        com = open(os.path.join(str(tmp_path / 'run'), 'out', 'rendered_images', 'com~1_gt.jpg'), 'rb').read()
        assert S.FILES[S.COM][2]['comment'] in com                          # Pillow carries the source's COM segment into the save


@pytest.mark.parametrize('name', RENDERING_SETS)
def test_the_device_leg_s_steps_on_the_host_models_give_the_host_leg_s_pixels(tmp_path, name):
    """decode (PIL here: the decoder's own tests pin it), mdjpeg_resample, the plan through mdjpeg_draw: the pixels the host
    leg hands to its encoder, for every image the device leg plans -- the thin boxes among them"""
    from megadetector_amd.feed import load_image
    got, counts, options, _, _, infos = run_set(tmp_path / 'run', name)
    label_map = {c['id']: c['name'].lower() if name == 'include' else c['name'] for c in S.CATEGORIES}
    planned, thin, resized = 0, 0, 0
    for info in infos:
        if not os.path.isfile(info['img_path']):
            continue
        try:
            job = VD.plan_job(info, options, label_map)
        except Exception:
            assert info['img_path'].endswith(('pic.png', 'broken.jpg')), info['img_path']
            continue
        pixels = np.array(load_image(info['img_path']), dtype=np.uint8, order='C')
        assert (pixels.shape[1], pixels.shape[0]) == job['source_size']
        if job['size'] != job['source_size']:
            pixels = jpeg_host.resample_lanczos(pixels, job['size'])
            resized += 1
        assert jpeg_host.draw_ops(pixels, job['plan'].ops, bytes(job['plan'].patches)) == jpeg_host.MDJPEG_OK
        try:
            VD.plan_job(info, options, label_map, thin_outlines=False)
        except PV.HostLeg:
            thin += 1
        # the host leg, up to its save
        from megadetector_amd.postprocess_batch_results import open_image
        image = open_image(info['img_path'])
        original_size = image.size
        size, resize = VD.viz_target(original_size, options.viz_size)
        if resize:
            image = image.resize(size, Image.Resampling.LANCZOS)
        VD.render_db_with_pil(image, info, original_size, options, label_map)
        assert np.array_equal(pixels, np.asarray(image)), info['output_file_name']
        assert job['comment'] == (S.FILES[S.COM][2]['comment'] if info['img_path'].endswith('com.jpg') else None)
        planned += 1
    assert planned == counts['rendered'] - ('pic_gt.jpg' in [i['output_file_name'] for i in infos])
    assert thin >= 1 or options.box_expansion == 3                        # (an expanded box is at least 7 pixels: not thin at 2)
    assert (resized == 0) == (name in S.UNRESIZED_SETS)


def _pillow_outline(width, height, box, thickness, rgb):
    image = Image.new('RGB', (width, height), (1, 2, 3))
    ImageDraw.Draw(image).rectangle([(box[0], box[1]), (box[2], box[3])], outline=rgb, width=thickness)
    return np.asarray(image)


@pytest.mark.parametrize('thickness', range(1, 9))
def test_thin_outlines_are_pillow_s_pixel_for_pixel(thickness):
    """every box of 1 .. 2t x 1 .. 2t + 3 pixels (and turned), at four offsets, two of them across the image's edge"""
    t = thickness
    width, height, rgb = 40, 36, (250, 128, 114)
    offsets = [(11.0, 9.0), (3.7, 20.2), (-2.0, 5.5), (width - 3.5, height - 2.25)]
    checked = 0
    for w in range(1, 2 * t + 1):
        for h in range(1, 2 * t + 4):
            for bw, bh in {(w, h), (h, w)}:
                for x, y in offsets:
                    box = (x, y, x + bw - 1, y + bh - 1)
                    assert int(box[2]) - int(box[0]) + 1 == bw and int(box[3]) - int(box[1]) + 1 == bh
                    want = _pillow_outline(width, height, box, t, rgb)
                    ops = PV.thin_outline_ops(*box, t, rgb)
                    assert all(op[0] == PV.OP_RECT for op in ops)
                    got = np.empty((height, width, 3), np.uint8)
                    got[:] = (1, 2, 3)
                    assert jpeg_host.draw_ops(got, ops) == jpeg_host.MDJPEG_OK
                    assert np.array_equal(got, want), (t, bw, bh, x, y)
                    if bw < 2 * t or bh < 2 * t:
                        assert PV.box_outline_ops(*box, t, rgb, thin_outlines=True) == ops
                        for call in (PV.outline_ops, PV.box_outline_ops):                 # with their defaults: the host leg's
                            with pytest.raises(PV.HostLeg):
                                call(*box, t, rgb)
                    else:
                        assert PV.box_outline_ops(*box, t, rgb, thin_outlines=True) == PV.outline_ops(*box, t, rgb)
                    checked += 1
    assert checked >= 4 * 2 * t * (2 * t + 3)


def test_thin_outlines_only_where_they_are_asked_for():
    import inspect
    options = PV.PreviewOptions(confidence_threshold=0.1)
    dets = [{'category': '1', 'conf': 0.9, 'bbox': [0.5, 0.5, 0.004, 0.003]}, {'category': '2', 'conf': 0.8, 'bbox': [0.1, 0.1, 0.5, 0.5]}]
    with pytest.raises(PV.HostLeg):
        PV.render_plan(dets, 640, 480, options)
    parameter = inspect.signature(PV.render_plan).parameters['thin_outlines']
    assert parameter.default is False and parameter.kind is inspect.Parameter.KEYWORD_ONLY
    plan = PV.render_plan(dets, 640, 480, options, thin_outlines=True)
    whole = PV.render_plan(dets[1:], 640, 480, options)
    assert PV.render_plan(dets[1:], 640, 480, options, thin_outlines=True).ops == whole.ops     # a box that is not thin: the four bars
    image = Image.new('RGB', (640, 480), (9, 9, 9))
    PV.render_with_pil(image, dets, options)
    got = np.empty((480, 640, 3), np.uint8)
    got[:] = 9
    assert jpeg_host.draw_ops(got, plan.ops, bytes(plan.patches)) == jpeg_host.MDJPEG_OK
    assert np.array_equal(got, np.asarray(image))
    # a box that is not thin is the four bars either way; reversed corners are the reference's failure either way
    assert PV.box_outline_ops(10, 10, 30, 30, 4, (1, 2, 3), thin_outlines=True) == PV.outline_ops(10, 10, 30, 30, 4, (1, 2, 3))
    with pytest.raises(PV.RenderFailure):
        PV.box_outline_ops(10, 10, 5, 30, 4, (1, 2, 3), thin_outlines=True)
