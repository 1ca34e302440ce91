"""
megadetector_amd.postprocess_batch_results against the reference's process_batch_results, host side: the sample, the result
sets, the decision per image, the HTML and the host leg of the rendering, on the scene of tests/postprocess_scene.py, against
tests/golden/postprocess_reference.json (written by tests/golden/gen_postprocess_reference.py from the reference's own run).
The sample, the tree and the HTML texts are compared always; the hashes of the rendered files when Pillow is the recorded
version and writes the recorded scene.  Independently of the fixture every rendered file is compared with what direct Pillow
calls write for its image.
"""

import io
import json
import os
from contextlib import redirect_stdout

import PIL
import pytest
from PIL import Image, ImageDraw

import postprocess_scene as S
from conftest import REPO
from megadetector_amd import postprocess_batch_results as PB
from megadetector_amd import preview as PV

GOLDEN = json.load(open(os.path.join(REPO, 'tests', 'golden', 'postprocess_reference.json')))


def run_set(tmp, name, backend='host', extra=None, **kw):
    """-> (what the run wrote (postprocess_scene.describe_output), counts, options, whether the same bytes are expected)"""
    tmp = str(tmp)
    image_folder, results_file = S.build(tmp)
    out = os.path.join(tmp, 'out')
    options = S.apply_options(PB.PostProcessingOptions(), image_folder, results_file, out, dict(S.OPTION_SETS[name], **(extra or {})))
    with redirect_stdout(io.StringIO()):
        ppresults = PB.process_batch_results(options, backend=backend, **kw)
    assert ppresults.output_html_file == os.path.join(out, 'index.html')
    exact = PIL.__version__ == GOLDEN['pillow'] and S.scene_hash(image_folder) == GOLDEN['scene']
    return S.describe_output(out, tmp), ppresults.counts, options, exact


def compare_output(got, want, exact):
    assert got['tree'] == want['tree']
    assert sorted(got['html']) == sorted(want['html'])
    for name, text in want['html'].items():
        assert got['html'][name] == text, '{}: the text differs'.format(name)
    assert sorted(got['sha256']) == sorted(want['sha256'])
    if exact:
        for name, sha in want['sha256'].items():
            assert got['sha256'][name] == sha, '{}: the bytes differ'.format(name)


def test_the_scene_and_the_option_sets_cover_what_the_issue_lists():
    assert len(S.OPTION_SETS) >= 14 and sorted(GOLDEN['sets']) == sorted(S.OPTION_SETS)
    sizes = [(w, h) for _, w, h, _, _, _ in S.IMAGES]
    assert (61, 97) in sizes and (333, 250) in sizes and all(w <= 333 and h <= 250 for w, h in sizes) and len(sizes) >= 14
    assert {how.get('subsampling', 2) for _, _, _, how, _, _ in S.IMAGES if how.get('mode') != 'L' and how} == {0, 1, 2}
    assert sum(1 for im in S.IMAGES if im[3].get('mode') == 'L') == 1 and sum(1 for im in S.IMAGES if 'exif' in im[3]) == 1
    assert sum(1 for im in S.IMAGES if im[0].endswith('.png')) == 1 and sum(1 for im in S.IMAGES if im[4] is None) == 1
    assert any(' ' in im[0] and '#' in im[0] for im in S.IMAGES) and any(im[0].count('/') == 2 for im in S.IMAGES)
    classified = [im for im in S.IMAGES if im[4] and any('classifications' in d for d in im[4])]
    confs = [d['classifications'][0][1] for im in classified for d in im[4] if 'classifications' in d]
    assert len(classified) == 4 and min(confs) < 0.5 < max(confs) and 0.5 in confs
    defaults = GOLDEN['sets']['defaults']
    assert {'detections_animal', 'detections_person', 'detections_vehicle', 'detections_animal_person', 'detections_animal_person_vehicle',
            'non_detections'} == {t.split('/')[0] for t in defaults['tree'] if '/' in t}
    assert 'detections_animal/detections_animal_sub~deer one1.jpg' in defaults['tree']           # flatten_path drops the '#'
    assert not any('gone' in t for t in defaults['tree']) and 'sub/gone.jpg' in defaults['sampled']      # listed, no file
    assert {'class_deer.html', 'class_cow.html', 'class_unreliable.html', 'class_bear.html'} <= set(defaults['html'])
    assert 'almost_detections.html' in GOLDEN['sets']['almost_default']['html']
    assert any('image_00000_00002' in t for t in GOLDEN['sets']['pages_of_3']['tree'])
    assert not any(t.startswith('non_detections/n') for t in GOLDEN['sets']['bypass_non_detections']['tree'])
    assert '<b>seq_num</b>: 3.0' in GOLDEN['sets']['fields_list']['html']['detections_animal.html']       # a column with holes is one of floats
    assert 'href' not in GOLDEN['sets']['width_120']['html']['detections_animal.html'].split('<img')[0]
    assert len(GOLDEN['sets']['sample_6_seed_0']['sampled']) == 6 != GOLDEN['sets']['sample_6_seed_7']['sampled']


@pytest.mark.parametrize('name', sorted(S.OPTION_SETS))
def test_host_backend_writes_what_the_reference_writes(tmp_path, name):
    got, counts, options, exact = run_set(tmp_path, name, extra={'parallelize_rendering_n_cores': 2})
    want = GOLDEN['sets'][name]
    print('exact bytes compared:', exact, counts)
    compare_output(got, want, exact)
    with redirect_stdout(io.StringIO()):
        d = PB.decide_sample(options)
    assert [x['file'] for x in d['decisions']] == want['sampled']
    rendered = [t for t in want['sha256']]
    assert counts['sampled'] == len(want['sampled']) and counts['rendered'] == counts['host'] == len(rendered) and counts['gpu'] == 0
    assert counts['sampled'] == counts['rendered'] + counts['unopened'] + counts['bypassed']
    assert counts['unopened'] == sum(1 for f in want['sampled'] if 'gone' in f or 'lost' in f)
    assert counts['decode_chunks'] == counts['resample_calls'] == counts['draw_calls'] == counts['encode_calls'] == 0


def _direct_pillow(path, detections, target_width, thresholds, label_map, classification_label_map, thickness, expansion, out_path):
    """open_image's steps, resize, ImageDraw and save, written out with Pillow alone for the scene's images"""
    image = Image.open(path)
    if image.mode in ('RGBA', 'L'):
        image = image.convert('RGB')
    exif = image.getexif() if hasattr(image, 'getexif') else {}
    if exif.get(274) == 6:
        image = image.rotate(270, expand=True)
    if target_width is not None:
        size = (target_width, int(target_width / (image.size[0] / image.size[1])))
        if size != image.size:
            image = image.resize(size, Image.Resampling.LANCZOS)
    width, height = image.size
    font = PV.load_font('arial.ttf', 16)
    drawn = [d for d in sorted(detections, key=lambda d: d['conf']) if d['conf'] >= thresholds[d['category']]]
    for d in drawn:
        strings = ['{}: {}%'.format(label_map[d['category']], round(100 * d['conf']))]
        clss = int(d['category'])
        if d.get('classifications'):
            best, best_conf = 0, -100
            for key, conf in d['classifications'][:3]:
                if conf < 0.5:
                    continue
                if conf > best_conf:
                    best, best_conf = int(key), conf
                strings.append('{}: {}%'.format(classification_label_map[key].lower(), round(100.0 * conf, 1)))
            clss = 3 + best
        color = PV.PREVIEW_COLORS[clss % len(PV.PREVIEW_COLORS)]
        x, y, w, h = d['bbox']
        left, right, top, bottom = x * width, (x + w) * width, y * height, (y + h) * height
        if expansion > 0:
            left, right, top, bottom = left - expansion, right + expansion, top - expansion, bottom + expansion
            left, right = min(max(left, 0), width - 1), min(max(right, 0), width - 1)
            top, bottom = min(max(top, 0), height - 1), min(max(bottom, 0), height - 1)
        draw = ImageDraw.Draw(image)
        draw.rectangle([(left, top), (right, bottom)], outline=color, width=thickness)
        # (where the label lines go is preview.stacked_labels, pinned against the reference by tests/test_preview_cpu.py)
        for padded, _, corner0, corner1, text_at in PV.stacked_labels(font, strings, left, top, bottom, height):
            draw.rectangle([corner0, corner1], fill=color)
            draw.text(text_at, padded, fill='black', font=font)
    image.save(out_path)


@pytest.mark.parametrize('name', ['defaults', 'dict_threshold', 'fields_dict', 'width_120', 'width_400', 'width_none'])
def test_every_rendered_file_is_what_direct_pillow_calls_write(tmp_path, name):
    got, counts, options, _ = run_set(tmp_path / 'run', name)
    with redirect_stdout(io.StringIO()):
        d = PB.decide_sample(options)
    checked = 0
    for decision in d['decisions']:
        rel = '{}/{}'.format(decision['category_string'], PB.sample_name_of(decision))
        source = os.path.join(options.image_base_dir, decision['file'])
        if not os.path.isfile(source):
            assert rel not in got['tree']
            continue
        thresholds = {k: PB.get_threshold_for_category_id(k, options, d['detection_categories']) for k in S.DETECTION_CATEGORIES}
        direct = str(tmp_path / ('direct' + os.path.splitext(rel)[1]))
        _direct_pillow(source, decision['detections'], options.viz_target_width, thresholds, S.DETECTION_CATEGORIES,
                       S.CLASSIFICATION_CATEGORIES, options.line_thickness, options.box_expansion, direct)
        with open(direct, 'rb') as f, open(os.path.join(options.output_dir, rel), 'rb') as g:
            assert f.read() == g.read(), rel
        checked += 1
    assert checked == counts['rendered'] == len(S.IMAGES) - 1


@pytest.mark.parametrize('name', ['width_120', 'width_400', 'defaults', 'dict_threshold'])
def test_the_device_legs_steps_on_the_host_models_give_the_host_legs_pixels(tmp_path, name):
    """The device's way without a device, at this tool's shapes -- reducing and enlarging, odd sizes, classification labels,
    per-category thresholds: Pillow's decode, the host model of the resample kernel and the plan through the host model of
    the drawing kernel must give the pixels the host leg draws (the encoder is pinned by the crops' tests)."""
    import numpy as np
    from megadetector_amd import jpeg_host as J
    image_folder, results_file = S.build(str(tmp_path))
    options = S.apply_options(PB.PostProcessingOptions(), image_folder, results_file, str(tmp_path / 'out'), S.OPTION_SETS[name])
    with redirect_stdout(io.StringIO()):
        d = PB.decide_sample(options)
    checked = enlarged = reduced = 0
    for decision in d['decisions']:
        source = os.path.join(image_folder, decision['file'])
        if not os.path.isfile(source) or decision['file'].endswith('.png'):
            continue
        job = PB._plan_job(decision, d['detection_categories'], d['classification_categories'], options)      # (no HostLeg in the scene)
        image = PB.open_image(source)
        assert job['source_size'] == image.size
        pixels = np.ascontiguousarray(np.asarray(image))
        model = J.resample_lanczos(pixels, job['size']) if job['size'] != job['source_size'] else pixels.copy()
        assert J.draw_ops(model, job['plan'].ops, bytes(job['plan'].patches)) == J.MDJPEG_OK
        host = image.resize(job['size'], Image.Resampling.LANCZOS) if job['size'] != job['source_size'] else image
        o, kw = PB.draw_arguments(decision, d['detection_categories'], d['classification_categories'])
        PV.render_with_pil(host, decision['detections'], o, **kw)
        assert np.array_equal(model, np.asarray(host)), decision['file']
        checked += 1
        enlarged += job['size'][0] > job['source_size'][0]
        reduced += job['size'][0] < job['source_size'][0]
    assert checked == len(S.IMAGES) - 2
    target = options.viz_target_width
    widths = [h if 'exif' in how else w for f, w, h, how, dets, _ in S.IMAGES if dets is not None and not f.endswith('.png')]
    assert (enlarged, reduced) == (sum(w < target for w in widths), sum(w > target for w in widths))
    assert enlarged >= 5 and (reduced >= 5 or name != 'width_120')


def test_the_sample_is_the_one_dataframe_sample_takes():
    # DataFrame.sample(n, random_state=seed) is RandomState(seed).choice(N, n, replace=False); pinned for N = 16 as recorded
    for name in ('sample_6_seed_0', 'sample_6_seed_7'):
        seed = S.OPTION_SETS[name]['sample_seed']
        rows = [im['file'].replace('\\', '/') for im in S.results()['images'] if 'failure' not in im]
        assert [rows[i] for i in PB.sample_indices(len(rows), 6, seed)] == GOLDEN['sets'][name]['sampled']
    assert PB.sample_indices(5, None, 0) == PB.sample_indices(5, -1, 0) == PB.sample_indices(5, 0, 0) == [0, 1, 2, 3, 4]
    assert sorted(PB.sample_indices(5, 9, 0)) == [0, 1, 2, 3, 4]
    unseeded = PB.sample_indices(16, 6, None)
    assert len(unseeded) == len(set(unseeded)) == 6 and all(0 <= i < 16 for i in unseeded)


def test_sample_seed_none_returns_n_distinct_images(tmp_path):
    got, counts, _, _ = run_set(tmp_path, 'sample_6_seed_0', extra={'sample_seed': None, 'rendering_bypass_sets': [
        'non_detections', 'detections_animal', 'detections_person', 'detections_vehicle', 'detections_animal_person',
        'detections_animal_person_vehicle']})
    assert counts['sampled'] == 6 and counts['bypassed'] == 6
    listed = [line for name, text in got['html'].items() if not name.startswith(('index', 'class_')) for line in text.split('\n')
              if '<img src=' in line]
    assert len(listed) == len(set(listed)) == 6


def test_the_random_order_is_a_permutation_of_the_entries(tmp_path):
    by_name, _, _, _ = run_set(tmp_path / 'a', 'defaults')
    shuffled, _, _, _ = run_set(tmp_path / 'b', 'defaults', extra={'html_sort_order': 'random'})
    assert shuffled['tree'] == by_name['tree'] and shuffled['html']['index.html'] == by_name['html']['index.html']
    for name, text in by_name['html'].items():
        entries = lambda t: sorted(t.replace('</body></html>\n', '').replace('<br/>', '').split('<p style'))
        assert entries(shuffled['html'][name]) == entries(text), name
    with pytest.raises(AssertionError, match='Unrecognized sort order'):
        run_set(tmp_path / 'c', 'defaults', extra={'html_sort_order': 'size'})


@pytest.mark.parametrize('attributes', [{'ground_truth_json_file': 'gt.json'}, {'image_base_dir': 'https://example.com/images'},
                                        {'api_detection_results': object(), 'api_other_fields': {}}])
def test_what_is_not_restated_raises_before_the_output_folder_exists(tmp_path, attributes):
    image_folder, results_file = S.build(str(tmp_path))
    out = str(tmp_path / 'out')
    options = S.apply_options(PB.PostProcessingOptions(), image_folder, results_file, out, attributes)
    for backend in ('host', 'gpu'):
        with pytest.raises(NotImplementedError):
            PB.process_batch_results(options, backend=backend)
        assert not os.path.exists(out)
    with pytest.raises(ValueError, match='backend'):
        PB.process_batch_results(S.apply_options(PB.PostProcessingOptions(), image_folder, results_file, out, {}), backend='cuda')


def test_a_dict_threshold_with_almost_detections_needs_their_threshold(tmp_path):
    image_folder, results_file = S.build(str(tmp_path))
    options = S.apply_options(PB.PostProcessingOptions(), image_folder, results_file, str(tmp_path / 'out'),
                              {'confidence_threshold': {'default': 0.5}, 'include_almost_detections': True})
    with pytest.raises(AssertionError, match='you need to supply a threshold for almost detections'):
        with redirect_stdout(io.StringIO()):
            PB.process_batch_results(options, backend='host')
    o = PB.PostProcessingOptions()
    o.confidence_threshold, o.include_almost_detections = 0.03, True
    with redirect_stdout(io.StringIO()):
        PB.resolve_thresholds(o, S.results())
    assert o.almost_detection_confidence_threshold == 0                                   # floored
    o = PB.PostProcessingOptions()
    with redirect_stdout(io.StringIO()):
        PB.resolve_thresholds(o, S.results())
    assert o.confidence_threshold == 0.2 and o.almost_detection_confidence_threshold is None      # MDv5's typical threshold
    o.confidence_threshold = {'animal': 0.3}
    assert PB.get_threshold_for_category_id('1', o, S.DETECTION_CATEGORIES) == 0.3
    with pytest.raises(AssertionError, match='no default supplied'):
        PB.get_threshold_for_category_id('2', o, S.DETECTION_CATEGORIES)
    with pytest.raises(AssertionError, match='Invalid category ID'):
        PB.get_threshold_for_category_id('9', o, S.DETECTION_CATEGORIES)


def test_loading_reads_a_missing_field_as_a_dataframe_does(tmp_path):
    _, results_file = S.build(str(tmp_path))
    with redirect_stdout(io.StringIO()):
        rows, other = PB.load_api_results(results_file, {'gone': 'lost'})
    by_file = {r['file']: r for r in rows}
    assert 'sub/nested/fox.jpg' in by_file and 'sub/lost.jpg' in by_file and 'images' not in other
    assert all(set(r) == set(rows[0]) for r in rows)
    assert by_file['a444.jpg']['seq_num'] == 3.0 and isinstance(by_file['a444.jpg']['seq_num'], float)
    assert PB.is_missing(by_file['a422.jpg']['seq_num']) and PB.is_missing(by_file['a420.jpg']['location'])
    assert by_file['grey.jpg']['location'] == 'ridge' and by_file['all3.jpg']['max_detection_conf'] == 0.95
    assert by_file['blank.jpg']['max_detection_conf'] == 0.0 and not PB.is_missing(by_file['failed.jpg']['failure'])
    assert PB.flatten_path('sub/deer one#1.jpg') == 'sub~deer one1.jpg' and PB.flatten_path('a\\b:c/d e .jpg') == 'a~b~c~d e .jpg'
    assert PB.clean_filename('class_red fox', replace_whitespace='_') == 'class_red_fox'


def test_the_command_line_maps_its_arguments_as_main_does(tmp_path):
    o, backend, device = PB.options_from_arguments(['r.json', 'out'])
    assert (o.md_results_file, o.output_dir, backend, device) == ('r.json', 'out', 'gpu', 0)
    assert o.parallelize_rendering and o.parallelize_rendering_n_cores == 4 and o.parallelize_rendering_with_threads
    assert o.max_figures_per_html_file is None and o.confidence_threshold is None and o.num_images_to_sample == 1000
    assert o.viz_target_width == 1200 and o.html_sort_order == 'filename' and o.separate_detections_by_category
    o, backend, device = PB.options_from_arguments(
        ['r.json', 'out', '--image_base_dir', 'images', '--confidence_threshold', '0.3', '--almost_detection_confidence_threshold', '0.2',
         '--include_almost_detections', '--num_images_to_sample', '-1', '--viz_target_width', '800', '--sort_by_confidence',
         '--n_cores', '6', '--parallelize_rendering_with_processes', '--no_separate_detections_by_category', '--open_output_file',
         '--max_figures_per_html_file', '50', '--html_sort_order', 'random', '--backend', 'host', '--device', '2'])
    assert (backend, device) == ('host', 2) and o.image_base_dir == 'images' and o.confidence_threshold == 0.3
    assert o.almost_detection_confidence_threshold == 0.2 and o.include_almost_detections and o.num_images_to_sample == -1
    assert o.viz_target_width == 800 and o.parallelize_rendering_n_cores == 6 and not o.parallelize_rendering_with_threads
    assert not o.separate_detections_by_category and o.open_output_file and o.max_figures_per_html_file == 50
    assert o.sort_by_confidence and o.html_sort_order == 'random'          # the reference reads --sort_by_confidence nowhere
    assert not hasattr(o, 'backend') and not hasattr(o, 'device')
    o, _, _ = PB.options_from_arguments(['r.json', 'out', '--n_cores', '1'])
    assert o.parallelize_rendering and o.parallelize_rendering_n_cores == 8           # as there: one core changes nothing
    with pytest.raises(AssertionError, match='Illegal number of cores'):
        PB.options_from_arguments(['r.json', 'out', '--n_cores', '0'])
    # and it runs: the same bytes as the call
    image_folder, results_file = S.build(str(tmp_path))
    out = str(tmp_path / 'out')
    with redirect_stdout(io.StringIO()) as printed:
        assert PB.main([results_file, out, '--image_base_dir', image_folder, '--num_images_to_sample', '-1', '--max_figures_per_html_file',
                        '1000', '--n_cores', '2', '--open_output_file', '--backend', 'host']) == 0
    assert '--open_output_file is ignored' in printed.getvalue()
    compare_output(S.describe_output(out, str(tmp_path)), GOLDEN['sets']['defaults'],
                   PIL.__version__ == GOLDEN['pillow'] and S.scene_hash(image_folder) == GOLDEN['scene'])


def _preview_generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_preview_golden', os.path.join(REPO, 'tests', 'golden', 'gen_preview_golden_from_reference.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_preview_plans_are_unchanged_without_the_category_thresholds():
    """the inputs of tests/golden/preview_reference.json (tests/test_preview_cpu.py pins what they give): the argument is the
    last one and optional, and a dict that names the options' own threshold for every category plans the very same ops"""
    import inspect
    golden = json.load(open(os.path.join(REPO, 'tests', 'golden', 'preview_reference.json')))
    gen = _preview_generator()
    for fn in (PV.drawn_detections, PV.render_plan, PV.render_with_pil):
        parameters = list(inspect.signature(fn).parameters.values())
        assert parameters[-1].name == 'category_thresholds' and parameters[-1].default is None
    translate = {'render_detections_only': 'detections_only', 'preserve_path_structure': 'preserve_path_structure',
                 'confidence_threshold': 'confidence_threshold', 'output_image_width': 'output_image_width', 'box_thickness': 'box_thickness',
                 'box_expansion': 'box_expansion', 'category_names_to_blur': 'blur_categories'}
    checked = 0
    for key, run in golden['runs'].items():
        o = PV.PreviewOptions(**{translate[k]: v for k, v in run['options'].items()})
        for name, (w, h, _, dets) in gen.IMAGES.items():
            if dets is None:
                continue
            size = PV.target_size(w, h, o.output_image_width)
            uniform = {d['category']: o.confidence_threshold for d in dets}
            assert PV.drawn_detections(dets, o) == PV.drawn_detections(dets, o, None) == PV.drawn_detections(dets, o, uniform)
            for labels in (True, False):
                try:
                    plan = PV.render_plan(dets, size[0], size[1], o, None, labels)
                except (PV.HostLeg, PV.RenderFailure) as e:
                    with pytest.raises(type(e)):
                        PV.render_plan(dets, size[0], size[1], o, None, labels, category_thresholds=uniform)
                    continue
                same = PV.render_plan(dets, size[0], size[1], o, None, labels, category_thresholds=uniform)
                assert plan.ops == same.ops and bytes(plan.patches) == bytes(same.patches)
                assert plan.labels == same.labels and plan.order == same.order
                checked += 1
    assert checked >= 20
    with pytest.raises(ValueError):
        PV.PreviewOptions(confidence_threshold=1.5)
    with pytest.raises(TypeError):
        PV.PreviewOptions(confidence_threshold={'1': 0.5})                 # still a number, as before
    dets = [{'category': '1', 'conf': 0.5, 'bbox': [0.1, 0.1, 0.5, 0.5]}, {'category': '2', 'conf': 0.5, 'bbox': [0.2, 0.2, 0.5, 0.5]}]
    o = PV.PreviewOptions(confidence_threshold=0.9)
    assert [d['category'] for d in PV.drawn_detections(dets, o, {'1': 0.5, '2': 0.6})] == ['1']
    assert [d['category'] for d in PV.drawn_detections(dets, o, {'1': None, '2': 0.5})] == ['1', '2']
    with pytest.raises(KeyError):
        PV.drawn_detections(dets, o, {'1': 0.5})
