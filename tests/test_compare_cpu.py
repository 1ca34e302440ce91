"""
megadetector_amd.compare_batch_results against the reference's compare_batch_results, host side: the categories, the samples,
the output names, the HTML and the host leg of the rendering, on the scene of tests/compare_scene.py, against
tests/golden/compare_reference.json (written by tests/golden/gen_compare_reference.py from the reference's own run).  The
samples, the tree and the HTML texts are compared always; the hashes of the rendered files when Pillow is the recorded
version and writes the recorded scene.  Independently of the fixture rendered files are compared with what direct Pillow
calls write, and the device leg's steps are run on the kernels' host models (mdjpeg_resample, mdjpeg_draw_from).
"""

import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import PIL
import pytest
from PIL import Image, ImageDraw

import compare_scene as S
from conftest import REPO
from megadetector_amd import compare_batch_results as C
from megadetector_amd import jpeg_host as J
from megadetector_amd import preview as PV

GOLDEN = S.load_golden(os.path.join(REPO, 'tests', 'golden', 'compare_reference.json'))


def run_set(tmp, name, backend='host', **kw):
    """-> (what the run wrote (describe_output), the results, the sampled [folder, file] in rendering order, whether the same
    bytes are expected)"""
    tmp = str(tmp)
    image_folder, files = S.build(tmp)
    out = os.path.join(tmp, 'out')
    sampled = []
    real = C.render_job_host

    def recorded(job):
        sampled.append([os.path.relpath(os.path.dirname(job['output_path']), out).replace(os.sep, '/'), job['file']])
        return real(job)

    C.render_job_host = recorded
    try:
        with redirect_stdout(io.StringIO()):
            results = S.run(C, name, image_folder, files, out, backend=backend, **kw)
    finally:
        C.render_job_host = real
    assert results.html_output_file == os.path.join(out, 'index.html')
    exact = PIL.__version__ == GOLDEN['pillow'] and S.scene_hash(image_folder) == GOLDEN['scene']
    return S.describe_output(out, tmp), results, sampled, exact


def compare_output(got, want, exact):
    assert got['tree'] == want['tree']
    assert sorted(got['html']) == sorted(want['html'])
    for name, text in want['html'].items():
        assert got['html'][name] == text, '{}: the text differs'.format(name)
    assert sorted(got['sha256']) == sorted(want['sha256'])
    if exact:
        for name, sha in want['sha256'].items():
            assert got['sha256'][name] == sha, '{}: the bytes differ'.format(name)


def _categories(record, comparison='cmp_000'):
    return {c: [f for folder, f in record['sampled'] if folder == comparison + '/' + c] for c in C.CATEGORIES_TO_PAGE_TITLES}


def test_the_scene_and_the_option_sets_cover_what_the_issue_lists():
    assert len(S.OPTION_SETS) >= 15 and sorted(GOLDEN['sets']) == sorted(S.OPTION_SETS)
    assert len(S.IMAGES) == 12 and all(96 <= w <= 400 and 96 <= h <= 400 for _, w, h, *_ in S.IMAGES)
    assert {how.get('subsampling', 2) for _, _, _, how, *_ in S.IMAGES if how.get('mode') != 'L' and how} == {0, 1, 2}
    assert sum(1 for im in S.IMAGES if im[3].get('mode') == 'L') == 1 and sum(1 for im in S.IMAGES if 'exif' in im[3]) == 1
    assert sum(1 for im in S.IMAGES if im[0].endswith('.png')) == 1 and sum(1 for im in S.IMAGES if '/' in im[0]) == 1
    assert [im[0] for im in S.IMAGES if im[5] is None] == [S.FAILED_IN_B]
    n_way = GOLDEN['sets']['n_way']
    per = [_categories(n_way, 'cmp_00{}'.format(i)) for i in range(3)]
    for category in C.CATEGORIES_TO_PAGE_TITLES:                    # every category is non-empty in some comparison
        assert any(p[category] for p in per), category
    where = {f: {c for p in per for c, files in p.items() if f in files} for f in S.FILES}
    assert sum(len(v) > 1 for v in where.values()) >= 5             # files that change their category between comparisons
    assert not any(S.FAILED_IN_B in files for files in per[0].values()) and any(S.FAILED_IN_B in files for files in per[1].values())
    dets = [d for im in S.IMAGES for side in im[4:] if side for d in side]
    assert any('transferred_from' in d for d in dets) and any('classifications' in d for d in dets)
    assert 'cmp_000/common_detections/sub~deep.jpg' in GOLDEN['sets']['defaults']['tree']
    assert any('image_00000_00002' in t for t in GOLDEN['sets']['pages_of_3']['tree'])
    assert '<b>Contents</b>' in n_way['html']['index.html'] and '<b>Contents</b>' not in GOLDEN['sets']['defaults']['html']['index.html']
    two = [GOLDEN['sets'][n]['sampled'] for n in ('sample_2_seed_0', 'sample_2_seed_7')]
    assert two[0] != two[1] and all(len(_categories(GOLDEN['sets'][n])['common_detections']) == 2 for n in ('sample_2_seed_0', 'sample_2_seed_7'))
    assert S.MISSING_FROM_B_SHORT not in [f for _, f in GOLDEN['sets']['non_matching']['sampled']]
    assert 'shown as C444.JPG' in GOLDEN['sets']['display_fn']['html']['cmp_000/common_detections.html']
    for name in S.N_WAY_SETS:
        e = GOLDEN['sets'][name]['expected']
        assert e['files_decoded_pil'] == 1 and 0 < e['host'] < e['jobs'] and e['files_decoded_gpu'] < e['jobs'] - e['host']


@pytest.mark.parametrize('name', sorted(S.OPTION_SETS))
def test_host_backend_writes_what_the_reference_writes(tmp_path, name):
    got, results, sampled, exact = run_set(tmp_path, name)
    want = GOLDEN['sets'][name]
    print('exact bytes compared:', exact, results.counts)
    compare_output(got, want, exact)
    assert sampled == want['sampled']
    counts = results.counts
    assert counts['jobs'] == counts['host'] == len(want['sha256']) == want['expected']['jobs'] and counts['gpu'] == 0
    assert counts['decode_chunks'] == counts['resample_calls'] == counts['draw_calls'] == counts['encode_calls'] == 0
    assert counts['files_decoded_gpu'] == counts['files_decoded_pil'] == 0
    assert all(r.categories_to_image_pairs is None for r in results.pairwise_results)


def test_the_pool_of_the_host_leg_writes_the_same_files(tmp_path):
    image_folder, files = S.build(str(tmp_path))
    trees = []
    for workers, threads in ((1, True), (3, True), (2, False)):
        options = C.BatchComparisonOptions()
        options.output_folder, options.image_folder = str(tmp_path / 'out_{}_{}'.format(workers, threads)), image_folder
        options.n_rendering_workers, options.parallelize_rendering_with_threads = workers, threads
        options.return_images_by_category = True
        with redirect_stdout(io.StringIO()):
            results = C.n_way_comparison([files['a'], files['b'], files['c']], options, backend='host')
        trees.append(S.describe_output(options.output_folder, str(tmp_path))['sha256'])
        assert set(results.pairwise_results[0].categories_to_image_pairs) == set(C.CATEGORIES_TO_PAGE_TITLES)
        assert 'sort_conf' in results.pairwise_results[0].categories_to_image_pairs['common_detections']['c444.jpg']
    assert trees[0] == trees[1] == trees[2] and len(trees[0]) == GOLDEN['sets']['n_way']['expected']['jobs']


def _pair(tmp_path, a='a', b='b', **attributes):
    image_folder, files = S.build(str(tmp_path))
    options = C.BatchComparisonOptions()
    options.output_folder, options.image_folder, options.n_rendering_workers = str(tmp_path / 'out'), image_folder, 1
    pairwise = C.PairwiseBatchComparisonOptions()
    pairwise.results_filename_a, pairwise.results_filename_b = files[a], files[b]
    options.pairwise_options = [pairwise]
    for k, v in attributes.items():
        setattr(options, k, v)
    return options, files


def _quiet(options, **kw):
    with redirect_stdout(io.StringIO()):
        return C.compare_batch_results(options, backend='host', **kw)


def test_the_error_cases_raise_what_the_reference_raises(tmp_path):
    options, files = _pair(tmp_path / 'lists', b='b_short')
    with pytest.raises(ValueError, match='set A has 12 images, set B has 11'):
        _quiet(options)
    options, files = _pair(tmp_path / 'categories')
    other = json.load(open(files['b']))
    other['detection_categories']['3'] = 'truck'
    json.dump(other, open(files['b'], 'w'))
    with pytest.raises(AssertionError, match='different categories'):
        _quiet(options)
    options.class_agnostic_comparison = True
    _quiet(options)
    options, files = _pair(tmp_path / 'names')
    renamed = json.load(open(files['b']))
    renamed['images'][0]['file'] = 'elsewhere.jpg'
    json.dump(renamed, open(files['b'], 'w'))
    with pytest.raises(AssertionError):
        _quiet(options)                                              # same number of images, another name: the bare assertion
    options, files = _pair(tmp_path / 'missing')
    os.remove(os.path.join(options.image_folder, 'c444.jpg'))
    with pytest.raises(AssertionError, match='c444.jpg does not exist'):
        _quiet(options)
    options, files = _pair(tmp_path / 'display', fn_to_display_fn={'c444.jpg': 'x'})
    with pytest.raises(AssertionError, match='fn_to_display_fn provided, but'):
        _quiet(options)
    options, files = _pair(tmp_path / 'folder')
    options.image_folder = str(tmp_path / 'nowhere')
    with pytest.raises(AssertionError, match="Can't find image folder"):
        _quiet(options)
    options, files = _pair(tmp_path / 'results')
    options.pairwise_options[0].results_filename_b = str(tmp_path / 'nowhere.json')
    with pytest.raises(AssertionError, match="Can't find results file"):
        _quiet(options)
    options, files = _pair(tmp_path / 'backend')
    with pytest.raises(ValueError, match='backend'):
        C.compare_batch_results(options, backend='cuda')
    with pytest.raises(AssertionError):
        C.n_way_comparison([files['a'], files['b']], options, detection_thresholds=[0.1], backend='host')


def test_an_unknown_category_skips_the_image_with_the_warning(tmp_path):
    options, files = _pair(tmp_path, return_images_by_category=True)
    odd = json.load(open(files['a']))
    odd['images'][0]['detections'][0]['category'] = '9'
    json.dump(odd, open(files['a'], 'w'))
    text = io.StringIO()
    with redirect_stdout(text):
        results = C.compare_batch_results(options, backend='host')
    assert 'Warning: unexpected category 9 for model A on file c444.jpg' in text.getvalue()
    assert not any('c444.jpg' in pairs for pairs in results.pairwise_results[0].categories_to_image_pairs.values())


@pytest.mark.parametrize('attributes', [{'ground_truth_file': 'gt.json'}, {'ground_truth_file': {'images': [], 'annotations': []}}])
def test_ground_truth_raises_before_the_output_folder_exists(tmp_path, attributes):
    options, files = _pair(tmp_path, **attributes)
    with pytest.raises(NotImplementedError, match='ground truth'):
        C.compare_batch_results(options, backend='host')
    with pytest.raises(NotImplementedError, match='ground truth'):
        C.compare_batch_results(options, backend='gpu')
    assert not os.path.exists(options.output_folder)
    assert not hasattr(C, 'find_equivalent_threshold') and not hasattr(C, 'find_image_level_detections_above_threshold')


def test_category_names_are_compared_as_sets(tmp_path):
    """two categories above the threshold on both sides, found in different orders: a common detection, whatever order the
    sets iterate in"""
    options, files = _pair(tmp_path, category_names_to_include=['person', 'animal'], return_images_by_category=True)
    for which, order in (('a', ('1', '2')), ('b', ('2', '1'))):
        data = json.load(open(files[which]))
        data['images'][0]['detections'] = [{'category': c, 'conf': 0.9, 'bbox': [0.1, 0.1, 0.4, 0.4]} for c in order]
        json.dump(data, open(files[which], 'w'))
    results = _quiet(options)
    assert 'c444.jpg' in results.pairwise_results[0].categories_to_image_pairs['common_detections']


def test_a_rendered_file_is_what_direct_pillow_calls_write(tmp_path):
    """c444.jpg of the defaults, written out with Pillow alone: 400 x 300 enlarged to 800 x 600, A's box in Red with an outline
    of 4 and its label above, then B's in RoyalBlue with an outline of 2 and its label below"""
    got, results, _, _ = run_set(tmp_path / 'run', 'defaults')
    image = Image.open(os.path.join(str(tmp_path / 'run'), 'images', 'c444.jpg')).resize((800, 600), Image.Resampling.LANCZOS)
    font = PV.load_font('arial.ttf', 16)
    draw = ImageDraw.Draw(image)
    for (x, y, w, h), conf, color, thickness, below in (((0.1, 0.2, 0.5, 0.6), 90, 'Red', 4, False), ((0.12, 0.22, 0.5, 0.6), 85, 'RoyalBlue', 2, True)):
        left, top, right, bottom = x * 800, y * 600, (x + w) * 800, (y + h) * 600
        draw.rectangle([(left, top), (right, bottom)], outline=color, width=thickness)
        text = ' animal: {}% '.format(conf)
        _, _, tw, th = font.getbbox(text)
        margin = int(np.ceil(0.05 * th))
        total = (1 + 2 * 0.05) * font.getbbox(text.strip())[3]
        text_bottom = int(bottom + total) if below else int(top)
        draw.rectangle([(int(left), text_bottom - th - 2 * margin), (int(left) + tw, text_bottom)], fill=color)
        draw.text((int(left) + margin, text_bottom - th - margin), text, fill='black', font=font)
    direct = str(tmp_path / 'direct.jpg')
    image.save(direct)
    with open(direct, 'rb') as f, open(os.path.join(str(tmp_path / 'run'), 'out', 'cmp_000', 'common_detections', 'c444.jpg'), 'rb') as g:
        assert f.read() == g.read()


@pytest.mark.parametrize('name', ['n_way', 'n_way_80', 'n_way_none', 'two_colours', 'no_category_names', 'no_classification_categories',
                                  'dict_thresholds'])
def test_the_device_legs_steps_on_the_host_models_give_the_host_legs_pixels(tmp_path, name):
    """The device's way without a device: Pillow's decode ONCE per file, the host model of the resample kernel ONCE per file,
    and the plans of all jobs of the file (preview.render_plan with the colormap, the bottom alignment and the custom
    strings; A's, then B's) through the host model of the fan-out draw in ONE call must give, for every job the plan accepts,
    the pixels the host leg draws (the encoder is pinned by the crops' tests)."""
    image_folder, files = S.build(str(tmp_path))
    captured = {}

    def plan_only(options, **kwargs):
        with redirect_stdout(io.StringIO()):
            captured['jobs'] = [job for plan in C.plan_comparisons(options)[1] for job in plan['jobs']]
        raise StopIteration

    real, C.compare_batch_results = C.compare_batch_results, plan_only
    try:
        with pytest.raises(StopIteration):
            S.run(C, name, image_folder, files, str(tmp_path / 'out'))
    finally:
        C.compare_batch_results = real
    planned, host, undecodable = C.plan_device_jobs(captured['jobs'])
    assert undecodable == [S.PNG] and {j['file'] for j in host} == {S.PNG, S.THIN}
    assert len(planned) + len(host) == GOLDEN['sets'][name]['expected']['jobs'] and len(host) == GOLDEN['sets'][name]['expected']['host']
    checked = groups = customs = 0
    for group in C.group_by_file(planned):
        image = C.open_image(group[0]['input_path'])
        assert group[0]['source_size'] == image.size and all(j['size'] == group[0]['size'] for j in group)
        size = group[0]['size']
        pixels = np.ascontiguousarray(np.asarray(image))
        shared = J.resample_lanczos(pixels, size) if size != image.size else pixels.copy()
        before = shared.copy()
        dests = [np.full_like(shared, 0xA5) for _ in group]
        op_image, ops, packed = C.DR.pack_ops([j['plan'] for j in group])
        assert J.draw_ops_from([shared.ctypes.data], [size], [size[0] * 3], [d.ctypes.data for d in dests], [0] * len(group),
                               [size[0] * 3] * len(group), op_image, ops, bytes(packed)) == J.MDJPEG_OK
        assert np.array_equal(shared, before)
        for job, model in zip(group, dests):
            pil = image.resize(size, Image.Resampling.LANCZOS) if size != image.size else image.copy()
            for detections, o, kw in job['sides']:
                PV.render_with_pil(pil, detections, o, **kw)
            assert np.array_equal(model, np.asarray(pil)), (job['comparison'], job['category'], job['file'])
            checked += 1
            customs += any(' (' in label for label in job['plan'].labels)
        groups += 1
    assert checked == len(planned) and customs >= 1 and groups == GOLDEN['sets'][name]['expected']['files_decoded_gpu']


def test_bottom_alignment_takes_the_references_fall_backs():
    """VTEXTALIGN_BOTTOM: below the box; above it when below leaves the image; inside at the bottom when above leaves it too"""
    font = PV.load_font('arial.ttf', 16)
    _, _, _, th = font.getbbox(' x ')
    total = 1.1 * font.getbbox('x')[3]
    margin = int(np.ceil(0.05 * th))

    def bottom_of(top, bottom, height, align):
        _, _, _, (_, y1), _ = next(PV.stacked_labels(font, ['x'], 10, top, bottom, height, align))
        return y1

    assert bottom_of(40, 60, 200, 'bottom') == int(60 + total)
    assert bottom_of(40, 195, 200, 'bottom') == 40
    assert bottom_of(5, 195, 200, 'bottom') == 195
    assert bottom_of(40, 60, 200, 'top') == 40 and bottom_of(5, 60, 200, 'top') == int(60 + total) and bottom_of(5, 195, 200, 'top') == int(5 + total)
    assert margin >= 1
    with pytest.raises(ValueError):
        next(PV.stacked_labels(font, ['x'], 10, 40, 60, 200, 'middle'))


def test_colormap_and_custom_strings_follow_the_reference():
    assert PV.box_color('1')[0] == 'Red' and PV.box_color('1', ['Red'])[0] == 'Red' and PV.box_color(None)[0] == 'Red'
    assert PV.box_color('3', ['Red', 'Gold'])[0] == 'Gold' and PV.box_color(4, ['Red', 'Gold'])[0] == 'Red'
    assert PV.box_color(None, ['Red', 'Gold'])[0] == 'Gold'
    with pytest.raises(IndexError):
        PV.box_color(None, ['Red'])
    # the custom strings are indexed by the position in the list SORTED by confidence (the reference's i_detection)
    dets = [{'category': '2', 'conf': 0.9, 'bbox': [0.1, 0.1, 0.5, 0.5]}, {'category': '1', 'conf': 0.5, 'bbox': [0.3, 0.4, 0.5, 0.5]}]
    o = PV.PreviewOptions(confidence_threshold=0.1, output_image_width=None)
    plan = PV.render_plan(dets, 300, 200, o, S.DETECTION_CATEGORIES, custom_strings=['(first)', ''])
    assert plan.labels == ['animal: 50% (first)', 'person: 90%']
    plan = PV.render_plan(dets, 300, 200, o, S.DETECTION_CATEGORIES, custom_strings=['', None], labels=False)
    assert plan.labels == ['', ''] and all(op[0] == PV.OP_RECT for op in plan.ops)
    plan = PV.render_plan(dets, 300, 200, o, None, labels=False, custom_strings=['(only)', ''])
    assert plan.labels == [' (only)', '']
    with pytest.raises(AssertionError):
        PV.render_plan(dets, 300, 200, o, S.DETECTION_CATEGORIES, custom_strings=['x'])
    classified = [dict(dets[0], classifications=[['1', 0.9]])]
    with pytest.raises(PV.HostLeg):
        PV.render_plan(classified, 300, 200, o, None, labels=False, classification_confidence_threshold=0.3)
    plan = PV.render_plan(classified, 300, 200, o, None, labels=False, classification_confidence_threshold=0.3,
                          unlabelled_classifications=True, colormap=['Red', 'Gold', 'Lime', 'Aqua'])
    assert plan.ops[0][5] == 0xFFFF00                              # class 3 + 0: Aqua (R | G << 8 | B << 16)


def test_render_plan_without_the_new_arguments_plans_what_it_planned(tmp_path):
    """on the scene of tests/test_preview_cpu.py: the defaults of the new arguments are the plan's earlier behaviour, pinned
    here against an independent statement of it -- PREVIEW_COLORS by category, labels above (stacked_labels' 'top')"""
    from test_preview_cpu import EQUAL, LABEL_MAP, SCENE, SCENE_SIZE
    for dets, (w, h), o in ((SCENE, SCENE_SIZE, PV.PreviewOptions()), (EQUAL, (301, 177), PV.PreviewOptions(box_expansion=10))):
        plain = PV.render_plan(dets, w, h, o, LABEL_MAP, True)
        explicit = PV.render_plan(dets, w, h, o, LABEL_MAP, True, colormap=None, vtextalign='top', custom_strings=None,
                                  unlabelled_classifications=False)
        named = PV.render_plan(dets, w, h, o, LABEL_MAP, True, colormap=list(PV.PREVIEW_COLORS), custom_strings=[''] * len(dets))
        for other in (explicit, named):
            assert (plain.ops, bytes(plain.patches), plain.labels, plain.order) == (other.ops, bytes(other.patches), other.labels, other.order)
        image = Image.new('RGB', (w, h), (40, 50, 60))
        want = image.copy()
        PV.render_with_pil(want, dets, o, LABEL_MAP, True)
        model = np.array(image)
        assert J.draw_ops(model, plain.ops, bytes(plain.patches)) == J.MDJPEG_OK and np.array_equal(model, np.asarray(want))
        assert plain.ops and any(op[0] == PV.OP_PATCH for op in plain.ops)


def test_the_command_line_maps_its_arguments_as_main_does(tmp_path):
    image_folder, files = S.build(str(tmp_path))
    out = str(tmp_path / 'out')
    text = io.StringIO()
    with redirect_stdout(text):
        results = C.main([out, image_folder, files['a'], files['b'], files['c'], '--detection_thresholds', '0.15', '0.15', '0.15',
                          '--n_rendering_workers', '1', '--open_results', '--backend', 'host'])
    assert '--open_results is accepted and ignored' in text.getvalue() and 'Wrote results to' in text.getvalue()
    compare_output(S.describe_output(out, str(tmp_path)), GOLDEN['sets']['n_way'], False)
    assert [p.pairwise_options.rendering_confidence_threshold_a for p in results.pairwise_results] == [0.15 * 0.6666] * 3
