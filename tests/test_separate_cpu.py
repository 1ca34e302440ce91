"""
megadetector_amd.separate_detections against the reference's separate_detections_into_folders, host side: the folder decision,
the file handling and the host leg of the manipulated copies, on the scene of tests/separate_scene.py, against
tests/golden/separate_reference.json (written by tests/golden/gen_separate_golden_from_reference.py from the reference's own
run).  The paths of the output tree and which files are byte copies are compared always; the bytes of the manipulated files
when Pillow is the recorded version and writes the recorded scene, otherwise their sampling, tables, dimensions and segments.
"""

import io
import json
import os
from contextlib import redirect_stdout

import PIL
import pytest

import separate_scene as S
from conftest import REPO
from megadetector_amd import separate_detections as SD

GOLDEN = json.load(open(os.path.join(REPO, 'tests', 'golden', 'separate_reference.json')))


def _scene_hash(sources):
    import hashlib
    return hashlib.sha256(json.dumps(sorted(sources.items())).encode()).hexdigest()


def run_set(tmp, name, backend='host', **kw):
    """-> (tree, sources left, counts, same bytes expected)"""
    image_folder, results_file = S.build(str(tmp))
    sources = S.source_hashes(image_folder)
    out = os.path.join(str(tmp), 'out')
    if name == 'no_overwrite':
        S.prepare_existing(out)
    options = S.apply_options(SD.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out, S.OPTION_SETS[name])
    with redirect_stdout(io.StringIO()):
        counts = SD.separate_detections_into_folders(options, backend=backend, **kw)
    exact = PIL.__version__ == GOLDEN['pillow'] and _scene_hash(sources) == GOLDEN['scene']
    return S.describe_tree(out, sources), sorted(S.source_hashes(image_folder).values()), counts, exact


def compare_tree(tree, want, exact):
    assert sorted(tree) == sorted(want)
    for name, entry in want.items():
        got = tree[name]
        assert got.get('copy_of') == entry.get('copy_of') and got.get('empty_folder') == entry.get('empty_folder'), name
        if entry.get('empty_folder') or entry.get('copy_of') is not None:
            continue
        if exact:
            assert got['sha256'] == entry['sha256'], '{}: the bytes differ'.format(name)
        for key in ('size', 'quant', 'sampling', 'segments'):
            assert got.get(key) == entry.get(key), '{}: {}'.format(name, key)


def test_the_scene_and_the_option_sets_cover_what_they_must():
    assert len(S.OPTION_SETS) >= 8 and sorted(GOLDEN['sets']) == sorted(S.OPTION_SETS)
    for needed in ('defaults', 'per_category', 'skip_empty', 'move', 'render_boxes', 'blur_and_boxes', 'classification_labels', 'no_overwrite'):
        assert needed in S.OPTION_SETS
    assert all(w <= 96 and h <= 64 for _, w, h, _, _ in S.IMAGES)
    tree = GOLDEN['sets']['render_boxes']['tree']
    samplings = {json.dumps(e['sampling'][0]) for e in tree.values() if e.get('sampling')}
    assert samplings == {'[1, 1]', '[2, 1]', '[2, 2]'}
    assert 0xE1 in tree['animal_person/exif_com.jpg']['segments'] and 0xFE in tree['animal_person/exif_com.jpg']['segments']
    assert tree['animal_person/rot6.jpg']['size'] == [64, 96] and tree['animals/grey.jpg']['sampling'][0] == [2, 2]
    assert tree['processing_failure/failed.jpg']['copy_of'] == 'failed.jpg' and tree['empty/empty.jpg']['copy_of'] == 'empty.jpg'
    folders = GOLDEN['sets']['classification_folders']['tree']
    assert {'animals/deer/sub/deer.jpg', 'animals/multiple/sub/multi.jpg', 'animals/unclassified/sub/bird.jpg',
            'animals/unclassified/sub/edge.jpg'} <= set(folders)
    assert 'animals/thresh.jpg' in GOLDEN['sets']['defaults']['tree']          # a confidence exactly at the threshold is in


@pytest.mark.parametrize('name', sorted(S.OPTION_SETS))
def test_host_backend_writes_the_tree_of_the_reference(tmp_path, name):
    tree, left, counts, exact = run_set(tmp_path, name)
    want = GOLDEN['sets'][name]
    print('exact bytes compared:', exact, counts)
    compare_tree(tree, want['tree'], exact)
    assert left == want['sources_left']
    n_manipulated = sum(1 for e in want['tree'].values() if not e.get('empty_folder') and e.get('copy_of') is None
                        and e['sha256'] not in {__import__('hashlib').sha256(v).hexdigest() for v in S.EXISTING.values()})
    assert counts['rendered'] == counts['host'] == n_manipulated and counts['gpu'] == 0
    assert counts['missing'] == 1 and counts['images'] == len(S.IMAGES) + 1


@pytest.mark.parametrize('name', sorted(S.ERROR_CASES))
def test_error_cases_raise_what_the_reference_raises(tmp_path, name):
    attributes = S.ERROR_CASES[name]
    image_folder, results_file = S.build(str(tmp_path))
    out = os.path.join(str(tmp_path), 'out')
    results_file = S.prepare_error_case(attributes, results_file, out)
    options = S.apply_options(SD.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, out, attributes)
    want = GOLDEN['errors'][name]
    with pytest.raises({'AssertionError': AssertionError, 'ValueError': ValueError, 'KeyError': KeyError}[want['type']]) as e:
        with redirect_stdout(io.StringIO()):
            SD.separate_detections_into_folders(options, backend='host')
    assert str(e.value).replace(str(tmp_path), '<tmp>') == want['message']


def _options(**kw):
    o = SD.SeparateDetectionsIntoFoldersOptions()
    o.base_output_folder = 'out'
    for k, v in kw.items():
        setattr(o, k, v)
    with redirect_stdout(io.StringIO()):
        SD.resolve_options(o, S.results())
    return o


def test_the_folder_decision_is_a_pure_function_of_entry_and_options():
    o = _options()
    by_name = {im['file']: im for im in S.results()['images']}
    rel = lambda name: os.path.relpath(SD.decide(by_name[name], o)[0], 'out').replace(os.sep, '/')
    assert o.category_name_to_threshold == {'animal': 0.2, 'person': 0.2, 'vehicle': 0.2}          # MDv5's typical threshold
    assert [rel(n) for n in ('a444.jpg', 'a422.jpg', 'a420.jpg', 'exif_com.jpg', 'all3.jpg', 'empty.jpg', 'blank.jpg', 'failed.jpg')] == \
        ['animals', 'people', 'vehicles', 'animal_person', 'animal_person_vehicle', 'empty', 'empty', 'processing_failure']
    assert SD.decide(by_name['thresh.jpg'], o) == (os.path.join('out', 'animals'), ['animal'])     # >= on 0.2, 0.19999 is out
    assert SD.decide(by_name['failed.jpg'], o)[1] is None
    assert sorted(os.path.basename(v) for v in o.category_name_to_folder.values()) == sorted(
        ['empty', 'processing_failure', 'animals', 'people', 'vehicles', 'animal_person', 'animal_vehicle', 'person_vehicle',
         'animal_person_vehicle'])
    # a detection equal to the running maximum does not replace it (>), and an unknown category is skipped
    im = {'file': 'x.jpg', 'detections': [{'category': '9', 'conf': 0.99, 'bbox': [0, 0, 1, 1]}]}
    with redirect_stdout(io.StringIO()):
        assert SD.decide(im, o)[1] == []
    # species folders: strictly above the classification threshold; 'multiple' for two listed ones; unlisted ones do not count alone
    c = _options(classification_thresholds='deer=0.75,cow=0.75')
    assert c.classification_thresholds == {'deer': 0.75, 'cow': 0.75}
    crel = lambda name: os.path.relpath(SD.decide(by_name[name], c)[0], 'out').replace(os.sep, '/')
    assert [crel(n) for n in ('sub/deer.jpg', 'sub/multi.jpg', 'sub/bird.jpg', 'sub/edge.jpg', 'exif_com.jpg')] == \
        ['animals/deer', 'animals/multiple', 'animals/unclassified', 'animals/unclassified', 'animal_person']
    p = _options(threshold=0.65, category_name_to_threshold={'animal': 0.55, 'person': 0.85, 'vehicle': None})
    assert p.category_name_to_threshold == {'animal': 0.55, 'person': 0.85, 'vehicle': 0.65}
    prel = lambda name: os.path.relpath(SD.decide(by_name[name], p)[0], 'out').replace(os.sep, '/')
    assert [prel(n) for n in ('a422.jpg', 'a420.jpg', 'rot6.jpg', 'all3.jpg')] == ['empty', 'vehicles', 'people', 'animal_person_vehicle']


def test_typical_threshold_and_debug_max_images(tmp_path):
    r = S.results()
    with redirect_stdout(io.StringIO()):
        assert SD.get_typical_confidence_threshold_from_results(r) == 0.2
        r['info']['detector_metadata'] = {'typical_detection_threshold': 0.37}
        assert SD.get_typical_confidence_threshold_from_results(r) == 0.37
        assert SD.get_typical_confidence_threshold_from_results({'info': {}}) == 0.2
    image_folder, results_file = S.build(str(tmp_path))
    options = S.apply_options(SD.SeparateDetectionsIntoFoldersOptions(), image_folder, results_file, str(tmp_path / 'out'),
                              {'debug_max_images': 3})
    with redirect_stdout(io.StringIO()):
        counts = SD.separate_detections_into_folders(options, backend='host')
    assert counts['images'] == 3 and counts['copied'] == 3
    with pytest.raises(ValueError, match='backend'):
        SD.separate_detections_into_folders(options, backend='cuda')


def test_command_line_runs_the_host_backend(tmp_path):
    image_folder, results_file = S.build(str(tmp_path))
    out = str(tmp_path / 'out')
    os.remove(os.path.join(image_folder, 'failed.jpg'))                  # (the command line has no allow_missing_files)
    data = json.load(open(results_file))
    data['images'] = [im for im in data['images'] if im['file'] not in (S.MISSING, 'failed.jpg')]
    json.dump(data, open(results_file, 'w'))
    with redirect_stdout(io.StringIO()):
        assert SD.main([results_file, image_folder, out, '--animal_threshold', '0.55', '--human_threshold', '0.85', '--threshold', '0.65',
                        '--render_boxes', '--category_names_to_blur', 'person', '--backend', 'host', '--n_threads', '2']) == 0
    assert os.path.isfile(os.path.join(out, 'animal_person_vehicle', 'all3.jpg')) and os.path.isfile(os.path.join(out, 'empty', 'a422.jpg'))
    with pytest.raises(AssertionError, match='Illegal animal threshold'):
        SD.main([results_file, image_folder, out, '--animal_threshold', '1.5', '--backend', 'host'])
