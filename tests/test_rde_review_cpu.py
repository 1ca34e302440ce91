"""
The RDE review folder without a GPU: the host model of the thumbnails kernel (mdjpeg_thumbnails: the statements of
csrc/resample.h the lanes run) against Pillow bit for bit; the plan of a sample (rde_review.sample_plan) and the host leg's
files against what the REAL reference did on the same seeded scene (tests/golden/rde_review_reference.json, made by
tests/golden/gen_rde_review_golden_from_reference.py); the removal pass against the reference's; what a failing sample
leaves; the index; and that find_repeat_detections itself still refuses the review-folder options.
"""

import copy
import datetime
import hashlib
import json
import os

import numpy as np
import pytest

import rde_review_scene as S
import thumbnail_cases as T
from megadetector_amd import jpeg_host as J
from megadetector_amd import rde_review as RV
from megadetector_amd import repeat_detections as RD

HERE = os.path.dirname(os.path.abspath(__file__))
NOW = datetime.datetime(2024, 5, 6, 7, 8, 9)

with open(os.path.join(HERE, 'golden', 'rde_review_reference.json')) as f:
    GOLDEN = json.load(f)


def rde_options():
    o = RD.RepeatDetectionOptions()
    o.occurrenceThreshold = S.OCCURRENCE_THRESHOLD
    return o


def review_options(image_base, output_base, changes):
    o = RV.ReviewFolderOptions()
    o.imageBase, o.outputBase = str(image_base), str(output_base)
    for k, v in changes.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


@pytest.fixture(scope='module')
def scenes(tmp_path_factory):
    """scene name ('plain', 'thin') -> (image folder, results as the file holds them): made once"""
    out = {}
    for name, thin in (('plain', False), ('thin', True)):
        folder = tmp_path_factory.mktemp('rde_review_' + name)
        out[name] = (str(folder), S.make_scene(str(folder), thin=thin))
    return out


def found(scenes, thin):
    folder, results = scenes['thin' if thin else 'plain']
    return folder, results, RD.mark_repeat_detections(copy.deepcopy(results), rde_options(), backend='host')


def test_host_model_of_the_thumbnails_against_pillow():
    matrix = T.cases()
    where, heights = T.place([size for _, _, size in matrix])
    sheets = T.Sheets(heights)
    want = T.expected(matrix, where, sheets)
    tiles = []
    for (pixels, box, size), (s, x, y) in zip(matrix, where):
        (sx, sy, sw, sh), canvas = T.canvas_of(box, pixels.shape[1], pixels.shape[0])
        tiles.append((pixels[sy:sy + sh, sx:sx + sw] if sw else None, canvas, sheets.view(s), x, y, size[0], size[1]))
    assert J.thumbnails(tiles) is True                               # ONE call
    for s in range(3):
        assert np.array_equal(sheets.backing[s], want[s]), 'sheet {}'.format(s)


def test_host_model_filters_and_refusals():
    from PIL import Image
    rng = np.random.default_rng(3)
    pixels = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    for filt, pil in ((0, Image.BICUBIC), (1, Image.BILINEAR), (2, Image.LANCZOS)):
        for size in ((7, 5), (64, 40), (31, 9)):
            sheet = np.zeros((size[1], size[0], 3), np.uint8)
            assert J.thumbnails([(pixels, (31, 23, 0, 0), sheet, 0, 0, size[0], size[1])], filt)
            assert np.array_equal(sheet, np.asarray(Image.fromarray(pixels).resize(size, pil))), (filt, size)
    sheet = np.full((4, 4, 3), 7, np.uint8)
    with pytest.raises(ValueError):
        J.thumbnails([(pixels, (31, 23, 0, 0), sheet, 0, 0, 4, 4)], 3)                # an unknown filter
    with pytest.raises(ValueError):
        J.thumbnails([(pixels, (31, 23, 1, 0), sheet, 0, 0, 4, 4)])                   # the rectangle leaves its canvas
    with pytest.raises(ValueError):
        J.thumbnails([(pixels, (31, 23, 0, 0), sheet, 1, 0, 4, 4)])                   # the tile leaves its sheet
    # a canvas of height 60000 around 8 rows, reduced to one output row: the rows of one output row do not fit on chip
    assert J.thumbnails([(pixels[:8], (31, 60000, 0, 100), sheet, 0, 0, 4, 1)]) is False
    assert (sheet == 7).all()


@pytest.mark.parametrize('name', list(S.OPTION_SETS))
def test_plan_against_the_reference(scenes, name, tmp_path):
    from PIL import Image
    thin, changes = S.OPTION_SETS[name]
    golden = GOLDEN['option_sets'][name]
    assert golden['options'] == changes and golden['thin'] == thin
    folder, results, rde = found(scenes, thin)
    # the marking itself, against the reference's
    signs = [None if im.get('detections') is None else [1 if d['conf'] < 0 else 0 for d in im['detections']]
             for im in rde.detectionResults['images']]
    assert signs == golden['marked']
    options = review_options(folder, tmp_path, changes)
    flat = RV.name_samples(rde.suspicious_detections)
    assert sorted(loc.sampleImageRelativeFileName for loc in flat) == golden['samples']

    def size_of(f):
        with Image.open(os.path.join(folder, f)) as im:
            return im.size

    for location in flat:
        want = golden['files'][location.sampleImageRelativeFileName]
        if thin:
            # the first box is 200 : 1: a tile of height 0 -- the reference left the primary-only file
            with pytest.raises(ValueError, match='height and width must be > 0'):
                RV.sample_plan(location, options, size_of)
            assert want['tiles'] == [] and want['size'] == [S.WIDTH, S.HEIGHT]
            continue
        plan = RV.sample_plan(location, options, size_of)
        if plan['layout'] is None:
            assert want['tiles'] == [] and want['primary'] is None and list(plan['image']) == want['size']
            continue
        assert list(plan['layout']['sheet']) == want['size']
        assert list(plan['layout']['primary']) == want['primary']['size']
        assert [plan['layout']['primary_x'], 0] == want['primary']['position']
        assert [{'crop': list(box), 'size': list(size), 'position': list(position)} for _, box, size, position in plan['tiles']] == want['tiles']


@pytest.mark.parametrize('name', list(S.OPTION_SETS))
def test_host_leg_files_against_the_reference(scenes, name, tmp_path):
    from PIL import Image
    import PIL
    thin, changes = S.OPTION_SETS[name]
    golden = GOLDEN['option_sets'][name]
    folder, _, rde = found(scenes, thin)
    counts = RV.write_review_folder(rde, review_options(folder, tmp_path, changes), backend='host', now=NOW, rde_options=rde_options())
    assert os.path.basename(counts['folder']) == 'filtering_2024.05.06.07.08.09'
    assert counts['sheets'] == counts['host'] == len(golden['samples']) and counts['gpu'] == 0
    assert sorted(os.listdir(counts['folder'])) == sorted(golden['samples'] + [RV.INDEX_NAME])
    for sample in golden['samples']:
        path = os.path.join(counts['folder'], sample)
        with Image.open(path) as im:
            assert list(im.size) == golden['files'][sample]['size']
        if PIL.__version__ == GOLDEN['pillow']:                          # the bytes are those of one Pillow version
            with open(path, 'rb') as f:
                assert hashlib.sha256(f.read()).hexdigest() == golden['files'][sample]['sha256'], sample


@pytest.mark.parametrize('name', ['defaults', 'primary_left'])
def test_removal_against_the_reference(scenes, name, tmp_path):
    golden = GOLDEN['option_sets'][name]
    removal = golden['removal']
    folder, results, rde = found(scenes, False)
    counts = RV.write_review_folder(rde, review_options(folder, tmp_path / 'out', S.OPTION_SETS[name][1]), backend='host', now=NOW,
                                    rde_options=rde_options())
    original = tmp_path / 'in.json'
    original.write_text(json.dumps(results))
    output = tmp_path / 'removed.json'
    if removal['form'] == 'deleted_files':
        for sample in removal['deleted']:
            os.remove(os.path.join(counts['folder'], sample))
        out = RV.remove_repeat_detections(str(original), str(output), counts['folder'], backend='host')
    else:
        keep = tmp_path / 'keep.txt'
        keep.write_text('\n'.join(s for s in golden['samples'] if s not in removal['deleted']) + '\n')
        out = RV.remove_repeat_detections(str(original), str(output), os.path.join(counts['folder'], RV.INDEX_NAME), str(keep), backend='host')
    written = json.loads(output.read_text())
    signs = [None if im.get('detections') is None else [1 if d['conf'] < 0 else 0 for d in im['detections']] for im in written['images']]
    assert signs == removal['negative']
    assert signs != golden['marked']                                     # (the deleted samples un-marked something)
    assert sum(len(s) for s in out.suspicious_detections) == len(golden['samples']) - len(removal['deleted'])
    # the writer of repeat_detections: values as they were, no "detections": null
    for a, b in zip(results['images'], written['images']):
        assert [abs(d['conf']) for d in a['detections']] == [abs(d['conf']) for d in b['detections']]


def test_a_sample_whose_tiles_fail_keeps_its_primary(scenes, tmp_path):
    from PIL import Image
    folder, _, rde = found(scenes, True)
    counts = RV.write_review_folder(rde, review_options(folder, tmp_path / 'a', {}), backend='host', now=NOW)
    samples = [f for f in os.listdir(counts['folder']) if f.endswith('.jpg')]
    assert len(samples) == 1
    with Image.open(os.path.join(counts['folder'], samples[0])) as im:
        assert im.size == (S.WIDTH, S.HEIGHT)
    _, _, rde = found(scenes, True)
    with pytest.raises(ValueError, match='height and width must be > 0'):
        RV.write_review_folder(rde, review_options(folder, tmp_path / 'b', {'bFailOnRenderError': True}), backend='host', now=NOW)
    # a missing instance file: the primary-only file too; a missing first image of the results: the early check
    folder, _, rde = found(scenes, False)
    flat = RV.name_samples(rde.suspicious_detections)
    flat[0].instances[-1].filename = 'camA/gone.jpg'
    counts = RV.write_review_folder(rde, review_options(folder, tmp_path / 'c', {}), backend='host', now=NOW)
    with Image.open(os.path.join(counts['folder'], flat[0].sampleImageRelativeFileName)) as im:
        assert im.size == (S.WIDTH, S.HEIGHT)
    with Image.open(os.path.join(counts['folder'], flat[1].sampleImageRelativeFileName)) as im:
        assert im.size == (256, 120)
    with pytest.raises(ValueError, match='imageBase'):
        RV.write_review_folder(rde, review_options(tmp_path, tmp_path / 'd', {}), backend='host', now=NOW)


def test_the_index_round_trips(scenes, tmp_path):
    folder, _, rde = found(scenes, False)
    counts = RV.write_review_folder(rde, review_options(folder, tmp_path, {'detectionTilesMaxCrops': 3}), backend='host', now=NOW,
                                    rde_options=rde_options())
    index, suspicious = RV.load_index(os.path.join(counts['folder'], RV.INDEX_NAME))
    assert index['options']['occurrenceThreshold'] == S.OCCURRENCE_THRESHOLD and index['review_options']['detectionTilesMaxCrops'] == 3
    assert index['dirs'] == rde.dirs and index['dir_index_to_name'] == {str(i): d for i, d in enumerate(rde.dirs)}
    assert len(suspicious) == len(rde.suspicious_detections)
    for got, want in zip(suspicious, rde.suspicious_detections):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert (a.sampleImageRelativeFileName, a.bbox, a.category, a.relativeDir, a.id) == \
                (b.sampleImageRelativeFileName, b.bbox, b.category, b.relativeDir, b.id)
            assert [(i.filename, i.i_detection, i.bbox, i.confidence, i.category) for i in a.instances] == \
                [(i.filename, i.i_detection, i.bbox, i.confidence, i.category) for i in b.instances]
    # what the second write of the same index gives is the same file
    again = RD.RepeatDetectionResults()
    again.dirs, again.suspicious_detections = rde.dirs, suspicious
    assert RV.index_for_folder(again, rde_options(), review_options(folder, tmp_path, {'detectionTilesMaxCrops': 3})) == index


def test_the_options_the_review_folder_does_not_restate():
    o = RV.ReviewFolderOptions()
    assert (o.lineThickness, o.boxExpansion, o.bRenderDetectionTiles, o.detectionTilesPrimaryImageWidth, o.detectionTilesCroppedGridWidth,
            o.detectionTilesPrimaryImageLocation, o.detectionTilesMaxCrops, o.bFailOnRenderError) == (10, 2, True, None, 0.6, 'right', 150, False)
    o.outputBase = 'x'
    for k, v in (('bRenderOtherDetections', True), ('maxOutputImageWidth', 800), ('otherDetectionsThreshold', 0.2)):
        bad = copy.copy(o)
        setattr(bad, k, v)
        with pytest.raises(NotImplementedError):
            RV.check_review_options(bad)


def test_find_repeat_detections_still_refuses_the_review_folder(scenes, tmp_path):
    _, results = scenes['plain']
    path = tmp_path / 'in.json'
    path.write_text(json.dumps(results))
    assert RD.RepeatDetectionOptions().bWriteFilteringFolder is False
    for k, v in (('bWriteFilteringFolder', True), ('filterFileToLoad', 'x/detectionIndex.json'), ('bRenderDetectionTiles', True),
                 ('outputBase', 'x')):
        o = rde_options()
        setattr(o, k, v)
        with pytest.raises(NotImplementedError, match='review folder'):
            RD.find_repeat_detections(str(path), None, o, backend='host')


def test_command_line(scenes, tmp_path):
    folder, results = scenes['plain']
    path = tmp_path / 'in.json'
    path.write_text(json.dumps(results))
    assert RV.main(['write', str(path), '--imageBase', folder, '--outputBase', str(tmp_path / 'out'), '--outputFile', str(tmp_path / 'marked.json'),
                    '--occurrenceThreshold', str(S.OCCURRENCE_THRESHOLD), '--detectionTilesMaxCrops', '3', '--backend', 'host']) == 0
    (made,) = os.listdir(tmp_path / 'out')
    samples = sorted(f for f in os.listdir(tmp_path / 'out' / made) if f.endswith('.jpg'))
    assert samples == GOLDEN['option_sets']['max_crops_3']['samples']
    os.remove(tmp_path / 'out' / made / samples[0])
    assert RV.main(['remove', str(path), str(tmp_path / 'removed.json'), str(tmp_path / 'out' / made)]) == 0
    marked, removed = json.loads((tmp_path / 'marked.json').read_text()), json.loads((tmp_path / 'removed.json').read_text())
    n = [sum(d['conf'] < 0 for im in r['images'] for d in im['detections']) for r in (marked, removed)]
    assert 0 < n[1] < n[0]


def test_run_detector_batch_writes_the_review_folder(tmp_path, monkeypatch):
    """--rde_review_folder: off by default, only with --rde_results_file, the main results byte for byte unchanged"""
    from PIL import Image
    from megadetector_amd import run_detector_batch as RDB
    from stub_detector import StubDetector
    root = tmp_path / 'images'
    rng = np.random.default_rng(0)
    for cam in ('cam0', 'cam1'):
        os.makedirs(root / cam)
        for i in range(6):
            Image.fromarray(rng.integers(0, 256, (90 + i, 120, 3), dtype=np.uint8)).save(root / cam / 'img_{}.png'.format(i))
    monkeypatch.setattr(RDB.run_detector, 'load_detector', lambda *a, **k: StubDetector())
    monkeypatch.setattr(RDB, 'datetime', type('FixedClock', (), {'now': staticmethod(lambda: __import__('datetime').datetime(2024, 1, 2))}))
    plain, with_rde, rde = str(tmp_path / 'plain.json'), str(tmp_path / 'with.json'), str(tmp_path / 'rde.json')
    common = ['stub', str(root), None, '--output_relative_filenames', '--recursive', '--quiet']
    RDB.main(common[:2] + [plain] + common[3:])
    RDB.main(common[:2] + [with_rde] + common[3:] + ['--rde_results_file', rde, '--rde_occurrence_threshold', '3', '--rde_iou_threshold', '0.8',
                                                     '--rde_backend', 'host', '--rde_review_folder', str(tmp_path / 'review')])
    assert open(plain, 'rb').read() == open(with_rde, 'rb').read()
    (made,) = os.listdir(tmp_path / 'review')
    assert made.startswith('filtering_')
    index, suspicious = RV.load_index(str(tmp_path / 'review' / made / RV.INDEX_NAME))
    names = sorted(loc.sampleImageRelativeFileName for locs in suspicious for loc in locs)
    assert names and sorted(os.listdir(tmp_path / 'review' / made)) == sorted(names + [RV.INDEX_NAME])
    assert index['review_options']['imageBase'] == str(root)
    with pytest.raises(AssertionError, match='--rde_results_file'):
        RDB.main(common[:2] + [str(tmp_path / 'x.json')] + common[3:] + ['--rde_review_folder', str(tmp_path / 'y')])


def test_host_model_under_sanitizers(tmp_path):
    """mdjpeg_thumbnails in a stand-alone build of image_host.cpp with AddressSanitizer + UBSan (host code; `make asan-jpeg`,
    the --thumbnails mode of host_asan_main.cpp): sources and sheets of their exact sizes at every alignment, LDS tiles of exactly the planned size --
    any access outside them, and any undefined arithmetic, ends the run"""
    import shutil
    import subprocess
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.skip('no g++')
    probe = subprocess.run([cxx, '-fsanitize=address,undefined', '-x', 'c++', '-', '-o', str(tmp_path / 'probe')],
                           input=b'int main() { return 0; }', capture_output=True)
    if probe.returncode != 0:
        pytest.skip('g++ has no sanitizer runtime')
    exe = str(tmp_path / 'jpeg_entropy_asan')
    subprocess.check_call(['make', '-C', os.path.join(os.path.dirname(HERE), 'megadetector_amd', 'csrc'), 'asan-jpeg', 'ASAN_OUT=' + exe])
    r = subprocess.run([exe, '--thumbnails'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'thumbnails: 48 runs' in r.stdout
