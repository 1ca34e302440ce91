"""
Folder resizing without a GPU (megadetector_amd/resize_images.py):

  * the host leg equals what the reference's own resize_image_folder returned and wrote for every option set of
    tests/resize_scene.py (tests/golden/resize_reference.json, written by tests/golden/gen_resize_reference.py): the result lists
    and, file by file, SHA-256, size, dimensions, sampling and tables;
  * every file it writes equals direct Pillow calls (open, convert, rotate, resize, save) written out here;
  * the device leg's steps, run on the host models -- plan_job, the pixels a device image holds, jpeg_host.resample_lanczos, the
    encoder's host model, jpeg_host.sampled_file -- give the host leg's bytes, and the files it leaves to the host leg are the
    ones named here;
  * the size rule, the enumeration, the assertions, the command line.
"""

import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

import jpeg_enc_sampled_ref as E
import resize_scene as S
from conftest import GOLDEN


@pytest.fixture(scope='module')
def golden():
    return S.load_golden(os.path.join(GOLDEN, 'resize_reference.json'))


@pytest.fixture(scope='module')
def exact(golden, tmp_path_factory):
    """the byte pins hold for the recorded Pillow version and scene; everything else is asserted whatever the version"""
    folder = str(tmp_path_factory.mktemp('scene'))
    S.build(folder)
    return S.is_exact(golden, folder)


@pytest.fixture(scope='module', autouse=True)
def _built():
    import __graft_entry__ as G
    G.build()


@pytest.mark.parametrize('name', list(S.OPTION_SETS))
def test_host_leg_equals_the_reference(tmp_path, golden, exact, name):
    from megadetector_amd import resize_images as R
    counts = {}
    results, out = S.run_set(R.resize_image_folder, str(tmp_path), name, backend='host', counts=counts)
    want = golden['resize'][name]
    assert results == want['results']
    S.compare_tree(S.describe_tree(out), want['tree'], exact)
    statuses = [r['status'] for r in results]
    assert counts['files'] == len(results) and counts['skipped'] == statuses.count('skipped') and counts['errors'] == statuses.count('error')
    assert counts['resized'] + counts['unresized'] == statuses.count('success') and counts['gpu'] == 0
    assert counts['host'] == len(results) - counts['skipped']
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    if name == 'no_overwrite':
        assert statuses.count('skipped') == 2
        for rel, data in S.EXISTING.items():
            with open(os.path.join(out, rel), 'rb') as f:
                assert f.read() == data
    if name == 'no_target':
        assert counts['resized'] == 0
    if name == 'files_relative':
        assert [r['output_fn'] for r in results] == ['{OUT}/sub/com.jpg', '{OUT}/dusk420.jpg', '{OUT}/sub/rot8.jpg', '{OUT}/missing.jpg']


def pillow_file(path, target_width, target_height, quality):
    """what the reference's calls come to for one file, written out: -> the bytes, or None for a file that is not written"""
    ImageFile.LOAD_TRUNCATED_IMAGES = True
    try:
        image = Image.open(path)
        if image.mode not in ('RGBA', 'RGB', 'L', 'I;16'):
            return None
        if image.mode in ('RGBA', 'L'):
            image = image.convert(mode='RGB')
        orientation = (image._getexif() or {}).get(274) if hasattr(image, '_getexif') else None
        if orientation in (3, 6, 8):
            image = image.rotate({3: 180, 6: 270, 8: 90}[orientation], expand=True)
        image.load()
        w, h = image.size
        if target_width == -1 and target_height == -1:
            size = (w, h)
        elif target_height == -1:
            size = (target_width, int(target_width / (w / h)))
        elif target_width == -1:
            size = (int((w / h) * target_height), target_height)
        else:
            size = (target_width, target_height)
        if min(size) <= 0:
            return None
        if size != (w, h):
            image = image.resize(size, Image.Resampling.LANCZOS)
        bio = io.BytesIO()
        if image.format == 'JPEG':
            image.save(bio, 'JPEG', exif=image.getexif(), quality=quality)
        else:
            image.save(bio, 'JPEG' if path.lower().endswith('.jpg') else 'PNG', exif=image.getexif(), quality=85 if quality == 'keep' else quality)
        return bio.getvalue()
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = False


@pytest.mark.parametrize('name', ['width_64', 'height_30', 'no_target', 'width_64_quality_50', 'no_target_quality_50'])
def test_every_written_file_equals_direct_pillow_calls(tmp_path, name):
    from megadetector_amd import resize_images as R
    kw = S.OPTION_SETS[name]
    results, out = S.run_set(R.resize_image_folder, str(tmp_path), name, backend='host')
    source = str(tmp_path / 'in')
    written = 0
    for (rel, *_), r in zip(sorted(S.IMAGES), results):
        want = pillow_file(os.path.join(source, rel), kw.get('target_width', -1), kw.get('target_height', -1), kw.get('quality', 'keep'))
        assert (want is None) == (r['status'] == 'error'), rel
        if want is not None:
            with open(os.path.join(out, rel), 'rb') as f:
                assert f.read() == want, rel
            written += 1
    assert written >= 13


#: what the device leg leaves to the host leg whatever the options: the GPU's decoder takes neither the progressive file nor the
#: truncated one, the PNGs are no JPEGs (and 'palette.png' does not load at all)
HOST_FILES = {'sub/prog.jpg', 'pic.png', 'palette.png', 'truncated.jpg'}


def device_steps_on_the_host(path, output, settings):
    """the device leg's steps for one file with the host models in the kernels' places -> the file's bytes"""
    from megadetector_amd import jpeg_host, resize_images as R
    from megadetector_amd.feed import load_image
    job = {'input': path, 'output': output}
    R.plan_job(job, *settings)
    pixels = np.ascontiguousarray(np.asarray(load_image(path)))               # what mdhip_jpeg_reconstruct leaves on the device
    assert (pixels.shape[1], pixels.shape[0]) == job['source_size']
    if job['size'] != job['source_size']:
        pixels = jpeg_host.resample_lanczos(pixels, job['size'])
    coef = E.coefficients(pixels, job['sampling'], *job['quant'])
    rc, scans, _, _ = jpeg_host.encode_subsequences([coef], [job['size']], 64, samplings=[job['sampling']])
    assert rc == jpeg_host.MDJPEG_OK
    return jpeg_host.sampled_file(job['size'][0], job['size'][1], job['quant'][0], job['quant'][1], job['sampling'], scans[0], job['exif'],
                                  job['comment']), job


@pytest.mark.parametrize('name', ['width_64', 'width_200_enlarging', 'both_80', 'height_30', 'no_enlarge_200', 'equal_to_some', 'no_target',
                                  'width_64_quality_50', 'width_64_quality_95', 'no_target_quality_50'])
def test_device_leg_steps_on_the_host_models_give_the_host_leg_bytes(tmp_path, name):
    from megadetector_amd import jpeg_host, resize_images as R
    kw = S.OPTION_SETS[name]
    results, out = S.run_set(R.resize_image_folder, str(tmp_path), name, backend='host')
    source = str(tmp_path / 'in')
    settings = (kw.get('target_width', -1), kw.get('target_height', -1), kw.get('no_enlarge_width', False), kw.get('quality', 'keep'))
    to_host, resized, own_tables = set(), 0, 0
    for (rel, *_), r in zip(sorted(S.IMAGES), results):
        try:
            data, job = device_steps_on_the_host(os.path.join(source, rel), os.path.join(out, rel), settings)
        except Exception:
            to_host.add(rel)
            continue
        assert r['status'] == 'success'
        with open(os.path.join(out, rel), 'rb') as f:
            assert f.read() == data, rel
        resized += job['resized']
        standard = jpeg_host.quant_tables(85 if settings[3] == 'keep' else settings[3])
        own_tables += job['sampling'] != 2 or not all((a == b).all() for a, b in zip(job['quant'], standard))
    assert to_host == HOST_FILES | ({'thin.jpg'} if settings[0] == 64 else set())
    if name in ('no_target', 'no_target_quality_50'):
        assert resized == 0
    if name == 'no_target':
        assert own_tables >= 5                  # the plain RGB JPEGs keep their own tables and sampling
    if name == 'width_64':
        # 64 x 48 ('L', and the file with the ICC profile) and 64 x 96 (orientation 6) are that size already; of those the
        # plain RGB JPEG keeps its format and with it its own tables
        assert resized == 7 and own_tables == 1


def test_planning_refuses_what_the_host_leg_takes(tmp_path):
    from megadetector_amd import resize_images as R
    from megadetector_amd.preview import HostLeg
    files = S.build(str(tmp_path / 'in'))
    dusk = files[0]
    job = {'input': dusk, 'output': str(tmp_path / 'x.jpg')}
    R.plan_job(job, 64, -1, False, 'keep')
    assert job['size'] == (64, 47) and job['resized'] and job['sampling'] == 2 and 'data' not in job['probe']
    with pytest.raises(HostLeg, match='not a JPEG name'):
        R.plan_job({'input': dusk, 'output': str(tmp_path / 'x.png')}, 64, -1, False, 'keep')
    with pytest.raises(HostLeg, match='65535'):
        R.plan_job({'input': dusk, 'output': str(tmp_path / 'x.jpg')}, 70000, -1, False, 'keep')
    for quality in (0, 101, 'best', 50.0):
        with pytest.raises(HostLeg, match='quality'):
            R.plan_job({'input': dusk, 'output': str(tmp_path / 'x.jpg')}, 64, -1, False, quality)
    with pytest.raises(AssertionError, match='Invalid image resize target 64,0'):
        R.plan_job({'input': files[-1], 'output': str(tmp_path / 'x.jpg')}, 64, -1, False, 'keep')
    with pytest.raises(HostLeg, match='does not decode'):
        R.plan_job({'input': files[10], 'output': str(tmp_path / 'x.jpg')}, 64, -1, False, 'keep')


def test_size_rule():
    from megadetector_amd.resize_images import resize_target
    assert resize_target((163, 121), 64) == (64, 47, True)                  # int(64 / (163 / 121)) = int(47.5...)
    assert resize_target((163, 121), -1, 30) == (40, 30, True)
    assert resize_target((163, 121), None, None) == (-1, -1, False)
    assert resize_target((163, 121), 200, -1, True) == (200, 148, False)
    assert resize_target((163, 121), 163, 121) == (163, 121, False)
    assert resize_target((163, 121), 80, 80) == (80, 80, True)
    assert resize_target((300, 2), 64) == (64, 0, True)
    assert resize_target((3, 1000), 7) == (7, 2333, True)                   # 7 / 0.003 in floats
    for w, h, t in [(4000, 3000, 1600), (1920, 1080, 640), (97, 61, 33), (61, 97, 33)]:
        assert resize_target((w, h), t)[1] == int(t / (w / h)) and resize_target((w, h), -1, t)[0] == int((w / h) * t)


def test_assertions_and_enumeration(tmp_path):
    from megadetector_amd import resize_images as R
    source = str(tmp_path / 'in')
    S.build(source)
    open(os.path.join(source, 'notes.txt'), 'w').close()
    open(os.path.join(source, 'UPPER.JPG'), 'wb').close()
    os.makedirs(os.path.join(source, 'no_dot'))
    found = R.find_images(source, recursive=True)
    assert found == sorted([n for n, *_ in S.IMAGES] + ['UPPER.JPG'])
    assert R.find_images(source, recursive=False) == sorted([n for n, *_ in S.IMAGES if '/' not in n] + ['UPPER.JPG'])
    with pytest.raises(AssertionError, match='Illegal pool type'):
        R.resize_image_folder(source, str(tmp_path / 'o'), pool_type='fibre', backend='host')
    with pytest.raises(AssertionError, match='Illegal pool type'):
        R.resize_images({}, pool_type='fibre', backend='host')
    with pytest.raises(AssertionError, match='is not a folder'):
        R.resize_image_folder(source + '.none', backend='host')
    assert R.resize_images({}, backend='host') == []


def test_resize_image_returns_the_reference_objects(tmp_path):
    from megadetector_amd import resize_images as R
    files = S.build(str(tmp_path / 'in'))
    image = Image.open(files[2])
    assert R.resize_image(image) is image and R.resize_image(image, 97, 61) is image
    small = R.resize_image(image, target_height=30)
    assert small.size == (int((97 / 61) * 30), 30) and small.format is None
    out = str(tmp_path / 'o.jpg')
    assert R.resize_image(files[2], 40, output_file=out).size == (40, 25) and Image.open(out).size == (40, 25)
    with pytest.raises(AssertionError, match='Invalid image resize target 64,0'):
        R.resize_image(files[-1], 64)


def test_pools_give_the_serial_results(tmp_path):
    from megadetector_amd import resize_images as R
    source = str(tmp_path / 'in')
    S.build(source)
    trees = []
    for k, (pool_type, n) in enumerate([('thread', 1), ('thread', 3), ('process', 2)]):
        out = str(tmp_path / 'o{}'.format(k))
        results = R.resize_image_folder(source, out, target_width=64, pool_type=pool_type, n_workers=n, backend='host')
        trees.append(([(r['status'], r['error']) for r in results], {k: v['sha256'] for k, v in S.describe_tree(out).items()}))
    assert trees[0] == trees[1] == trees[2]


def test_command_line_runs_the_host_backend(tmp_path, golden, exact, capsys):
    from megadetector_amd import resize_images as R
    source, out = str(tmp_path / 'in'), str(tmp_path / 'out')
    S.build(source)
    assert R.main([source, out, '--target_width', '64', '--backend', 'host', '--n_workers', '1']) == 0
    S.compare_tree(S.describe_tree(out), golden['resize']['width_64']['tree'], exact)
    text = capsys.readouterr().out
    assert 'Invalid image resize target 64,0' in text and '15 files: 10 resized, 3 written unresized, 0 skipped, 2 errors (0 on the device, 15 on the host)' in text
    assert R.main([source, '--target_height', '30', '--quality', '50', '--no_recursive', '--no_overwrite', '--backend', 'host', '--n_workers', '1']) == 0
    assert '11 files: 0 resized, 0 written unresized, 11 skipped' in capsys.readouterr().out
