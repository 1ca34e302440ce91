"""Change detection on the GPU: mdhip_change_detect against its host model mdjpeg_change_detect, array for array, on the cases of
tests/test_change_cpu.py; the region stage alone (mdhip_label_regions_on) against scipy.ndimage.label on masks dilation never
makes; the tool's gpu leg against its host leg, CSV byte for CSV byte, over JPEG folders that span several decode chunks."""

import os

import numpy as np
import pytest

import change_ref as R
from test_change_cpu import STAGE_CASES, adversarial_masks, record_of, regions_of, stage_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from megadetector_amd.hip_backend import HipContext
    c = HipContext.for_images(0)
    yield c
    c.close()


def device_change_detect(ctx, images, pairs, record, blurred=None, want_masks=True):
    """jpeg_host.change_detect's interface on the device"""
    import torch
    dev = torch.device('cuda', 0)
    n = len(images)
    blurred = list(blurred) if blurred is not None else [None] * n
    keep, ptrs, sizes, planes, ready = [], [], [], [], []
    for i in range(n):
        if blurred[i] is not None:
            h, w = blurred[i].shape
            planes.append(torch.from_numpy(np.ascontiguousarray(blurred[i])).to(dev))
            ptrs.append(0), ready.append(1)
        else:
            h, w = images[i].shape[:2]
            keep.append(torch.from_numpy(np.ascontiguousarray(images[i])).to(dev))
            planes.append(torch.zeros((h, w), dtype=torch.uint8, device=dev))
            ptrs.append(keep[-1].data_ptr()), ready.append(0)
        sizes.append((w, h))
    masks = [torch.zeros((sizes[a][1], sizes[a][0]), dtype=torch.uint8, device=dev) for a, _ in pairs]
    res = ctx.change_detect(ptrs, sizes, [p.data_ptr() for p in planes], ready, pairs, record, [m.data_ptr() for m in masks] if want_masks else None)
    torch.cuda.synchronize()
    res = dict(res)
    res['blurred'] = [p.cpu().numpy() for p in planes]
    res['masks'] = [m.cpu().numpy() for m in masks]
    return res


def assert_same_results(got, want, cap_rows=True):
    for key in ('counts', 'hist', 'thresholds', 'n_regions', 'overflow'):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    for p in range(len(want['counts'])):
        assert regions_of(got, p)[:got['regions'].shape[1]] == regions_of(want, p)[:want['regions'].shape[1]]
        np.testing.assert_array_equal(got['masks'][p], want['masks'][p])
    for a, b in zip(got['blurred'], want['blurred']):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('h,w,kw', STAGE_CASES, ids=lambda v: None if isinstance(v, int) else '-'.join('{}{}'.format(k[:4], x) for k, x in v.items()))
def test_device_equals_the_host_model(ctx, h, w, kw):
    from megadetector_amd import jpeg_host
    kw = dict(kw)
    prev, curr = stage_pair(h, w, kw.pop('scene', None))
    rec = record_of(kw)
    want = jpeg_host.change_detect([prev, curr], [(0, 1)], rec, want_masks=True)
    assert_same_results(device_change_detect(ctx, [prev, curr], [(0, 1)], rec), want)


@pytest.mark.parametrize('threshold_type', ['global', 'otsu'])
def test_pairs_of_several_sizes_and_a_carried_plane_in_one_call(ctx, threshold_type):
    from megadetector_amd import jpeg_host
    a, b = stage_pair(150, 211)             # wider than the 64-pixel runs and the 256-pixel strips' remainder
    c, d = stage_pair(33, 80)
    e, f = stage_pair(300, 70)
    rec = record_of(dict(min_area=20, blur_kernel_size=9, threshold_type=threshold_type, dilate_kernel_size=3, dilate_iterations=3))
    pairs = [(0, 1), (2, 3), (1, 0), (4, 5)]
    want = jpeg_host.change_detect([a, b, c, d, e, f], pairs, rec, want_masks=True)
    assert_same_results(device_change_detect(ctx, [a, b, c, d, e, f], pairs, rec), want)
    carried = [want['blurred'][0], None, None, want['blurred'][3], None, None]
    got = device_change_detect(ctx, [None, b, c, None, e, f], pairs, rec, blurred=carried)
    assert_same_results(got, want)


def test_region_cap_on_the_device(ctx):
    from megadetector_amd import jpeg_host
    grid = np.zeros((21, 131, 3), np.uint8)
    grid[::2, ::2] = 255
    rec = record_of(dict(blur_kernel_size=1, dilate_iterations=0, min_area=0), cap=10)
    want = jpeg_host.change_detect([np.zeros_like(grid), grid], [(0, 1)], rec, want_masks=True)
    got = device_change_detect(ctx, [np.zeros_like(grid), grid], [(0, 1)], rec)
    assert got['overflow'][0] == 1 and got['n_regions'][0] == 11 * 66
    np.testing.assert_array_equal(got['regions'], want['regions'])
    assert_same_results(got, want)


def big_masks():
    """the adversarial shapes at 300 x 400 (wider and taller than a workgroup's 64 x 4 pixels many times over)"""
    return adversarial_masks(300, 400)


@pytest.mark.parametrize('size', ['37x70', '300x400'])
@pytest.mark.parametrize('name', sorted(adversarial_masks()))
def test_label_hook_equals_scipy(ctx, name, size):
    mask = (adversarial_masks() if size == '37x70' else big_masks())[name]
    want_labels, want_regions = R.regions(mask, 0)
    labels, n, regions, overflow = ctx.label_regions_on(mask * 7, min_area=0, cap=65536)
    np.testing.assert_array_equal(labels, want_labels)
    assert n == len(want_regions) and not overflow
    assert [tuple(int(v) for v in r) for r in regions] == want_regions
    # a min_area in the middle of the areas, and a cap below the count
    areas = sorted(r[4] for r in want_regions)
    if len(areas) > 2:
        cut = areas[len(areas) // 2]
        kept = [r for r in want_regions if r[4] > cut]
        _, n2, regions2, overflow2 = ctx.label_regions_on(mask, min_area=cut, cap=2)
        assert n2 == len(kept) and overflow2 == (len(kept) > 2)
        assert [tuple(int(v) for v in r) for r in regions2] == kept[:2]


# ---- the tool ---------------------------------------------------------------------------------------------------------------------

def jpeg_scene(root):
    """two cameras of six roughly 160 x 120 JPEGs: 4:2:0 and 4:4:4 sampling, one progressive file (PIL decodes it), one file
    that is no picture, one image of another size"""
    from PIL import Image
    rng = np.random.default_rng(11)
    folders = []
    for name, (h, w), sampling in (('cam_420', (120, 160), 2), ('cam_444', (118, 157), 0)):
        folder = os.path.join(root, name)
        os.makedirs(folder)
        for k, frame in enumerate(R.camera_frames(h, w, 6, 5 if sampling else 6)):
            frame = np.clip(frame.astype(int) + rng.integers(-6, 7, frame.shape), 0, 255).astype(np.uint8)      # sensor noise
            path = os.path.join(folder, 'img_{:03d}.jpg'.format(k))
            if name == 'cam_420' and k == 3:
                with open(path, 'wb') as f:
                    f.write(b'\xff\xd8 no picture')
            elif name == 'cam_444' and k == 4:
                Image.fromarray(frame[:90, :100]).save(path, quality=90, subsampling=sampling)
            else:
                Image.fromarray(frame).save(path, quality=90, subsampling=sampling, progressive=(name == 'cam_444' and k == 1))
        folders.append(folder)
    return folders


@pytest.fixture(scope='module')
def jpeg_folders(tmp_path_factory):
    return jpeg_scene(str(tmp_path_factory.mktemp('change_jpeg')))


@pytest.mark.parametrize('kw', [dict(min_area=40), dict(min_area=40, threshold_type='OTSU', ignore_fraction=-0.2, blur_kernel_size=7)],
                         ids=['global', 'otsu'])
def test_tool_gpu_leg_equals_host_leg(jpeg_folders, tmp_path, monkeypatch, kw):
    from megadetector_amd import change_detection as CD
    from megadetector_amd import device_render
    monkeypatch.setattr(device_render, 'DECODE_CHUNK_BYTES', 130000)          # two images a chunk: a camera spans three chunks
    kw = dict(kw, workers=1)
    if 'threshold_type' in kw:
        kw['threshold_type'] = getattr(CD.ThresholdType, kw['threshold_type'])
    options = CD.ChangeDetectionOptions(**kw)
    host_csv, gpu_csv = str(tmp_path / 'host.csv'), str(tmp_path / 'gpu.csv')
    host_rows, _ = CD.process_folders(jpeg_folders, options, host_csv, backend='host')
    profile = {}
    gpu_rows, counts = CD.process_folders(jpeg_folders, options, gpu_csv, backend='gpu', profile=profile)
    assert gpu_rows == host_rows
    with open(host_csv, 'rb') as f, open(gpu_csv, 'rb') as g:
        assert f.read() == g.read()
    assert sum(r['motion_detected'] for r in host_rows) >= 4
    # 10 pairs: two have the file that is no picture, two the image of another size
    assert counts == {'gpu_pairs': 6, 'host_pairs': 0, 'pil_decodes': 1}
    assert profile['change_detect'] > 0 and profile['decode'] > 0
    a, b = os.path.join(jpeg_folders[0], 'img_000.jpg'), os.path.join(jpeg_folders[0], 'img_001.jpg')
    assert CD.detect_motion(a, b, options, backend='gpu') == CD.detect_motion(a, b, options, backend='host')


def test_a_pair_over_the_region_cap_goes_to_the_host_model(tmp_path):
    from PIL import Image
    from megadetector_amd import change_detection as CD
    folder = str(tmp_path / 'dots')
    os.makedirs(folder)
    dots = np.zeros((64, 96, 3), np.uint8)
    dots[::2, ::2] = 255                                                       # 32 x 48 single pixels: six times the cap
    for k, frame in enumerate((np.zeros_like(dots), dots, np.zeros_like(dots))):
        Image.fromarray(frame).save(os.path.join(folder, 'img_{}.png'.format(k)))
    Image.fromarray(R.planted(np.zeros_like(dots), [(5, 5, 9, 9, (255, 255, 255))])).save(os.path.join(folder, 'img_3.png'))
    options = CD.ChangeDetectionOptions(min_area=0, dilate_iterations=0, blur_kernel_size=1, workers=1)
    assert 32 * 48 > CD.REGION_CAP
    host_rows, _ = CD.process_folders([folder], options, backend='host')
    gpu_rows, counts = CD.process_folders([folder], options, backend='gpu')
    assert gpu_rows == host_rows
    assert [r['num_regions'] for r in gpu_rows] == [0, 32 * 48, 32 * 48, 1]
    assert counts == {'gpu_pairs': 1, 'host_pairs': 2, 'pil_decodes': 4}
