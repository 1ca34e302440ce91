"""
The three written products of run_detector_batch together -- crop_folder, blur_folder and preview_folder in one run -- against
the runs with each folder alone: the same trees byte for byte, the same counts, and results that carry none of the products.
With CroppingStub the detector makes the crops (crops=) and the driver makes the other two, so the per-product keyword filter
is exercised.  The folder and the stubs are those of test_crops_cpu.py.
"""

import pytest

from megadetector_amd import run_detector_batch as RDB
from stub_detector import StubDetector
from test_crops_cpu import CroppingStub, _folder, _tree

MODES = {'one_by_one': {}, 'batched': {'batch_size': 4}, 'queue': {'batch_size': 4, 'use_image_queue': True, 'loader_workers': 2}}
COUNTS = {'crop': 'last_crop_counts', 'blur': 'last_blur_counts', 'preview': 'last_preview_counts'}


def _by_file(results):
    return sorted(results, key=lambda r: r['file'])              # (the image queue hands results on as they come)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('stub', [StubDetector, CroppingStub])
def test_three_folders_in_one_run_equal_the_runs_with_each_alone(tmp_path, stub, mode):
    folder, files = _folder(tmp_path)
    run = lambda **kw: RDB.load_and_run_detector_batch('stub', files, detector=stub(), quiet=True, confidence_threshold=0.05,
                                                       **dict(MODES[mode], **kw))
    options = {
        'crop': lambda out: dict(crop_folder=out, crop_base=folder),
        'blur': lambda out: dict(blur_folder=out, blur_base=folder, blur_categories=('animal', 'person', 'vehicle'),
                                 blur_confidence_threshold=0.0),
        'preview': lambda out: dict(preview_folder=out, preview_base=folder, preview_width=200, preview_preserve_paths=True)}
    plain = run()
    assert len(plain) == len(files) and not any(k in r for r in plain for k in ('crops', 'blurred', 'preview'))
    alone = {}
    for product, kw in options.items():
        out = str(tmp_path / (product + '_alone'))
        assert _by_file(run(**kw(out))) == _by_file(plain)
        alone[product] = (_tree(out), dict(getattr(RDB, COUNTS[product])))
    together = {}
    for product, kw in options.items():
        together.update(kw(str(tmp_path / (product + '_together'))))
    got = run(**together)
    assert not any(k in r for r in got for k in ('crops', 'blurred', 'preview'))
    assert _by_file(got) == _by_file(plain)
    for product, (tree, counts) in alone.items():
        assert len(tree) >= 1 and any(n.endswith('.png') for n in tree) and any(n.startswith('sub/') for n in tree), (product, sorted(tree))
        assert counts['files'] == len(tree)
        assert _tree(str(tmp_path / (product + '_together'))) == tree, product
        assert getattr(RDB, COUNTS[product]) == counts, product
    # who made the crops: the detector with crops= (counted as 'gpu'), the driver otherwise; the other two always the driver
    crop_counts = alone['crop'][1]
    assert (crop_counts['gpu'] > 0, crop_counts['host_jpeg'] > 0) == ((True, False) if stub is CroppingStub else (False, True))
    assert alone['blur'][1]['gpu'] == 0 and alone['preview'][1]['gpu'] == 0
