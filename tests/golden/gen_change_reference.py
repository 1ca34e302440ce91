"""Writes tests/golden/change_reference.json from the reference's own detection/change_detection.py.

    python tests/golden/gen_change_reference.py REFERENCE_ROOT

The reference module is imported with a stand-in `cv2` (tests/change_ref.py standin_cv2: this project's definitions of the
numeric steps, contourArea as pixel count, findContours in label order), so what the fixture pins is everything that is NOT
arithmetic: the image list and its order, the first image's row, the pair loop, the unreadable-image rule, the region strings,
the columns, the text DataFrame.to_csv(index=False) writes, and which rows create_change_previews samples.  Needs pandas and
tqdm, which the reference imports.  Paths are stored with the scene's root replaced by {ROOT}."""

import json
import os
import random
import sys
import tempfile
import types

OPTIONAL_IMPORTS = ('jsonpickle',)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import change_ref  # noqa: E402


def main(reference_root):
    sys.modules['cv2'] = change_ref.standin_cv2()
    for name in OPTIONAL_IMPORTS:                   # imported by the reference's utility modules, called by nothing used here
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, reference_root)
    from megadetector.detection import change_detection as ref
    out = {'option_sets': change_ref.REFERENCE_OPTION_SETS, 'runs': []}
    with tempfile.TemporaryDirectory() as root:
        root = os.path.realpath(root)
        folders = change_ref.build_reference_scene(root)
        for kwargs in change_ref.REFERENCE_OPTION_SETS:
            kw = dict(kwargs, workers=1)
            if 'threshold_type' in kw:
                kw['threshold_type'] = getattr(ref.ThresholdType, kw['threshold_type'])
            csv_path = os.path.join(root, 'out.csv')
            frame = ref.process_folders(folders, ref.ChangeDetectionOptions(**kw), csv_path)
            with open(csv_path, newline='') as f:
                text = f.read()
            os.remove(csv_path)
            rows = [{k: (v.item() if hasattr(v, 'item') else v) for k, v in r.items()} for r in frame.to_dict(orient='records')]
            # which rows the previews sample: the reference's own filter and random calls, the drawing stubbed out
            sampled = {}
            for seed, num in ((0, 2), (7, 10), (3, None)):
                paths = ref.create_change_previews(frame, os.path.join(root, 'previews'), num_samples=num, random_seed=seed)
                sampled['{},{}'.format(seed, num)] = [os.path.basename(p) for p in paths]
            out['runs'].append({'rows': json.loads(json.dumps(rows).replace(root, '{ROOT}')), 'csv': text.replace(root, '{ROOT}'),
                                'sampled': sampled})
        empty = ref.process_folders([os.path.join(root, 'cam_empty')], ref.ChangeDetectionOptions(workers=1), os.path.join(root, 'e.csv'))
        assert len(empty) == 0
        with open(os.path.join(root, 'e.csv'), newline='') as f:
            out['empty_csv'] = f.read()
    with open(os.path.join(HERE, 'change_reference.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', len(out['runs']), 'runs')


if __name__ == '__main__':
    main(sys.argv[1])
