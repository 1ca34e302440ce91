"""
The scene of the video rendering tests: one results file of six videos (and one still image, which the tool must filter out)
and the option sets the reference's visualize_video_output was run with (tests/golden/gen_video_render_reference.py), and the
small Motion-JPEG AVI files the frame tests render, muxed at run time with tests/avi_fixtures.py.
"""

import json
import os

import avi_fixtures as A

DETECTION_CATEGORIES = {'1': 'animal', '2': 'person', '3': 'vehicle'}
CLASSIFICATION_CATEGORIES = {'0': 'Deer', '1': 'Red Fox', '2': 'bird/other'}


def _det(frame, category, conf, bbox, classifications=None):
    d = {'category': category, 'conf': conf, 'bbox': bbox, 'frame_number': frame}
    if classifications is not None:
        d['classifications'] = classifications
    return d


#: 'missing.avi' is never written; 'a/failed.avi' failed in the detector's run
VIDEOS = [
    {'file': 'a/one.avi', 'frame_rate': 30.0, 'frames_processed': [0, 2, 4, 6, 8, 10], 'detections': [
        _det(2, '1', 0.91, [0.1, 0.2, 0.4, 0.5]), _det(2, '2', 0.45, [0.5, 0.1, 0.3, 0.6]), _det(4, '1', 0.12, [0.2, 0.2, 0.3, 0.3]),
        _det(6, '3', 0.6, [0.0, 0.0, 0.5, 0.5]), _det(8, '1', 0.05, [0.3, 0.3, 0.3, 0.3])]},
    {'file': 'a/failed.avi', 'frame_rate': -1.0, 'frames_processed': [], 'failure': 'Failure processing video: no frames', 'detections': None},
    {'file': 'b/empty.avi', 'frame_rate': 25.0, 'frames_processed': [0, 5, 10], 'detections': []},
    {'file': 'b/c/deer.avi', 'frame_rate': 24.0, 'frames_processed': [0, 3, 6, 9], 'detections': [
        _det(3, '1', 0.8, [0.2, 0.3, 0.4, 0.4], [['0', 0.9], ['1', 0.35]]), _det(6, '1', 0.7, [0.25, 0.3, 0.4, 0.4], [['0', 0.85]]),
        _det(6, '2', 0.3, [0.6, 0.1, 0.3, 0.5])]},
    {'file': 'two.mp4', 'frame_rate': 29.97, 'frames_processed': [0, 10, 20, 30, 40], 'detections': [
        _det(10, '1', 0.5, [0.1, 0.1, 0.5, 0.5], [['0', 0.6], ['1', 0.55], ['2', 0.2]]), _det(30, '1', 0.1, [0.1, 0.1, 0.2, 0.2])]},
    {'file': 'missing.avi', 'frame_rate': 30.0, 'frames_processed': [0, 1], 'detections': [_det(0, '1', 0.9, [0.1, 0.1, 0.5, 0.5])]},
]
ON_DISK = [v['file'] for v in VIDEOS if v['file'] != 'missing.avi']

RESULTS = {'info': {'format_version': '1.5', 'detector': 'stub'}, 'detection_categories': DETECTION_CATEGORIES,
           'classification_categories': CLASSIFICATION_CATEGORIES,
           'images': VIDEOS[:2] + [{'file': 'still/image.jpg', 'detections': []}] + VIDEOS[2:]}

#: name -> attributes set on VideoVisualizationOptions (everything else: the defaults)
OPTION_SETS = {
    'default': {},
    'threshold_050': {'confidence_threshold': 0.5},
    'trim': {'trim_to_detections': True},
    'fs_12': {'rendering_fs': 12},
    'fs_speedup_2': {'rendering_fs': -2},
    'fs_string': {'rendering_fs': '7.5'},
    'flatten': {'flatten_output': True},
    'flatten_extension': {'flatten_output': True, 'path_separator_replacement': '~', 'output_extension': 'avi'},
    'extension_dot': {'output_extension': '.mjpeg.avi'},
    'exclude_strings': {'exclude_category_name_strings': ['none', 'deer_red fox']},
    'exclude_string_one': {'exclude_category_name_strings': 'deer'},
    'exclude_names': {'exclude_category_names': ['red fox']},
    'include_names': {'include_category_names': ['deer'], 'classification_confidence_threshold': 0.8},
    'include_no_match': {'include_category_names': 'bird', 'classification_confidence_threshold': 0.58},
    'names_start': {'include_category_names_in_filenames': 'start'},
    'names_end': {'include_category_names_in_filenames': 'end', 'classification_confidence_threshold': 0.3},
    'min_length': {'min_output_length_seconds': 0.3},
    'sample_3': {'sample': 3, 'random_seed': 7},
}


def apply_options(options, attributes):
    for k, v in attributes.items():
        assert hasattr(options, k), k
        setattr(options, k, v)
    options.parallelize_rendering = False
    return options


def build(folder, touch=True):
    """writes the results file and, with touch, an empty file for every video that is on disk.  -> (video folder, results file)"""
    video_dir = os.path.join(folder, 'videos')
    for rel in ON_DISK:
        path = os.path.join(video_dir, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if touch:
            open(path, 'wb').close()
    results_file = os.path.join(folder, 'results.json')
    with open(results_file, 'w') as f:
        json.dump(RESULTS, f)
    return video_dir, results_file


# ---- small videos for the frame tests ----------------------------------------------------------------------------------------------
N_FRAMES = 6


def progressive(arr, sampling='420'):
    return A.jpeg_bytes(arr, sampling, progressive=True)


def small_video(path, size, sampling, seed, implied_tables=False, dropped=None, progressive_frame=None, rate=30):
    """a six-frame MJPG AVI of `size`: block noise, Pillow's quality 85; implied_tables: the frames carry no DHT segment;
    dropped: this frame is a 0-byte chunk; progressive_frame: this frame is a progressive JPEG.  -> the stored chunks"""
    w, h = size
    frames = []
    for i in range(N_FRAMES):
        arr = A.block_noise(w, h, seed * 100 + i)
        data = progressive(arr, sampling) if i == progressive_frame else A.jpeg_bytes(arr, sampling)
        if implied_tables and i != progressive_frame:
            data = A.strip_dht(data)
        frames.append(b'' if i == dropped else data)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    A.write_avi(path, frames, size, rate=rate)
    return frames


#: file -> keyword arguments of small_video
SMALL_VIDEOS = {
    'v444.avi': dict(size=(64, 48), sampling='444', seed=1),
    'v422.avi': dict(size=(70, 50), sampling='422', seed=2, implied_tables=True),
    'sub/v420.avi': dict(size=(70, 50), sampling='420', seed=3, dropped=3),
    'sub/prog.avi': dict(size=(64, 48), sampling='420', seed=4, progressive_frame=2),
}


def small_results(classified=False, thin=False):
    """a results file over SMALL_VIDEOS, every frame processed: boxes (animal, person) on frames 1, 2 and 4, a person alone on
    frame 5, nothing on frames 0 and 3; classified: the animals carry classifications; thin: frame 4 of v444.avi also gets a
    box thinner than its outline"""
    images = []
    for name in SMALL_VIDEOS:
        cls = [['0', 0.9], ['1', 0.55], ['2', 0.1]] if classified else None
        dets = [_det(1, '1', 0.9, [0.1, 0.15, 0.5, 0.6], cls), _det(1, '2', 0.5, [0.55, 0.3, 0.4, 0.6]),
                _det(2, '1', 0.7, [0.0, 0.0, 0.6, 0.7], cls), _det(2, '1', 0.1, [0.2, 0.2, 0.2, 0.2]),
                _det(4, '2', 0.8, [0.3, 0.2, 0.45, 0.7]), _det(4, '1', 0.4, [0.05, 0.4, 0.5, 0.55], [['1', 0.45]] if classified else None),
                _det(5, '2', 0.6, [0.4, 0.1, 0.5, 0.8])]
        if thin and name == 'v444.avi':
            dets.append(_det(4, '3', 0.9, [0.5, 0.5, 0.05, 0.5]))
        images.append({'file': name, 'frame_rate': 30.0, 'frames_processed': list(range(N_FRAMES)), 'detections': dets})
    return {'info': {'format_version': '1.5'}, 'detection_categories': DETECTION_CATEGORIES,
            'classification_categories': CLASSIFICATION_CATEGORIES, 'images': images}


def build_small(folder, **kw):
    """-> (video folder, results file, {file: stored chunks})"""
    video_dir = os.path.join(folder, 'videos')
    stored = {name: small_video(os.path.join(video_dir, name), **args) for name, args in SMALL_VIDEOS.items()}
    results_file = os.path.join(folder, 'results.json')
    with open(results_file, 'w') as f:
        json.dump(small_results(**kw), f)
    return video_dir, results_file, stored
