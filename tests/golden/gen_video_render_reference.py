"""
Generates tests/golden/video_render_reference.json by running the reference's own visualize_video_output
(visualization/visualize_video_output.py, read-only) on the results file of tests/video_render_scene.py, once per option set.
The reference cannot travel to the GPU machine, so what it decides is recorded as a fixture together with this script;
tests/test_video_render_cpu.py asserts that megadetector_amd.visualize_video_output reproduces it.

The reference reads and writes video with OpenCV, which is not installed here, so its module is imported with a stand-in
`cv2` in sys.modules -- cvtColor reverses the channels, VideoWriter records path, frame rate, size and the number of frames
written -- and its run_callback_on_frames is replaced by a function that feeds one generated numpy frame per requested frame
number to the callback.  Its render_detection_bounding_boxes is wrapped, so that the detections it is handed are recorded per
frame.  Its _process_video is wrapped too: where it raises (it formats a variable that was never bound when
include_category_names meets a video without classification names), the exception's type is recorded as that video's result.

Recorded per option set, per video in the order of the results returned: the result dict, and for a video that was written
its output path relative to the output folder, its frame rate and size, the frame numbers requested and the detections handed
to the renderer for each (an empty list: the renderer was not called).

Run:  python tests/golden/gen_video_render_reference.py /path/to/reference
"""

import io
import json
import os
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import video_render_scene as S  # noqa: E402

WRITERS = []


class _Writer:
    def __init__(self, path, fourcc, fps, size):
        self.path, self.fourcc, self.fps, self.size, self.frames = path, fourcc, fps, size, 0
        WRITERS.append(self)

    def isOpened(self):
        return True

    def write(self, frame):
        self.frames += 1

    def release(self):
        pass


def stand_in_cv2():
    cv2 = types.ModuleType('cv2')
    cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR = 4, 4
    cv2.cvtColor = lambda array, code: np.ascontiguousarray(array[:, :, ::-1])
    cv2.VideoWriter_fourcc = lambda *chars: ''.join(chars)
    cv2.VideoWriter = _Writer
    cv2.__getattr__ = lambda name: 0
    return cv2


def import_reference(root):
    sys.path.insert(0, root)
    sys.modules['cv2'] = stand_in_cv2()
    sys.modules.setdefault('jsonpickle', types.ModuleType('jsonpickle'))
    hf = types.ModuleType('humanfriendly')
    hf.format_timespan = lambda s: '{:.2f} seconds'.format(s)
    sys.modules.setdefault('humanfriendly', hf)
    from megadetector.visualization import visualize_video_output as ref
    return ref


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    state = {}

    def run_callback_on_frames(input_video_file, frame_callback, frames_to_process=None, verbose=False):
        state['requested'] = list(frames_to_process)
        state['handed'] = []
        for n in frames_to_process:
            state['handed'].append([])
            frame_callback(np.full((48, 64, 3), n % 251, dtype=np.uint8), 'frame{:06d}.jpg'.format(n))

    def render(detections, image, label_map, classification_label_map, classification_confidence_threshold):
        state['handed'][-1] = json.loads(json.dumps(detections))
        state['maps'] = [label_map, classification_label_map, classification_confidence_threshold]

    process_video = ref._process_video

    def recorded(video_entry, *args, **kwargs):
        state.clear()
        del WRITERS[:]
        try:
            result = process_video(video_entry, *args, **kwargs)
        except Exception as e:
            result = {'file': video_entry['file'], 'success': False, 'error': 'raised', 'frames_processed': 0, 'raises': type(e).__name__}
        record = {'result': result}
        if WRITERS:
            w = WRITERS[0]
            record.update(output=os.path.relpath(w.path, state_out[0]).replace(os.sep, '/'), fps=w.fps, size=list(w.size), fourcc=w.fourcc,
                          frames_written=w.frames, frames=state['requested'], detections=state['handed'])
        records.append(record)
        return result

    ref.run_callback_on_frames = run_callback_on_frames
    ref.render_detection_bounding_boxes = render
    ref._process_video = recorded
    golden = {'note': 'written by tests/golden/gen_video_render_reference.py from the reference module itself', 'results': S.RESULTS,
              'sets': {}}
    state_out = [None]
    for name, attributes in S.OPTION_SETS.items():
        with tempfile.TemporaryDirectory() as tmp:
            video_dir, results_file = S.build(tmp)
            state_out[0] = os.path.join(tmp, 'out')
            records = []
            options = S.apply_options(ref.VideoVisualizationOptions(), attributes)
            options.fourcc = 'MJPG'
            with redirect_stdout(io.StringIO()):
                ref.visualize_video_output(results_file, state_out[0], video_dir, options)
            for r in records:
                if r['result'].get('error'):
                    r['result']['error'] = r['result']['error'].replace(tmp, '<tmp>')
            golden['sets'][name] = records
    path = os.path.join(REPO, 'tests', 'golden', 'video_render_reference.json')
    with open(path, 'w') as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote {} ({} option sets)'.format(path, len(golden['sets'])))


if __name__ == '__main__':
    main()
