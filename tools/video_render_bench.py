"""
Rendering detections into Motion-JPEG videos, device leg against host leg: frames per second of visualize_video_output over
one generated file.

    python tools/video_render_bench.py [--frames 1536] [--size 1280x720] [--rounds 3] [--pool 16] [--out FILE]

Generates a 4:2:2 quality-85 MJPEG AVI as tools/video_bench.py does, split into `--pool` files so that the host leg's pool has
a video per worker, and a results file in which every frame is processed and every second processed frame carries three boxes
(an animal, a person, a vehicle).  Per mode -- quality 'keep', 'keep' with keep_source_blocks, quality 75 -- both legs are
warmed once and then alternated in one process for `--rounds` rounds: backend='gpu', backend='host' with one thread, and
backend='host' with a pool of `--pool` threads.  The output files of the legs are compared in every round (the run stops where
they differ).  Then one more device run per mode with the device waited for around each kind of call, for the milliseconds
that go into decode, blur, draw and encode.  A chunk of the device leg holds 256 MiB of decoded pixels (97 frames of this size;
with keep_source_blocks the coefficient planes count too: 41 frames), so the modes differ in their number of chunks.  The
parent of this tool cannot be measured: the baseline is the host leg.
"""

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

MODES = [('keep', dict(quality='keep')), ('keep+blocks', dict(quality='keep', keep_source_blocks=True)), ('q75', dict(quality=75))]
BOXES = [('1', 0.91, [0.10, 0.20, 0.30, 0.40]), ('2', 0.80, [0.55, 0.15, 0.20, 0.60]), ('3', 0.60, [0.30, 0.65, 0.35, 0.25])]


def make_scene(folder, n_frames, width, height, n_files):
    from video_bench import make_video
    video_dir = os.path.join(folder, 'videos')
    os.makedirs(video_dir)
    per_file = n_frames // n_files
    images, mean_bytes = [], 0.0
    for k in range(n_files):
        name = 'clip_{:02d}.avi'.format(k)
        mean_bytes = make_video(os.path.join(video_dir, name), per_file, width, height)
        dets = [{'category': c, 'conf': conf, 'bbox': bbox, 'frame_number': i} for i in range(0, per_file, 2) for c, conf, bbox in BOXES]
        images.append({'file': name, 'frame_rate': 30.0, 'frames_processed': list(range(per_file)), 'detections': dets})
    results_file = os.path.join(folder, 'results.json')
    with open(results_file, 'w') as f:
        json.dump({'info': {'format_version': '1.5'}, 'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'},
                   'images': images}, f)
    return video_dir, results_file, per_file * n_files, mean_bytes


def tree(folder):
    """name -> SHA-256 of every file of the folder, which is then removed (a round writes hundreds of megabytes)"""
    import hashlib
    import shutil
    out = {}
    for name in sorted(os.listdir(folder)):
        with open(os.path.join(folder, name), 'rb') as f:
            out[name] = hashlib.sha256(f.read()).hexdigest()
    shutil.rmtree(folder)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1536, help='in all files together: enough for a timed window of about a second on the device leg')
    ap.add_argument('--size', default='1280x720')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pool', type=int, default=16)
    ap.add_argument('--blur', action='store_true', help='also blur the people')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    assert args.rounds >= 3, 'at least three rounds'
    width, height = (int(v) for v in args.size.split('x'))
    from megadetector_amd import visualize_video_output as V
    from megadetector_amd.hip_backend import HipContext
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def run(leg, mode, out_dir, profile=None):
        options = V.VideoVisualizationOptions()
        for k, v in dict(MODES)[mode].items():
            setattr(options, k, v)
        if args.blur:
            options.blur_category_names = 'person'
        backend = 'gpu' if leg == 'gpu' else 'host'
        options.parallelize_rendering = leg == 'host_pool'
        options.parallelize_rendering_n_cores = args.pool
        real = sys.stdout
        sys.stdout = open(os.devnull, 'w')
        try:
            t0 = time.perf_counter()
            results = V.visualize_video_output(results_file, out_dir, video_dir, options, backend=backend, ctx=ctx if backend == 'gpu' else None,
                                               profile=profile)
            el = time.perf_counter() - t0
        finally:
            sys.stdout.close()
            sys.stdout = real
        assert all(r['success'] for r in results), [r['error'] for r in results if not r['success']]
        return el, results

    with tempfile.TemporaryDirectory() as tmp:
        video_dir, results_file, n, mean_bytes = make_scene(tmp, args.frames, width, height, args.pool)
        say('videos: {} files, {} frames {}x{} 4:2:2 quality 85 MJPEG AVI, no DHT, {:.0f} bytes / frame; three boxes on every second '
            'frame{}'.format(args.pool, n, width, height, mean_bytes, ', people blurred' if args.blur else ''))
        ctx = HipContext.for_images(0)
        legs = ('gpu', 'host_1', 'host_pool')
        summary = {}
        try:
            for mode, _ in MODES:
                rates = {leg: [] for leg in legs}
                for rnd in range(args.rounds + 1):                # round 0 warms every leg up and is not counted
                    trees = {}
                    for leg in legs:
                        out_dir = os.path.join(tmp, 'out_{}_{}_{}'.format(mode, leg, rnd))
                        el, results = run(leg, mode, out_dir)
                        trees[leg] = tree(out_dir)
                        if rnd:
                            rates[leg].append(n / el)
                    assert trees['gpu'] == trees['host_1'] == trees['host_pool'], 'round {} of {}: the legs wrote different files'.format(rnd, mode)
                    if rnd:
                        say('  {} round {}: gpu {:.1f}, host (1 thread) {:.1f}, host ({} threads) {:.1f} frames/s; files equal'.format(
                            mode, rnd, rates['gpu'][-1], rates['host_1'][-1], args.pool, rates['host_pool'][-1]))
                profile = {'ms': {}}
                _, results = run('gpu', mode, os.path.join(tmp, 'out_{}_profile'.format(mode)), profile)
                tree(os.path.join(tmp, 'out_{}_profile'.format(mode)))
                counts = {k: sum(r[k] for r in results) for k in ('frames_copied', 'frames_rendered', 'frames_host')}
                summary[mode] = {'frames_per_s': {leg: float(np.median(rates[leg])) for leg in legs}, 'ms': profile['ms'],
                                 'calls': {k: v for k, v in profile.items() if k != 'ms'}, **counts}
                say('{}: median gpu {:.1f}, host (1 thread) {:.1f}, host ({} threads) {:.1f} frames/s; {}; device calls {} waited for: {}'.format(
                    mode, *(summary[mode]['frames_per_s'][leg] for leg in ('gpu', 'host_1')), args.pool,
                    summary[mode]['frames_per_s']['host_pool'], counts, summary[mode]['calls'],
                    ', '.join('{} {:.1f} ms'.format(k, v) for k, v in profile['ms'].items())))
        finally:
            ctx.close()
        say(json.dumps(summary))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
