"""
Times change detection on generated camera folders, in one process: the tool's gpu leg (mdhip_change_detect, files decoded on
the device) against its host leg (mdjpeg_change_detect, files decoded by PIL) on one thread and on a pool of 16, all three warmed
and alternating.  The folders hold 3-megapixel JPEGs of a static, slightly noisy scene with an object planted on some frames.
Asserts that the three legs write the same CSV text; prints images per second of each leg and, from one extra profiled run of
the gpu leg, the waited-for milliseconds per kind of device call.  The baseline is the host leg: the parent commit has no such
tool, and the reference's own speed cannot be measured without OpenCV.  `--out FILE` also writes what is printed.

usage: python tools/change_bench.py [--cameras 4] [--per_camera 12] [--width 2048 --height 1536] [--rounds 3] [--out profiles/change_detection.txt]
"""

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def generate(root, cameras, per_camera, width, height, seed=1):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    folders = []
    for c in range(cameras):
        folder = os.path.join(root, 'cam{:02d}'.format(c))
        os.makedirs(folder)
        base = np.stack([60 + 120 * xx // width + 20 * c, 180 - 100 * yy // height, 40 + (xx // 16 + yy // 16) % 48], -1).astype(np.int16)
        for k in range(per_camera):
            frame = base + rng.integers(-4, 5, base.shape, dtype=np.int16)
            if k % 3 == 1:                                      # an object on every third frame, somewhere else each time
                w, h = int(rng.integers(width // 12, width // 5)), int(rng.integers(height // 12, height // 5))
                x, y = int(rng.integers(0, width - w)), int(rng.integers(0, height - h))
                frame[y:y + h, x:x + w] = rng.integers(0, 256, 3)
            Image.fromarray(np.clip(frame, 0, 255).astype(np.uint8)).save(os.path.join(folder, 'IMG_{:04d}.JPG'.format(k)), quality=90)
        folders.append(folder)
    return folders


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cameras', type=int, default=16)
    ap.add_argument('--per_camera', type=int, default=4)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--height', type=int, default=1536)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pool', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from megadetector_amd import change_detection as CD

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as root:
        folders = generate(root, args.cameras, args.per_camera, args.width, args.height)
        n_images = args.cameras * args.per_camera
        legs = {'gpu': dict(backend='gpu', workers=1), 'host x1': dict(backend='host', workers=1),
                'host x{}'.format(args.pool): dict(backend='host', workers=args.pool)}
        texts, times, counts = {}, {k: [] for k in legs}, {}

        def run(name, profile=None):
            leg = legs[name]
            options = CD.ChangeDetectionOptions(workers=leg['workers'])
            stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
            try:
                t0 = time.perf_counter()
                rows, counts[name] = CD.process_folders(folders, options, None, backend=leg['backend'], profile=profile)
                dt = time.perf_counter() - t0
            finally:
                sys.stdout.close()
                sys.stdout = stdout
            texts[name] = CD.csv_text(rows)
            print('    ran {}: {:.3f} s'.format(name, dt), file=sys.stderr, flush=True)
            return dt, rows

        for name in legs:                                       # warm: libraries, device context, page cache
            run(name)
        for _ in range(args.rounds):
            for name in legs:
                times[name].append(run(name)[0])
        _, rows = run('gpu')
        profile = {}
        run('gpu', profile)
        assert texts['gpu'] == texts['host x1'] == texts['host x{}'.format(args.pool)], 'the legs disagree'
        say('change detection, {} cameras x {} JPEGs of {} x {} ({:.1f} MP), default options; {} rows, {} with motion; equal CSV text in all legs'
            .format(args.cameras, args.per_camera, args.width, args.height, args.width * args.height / 1e6, len(rows),
                    sum(r['motion_detected'] for r in rows)))
        for name in legs:
            med = statistics.median(times[name])
            say('  {:<9} {:8.1f} images/s   (median of {}: {:.3f} s; all: {})'.format(
                name, n_images / med, args.rounds, med, ' '.join('{:.3f}'.format(t) for t in times[name])))
        say('  gpu leg counts: {}'.format(counts['gpu']))
        say('  gpu leg, one profiled run, waited-for ms per kind of device call: ' +
            ', '.join('{} {:.1f}'.format(k, v) for k, v in sorted(profile.items())))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
