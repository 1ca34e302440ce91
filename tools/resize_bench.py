"""
Times resize_image_folder over a generated folder of 3-megapixel 4:2:2 quality-90 JPEGs at two targets (width 1600 and width
640), all legs in one process: the device leg (decode, resize and encode on the GPU, one call of each kind a decode chunk), and
the host leg -- the reference's own PIL calls per file (load_image, Image.resize, exif_preserving_save), the baseline -- on one
thread, on the reference's default pool size of 10 and on a pool of 16 (pools of threads: this process holds the device, and a
process that has it open is not forked; Pillow releases the interpreter lock while it decodes, resizes and encodes).  Every leg is warmed once, then the legs alternate; the output
trees of all legs are compared byte for byte in every round.  A last, profiled device run gives the waited-for time around each
kind of device call; what is left of the leg's time is host work (reading and probing the files, planning, the files around the
scans, writing).  The parent commit has no such tool.  Prints the figures; `--out FILE` also writes them.

usage: python tools/resize_bench.py [--frame 2048x1536] [--images 512] [--rounds 3] [--targets 1600,640] [--out profiles/resize.txt]
"""

import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def read_tree(folder):
    out = {}
    for root, _, names in os.walk(folder):
        for n in names:
            with open(os.path.join(root, n), 'rb') as f:
                out[os.path.relpath(os.path.join(root, n), folder)] = f.read()
    return out


def generate(folder, n, width, height, seed=1):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = np.stack([60 + 120 * xx // width, 180 - 100 * yy // height, 40 + (xx // 16 + yy // 16) % 48], -1).astype(np.int16)
    exif = Image.Exif()
    exif[271] = 'a camera trap'
    exif[306] = '2021:03:04 05:06:07'
    for k in range(n):
        frame = np.clip(base + rng.integers(-6, 7, base.shape, dtype=np.int16) + 3 * (k % 7), 0, 255).astype(np.uint8)
        sub = os.path.join(folder, 'cam{:02d}'.format(k % 8))
        os.makedirs(sub, exist_ok=True)
        Image.fromarray(frame).save(os.path.join(sub, 'IMG_{:04d}.JPG'.format(k)), quality=90, subsampling=1, exif=exif)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frame', default='2048x1536')
    ap.add_argument('--images', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--targets', default='1600,640')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from megadetector_amd import resize_images as R
    from megadetector_amd.hip_backend import HipContext
    assert torch.cuda.is_available(), 'this tool measures on a GPU'

    W, H = (int(v) for v in args.frame.split('x'))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    tmp = tempfile.mkdtemp(prefix='resize_bench_')
    try:
        source = os.path.join(tmp, 'in')
        generate(source, args.images, W, H)
        ctx = HipContext.for_images(0)
        legs = {'device leg': dict(backend='gpu', ctx=ctx, n_workers=1),
                'host leg, one thread': dict(backend='host', n_workers=1),
                "host leg, the reference's default pool size of 10": dict(backend='host', n_workers=10, pool_type='thread'),
                'host leg, a pool of 16': dict(backend='host', n_workers=16, pool_type='thread')}
        say('resize_bench: {} files of {}x{}, 4:2:2 quality 90, with an EXIF block; quality \'keep\'; host pools are threads'.format(args.images, W, H))
        say('device: {}'.format(torch.cuda.get_device_name(0)))
        for target in [int(v) for v in args.targets.split(',')]:
            times, equal = {k: [] for k in legs}, True

            def run(name, profile=False, counts=None):
                out = os.path.join(tmp, 'out')
                shutil.rmtree(out, ignore_errors=True)
                stdout, sys.stdout = sys.stdout, open(os.devnull, 'w')
                try:
                    t0 = time.perf_counter()
                    results = R.resize_image_folder(source, out, target_width=target, profile=profile, counts=counts, **legs[name])
                    dt = time.perf_counter() - t0
                finally:
                    sys.stdout.close()
                    sys.stdout = stdout
                assert all(r['status'] == 'success' for r in results)
                print('    ran {} at {}: {:.3f} s'.format(name, target, dt), file=sys.stderr, flush=True)
                return dt, out

            for name in legs:                                   # warm: libraries, device context, page cache
                run(name)
            for _ in range(args.rounds):
                trees = []
                for name in legs:
                    dt, out = run(name)
                    times[name].append(dt)
                    trees.append(read_tree(out))
                equal = equal and all(t == trees[0] for t in trees[1:])
            counts = {}
            dt, _ = run('device leg', profile=True, counts=counts)
            say('target width {} ({} x {}):'.format(target, target, int(target / (W / H))))
            for name in legs:
                rates = sorted(args.images / t for t in times[name])
                say('  {:<58} {:8.1f} files a second (median of {}; {:.1f} .. {:.1f}; a timed window is {:.2f} s)'.format(
                    name + ':', statistics.median(rates), args.rounds, rates[0], rates[-1], statistics.median(times[name])))
            device_ms = sum(counts['ms'].values())
            say('  device leg, profiled run ({:.2f} s), waited-for milliseconds around each kind of device call for {} files in {} chunks: {}'
                .format(dt, counts['gpu'], counts['decode_chunks'], ', '.join('{} {:.1f}'.format(k, v) for k, v in sorted(counts['ms'].items()))))
            say('  of the profiled run {:.0f} % is waiting for the device and {:.0f} % is host work'.format(
                100 * device_ms / 1e3 / dt, 100 - 100 * device_ms / 1e3 / dt))
            say('  device leg counts: {}'.format({k: v for k, v in counts.items() if k != 'ms'}))
            say('  the output trees of all legs were byte-equal in every round: {}'.format(equal))
            assert equal
        ctx.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
