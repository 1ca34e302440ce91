"""
The RDE review folder, both legs on the same input in the same run: rde_review.write_review_folder with backend='host' (the
reference's way: PIL opens and fully decodes one file per tile) against backend='gpu' (every file of a group of sheets
decoded once on the device, one mdhip_thumbnails call per decode chunk, one encoder call per group).

The input is generated: --cameras cameras of --images 3-MP JPEGs (2048 x 1536, noise over a gradient, quality 85) with
--spots planted boxes each, which come back in most images -- so a sheet carries tens to 150 tiles.  The legs alternate
(host, gpu, host, gpu, ...); the host leg runs with one thread and with the reference's ten (its nWorkers default, threads).
The files of the two legs are compared byte for byte before any figure is printed.

Run:  python tools/rde_review_bench.py [--cameras 3 --images 60 --spots 3 --rounds 2]
"""

import argparse
import copy
import os
import statistics
import sys
import tempfile
import time
from multiprocessing.pool import ThreadPool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from megadetector_amd import rde_review as RV                # noqa: E402
from megadetector_amd import repeat_detections as RD         # noqa: E402

WIDTH, HEIGHT = 2048, 1536


def make_input(folder, cameras, images, spots, seed=1):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    base = np.stack([xx * 255 // WIDTH, yy * 255 // HEIGHT, (xx + yy) * 255 // (WIDTH + HEIGHT)], axis=2).astype(np.int16)
    out = []
    for c in range(cameras):
        os.makedirs(os.path.join(folder, 'cam{}'.format(c)))
        places = [(rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6), rng.uniform(0.15, 0.3), rng.uniform(0.15, 0.3)) for _ in range(spots)]
        for k in range(images):
            name = 'cam{}/I{:04d}.jpg'.format(c, k)
            noisy = np.clip(base + rng.integers(-30, 31, (HEIGHT, WIDTH, 1), dtype=np.int16), 0, 255).astype(np.uint8)
            Image.fromarray(noisy).save(os.path.join(folder, name), quality=85)
            dets = []
            for x, y, w, h in places:
                if rng.random() < 0.9:
                    jx, jy = rng.integers(-1, 2, 2) / 1000.0
                    dets.append({'category': '1', 'conf': round(float(rng.uniform(0.2, 0.95)), 3),
                                 'bbox': [round(x + jx, 3), round(y + jy, 3), round(w, 3), round(h, 3)]})
            out.append({'file': name, 'detections': dets})
    return {'info': {'format_version': '1.4'}, 'detection_categories': {'1': 'animal'}, 'images': out}


def host_leg(rde, options, threads):
    """the host leg as the reference runs it: its serial first pass, then the samples on `threads` threads"""
    os.makedirs(options.outputBase, exist_ok=True)
    flat = RV.name_samples(rde.suspicious_detections)
    if threads == 1:
        for location in flat:
            RV.render_sample_host(location, options.outputBase, options)
    else:
        with ThreadPool(threads) as pool:
            pool.map(lambda location: RV.render_sample_host(location, options.outputBase, options), flat)
    return len(flat)


def files_of(folder):
    return {n: open(os.path.join(folder, n), 'rb').read() for n in sorted(os.listdir(folder)) if n.endswith('.jpg')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cameras', type=int, default=3)
    ap.add_argument('--images', type=int, default=60)
    ap.add_argument('--spots', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    args = ap.parse_args()
    from megadetector_amd.hip_backend import HipContext
    with tempfile.TemporaryDirectory() as tmp:
        images = os.path.join(tmp, 'images')
        t0 = time.perf_counter()
        results = make_input(images, args.cameras, args.images, args.spots)
        print('input: {} cameras x {} images of {} x {}, {} spots each (made in {:.1f} s)'.format(
            args.cameras, args.images, WIDTH, HEIGHT, args.spots, time.perf_counter() - t0))
        rde_options = RD.RepeatDetectionOptions()
        ctx = HipContext.for_images(0)
        seconds = {'host x1': [], 'host x10': [], 'gpu': []}
        counts = None

        def options_for(name):
            o = RV.ReviewFolderOptions()
            o.imageBase, o.outputBase = images, os.path.join(tmp, name)
            return o

        for r in range(args.rounds + 1):                                 # round 0 warms both legs up and is not counted
            for leg in ('host x1', 'gpu', 'host x10', 'gpu'):
                if r == 0 and leg == 'host x10':
                    continue
                rde = RD.mark_repeat_detections(copy.deepcopy(results), rde_options, backend='gpu')
                name = '{}_{}_{}'.format(leg.replace(' ', ''), r, len(seconds[leg]))
                t0 = time.perf_counter()
                if leg == 'gpu':
                    counts = RV.write_review_folder(rde, options_for(name), backend='gpu', ctx=ctx)
                    folder = counts['folder']
                else:
                    o = options_for(name)
                    host_leg(rde, o, 1 if leg == 'host x1' else 10)
                    folder = o.outputBase
                dt = time.perf_counter() - t0
                if r:
                    seconds[leg].append(dt)
                if leg == 'gpu':
                    gpu_files = files_of(folder)
                else:
                    host_files = files_of(folder)
            assert gpu_files == host_files and gpu_files, 'the two legs wrote different files'
        rde = RD.mark_repeat_detections(copy.deepcopy(results), rde_options, backend='gpu')
        profiled = RV.write_review_folder(rde, options_for('profiled'), backend='gpu', ctx=ctx, profile=True)
        sheets = counts['sheets']
        tiles_per_sheet = counts['tiles'] / max(sheets, 1)
        print('{} sheets, {:.0f} tiles a sheet; the files of the two legs are equal byte for byte'.format(sheets, tiles_per_sheet))
        for leg, ts in seconds.items():
            med = statistics.median(ts)
            print('{:9s} {:7.2f} s median of {} ({:.2f} .. {:.2f}): {:6.2f} sheets/s'.format(leg, med, len(ts), min(ts), max(ts), sheets / med))
        print('gpu leg: {} sheets on the GPU, {} by the host leg; files decoded: {} on the GPU, {} by PIL (the host leg decodes {}); '
              '{} tiles in {} mdhip_thumbnails calls ({:.0f} a call); {} decode chunks, {} encoder calls'.format(
                  counts['gpu'], counts['host'], counts['files_decoded_gpu'], counts['files_decoded_pil'], counts['tiles'] + sheets,
                  counts['tiles'], counts['tile_calls'], counts['tiles'] / max(counts['tile_calls'], 1), counts['decode_chunks'],
                  counts['encode_calls']))
        groups = max(profiled['encode_calls'], 1)
        print('gpu leg, per group of sheets ({} groups; the device waited for around each kind of call): decode {:.1f} ms, '
              'thumbnails {:.1f} ms, encode {:.1f} ms'.format(groups, profiled['ms'].get('decode', 0.0) / groups,
                                                             profiled['ms'].get('thumbnails', 0.0) / groups,
                                                             profiled['ms'].get('encode', 0.0) / groups))
        ctx.close()


if __name__ == '__main__':
    main()
