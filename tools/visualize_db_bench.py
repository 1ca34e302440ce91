"""
Times visualize_db over a generated COCO Camera Traps database of 3-megapixel 4:2:2 quality-90 JPEGs with four ground-truth
boxes each, a quarter of the boxes thinner than twice their outline once the image is 1000 pixels wide (default options: every image is
resized, drawn on and saved), both legs in one process: the host leg, which is the reference's own PIL calls per image
(open_image, resize_image, render_db_bounding_boxes, Image.save), on one thread, on the reference's pool of 12 threads and on a
pool of --threads, and the device leg (decode, resample, draw and encode on the GPU, one call of each kind per chunk of
images).  Both legs are warmed up once, then alternate; every round's output trees are compared byte for byte.  A profiled
device run gives the time waited for around each kind of device call.  A last device run with thin_outlines off (a switch of
the bench alone) counts the images that thin boxes would send to the host leg.  Prints the figures; `--out FILE` also writes
them.

usage: python tools/visualize_db_bench.py [--frame 2048x1536] [--images 384] [--threads 16] [--rounds 3] [--out profiles/visualize_db.txt]
"""

import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from contextlib import redirect_stdout

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frame', default='2048x1536')
    ap.add_argument('--images', type=int, default=384, help='enough that each leg runs for more than a second')
    ap.add_argument('--threads', type=int, default=16, help="workers of the host leg's largest pool")
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    from megadetector_amd import visualize_db as VD

    W, H = (int(v) for v in args.frame.split('x'))
    n = args.images
    tmp = tempfile.mkdtemp(prefix='visualize_db_bench_')
    try:
        rng = np.random.default_rng(1)
        base = np.linspace(0, 255, W)[None, :, None] * np.ones((H, 1, 3)) * 0.7 + rng.normal(0, 12, (H, W, 3))
        images_dir = os.path.join(tmp, 'images')
        os.makedirs(images_dir)
        images, annotations = [], []
        for i in range(n):
            name = 'cam{}/img{:04d}.jpg'.format(i % 4, i)
            os.makedirs(os.path.dirname(os.path.join(images_dir, name)), exist_ok=True)
            Image.fromarray(np.clip(base + 3 * (i % 32), 0, 255).astype(np.uint8)).save(os.path.join(images_dir, name), quality=90, subsampling=1)
            images.append({'id': name, 'file_name': name, 'width': W, 'height': H})
            for k in range(4):
                # boxes of a fifth of the image, and a quarter of all boxes of 9 x 7 source pixels (5 x 4 at 1000 pixels wide): two,
                # one, one and none of them in every four images
                thin = k >= 4 - (2, 1, 1, 0)[i % 4]
                box = [W * (0.1 + 0.2 * k) + i % 7, H * 0.7, 8, 6] if thin else [W * (0.05 + 0.2 * k), H * (0.1 + 0.1 * k), W * 0.18, H * 0.25]
                annotations.append({'id': '{}_{}'.format(i, k), 'image_id': name, 'category_id': 1 + k % 3, 'bbox': box})
        del base
        db_file = os.path.join(tmp, 'db.json')
        with open(db_file, 'w') as f:
            json.dump({'info': {}, 'images': images, 'annotations': annotations,
                       'categories': [{'id': 1, 'name': 'deer'}, {'id': 2, 'name': 'fox'}, {'id': 3, 'name': 'boar'}]}, f)

        def run(backend, threads=None, **kw):
            out = os.path.join(tmp, 'out')
            shutil.rmtree(out, ignore_errors=True)
            o = VD.DbVizOptions()
            if threads == 1:
                o.parallelize_rendering = False
            elif threads is not None:
                o.parallelize_rendering_n_cores = threads
            counts = {}
            t0 = time.perf_counter()
            with redirect_stdout(io.StringIO()):
                VD.visualize_db(db_file, out, images_dir, o, backend=backend, counts=counts, **kw)
            return time.perf_counter() - t0, counts, out

        run('gpu')                                                        # warm-up: the runtime, the first launches
        run('host', threads=args.threads)
        pools = [1, 12, args.threads] if args.threads != 12 else [1, 12]
        gpu_s, host_s, equal = [], {p: [] for p in pools}, True
        for k in range(args.rounds):
            print('round {} of {}'.format(k + 1, args.rounds), file=sys.stderr, flush=True)
            t, counts, out = run('gpu')
            assert counts['gpu'] == n and counts['host'] == 0 and counts['files_decoded_pil'] == 0, counts
            gpu_s.append(t)
            gpu_tree = read_tree(out)
            for p in pools:
                t, _, out = run('host', threads=p)
                host_s[p].append(t)
                equal = equal and read_tree(out) == gpu_tree
        wall, profiled, _ = run('gpu', profile=True)
        t_off, off, out = run('gpu', thin_outlines=False)
        equal = equal and read_tree(out) == gpu_tree
        med = statistics.median
        spread = lambda v: '{:.1f} files a second (median of {}; {:.1f} .. {:.1f})'.format(n / med(v), len(v), n / max(v), n / min(v))
        ms = profiled['ms']
        device_ms = sum(ms.values())
        lines = [
            'visualize_db_bench: {} files of {}x{}, 4:2:2 quality 90, 4 ground-truth boxes each, a quarter of all boxes 5 x 4 pixels at the rendered size (in 3 of 4 images); '
            'default options (1000 pixels wide)'.format(n, W, H),
            'device: {}'.format(torch.cuda.get_device_name(0)),
            'windows: each leg runs {:.1f} .. {:.1f} s a round; {} rounds, the legs alternating in one process after one warm-up each'.format(
                min(min(gpu_s), min(min(v) for v in host_s.values())), max(max(gpu_s), max(max(v) for v in host_s.values())), args.rounds),
            'device leg (decode + resample + draw + encode on the GPU, files and HTML written):  ' + spread(gpu_s),
        ]
        for p in pools:
            what = 'one thread' if p == 1 else "the reference's pool of 12 threads" if p == 12 else 'a pool of {} threads'.format(p)
            lines.append("host leg, the reference's PIL calls, {}:  ".format(what) + spread(host_s[p]))
        lines += [
            'device leg, profiled run of {:.2f} s, milliseconds waited for around each kind of device call for {} files in {} chunk(s): '.format(
                wall, n, profiled['decode_chunks']) + ', '.join('{} {:.1f}'.format(k, ms.get(k, 0.0)) for k in ('decode', 'resample', 'draw', 'encode')),
            'host work (reading and probing the files, planning, writing the files and the HTML) is {:.1%} of the profiled run\'s wall time'.format(
                1 - device_ms / (wall * 1e3)),
            'thin outlines: with thin_outlines off the host leg takes {} of {} images ({:.1%}) and the run makes {:.1f} files a second '
            '(one run, {} host threads); with it on, none'.format(off['host'], n, off['host'] / n, n / t_off, 12),
            'the output trees of all legs were byte-equal in every round: {}'.format(equal),
        ]
        print('\n'.join(lines))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return 0 if equal else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
