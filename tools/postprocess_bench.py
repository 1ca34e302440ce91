"""
Times postprocess_batch_results over a generated folder of 3-megapixel 4:2:2 quality-90 JPEGs with four boxes each
(num_images_to_sample=-1, defaults otherwise: every image is resized to 1200 pixels wide, drawn on and saved), both legs in one
process: the host leg, which is the reference's own PIL calls per image (open_image, resize_image,
render_detection_bounding_boxes, Image.save), on one thread, on the reference's default pool of 8 threads and on a pool of
--threads, and the device leg (decode, resample, draw and encode on the GPU, one call of each kind per chunk of images).  Both
legs are warmed up once, then alternate; every round's output trees are compared byte for byte.  A last, profiled device run
gives the time around each kind of device call, and with it the share of that run's wall time that is host work (reading and
probing the files, planning, packing, writing the files and the HTML).  Prints the figures; `--out FILE` also writes them.

usage: python tools/postprocess_bench.py [--frame 2048x1536] [--images 512] [--boxes 4] [--threads 16] [--rounds 3] [--out profiles/postprocess.txt]
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
    ap.add_argument('--images', type=int, default=512, help='enough that each leg runs for more than a second')
    ap.add_argument('--boxes', type=int, default=4)
    ap.add_argument('--threads', type=int, default=16, help="workers of the host leg's largest pool")
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    from megadetector_amd import postprocess_batch_results as PB

    W, H = (int(v) for v in args.frame.split('x'))
    n = args.images
    tmp = tempfile.mkdtemp(prefix='postprocess_bench_')
    try:
        rng = np.random.default_rng(1)
        base = np.linspace(0, 255, W)[None, :, None] * np.ones((H, 1, 3)) * 0.7 + rng.normal(0, 12, (H, W, 3))
        images_dir = os.path.join(tmp, 'images')
        os.makedirs(images_dir)
        entries = []
        for i in range(n):
            name = 'cam{}/img{:04d}.jpg'.format(i % 4, i)
            os.makedirs(os.path.dirname(os.path.join(images_dir, name)), exist_ok=True)
            Image.fromarray(np.clip(base + 3 * (i % 32), 0, 255).astype(np.uint8)).save(os.path.join(images_dir, name), quality=90, subsampling=1)
            dets = [{'category': str(1 + k % 3), 'conf': round(0.95 - 0.1 * k, 2), 'bbox': [0.05 + 0.2 * k, 0.1 + 0.1 * k, 0.18, 0.25]}
                    for k in range(args.boxes)]
            entries.append({'file': name, 'detections': dets})
        del base
        results_file = os.path.join(tmp, 'results.json')
        with open(results_file, 'w') as f:
            json.dump({'info': {'detector': 'md_v5a.0.0.pt'}, 'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'},
                       'images': entries}, f)

        def run(backend, threads=None, **kw):
            out = os.path.join(tmp, 'out')
            shutil.rmtree(out, ignore_errors=True)
            o = PB.PostProcessingOptions()
            o.md_results_file, o.image_base_dir, o.output_dir, o.num_images_to_sample = results_file, images_dir, out, -1
            if threads == 1:
                o.parallelize_rendering = False
            elif threads is not None:
                o.parallelize_rendering_n_cores = threads
            t0 = time.perf_counter()
            with redirect_stdout(io.StringIO()):
                counts = PB.process_batch_results(o, backend=backend, **kw).counts
            return time.perf_counter() - t0, counts, out

        run('gpu')                                                        # warm-up: the runtime, the first launches
        run('host', threads=args.threads)
        pools = [1, 8, args.threads] if args.threads != 8 else [1, 8]
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
        med = statistics.median
        spread = lambda v: '{:.1f} files a second (median of {}; {:.1f} .. {:.1f})'.format(n / med(v), len(v), n / max(v), n / min(v))
        ms = profiled['ms']
        device_ms = sum(ms.values())
        lines = [
            'postprocess_bench: {} files of {}x{}, 4:2:2 quality 90, {} boxes each; num_images_to_sample=-1, defaults otherwise (1200 pixels wide)'.format(
                n, W, H, args.boxes),
            'device: {}'.format(torch.cuda.get_device_name(0)),
            'windows: each leg runs {:.1f} .. {:.1f} s a round; {} rounds, the legs alternating in one process after one warm-up each'.format(
                min(min(gpu_s), min(min(v) for v in host_s.values())), max(max(gpu_s), max(max(v) for v in host_s.values())), args.rounds),
            'device leg (decode + resample + draw + encode on the GPU, files and HTML written):  ' + spread(gpu_s),
        ]
        for p in pools:
            what = 'one thread' if p == 1 else "the reference's default pool of 8 threads" if p == 8 else 'a pool of {} threads'.format(p)
            lines.append("host leg, the reference's PIL calls, {}:  ".format(what) + spread(host_s[p]))
        lines += [
            'device leg, profiled run of {:.2f} s, milliseconds around each kind of device call for {} files in {} chunk(s): '.format(
                wall, n, profiled['decode_chunks']) + ', '.join('{} {:.1f}'.format(k, ms.get(k, 0.0)) for k in ('decode', 'resample', 'draw', 'encode')),
            'of the {:.0f} ms around device calls {:.1%} are the decode calls (entropy decode and reconstruction, with the packing and the upload of the scans)'.format(
                device_ms, ms.get('decode', 0.0) / device_ms),
            'host work (reading and probing the files, planning, writing the files and the HTML) is {:.1%} of the profiled run\'s wall time'.format(
                1 - device_ms / (wall * 1e3)),
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
