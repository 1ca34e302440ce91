"""
Times separate_detections_into_folders with --render_boxes --category_names_to_blur person over a generated folder of
3-megapixel 4:2:2 JPEGs (a few boxes and one person box each), both legs in one run: the host leg, which is the reference's own
PIL calls per image (load_image, blur_detections, render_detection_bounding_boxes per category, exif_preserving_save), on one
thread and on the reference's thread pool, and the device leg (decode, blur, draw and encode on the GPU, one call of each kind
per chunk of images).  Both legs are warmed up once, then alternate; every round's output trees are compared byte for byte.
A last, profiled device run gives the time around each kind of device call.  A fourth leg is the device leg with
--keep_source_blocks, alternating with the plain device leg in the same rounds (its baseline), with its own profiled run; its
tree is compared with the host leg's under the same option once.  For one file of the scene the shares of 8x8 blocks that keep
the source's coefficients, and of pixels Pillow decodes identically to the source, are computed on the CPU with and without the
option.  Prints the figures; `--out FILE` also writes them.

usage: python tools/separate_bench.py [--frame 2048x1536] [--images 576] [--boxes 4] [--threads 16] [--rounds 3] [--out profiles/separate.txt]
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
    ap.add_argument('--images', type=int, default=576, help="enough that each leg runs for more than a second")
    ap.add_argument('--boxes', type=int, default=4, help='boxes per image beside the person box')
    ap.add_argument('--threads', type=int, default=16, help='workers of the host leg\'s pool (the reference\'s n_threads)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    from megadetector_amd import separate_detections as SD
    from megadetector_amd.hip_backend import HipContext

    W, H = (int(v) for v in args.frame.split('x'))
    n = args.images
    tmp = tempfile.mkdtemp(prefix='separate_bench_')
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
            dets = [{'category': '1' if k % 2 == 0 else '3', 'conf': round(0.95 - 0.1 * k, 2), 'bbox': [0.05 + 0.2 * k, 0.1 + 0.1 * k, 0.18, 0.25]}
                    for k in range(args.boxes)]
            dets.append({'category': '2', 'conf': 0.9, 'bbox': [0.4, 0.3, 0.25, 0.5]})
            entries.append({'file': name, 'detections': dets})
        del base
        results_file = os.path.join(tmp, 'results.json')
        with open(results_file, 'w') as f:
            json.dump({'info': {'detector': 'md_v5a.0.0.pt'}, 'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'},
                       'images': entries}, f)

        def run(backend, threads=1, keep=False, **kw):
            out = os.path.join(tmp, 'out')
            shutil.rmtree(out, ignore_errors=True)
            o = SD.SeparateDetectionsIntoFoldersOptions()
            o.results_file, o.base_input_folder, o.base_output_folder = results_file, images_dir, out
            o.render_boxes, o.category_names_to_blur, o.n_threads = True, 'person', threads
            o.keep_source_blocks = keep
            t0 = time.perf_counter()
            with redirect_stdout(io.StringIO()):
                counts = SD.separate_detections_into_folders(o, backend=backend, **kw)
            return time.perf_counter() - t0, counts, out

        ctx = HipContext.for_images(0)
        run('gpu', ctx=ctx)                                               # warm-up: scratch buffers, the first launches
        run('host')
        run('gpu', ctx=ctx, keep=True)
        gpu_s, kept_s, host_s, pool_s, equal = [], [], [], [], True
        for k in range(args.rounds):
            print('round {} of {}'.format(k + 1, args.rounds), file=sys.stderr, flush=True)
            t, counts, out = run('gpu', ctx=ctx)
            assert counts['gpu'] == n and counts['host'] == 0, counts
            gpu_s.append(t)
            gpu_tree = read_tree(out)
            t, counts, out = run('gpu', ctx=ctx, keep=True)
            assert counts['gpu'] == n and counts['host'] == 0 and counts['kept'] == n and counts['kept_refused'] == 0, counts
            kept_s.append(t)
            kept_tree = read_tree(out)
            t, _, out = run('host')
            host_s.append(t)
            equal = equal and read_tree(out) == gpu_tree
            t, _, out = run('host', threads=args.threads)
            pool_s.append(t)
            equal = equal and read_tree(out) == gpu_tree
        _, profiled, _ = run('gpu', ctx=ctx, profile=True)
        _, profiled_kept, _ = run('gpu', ctx=ctx, keep=True, profile=True)
        ctx.close()
        _, counts, out = run('host', threads=args.threads, keep=True)
        kept_equal = counts['kept'] == n and read_tree(out) == kept_tree

        # one file of the scene on the CPU: blocks that keep the source's coefficients, pixels Pillow decodes as the source's
        from megadetector_amd import jpeg_host as J
        name = entries[0]['file']
        with open(os.path.join(images_dir, name), 'rb') as f:
            source = f.read()
        rel = next(k for k in gpu_tree if k.endswith(os.path.basename(name)))

        def shares(data):
            (_, ha, ca), (_, hb, cb) = J.decode(data), J.decode(source)
            same = [(a == b).all(axis=2) for a, b in zip(ha.planes(ca), hb.planes(cb))]
            pa, pb = np.asarray(Image.open(io.BytesIO(data)).convert('RGB')), np.asarray(Image.open(io.BytesIO(source)).convert('RGB'))
            return sum(int(v.sum()) for v in same) / sum(v.size for v in same), float((pa == pb).all(axis=2).mean())

        plain_share, kept_share = shares(gpu_tree[rel]), shares(kept_tree[rel])
        med = statistics.median
        spread = lambda v: '{:.1f} files a second (median of {}; {:.1f} .. {:.1f})'.format(n / med(v), len(v), n / max(v), n / min(v))
        ms, ms_kept = profiled['ms'], profiled_kept['ms']
        ratio = med(gpu_s) / med(kept_s)
        lines = [
            'separate_bench: {} files of {}x{}, 4:2:2 quality 90, {} boxes and one person box each; --render_boxes --category_names_to_blur person'.format(
                n, W, H, args.boxes),
            'device: {}'.format(torch.cuda.get_device_name(0)),
            'device leg (decode + blur + draw + encode on the GPU, files written):  ' + spread(gpu_s),
            'host leg, the reference\'s PIL calls, one thread:                       ' + spread(host_s),
            'host leg, the reference\'s pool of {} threads:                          '.format(args.threads) + spread(pool_s),
            'device leg, profiled run, milliseconds around each kind of device call for {} files in {} chunk(s): '.format(n, profiled['decode_chunks']) +
            ', '.join('{} {:.1f}'.format(k, ms.get(k, 0.0)) for k in ('decode', 'blur', 'draw', 'encode')),
            'the output trees of all legs were byte-equal in every round: {}'.format(equal),
            'device leg with --keep_source_blocks, alternating with the device leg above (its baseline):  ' + spread(kept_s) +
            '; {:.3f} x the baseline'.format(ratio),
            'the same, profiled run, milliseconds around each kind of device call: ' +
            ', '.join('{} {:.1f}'.format(k, ms_kept.get(k, 0.0)) for k in ('decode', 'blur', 'draw', 'encode_kept', 'encode')) +
            ' (encode_kept is the mdhip_jpeg_encode_kept call with its read-back; without the option the encode call took {:.1f})'.format(ms.get('encode', 0.0)),
            'its tree equals the host leg\'s with the option ({} threads), every copy kept: {}'.format(args.threads, kept_equal),
            'one file of the scene against its source, without the option: {:.1%} of the blocks keep their coefficients, Pillow decodes {:.1%} of the pixels identically'.format(*plain_share),
            'the same file with the option:                                 {:.1%} of the blocks keep their coefficients, Pillow decodes {:.1%} of the pixels identically'.format(*kept_share),
        ]
        print('\n'.join(lines))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return 0 if equal and kept_equal else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
