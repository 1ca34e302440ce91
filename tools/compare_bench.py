"""
Times compare_batch_results over a generated folder of 3-megapixel 4:2:2 quality-90 JPEGs and THREE results files with planted
disagreements, hence three pairwise comparisons in which every file is rendered three times (defaults otherwise: 800 pixels
wide), both legs in one process: the host leg, which is the reference's own PIL calls per comparison and image (open_image,
resize_image, render_detection_bounding_boxes twice, Image.save), on one thread, on the reference's default pool of 10
threads and on a pool of --threads, and the device leg (each file decoded and resampled ONCE per chunk, one fan-out draw and
one encode call per chunk).  Both legs are warmed up once, then alternate; every round's output trees are compared byte for
byte.  A last, profiled device run gives the time around each kind of device call.

In the same run mdhip_draw_ops_from is timed for one chunk against what the library offered before it for the same result:
a device-to-device copy per destination, then mdhip_draw_ops in place.  The two alternate; device events around --calls calls.

usage: python tools/compare_bench.py [--frame 2048x1536] [--images 256] [--threads 16] [--rounds 3] [--out profiles/compare.txt]
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


def detections(i, which):
    """four boxes a file; which results file sees which of them above the threshold changes with the file's number, so that
    over the three comparisons every category is used"""
    dets = []
    for k in range(4):
        conf = round(0.95 - 0.1 * k, 2)
        if (i + k + which) % 5 == 0:
            conf = 0.12                                              # drawn (above 0.1), not a detection (below 0.15)
        dets.append({'category': str(1 + (k + (which if i % 7 == 0 else 0)) % 3), 'conf': conf,
                     'bbox': [0.05 + 0.2 * k + 0.01 * which, 0.1 + 0.1 * k, 0.18, 0.25]})
    if i % 4 == which:
        dets = [dict(d, conf=0.12) for d in dets]                    # a non-detection in this file
    return dets


def fan_out_bench(torch, args):
    """one chunk: --shared images of 800 x 600 with three destinations each, eight boxes and their labels a destination"""
    from megadetector_amd import device_render as DR
    from megadetector_amd import preview as PV
    from megadetector_amd.hip_backend import HipContext
    device = torch.device('cuda:0')
    ctx = HipContext.for_images(0)
    try:
        W, H, n_src, fan = 800, 600, args.shared, 3
        g = torch.Generator(device='cpu').manual_seed(1)
        shared = [torch.randint(0, 256, (W * H * 3,), dtype=torch.uint8, generator=g).to(device) for _ in range(n_src)]
        o = PV.PreviewOptions(confidence_threshold=0.1, output_image_width=None)
        plans = []
        for m in range(n_src * fan):
            dets = [{'category': str(1 + k % 3), 'conf': 0.9 - 0.05 * k, 'bbox': [0.03 + 0.11 * k, 0.1 + 0.05 * ((k + m) % 6), 0.1, 0.3]} for k in range(8)]
            plans.append(PV.render_plan(dets, W, H, o))
        dst_src = [m // fan for m in range(n_src * fan)]
        sizes = [(W, H)] * n_src
        new = [torch.empty(W * H * 3, dtype=torch.uint8, device=device) for _ in plans]
        old = [torch.empty(W * H * 3, dtype=torch.uint8, device=device) for _ in plans]
        op_image, ops, packed = DR.pack_ops(plans)
        patches = torch.from_numpy(np.frombuffer(bytes(packed), np.uint8).copy()).to(device)

        def fan_out():
            ctx.draw_ops_from([t.data_ptr() for t in shared], sizes, [W * 3] * n_src, [t.data_ptr() for t in new], dst_src,
                              [W * 3] * len(new), op_image, ops, patches.data_ptr(), len(packed))

        def copies_then_draw():
            for m, t in enumerate(old):
                t.copy_(shared[dst_src[m]])
            ctx.draw_ops([t.data_ptr() for t in old], [(W, H)] * len(old), [W * 3] * len(old), op_image, ops, patches.data_ptr(), len(packed))

        def timed(f):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.calls):
                f()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) / args.calls

        for _ in range(3):
            fan_out()
            copies_then_draw()
        torch.cuda.synchronize()
        equal = all(torch.equal(a, b) for a, b in zip(new, old))
        a_ms, b_ms = [], []
        for _ in range(args.repetitions):
            a_ms.append(timed(fan_out))
            b_ms.append(timed(copies_then_draw))
        med = statistics.median
        moved = 2 * len(new) * W * H * 3
        faster = max(a_ms) < min(b_ms)
        return [
            'fan-out draw, one chunk: {} shared images of {}x{}, {} destinations, {} operations; {} repetitions of {} calls, alternating, device events'.format(
                n_src, W, H, len(new), len(ops), args.repetitions, args.calls),
            'mdhip_draw_ops_from (one launch):                         {:.3f} ms a call (median; {:.3f} .. {:.3f}), {:.0f} GB/s of bytes read and written'.format(
                med(a_ms), min(a_ms), max(a_ms), moved / med(a_ms) / 1e6),
            '{} device-to-device copies, then mdhip_draw_ops in place:  {:.3f} ms a call (median; {:.3f} .. {:.3f})'.format(
                len(old), med(b_ms), min(b_ms), max(b_ms)),
            'both ways give the same bytes: {}; the new call is faster by more than the spread of the repetitions: {}'.format(equal, faster),
        ], equal
    finally:
        ctx.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frame', default='2048x1536')
    ap.add_argument('--images', type=int, default=256, help='enough that each leg runs for more than a second')
    ap.add_argument('--threads', type=int, default=16, help="workers of the host leg's largest pool")
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shared', type=int, default=16, help='shared images of the fan-out measurement')
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--repetitions', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    from megadetector_amd import compare_batch_results as CB

    W, H = (int(v) for v in args.frame.split('x'))
    n = args.images
    tmp = tempfile.mkdtemp(prefix='compare_bench_')
    try:
        rng = np.random.default_rng(1)
        base = np.linspace(0, 255, W)[None, :, None] * np.ones((H, 1, 3)) * 0.7 + rng.normal(0, 12, (H, W, 3))
        images_dir = os.path.join(tmp, 'images')
        os.makedirs(images_dir)
        names = []
        for i in range(n):
            name = 'cam{}/img{:04d}.jpg'.format(i % 4, i)
            os.makedirs(os.path.dirname(os.path.join(images_dir, name)), exist_ok=True)
            Image.fromarray(np.clip(base + 3 * (i % 32), 0, 255).astype(np.uint8)).save(os.path.join(images_dir, name), quality=90, subsampling=1)
            names.append(name)
        del base
        results_files = []
        for which in range(3):
            results_files.append(os.path.join(tmp, 'results_{}.json'.format('abc'[which])))
            with open(results_files[-1], 'w') as f:
                json.dump({'info': {'detector': 'model {}'.format('abc'[which])}, 'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'},
                           'images': [{'file': name, 'detections': detections(i, which)} for i, name in enumerate(names)]}, f)

        def run(backend, threads=None, **kw):
            out = os.path.join(tmp, 'out')
            shutil.rmtree(out, ignore_errors=True)
            o = CB.BatchComparisonOptions()
            o.output_folder, o.image_folder = out, images_dir
            if threads is not None:
                o.n_rendering_workers = threads
            _n_way_options(CB, o, results_files)
            t0 = time.perf_counter()
            with redirect_stdout(io.StringIO()):
                results = CB.compare_batch_results(o, backend=backend, **kw)
            return time.perf_counter() - t0, results.counts, out

        run('gpu')                                                        # warm-up: the runtime, the first launches
        run('host', threads=args.threads)
        pools = [1, 10, args.threads] if args.threads != 10 else [1, 10]
        gpu_s, host_s, equal = [], {p: [] for p in pools}, True
        jobs = None
        for k in range(args.rounds):
            print('round {} of {}'.format(k + 1, args.rounds), file=sys.stderr, flush=True)
            t, counts, out = run('gpu')
            jobs = counts['jobs']
            assert counts['gpu'] == jobs and counts['host'] == 0 and counts['files_decoded_pil'] == 0, counts
            assert counts['files_decoded_gpu'] < jobs, counts
            gpu_s.append(t)
            gpu_tree = read_tree(out)
            for p in pools:
                t, _, out = run('host', threads=p)
                host_s[p].append(t)
                equal = equal and read_tree(out) == gpu_tree
        categories = sorted({os.path.dirname(rel) for rel in gpu_tree if rel.endswith('.jpg')})
        wall, profiled, _ = run('gpu', profile=True)
        med = statistics.median
        spread = lambda v: '{:.1f} renderings a second (median of {}; {:.1f} .. {:.1f})'.format(jobs / med(v), len(v), jobs / max(v), jobs / min(v))
        ms = profiled['ms']
        device_ms = sum(ms.values())
        lines = [
            'compare_bench: {} files of {}x{}, 4:2:2 quality 90, 4 boxes each in three results files; three pairwise comparisons, {} renderings in {} category folders, defaults otherwise (800 pixels wide)'.format(
                n, W, H, jobs, len(categories)),
            'device: {}'.format(torch.cuda.get_device_name(0)),
            'windows: each leg runs {:.1f} .. {:.1f} s a round; {} rounds, the legs alternating in one process after one warm-up each'.format(
                min(min(gpu_s), min(min(v) for v in host_s.values())), max(max(gpu_s), max(max(v) for v in host_s.values())), args.rounds),
            'device leg ({} files decoded for {} renderings; resample, fan-out draw and encode on the GPU; files and HTML written):  '.format(
                counts['files_decoded_gpu'], jobs) + spread(gpu_s),
        ]
        for p in pools:
            what = 'one thread' if p == 1 else "the reference's default pool of 10 threads" if p == 10 else 'a pool of {} threads'.format(p)
            lines.append("host leg, the reference's PIL calls, {}:  ".format(what) + spread(host_s[p]))
        lines += [
            'device leg, profiled run of {:.2f} s, milliseconds around each kind of device call for {} renderings in {} chunk(s): '.format(
                wall, jobs, profiled['decode_chunks']) + ', '.join('{} {:.1f}'.format(k, ms.get(k, 0.0)) for k in ('decode', 'resample', 'draw', 'encode')),
            'host work (reading and probing the files, planning, packing, writing the files and the HTML) is {:.1%} of the profiled run\'s wall time'.format(
                1 - device_ms / (wall * 1e3)),
            'the output trees of all legs were byte-equal in every round: {}'.format(equal),
        ]
        fan_lines, fan_equal = fan_out_bench(torch, args)
        lines += fan_lines
        print('\n'.join(lines))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return 0 if equal and fan_equal else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _n_way_options(CB, options, results_files):
    """the pairwise options n_way_comparison makes with its defaults (compare_batch_results itself takes profile=)"""
    options.pairwise_options = []
    for i in range(len(results_files)):
        for j in range(i + 1, len(results_files)):
            p = CB.PairwiseBatchComparisonOptions()
            p.results_filename_a, p.results_filename_b = results_files[i], results_files[j]
            p.rendering_confidence_threshold_a = p.rendering_confidence_threshold_b = 0.15 * 0.6666
            p.detection_thresholds_a, p.detection_thresholds_b = {'default': 0.15}, {'default': 0.15}
            options.pairwise_options.append(p)
    return options


if __name__ == '__main__':
    sys.exit(main())
