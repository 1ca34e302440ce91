"""
Times repeat-detection elimination on a generated result set, in one run: backend='gpu' (mdhip_repeat_detections) against
backend='host' (mdjpeg_repeat_detections: one thread, the same rule, the same arithmetic), legs alternating.  The result set
is many cameras with a stated number of detections each and one large camera; a camera's detections come from drifting spots
(rocks that are boxed again and again) among random boxes.  Reported: the boxes that take part, the whole call of either
backend by the host clock, the device time of the three phases apart from the upload and the read-back (events on the call's
stream: mdhip_repeat_detections_times), the whole function on the results in memory, and that both backends gave the same
arrays.  The reference's own time, with its quadtree, is not measured here: the package it uses is not installed.
Prints the figures; `--out FILE` also writes them.

usage: python tools/rde_bench.py [--cameras 150] [--per_camera 2000] [--large 60000] [--rounds 3] [--out profiles/rde.txt]
"""

import argparse
import copy
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def camera_detections(rng, n):
    """n detections of one camera as arrays: 70 % from one of 40 spots that drift slowly, the rest anywhere"""
    spots = np.stack([rng.uniform(0.02, 0.5, 40), rng.uniform(0.02, 0.6, 40), rng.uniform(0.05, 0.3, 40), rng.uniform(0.05, 0.3, 40)], 1)
    drift = rng.uniform(0.0, 0.3, 40) / max(n, 1)
    which = rng.integers(0, 40, n)
    at_spot = rng.random(n) < 0.7
    x = np.where(at_spot, spots[which, 0] + drift[which] * np.arange(n) + rng.normal(0, 0.002, n), rng.uniform(0, 0.6, n))
    y = np.where(at_spot, spots[which, 1] + rng.normal(0, 0.002, n), rng.uniform(0, 0.6, n))
    w = np.where(at_spot, spots[which, 2], rng.uniform(0.03, 0.4, n))
    h = np.where(at_spot, spots[which, 3], rng.uniform(0.03, 0.4, n))
    cat = np.where(at_spot, 1 + which % 3, rng.integers(1, 4, n))
    conf = rng.uniform(0.1, 1.0, n)
    return x, y, w, h, cat, conf


def generated_results(cameras, per_camera, large, seed=1):
    rng = np.random.default_rng(seed)
    images = []
    sizes = [per_camera] * cameras + ([large] if large else [])
    for c, n in enumerate(sizes):
        x, y, w, h, cat, conf = camera_detections(rng, n)
        k = 0
        i = 0
        while k < n:
            m = min(n - k, 1 + i % 4)                      # one to four detections an image
            images.append({'file': 'site{:02d}/cam{:04d}/IMG_{:06d}.JPG'.format(c % 7, c, i),
                           'detections': [{'category': str(int(cat[j])), 'conf': float(conf[j]),
                                           'bbox': [float(x[j]), float(y[j]), float(w[j]), float(h[j])]} for j in range(k, k + m)]})
            k += m
            i += 1
    return {'info': {'format_version': '1.4', 'detector': 'generated'},
            'detection_categories': {'1': 'animal', '2': 'person', '3': 'vehicle'}, 'images': images}, sizes


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cameras', type=int, default=150)
    ap.add_argument('--per_camera', type=int, default=2000, help='detections of each camera')
    ap.add_argument('--large', type=int, default=60000, help='detections of the one large camera (0: none)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), 'rde_bench needs a GPU: a time from anywhere else says nothing'
    from megadetector_amd import _lib
    from megadetector_amd import repeat_detections as RD

    results, sizes = generated_results(args.cameras, args.per_camera, args.large)
    options = RD.RepeatDetectionOptions()
    t0 = time.perf_counter()
    prepared = RD.prepare_results(copy.deepcopy(results), options)
    rows = RD.group_images(prepared['images'], options)
    boxes, where = RD.collect_boxes(prepared['images'], rows, options)
    t_collect = time.perf_counter() - t0
    lib = _lib.load()
    ms = (C.c_float * 3)()
    thr, occ = options.iouThreshold, options.occurrenceThreshold

    gpu_s, host_s, phases, fn_gpu, fn_host = [], [], [], [], []
    same = True
    for it in range(args.rounds + 1):                         # the first round warms both legs up and is not counted
        t0 = time.perf_counter()
        got = RD.match_boxes(boxes, thr, False, occ, backend='gpu', device=args.device)
        t1 = time.perf_counter()
        assert lib.mdhip_repeat_detections_times(ms) == 0
        want = RD.match_boxes(boxes, thr, False, occ, backend='host')
        t2 = time.perf_counter()
        same = same and all(np.array_equal(g, w) for g, w in zip(got, want))
        a = RD.mark_repeat_detections(copy.deepcopy(results), options, backend='gpu', device=args.device) if it == 1 else None
        t3 = time.perf_counter()
        b = RD.mark_repeat_detections(copy.deepcopy(results), options, backend='host') if it == 1 else None
        t4 = time.perf_counter()
        if it >= 1:
            gpu_s.append(t1 - t0)
            host_s.append(t2 - t1)
            phases.append(list(ms))
        if it == 1:
            fn_gpu.append(t3 - t2)
            fn_host.append(t4 - t3)
            same = same and a.detectionResults == b.detectionResults
    med = statistics.median
    n_cand, n_pairs = int(got[0].sum()), len(got[2])
    p = [med(x[i] for x in phases) for i in range(3)]
    lines = [
        'rde_bench: {} cameras of {} detections{}; {} images, {} boxes take part; iouThreshold {}, occurrenceThreshold {}; {} rounds '
        '(median; min), legs alternating'.format(args.cameras, args.per_camera, ' and one of {}'.format(args.large) if args.large else '',
                                                 len(results['images']), len(boxes), thr, occ, args.rounds),
        'device: {}'.format(torch.cuda.get_device_name(args.device)),
        'candidates {}, pairs written {}; both backends gave the same arrays and the same marked results: {}'.format(n_cand, n_pairs, same),
        'mdhip_repeat_detections, the whole call (allocation, upload, kernels, read-back; host clock): {:.1f} ms; {:.1f} ms'.format(
            med(gpu_s) * 1e3, min(gpu_s) * 1e3),
        '  of it on the device (events): resolving the candidates {:.2f} ms, counting the instances {:.2f} ms, writing the pairs {:.2f} ms'.format(*p),
        'mdjpeg_repeat_detections, the host model, one thread (host clock):                            {:.1f} ms; {:.1f} ms'.format(
            med(host_s) * 1e3, min(host_s) * 1e3),
        'whole call, host over gpu: {:.2f}'.format(med(host_s) / med(gpu_s)),
        'filtering and collecting the boxes in Python, common to both: {:.0f} ms'.format(t_collect * 1e3),
        'mark_repeat_detections on the results in memory, once each: gpu {:.0f} ms, host {:.0f} ms (the copy of the results included)'.format(
            fn_gpu[0] * 1e3, fn_host[0] * 1e3),
        'the reference with its quadtree is not measured: its package is not installed, and a stand-in index is no comparison',
    ]
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    assert same, 'the backends disagree'


if __name__ == '__main__':
    main()
