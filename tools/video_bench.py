"""
Motion-JPEG video, device decode against host decode: frames per second of process_videos over one generated file.

    python tools/video_bench.py [--frames 300] [--size 1280x720] [--batch 8] [--reps 3] [--model YOLOV5X6_MD] [--dtype bf16]

Generates a 4:2:2 quality-85 MJPEG AVI (frames without Huffman tables, no restart markers, as cameras write them) with the
tests' own writer (tests/avi_fixtures.py), then runs process_videos over it with mjpeg='gpu' and mjpeg='host', alternating,
in one process with ONE detector of seeded weights (as bench.py: no checkpoint is needed), and prints frames/s of both legs,
whether their JSON agrees, and what the two JPEG kernels' calls cost for one batch of the file's frames.
"""

import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def make_video(path, n_frames, width, height, distinct=16):
    """a camera-trap-like clip: a smooth background with texture and a block that moves; `distinct` frames, cycled"""
    import avi_fixtures as AF
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:height, 0:width]
    base = np.stack([xx * 200 // width + 20, yy * 180 // height + 40, (xx + yy) * 160 // (width + height) + 30], -1).astype(np.int16)
    base += rng.integers(-12, 13, base.shape, dtype=np.int16)
    frames = []
    for k in range(distinct):
        f = base.copy()
        x0, y0 = (k * 53) % (width - 200), (k * 29) % (height - 150)
        f[y0:y0 + 150, x0:x0 + 200] = rng.integers(0, 256, (150, 200, 3), dtype=np.int16)
        frames.append(AF.strip_dht(AF.jpeg_bytes(np.clip(f, 0, 255).astype(np.uint8), '422', 85)))
    stored = [frames[i % distinct] for i in range(n_frames)]
    AF.write_avi(path, stored, (width, height), rate=30)
    return sum(len(s) for s in stored) / n_frames


def kernel_times(det, path, batch, reps=5):
    """(entropy-decode ms, reconstruction ms) of one call each for `batch` frames of the file, scans already on the device"""
    import torch
    from megadetector_amd import process_video as PV
    src = PV.MJPEGAVIFrameSource(path, device=True)
    images = [h.materialise() for _, h in zip(range(batch), src)]
    src.close()
    ctx = det._ctx
    scans = [torch.from_numpy(np.array(im.scan_bytes)).cuda() for im in images]
    coefs = [torch.empty(im.coef_count, dtype=torch.int16, device='cuda') for im in images]
    cis = [im.coefficient_image() for im in images]
    outs = [torch.empty(int(np.prod(ci.shape)), dtype=torch.uint8, device='cuda') for ci in cis]
    t_ent, t_rec = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        status = ctx.jpeg_entropy_decode(images, [s.data_ptr() for s in scans], [c.data_ptr() for c in coefs])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ctx.jpeg_reconstruct(cis, [c.data_ptr() for c in coefs], [o.data_ptr() for o in outs])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        assert (status == 0).all()
        t_ent.append((t1 - t0) * 1e3)
        t_rec.append((t2 - t1) * 1e3)
    return float(np.median(t_ent[1:])), float(np.median(t_rec[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--size', default='1280x720')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--frame_sample', type=int, default=1)
    ap.add_argument('--model', default='YOLOV5X6_MD')
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    width, height = (int(v) for v in args.size.split('x'))
    from megadetector_amd import process_video as PV, run_detector
    model = 'synthetic:{}:0'.format(args.model)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'clip.avi')
        mean_bytes = make_video(path, args.frames, width, height)
        say('video: {} frames {}x{} 4:2:2 quality 85 MJPEG AVI, no DHT, no restart markers, {:.0f} bytes / frame'.format(
            args.frames, width, height, mean_bytes))
        det = run_detector.load_detector(model, detector_options={'batch_size': args.batch, 'dtype': args.dtype})
        say('detector: {} seeded weights, {}, batch {}, frame_sample {}'.format(args.model, args.dtype, args.batch, args.frame_sample))
        texts, rates = {}, {'gpu': [], 'host': []}
        real_stdout = sys.stdout
        for rep in range(args.reps + 1):                      # repetition 0 warms both legs up and is not counted
            for leg in ('gpu', 'host'):
                out = os.path.join(tmp, '{}.json'.format(leg))
                sys.stdout = open(os.devnull, 'w')
                try:
                    t0 = time.perf_counter()
                    images = PV.process_videos(model, path, out, frame_sample=args.frame_sample, batch_size=args.batch,
                                               detector=det, mjpeg=leg)
                    el = time.perf_counter() - t0
                finally:
                    sys.stdout.close()
                    sys.stdout = real_stdout
                n = len(images[0]['frames_processed'])
                texts[leg] = re.sub(r'"detection_completion_time": "[^"]*"', '', open(out).read())
                if rep:
                    rates[leg].append(n / el)
                    say("  rep {} mjpeg='{}': {} frames in {:.3f} s = {:.1f} frames/s".format(rep, leg, n, el, n / el))
        ent, rec = kernel_times(det, path, args.batch)
        say('json of the two legs identical: {}'.format(texts['gpu'] == texts['host']))
        say('device leg: entropy decode {:.3f} ms, reconstruction {:.3f} ms per batch of {} frames (one call each, synchronised)'.format(
            ent, rec, args.batch))
        result = {'frames_per_s_gpu': float(np.median(rates['gpu'])), 'frames_per_s_host': float(np.median(rates['host'])),
                  'entropy_ms_per_batch': ent, 'reconstruct_ms_per_batch': rec, 'batch': args.batch, 'frames': args.frames,
                  'size': args.size, 'json_identical': texts['gpu'] == texts['host'],
                  'entropy_decoded': det.jpeg_images_entropy_decoded, 'entropy_fallbacks': det.jpeg_entropy_fallbacks}
        say(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
