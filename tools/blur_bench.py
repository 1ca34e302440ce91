"""
Times the GPU blur of person-sized boxes against Pillow on the host, in one run: mdhip_blur_regions alone, the whole
blurred copy (device copy + blur + mdhip_jpeg_encode of the frame + the file around the scan), and the reference's
blur_detections + save(quality=85) on the same pixels and boxes.  Prints the figures; `--out FILE` also writes them.

usage: python tools/blur_bench.py [--frame 2048x1536] [--box 300x600] [--boxes 2] [--images 8] [--rounds 20] [--out profiles/blur.txt]
"""

import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frame', default='2048x1536')
    ap.add_argument('--box', default='300x600')
    ap.add_argument('--boxes', type=int, default=2, help='boxes per image')
    ap.add_argument('--images', type=int, default=8, help='images per call')
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from PIL import Image, ImageFilter
    from megadetector_amd import blur as B, weights_io, yolo_yaml
    from megadetector_amd.hip_backend import HipContext

    W, H = (int(v) for v in args.frame.split('x'))
    bw, bh = (int(v) for v in args.box.split('x'))
    rng = np.random.default_rng(1)
    # smooth content with noise on it: what a JPEG encoder sees in a photograph matters for the encode leg only
    base = np.linspace(0, 255, W)[None, :, None] * np.ones((H, 1, 3)) * 0.7 + rng.normal(0, 12, (H, W, 3))
    frames = [np.clip(base + 10 * i, 0, 255).astype(np.uint8) for i in range(args.images)]
    rects = [(100 + 700 * k, 200 + 100 * k, 100 + 700 * k + bw, 200 + 100 * k + bh) for k in range(args.boxes)]
    assert all(r[2] <= W and r[3] <= H for r in rects)
    dets = [{'category': '2', 'conf': 0.9 - 0.1 * k, 'bbox': [l / W, t / H, (r - l) / W, (b - t) / H]} for k, (l, t, r, b) in enumerate(rects)]
    opt = B.BlurOptions()
    ids = opt.category_ids()
    assert B.rectangles_to_blur(dets, W, H, opt, ids) == rects

    ctx = HipContext(weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1), dtype='fp16', max_batch=2, max_h=320, max_w=320)
    dev = [torch.from_numpy(f.reshape(-1)).to('cuda:0') for f in frames]
    n = args.images
    rect_image = [i for i in range(n) for _ in rects]
    all_rects = [r for _ in range(n) for r in rects]
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernel_ms, copy_ms, pil_blur_ms, pil_save_ms = [], [], [], []
    for it in range(args.rounds + 2):
        work = [d.clone() for d in dev]
        torch.cuda.synchronize()
        start.record()
        ctx.blur_regions([w.data_ptr() for w in work], [(W, H)] * n, [W * 3] * n, rect_image, all_rects, opt.radius)
        stop.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        files, _ = B.blurred_of_device_images(ctx, [(d, W, H, 'f{}.jpg'.format(i), dets) for i, d in enumerate(dev)], opt, ids)
        t1 = time.perf_counter()
        im = Image.fromarray(frames[it % n])
        t2 = time.perf_counter()
        for l, t, r, b in rects:
            im.paste(im.crop((l, t, r, b)).filter(ImageFilter.GaussianBlur(opt.radius)), (l, t))
        t3 = time.perf_counter()
        bio = io.BytesIO()
        im.save(bio, format='JPEG', quality=opt.quality)
        t4 = time.perf_counter()
        if it == 0:
            assert files[0] is not None and bio.getvalue() == files[0], 'the GPU copy is not the file Pillow writes'
        if it >= 2:
            kernel_ms.append(start.elapsed_time(stop) / n)
            copy_ms.append((t1 - t0) * 1e3 / n)
            pil_blur_ms.append((t3 - t2) * 1e3)
            pil_save_ms.append((t4 - t3) * 1e3)
    med = statistics.median
    lines = [
        'blur_bench: frame {}x{}, {} boxes of {}x{} per image, radius {}, quality {}, {} images per call, {} rounds (median; min)'.format(
            W, H, args.boxes, bw, bh, opt.radius, opt.quality, n, args.rounds),
        'device: {}'.format(torch.cuda.get_device_name(0)),
        'mdhip_blur_regions, kernels only (events), per image:             {:.3f} ms; {:.3f} ms'.format(med(kernel_ms), min(kernel_ms)),
        'blurred copy on the GPU (copy + blur + encode + file, host clock), per image: {:.3f} ms; {:.3f} ms'.format(med(copy_ms), min(copy_ms)),
        'Pillow blur_detections (crop, GaussianBlur, paste), per image:    {:.3f} ms; {:.3f} ms'.format(med(pil_blur_ms), min(pil_blur_ms)),
        'Pillow save(quality={}) of the frame, per image:                  {:.3f} ms; {:.3f} ms'.format(opt.quality, med(pil_save_ms), min(pil_save_ms)),
        'the file of image 0 equals Pillow\'s, byte for byte; the reference also decodes the file a second time (not timed)',
    ]
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
