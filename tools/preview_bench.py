"""
Times the annotated previews of a batch of 3-megapixel frames, in one run, both ways over the same generated files and
detections: the host leg (what the reference's visualize_detector_output.py does per image: PIL decodes the file, resizes it
with LANCZOS, draws the boxes and labels, saves the JPEG) and the device leg from images that are in device memory already
(mdhip_resample_lanczos, mdhip_draw_ops and mdhip_jpeg_encode alone, by device events; then the whole of
preview.previews_of_device_images by the host clock, planning and label rasterising on the host included).  Prints the
figures; `--out FILE` also writes them.

usage: python tools/preview_bench.py [--frame 2048x1536] [--width 1000] [--boxes 6] [--images 32] [--rounds 5] [--out profiles/preview.txt]
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
    ap.add_argument('--width', type=int, default=1000)
    ap.add_argument('--boxes', type=int, default=6, help='boxes per image')
    ap.add_argument('--images', type=int, default=32, help='images per call')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from PIL import Image
    from megadetector_amd import preview as P, weights_io, yolo_yaml
    from megadetector_amd.crops import encode_windows
    from megadetector_amd.hip_backend import HipContext

    W, H = (int(v) for v in args.frame.split('x'))
    n = args.images
    rng = np.random.default_rng(1)
    # smooth content with noise on it: what a JPEG codec sees in a photograph matters for the decode and encode legs
    base = np.linspace(0, 255, W)[None, :, None] * np.ones((H, 1, 3)) * 0.7 + rng.normal(0, 12, (H, W, 3))
    frames = [np.clip(base + 3 * i, 0, 255).astype(np.uint8) for i in range(n)]
    del base
    dets = [{'category': str(1 + k % 3), 'conf': round(0.95 - 0.1 * k, 2), 'bbox': [0.05 + 0.14 * k, 0.1 + 0.08 * k, 0.2, 0.3]} for k in range(args.boxes)]
    opt = P.PreviewOptions(output_image_width=args.width)
    size = P.target_size(W, H, opt.output_image_width)
    files = []
    for f in frames:
        bio = io.BytesIO()
        Image.fromarray(f).save(bio, format='JPEG', quality=90)
        files.append(bio.getvalue())
    # the detector sees the DECODED file, so that is what lies in device memory
    frames = [np.array(Image.open(io.BytesIO(b)).convert('RGB')) for b in files]

    def host_leg(data):
        image = Image.open(io.BytesIO(data)).convert('RGB')
        image = image.resize(size, Image.LANCZOS)
        P.render_with_pil(image, dets, opt)
        out = io.BytesIO()
        image.save(out, format='JPEG')
        return out.getvalue()

    ctx = HipContext(weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1), dtype='fp16', max_batch=2, max_h=320, max_w=320)
    dev = [torch.from_numpy(f.reshape(-1)).to('cuda:0') for f in frames]
    entries = [(d, W, H, 'f{}.jpg'.format(i), dets) for i, d in enumerate(dev)]
    plan = P.render_plan(dets, size[0], size[1], opt)
    patches = torch.from_numpy(np.frombuffer(bytes(plan.patches), np.uint8).copy()).to('cuda:0')
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    resample_ms, draw_ms, encode_ms, device_s, host_s = [], [], [], [], []
    k = min(n, 8)                                            # the host leg is slow: a part of the batch a round
    for it in range(args.rounds + 2):
        out = [torch.empty(size[0] * size[1] * 3, dtype=torch.uint8, device='cuda:0') for _ in range(n)]
        torch.cuda.synchronize()
        ev[0].record()
        ctx.resample_lanczos([d.data_ptr() for d in dev], [(W, H)] * n, [W * 3] * n, [o.data_ptr() for o in out], [size] * n, [size[0] * 3] * n)
        ev[1].record()
        ctx.draw_ops([o.data_ptr() for o in out], [size] * n, [size[0] * 3] * n, [i for i in range(n) for _ in plan.ops], plan.ops * n,
                     patches.data_ptr(), len(plan.patches))
        ev[2].record()
        torch.cuda.synchronize()
        ev[3].record()
        encode_windows(ctx, [o.data_ptr() for o in out], [size[0] * 3] * n, [(0, 0) + tuple(size)] * n, opt.quality)
        ev[4].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        made, counts = P.previews_of_device_images(ctx, entries, opt)
        t2 = time.perf_counter()
        host = [host_leg(files[(it * k + j) % n]) for j in range(k)]
        t3 = time.perf_counter()
        if it == 0:
            assert counts == {'gpu': n, 'host': 0, 'skipped': 0}, counts
            assert made[0][0] == host[0], 'the GPU file is not the file the host leg writes'
        if it >= 2:
            resample_ms.append(ev[0].elapsed_time(ev[1]))
            draw_ms.append(ev[1].elapsed_time(ev[2]))
            encode_ms.append(ev[3].elapsed_time(ev[4]))
            device_s.append((t2 - t1) / n)
            host_s.append((t3 - t2) / k)
    med = statistics.median
    lines = [
        'preview_bench: frame {}x{} -> {}x{}, {} boxes with labels per image, quality {}, {} images per call, {} rounds (median; min)'.format(
            W, H, size[0], size[1], args.boxes, opt.quality, n, args.rounds),
        'device: {}'.format(torch.cuda.get_device_name(0)),
        'mdhip_resample_lanczos, both passes (events), per {} images:            {:.3f} ms; {:.3f} ms'.format(n, med(resample_ms), min(resample_ms)),
        'mdhip_draw_ops, {} operations an image (events), per {} images:         {:.3f} ms; {:.3f} ms'.format(len(plan.ops), n, med(draw_ms), min(draw_ms)),
        'mdhip_jpeg_encode with the read-back of the scans (events), per {} images: {:.3f} ms; {:.3f} ms'.format(n, med(encode_ms), min(encode_ms)),
        'device leg end to end (plan + resample + draw + encode + file, host clock): {:.3f} ms an image = {:.1f} files a second'.format(
            med(device_s) * 1e3, 1.0 / med(device_s)),
        'host leg (PIL decode + LANCZOS resize + draw + save, one thread):           {:.3f} ms an image = {:.1f} files a second'.format(
            med(host_s) * 1e3, 1.0 / med(host_s)),
        'the file of image 0 equals the host leg\'s, byte for byte; the device leg starts from pixels that detection has left in device memory',
    ]
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
