"""
Times the classifier input of a batch of 3-megapixel frames, in one run, over the same generated frames and boxes:
mdhip_classifier_input alone (device events) beside mdhip_resample_lanczos of the same windows to the same sizes (the
two-launch resize the previews use: more taps, an image between the passes, no normalisation); the device leg end to end
by the host clock (classify.classifications_of_device_images without a model -- the tensor alone -- and with a conv-free
model); and the host leg (PIL crop + resize + normalise, one thread) on the same crops.  Prints the figures; `--out FILE` also
writes them.

usage: python tools/classify_bench.py [--frame 2048x1536] [--size 224] [--boxes 6] [--images 32] [--rounds 5] [--out profiles/classify.txt]
"""

import argparse
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
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--boxes', type=int, default=6, help='boxes per image')
    ap.add_argument('--images', type=int, default=32, help='images per call')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from megadetector_amd import classify as K, weights_io, yolo_yaml
    from megadetector_amd.crops import device_stream
    from megadetector_amd.hip_backend import HipContext

    W, H = (int(v) for v in args.frame.split('x'))
    n, S = args.images, args.size
    rng = np.random.default_rng(1)
    base = np.linspace(0, 255, W)[None, :, None] * np.ones((H, 1, 3)) * 0.7 + rng.normal(0, 12, (H, W, 3))
    frames = [np.clip(base + 3 * i, 0, 255).astype(np.uint8) for i in range(n)]
    del base
    # boxes of growing size, from a reduction of about 1.4 to about 4.5 at 224; the last one leaves the square at the border
    dets = [{'category': '1', 'conf': round(0.95 - 0.1 * k, 2), 'bbox': [0.03 + 0.1 * k, 0.05 + 0.05 * k, 0.12 + 0.07 * k, 0.2 + 0.09 * k]}
            for k in range(args.boxes)]

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(3)
            self.pool, self.flat, self.fc = torch.nn.AdaptiveAvgPool2d(4), torch.nn.Flatten(), torch.nn.Linear(48, 5)

        def forward(self, x):
            return self.fc(self.flat(self.pool(x)))

    opt = K.ClassifyOptions(Model(), image_size=S, batch_size=n * args.boxes)
    picked, skipped = K.pick_crops(dets, W, H, opt)
    assert not skipped and all(c[4] is not None for _, c in picked)
    canvases = [c for _, c in picked]

    ctx = HipContext(weights_io.synthetic_weights(yolo_yaml.YOLOV5N6_TEST, seed=1), dtype='fp16', max_batch=2, max_h=320, max_w=320)
    dev = [torch.from_numpy(f.reshape(-1)).to('cuda:0') for f in frames]
    entries = [(d, W, H, 'f{}.jpg'.format(i), dets) for i, d in enumerate(dev)]
    jobs = [(d, W, c) for d in dev for c in canvases]
    m = len(jobs)
    recs = [(t.data_ptr() + y0 * w * 3 + x0 * 3, w * 3, x1 - x0, y1 - y0, cw, ch, ox, oy) for t, w, (cw, ch, ox, oy, (x0, y0, x1, y1)) in jobs]
    # the baseline: the windows (the part of each canvas that holds pixels) to the size the canvas is resized to
    sizes = [K.resized_geometry(c[0], c[1], S)[:2] for _, _, c in jobs]
    x = torch.empty((m, 3, S, S), dtype=torch.float32, device='cuda:0')
    outs = [torch.empty(w * h * 3, dtype=torch.uint8, device='cuda:0') for w, h in sizes]
    ext = device_stream(0, dev[0].device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    kernel_ms, lanczos_ms, tensor_s, model_s, host_s = [], [], [], [], []
    k = min(m, 24)                                           # the host leg is slow: a part of the crops a round
    for it in range(args.rounds + 2):
        torch.cuda.synchronize()
        ev[0].record()
        assert ctx.classifier_input(recs, S, x.data_ptr(), opt.filter, opt.mean, opt.std)
        ev[1].record()
        ctx.resample_lanczos([r[0] for r in recs], [(r[2], r[3]) for r in recs], [r[1] for r in recs], [o.data_ptr() for o in outs], sizes,
                             [w * 3 for w, _ in sizes])
        ev[2].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        made = K.classifier_inputs_of_device_images(ctx, jobs, opt, ext)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lists, counts = K.classifications_of_device_images(ctx, entries, opt)
        t2 = time.perf_counter()
        host = [K.classifier_input_host(frames[((it * k + j) // len(canvases)) % n], canvases[(it * k + j) % len(canvases)], opt) for j in range(k)]
        t3 = time.perf_counter()
        if it == 0:
            assert counts == {'gpu': m, 'host': 0, 'skipped': 0}, counts
            want = K.classifier_input_host(frames[0], canvases[0], opt)
            assert np.array_equal(made[0].cpu().numpy().view(np.uint32), want.view(np.uint32)), 'the tensor is not the host leg\'s'
        if it >= 2:
            kernel_ms.append(ev[0].elapsed_time(ev[1]))
            lanczos_ms.append(ev[1].elapsed_time(ev[2]))
            tensor_s.append((t1 - t0) / m)
            model_s.append((t2 - t1) / m)
            host_s.append((t3 - t2) / k)
    med = statistics.median
    lines = [
        'classify_bench: frame {}x{}, {} boxes per image (canvases {}), size {}, bicubic, {} images = {} crops per call, {} rounds (median; min)'.format(
            W, H, args.boxes, ', '.join('{}x{}'.format(c[0], c[1]) for c in canvases), S, n, m, args.rounds),
        'device: {}'.format(torch.cuda.get_device_name(0)),
        'mdhip_classifier_input, one launch (events), per {} crops:                         {:.3f} ms; {:.3f} ms'.format(m, med(kernel_ms), min(kernel_ms)),
        'mdhip_resample_lanczos of the same windows to the same sizes, two launches (events): {:.3f} ms; {:.3f} ms'.format(med(lanczos_ms), min(lanczos_ms)),
        'device leg, the tensor alone (records + kernel, host clock):         {:.4f} ms a crop = {:.0f} crops a second'.format(
            med(tensor_s) * 1e3, 1.0 / med(tensor_s)),
        'device leg end to end with the conv-free model and the lists (host clock): {:.4f} ms a crop = {:.0f} crops a second'.format(
            med(model_s) * 1e3, 1.0 / med(model_s)),
        'host leg (PIL crop + bicubic resize + normalise, one thread, no model):     {:.4f} ms a crop = {:.0f} crops a second'.format(
            med(host_s) * 1e3, 1.0 / med(host_s)),
        'the tensor of crop 0 equals the host leg\'s, bit for bit; the device leg starts from pixels that detection has left in device memory',
    ]
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
