"""
Measures the GPU JPEG feed (run_detector_batch --gpu_jpeg / --gpu_jpeg_entropy), each figure next to its baseline from
the same run.

  host (no GPU needed)   per file, single thread, same process, the loader's work in its three modes: np.asarray(load_image(f))
                         (PIL's full decode), mdjpeg_parse + mdjpeg_decode (entropy decode only, --gpu_jpeg), and
                         mdjpeg_parse + mdjpeg_scan + the copy of the file into a slot (no symbol decoded,
                         --gpu_jpeg_entropy); median and quartiles of >= 20 repeats, the three modes interleaved repeat by
                         repeat, on JPEGs written here with Pillow from seeded images at 3 MP (4:2:0 and 4:2:2, quality
                         75 / 90 / 95, with and without restart markers)
  --gpu                  the kernels alone, batch 32: mdhip_jpeg_entropy_decode (whole call, it returns when the planes are
                         written; with the subsequences, repeated decodes and pass-2 launches it needed) and
                         mdhip_jpeg_reconstruct (events on the stream); and the end-to-end run_detector_batch rate without
                         a switch, with gpu_jpeg and with gpu_jpeg='entropy' on the same files with the same number of
                         loader processes, interleaved

    python tools/jpeg_feed_bench.py [--gpu] [--out profiles/jpeg_feed.txt] [--files 64] [--loader_workers 12]
"""

import argparse
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W3MP, H3MP = 2048, 1536


def seeded_image(seed, w=W3MP, h=H3MP):
    """a camera-like frame: smooth large structures plus fine texture and sensor noise (so that AC coefficients are alive)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 3), np.float32)
    for c in range(3):
        acc = 110 + 60 * np.sin(xx / (90 + 40 * c) + seed) * np.cos(yy / (70 + 25 * c))
        coarse = rng.integers(0, 256, (h // 32 + 2, w // 32 + 2)).astype(np.float32)
        acc += 0.35 * (np.kron(coarse, np.ones((32, 32), np.float32))[:h, :w] - 128)
        fine = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1)).astype(np.float32)
        acc += 0.12 * (np.kron(fine, np.ones((4, 4), np.float32))[:h, :w] - 128)
        acc += rng.normal(0, 3.0, (h, w))
        img[..., c] = acc
    return np.clip(img, 0, 255).astype(np.uint8)


def write_files(folder, n, variants):
    """variants: (subsampling, quality) or (subsampling, quality, restart_marker_rows)"""
    from PIL import Image
    out = []
    for i in range(n):
        sub, q = variants[i % len(variants)][:2]
        rst = variants[i % len(variants)][2] if len(variants[i % len(variants)]) > 2 else 0
        p = os.path.join(folder, 'f{:03d}_{}_q{}{}.jpg'.format(i, '420' if sub == 2 else '422', q, '_rst' if rst else ''))
        kw = {'restart_marker_rows': rst} if rst else {}
        Image.fromarray(seeded_image(i % 8)).save(p, 'JPEG', quality=q, subsampling=sub, **kw)
        out.append(p)
    return out


def median_ms(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def interleaved_ms(fns, repeats):
    """times the callables in turn, repeat by repeat; -> per callable (median, lower quartile, upper quartile) in ms"""
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return [tuple(float(np.percentile(t, q)) for q in (50, 25, 75)) for t in ts]


def host_part(folder, repeats, say):
    from megadetector_amd import jpeg_host
    from megadetector_amd.feed import load_image
    say('host, one thread, {} repeats per file with the three modes interleaved, {} x {} pixels; median [quartiles] in ms'.format(
        repeats, W3MP, H3MP))
    say('{:<8} {:>4} {:>4} {:>10}  {:>22} {:>22} {:>22} {:>10} {:>12}'.format(
        'sampling', 'q', 'rst', 'file bytes', 'PIL full decode', 'coefficients (--gpu_jpeg)', 'scan (--gpu_jpeg_entropy)', 'coef/scan',
        'margin ms'))
    rows = []
    for sub, q, rst in [(2, 75, 0), (2, 90, 0), (2, 95, 0), (1, 75, 0), (1, 90, 0), (1, 95, 0), (2, 75, 1), (2, 90, 1), (2, 95, 1), (1, 90, 1)]:
        p = write_files(folder, 1, [(sub, q, rst)])[0]
        data = open(p, 'rb').read()
        hd = jpeg_host.parse(data)
        buf = np.empty(hd.coef_count, dtype=np.int16)
        slot = np.empty(jpeg_host.SLOT_HEADER_BYTES + 2 * hd.coef_count, dtype=np.uint8)

        def coefficients():
            assert jpeg_host.parse(data).supported
            rc, _, _ = jpeg_host.decode(data, out=buf)
            assert rc == 0

        def scan():
            assert jpeg_host.parse(data).supported
            assert jpeg_host.scan_into_slot(data, slot, 0) == 0

        t_pil, t_coef, t_scan = interleaved_ms([lambda: np.asarray(load_image(p)), coefficients, scan], repeats)
        # the margin: the slower quartile of the scan leg against the faster quartile of the coefficient leg
        margin = t_coef[1] - t_scan[2]
        rows.append((sub, q, rst, t_pil, t_coef, t_scan, margin))
        fmt = lambda t: '{:8.2f} [{:6.2f} {:6.2f}]'.format(*t)
        say('{:<8} {:>4} {:>4} {:>10}  {:>22} {:>22} {:>22} {:>10.1f} {:>12.2f}'.format(
            '4:2:0' if sub == 2 else '4:2:2', q, 'rows' if rst else '-', len(data), fmt(t_pil), fmt(t_coef), fmt(t_scan),
            t_coef[0] / t_scan[0], margin))
    say('margin = lower quartile of the coefficient leg minus upper quartile of the scan leg: positive means the scan mode is '
        'faster by more than the spread of both')
    return rows


def gpu_part(folder, n_files, loader_workers, say):
    import torch
    from megadetector_amd import feed, jpeg_host, run_detector, run_detector_batch as RDB
    from megadetector_amd.jpeg_host import CoefficientImage
    files = write_files(folder, n_files, [(2, 90), (1, 90), (2, 75), (2, 95), (2, 90, 1), (1, 75), (2, 75, 1), (1, 95)])
    det = run_detector.load_detector('synthetic', detector_options={'batch_size': 32})
    ctx = det._ctx
    # --- the kernels alone: 32 images resident on the device
    images, coefs, outs = [], [], []
    for f in files[:32]:
        rc, hd, coef = jpeg_host.decode(open(f, 'rb').read())
        assert rc == 0
        im = CoefficientImage.from_header(hd, coef, 0)
        images.append(im)
        coefs.append(torch.from_numpy(coef).cuda())
        outs.append(torch.empty(int(np.prod(im.shape)), dtype=torch.uint8, device='cuda'))
    s = torch.cuda.current_stream()
    cp, op = [c.data_ptr() for c in coefs], [o.data_ptr() for o in outs]
    for _ in range(3):
        ctx.jpeg_reconstruct(images, cp, op, stream=s.cuda_stream)
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        ctx.jpeg_reconstruct(images, cp, op, stream=s.cuda_stream)
        b.record(s)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    px = sum(int(np.prod(im.shape[:2])) for im in images)
    say('')
    say('kernels alone: mdhip_jpeg_reconstruct of {} images ({:.1f} MP): median {:.3f} ms, min {:.3f} ms per call '
        '(20 calls, events on the stream)'.format(len(images), px / 1e6, float(np.median(ts)), min(ts)))
    want = np.asarray(feed.load_image(files[0]))
    assert np.array_equal(outs[0].cpu().numpy().reshape(want.shape), want), 'reconstruction differs from PIL'
    # --- the entropy kernels alone: the same 32 files as compressed scans resident on the device
    scans = []
    for f in files[:32]:
        rc, si, why = jpeg_host.ScanImage.from_bytes(open(f, 'rb').read())
        assert rc == 0, why
        scans.append(si)
    dscan = [torch.from_numpy(np.array(si.scan_bytes)).cuda() for si in scans]
    sp = [t.data_ptr() for t in dscan]
    torch.cuda.synchronize()
    for bits in (1024, 512, 2048):
        for _ in range(2):
            status = ctx.jpeg_entropy_decode(scans, sp, cp, bits, stream=s.cuda_stream)
        assert (status == 0).all()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            ctx.jpeg_entropy_decode(scans, sp, cp, bits, stream=s.cuda_stream)
            ts.append((time.perf_counter() - t0) * 1e3)
        st = ctx.jpeg_entropy_stats()
        say('kernels alone: mdhip_jpeg_entropy_decode of {} images, {} scan bytes, subsequences of {} bits: median {:.3f} ms, min '
            '{:.3f} ms per call (10 calls, host clock around the synchronous call: upload of the descriptors, all passes, '
            'status read-back); {} subsequences, {:.2f} decodes per subsequence in pass 2, {} pass-2 launches'.format(
                len(scans), sum(si.nbytes for si in scans), bits, float(np.median(ts)), min(ts), st['subsequences'],
                st['decoded_again'] / max(st['subsequences'], 1), st['sync_launches']))
    ctx.jpeg_entropy_decode(scans, sp, cp, 0, stream=s.cuda_stream)
    for c, im, f in list(zip(coefs, images, files))[:4]:
        assert np.array_equal(c.cpu().numpy(), np.asarray(im.coef)), 'entropy decode differs from mdjpeg_decode: ' + f
    del coefs, outs, dscan
    # --- end to end
    say('')
    say('end to end: run_detector_batch, {} files of 3 MP, batch 32, {} loader processes, shared ring'.format(len(files), loader_workers))
    for gpu_jpeg in (False, True, 'entropy', False, True, 'entropy'):
        t0 = time.perf_counter()
        res = RDB.load_and_run_detector_batch('synthetic', files, quiet=True, detector=det, batch_size=32, use_image_queue=True,
                                              use_threads_for_queue=False, loader_workers=loader_workers, gpu_jpeg=gpu_jpeg)
        dt = time.perf_counter() - t0
        assert len(res) == len(files) and not any('failure' in r for r in res)
        say('  gpu_jpeg={!s:<8}  {:.2f} s  {:.1f} images/s (includes starting the loader processes)  feed {}'.format(
            gpu_jpeg, dt, len(files) / dt, dict(RDB.last_feed_counts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpu', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'jpeg_feed.txt'))
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--loader_workers', type=int, default=12)
    args = ap.parse_args()
    assert args.repeats >= 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from PIL import features
    import PIL
    say('# tools/jpeg_feed_bench.py{}   Pillow {} (libjpeg-turbo {})'.format(' --gpu' if args.gpu else '', PIL.__version__,
                                                                          features.version('jpg')))
    with tempfile.TemporaryDirectory() as folder:
        host_part(folder, args.repeats, say)
        if args.gpu:
            gpu_part(folder, args.files, args.loader_workers, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
