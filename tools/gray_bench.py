"""
Times the gray-pixel share of a generated folder, in one process: gray_scale.gray_scale_fractions on the device (files decoded on
the GPU, ONE mdhip_gray_count call a decode chunk) against its host leg (the reference's PIL calls per file, one thread), both
warmed, then alternating; the floats of the two legs are compared in every round.  Then mdhip_gray_count on its own: the images
of one decode chunk stay in device memory and the call is repeated between two device events -- the time of a call is what a
caller waits for (the records go up, the counters are zeroed, the kernel runs, the counts come back), and the bytes are the
3 bytes a pixel of the windows, which is all the kernel reads.  The baseline is the host leg: the parent commit has no such tool.
`--out FILE` also writes what is printed.

usage: python tools/gray_bench.py [--files 256] [--width 2048 --height 1536] [--rounds 3] [--calls 200] [--out profiles/gray.txt]
"""

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_RATE_TBS = 5.28                    # profiles/pw_stream.txt (tools/peaks.cpp): the copy ceiling measured for this project


def generate(root, n, width, height, seed=1):
    """day pictures, night pictures (gray) and dusk pictures (gray above some row), 4:2:2 at quality 90"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = np.stack([60 + 120 * xx // width, 180 - 100 * yy // height, 40 + (xx // 16 + yy // 16) % 48], -1).astype(np.int16)
    files = []
    for k in range(n):
        frame = np.clip(base + rng.integers(-6, 7, base.shape, dtype=np.int16) + 3 * (k % 7), 0, 255).astype(np.uint8)
        if k % 3 == 1:
            frame[:] = frame[..., 1:2]
        elif k % 3 == 2:
            rows = int(rng.integers(height // 4, 3 * height // 4))
            frame[:rows] = frame[:rows, :, 1:2]
        path = os.path.join(root, 'IMG_{:04d}.JPG'.format(k))
        Image.fromarray(frame).save(path, quality=90, subsampling=1)
        files.append(path)
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--height', type=int, default=1536)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from megadetector_amd import device_decode, device_render, gray_scale as G
    from megadetector_amd.hip_backend import HipContext
    assert torch.cuda.is_available(), 'this tool measures on a GPU'

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as root:
        files = generate(root, args.files, args.width, args.height)
        ctx = HipContext.for_images(0)
        times, counts, got = {'gpu': [], 'host': []}, {}, {}

        def run(name, profile=False):
            counts[name] = {}
            t0 = time.perf_counter()
            got[name] = G.gray_scale_fractions(files, backend=name, ctx=ctx if name == 'gpu' else None, counts=counts[name], profile=profile)
            dt = time.perf_counter() - t0
            print('    ran {}: {:.3f} s'.format(name, dt), file=sys.stderr, flush=True)
            return dt

        for name in times:                                      # warm: libraries, device context, page cache
            run(name)
        for _ in range(args.rounds):
            for name in times:
                times[name].append(run(name))
            assert [f.hex() for f in got['gpu']] == [f.hex() for f in got['host']], 'the legs disagree'
        plain_counts = dict(counts['gpu'])
        run('gpu', profile=True)
        say('gray-pixel share, {} JPEGs of {} x {} ({:.1f} MP, 4:2:2, quality 90), crop (0.1, 0.1); shares from {:.3f} to {:.3f}; equal floats '
            'in both legs in all {} rounds'.format(args.files, args.width, args.height, args.width * args.height / 1e6, min(got['gpu']),
                                                   max(got['gpu']), args.rounds))
        for name, label in (('gpu', 'gpu'), ('host', 'host x1')):
            med = statistics.median(times[name])
            say('  {:<8} {:8.1f} files/s   (median of {}: {:.3f} s; all: {})'.format(
                label, args.files / med, args.rounds, med, ' '.join('{:.3f}'.format(t) for t in times[name])))
        say('  gpu leg counts: {}'.format(plain_counts))
        say('  gpu leg, one profiled run, waited-for ms per kind of device call: ' +
            ', '.join('{} {:.1f}'.format(k, v) for k, v in sorted(counts['gpu']['ms'].items())))

        # ---- the call on its own: one decode chunk's images stay on the device
        device = torch.device('cuda', 0)
        jobs = [G.plan_file(f, (0.1, 0.1)) for f in files]
        chunk = device_render.chunked(jobs, lambda j: 3 * j['size'][0] * j['size'][1], device_render.DECODE_CHUNK_BYTES)[0]
        pixels, _ = device_decode.decode_scans(ctx, torch, device, [j['scan'] for j in chunk])
        call = ([t.data_ptr() for t in pixels], [j['size'] for j in chunk], [3 * j['size'][0] for j in chunk], [j['window'] for j in chunk])
        nbytes = sum(3 * j['window'][2] * j['window'][3] for j in chunk)
        want = ctx.gray_count(*call)
        for _ in range(10):
            ctx.gray_count(*call)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.calls):
            last = ctx.gray_count(*call)
        end.record()
        torch.cuda.synchronize()
        assert last == want
        window_ms = start.elapsed_time(end)
        per_call = window_ms / args.calls
        say('  mdhip_gray_count alone: {} images of one decode chunk ({:.1f} MB inside the windows), {} calls between two device events: '
            'window {:.1f} ms, {:.3f} ms a call = {:.2f} TB/s read (the project\'s measured copy ceiling: {} TB/s, context not a bar); '
            'a call is upload of the records, zeroing, the kernel and the read-back of the counts, waited for'
            .format(len(chunk), nbytes / 1e6, args.calls, window_ms, per_call, nbytes / per_call / 1e9, COPY_RATE_TBS))
        if per_call < 0.1:
            say('  (a call of under 0.1 ms is mostly launch and copy overhead)')
        ctx.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
