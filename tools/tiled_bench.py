"""
Tiles per second of tiled inference on one large image, three ways (a tool, not a test; bench.py is the headline):
  windows: HIPDetector.generate_detections_for_tiles -- the image is uploaded once, tiles are cut on the GPU;
  windows_jpeg: the same with jpeg_quality=95 -- every tile goes through the reference's JPEG round trip on the GPU
           (mdhip_jpeg_recompress); the line also carries the milliseconds its kernels take per 32 tiles (HIP events);
  crops:   np.ascontiguousarray crops of the same image through generate_detections_one_batch -- what a caller could do
           before the windowed letterbox existed.
One synthetic 6000x4000 u8 image (default_rng(0)), seeded YOLOv5x6 weights, 1280 px tiles at overlap 0.5.  Prints one JSON
line per run.  Run each leg in its own process under a time limit:
  timeout -k 10 600 python tools/tiled_bench.py --leg windows && timeout -k 10 600 python tools/tiled_bench.py --leg crops \
    && timeout -k 10 600 python tools/tiled_bench.py --leg windows_jpeg
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=['windows', 'crops', 'windows_jpeg'], required=True)
    ap.add_argument('--repeats', type=int, default=5, help='timed passes over the image')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--dtype', default='fp16')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--model', default='synthetic')
    args = ap.parse_args()
    import torch
    from megadetector_amd.detector import HIPDetector
    from megadetector_amd.run_tiled_inference import get_patch_boundaries
    assert torch.cuda.is_available(), 'tiled_bench needs a GPU'
    img = np.random.default_rng(0).integers(0, 256, (4000, 6000, 3), dtype=np.uint8)
    tile = (1280, 1280)
    origins = [tuple(p) for p in get_patch_boundaries((6000, 4000), tile, (640, 640))]
    ids = ['t{}'.format(i) for i in range(len(origins))]
    det = HIPDetector(args.model, {'batch_size': args.batch, 'dtype': args.dtype, 'device': 'cuda:0'})

    def one_pass():
        if args.leg == 'windows':
            return det.generate_detections_for_tiles(img, origins, tile, tile_ids=ids)
        if args.leg == 'windows_jpeg':
            return det.generate_detections_for_tiles(img, origins, tile, tile_ids=ids, jpeg_quality=95)
        crops = [np.ascontiguousarray(img[y:y + tile[1], x:x + tile[0]]) for x, y in origins]
        return det.generate_detections_one_batch(crops, ids)

    for _ in range(args.warmup):
        res = one_pass()
    assert all(r.get('failure') is None for r in res), [r for r in res if r.get('failure')][:1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.repeats):
        one_pass()                                    # (both calls return host results: the device work has finished)
    dt = time.perf_counter() - t0
    extra = {}
    if args.leg == 'windows_jpeg':                    # the new kernels alone: 32 windows of the device image, HIP events
        parent = torch.from_numpy(img.reshape(-1)).to('cuda:0')
        out = torch.empty(32 * tile[0] * tile[1] * 3, dtype=torch.uint8, device='cuda:0')
        wins = [parent.data_ptr() + y * 6000 * 3 + x * 3 for x, y in origins[:32]]
        outs = [out.data_ptr() + i * tile[0] * tile[1] * 3 for i in range(32)]

        def kernels():
            det._ctx.jpeg_recompress(wins, [tile] * 32, [6000 * 3] * 32, 95, outs)

        kernels()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            kernels()
        e1.record()
        torch.cuda.synchronize()
        extra = {'jpeg_quality': 95, 'recompress_ms_per_32_tiles': round(e0.elapsed_time(e1) / 10, 4)}
    print(json.dumps(dict(extra, **{'tool': 'tiled_bench', 'leg': args.leg, 'image': [6000, 4000], 'tile': list(tile), 'overlap': 0.5,
                      'tiles_per_image': len(origins), 'repeats': args.repeats, 'dtype': args.dtype, 'batch': args.batch,
                      'seconds': round(dt, 4), 'images_per_s': round(args.repeats / dt, 3),
                      'tiles_per_s': round(args.repeats * len(origins) / dt, 2),
                      'detections': sum(len(r['detections']) for r in res)})))


if __name__ == '__main__':
    main()
