"""
The cases of the fan-out draw (mdhip_draw_ops_from and its host model mdjpeg_draw_from), shared by test_draw_from_cpu.py and
test_gpu_draw_from.py.  A case is a dict:

  sources   [(H x W x 3 uint8 array, bytes a row)]
  dests     [(index of its source, bytes a row, shift)]: the destination begins `shift` bytes behind a 16-byte boundary
            (the sources begin on one)
  op_image, ops, patches   the operations as the call takes them; op_image names a destination

Every image lies in an allocation of its own that is filled with GUARD, with LEAD bytes in front of the image and TAIL
behind it, so that a byte written beside the 3 * width bytes of a row shows.
"""

import numpy as np

GUARD = 0xA5
LEAD = 32                               # a multiple of 16: an allocation's alignment is its image's
TAIL = 48
SIZES = [(1, 1), (5, 3), (7, 5), (33, 17), (131, 67)]          # rows of 3, 15, 21, 99 and 393 bytes: none a multiple of 16
PATCH_W, PATCH_H = 9, 4


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def patch_bytes():
    return bytes((200 + i) & 255 for i in range(PATCH_W * PATCH_H * 3 + 7))


def operations(w, h):
    """per destination of one w x h source its operations: 0 -- rectangles and patches that overlap (the last wins) and hang
    over every edge, and a patch wholly outside; 1 -- none (a copy); 2 -- a rectangle over the whole image, then a patch"""
    pw, ph = PATCH_W, PATCH_H
    return [[[0, -3, -2, w // 2, h // 2, 0x0000FF, 0, 0], [0, w // 3, h // 3, w + 4, h + 9, 0x00FF00, 0, 0],
             [1, -4, h - 2, pw, ph, 7, 0, 0], [1, w - 2, -1, pw, ph, 0, 0, 0], [0, w // 2, 0, w // 2, h - 1, 0x123456, 0, 0],
             [1, w + 1, h + 1, pw, ph, 0, 0, 0], [0, w - 1, h - 1, w - 1, h - 1, 0x0A0B0C, 0, 0]],
            [],
            [[0, -100, -100, 100000, 100000, 0xABCDEF, 0, 0], [1, 0, 0, pw, ph, 3, 0, 0]]]


def case(w, h, pad, shift, n_dests=3, seed=0):
    """n_dests (2 or 3) destinations on one w x h source and one on a second source of 6 x 2 pixels, all in one call; the
    operations of the destinations interleaved in the list"""
    lists = operations(w, h)[:n_dests] + [[[0, 6, 0, 11, 3, 0x111111, 0, 0], [0, 1, 1, 3, 1, 0x222222, 0, 0]]]
    op_image, ops = [], []
    for j in range(max(len(q) for q in lists)):
        for m, q in enumerate(lists):
            if j < len(q):
                op_image.append(m)
                ops.append(q[j])
    return {'sources': [(noise(w, h, 100 + seed), w * 3 + pad), (noise(6, 2, 200 + seed), 18)],
            'dests': [(0, w * 3 + (5 if pad else 0), shift)] * n_dests + [(1, 18 + (5 if pad else 0), shift)],
            'op_image': op_image, 'ops': ops, 'patches': patch_bytes(), 'lists': lists}


def all_cases():
    """every size at both pitches and the four alignments of a destination against its source, two or three destinations"""
    out = []
    for i, (w, h) in enumerate(SIZES):
        for pad in (0, 5):
            for shift in range(4):
                out.append(case(w, h, pad, shift, n_dests=2 + (shift + i) % 2, seed=len(out)))
    return out


def extent(w, h, pitch):
    return pitch * (h - 1) + w * 3


def source_buffers(c):
    """per source its allocation as a host array: the image at LEAD with its pitch, GUARD elsewhere"""
    out = []
    for rgb, pitch in c['sources']:
        h, w = rgb.shape[:2]
        buf = np.full(LEAD + extent(w, h, pitch) + TAIL, GUARD, np.uint8)
        for y in range(h):
            buf[LEAD + y * pitch:LEAD + y * pitch + w * 3] = rgb[y].reshape(-1)
        out.append(buf)
    return out


def dest_buffers(c):
    """per destination its allocation filled with GUARD; the image will begin at LEAD + shift"""
    out = []
    for k, pitch, shift in c['dests']:
        h, w = c['sources'][k][0].shape[:2]
        out.append(np.full(LEAD + shift + extent(w, h, pitch) + TAIL, GUARD, np.uint8))
    return out


def call_arguments(c, src_base, dst_base):
    """the arguments of draw_ops_from (jpeg_host's and HipContext's alike) for allocations at the given base addresses"""
    return ([b + LEAD for b in src_base], [(rgb.shape[1], rgb.shape[0]) for rgb, _ in c['sources']], [p for _, p in c['sources']],
            [b + LEAD + shift for b, (_, _, shift) in zip(dst_base, c['dests'])], [k for k, _, _ in c['dests']],
            [p for _, p, _ in c['dests']], c['op_image'], c['ops'])


def aligned_copy(buf):
    """buf in host memory whose first byte lies on a 16-byte boundary (the view keeps its allocation alive)"""
    raw = np.empty(buf.size + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    view = raw[off:off + buf.size]
    view[:] = buf
    return view


def host_model(c):
    """mdjpeg_draw_from on the case -> (code, the destinations' allocations, the sources' allocations afterwards)"""
    from megadetector_amd import jpeg_host as J
    srcs = [aligned_copy(b) for b in source_buffers(c)]
    dsts = [aligned_copy(b) for b in dest_buffers(c)]
    rc = J.draw_ops_from(*call_arguments(c, [b.ctypes.data for b in srcs], [b.ctypes.data for b in dsts]), c['patches'])
    return rc, dsts, srcs


def copy_then_draw(c):
    """what the destinations' allocations must hold: GUARD, and in the rows the source's pixels under mdjpeg_draw"""
    from megadetector_amd import jpeg_host as J
    out = []
    for (k, pitch, shift), buf, ops in zip(c['dests'], dest_buffers(c), c['lists']):
        img = c['sources'][k][0].copy()
        if ops:
            assert J.draw_ops(img, ops, c['patches']) == J.MDJPEG_OK
        h, w = img.shape[:2]
        for y in range(h):
            buf[LEAD + shift + y * pitch:LEAD + shift + y * pitch + w * 3] = img[y].reshape(-1)
        out.append(buf)
    return out
