"""
The case list of the gray-pixel count (tests/test_gray_cpu.py for the host model, tests/test_gpu_gray.py for the kernel): small
images that lie at a byte offset inside a sentinel-filled allocation, with a tight or a padded pitch, so that a byte read
outside the 3 * w bytes of a window's rows shows as a miscount.

A case is {'name', 'w', 'h', 'offset', 'pitch', 'window', 'sentinel', 'buffer' (uint8, the whole allocation), 'want'}: the image's
first pixel is buffer[offset], row y starts at buffer[offset + y * pitch]; every byte of the buffer that belongs to no pixel
holds the sentinel -- 0x55 everywhere looks gray, the other pattern (a counter that never repeats within three bytes) does not,
so a read outside miscounts one way or the other.  `want` comes from numpy on the pixel arrays, never from the code under test.
"""

import numpy as np

WIDTHS = (1, 5, 15, 16, 17, 33)
HEIGHTS = (1, 2)
OFFSETS = (0, 1, 3, 7)
GUARD = 64                                      # sentinel bytes before and behind every image


def _fill(n, gray_sentinel):
    if gray_sentinel:
        return np.full(n, 0x55, np.uint8)
    return (np.arange(n) % 251 + 1).astype(np.uint8)            # three neighbours are never equal


def place(pixels, offset, pad, gray_sentinel):
    """pixels (h, w, 3) at byte `offset` behind the guard of a fresh buffer, rows pad bytes apart -> (buffer, offset, pitch)"""
    h, w, _ = pixels.shape
    pitch = 3 * w + pad
    start = GUARD + offset
    buffer = _fill(start + (h - 1) * pitch + 3 * w + GUARD, gray_sentinel)
    for y in range(h):
        buffer[start + y * pitch:start + y * pitch + 3 * w] = pixels[y].reshape(-1)
    return buffer, start, pitch


def view(case):
    """the case's image as an (h, w, 3) view of its buffer (strides (pitch, 3, 1)): what jpeg_host.gray_count takes"""
    return np.lib.stride_tricks.as_strided(case['buffer'][case['offset']:], (case['h'], case['w'], 3), (case['pitch'], 3, 1), writeable=False)


def count(pixels, window):
    x, y, w, h = window
    p = pixels[y:y + h, x:x + w].astype(np.int32)
    return int(np.logical_and(p[..., 0] == p[..., 1], p[..., 0] == p[..., 2]).sum())


def _case(name, pixels, offset, pad, window, gray_sentinel):
    buffer, start, pitch = place(pixels, offset, pad, gray_sentinel)
    h, w, _ = pixels.shape
    return {'name': '{} {}x{} +{} pad {} window {} sentinel {}'.format(name, w, h, offset, pad, window, 'gray' if gray_sentinel else 'colour'),
            'w': w, 'h': h, 'offset': start, 'pitch': pitch, 'window': tuple(window), 'sentinel': gray_sentinel, 'buffer': buffer,
            'want': count(pixels, window)}


def cases():
    rng = np.random.default_rng(77)
    out = []
    for w in WIDTHS:
        for h in HEIGHTS:
            for offset in OFFSETS:
                for pad in (0, 5 if w % 2 else 4):              # tight (3 * w: odd for an odd w), and padded to another parity
                    for gray_sentinel in (True, False):
                        # random: about half the pixels gray, the others off by one in one channel
                        base = rng.integers(0, 256, (h, w, 1)).astype(np.uint8).repeat(3, axis=2)
                        off = rng.integers(0, 6, (h, w))
                        for c in range(3):
                            base[..., c] ^= (off == c + 1).astype(np.uint8)
                        windows = [(0, 0, w, h)] + ([(1, 0, w - 1, h)] if w > 1 else []) + ([(5, h - 1, w - 5, 1)] if w > 5 else [])
                        for window in windows:
                            out.append(_case('random', base, offset, pad, window, gray_sentinel))
                        # all gray: the count is w * h
                        gray = rng.integers(0, 256, (h, w, 1)).astype(np.uint8).repeat(3, axis=2)
                        out.append(_case('all gray', gray, offset, pad, (0, 0, w, h), gray_sentinel))
                        # one pixel that is not gray: each corner, and pixel 5 of a row (bytes 15 .. 17 straddle a 16-byte line)
                        spots = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)} | ({(5, h - 1)} if w > 5 else set())
                        for k, (x, y) in enumerate(sorted(spots)):
                            one = gray.copy()
                            one[y, x, k % 3] ^= 0x80
                            out.append(_case('one at ({}, {})'.format(x, y), one, offset, pad, (0, 0, w, h), gray_sentinel))
    return out


def many(n=24):
    """n images of different sizes for ONE call, among them one that is much larger than the others (several workgroups,
    strides of the grid) and one of a single pixel"""
    rng = np.random.default_rng(78)
    out = []
    for k in range(n):
        w, h = (1, 1) if k == 0 else (1203, 517) if k == 7 else (int(rng.integers(2, 90)), int(rng.integers(1, 40)))
        base = rng.integers(0, 256, (h, w, 1)).astype(np.uint8).repeat(3, axis=2)
        base[..., 1] ^= (rng.integers(0, 3, (h, w)) == 0).astype(np.uint8)
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        window = (x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))) if k % 2 else (0, 0, w, h)
        out.append(_case('many {}'.format(k), base, int(rng.integers(0, 8)), int(rng.integers(0, 7)), window, bool(k % 3)))
    return out
