"""
The kernel matrix of the thumbnails (mdhip_thumbnails on the GPU, its host model mdjpeg_thumbnails on the CPU), shared by
tests/test_rde_review_cpu.py and tests/test_gpu_rde_review.py: seeded images, crop boxes, output sizes, where every tile goes
in one of three sheets, and what Pillow leaves in those sheets -- image.crop(box).resize((w, h)) + sheet.paste(tile, (x, y)).

A sheet lives in a backing buffer with guard bytes on both sides, an ODD offset of its first pixel and 0, 1 or 7 bytes of
padding behind each row; the buffers start as seeded noise, so comparing a whole buffer with Pillow's also says that no byte
outside the tiles changed.
"""

import numpy as np

SHEET_WIDTH = 96
GUARD = 37                      # odd: the first pixel of a sheet lies at an odd address of an aligned allocation
PADDINGS = (0, 1, 7)


def cases(seed=5):
    """[(image H x W x 3, crop box (x0, y0, x1, y1) in its pixels, (out_w, out_h))]"""
    rng = np.random.default_rng(seed)

    def image(w, h):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)

    def whole(w, h, out):
        return image(w, h), (0, 0, w, h), out

    out = [whole(97, 61, (13, 9)), whole(9, 7, (40, 31)), whole(40, 30, (40, 11)), whole(40, 30, (17, 30)), whole(31, 20, (31, 20)),
           whole(50, 40, (1, 1)), whole(1, 1, (5, 5)),
           # the canvas leaves the image on one side at a time: left, right, top, bottom
           (image(40, 30), (-10, 0, 40, 30), (20, 12)), (image(40, 30), (0, 0, 50, 30), (20, 12)),
           (image(40, 30), (0, -11, 40, 30), (20, 12)), (image(40, 30), (0, 0, 40, 41), (20, 12)),
           # the same with the size kept (a copy with zeros)
           (image(40, 30), (-10, 0, 40, 30), (50, 30)),
           # wholly outside: all zero
           (image(40, 30), (50, 40, 62, 49), (5, 4)),
           # a tap run that crosses strips of the source
           whole(1300, 40, (20, 3))]
    small = image(8, 8)
    out += [(small, (0, 0, 8, 8), (5, 5)) for _ in range(200)]
    return out


def canvas_of(box, width, height):
    """the crop box of an image of width x height as the tile record wants it: (x, y, src_w, src_h) of the rectangle of image
    pixels inside the box -- src_w = src_h = 0 when there is none -- and (canvas_w, canvas_h, off_x, off_y)"""
    x0, y0, x1, y1 = box
    ix0, iy0, ix1, iy1 = max(x0, 0), max(y0, 0), min(x1, width), min(y1, height)
    if ix1 <= ix0 or iy1 <= iy0:
        return (0, 0, 0, 0), (x1 - x0, y1 - y0, 0, 0)
    return (ix0, iy0, ix1 - ix0, iy1 - iy0), (x1 - x0, y1 - y0, ix0 - x0, iy0 - y0)


def place(sizes):
    """Tile i goes to sheet i % 3 (the list interleaves the sheets), packed left to right in rows without gaps, so that
    neighbours touch.  -> ([(sheet, x, y)], [height of each sheet])"""
    x, y, row = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    where = []
    for i, (w, h) in enumerate(sizes):
        s = i % 3
        if x[s] + w > SHEET_WIDTH:
            x[s], y[s], row[s] = 0, y[s] + row[s], 0
        where.append((s, x[s], y[s]))
        x[s] += w
        row[s] = max(row[s], h)
    return where, [y[s] + row[s] for s in range(3)]


class Sheets:
    """the three backing buffers (`backing`, uint8), and per sheet its offset, pitch and height"""

    def __init__(self, heights, seed=9):
        rng = np.random.default_rng(seed)
        self.heights = heights
        self.pitches = [SHEET_WIDTH * 3 + pad for pad in PADDINGS]
        self.backing = [rng.integers(0, 256, GUARD + p * (h - 1) + SHEET_WIDTH * 3 + GUARD, dtype=np.uint8)
                        for p, h in zip(self.pitches, heights)]

    def view(self, s, backing=None):
        """sheet s as an H x W x 3 array with strided rows, over `backing` (default: the sheets' own buffers)"""
        b = self.backing[s] if backing is None else backing
        return np.lib.stride_tricks.as_strided(b[GUARD:], (self.heights[s], SHEET_WIDTH, 3), (self.pitches[s], 3, 1))


def expected(matrix, where, sheets):
    """what Pillow leaves in copies of the backing buffers"""
    from PIL import Image
    out = [b.copy() for b in sheets.backing]
    images = [Image.fromarray(np.ascontiguousarray(sheets.view(s))) for s in range(3)]
    for (pixels, box, size), (s, x, y) in zip(matrix, where):
        images[s].paste(Image.fromarray(pixels).crop(box).resize(size), (x, y))
    for s in range(3):
        sheets.view(s, out[s])[:] = np.asarray(images[s])
    return out
