"""JPEG files for the JPEG-feed tests, written with Pillow at run time from seeded arrays and the bundled images (no JPEG
fixture is committed: the files always match the Pillow that judges them)."""

import os

import numpy as np

from conftest import GOLDEN

SAMPLINGS = ('444', '422', '420', 'gray')
QUALITIES = (30, 75, 95, 100)
RESTARTS = (None, 'rows', 'blocks')           # none / every MCU row / every 3 blocks
ORIENTATIONS = (None, 1, 3, 6, 8)
CONTENTS = ('noise', 'gradient', 'natural')
BUNDLED_JPEG = os.path.join(GOLDEN, 'bundled_images', 'anaconda-prompt-base.jpg')

_natural = {}


def bundled_size():
    from PIL import Image
    with Image.open(BUNDLED_JPEG) as im:
        return im.size


def content(kind, w, h, seed=0):
    """an h x w x 3 uint8 image: noise (all 63 AC coefficients alive), a smooth gradient (DC-only blocks) or a natural image"""
    if kind == 'noise':
        return np.random.default_rng(seed + 7919 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'gradient':
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], -1).astype(np.uint8)
    if kind == 'natural':
        from PIL import Image
        if 'im' not in _natural:
            _natural['im'] = Image.open(BUNDLED_JPEG).convert('RGB')
        im = _natural['im']
        return np.asarray(im if im.size == (w, h) else im.resize((w, h), Image.BILINEAR))
    raise ValueError(kind)


def write_jpeg(path, arr, sampling='420', quality=75, optimize=False, restart=None, orientation=None, **extra):
    from PIL import Image, ImageFile
    im = Image.fromarray(arr)
    kw = dict(quality=quality, optimize=optimize)
    if sampling == 'gray':
        im = im.convert('L')
    else:
        kw['subsampling'] = {'444': 0, '422': 1, '420': 2}[sampling]
    if restart == 'rows':
        kw['restart_marker_rows'] = 1
    elif restart == 'blocks':
        kw['restart_marker_blocks'] = 3
    if orientation is not None:
        exif = Image.Exif()
        exif[274] = orientation
        kw['exif'] = exif
    kw.update(extra)
    # Pillow's encoder writes an optimised or progressive file through ONE buffer of MAXBLOCK bytes
    saved = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(saved, arr.shape[0] * arr.shape[1] * 4 + (1 << 16))
    try:
        im.save(path, 'JPEG', **kw)
    finally:
        ImageFile.MAXBLOCK = saved
    return path


def scan_range(data):
    """(first byte of entropy-coded data, position of the EOI marker) of a single-scan JPEG"""
    p = 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        ln = (data[p + 2] << 8) | data[p + 3]
        if m == 0xDA:
            return p + 2 + ln, data.rindex(b'\xff\xd9')
        p += 2 + ln


def ensure_libmdjpeg():
    """the loaders' decoder is part of the normal build; a tree that was not built yet gets just this (host-only) target"""
    import subprocess
    from conftest import REPO
    from megadetector_amd import jpeg_host
    if not os.path.exists(jpeg_host.LIB_PATH):
        subprocess.check_call(['make', '-C', os.path.join(REPO, 'megadetector_amd', 'csrc'), '../libmdjpeg.so'])
    return jpeg_host
