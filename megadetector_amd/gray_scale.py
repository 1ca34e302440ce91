"""
The share of gray pixels (R == G == B) of images: the reference's way to tell night (infra-red) images from day images when
EXIF says nothing (visualization_utils.gray_scale_fraction), for whole folders.

  gray_scale_fraction(image, crop_size)      the reference's function, restated statement for statement: PIL on the host, one
                                             file.  Image.open WITHOUT the EXIF rotation; mode 'L' or a single band is 1.0 and
                                             nothing is decoded; int(height * crop) rows come off the top and the bottom.
  gray_scale_fractions(filenames, ...)       ours: a list of files -> a list of floats, None where the reference's function
                                             raises for the file (one that does not open, a truncated one).  Every float is
                                             exactly the reference's for that file, on either backend: n_gray / n_pixels of
                                             two integers.

backend='host' calls gray_scale_fraction per file.  backend='gpu' works on a context without a model: the baseline RGB JPEGs
the GPU's decoder takes are decoded in chunks (device_decode.decode_scans: one entropy-decode and one reconstruct call a
chunk) and counted by ONE mdhip_gray_count call a chunk (csrc/gray_kernels.cpp; the statement is csrc/gray_count.h's).  A device
image holds the pixels after the EXIF rotation, which the reference does not apply, so the band of rows the reference keeps
becomes the rectangle of the rotated image that holds the same pixels (window_of); a count does not depend on the order of
its pixels.  The host leg takes, per file and counted: a file that is no RGB JPEG or that the decoder does not take or flags,
a negative crop, a chunk that fails on the device.

The reference loads files that end early (visualization_utils sets ImageFile.LOAD_TRUNCATED_IMAGES when imported).  This package
does not set that flag, so the functions here raise it while a call is inside and put it back after.  The flag is Pillow's and
process-wide: do not run them in a process whose other threads must refuse truncated files at the same time (the detector's
feed, the results-file tools) -- while a call runs, those threads load such files too.

CLI: python -m megadetector_amd.gray_scale FOLDER [--output_csv F --crop_top 0.1 --crop_bottom 0.1 --backend gpu|host --device 0]
"""

import argparse
import os
import sys
import threading
from contextlib import contextmanager

import numpy as np

COUNT_KEYS = ('files', 'gpu', 'host', 'no_decode', 'unreadable', 'files_decoded_gpu', 'files_decoded_pil', 'decode_chunks', 'gray_calls')


_TRUNCATED_LOCK = threading.Lock()
_TRUNCATED_USERS = [0, False]           # calls inside the rule, and the flag's value before the first of them


@contextmanager
def _reference_truncation_rule():
    """The reference's visualization_utils sets ImageFile.LOAD_TRUNCATED_IMAGES = True when it is imported, so its functions
    answer for a file that ends early (Pillow fills what is missing with gray).  This package leaves the flag alone -- its other
    tools treat such a file as a failure -- so it is raised here while at least one call is inside and put back when the last
    one leaves; the calls of a thread pool run side by side."""
    from PIL import ImageFile
    with _TRUNCATED_LOCK:
        if _TRUNCATED_USERS[0] == 0:
            _TRUNCATED_USERS[1] = ImageFile.LOAD_TRUNCATED_IMAGES
            ImageFile.LOAD_TRUNCATED_IMAGES = True
        _TRUNCATED_USERS[0] += 1
    try:
        yield
    finally:
        with _TRUNCATED_LOCK:
            _TRUNCATED_USERS[0] -= 1
            if _TRUNCATED_USERS[0] == 0:
                ImageFile.LOAD_TRUNCATED_IMAGES = _TRUNCATED_USERS[1]


def gray_scale_fraction(image, crop_size=(0.1, 0.1)):
    """reference visualization_utils.py gray_scale_fraction: image is a file name or a PIL image (URLs are not part of this
    package); crop_size the fractions of the height that come off the top and the bottom.  -> the fraction of pixels with
    R == G == B"""
    with _reference_truncation_rule():
        return _gray_scale_fraction(image, crop_size)


def _gray_scale_fraction(image, crop_size):
    from PIL import Image
    if isinstance(image, str):
        image = Image.open(image)

    if image.mode == 'L':
        return 1.0

    if len(image.getbands()) == 1:
        return 1.0

    if crop_size[0] > 0 or crop_size[1] > 0:

        assert (crop_size[0] + crop_size[1]) < 1.0, 'Illegal crop size: {}'.format(str(crop_size))

        top_crop_pixels = int(image.height * crop_size[0])
        bottom_crop_pixels = int(image.height * crop_size[1])

        left = 0
        right = image.width

        first_crop = image.crop((left, top_crop_pixels, right, image.height))
        second_crop = first_crop.crop((left, 0, right, first_crop.height - bottom_crop_pixels))

        image = second_crop

    r = np.array(image.getchannel(0))
    g = np.array(image.getchannel(1))
    b = np.array(image.getchannel(2))

    gray_pixels = np.logical_and(r == g, r == b)
    n_pixels = gray_pixels.size
    n_gray_pixels = gray_pixels.sum()

    return n_gray_pixels / n_pixels


def crop_rows(height, crop_size):
    """(rows off the top, rows off the bottom) of an image of `height` rows, with the reference's statements and its assertion"""
    if crop_size[0] > 0 or crop_size[1] > 0:
        assert (crop_size[0] + crop_size[1]) < 1.0, 'Illegal crop size: {}'.format(str(crop_size))
        return int(height * crop_size[0]), int(height * crop_size[1])
    return 0, 0


def window_of(stored_size, rotation, top, bottom):
    """The rectangle (x, y, w, h) of the image load_image gives -- the stored image turned counter-clockwise by `rotation`
    degrees, as Image.rotate(rotation, expand=True) turns it -- that holds the stored rows top .. height - bottom - 1.
    180: stored row r is row height - 1 - r.  90: stored row r is column r.  270: stored row r is column height - 1 - r."""
    width, height = stored_size
    rows = height - top - bottom
    if rotation == 0:
        return (0, top, width, rows)
    if rotation == 180:
        return (0, bottom, width, rows)
    if rotation == 90:
        return (top, 0, rows, width)
    if rotation == 270:
        return (bottom, 0, rows, width)
    raise ValueError('rotation {}'.format(rotation))


def plan_file(path, crop_size):
    """What the device leg does with a file: None (it does not open), a float (the reference answers without a decode),
    'host' (the host leg takes it), or {'file', 'scan', 'size' (after rotation), 'window', 'pixels'} for the device."""
    from PIL import Image
    from . import jpeg_host
    from .feed import open_for_coefficients
    try:
        image = Image.open(path)
    except Exception:
        return None
    if image.mode == 'L' or len(image.getbands()) == 1:
        return 1.0
    top, bottom = crop_rows(image.height, crop_size)
    if image.format != 'JPEG' or image.mode != 'RGB' or top < 0 or bottom < 0:
        return 'host'
    try:
        _, rotation = open_for_coefficients(path)
        with open(path, 'rb') as f:
            data = f.read()
        if not jpeg_host.parse(data).supported:
            return 'host'
        rc, scan, _ = jpeg_host.ScanImage.from_bytes(data, rotation)
    except Exception:
        return 'host'
    if rc != jpeg_host.MDJPEG_OK or scan is None:
        return 'host'
    width, height = image.size
    size = (height, width) if rotation in (90, 270) else (width, height)
    return {'file': path, 'scan': scan, 'size': size, 'window': window_of((width, height), rotation, top, bottom),
            'pixels': width * (height - top - bottom)}


def _host_fraction(path, crop_size):
    try:
        return float(gray_scale_fraction(path, crop_size))
    except AssertionError:
        raise
    except Exception:
        return None


def gray_scale_fractions(filenames, crop_size=(0.1, 0.1), backend='gpu', device=0, ctx=None, counts=None, profile=False):
    """gray_scale_fraction for every file of `filenames`: -> a list of floats in their order, None where the file does not open
    or does not decode.  counts: a dict that is filled in place with COUNT_KEYS (and, with profile, 'ms' per kind of device
    call).  An illegal crop is the reference's AssertionError."""
    assert backend in ('gpu', 'host'), 'Illegal backend: {}'.format(backend)
    filenames = list(filenames)
    counts = {} if counts is None else counts
    counts.update({k: 0 for k in COUNT_KEYS})
    counts['files'] = len(filenames)
    if profile:
        counts['ms'] = {}
    out = [None] * len(filenames)
    if backend == 'host':
        host = list(range(len(filenames)))
    else:
        host, jobs = [], []
        for i, path in enumerate(filenames):
            plan = plan_file(path, crop_size)
            if plan is None or isinstance(plan, float):
                out[i] = plan
                counts['unreadable'] += plan is None
                counts['no_decode'] += plan is not None
            elif plan == 'host':
                host.append(i)
            else:
                plan['index'] = i
                jobs.append(plan)
        if jobs:
            host += _device_leg(jobs, out, device, ctx, counts, profile)
    for i in sorted(host):
        out[i] = _host_fraction(filenames[i], crop_size)
        counts['host'] += 1
        counts['files_decoded_pil'] += 1
        counts['unreadable'] += out[i] is None
    return out


def _device_leg(jobs, out, device, ctx, counts, profile):
    """the jobs in decode chunks: per chunk one decode and ONE mdhip_gray_count call.  -> the indices the host leg takes"""
    import torch
    from . import device_decode, device_render
    from .hip_backend import HipContext

    def render_chunk(ctx, torch, device, chunk, clock):
        with clock('decode'):
            pixels, _ = device_decode.decode_scans(ctx, torch, device, [j['scan'] for j in chunk])
        done = [(j, t) for j, t in zip(chunk, pixels) if t is not None]
        if done:
            with clock('gray_count'):
                got = ctx.gray_count([t.data_ptr() for _, t in done], [j['size'] for j, _ in done], [3 * j['size'][0] for j, _ in done],
                                     [j['window'] for j, _ in done])
            counts['gray_calls'] += 1
            for (j, _), n_gray in zip(done, got):
                out[j['index']] = n_gray / j['pixels']
            counts['gpu'] += len(done)
            counts['files_decoded_gpu'] += len(done)
        return [j for j, t in zip(chunk, pixels) if t is None]                  # a file the decoder flags

    with HipContext.images_or(ctx, device) as ctx:
        left = device_render.run_chunks(ctx, torch, jobs, lambda j: 3 * j['size'][0] * j['size'][1], render_chunk, counts, profile)
    return [j['index'] for j in left]


def main(argv=None):
    from .ref_utils import find_images
    parser = argparse.ArgumentParser(description='The fraction of gray pixels (R == G == B) of every image of a folder, as CSV')
    parser.add_argument('folder')
    parser.add_argument('--output_csv', default=None, help='the file the rows go to (default: standard output)')
    parser.add_argument('--crop_top', type=float, default=0.1, help='fraction of the height that comes off the top')
    parser.add_argument('--crop_bottom', type=float, default=0.1, help='fraction of the height that comes off the bottom')
    parser.add_argument('--backend', choices=('gpu', 'host'), default='gpu')
    parser.add_argument('--device', type=int, default=0)
    args = parser.parse_args(argv)
    files = find_images(args.folder, recursive=True)
    counts = {}
    fractions = gray_scale_fractions(files, (args.crop_top, args.crop_bottom), backend=args.backend, device=args.device, counts=counts)
    lines = ['image,gray_scale_fraction']
    for path, fraction in zip(files, fractions):
        relative = os.path.relpath(path, args.folder).replace('\\', '/')
        lines.append('{},{}'.format('"{}"'.format(relative.replace('"', '""')) if any(c in relative for c in ',"\n') else relative,
                                    '' if fraction is None else repr(fraction)))
    text = '\n'.join(lines) + '\n'
    if args.output_csv:
        with open(args.output_csv, 'w', newline='') as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print('{} files: {} on the device, {} on the host, {} unreadable'.format(counts['files'], counts['gpu'], counts['host'],
                                                                               counts['unreadable']), file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
