"""
Resizing a folder of images before it is shared, labelled or zipped: the reference's visualization_utils.resize_image,
resize_images and resize_image_folder, with its argument names and defaults, on two legs that write the same bytes.

Restated statement for statement: the size rule (int(target_width / (w / h)) and int((w / h) * target_height), in floats), None
as -1, the three ways to "no resize" ((-1, -1), no_enlarge_width, already that size) which all WRITE the unresized image, the
assertion `Invalid image resize target`, which becomes that file's 'error', 'skipped' for an existing target without
overwrite, os.makedirs of the target's folder, the enumeration of path_utils.find_images (recursive glob of *.*, the
reference's extension list, sorted, relative, forward slashes), output_folder None as resizing in place, the assertion on
pool_type, and exif_preserving_save with its quirks (ref_utils.exif_preserving_save): a resized, rotated or
converted image has no format, so quality 'keep' becomes 85 at 4:2:0 and an integer quality is passed through; an unresized
plain RGB JPEG keeps its format, so 'keep' re-encodes it with the source's own tables and sampling; the EXIF block is the
image's getexif() as Pillow serialises it, the Orientation tag of a file load_image turned included.  The reference loads
files that end early (it sets ImageFile.LOAD_TRUNCATED_IMAGES when imported); so do both legs here, for the length of a call.

backend='host' makes exactly the reference's PIL calls, in the reference's pool.  backend='gpu' works on a context without a
model: the files in input order in decode chunks (device_render.chunked), each decoded once on the device; per chunk ONE
mdhip_resample_lanczos call for the files whose size changes and ONE mdhip_jpeg_encode_sampled call for all of them (quality
tables at 4:2:0, or an unresized plain JPEG's own tables and sampling); jpeg_host.sampled_file writes each file.  All inputs of
a chunk are read before any of its outputs is written, which resizing in place depends on.  The host leg takes, per file and
counted: a file the device does not decode, an output name Pillow does not save as JPEG, a side above 65535, a quality whose
tables jpeg_host.quant_tables does not give, a source whose tables or sampling sampled_file does not write, a chunk that fails
on the device, and every file for which anything raises -- so an 'error' string is always the one PIL raised.

The reference loads files that end early (visualization_utils sets ImageFile.LOAD_TRUNCATED_IMAGES when imported).  This package
does not set that flag, so the functions here raise it while a call is inside and put it back after.  The flag is Pillow's and
process-wide: do not run them in a process whose other threads must refuse truncated files at the same time (the detector's
feed, the results-file tools) -- while a call runs, those threads load such files too.

CLI: python -m megadetector_amd.resize_images INPUT_FOLDER [OUTPUT_FOLDER] --target_width W --target_height H
         [--no_enlarge_width --quality keep|Q --no_recursive --no_overwrite --n_workers N --backend gpu|host --device 0]
"""

import argparse
import os
import sys
from functools import partial

from . import device_render as DR
from .gray_scale import _reference_truncation_rule
from .preview import HostLeg
from .ref_utils import DEFAULT_SAVE_QUALITY as DEFAULT_QUALITY
from .ref_utils import exif_preserving_save, quality_argument
from .ref_utils import find_images as _find_images

#: path_utils.find_images(dirname, recursive, return_relative_paths=True, convert_slashes=True)
find_images = partial(_find_images, return_relative_paths=True)
COUNT_KEYS = ('files', 'resized', 'unresized', 'skipped', 'errors', 'gpu', 'host', 'files_decoded_gpu', 'files_decoded_pil',
              'decode_chunks', 'resample_calls', 'encode_calls')


def resize_target(size, target_width=-1, target_height=-1, no_enlarge_width=False):
    """resize_image's decision for an image of `size` (width, height): -> (target_width, target_height, resize_required), the
    reference's statements in the reference's order.  The assertion on the target is the caller's, as in the reference."""
    if target_width is None:
        target_width = -1
    if target_height is None:
        target_height = -1
    resize_required = True
    if target_width == -1 and target_height == -1:
        resize_required = False
    elif target_width == -1 or target_height == -1:
        aspect_ratio = size[0] / size[1]
        if target_width != -1:
            target_height = int(target_width / aspect_ratio)
        else:
            target_width = int(aspect_ratio * target_height)
    if (no_enlarge_width) and (target_width > size[0]):
        resize_required = False
    if (target_width == size[0]) and (target_height == size[1]):
        resize_required = False
    return target_width, target_height, resize_required


def _resize_image(image, target_width, target_height, output_file, no_enlarge_width, verbose, quality):
    """resize_image; -> (the image it returns, whether it resized)"""
    from PIL import Image
    from .feed import load_image
    image_fn = 'in_memory'
    if isinstance(image, str):
        image_fn = image
        image = load_image(image)
    target_width, target_height, resize_required = resize_target(image.size, target_width, target_height, no_enlarge_width)
    if verbose and no_enlarge_width and target_width > image.size[0]:
        print('Bypassing image enlarge for {} --> {}'.format(image_fn, str(output_file)))
    if not resize_required:
        if output_file is not None:
            if verbose:
                print('No resize required for resize {} --> {}'.format(image_fn, str(output_file)))
            exif_preserving_save(image, output_file, quality=quality)
        return image, False
    assert target_width > 0 and target_height > 0, 'Invalid image resize target {},{}'.format(target_width, target_height)
    resized_image = image.resize((target_width, target_height), Image.Resampling.LANCZOS)
    if output_file is not None:
        exif_preserving_save(resized_image, output_file, quality=quality)
    return resized_image, True


def resize_image(image, target_width=-1, target_height=-1, output_file=None, no_enlarge_width=False, verbose=False, quality='keep'):
    """visualization_utils.resize_image: image is a PIL image or a file name (URLs are not part of this package).  Always PIL:
    this is the host leg's unit.  -> the resized image, or the image itself when no resize is required"""
    with _reference_truncation_rule():
        return _resize_image(image, target_width, target_height, output_file, no_enlarge_width, verbose, quality)[0]


def _result(input_fn, output_fn, status, error=None):
    return {'input_fn': input_fn, 'output_fn': output_fn, 'status': status, 'error': error}


def _resize_absolute_image(input_output_files, target_width, target_height, no_enlarge_width, verbose, quality, overwrite):
    """the reference's wrapper of the same name; -> (its result dict, None or whether the file was resized)"""
    input_fn_abs, output_fn_abs = input_output_files
    error, resized = None, None
    if (not overwrite) and (os.path.isfile(output_fn_abs)):
        status = 'skipped'
    else:
        os.makedirs(os.path.dirname(output_fn_abs), exist_ok=True)
        try:
            with _reference_truncation_rule():
                _, resized = _resize_image(input_fn_abs, target_width, target_height, output_fn_abs, no_enlarge_width, verbose, quality)
            status = 'success'
        except Exception as e:
            if verbose:
                print('Error resizing {}: {}'.format(input_fn_abs, str(e)))
            status = 'error'
            error = str(e)
    return _result(input_fn_abs, output_fn_abs, status, error), resized


def _count_result(counts, result, resized):
    if result['status'] == 'skipped':
        counts['skipped'] += 1
    elif result['status'] == 'error':
        counts['errors'] += 1
    else:
        counts['resized' if resized else 'unresized'] += 1


# ---- the device leg ----------------------------------------------------------------------------------------------------------------

def plan_job(job, target_width, target_height, no_enlarge_width, quality):
    """What the device needs for one file, before any pixel is decoded: fills job['probe', 'source_size', 'size', 'resized',
    'sampling', 'quant', 'exif', 'comment'] and returns the job.  Raises preview.HostLeg, and whatever else the planning raises also sends the file
    to the host leg, which then raises what the reference raises."""
    from . import jpeg_host
    from .device_decode import plan_source
    p, source_size = plan_source(job['input'], job['output'], keep_data=True)
    src = jpeg_host.keep_source(job['input'], p['data'])
    p.pop('data', None)                                                 # (the scan holds what the decoder needs)
    width, height, resized = resize_target(source_size, target_width, target_height, no_enlarge_width)
    if resized:
        assert width > 0 and height > 0, 'Invalid image resize target {},{}'.format(width, height)
        if max(width, height) > 65535:
            raise HostLeg('a side above 65535 pixels')
    else:
        width, height = source_size
    if len(src['exif']) > 65533 or len(src['comment'] or b'') > 65533:
        raise HostLeg('an EXIF block or a comment Pillow refuses')
    if src['keep'] and not resized and quality == 'keep':
        if src['quant'] is None:
            raise HostLeg('tables or a sampling the device does not restate')
        job['sampling'], job['quant'] = src['sampling'], src['quant']
    else:
        q = DEFAULT_QUALITY if quality == 'keep' else quality                # (no format: 'keep' is the default quality)
        try:
            job['sampling'], job['quant'] = 2, list(jpeg_host.quant_tables(q))
        except ValueError:
            raise HostLeg('a quality whose tables quant_tables does not give')
    job['probe'], job['source_size'], job['size'], job['resized'] = p, tuple(source_size), (width, height), resized
    job['exif'], job['comment'] = src['exif'], src['comment']
    return job


def render_chunk(ctx, torch, device, chunk, clock, plan, counts, done):
    """One decode chunk of a resize tool: every file planned and read (plan(job) fills the job as plan_job does and returns
    it, or raises), then decoded by the GPU's decoder alone (a file it flags is the host leg's as it is), ONE resample call,
    ONE encode call, then the files written and done(job) called for each.  -> the jobs the host leg has to make"""
    from .device_decode import decode_scans
    jobs, host = DR.plan_each(chunk, plan)
    if not jobs:
        return host
    with clock('decode'):
        decoded, _ = decode_scans(ctx, torch, device, [j['probe']['scan'] for j in jobs])
    host += [j for j, t in zip(jobs, decoded) if t is None]                # a file the decoder flags
    tensors = [t for t in decoded if t is not None]
    jobs = [j for j, t in zip(jobs, decoded) if t is not None]
    counts['files_decoded_gpu'] += len(jobs)

    def encode(tensors, jobs):
        with clock('encode'):
            return DR.encode_sampled(ctx, device, tensors, jobs), 1

    def write(job, data):
        DR.write_bytes(job['output'], data)
        done(job)

    if jobs:
        DR.render_jobs(ctx, torch, device, jobs, tensors, counts, clock, encode, write, draw=False)
    return host


def _light_size(path):
    """decoded bytes of a file from its header, for the cut into chunks; None when it does not open (the host leg's)"""
    from .feed import open_for_coefficients
    try:
        image, _ = open_for_coefficients(path)
        return image.size[0] * image.size[1] * 3
    except Exception:
        return None


def resize_images(input_file_to_output_file, target_width=-1, target_height=-1, no_enlarge_width=False, verbose=False, quality='keep',
                  pool_type='process', n_workers=10, overwrite=True, backend='gpu', device=0, ctx=None, profile=False, counts=None):
    """visualization_utils.resize_images: resizes every image of the dict input file -> output file.  -> a list of
    {'input_fn', 'output_fn', 'status' ('success', 'skipped', 'error'), 'error'} in input order.  counts: a dict that is filled
    in place with COUNT_KEYS (and, with profile, 'ms' per kind of device call).  pool_type and n_workers size the host leg's
    pool; with the gpu backend that pool is one of threads."""
    assert pool_type in ('process', 'thread'), 'Illegal pool type {}'.format(pool_type)
    assert backend in ('gpu', 'host'), 'Illegal backend: {}'.format(backend)
    pairs = [(input_fn, input_file_to_output_file[input_fn]) for input_fn in input_file_to_output_file]
    counts = {} if counts is None else counts
    counts.update({k: 0 for k in COUNT_KEYS})
    counts['files'] = len(pairs)
    if profile:
        counts['ms'] = {}
    settings = (target_width, target_height, no_enlarge_width, quality)
    results = [None] * len(pairs)
    host = list(range(len(pairs)))
    if backend == 'gpu':
        host, items = [], []
        for index, (input_fn, output_fn) in enumerate(pairs):
            if (not overwrite) and (os.path.isfile(output_fn)):
                results[index] = _result(input_fn, output_fn, 'skipped')
                counts['skipped'] += 1
                continue
            nbytes = _light_size(input_fn)
            if nbytes is None:
                host.append(index)
                continue
            os.makedirs(os.path.dirname(output_fn), exist_ok=True)
            items.append({'index': index, 'input': input_fn, 'output': output_fn, 'bytes': nbytes})
        def done(j):
            results[j['index']] = _result(j['input'], j['output'], 'success')
            _count_result(counts, results[j['index']], j['resized'])

        if items:
            import torch
            from .hip_backend import HipContext
            with HipContext.images_or(ctx, device) as ctx:
                left = DR.run_chunks(ctx, torch, items, lambda j: j['bytes'],
                                     partial(render_chunk, plan=lambda j: plan_job(j, *settings), counts=counts, done=done), counts, profile)
            host += [j['index'] for j in left]
        host.sort()
    function = partial(_resize_absolute_image, target_width=target_width, target_height=target_height, no_enlarge_width=no_enlarge_width,
                       verbose=verbose, quality=quality, overwrite=overwrite)
    if n_workers == 1 or not host:
        made = [function(pairs[i]) for i in host]
    else:
        if verbose:
            print('Starting resizing pool with {} {}'.format(n_workers, 'threads' if pool_type == 'thread' or backend == 'gpu' else 'processes'))
        try:
            made = DR.pool_map(function, [pairs[i] for i in host], n_workers, pool_type == 'thread' or backend == 'gpu')
        finally:
            print('Pool closed and joined for image resizing')
    for i, (result, resized) in zip(host, made):
        results[i] = result
        _count_result(counts, result, resized)
        counts['host'] += result['status'] != 'skipped'
        counts['files_decoded_pil'] += resized is not None
    return results


def resize_image_folder(input_folder, output_folder=None, target_width=-1, target_height=-1, no_enlarge_width=False, verbose=False,
                        quality='keep', pool_type='process', n_workers=10, recursive=True, image_files_relative=None, overwrite=True,
                        backend='gpu', device=0, ctx=None, profile=False, counts=None):
    """visualization_utils.resize_image_folder: every image below input_folder (or those of image_files_relative) resized into
    the same relative path below output_folder; None: in place.  -> resize_images' list"""
    assert os.path.isdir(input_folder), '{} is not a folder'.format(input_folder)
    if output_folder is None:
        output_folder = input_folder
    else:
        os.makedirs(output_folder, exist_ok=True)
    assert pool_type in ('process', 'thread'), 'Illegal pool type {}'.format(pool_type)
    if image_files_relative is None:
        if verbose:
            print('Enumerating images')
        image_files_relative = find_images(input_folder, recursive=recursive)
        if verbose:
            print('Found {} images'.format(len(image_files_relative)))
    input_file_to_output_file = {}
    for fn_relative_in in image_files_relative:
        input_file_to_output_file[os.path.join(input_folder, fn_relative_in)] = os.path.join(output_folder, fn_relative_in)
    return resize_images(input_file_to_output_file=input_file_to_output_file, target_width=target_width, target_height=target_height,
                         no_enlarge_width=no_enlarge_width, verbose=verbose, quality=quality, pool_type=pool_type, n_workers=n_workers,
                         overwrite=overwrite, backend=backend, device=device, ctx=ctx, profile=profile, counts=counts)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Resize every image of a folder (in place without an output folder)')
    parser.add_argument('input_folder')
    parser.add_argument('output_folder', nargs='?', default=None)
    parser.add_argument('--target_width', type=int, default=-1)
    parser.add_argument('--target_height', type=int, default=-1)
    parser.add_argument('--no_enlarge_width', action='store_true')
    parser.add_argument('--quality', type=quality_argument, default='keep', help="'keep' or an integer JPEG quality")
    parser.add_argument('--no_recursive', action='store_true')
    parser.add_argument('--no_overwrite', action='store_true')
    parser.add_argument('--n_workers', type=int, default=10, help='size of the host leg\'s pool')
    parser.add_argument('--backend', choices=('gpu', 'host'), default='gpu')
    parser.add_argument('--device', type=int, default=0)
    args = parser.parse_args(argv)
    counts = {}
    results = resize_image_folder(args.input_folder, args.output_folder, target_width=args.target_width, target_height=args.target_height,
                                  no_enlarge_width=args.no_enlarge_width, quality=args.quality,
                                  n_workers=args.n_workers, recursive=not args.no_recursive, overwrite=not args.no_overwrite,
                                  backend=args.backend, device=args.device, counts=counts)
    for r in results:
        if r['status'] == 'error':
            print('Error resizing {}: {}'.format(r['input_fn'], r['error']))
    print('{files} files: {resized} resized, {unresized} written unresized, {skipped} skipped, {errors} errors '
          '({gpu} on the device, {host} on the host)'.format(**counts))
    return 0


if __name__ == '__main__':
    sys.exit(main())
