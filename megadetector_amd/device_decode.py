"""
Files of a folder, and the stored frames of videos, as RGB pixels in device memory, each decoded once: what the tools that work
on written results files share (rde_review.py, separate_detections.py, postprocess_batch_results.py, compare_batch_results.py,
visualize_video_output.py), with what they check of a file before they decode it (plan_source).  What follows the decode --
blur, draw, encode -- is device_render.py.  A baseline JPEG the GPU's decoder takes goes through mdhip_jpeg_entropy_decode and
mdhip_jpeg_reconstruct on a context that needs no model -- one call each for a whole chunk of files -- and comes out as the
pixels the reference's load_image gives, EXIF rotation included; every other file, and a JPEG the decoder flags, is decoded
by PIL and uploaded.
"""

import os


def probe(path, keep_data=False):
    """What the device leg needs of a file before any pixel is decoded: {'size': (width, height) as open_image gives them,
    'scan': a jpeg_host.ScanImage when the GPU's decoder takes the file, else None}; with keep_data also 'data', the bytes of
    a file Pillow calls a JPEG (else None).  Raises what opening it raises."""
    from . import jpeg_host
    from .feed import open_for_coefficients
    image, rotation = open_for_coefficients(path)
    size = (image.size[1], image.size[0]) if rotation in (90, 270) else image.size
    scan = data = None
    if image.format == 'JPEG':
        with open(path, 'rb') as f:
            data = f.read()
        if jpeg_host.parse(data).supported:
            rc, scan, _ = jpeg_host.ScanImage.from_bytes(data, rotation)
            if rc != jpeg_host.MDJPEG_OK:
                scan = None
    out = {'size': tuple(size), 'scan': scan}
    if keep_data:
        out['data'] = data
    return out


def plan_source(path, output_name, target_width=None, keep_data=False, probes=None):
    """What every results-file tool checks of a job before any pixel is decoded: -> (probe(path, keep_data), the size the image
    is rendered at: resize_image's for target_width, its own for None).  Raises preview.HostLeg, the checks in this order: a
    file that does not open, a file the device does not decode, an output name Pillow does not save as JPEG, a side above
    65535 pixels; a target that is not positive is the reference's AssertionError.  probes: a dict that keeps what probe gave
    or raised per path, so a file is probed once however many jobs draw on it."""
    from .crops import is_jpeg_name
    from .preview import HostLeg, resized_size
    p = None if probes is None else probes.get(path)
    if p is None:
        try:
            p = probe(path, keep_data)
        except Exception as e:
            p = e
        if probes is not None:
            probes[path] = p
    if isinstance(p, Exception):
        raise HostLeg('a file that does not open: PIL raises what the reference raises')
    if p['scan'] is None:
        raise HostLeg('a file the device does not decode')
    if not is_jpeg_name(output_name):
        raise HostLeg('not a JPEG name')
    width, height = p['size']
    size = resized_size(width, height, target_width)
    if max(width, height, size[0], size[1]) > 65535:
        raise HostLeg('a side above 65535 pixels')
    return p, size


def decode_scans(ctx, torch, device, images, keep_coefficients=False):
    """jpeg_host.ScanImage objects -> their RGB pixels in device memory: ONE mdhip_jpeg_entropy_decode call and ONE
    mdhip_jpeg_reconstruct call for all of them, whatever their sizes, samplings and tables.  -> (pixels, coefficients): per
    image a flat uint8 device tensor, None for an image the decoder flags; per image None or, with keep_coefficients and for a
    decoded image, (device pointer to its quantised planes in the layout of mdjpeg_decode, the tensor that holds them) -- the
    planes live as long as the caller keeps the entry."""
    import numpy as np
    pixels, coefficients = [None] * len(images), [None] * len(images)
    if not images:
        return pixels, coefficients
    scan_offs, coef_offs, nbytes, nvals = [], [], 0, 0
    for im in images:
        scan_offs.append(nbytes)
        nbytes += (im.nbytes + 255) // 256 * 256 + 256
        coef_offs.append(nvals)
        nvals += (im.coef_count + 127) // 128 * 128
    host = np.zeros(nbytes, dtype=np.uint8)
    for im, off in zip(images, scan_offs):
        host[off:off + im.nbytes] = im.scan_bytes
    compressed = torch.from_numpy(host).to(device)
    coefs = torch.empty(max(nvals, 1), dtype=torch.int16, device=device)
    status = ctx.jpeg_entropy_decode(images, [compressed.data_ptr() + o for o in scan_offs], [coefs.data_ptr() + 2 * o for o in coef_offs])
    clean = [k for k, st in enumerate(status) if st == 0]
    if clean:
        outs = [torch.empty(int(np.prod(images[k].shape)), dtype=torch.uint8, device=device) for k in clean]
        ctx.jpeg_reconstruct([images[k].coefficient_image() for k in clean], [coefs.data_ptr() + 2 * coef_offs[k] for k in clean],
                             [t.data_ptr() for t in outs])
        for k, t in zip(clean, outs):
            pixels[k] = t
            if keep_coefficients:
                coefficients[k] = (coefs.data_ptr() + 2 * coef_offs[k], coefs)
    return pixels, coefficients


def decode_chunk(ctx, torch, device, image_base, files, probes, counts, via_pil=None, coefficients=None):
    """file -> flat uint8 device tensor of its RGB pixels, each file decoded once: the JPEGs the decoder takes through
    decode_scans (one entropy-decode and one reconstruct call for the chunk), every other file -- and a JPEG the
    decoder flags -- through PIL and an upload.  files are relative to image_base; probes: file -> probe(); counts gets
    'files_decoded_gpu' and 'files_decoded_pil' added to; via_pil: a set that receives the files PIL decoded; coefficients: a
    dict that receives, per file the GPU decoded, (device pointer to its quantised planes in the layout of mdjpeg_decode, the
    tensor that holds them) -- the planes live as long as the caller keeps the entry; None: they are freed with the call.
    -> (pixels, the files PIL could not decode either)"""
    import numpy as np
    from .feed import load_image
    pixels, failed = {}, set()
    scans = [f for f in files if probes[f]['scan'] is not None]
    decoded, planes = decode_scans(ctx, torch, device, [probes[f]['scan'] for f in scans], coefficients is not None)
    for f, t, c in zip(scans, decoded, planes):
        if t is not None:
            pixels[f] = t
            counts['files_decoded_gpu'] += 1
            if coefficients is not None:
                coefficients[f] = c
    for f in files:
        if f not in pixels:
            try:
                array = np.ascontiguousarray(np.asarray(load_image(os.path.join(image_base, f))))
            except Exception:
                failed.add(f)                                           # what needs it goes to the caller's host leg, which fails as PIL does
                continue
            pixels[f] = torch.from_numpy(array.reshape(-1).copy()).to(device)
            counts['files_decoded_pil'] += 1
            if via_pil is not None:
                via_pil.add(f)
    return pixels, failed


def decode_stage(ctx, torch, device, image_base, files, probes, counts, clock, keep_coefficients=False):
    """The decode of one chunk of a results-file tool, timed as 'decode' by `clock` (a device_render.Clock): decode_chunk for
    `files`, of which the tool renders only what the GPU's decoder took.  -> (pixels: file -> flat uint8 device tensor, the
    refused files -- those PIL decoded or could not decode either: their jobs go to the host leg --, coefficients: None, or
    with keep_coefficients decode_chunk's dict, which keeps the sources' planes until the caller drops it)"""
    via_pil = set()
    coefficients = {} if keep_coefficients else None
    with clock('decode'):
        pixels, failed = decode_chunk(ctx, torch, device, image_base, files, probes, counts, via_pil, coefficients)
    return pixels, failed | via_pil, coefficients
