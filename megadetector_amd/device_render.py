"""
The device render path: what follows the decode for images that lie in device memory, shared by the preview folder (preview.py),
the blurred copies (blur.py), the crops (crops.py), the RDE review sheets (rde_review.py), separate_detections.py,
postprocess_batch_results.py, compare_batch_results.py, visualize_video_output.py, visualize_db.py, resize_images.py and
resize_coco_dataset.py.  device_decode.py brings files into device memory; this module changes and encodes them:

  run_chunks      the device leg of a results-file tool: its planned jobs in decode chunks, a chunk that fails handed to the
                  host leg, the host leg's jobs in their order
  plan_each       the planning loop in front of it: plan(item), or the host leg for an item whose planning raises
  job_bytes       the device bytes of a planned image in its decode chunk
  decode_front    the front of a chunk: ONE device_decode.decode_stage for its distinct files; the jobs of a refused file are
                  the host leg's
  render_jobs     the tail of a chunk: resample_jobs, draw_plans, encode_and_write
  resample_jobs   resample_stage for the jobs whose 'size' is not their 'source_size', counted
  encode_and_write  the tool's encoder call or calls, then -- after this last device call of the chunk -- its files, counted
  encode_whole    the encoder of the tools that save as Image.save does: ONE crops.encode_windows call for whole images
  resample_stage  ONE mdhip_resample_lanczos call for the images of a chunk whose size changes
  blur_rects     ONE mdhip_blur_regions call for the rectangles of a batch of images
  draw_plans      ONE mdhip_draw_ops call for the preview.RenderPlan of each image, the label patches of all of them uploaded
                  once in one buffer (pack_ops)
  draw_plans_from ONE mdhip_draw_ops_from call that makes every rendering of a chunk from the shared images they draw on
  blur_and_draw   the two for a chunk of jobs
  read_encoded    an encoder call into a guessed buffer, once more with the size the call asked for, and the read-back
  encode_sampled  ONE mdhip_jpeg_encode_sampled call, jpeg_host.sampled_file around each scan
  encode_kept     ONE mdhip_jpeg_encode_kept call for the copies that keep their source's JPEG blocks
  encode_copies   the two for a chunk of copies, some of which keep their source's blocks

and, for the host leg that writes the same bytes, blur_with_pil, kept_file_host and pool_map, the reference's pool.  chunked,
DECODE_CHUNK_BYTES and file_twice cut a run into decode chunks; Clock times the kinds of device call of a profiled run.
Apart from run_chunks' wait at its end, nothing here synchronises the device unless a Clock was given a dict to fill.
"""

import datetime
from contextlib import contextmanager, nullcontext

from .blur import DEFAULT_BLUR_RADIUS
from .preview import OP_PATCH

DECODE_CHUNK_BYTES = 256 << 20                   # decoded pixels of one decode chunk: 28 files at 3 MP, 97 frames of 1280 x 720


def chunked(items, size_of, limit, also_break=None):
    """items in their order as a list of chunks, greedily: an item starts a new chunk when its size_of(item) bytes no longer
    fit under `limit` beside the chunk's, or when also_break(chunk, item) says so.  An item above the limit gets a chunk of
    its own; no chunk is empty."""
    chunks, room = [], 0
    for item in items:
        size = size_of(item)
        if not chunks or size > room or (also_break is not None and also_break(chunks[-1], item)):
            chunks.append([])
            room = limit
        chunks[-1].append(item)
        room -= size
    return chunks


class Clock:
    """`with clock('decode'):` adds the milliseconds of the block to ms['decode'], the device waited for before and after, so a
    profiled run is slower than a plain one; with ms None the block just runs and neither torch nor the device is touched"""

    def __init__(self, torch, device, ms):
        self.torch, self.device, self.ms = torch, device, ms

    @contextmanager
    def __call__(self, key):
        if self.ms is None:
            yield
            return
        self.torch.cuda.synchronize(self.device)
        t0 = datetime.datetime.now()
        yield
        self.torch.cuda.synchronize(self.device)
        self.ms[key] = self.ms.get(key, 0.0) + (datetime.datetime.now() - t0).total_seconds() * 1e3


def file_twice(chunk, job):
    """chunked's also_break of the tools whose jobs are files: a file that is listed twice has its jobs in two chunks"""
    return any(j['file'] == job['file'] for j in chunk)


def run_chunks(ctx, torch, items, size_of, render_chunk, counts, profile, host=(), also_break=None, jobs_of=None, order=None):
    """The device leg of a results-file tool around its planned `items`: cuts them into decode chunks (chunked, under
    DECODE_CHUNK_BYTES), calls render_chunk(ctx, torch, device, chunk, clock) for each -- it returns the jobs of the chunk
    that the host leg has to make, and writes a chunk's files after its last device call -- and waits for the device at the
    end.  A chunk whose rendering raises HipError goes to the host leg as a whole, with a warning; anything else propagates.
    counts: gets 'decode_chunks' added to and, with profile, its 'ms' filled by the Clock the chunks are given.  host: the
    jobs that could not be planned.  jobs_of(item): the host leg's jobs of an item that is not one itself.  order: job ->
    its place in the tool's input.  -> the jobs of the host leg: in that order, or without one `host` and then what the
    chunks gave back."""
    from ._lib import HipError
    device = torch.device('cuda:{}'.format(ctx.device))
    clock = Clock(torch, device, counts['ms'] if profile else None)
    host = list(host)
    with torch.cuda.device(device):
        for chunk in chunked(items, size_of, DECODE_CHUNK_BYTES, also_break):
            counts['decode_chunks'] += 1
            try:
                host += render_chunk(ctx, torch, device, chunk, clock)
            except HipError as e:
                jobs = chunk if jobs_of is None else [j for item in chunk for j in jobs_of(item)]
                print('Warning: rendering {} images on the device failed ({}); PIL renders them'.format(len(jobs), e))
                host += jobs
        torch.cuda.synchronize(device)
    return host if order is None else sorted(host, key=order)


def resample_stage(ctx, torch, device, sources, source_sizes, sizes, clock):
    """sources (flat uint8 device tensors of source_sizes (width, height)) at `sizes`: -> (per image the source itself where
    the size stays, else a new tensor, whether the call was made) -- the new ones filled by ONE mdhip_resample_lanczos
    call, timed as 'resample'"""
    out = [s if size == source_size else torch.empty(size[0] * size[1] * 3, dtype=torch.uint8, device=device)
           for s, source_size, size in zip(sources, source_sizes, sizes)]
    resized = [k for k in range(len(sources)) if sizes[k] != source_sizes[k]]
    if resized:
        with clock('resample'):
            ctx.resample_lanczos([sources[k].data_ptr() for k in resized], [source_sizes[k] for k in resized],
                                 [source_sizes[k][0] * 3 for k in resized], [out[k].data_ptr() for k in resized],
                                 [sizes[k] for k in resized], [sizes[k][0] * 3 for k in resized])
    return out, bool(resized)


def plan_each(items, plan):
    """The planning loop of a device leg, before any pixel is decoded: -> (plan(item) of every item, the items whose
    planning raised anything -- the host leg's, which then raises what the reference raises), both in the items' order"""
    planned, host = [], []
    for item in items:
        try:
            planned.append(plan(item))
        except Exception:
            host.append(item)
    return planned, host


def job_bytes(job):
    """device bytes of a planned image in its decode chunk: its decoded pixels and its resized ones"""
    (w, h), (tw, th) = job['source_size'], job['size']
    return w * h * 3 + (tw * th * 3 if (tw, th) != (w, h) else 0)


def decode_front(ctx, torch, device, jobs, image_base, counts, clock, keep_coefficients=False):
    """The front of a chunk: ONE device_decode.decode_stage for the distinct files (relative to image_base) of `jobs`, each a
    dict with its 'file' and that file's 'probe'.  -> (the jobs whose file the GPU's decoder took, their pixel tensors -- jobs
    of one file share one --, the jobs of the refused files in their order: the host leg's, decode_stage's coefficients, which
    with keep_coefficients keep the sources' planes alive as long as the caller holds them)"""
    from .device_decode import decode_stage
    probes = {j['file']: j['probe'] for j in jobs}
    pixels, refused, coefficients = decode_stage(ctx, torch, device, image_base, list(probes), probes, counts, clock, keep_coefficients)
    taken = [j for j in jobs if j['file'] not in refused]
    return taken, [pixels[j['file']] for j in taken], [j for j in jobs if j['file'] in refused], coefficients


def resample_jobs(ctx, torch, device, jobs, tensors, counts, clock):
    """resample_stage for `tensors`, the pixels of `jobs` at their 'source_size': -> the images at the jobs' 'size', the tensor
    itself where the size stays; counts['resample_calls'] moves when the call was made"""
    out, called = resample_stage(ctx, torch, device, tensors, [j['source_size'] for j in jobs], [j['size'] for j in jobs], clock)
    counts['resample_calls'] += called
    return out


def write_bytes(path, data):
    with open(path, 'wb') as f:
        f.write(data)


def encode_and_write(jobs, tensors, counts, encode, write):
    """The end of a chunk: encode(tensors, jobs) -> (the files, the encoder calls made) makes the tool's encoder call or calls
    under its own clock keys; then, after this last device call of the chunk, write(job, file) for each job in order"""
    files, calls = encode(tensors, jobs)
    counts['encode_calls'] += calls
    for job, data in zip(jobs, files):
        write(job, data)
    counts['gpu'] += len(jobs)


def render_jobs(ctx, torch, device, jobs, tensors, counts, clock, encode, write, draw=True):
    """The tail of a chunk for `jobs` (not empty) with their decoded `tensors`: resample_jobs, with `draw` ONE draw_plans
    call for the jobs' 'plan' in place on the result (counts['draw_calls'] moves when the call was made), then
    encode_and_write.  separate_detections, whose copies are never resized and are blurred first, calls blur_and_draw and
    encode_and_write itself."""
    tensors = resample_jobs(ctx, torch, device, jobs, tensors, counts, clock)
    if draw:
        counts['draw_calls'] += draw_plans(ctx, [t.data_ptr() for t in tensors], [j['size'] for j in jobs], [j['plan'] for j in jobs], device,
                                           clock=clock)
    encode_and_write(jobs, tensors, counts, encode, write)


# ---- blur and draw -------------------------------------------------------------------------------------------------------------

def blur_rects(ctx, ptrs, sizes, rects_per_image, radius, stream=0):
    """ONE mdhip_blur_regions call for images in device memory (ptrs, sizes (width, height), rows of 3 * width bytes), changed
    in place: rects_per_image[k] the (left, top, right, bottom) rectangles of image k, applied in their order.  No call when
    no image has a rectangle.  -> whether the call was made"""
    rect_image = [k for k, rects in enumerate(rects_per_image) for _ in rects]
    if not rect_image:
        return False
    ctx.blur_regions(ptrs, sizes, [w * 3 for w, _ in sizes], rect_image, [r for rects in rects_per_image for r in rects], radius,
                     stream=stream)
    return True


def pack_ops(plans):
    """The preview.RenderPlan of each image of a batch as the arguments of one mdhip_draw_ops call: -> (op_image, ops, packed) --
    the image of every row, the rows in the order of the plans, and all label patches in one buffer, a patch that several
    images share or one image repeats stored once.  RECT rows are the plans' own; PATCH rows get their offset into `packed`."""
    packed, where, op_image, ops = bytearray(), {}, [], []
    for k, plan in enumerate(plans):
        for op in plan.ops:
            if op[0] == OP_PATCH:
                data = plan.patch_of(op)
                if data not in where:
                    where[data] = len(packed)
                    packed += data
                op = op[:5] + [where[data]] + op[6:]
            op_image.append(k)
            ops.append(op)
    return op_image, ops, packed


def draw_plans(ctx, ptrs, sizes, plans, device, stream=0, clock=None):
    """ONE mdhip_draw_ops call that draws plans[k] on image k (in place), after ONE upload of the packed patches on torch's
    current stream (the caller makes `stream` that one).  No call when the plans hold no operation.  clock: a Clock that
    times the upload and the call as 'draw' (not the packing, which is host work).  -> whether the call was made"""
    import numpy as np
    import torch
    op_image, ops, packed = pack_ops(plans)
    if not ops:
        return False
    with clock('draw') if clock is not None else nullcontext():
        patches = torch.from_numpy(np.frombuffer(bytes(packed) or b'\0', np.uint8).copy()).to(device)
        ctx.draw_ops(ptrs, sizes, [w * 3 for w, _ in sizes], op_image, ops, patches.data_ptr(), len(packed), stream=stream)
    return True


def draw_plans_from(ctx, src_ptrs, sizes, dst_ptrs, dst_src, plans, device, stream=0, clock=None):
    """ONE mdhip_draw_ops_from call that MAKES destination k (rows of 3 * width bytes at dst_ptrs[k]) from source dst_src[k]
    (src_ptrs, sizes (width, height), rows of 3 * width bytes; only read) under plans[k], after ONE upload of the packed
    patches on torch's current stream (the caller makes `stream` that one): the fan-out of a source that several renderings
    draw on.  A destination whose plan holds no operation is a copy.  No call without destinations.  clock: a Clock that times
    the upload and the call as 'draw'.  -> whether the call was made"""
    import numpy as np
    import torch
    if not dst_ptrs:
        return False
    op_image, ops, packed = pack_ops(plans)
    with clock('draw') if clock is not None else nullcontext():
        patches = torch.from_numpy(np.frombuffer(bytes(packed) or b'\0', np.uint8).copy()).to(device)
        ctx.draw_ops_from(src_ptrs, sizes, [w * 3 for w, _ in sizes], dst_ptrs, dst_src, [sizes[k][0] * 3 for k in dst_src], op_image, ops,
                          patches.data_ptr(), len(packed), stream=stream)
    return True


def blur_and_draw(ctx, device, tensors, jobs, clock, radius=DEFAULT_BLUR_RADIUS, stream=0):
    """blur_rects and then draw_plans for the images `tensors` (flat uint8 device tensors, changed in place) of `jobs`: of each
    job its 'size', its 'rects' to blur and its 'plan'.  stream: the raw stream the calls go on (the caller makes it torch's
    current one).  -> (whether it blurred, whether it drew)"""
    sizes = [j['size'] for j in jobs]
    ptrs = [t.data_ptr() for t in tensors]
    blurred = False
    if any(j['rects'] for j in jobs):
        with clock('blur'):
            blurred = blur_rects(ctx, ptrs, sizes, [j['rects'] for j in jobs], radius, stream)
    return blurred, draw_plans(ctx, ptrs, sizes, [j['plan'] for j in jobs], device, stream, clock)


def changed_rectangles(blur_rects, ops):
    """What a copy's plan changes, as (left, top, right, bottom) with right and bottom exclusive: the blur rectangles as they
    are, a solid rectangle x0 .. x1, y0 .. y1 (inclusive) of the plan's `ops` as (x0, y0, x1 + 1, y1 + 1), a pasted patch as
    (x, y, x + w, y + h).  Not clipped: mdhip_jpeg_encode_kept and jpeg_host.keep_merge clip to the image."""
    out = [tuple(int(v) for v in r) for r in blur_rects]
    for op in ops:
        if op[0] == OP_PATCH:
            out.append((op[1], op[2], op[1] + op[3], op[2] + op[4]))
        else:
            out.append((op[1], op[2], op[3] + 1, op[4] + 1))
    return out


# ---- the encoders --------------------------------------------------------------------------------------------------------------

def read_encoded(call, capacity, device, what):
    """An encoder call into a buffer of `capacity` bytes on `device`, the caller's guess at the output, and a second call with
    the size the first asked for when the guess was too small.  call(out_ptr, capacity) -> (fits, offsets, sizes, needed,
    *rest).  -> (the output as a host uint8 array, offsets, sizes, rest)"""
    import torch
    for _ in range(2):
        out = torch.empty(capacity, dtype=torch.uint8, device=device)
        fits, offs, lens, needed, *rest = call(out.data_ptr(), capacity)
        if fits:
            return out[:max(needed, 1)].cpu().numpy(), offs, lens, rest
        capacity = needed
    raise RuntimeError('{} asked for {} bytes and refused a buffer of that size'.format(what, needed))


def _sampled_guess(sizes):
    # far below the bound (ctx.jpeg_encode_sampled_bound): half a byte a sample and the 8 x 8 blocks' fixed cost
    return sum(w * h * 3 // 2 + 64 * ((w + 7) // 8) * ((h + 7) // 8) + 64 for w, h in sizes)


def _sampled_file(job, scan):
    from . import jpeg_host
    (w, h), (ql, qc) = job['size'], job['quant']
    return jpeg_host.sampled_file(w, h, ql, qc, job['sampling'], scan, job['exif'], job['comment'])


def encode_sampled(ctx, device, tensors, jobs, stream=0):
    """ONE mdhip_jpeg_encode_sampled call (read_encoded) for the images `tensors` of `jobs`: each with its job's 'size',
    'sampling' and 'quant' tables, the file written with its 'exif' and 'comment'.  -> the files"""
    sizes = [j['size'] for j in jobs]
    host, offs, lens, _ = read_encoded(
        lambda out_ptr, capacity: ctx.jpeg_encode_sampled([t.data_ptr() for t in tensors], sizes, [w * 3 for w, _ in sizes],
                                                          [j['sampling'] for j in jobs], [j['quant'] for j in jobs],
                                                          out_ptr, capacity, stream),
        _sampled_guess(sizes), device, 'mdhip_jpeg_encode_sampled')
    return [_sampled_file(j, host[o:o + n].tobytes()) for j, o, n in zip(jobs, offs, lens)]


def encode_kept(ctx, device, tensors, jobs, source_ptrs, stream=0):
    """ONE mdhip_jpeg_encode_kept call (read_encoded) for copies that keep their source's blocks outside their job's 'changed'
    rectangles; source_ptrs: per job the device pointer to its source's quantised planes.  -> the files; None for a copy the
    call flagged"""
    sizes = [j['size'] for j in jobs]
    rect_image = [k for k, j in enumerate(jobs) for _ in j['changed']]
    rects = [r for j in jobs for r in j['changed']]
    host, offs, lens, (status,) = read_encoded(
        lambda out_ptr, capacity: ctx.jpeg_encode_kept([t.data_ptr() for t in tensors], sizes, [w * 3 for w, _ in sizes],
                                                       [j['sampling'] for j in jobs], [j['quant'] for j in jobs], source_ptrs,
                                                       rect_image, rects, out_ptr, capacity, stream),
        _sampled_guess(sizes), device, 'mdhip_jpeg_encode_kept')
    return [None if st else _sampled_file(j, host[o:o + n].tobytes()) for j, o, n, st in zip(jobs, offs, lens, status)]


def encode_whole(ctx, clock, quality, tensors, jobs):
    """encode_and_write's encoder of the tools whose reference saves with Image.save: ONE crops.encode_windows call ('encode'
    on the clock) for the whole images `tensors` of the jobs' 'size' at `quality`, with a job's 'comment' where it has one"""
    from .crops import encode_windows
    sizes = [j['size'] for j in jobs]
    with clock('encode'):
        files = encode_windows(ctx, [t.data_ptr() for t in tensors], [w * 3 for w, _ in sizes], [(0, 0, w, h) for w, h in sizes], quality,
                               comments=[j.get('comment') for j in jobs])
    return files, 1


def encode_copies(ctx, device, tensors, jobs, source_ptrs, clock, reencode_flagged, stream=0):
    """The files of a chunk's copies: ONE encode_kept call ('encode_kept' on the clock) for the jobs with 'keep' whose
    source's planes are on the device (source_ptrs: per job the pointer, or None), then ONE encode_sampled call ('encode')
    for the jobs without 'keep' -- and, with reencode_flagged, in the same call for every copy that has no file yet, so one
    the kept call flagged is encoded whole.  Neither call is made without a copy for it.
    -> (the files, None for a copy left to the host leg; the encoder calls made; the copies the kept call flagged)"""
    files, calls = [None] * len(jobs), 0
    kept = [k for k, j in enumerate(jobs) if j['keep'] and source_ptrs[k] is not None]
    if kept:
        with clock('encode_kept'):
            made = encode_kept(ctx, device, [tensors[k] for k in kept], [jobs[k] for k in kept], [source_ptrs[k] for k in kept], stream)
        for k, data in zip(kept, made):
            files[k] = data
        calls += 1
    flagged = sum(files[k] is None for k in kept)
    rest = [k for k, j in enumerate(jobs) if (files[k] is None if reencode_flagged else not j['keep'])]
    if rest:
        with clock('encode'):
            made = encode_sampled(ctx, device, [tensors[k] for k in rest], [jobs[k] for k in rest], stream)
        for k, data in zip(rest, made):
            files[k] = data
        calls += 1
    return files, calls, flagged


# ---- the host leg's share ------------------------------------------------------------------------------------------------------

def pool_map(function, items, n, threads):
    """[function(item) for item in items] on the reference's pool of n threads or processes (None: the pool's default
    size), the results in the order of the items"""
    from multiprocessing.pool import Pool, ThreadPool
    kind = ThreadPool if threads else Pool
    pool = kind() if n is None else kind(n)
    try:
        return list(pool.imap(function, items))
    finally:
        pool.close()
        pool.join()


def blur_with_pil(image, rects, radius=DEFAULT_BLUR_RADIUS):
    """visualization_utils.blur_detections :509-531 for rectangles with area (blur.blur_rectangle), IN PLACE on a PIL image"""
    from PIL import ImageFilter
    for rect in rects:
        region = image.crop(rect)
        image.paste(region.filter(ImageFilter.GaussianBlur(radius=radius)), (rect[0], rect[1]))


def kept_file_host(pil_image, keep, exif=b''):
    """The host leg of a copy that keeps its source's blocks: Pillow encodes the modified pixels in memory with the source's
    tables and sampling, and the file gets Pillow's blocks in every MCU a rectangle of keep['changed'] touches and the source's
    (keep['coef']) elsewhere, with `exif` as its APP1 block (none when empty).  keep['src']: jpeg_host.keep_source's record.
    -> the file, or None when no baseline scan holds the merged blocks"""
    import io
    from . import jpeg_host
    src, (width, height) = keep['src'], keep['size']
    ql, qc = src['quant']
    bio = io.BytesIO()
    pil_image.save(bio, 'JPEG', qtables=[[int(v) for v in ql], [int(v) for v in qc]], subsampling=src['sampling'])
    rc, _, planes = jpeg_host.decode(bio.getvalue())
    if rc != jpeg_host.MDJPEG_OK or planes.size != keep['coef'].size:
        return None
    if jpeg_host.keep_merge(planes, keep['coef'], (width, height), src['sampling'], keep['changed']):
        return None
    rc, scans, _, _ = jpeg_host.encode_subsequences([planes], [(width, height)], samplings=[src['sampling']])
    if rc != jpeg_host.MDJPEG_OK:
        return None
    return jpeg_host.sampled_file(width, height, ql, qc, src['sampling'], scans[0], exif, src['comment'])
