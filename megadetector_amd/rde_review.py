"""
The review folder of repeat-detection elimination, and the removal pass that follows a person's review.  The reference:
postprocessing/repeat_detection_elimination/repeat_detections_core.py (the "Create filtering directory" block of
find_repeat_detections, _render_sample_image_for_detection, _render_bounding_box, the filterFileToLoad branch),
visualization/render_images_with_thumbnails.py and remove_repeat_detections.py.

The workflow has three steps.  repeat_detections.find_repeat_detections finds the candidates and marks them.
write_review_folder writes outputBase/filtering_<Y.m.d.H.M.S>/ with one sample image per suspicious candidate -- the best
instance's image with the candidate's box drawn and, beside it, a grid of crops of up to detectionTilesMaxCrops instances --
and detectionIndex.json.  A person deletes the samples that show real animals.  remove_repeat_detections then marks, on the
ORIGINAL results, only the candidates whose sample is still there.

What a sample is is restated statement for statement; sheet_layout and tile_geometry are that arithmetic.  backend='host' makes
every sample with exactly the reference's PIL calls.  backend='gpu' decodes every file a group of sheets needs ONCE on the
device (the reference opens and fully decodes one file per tile), makes all tiles of a decode chunk in one mdhip_thumbnails
call, the primaries with the preview calls (draw, quality-75 round trip, LANCZOS) and all sheets of a group in one
mdhip_jpeg_encode call; every file equals the host leg's byte for byte, except that a COM segment of a source file is not
copied into a sample without tiles.  A sheet the device does not restate (preview.HostLeg, MDHIP_EUNSUPPORTED, a side above
65535 pixels) and a sample whose rendering fails in any way go to the host leg as a whole, which leaves what the reference
leaves: the primary-only file, or nothing.

Not restated, NotImplementedError: bRenderOtherDetections=True (the reference's default; False here) and with it
maxOutputImageWidth and the otherDetections* options; smartSort='clustersort'.  detectionIndex.json is plain JSON in a layout
of our own -- the reference's is a jsonpickle dump -- and the two are NOT interchangeable.

Command line:  python -m megadetector_amd.rde_review write INPUT --imageBase D --outputBase D [--outputFile F ...]
               python -m megadetector_amd.rde_review remove INPUT OUTPUT FILTERING_DIR [--filteredFileListToLoad F]
"""

import argparse
import datetime
import json
import math
import os
import sys
import traceback

from . import preview as PV
from . import repeat_detections as RD
from .device_decode import decode_chunk, probe
from .device_render import DECODE_CHUNK_BYTES, Clock, chunked, draw_plans

INDEX_NAME = 'detectionIndex.json'           # reference detection_index_file_name_base

# Device bytes the sheets of one group and what is made on the way to them may take.  A sheet at 3 MP is about 15 MB (the
# primary plus a grid of 0.6 its width) and its primary passes through three more images of 9 MB (drawn copy, round trip,
# resize); 1 GiB is some 25 such sheets -- enough that the one encoder call and the once-per-group decode of a camera's files
# amortise, small beside the 288 GB of the device and beside a detector that may share it.
GROUP_DEVICE_BYTES = 1 << 30
BICUBIC = 0                                  # Image.resize without a filter, for RGB (csrc/resample.h MD_FILTER_BICUBIC)
SAMPLE_QUALITY = 75                          # Image.save(path) of a JPEG: Pillow's default


class ReviewFolderOptions:
    """The review-folder options of the reference's RepeatDetectionOptions, under its names and with its defaults -- except
    bRenderOtherDetections, which is False here (True is NotImplementedError)."""

    def __init__(self):
        self.imageBase = ''                              #: folder the results' file names are relative to
        self.outputBase = ''                             #: folder the filtering_<date> folder is made in
        self.lineThickness = 10                          #: of the candidate's box in the primary image
        self.boxExpansion = 2
        self.bRenderDetectionTiles = True                #: a grid of crops beside the primary image
        self.detectionTilesPrimaryImageWidth = None      #: None: the image's own width
        self.detectionTilesCroppedGridWidth = 0.6        #: <= 1: a fraction of the primary width, else pixels
        self.detectionTilesPrimaryImageLocation = 'right'
        self.detectionTilesMaxCrops = 150                #: None: no limit
        self.bFailOnRenderError = False
        self.bRenderOtherDetections = False
        self.maxOutputImageWidth = None
        self.otherDetectionsThreshold = None
        self.otherDetectionsLineWidth = None
        self.otherDetectionsColors = None

    NAMES = ('imageBase', 'outputBase', 'lineThickness', 'boxExpansion', 'bRenderDetectionTiles', 'detectionTilesPrimaryImageWidth',
             'detectionTilesCroppedGridWidth', 'detectionTilesPrimaryImageLocation', 'detectionTilesMaxCrops', 'bFailOnRenderError')


def check_review_options(options):
    if options.bRenderOtherDetections:
        raise NotImplementedError('bRenderOtherDetections is not restated here: the other detections of a sample image are not drawn')
    given = [k for k in ('maxOutputImageWidth', 'otherDetectionsThreshold', 'otherDetectionsLineWidth', 'otherDetectionsColors')
             if getattr(options, k, None) is not None]
    if given:
        raise NotImplementedError('{} belong(s) to bRenderOtherDetections, which is not restated here'.format(', '.join(given)))
    if not options.outputBase:
        raise ValueError('outputBase is needed')                     # the reference asserts
    if options.imageBase is None:
        raise ValueError('imageBase is needed')


# ---- the first, serial pass ------------------------------------------------------------------------------------------------

def name_samples(suspicious_detections):
    """The reference's serial loop: every candidate's instances sorted by confidence descending (list.sort(reverse=True) is
    stable: equal confidences keep their order) and its sample named.  Returns the candidates as one flat list."""
    flat = []
    for i_dir, locations in enumerate(suspicious_detections):
        for i_detection, location in enumerate(locations):
            location.instances.sort(key=lambda i: i.confidence, reverse=True)
            location.sampleImageRelativeFileName = 'dir{:0>4d}_det{:0>4d}_n{:0>4d}.jpg'.format(i_dir, i_detection, len(location.instances))
            flat.append(location)
    return flat


def primary_detection(location):
    """DetectionLocation.to_api_detection: the candidate's box with the best instance's confidence and category"""
    confidences = [i.confidence for i in location.instances]
    assert confidences[0] == max(confidences), 'Cannot convert an unsorted DetectionLocation to an API detection'
    return {'conf': location.instances[0].confidence, 'bbox': location.bbox, 'category': location.instances[0].category}


def draw_options(options):
    """render_detection_bounding_boxes([d], im, thickness=lineThickness, expansion=boxExpansion, confidence_threshold=-10) and
    everything else at its default, as preview.render_plan / render_with_pil take it (with label_map {}: 'show_categories')"""
    o = PV.PreviewOptions(confidence_threshold=0, output_image_width=None, box_thickness=options.lineThickness,
                          box_expansion=options.boxExpansion)
    o.confidence_threshold = -10
    return o


def tile_instances(location, options):
    n = options.detectionTilesMaxCrops
    return location.instances[0:n] if n is not None and len(location.instances) > n else location.instances


# ---- the arithmetic of a sheet ---------------------------------------------------------------------------------------------

def grid_width(options, primary_image_width):
    if options.detectionTilesCroppedGridWidth <= 1.0:
        return round(options.detectionTilesCroppedGridWidth * primary_image_width)
    return options.detectionTilesCroppedGridWidth


def grid_shape(grid_w, grid_h, first_box, n_crops):
    """the rows, columns and cell size of the grid: the row count whose aspect cols * w0 / (rows * h0), w0 and h0 the NORMALISED
    width and height of the first box, is nearest to the grid's (the first minimum wins); floor-sized cells"""
    grid_aspect = grid_w / grid_h
    w0, h0 = first_box[2], first_box[3]
    rows, best = None, None
    for candidate in range(1, n_crops + 1):
        error = abs(grid_aspect - (math.ceil(n_crops / candidate) * w0) / (candidate * h0))
        if rows is None or error < best:
            rows, best = candidate, error
    assert rows is not None
    cols = math.ceil(n_crops / rows)
    return rows, cols, (math.floor(grid_w / cols), math.floor(grid_h / rows))


def sheet_layout(image_size, options, first_box, n_crops):
    """
    render_images_with_thumbnails up to the crops, for a primary image of image_size as it was saved: a dict with 'primary'
    (its size on the sheet), 'primary_x', 'sheet' (the sheet's size), 'rows', 'cols', 'cell' and 'grid_x' (where the grid
    starts).  Raises what the reference's statements raise.
    """
    location = options.detectionTilesPrimaryImageLocation
    assert location in ['left', 'right']
    width = options.detectionTilesPrimaryImageWidth if options.detectionTilesPrimaryImageWidth is not None else image_size[0]
    grid_w = grid_width(options, width)
    primary = PV.target_size(image_size[0], image_size[1], width)       # resize_image(image, width, target_height=-1)
    assert primary is not None, 'Invalid image resize target'
    rows, cols, cell = grid_shape(grid_w, primary[1], first_box, n_crops)
    sheet = (primary[0] + grid_w, primary[1])
    if not all(isinstance(v, int) for v in sheet):
        raise TypeError('an image size must be two integers, not {!r}'.format(sheet))           # Image.new refuses it
    if sheet[0] < 0 or sheet[1] < 0:
        raise ValueError('Width and height must be >= 0')
    return {'primary': primary, 'primary_x': grid_w if location == 'right' else 0, 'sheet': sheet, 'rows': rows, 'cols': cols,
            'cell': cell, 'grid_x': primary[0] if location == 'left' else 0}


def tile_geometry(box, image_size, cell):
    """crop_image_with_normalized_coordinates and the scaling of one crop: (crop box in pixels of its own image, tile size).
    Image.crop rounds the four floats with Python's round (a half goes to the even neighbour)."""
    x, y, w, h = box[0] * image_size[0], box[1] * image_size[1], box[2] * image_size[0], box[3] * image_size[1]
    x0, y0, x1, y1 = map(int, map(round, (x, y, x + w, y + h)))
    if x1 < x0:
        raise ValueError("Coordinate 'right' is less than 'left'")
    if y1 < y0:
        raise ValueError("Coordinate 'lower' is less than 'upper'")
    cw, ch = x1 - x0, y1 - y0
    scale = min(cell[0] / cw, cell[1] / ch)                              # (a crop without width: ZeroDivisionError)
    size = (int(cw * scale), int(ch * scale))
    if size[0] <= 0 or size[1] <= 0:
        raise ValueError('height and width must be > 0')
    return (x0, y0, x1, y1), size


def tile_position(k, layout):
    return layout['grid_x'] + (k % layout['cols']) * layout['cell'][0], (k // layout['cols']) * layout['cell'][1]


def sample_plan(location, options, size_of):
    """
    The geometry of one sample from the sizes of its files (size_of: relative file name -> (width, height) as open_image gives
    them): {'name', 'file', 'image' (size of the primary's file), 'layout' (None without tiles), 'tiles': [(file, crop box,
    tile size, paste position)]}.  Raises what the reference's rendering would raise.
    """
    plan = {'name': location.sampleImageRelativeFileName, 'file': location.instances[0].filename, 'layout': None, 'tiles': []}
    plan['image'] = size_of(plan['file'])
    if not options.bRenderDetectionTiles:
        return plan
    instances = tile_instances(location, options)
    layout = plan['layout'] = sheet_layout(plan['image'], options, instances[0].bbox, len(instances))
    for k, instance in enumerate(instances):
        box, size = tile_geometry(instance.bbox, size_of(instance.filename), layout['cell'])
        plan['tiles'].append((instance.filename, box, size, tile_position(k, layout)))
    return plan


# ---- the host leg: the reference's PIL calls --------------------------------------------------------------------------------

def _thumbnails_with_pil(primary_file, primary_width, files, boxes, cropped_grid_width, output_file, primary_location):
    """render_images_with_thumbnails, call for call"""
    from PIL import Image
    from .feed import load_image
    assert len(files) == len(boxes), 'Length of secondary image list and bounding box list should be equal'
    assert primary_location in ['left', 'right']
    primary = load_image(primary_file)
    if primary_width is not None:
        size = PV.target_size(primary.size[0], primary.size[1], primary_width)
        assert size is not None, 'Invalid image resize target'
        if size != primary.size:
            primary = primary.resize(size, Image.LANCZOS)
    grid_width_ = cropped_grid_width
    _, cols, (cell_w, cell_h) = grid_shape(grid_width_, primary.size[1], boxes[0], len(files))
    crops = []
    for name, box in zip(files, boxes):
        other = load_image(name)
        w, h = other.size
        crop = other.crop((box[0] * w, box[1] * h, box[0] * w + box[2] * w, box[1] * h + box[3] * h))
        scale = min(cell_w / crop.size[0], cell_h / crop.size[1])
        crops.append(crop.resize((int(crop.size[0] * scale), int(crop.size[1] * scale))))
    sheet = Image.new('RGB', (primary.size[0] + grid_width_, primary.size[1]))
    sheet.paste(primary, (grid_width_ if primary_location == 'right' else 0, 0))
    i_row = i_col = 0
    for image in crops:
        x = i_col * cell_w
        if primary_location == 'left':
            x += primary.size[0]
        sheet.paste(image, (x, i_row * cell_h))
        i_col += 1
        if i_col >= cols:
            i_col = 0
            i_row += 1
    parent = os.path.dirname(output_file)
    if len(parent) > 0:
        os.makedirs(parent, exist_ok=True)
    sheet.save(output_file)


def render_sample_host(location, filtering_dir, options):
    """_render_sample_image_for_detection with bRenderOtherDetections off: the file of one sample by PIL.  Everything from
    opening the image on is caught (and raised again with bFailOnRenderError); the sample keeps what was written until then."""
    from .feed import load_image
    output = os.path.join(filtering_dir, location.sampleImageRelativeFileName)
    path = os.path.join(options.imageBase, location.instances[0].filename)
    assert os.path.isfile(path), 'Not a file: {}'.format(path)
    try:
        im = load_image(path)                                           # open_image: EXIF rotation, RGB
        PV.render_with_pil(im, [primary_detection(location)], draw_options(options), label_map={}, labels=True)
        im.save(output)
        if options.bRenderDetectionTiles:
            width = options.detectionTilesPrimaryImageWidth if options.detectionTilesPrimaryImageWidth is not None else im.size[0]
            instances = tile_instances(location, options)
            _thumbnails_with_pil(output, width, [os.path.join(options.imageBase, i.filename) for i in instances],
                                 [i.bbox for i in instances], grid_width(options, width), output,
                                 options.detectionTilesPrimaryImageLocation)
    except Exception as e:
        print('Warning: error rendering bounding box from {} to {}: {} ({})'.format(path, output, e, traceback.format_exc()))
        if options.bFailOnRenderError:
            raise


# ---- the device leg ----------------------------------------------------------------------------------------------------------

def _render_group_device(ctx, torch, device, group, probes, filtering_dir, options, counts):
    """The sheets of one group (plans of sample_plan with their RenderPlan under 'draw'): their files decoded once in chunks, per
    chunk one mdhip_thumbnails call and the primaries' calls, one encoder call for the group.  Returns the plans it could not
    make (MDHIP_EUNSUPPORTED): the host leg makes them.  With counts['ms'] (write_review_folder(profile=True)) the kinds of
    call are timed into it (device_render.Clock)."""
    from .crops import encode_windows
    clock = Clock(torch, device, counts.get('ms'))
    # the sheets (black) and, without tiles, nothing yet: the drawn primary is the image
    sheets = {}
    for p in group:
        if p['layout'] is not None:
            w, h = p['layout']['sheet']
            sheets[p['name']] = torch.zeros(w * h * 3, dtype=torch.uint8, device=device)
    needed = []
    for p in group:
        for f in [p['file']] + [t[0] for t in p['tiles']]:
            if f not in needed:
                needed.append(f)
    refused = set()
    for files in chunked(needed, lambda f: probes[f]['size'][0] * probes[f]['size'][1] * 3, DECODE_CHUNK_BYTES):
        counts['decode_chunks'] += 1
        with clock('decode'):
            pixels, failed = decode_chunk(ctx, torch, device, options.imageBase, files, probes, counts)
        refused.update(p['name'] for p in group if p['file'] in failed or any(t[0] in failed for t in p['tiles']))
        tiles = []
        for p in group:
            if p['name'] in refused:
                continue
            sheet_w = p['layout']['sheet'][0] if p['layout'] is not None else 0
            for f, (x0, y0, x1, y1), (tw, th), (x, y) in p['tiles']:
                if f not in pixels:
                    continue
                w, h = probes[f]['size']
                ix0, iy0, ix1, iy1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
                inside = ix1 > ix0 and iy1 > iy0
                src = pixels[f].data_ptr() + (iy0 * w + ix0) * 3 if inside else 0
                tiles.append((p['name'], (src, w * 3, ix1 - ix0 if inside else 0, iy1 - iy0 if inside else 0, x1 - x0, y1 - y0,
                                          ix0 - x0 if inside else 0, iy0 - y0 if inside else 0, tw, th,
                                          sheets[p['name']].data_ptr() + (y * sheet_w + x) * 3, sheet_w * 3)))
        tiles = [t for t in tiles if t[0] not in refused]
        while tiles:
            with clock('thumbnails'):
                ok = ctx.thumbnails([t[1] for t in tiles[:65535]], BICUBIC)
            if ok:
                counts['tile_calls'] += 1
                counts['tiles'] += len(tiles[:65535])
                tiles = tiles[65535:]
                continue
            # a tile the device refuses: find its sheet (the call is all or nothing), hand that sheet to the host leg
            for name, rec in tiles[:65535]:
                if name not in refused and not ctx.thumbnails([rec], BICUBIC):
                    refused.add(name)
            tiles = [t for t in tiles if t[0] not in refused]
        # the primaries whose file is in this chunk: draw on a copy, then (with tiles) the quality-75 round trip of the
        # saved file, LANCZOS when the size changes, into the sheet
        prim = [p for p in group if p['file'] in pixels and p['name'] not in refused]
        if not prim:
            continue
        drawn = [pixels[p['file']].clone() for p in prim]
        sizes = [p['image'] for p in prim]
        draw_plans(ctx, [t.data_ptr() for t in drawn], sizes, [p['draw'] for p in prim], device)
        tiled = [k for k, p in enumerate(prim) if p['layout'] is not None]
        for k, p in enumerate(prim):
            if p['layout'] is None:
                sheets[p['name']] = drawn[k]
        if tiled:
            saved = [torch.empty_like(drawn[k]) for k in tiled]
            ctx.jpeg_recompress([drawn[k].data_ptr() for k in tiled], [sizes[k] for k in tiled], [sizes[k][0] * 3 for k in tiled],
                                SAMPLE_QUALITY, [t.data_ptr() for t in saved])
            resized = [j for j, k in enumerate(tiled) if prim[k]['layout']['primary'] != sizes[k]]
            if resized:
                ctx.resample_lanczos([saved[j].data_ptr() for j in resized], [sizes[tiled[j]] for j in resized],
                                     [sizes[tiled[j]][0] * 3 for j in resized],
                                     [sheets[prim[tiled[j]]['name']].data_ptr() + prim[tiled[j]]['layout']['primary_x'] * 3 for j in resized],
                                     [prim[tiled[j]]['layout']['primary'] for j in resized],
                                     [prim[tiled[j]]['layout']['sheet'][0] * 3 for j in resized])
            for j, k in enumerate(tiled):
                if j in resized:
                    continue
                layout = prim[k]['layout']
                (w, h), x = layout['primary'], layout['primary_x']
                sheets[prim[k]['name']].view(layout['sheet'][1], layout['sheet'][0], 3)[:, x:x + w] = saved[j].view(h, w, 3)
        del pixels
    made = [p for p in group if p['name'] not in refused]
    if made:
        dims = [p['layout']['sheet'] if p['layout'] is not None else p['image'] for p in made]
        with clock('encode'):
            files = encode_windows(ctx, [sheets[p['name']].data_ptr() for p in made], [d[0] * 3 for d in dims],
                                   [(0, 0, d[0], d[1]) for d in dims], SAMPLE_QUALITY)
        counts['encode_calls'] += 1
        for p, data in zip(made, files):
            with open(os.path.join(filtering_dir, p['name']), 'wb') as f:
                f.write(data)
        counts['gpu'] += len(made)
    return [p for p in group if p['name'] in refused]


def _plan_bytes(plan):
    w, h = plan['image']
    sheet = plan['layout']['sheet'] if plan['layout'] is not None else (0, 0)
    return sheet[0] * sheet[1] * 3 + 3 * w * h * 3


def _render_device(flat, filtering_dir, options, ctx, device, counts):
    import torch
    dev = torch.device('cuda:{}'.format(device))
    probes = {}

    def size_of(f):
        if f not in probes:
            probes[f] = probe(os.path.join(options.imageBase, f))
        return probes[f]['size']

    draw = draw_options(options)
    # location by location (the candidates of a location are consecutive in `flat`), in groups under the byte budget
    start = 0
    while start < len(flat):
        stop = start
        while stop < len(flat) and flat[stop].relativeDir == flat[start].relativeDir:
            stop += 1
        group, used = [], 0
        for location in flat[start:stop] + [None]:
            plan = None
            if location is not None:
                path = os.path.join(options.imageBase, location.instances[0].filename)
                assert os.path.isfile(path), 'Not a file: {}'.format(path)
                try:
                    plan = sample_plan(location, options, size_of)
                    if max(plan['layout']['sheet'] if plan['layout'] is not None else plan['image']) > 65535:
                        raise PV.HostLeg('a sheet above 65535 pixels a side')
                    if plan['layout'] is not None:
                        sw, sh = plan['layout']['sheet']
                        if any(x < 0 or y < 0 or x + w > sw or y + h > sh for _, _, (w, h), (x, y) in plan['tiles']):
                            raise PV.HostLeg('a tile that leaves its sheet (Image.paste clips it)')
                    plan['draw'] = PV.render_plan([primary_detection(location)], plan['image'][0], plan['image'][1], draw, {}, True)
                    plan['location'] = location
                except Exception:
                    # not restated on the device, or the reference's own rendering fails: the host leg leaves what it leaves
                    render_sample_host(location, filtering_dir, options)
                    counts['host'] += 1
                    continue
            if group and (plan is None or used + _plan_bytes(plan) > GROUP_DEVICE_BYTES):
                with torch.cuda.device(dev):
                    for p in _render_group_device(ctx, torch, dev, group, probes, filtering_dir, options, counts):
                        render_sample_host(p['location'], filtering_dir, options)
                        counts['host'] += 1
                group, used = [], 0
            if plan is not None:
                group.append(plan)
                used += _plan_bytes(plan)
        probes.clear()
        start = stop
    torch.cuda.synchronize(dev)


# ---- the folder ---------------------------------------------------------------------------------------------------------------

def index_for_folder(rde_results, rde_options, review_options):
    """detectionIndex.json: the layout of <output>.rde_index.json plus each candidate's sample file name, dir_index_to_name and
    the options of both stages.  Plain JSON of our own; NOT the reference's jsonpickle file."""
    index = RD.index_for_file(rde_results, rde_options or RD.RepeatDetectionOptions())
    for locations, entries in zip(rde_results.suspicious_detections, index['suspicious_detections']):
        for location, entry in zip(locations, entries):
            entry['sampleImageRelativeFileName'] = location.sampleImageRelativeFileName
            for instance, e in zip(location.instances, entry['instances']):
                e['category'] = instance.category
    index['dir_index_to_name'] = {str(i): d for i, d in enumerate(rde_results.dirs)}
    index['review_options'] = {k: getattr(review_options, k) for k in ReviewFolderOptions.NAMES}
    return index


def load_index(path):
    """-> (index dict, suspicious_detections as lists of DetectionLocation with their sample names)"""
    with open(path, 'r') as f:
        index = json.load(f)
    suspicious = []
    for i_dir, entries in enumerate(index['suspicious_detections']):
        locations = []
        for entry in entries:
            instances = [RD.IndexedDetection(i['i_detection'], i['filename'], i['bbox'], i['confidence'], i.get('category', entry['category']))
                         for i in entry['instances']]
            location = RD.DetectionLocation(instances[0], entry['relativeDir'], entry['id'])
            location.instances = instances
            location.bbox, location.category = entry['bbox'], entry['category']
            location.sampleImageRelativeFileName = entry['sampleImageRelativeFileName']
            locations.append(location)
        suspicious.append(locations)
    return index, suspicious


def write_review_folder(rde_results, review_options, backend='gpu', device=0, ctx=None, now=None, rde_options=None, profile=False):
    """
    Writes review_options.outputBase/filtering_<Y.m.d.H.M.S>/ for the RepeatDetectionResults of find_repeat_detections: one
    sample per suspicious candidate and detectionIndex.json.  backend 'host': PIL, no GPU; 'gpu': on HIP device `device`, on
    `ctx` (a HipContext, e.g. a detector's) or on a context without a model made for the call.  now: the datetime in the
    folder's name.  rde_options: the options the candidates were found with, for the index.  profile: also counts['ms'], the
    milliseconds of the decode, thumbnails and encode calls (the device is waited for around each: slower).
    Returns counts: 'sheets', those made on the 'gpu' and by the 'host' leg, 'files_decoded_gpu', 'files_decoded_pil',
    'tile_calls' (mdhip_thumbnails calls), and beside them 'decode_chunks', 'tiles', 'encode_calls' and 'folder'.
    """
    check_review_options(review_options)
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    os.makedirs(review_options.outputBase, exist_ok=True)
    # the reference's early check: the first image of the results must exist under imageBase
    images = rde_results.detectionResults['images']
    if images:
        first = os.path.join(review_options.imageBase, images[0]['file'])
        if not os.path.isfile(first):
            raise ValueError('Could not find file {} in folder {}: is imageBase right?'.format(images[0]['file'], review_options.imageBase))
    now = now or datetime.datetime.now()
    folder = os.path.join(review_options.outputBase, 'filtering_' + now.strftime('%Y.%m.%d.%H.%M.%S'))
    os.makedirs(folder, exist_ok=True)
    flat = name_samples(rde_results.suspicious_detections)
    counts = {'sheets': len(flat), 'gpu': 0, 'host': 0, 'files_decoded_gpu': 0, 'files_decoded_pil': 0, 'tile_calls': 0,
              'decode_chunks': 0, 'tiles': 0, 'encode_calls': 0}
    if profile:
        counts['ms'] = {}
    if backend == 'host':
        for location in flat:
            render_sample_host(location, folder, review_options)
        counts['host'] = len(flat)
    elif flat:
        from .hip_backend import HipContext
        with HipContext.images_or(ctx, device) as ctx:
            _render_device(flat, folder, review_options, ctx, ctx.device, counts)
    RD.write_json(os.path.join(folder, INDEX_NAME), index_for_folder(rde_results, rde_options, review_options), force_str=True)
    counts['folder'] = folder
    return counts


def find_and_write(input_filename, output_file_name=None, rde_options=None, review_options=None, backend='gpu', device=0, now=None):
    """Both stages in one call: find_repeat_detections, then write_review_folder.  -> (RepeatDetectionResults, counts)"""
    rde_options = rde_options or RD.RepeatDetectionOptions()
    check_review_options(review_options)
    results = RD.find_repeat_detections(input_filename, output_file_name, rde_options, backend=backend, device=device)
    return results, write_review_folder(results, review_options, backend=backend, device=device, now=now, rde_options=rde_options)


# ---- the removal pass ---------------------------------------------------------------------------------------------------------

def remove_repeat_detections(input_file, output_file, filtering_dir_or_index, filtered_file_list=None, backend='gpu'):
    """
    The reference's remove_repeat_detections (find_repeat_detections with filterFileToLoad): loads the index of a review folder,
    keeps a candidate only if its sample file is still in the folder -- or, with filtered_file_list (a text file, one sample
    name a line: filteredFileListToLoad), only if its name is in that list -- and marks the kept candidates' instances negative
    on the ORIGINAL results of input_file, with the reference's assertions; writes output_file as repeat_detections does.
    The candidates come from the index: nothing is launched on a GPU, whatever `backend` says.  -> RepeatDetectionResults
    """
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    assert os.path.exists(filtering_dir_or_index), "Can't find input file/folder {}".format(filtering_dir_or_index)
    index_file = filtering_dir_or_index if os.path.isfile(filtering_dir_or_index) else os.path.join(filtering_dir_or_index, INDEX_NAME)
    index, suspicious = load_index(index_file)
    base = os.path.dirname(index_file)
    options = RD.RepeatDetectionOptions()
    for k, v in index['options'].items():
        setattr(options, k, v)
    with open(input_file, 'r') as f:
        results = RD.prepare_results(json.load(f), options)
    images = results['images']
    dirs = list(RD.group_images(images, options).keys())
    assert len(suspicious) == len(dirs)
    file_list = None
    if filtered_file_list is not None:
        with open(filtered_file_list) as f:
            file_list = [x.strip() for x in f.readlines()]
    n_loaded = n_removed = 0
    for i_dir, locations in enumerate(suspicious):
        n_loaded += len(locations)
        if file_list is None:
            kept = [loc for loc in locations if os.path.isfile(os.path.join(base, loc.sampleImageRelativeFileName))]
        else:
            kept = [loc for loc in locations if loc.sampleImageRelativeFileName in file_list]
        n_removed += len(locations) - len(kept)
        suspicious[i_dir] = kept
    print('Removed {} of {} total detections via manual filtering'.format(n_removed, n_loaded))
    # _update_detection_table
    row_of = {im['file']: i for i, im in enumerate(images)}
    n_bbox_changes = 0
    for locations in suspicious:
        for location in locations:
            for instance in location.instances:
                iou = _get_iou(instance.bbox, location.bbox)
                assert iou >= options.iouThreshold
                assert instance.filename in row_of
                d = images[row_of[instance.filename]]['detections'][instance.i_detection]
                assert instance.bbox[0:4] == d['bbox'][0:4]
                if d['conf'] >= 0:
                    d['conf'] = -1 * d['conf']
                    n_bbox_changes += 1
    for im in images:
        if im.get('detections'):
            im['max_detection_conf'] = max(d['conf'] for d in im['detections'])
    out = RD.RepeatDetectionResults()
    out.detectionResults = results
    out.otherFields = {k: v for k, v in results.items() if k != 'images'}
    out.dirs = dirs
    out.suspicious_detections = suspicious
    out.n_bbox_changes = n_bbox_changes
    if output_file:
        RD.write_json(output_file, RD.results_for_file(results), force_str=True)
    return out


def _get_iou(bb1, bb2):
    """ct_utils.get_iou on [x, y, w, h] boxes, operation for operation"""
    bb1 = [bb1[0], bb1[1], bb1[0] + bb1[2], bb1[1] + bb1[3]]
    bb2 = [bb2[0], bb2[1], bb2[0] + bb2[2], bb2[1] + bb2[3]]
    assert bb1[0] < bb1[2], 'Malformed bounding box (x2 >= x1)'
    assert bb1[1] < bb1[3], 'Malformed bounding box (y2 >= y1)'
    assert bb2[0] < bb2[2], 'Malformed bounding box (x2 >= x1)'
    assert bb2[1] < bb2[3], 'Malformed bounding box (y2 >= y1)'
    x_left, y_top = max(bb1[0], bb2[0]), max(bb1[1], bb2[1])
    x_right, y_bottom = min(bb1[2], bb2[2]), min(bb1[3], bb2[3])
    if x_right < x_left or y_bottom < y_top:
        return 0.0
    intersection_area = (x_right - x_left) * (y_bottom - y_top)
    bb1_area = (bb1[2] - bb1[0]) * (bb1[3] - bb1[1])
    bb2_area = (bb2[2] - bb2[0]) * (bb2[3] - bb2[1])
    iou = intersection_area / float(bb1_area + bb2_area - intersection_area)
    assert iou >= 0.0, 'Illegal IOU < 0'
    assert iou <= 1.0, 'Illegal IOU > 1'
    return iou


# ---- command line -------------------------------------------------------------------------------------------------------------

RDE_ARGUMENTS = ('confidenceMin', 'confidenceMax', 'iouThreshold', 'occurrenceThreshold', 'minSuspiciousDetectionSize',
                 'maxSuspiciousDetectionSize', 'maxImagesPerFolder', 'nDirLevelsFromLeaf')


def main(argv=None):
    d, r = RD.RepeatDetectionOptions(), ReviewFolderOptions()
    ap = argparse.ArgumentParser(description='The review folder of repeat-detection elimination, and the removal pass after a review')
    sub = ap.add_subparsers(dest='command', required=True)
    w = sub.add_parser('write', help='find the repeat detections of a results file and write the review folder')
    w.add_argument('inputFile', type=str, help='MD results .json file to process')
    w.add_argument('--imageBase', type=str, required=True, help='folder the file names of the results are relative to')
    w.add_argument('--outputBase', type=str, required=True, help='folder the filtering_<date> folder is made in')
    w.add_argument('--outputFile', type=str, default=None, help='.json file to write the marked results to')
    for k in RDE_ARGUMENTS:
        w.add_argument('--' + k, type=int if isinstance(getattr(d, k), int) or k == 'maxImagesPerFolder' else float, default=getattr(d, k))
    w.add_argument('--excludeClasses', nargs='+', type=int, default=None)
    w.add_argument('--lineThickness', type=int, default=r.lineThickness)
    w.add_argument('--boxExpansion', type=int, default=r.boxExpansion)
    w.add_argument('--omitDetectionTiles', action='store_true', help='samples without the grid of crops')
    w.add_argument('--detectionTilesPrimaryImageWidth', type=int, default=r.detectionTilesPrimaryImageWidth)
    w.add_argument('--detectionTilesCroppedGridWidth', type=float, default=r.detectionTilesCroppedGridWidth)
    w.add_argument('--detectionTilesPrimaryImageLocation', type=str, default=r.detectionTilesPrimaryImageLocation)
    w.add_argument('--detectionTilesMaxCrops', type=int, default=r.detectionTilesMaxCrops)
    w.add_argument('--backend', choices=('host', 'gpu'), default='gpu', help="'host': PIL and the host model of the kernels, no GPU needed")
    w.add_argument('--device', type=int, default=0, help='HIP device of the gpu backend')
    m = sub.add_parser('remove', help='mark only the candidates whose samples are still in the review folder')
    m.add_argument('inputFile', type=str, help='the ORIGINAL MD results .json file')
    m.add_argument('outputFile', type=str)
    m.add_argument('filteringDir', type=str, help='the filtering_<date> folder (or its detectionIndex.json) after the review')
    m.add_argument('--filteredFileListToLoad', type=str, default=None, help='text file with the sample names to keep, instead of the folder')
    args = ap.parse_args(argv)
    if args.command == 'remove':
        remove_repeat_detections(args.inputFile, args.outputFile, args.filteringDir, args.filteredFileListToLoad)
        return 0
    for k in RDE_ARGUMENTS:
        setattr(d, k, getattr(args, k))
    if args.excludeClasses is not None:
        d.excludeClasses = args.excludeClasses
    for k in ('imageBase', 'outputBase', 'lineThickness', 'boxExpansion', 'detectionTilesPrimaryImageWidth', 'detectionTilesPrimaryImageLocation',
              'detectionTilesMaxCrops'):
        setattr(r, k, getattr(args, k))
    r.bRenderDetectionTiles = not args.omitDetectionTiles
    g = args.detectionTilesCroppedGridWidth
    r.detectionTilesCroppedGridWidth = int(g) if g > 1.0 and float(g).is_integer() else g
    _, counts = find_and_write(args.inputFile, args.outputFile, d, r, backend=args.backend, device=args.device)
    print('Wrote {} samples to {} ({})'.format(counts['sheets'], counts['folder'], ', '.join('{} {}'.format(k, v) for k, v in counts.items() if k != 'folder')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
