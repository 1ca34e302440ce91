"""
Rendering the detections of a video results file into videos, as the reference does it (visualization/
visualize_video_output.py: per video, every processed frame is read again, render_detection_bounding_boxes draws on it, and
the frames are written as a video whose frame rate follows the sampling interval) -- for Motion-JPEG AVI files, which this
package reads (avi.AviFile) and writes (avi.write_mjpeg_avi) itself, with no OpenCV.

What is restated statement for statement (visualize_video_output.py:131-343, :348-493, :623-762): the validation, the loading
and the filter to video entries, the sampling, and per video (plan_video) the failed entry, the path assertions, the output
name (flatten_output, output_extension, the category filters, the category names in the file name), the frames to process,
the output frame rate, min_output_length_seconds, the result dicts with their error strings, and the summary counts.

Not restated: fourcc is 'MJPG' or NotImplementedError (the reference's default 'h264' cannot be written here); an input that
is not an AVI with an MJPG stream is that video's error ('not a Motion-JPEG AVI'); the parallelize_* options size the pool
of the host leg and are ignored by the gpu leg; where include_category_names meets a video without any classification name
the reference formats a variable that was never bound and raises, and here the video is skipped ('Skipped: none').

Ours (all off or neutral by default; the reference's TODO.md asks for them: "Add blurring to video rendering", "Add quality
parameters to visualize_video_output"):
  blur_category_names, blur_radius   blur.py's box selection with confidence_threshold, applied before the drawing
  quality                            'keep': a touched frame is re-encoded with the stored frame's own quantisation tables and
                                     chroma sampling; 1 .. 95: Pillow's save(quality=Q), 4:2:0
  keep_source_blocks                 with 'keep': the MCUs no blur or draw rectangle touches keep the stored frame's
                                     coefficients (as separate_detections does it, with its guarantees and non-guarantees)
In both 'keep' modes a processed frame on which nothing is drawn and nothing blurred is written as the stored frame, with the
standard Huffman tables written in where it implies them (jpeg_host.with_standard_tables): neither decoded nor encoded.

A frame has two legs that write the same bytes:
  backend='host'   Pillow: feed.load_image of the stored JPEG, blur_detections, the reference's drawing, Image.save with
                   qtables= / subsampling= or quality=.
  backend='gpu'    the device render path (device_render.py; DESIGN.md, "the device render path"), per chunk of frames -- of
                   one video or of several, each with its own size, sampling and tables -- on a context without a model: the
                   frames decoded once (device_decode.decode_scans), ONE mdhip_blur_regions call,
                   ONE mdhip_draw_ops call, ONE mdhip_jpeg_encode_kept and ONE mdhip_jpeg_encode_sampled call, and
                   jpeg_host.sampled_file around each scan.  A frame the device does not restate -- a box thinner than its
                   outline, a stored frame the decoder does not take or flags, tables or a sampling sampled_file does not
                   write, merged blocks no baseline scan holds -- goes to the host leg as a whole ('frames_host').

The same pass: process_video.process_videos(..., render_folder=) writes the same files while it detects (InPassRenderer below):
the device leg's frames are made by the detector (RenderProduct, HIPDetector's render=) from the images it decoded, the rest by
the host leg from the stored bytes the frame source kept; no file is read twice.

Memory: the host leg streams every frame into the writer; the device leg and the same pass hold a video's finished JPEG frames
until its last one is there (chunks end inside videos, batches arrive one by one): about the size of the output file.

Command line:  python -m megadetector_amd.visualize_video_output RESULTS OUT_DIR VIDEO_DIR [the reference's flags]
               [--blur_category_names person] [--blur_radius 40] [--quality keep|1..95] [--keep_source_blocks]
               [--backend gpu|host] [--device 0]
"""

import argparse
import io
import json
import os
import random
import sys

from . import device_render as DR
from . import preview as PV
from .avi import AviError, AviFile, write_mjpeg_avi
from .blur import DEFAULT_BLUR_RADIUS, BlurOptions, blur_rectangle, select_detections
from .constants import DEFAULT_DETECTOR_LABEL_MAP
from .crops import Product
from .ref_utils import clean_filename, insert_before_extension, path_is_abs, quality_argument

DEFAULT_CLASSIFICATION_THRESHOLD = 0.4
DEFAULT_DETECTION_THRESHOLD = 0.15
NO_FRAMES_STRING = 'No frames with detections to process'
SKIPPED_STRING = 'Skipped'
NOT_MJPEG_STRING = 'not a Motion-JPEG AVI'
VIDEO_EXTENSIONS = ('.mp4', '.avi', '.mpeg', '.mpg', '.mov', '.mkv', '.flv')        # detection/video_utils.py:35
DEFAULT_HOST_QUALITY = 85                                 # exif_preserving_save's default_quality: a frame that is no RGB JPEG


class VideoVisualizationOptions:
    """The reference's options, under its names and with its defaults (but fourcc), and ours below them."""

    def __init__(self):
        self.confidence_threshold = DEFAULT_DETECTION_THRESHOLD
        self.sample = -1                                 #: sample N videos (-1: all)
        self.random_seed = None
        self.classification_confidence_threshold = DEFAULT_CLASSIFICATION_THRESHOLD
        self.rendering_fs = 'auto'                       #: fps, 'auto' (from the sampling interval), negative: a speed-up
        self.fourcc = 'MJPG'                             #: (the reference: 'h264') the only codec written here
        self.trim_to_detections = False
        self.output_extension = None
        self.flatten_output = False
        self.path_separator_replacement = '#'
        self.min_output_length_seconds = None
        self.parallelize_rendering = True                #: the host leg's pool; the gpu leg ignores the three
        self.parallelize_rendering_n_cores = 8
        self.parallelize_rendering_with_threads = True
        self.include_category_names_in_filenames = None  #: 'start', 'end' or None
        self.exclude_category_name_strings = None
        self.exclude_category_names = None
        self.include_category_names = None
        # ---- not the reference's ----
        self.blur_category_names = None                  #: a list of detection category names, or 'person,vehicle'
        self.blur_radius = DEFAULT_BLUR_RADIUS
        self.quality = 'keep'                            #: 'keep' or 1 .. 95
        self.keep_source_blocks = False                  #: only with quality 'keep'


# ---- the reference's support functions -----------------------------------------------------------------------------------------

def is_video_file(s):
    return os.path.splitext(s)[1].lower() in VIDEO_EXTENSIONS


def _get_video_output_framerate(video_entry, original_framerate, rendering_fs='auto'):
    """:131-202"""
    if rendering_fs != 'auto':
        if float(rendering_fs) < 0:
            speedup_factor = abs(float(rendering_fs))
            if ('detections' not in video_entry) or (len(video_entry['detections']) == 0):
                return original_framerate * speedup_factor
            frame_numbers = []
            for detection in video_entry['detections']:
                if 'frame_number' in detection:
                    frame_numbers.append(detection['frame_number'])
            if len(frame_numbers) < 2:
                return original_framerate * speedup_factor
            frame_numbers = sorted(set(frame_numbers))
            first_interval = frame_numbers[1] - frame_numbers[0]
            base_output_fps = original_framerate / first_interval
            return base_output_fps * speedup_factor
        else:
            return float(rendering_fs)
    if 'detections' not in video_entry or len(video_entry['detections']) == 0:
        return original_framerate
    frame_numbers = []
    for detection in video_entry['detections']:
        if 'frame_number' in detection:
            frame_numbers.append(detection['frame_number'])
    frame_numbers = sorted(set(frame_numbers))
    if len(frame_numbers) < 2:
        return original_framerate
    first_interval = frame_numbers[1] - frame_numbers[0]
    return original_framerate / first_interval


def _get_frames_to_process(video_entry, confidence_threshold, trim_to_detections=False):
    """:205-272"""
    if 'detections' not in video_entry:
        return []
    if 'frames_processed' in video_entry:
        frame_numbers = set(video_entry['frames_processed'])
    else:
        frame_numbers = set()
    for detection in video_entry['detections']:
        if 'frame_number' in detection:
            if 'frames_processed' in video_entry:
                if detection['frame_number'] not in frame_numbers:
                    print('Warning: frames_processed field present in {}, but frame {} is missing'.format(
                        video_entry['file'], detection['frame_number']))
            frame_numbers.add(detection['frame_number'])
        else:
            print('Warning: detections in {} lack frame numbers'.format(video_entry['file']))
    frame_numbers = sorted(list(frame_numbers))
    if trim_to_detections and (len(frame_numbers) > 0):
        above_threshold_frames = set()
        for detection in video_entry['detections']:
            if detection['conf'] >= confidence_threshold:
                above_threshold_frames.add(detection['frame_number'])
        if len(above_threshold_frames) > 0:
            above_threshold_frames = sorted(list(above_threshold_frames))
            first_detection_frame = above_threshold_frames[0]
            last_detection_frame = above_threshold_frames[-1]
            trimmed_frames = []
            for frame_num in frame_numbers:
                if (first_detection_frame <= frame_num) and (frame_num <= last_detection_frame):
                    trimmed_frames.append(frame_num)
            return trimmed_frames
        else:
            return []
    return frame_numbers


def _get_detections_for_frame(video_entry, frame_number, confidence_threshold):
    """:275-298"""
    if 'detections' not in video_entry:
        return []
    frame_detections = []
    for detection in video_entry['detections']:
        if ((detection['frame_number'] == frame_number) and (detection['conf'] >= confidence_threshold)):
            frame_detections.append(detection)
    return frame_detections


def _get_classification_names(video_entry, classification_label_map, options):
    """:301-343"""
    classification_names = set()
    if ('detections' not in video_entry) or (video_entry['detections'] is None):
        return classification_names
    for det in video_entry['detections']:
        if det['conf'] < options.confidence_threshold:
            continue
        if 'classifications' not in det:
            continue
        for classification in det['classifications']:
            classification_category_id = classification[0]
            classification_conf = classification[1]
            if classification_conf < options.classification_confidence_threshold:
                continue
            classification_category_name = classification_label_map[classification_category_id]
            classification_category_name = clean_filename(classification_category_name, force_lower=True)
            classification_names.add(classification_category_name)
    return classification_names


def plan_video(video_entry, classification_label_map, options, video_dir, out_dir, input_video_path=None):
    """
    _process_video :371-493, everything in front of the first frame that is read: -> (result, plan).  plan is None when the
    result is final (its 'error' says why); else {'input', 'output', 'frames', 'fps'}: the paths, the frame numbers to
    process and the frame rate of the output.  Creates the output file's folder, as the reference does at this point.
    input_video_path: where the video lies, for a caller that knows (process_video); video_dir then only picks the assertion.
    """
    result = {'file': video_entry['file'], 'success': False, 'error': None, 'frames_processed': 0}
    if ('failure' in video_entry) and (video_entry['failure'] is not None):
        result['error'] = 'Ignoring failed video: {}'.format(video_entry['failure'])
        return result, None
    if video_dir is None:
        input_video_path = video_entry['file']
        assert path_is_abs(input_video_path), 'Absolute paths are required when no video base dir is supplied'
    else:
        assert not path_is_abs(video_entry['file']), 'Relative paths are required when a video base dir is supplied'
        input_video_path = input_video_path or os.path.join(video_dir, video_entry['file'])
    if not os.path.exists(input_video_path):
        result['error'] = 'Video not found: {}'.format(input_video_path)
        return result, None
    output_fn_relative = video_entry['file']
    if options.flatten_output:
        output_fn_relative = output_fn_relative.replace('\\', '/')
        output_fn_relative = output_fn_relative.replace('/', options.path_separator_replacement)
    if options.output_extension is not None:
        ext = options.output_extension
        if not ext.startswith('.'):
            ext = '.' + ext
        output_fn_relative = os.path.splitext(output_fn_relative)[0] + ext
    category_names_list = _get_classification_names(video_entry, classification_label_map, options)
    if len(category_names_list) > 0:
        category_names = '_'.join(sorted(list(category_names_list)))
    else:
        category_names = 'none'
    if options.exclude_category_name_strings is not None:
        if isinstance(options.exclude_category_name_strings, str):
            options.exclude_category_name_strings = [options.exclude_category_name_strings]
        if category_names in options.exclude_category_name_strings:
            print('Ignoring category string {} for {}'.format(category_names, output_fn_relative))
            result['error'] = SKIPPED_STRING + ': {}'.format(category_names)
            return result, None
    if options.exclude_category_names is not None:
        if isinstance(options.exclude_category_names, str):
            options.exclude_category_names = [options.exclude_category_names]
        for category_name in category_names_list:
            if category_name in options.exclude_category_names:
                print('Ignoring category {} for {}'.format(category_name, output_fn_relative))
                result['error'] = SKIPPED_STRING + ': {}'.format(category_name)
                return result, None
    if options.include_category_names is not None:
        if isinstance(options.include_category_names, str):
            options.include_category_names = [options.include_category_names]
        found_matching_category = False
        for category_name in category_names_list:
            if category_name in options.include_category_names:
                found_matching_category = True
                break
        if not found_matching_category:
            # (the reference formats `category_name`, the loop's last value, and raises NameError for a video without any
            # classification name: such a video is skipped under the string 'none' here)
            category_name = sorted(category_names_list)[-1] if len(category_names_list) > 0 else category_names
            print('No match to required categories in {} for {}'.format(category_name, output_fn_relative))
            result['error'] = SKIPPED_STRING + ': {}'.format(category_name)
            return result, None
    if options.include_category_names_in_filenames is not None:
        if options.include_category_names_in_filenames == 'start':
            output_fn_relative = category_names + '_' + output_fn_relative
        else:
            output_fn_relative = insert_before_extension(output_fn_relative, category_names, check=True)
    output_fn_abs = os.path.join(out_dir, output_fn_relative)
    parent_dir = os.path.dirname(output_fn_abs)
    if len(parent_dir) > 0:
        os.makedirs(parent_dir, exist_ok=True)
    frames_to_process = _get_frames_to_process(video_entry, options.confidence_threshold, options.trim_to_detections)
    if len(frames_to_process) == 0:
        result['error'] = NO_FRAMES_STRING
        return result, None
    original_framerate = video_entry['frame_rate']
    output_framerate = _get_video_output_framerate(video_entry, original_framerate, options.rendering_fs)
    if options.min_output_length_seconds is not None:
        output_length = len(frames_to_process) / output_framerate
        if output_length < options.min_output_length_seconds:
            print('Skipping video {}, {}s is below minimum length ({}s)'.format(
                video_entry['file'], output_length, options.min_output_length_seconds))
            result['error'] = 'Skipped, below minimum length'
            return result, None
    return result, {'input': input_video_path, 'output': output_fn_abs, 'frames': frames_to_process, 'fps': output_framerate}


# ---- what is drawn on a frame ---------------------------------------------------------------------------------------------------

def check_options(options):
    """what of the options is ours to refuse, before anything is read"""
    from . import jpeg_host
    if options.fourcc != 'MJPG':
        raise NotImplementedError("fourcc {!r}: only 'MJPG' is written".format(options.fourcc))
    if options.quality != 'keep':
        options.quality = jpeg_host.check_quality(options.quality)
        if options.quality > 95:
            raise ValueError("quality is 'keep' or 1 .. 95, got {!r}".format(options.quality))
    if options.keep_source_blocks and options.quality != 'keep':
        raise ValueError("keep_source_blocks needs quality='keep'")
    if not 0.0 <= float(options.blur_radius) <= 512.0:
        raise ValueError('blur radius {!r} is outside 0 .. 512'.format(options.blur_radius))


def _draw_options():
    """render_detection_bounding_boxes' defaults, which the reference's call leaves alone: threshold 0, thickness 4, no
    expansion, 16-pixel arial.ttf, the most confident box on top"""
    return PV.PreviewOptions(confidence_threshold=0, output_image_width=None)


class FramePlanner:
    """The maps and options of one run, and what they make of a frame's detections."""

    def __init__(self, detector_label_map, classification_label_map, options):
        self.label_map, self.classification_label_map, self.options = detector_label_map, classification_label_map, options
        self.draw = _draw_options()
        self.blur = None
        if options.blur_category_names is not None:
            self.blur = BlurOptions(options.blur_category_names, options.confidence_threshold, options.blur_radius)
            self.blur_ids = self.blur.category_ids(detector_label_map)

    def rectangles(self, detections, width, height):
        """the rectangles with area to blur, in the order they are applied (blur.select_detections)"""
        if self.blur is None:
            return []
        rects = [blur_rectangle(d['bbox'], width, height) for d in select_detections(detections, self.blur, self.blur_ids)]
        return [r for r in rects if r is not None]

    def touched(self, detections, width, height):
        """whether anything is drawn on or blurred in a frame of this size with these detections"""
        return len(PV.drawn_detections(detections, self.draw)) > 0 or len(self.rectangles(detections, width, height)) > 0

    def draw_with_pil(self, image, detections):
        """render_detection_bounding_boxes(detections, image, detector_label_map, classification_label_map,
        classification_confidence_threshold=...) by PIL's own calls in the reference's order, IN PLACE"""
        PV.render_with_pil(image, detections, self.draw, self.label_map, classification_label_map=self.classification_label_map,
                           classification_confidence_threshold=self.options.classification_confidence_threshold)

    def plan(self, detections, width, height):
        """draw_with_pil as a preview.RenderPlan, what device_render.blur_and_draw draws.  Raises preview.HostLeg or
        preview.RenderFailure."""
        return PV.render_plan(detections, width, height, self.draw, self.label_map,
                              classification_label_map=self.classification_label_map,
                              classification_confidence_threshold=self.options.classification_confidence_threshold)

    def ops(self, detections, width, height):
        """plan() for a caller that wants the rows and the patches apart: (the rows, a PATCH row's column 5 the index of its
        patch; the patches as a list of bytes).  The device leg takes the plan itself."""
        plan = self.plan(detections, width, height)
        patches = [plan.patch_of(op) for op in plan.ops if op[0] == PV.OP_PATCH]
        at = iter(range(len(patches)))
        return [op[:5] + [next(at)] + op[6:] if op[0] == PV.OP_PATCH else op for op in plan.ops], patches


# ---- one frame -------------------------------------------------------------------------------------------------------------------

def _frame_size(data):
    from PIL import Image
    return Image.open(io.BytesIO(data)).size


def _keep_source(data):
    """jpeg_host.keep_source of a stored frame; 'quant' is None unless Pillow would re-encode it with two 8-bit tables at
    4:4:4 / 4:2:2 / 4:2:0 that jpeg_host.sampled_file writes"""
    from . import jpeg_host
    src = jpeg_host.keep_source(io.BytesIO(data), data)
    if not src['keep'] or len(src['comment'] or b'') > 65533 or max(src['size']) > 65535:
        src['quant'] = None
    return src


def passes_through(data, detections, planner):
    """whether a stored frame (with its tables written in) is written as it is: 'keep', and nothing drawn or blurred"""
    if planner.options.quality != 'keep':
        return False
    width, height = _frame_size(data)
    return not planner.touched(detections, width, height)


def render_frame_host(data, detections, planner):
    """The host leg of one frame that does not pass through: `data` is jpeg_host.with_standard_tables(the stored frame).
    -> the JPEG file of the output frame.  Raises what Pillow raises."""
    from . import jpeg_host
    from .feed import load_image
    options = planner.options
    pil_image = load_image(io.BytesIO(data))
    width, height = pil_image.size
    rects = planner.rectangles(detections, width, height)
    src = keep = None
    if options.quality == 'keep':
        src = _keep_source(data)
        if options.keep_source_blocks and src['quant'] is not None:
            try:
                changed = DR.changed_rectangles(rects, planner.plan(detections, width, height).ops)
                rc, _, coef = jpeg_host.decode(data)
                if rc == jpeg_host.MDJPEG_OK:
                    keep = {'src': src, 'coef': coef, 'size': (width, height), 'changed': changed}
            except Exception:
                keep = None                              # (a drawing the plan does not restate: the frame is encoded whole)
    DR.blur_with_pil(pil_image, rects, options.blur_radius)
    if detections:
        planner.draw_with_pil(pil_image, detections)
    if keep is not None:
        kept = DR.kept_file_host(pil_image, keep)
        if kept is not None:
            return kept
    out = io.BytesIO()
    if options.quality != 'keep':
        pil_image.save(out, 'JPEG', quality=options.quality)
    elif src['quant'] is not None:
        ql, qc = src['quant']
        pil_image.save(out, 'JPEG', qtables=[[int(v) for v in ql], [int(v) for v in qc]], subsampling=src['sampling'])
    elif pil_image.format == 'JPEG':
        pil_image.save(out, 'JPEG', quality='keep')
    else:
        pil_image.save(out, 'JPEG', quality=DEFAULT_HOST_QUALITY)
    return out.getvalue()


def plan_frame_device(data, detections, planner):
    """What the device needs for one frame that does not pass through, before any pixel is decoded: a job for
    device_render.blur_and_draw and its encoders.  Raises preview.HostLeg, also where the reference's own drawing raises (the
    host leg then raises it as the reference does)."""
    from . import jpeg_host
    from .feed import open_for_coefficients
    options = planner.options
    try:
        image, rotation = open_for_coefficients(io.BytesIO(data))
    except Exception as e:
        raise PV.HostLeg(str(e))
    if image.format != 'JPEG' or image.mode != 'RGB' or rotation != 0:
        raise PV.HostLeg('not a plain RGB JPEG')
    rc, scan, reason = jpeg_host.ScanImage.from_bytes(data, 0)
    if rc != jpeg_host.MDJPEG_OK:
        raise PV.HostLeg('a frame the device does not decode: {}'.format(reason))
    width, height = image.size
    job = {'size': (width, height), 'scan': scan, 'exif': b'', 'keep': False}
    if options.quality == 'keep':
        src = _keep_source(data)
        if src['quant'] is None:
            raise PV.HostLeg('tables or a sampling the device does not restate')
        job['sampling'], job['quant'], job['comment'] = src['sampling'], src['quant'], src['comment']
    else:
        comment = image.info.get('comment')
        if len(comment or b'') > 65533 or max(width, height) > 65535:
            raise PV.HostLeg('a comment or a size Pillow refuses')
        job['sampling'], job['quant'], job['comment'] = 2, list(jpeg_host.quant_tables(options.quality)), comment
    job['rects'] = planner.rectangles(detections, width, height)
    try:
        job['plan'] = planner.plan(detections, width, height)
    except PV.RenderFailure as e:
        raise PV.HostLeg(str(e))
    if options.quality == 'keep' and options.keep_source_blocks:
        job['keep'], job['changed'] = True, DR.changed_rectangles(job['rects'], job['plan'].ops)
    return job


def render_decoded(ctx, device, pixels, planes, jobs, planner, profile, clock, stream=0):
    """What follows the decode, for frames whose pixels lie in device memory (device_render): ONE mdhip_blur_regions call, ONE
    mdhip_draw_ops call and ONE call of each encoder the jobs need.  pixels: per job a flat uint8 device tensor (changed in place) or None
    for a frame the decoder flagged; planes: per job None or (device pointer to its quantised planes, what holds them).
    stream: the raw stream of the calls (the caller makes it torch's current one).  -> per job the JPEG file of its output
    frame, None for a frame the host leg has to make (flagged, or no baseline scan holds its merged blocks)"""
    files = [None] * len(jobs)
    live = [k for k in range(len(jobs)) if pixels[k] is not None]
    if not live:
        return files
    tensors, live_jobs = [pixels[k] for k in live], [jobs[k] for k in live]
    blurred, drawn = DR.blur_and_draw(ctx, device, tensors, live_jobs, clock, planner.options.blur_radius, stream)
    profile['blur_calls'] += blurred
    profile['draw_calls'] += drawn
    # (a frame the kept call flagged is the host leg's)
    made, calls, _ = DR.encode_copies(ctx, device, tensors, live_jobs, [planes[k] and planes[k][0] for k in live], clock, False, stream)
    profile['encode_calls'] += calls
    for k, data in zip(live, made):
        files[k] = data
    return files


def render_chunk_device(ctx, torch, device, jobs, planner, profile, clock):
    """The frames of one chunk of the standalone tool: decoded once (device_decode.decode_scans), then render_decoded"""
    from .device_decode import decode_scans
    with clock('decode'):
        pixels, planes = decode_scans(ctx, torch, device, [j['scan'] for j in jobs], any(j['keep'] for j in jobs))
    profile['decode_calls'] += 1
    return render_decoded(ctx, device, pixels, planes, jobs, planner, profile, clock)


# ---- the videos of a run ---------------------------------------------------------------------------------------------------------

class _Video:
    """a video on its way on the device leg: its result, its plan, and its output frames as they are finished.  The frames
    of a chunk come back together and chunks end inside videos, so the finished JPEG frames of a video are held here until
    its last one is there: about the size of the output file, at most 2 GiB (the writer refuses more)."""

    def __init__(self, result, plan, source):
        self.result, self.plan, self.source = result, plan, source
        self.frames, self.pending, self.failed, self.enumerated = [], 0, False, False
        for key in ('frames_copied', 'frames_rendered', 'frames_host'):
            result[key] = 0

    def fail(self, e):
        import traceback
        if not self.failed:
            self.failed = True
            self.result['error'] = 'Error processing video frames: {} ({})'.format(str(e), ''.join(
                traceback.format_exception(type(e), e, e.__traceback__)))

    def finish(self):
        """_process_video :571-616 once the last frame is there: writes the file and completes the result"""
        result = self.result
        self.source.close()
        if self.failed:
            for key in ('frames_copied', 'frames_rendered', 'frames_host'):
                result[key] = 0
            return
        if len(self.frames) > 0:
            try:
                write_mjpeg_avi(self.plan['output'], self.frames, self.plan['fps'], self.source.width, self.source.height)
                result['success'] = True
                result['frames_processed'] = len(self.frames)
            except Exception as e:
                result['error'] = 'Error writing output video: {}'.format(str(e))
        else:
            result['error'] = 'No frames were processed for video {}'.format(result['file'])
        self.frames = None


def _open_video(video_entry, classification_label_map, options, video_dir, out_dir):
    """-> (result, _Video or None)"""
    result, plan = plan_video(video_entry, classification_label_map, options, video_dir, out_dir)
    if plan is None:
        return result, None
    try:
        source = AviFile(plan['input'])
    except (AviError, OSError) as e:
        result['error'] = '{}: {}'.format(NOT_MJPEG_STRING, str(e))
        return result, None
    return result, _Video(result, plan, source)


def _stored_frames(video, video_entry, options):
    """(the stored frame with its tables written in, the detections handed to the renderer) of every frame to process that
    the file holds, in order"""
    from . import jpeg_host
    for frame_number in video.plan['frames']:
        if not 0 <= frame_number < video.source.n_frames:
            continue                                     # (run_callback_on_frames delivers the frames the file has)
        data = jpeg_host.with_standard_tables(video.source.read_frame(frame_number))
        yield data, _get_detections_for_frame(video_entry, frame_number, options.confidence_threshold)


class _FrameError(Exception):
    """making a frame raised: carries what was raised through the writer"""


def _process_video_host(video_entry, planner, classification_label_map, options, video_dir, out_dir):
    """one video of the host leg: every output frame goes to the writer as it is made, none is held"""
    result, video = _open_video(video_entry, classification_label_map, options, video_dir, out_dir)
    if video is None:
        return result

    def frames():
        try:
            for data, detections in _stored_frames(video, video_entry, options):
                if passes_through(data, detections, planner):
                    result['frames_copied'] += 1
                    yield data
                else:
                    made = render_frame_host(data, detections, planner)
                    result['frames_rendered'] += 1
                    result['frames_host'] += 1
                    yield made
        except Exception as e:
            raise _FrameError() from e

    source = video.source
    try:
        n = write_mjpeg_avi(video.plan['output'], frames(), video.plan['fps'], source.width, source.height)
        if n > 0:
            result['success'] = True
            result['frames_processed'] = n
        else:
            os.remove(video.plan['output'])
            result['error'] = 'No frames were processed for video {}'.format(result['file'])
    except _FrameError as e:
        video.fail(e.__cause__)
    except Exception as e:
        result['error'] = 'Error writing output video: {}'.format(str(e))
    finally:
        source.close()
    if not result['success']:
        for key in ('frames_copied', 'frames_rendered', 'frames_host'):
            result[key] = 0
    return result


def _run_host(video_entries, planner, classification_label_map, options, video_dir, out_dir):
    from functools import partial
    worker = partial(_process_video_host, planner=planner, classification_label_map=classification_label_map, options=options,
                     video_dir=video_dir, out_dir=out_dir)
    if not options.parallelize_rendering:
        return [worker(e) for e in video_entries]
    from multiprocessing.pool import Pool, ThreadPool
    kind = ThreadPool if options.parallelize_rendering_with_threads else Pool
    pool = kind() if options.parallelize_rendering_n_cores is None else kind(options.parallelize_rendering_n_cores)
    try:
        return list(pool.imap(worker, video_entries))
    finally:
        pool.close()
        pool.join()


def _run_device(video_entries, planner, classification_label_map, options, video_dir, out_dir, ctx, profile):
    import torch
    from ._lib import HipError
    device = torch.device('cuda:{}'.format(ctx.device))
    clock = DR.Clock(torch, device, profile.get('ms'))
    # (not device_render.chunked: a chunk is rendered as soon as it is full, while the videos are still being read)
    results, chunk, room, device_off = [], [], [DR.DECODE_CHUNK_BYTES], []

    def host_frame(video, slot, data, detections):
        try:
            video.frames[slot] = render_frame_host(data, detections, planner)
            video.result['frames_host'] += 1
        except Exception as e:
            video.fail(e)

    def flush():
        """the device calls of the queued frames, and the files of the videos that are complete with them"""
        jobs = [entry[4] for entry in chunk]
        if jobs:
            profile['chunks'] += 1
            try:
                files = render_chunk_device(ctx, torch, device, jobs, planner, profile, clock)
            except HipError as e:
                # not a refusal this code expects: nothing more is started on the device in this run, PIL makes the rest
                print('Warning: rendering {} frames on the device failed ({}); the device leg ends here, PIL renders every '
                      'further frame'.format(len(jobs), e))
                device_off.append(e)
                files = [None] * len(jobs)
            for (video, slot, data, detections, _), made in zip(chunk, files):
                if made is None:
                    host_frame(video, slot, data, detections)
                else:
                    video.frames[slot] = made
                video.pending -= 1
        for video in {id(entry[0]): entry[0] for entry in chunk}.values():
            if video.pending == 0 and video.enumerated:
                video.finish()
        del chunk[:]
        room[0] = DR.DECODE_CHUNK_BYTES

    with torch.cuda.device(device):
        for video_entry in video_entries:
            result, video = _open_video(video_entry, classification_label_map, options, video_dir, out_dir)
            results.append(result)
            if video is None:
                continue
            try:
                for data, detections in _stored_frames(video, video_entry, options):
                    if passes_through(data, detections, planner):
                        video.frames.append(data)
                        result['frames_copied'] += 1
                        continue
                    result['frames_rendered'] += 1
                    video.frames.append(None)
                    slot = len(video.frames) - 1
                    try:
                        if device_off:
                            raise PV.HostLeg('the device leg has ended')
                        job = plan_frame_device(data, detections, planner)
                    except PV.HostLeg:
                        host_frame(video, slot, data, detections)
                        continue
                    size = job['size'][0] * job['size'][1] * 3 + (2 * int(job['scan'].coef_count) if job['keep'] else 0)
                    if chunk and size > room[0]:
                        flush()
                    chunk.append((video, slot, data, detections, job))
                    video.pending += 1
                    room[0] -= size
            except Exception as e:
                video.fail(e)
            video.enumerated = True
            if video.pending == 0:
                video.finish()
        flush()
        if not device_off:
            torch.cuda.synchronize(device)
    return results


# ---- the same pass: process_video renders what it decoded ---------------------------------------------------------------------------

class RenderProduct(Product):
    """render=: result['rendered_frame'] = the JPEG file of the output frame, made from the frame's pixels in device memory
    (and, for keep_source_blocks, from the coefficient planes the entropy decoder left there); None for a frame that is
    written as stored or that the host leg has to make.  options: an InPassRenderer."""

    key = 'rendered_frame'
    wants_source = True              #: entries carry a sixth element, the image as the detector holds it ('img_original')

    def nothing(self):
        return None

    def _host(self, pixels, name, detections):
        return None, None

    def _device(self, ctx, entries, stream):
        return self.options.frames_of_device_images(ctx, entries, stream)


class InPassRenderer:
    """
    The annotated videos of a detection pass (process_video): per video, the stored JPEG of every processed frame is kept as
    it is read (MJPEGAVIFrameSource.remember), the output frame of each is made when its detections are there -- on the device
    leg by RenderProduct from the image the pass decoded, else by the standalone tool's own functions from the stored bytes --
    and when the video ends plan_video decides, from the entry the results file will hold, whether and where it is written,
    which frames and at which rate.  The files are those visualize_video_output writes from the pass's JSON.  `results` gets
    the result dict of every video.
    """

    def __init__(self, render_folder, options=None):
        options = VideoVisualizationOptions() if options is None else options
        check_options(options)
        self.folder, self.options = render_folder, options
        self.planner = FramePlanner(DEFAULT_DETECTOR_LABEL_MAP, {}, options)      # the maps write_results_to_file writes
        self.profile = {key: 0 for key in ('blur_calls', 'draw_calls', 'encode_calls')}
        self.results = []
        self.stored, self.frames, self.on_device = {}, {}, False

    def begin_video(self, source):
        """source: the video's frame source; only an MJPEGAVIFrameSource is rendered"""
        self.stored, self.frames = {}, {}
        self.on_device = bool(getattr(source, 'device', False))
        if hasattr(source, 'avi'):
            source.remember = self.stored

    def frame_detections(self, detections):
        """_get_detections_for_frame of the results file to come: its order (confidence descending, stable) and the threshold"""
        from .crops import output_order
        return [d for d in output_order(detections) if d['conf'] >= self.options.confidence_threshold]

    def frames_of_device_images(self, ctx, entries, stream=0):
        """entries: [(tensor, width, height, frame name, detections, the detector's image)], the tensors NOT changed.  ONE blur,
        ONE draw and ONE call of each encoder for the frames of the batch that are rendered on the device."""
        import torch
        from .crops import device_stream
        from .jpeg_host import DeviceCoefficientImage
        out, jobs, where = [None] * len(entries), [], []
        for e, (tensor, width, height, name, detections, source) in enumerate(entries):
            data = self.stored.get(name)
            if data is None or not isinstance(source, DeviceCoefficientImage):
                continue                                 # (a frame Pillow decoded for the pass: the host leg, as in the tool)
            dets = self.frame_detections(detections)
            try:
                if passes_through(data, dets, self.planner):
                    continue
                job = plan_frame_device(data, dets, self.planner)
            except Exception:
                continue                                 # (the host leg makes it, or raises what the tool raises)
            if job['size'] != (width, height):
                continue
            job['planes'] = (source.coef.data_ptr(), source.coef) if job['keep'] else None
            jobs.append(job)
            where.append(e)
        if not jobs:
            return out, {'gpu': 0}
        device = entries[0][0].device
        ext = device_stream(stream, device)
        with torch.cuda.stream(ext):
            pixels = [entries[e][0].clone() for e in where]
            files = render_decoded(ctx, device, pixels, [j['planes'] for j in jobs], jobs, self.planner, self.profile,
                                   DR.Clock(torch, device, None), ext.cuda_stream)
        for e, data in zip(where, files):
            out[e] = data
        return out, {'gpu': sum(f is not None for f in files)}

    def take(self, results):
        """the detector's results of some frames of the video (their 'file' is the frame's name): takes the rendered frame out
        of each, or makes the output frame as the standalone tool does"""
        import re
        for r in results:
            name = os.path.basename(r['file'])
            made = r.pop(RenderProduct.key, None)
            data = self.stored.pop(name, None)
            if data is None:
                continue                                 # (no Motion-JPEG source: nothing is rendered)
            n = int(re.search(r'frame(\d+)\.jpg', name).group(1))
            try:
                dets = self.frame_detections(r.get('detections'))
                if made is not None:
                    self.frames[n] = (made, 'gpu')
                elif passes_through(data, dets, self.planner):
                    self.frames[n] = (data, 'copied')
                else:
                    self.frames[n] = (render_frame_host(data, dets, self.planner), 'host')
            except Exception as e:
                self.frames[n] = (e, 'failed')

    def end_video(self, video_entry, path, source):
        """video_entry: the video's entry as the results file will hold it; writes the video, appends its result"""
        result, plan = plan_video(video_entry, {}, self.options, '', self.folder, input_video_path=path)
        frames, self.frames, self.stored = self.frames, {}, {}
        if plan is not None and not hasattr(source, 'avi'):
            result['error'], plan = '{}: {}'.format(NOT_MJPEG_STRING, path), None
        if plan is not None:
            video = _Video(result, plan, source.avi)
            for n in plan['frames']:
                if n not in frames:
                    continue
                data, how = frames[n]
                if how == 'failed':
                    video.fail(data)
                    break
                video.frames.append(data)
                result['frames_copied' if how == 'copied' else 'frames_rendered'] += 1
                result['frames_host'] += how == 'host'
            video.finish()
        for key in ('frames_copied', 'frames_rendered', 'frames_host'):
            result.setdefault(key, 0)
        self.results.append(result)
        return result


# ---- the entry function ----------------------------------------------------------------------------------------------------------

def visualize_video_output(detector_output_path, out_dir, video_dir, options=None, backend='gpu', device=0, ctx=None, profile=None):
    """
    The reference's visualize_video_output(detector_output_path, out_dir, video_dir, options) for Motion-JPEG AVI files.
    backend 'host': Pillow, no GPU; 'gpu': the frames on HIP device `device`, on `ctx` (a HipContext) or on a context
    without a model made for the call.  profile: a dict that receives 'chunks' and the numbers of 'decode_calls', 'blur_calls',
    'draw_calls' and 'encode_calls' of the gpu leg; when it holds a dict under 'ms', also the milliseconds around each kind of
    device call (the device is waited for around each: slower).
    Returns the reference's list of results, one per video -- 'file', 'success', 'error', 'frames_processed' -- each with
    'frames_copied' (written as stored), 'frames_rendered' (decoded, changed and encoded) and of these 'frames_host' (made by
    the host leg).
    """
    if backend not in ('gpu', 'host'):
        raise ValueError("backend must be 'gpu' or 'host', not {!r}".format(backend))
    if options is None:
        options = VideoVisualizationOptions()
    check_options(options)
    if (video_dir is not None) and (os.path.abspath(out_dir) == os.path.abspath(video_dir)):
        raise ValueError('Output directory cannot be the same as video directory')
    print('Loading results from {}'.format(detector_output_path))
    with open(detector_output_path, 'r') as f:
        results_data = json.load(f)
    assert 'images' in results_data, 'Detector output file should be a json file with an "images" field.'
    detector_label_map = results_data.get('detection_categories', DEFAULT_DETECTOR_LABEL_MAP)
    classification_label_map = results_data.get('classification_categories', {})
    video_entries = []
    for entry in results_data['images']:
        if is_video_file(entry['file']):
            video_entries.append(entry)
    print('Found {} videos in results file'.format(len(video_entries)))
    if (options.sample is not None) and (options.sample > 0) and (len(video_entries) > options.sample):
        if options.random_seed is not None:
            random.seed(options.random_seed)
        n_videos_available = len(video_entries)
        video_entries = random.sample(video_entries, options.sample)
        print('Sampled {} of {} videos for processing'.format(len(video_entries), n_videos_available))
    os.makedirs(out_dir, exist_ok=True)
    planner = FramePlanner(detector_label_map, classification_label_map, options)
    profile = {} if profile is None else profile
    for key in ('chunks', 'decode_calls', 'blur_calls', 'draw_calls', 'encode_calls'):
        profile[key] = 0
    if backend == 'host':
        results = _run_host(video_entries, planner, classification_label_map, options, video_dir, out_dir)
    else:
        from .hip_backend import HipContext
        with HipContext.images_or(ctx, device) as ctx:
            results = _run_device(video_entries, planner, classification_label_map, options, video_dir, out_dir, ctx, profile)
    for r in results:
        for key in ('frames_copied', 'frames_rendered', 'frames_host'):
            r.setdefault(key, 0)
    n_empty = n_failed = n_successful = n_skipped = 0
    for r in results:
        if r['success']:
            assert r['error'] is None
            n_successful += 1
        else:
            assert r['error'] is not None
            if NO_FRAMES_STRING in r['error']:
                n_empty += 1
            elif SKIPPED_STRING in r['error']:
                n_skipped += 1
            else:
                n_failed += 1
    total_frames = sum(r['frames_processed'] for r in results if r['success'])
    print('\nProcessing complete:')
    print('  Successfully processed: {} videos'.format(n_successful))
    print('  No above-threshold detections: {} videos'.format(n_empty))
    print('  Failed: {} videos'.format(n_failed))
    print('  Skipped: {} videos'.format(n_skipped))
    print('  Total frames rendered: {}'.format(total_frames))
    return results


# ---- command line ----------------------------------------------------------------------------------------------------------------

def main(argv=None):
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                     description='Render videos with bounding boxes predicted by a detector above a confidence '
                                                 'threshold, and save the rendered videos.')
    parser.add_argument('detector_output_path', type=str, help='Path to json output file of the detector')
    parser.add_argument('out_dir', type=str, help='Path to directory where the rendered videos will be saved. '
                                                  'The directory will be created if it does not exist.')
    parser.add_argument('video_dir', type=str, help='Path to directory containing the input videos')
    parser.add_argument('--confidence_threshold', type=float, default=DEFAULT_DETECTION_THRESHOLD,
                        help='Confidence threshold above which detections will be rendered')
    parser.add_argument('--sample', type=int, default=-1,
                        help='Number of videos to randomly sample for processing. Set to -1 to process all videos')
    parser.add_argument('--random_seed', type=int, default=None, help='Random seed for reproducible sampling')
    parser.add_argument('--classification_confidence_threshold', type=float, default=DEFAULT_CLASSIFICATION_THRESHOLD,
                        help='Value between 0 and 1, indicating the confidence threshold above which classifications will be rendered')
    parser.add_argument('--rendering_fs', default='auto',
                        help='Frame rate for output videos. Use "auto" to calculate based on detection frame intervals, positive '
                             'float for explicit fps, or negative float for speedup factor (e.g. -2.0 = 2x faster)')
    parser.add_argument('--fourcc', type=str, default='MJPG', help="Fourcc codec specification for video encoding (only 'MJPG')")
    parser.add_argument('--trim_to_detections', action='store_true',
                        help='Skip frames before first and after last above-threshold detection')
    parser.add_argument('--blur_category_names', type=str, default=None,
                        help='Comma-separated detection category names to blur before drawing, e.g. "person" (not in the reference)')
    parser.add_argument('--blur_radius', type=float, default=DEFAULT_BLUR_RADIUS, help='Radius of the blur (not in the reference)')
    parser.add_argument('--quality', type=quality_argument, default='keep',
                        help="'keep': re-encode a touched frame with the stored frame's tables and sampling; 1 .. 95: Pillow's "
                             "quality, 4:2:0 (not in the reference)")
    parser.add_argument('--keep_source_blocks', action='store_true',
                        help="With --quality keep: untouched MCUs keep the stored frame's JPEG blocks (not in the reference)")
    parser.add_argument('--backend', choices=('host', 'gpu'), default='gpu', help="'host': Pillow, no GPU needed")
    parser.add_argument('--device', type=int, default=0, help='HIP device of the gpu backend')
    args = parser.parse_args(argv)
    options = VideoVisualizationOptions()
    for name in ('confidence_threshold', 'sample', 'random_seed', 'classification_confidence_threshold', 'rendering_fs', 'fourcc',
                 'trim_to_detections', 'blur_category_names', 'blur_radius', 'quality', 'keep_source_blocks'):
        setattr(options, name, getattr(args, name))
    visualize_video_output(args.detector_output_path, args.out_dir, args.video_dir, options, backend=args.backend, device=args.device)
    return 0


if __name__ == '__main__':
    sys.exit(main())
