"""
HIPDetector: drop-in for the reference's PTDetector
(megadetector/detection/pytorch_detector.py:739-1480) with the per-batch hot path running as
hand-written HIP on one MI355X (libmdhip.so).

Same constructor, same three public methods, same return dicts and failure conventions
(SURVEY.md section 8(b)):
  preprocess_image(img, image_id, image_size, verbose)            -> dict      (:964)
  generate_detections_one_batch(imgs, ids, threshold, ...)        -> list[dict] (:1124)
  generate_detections_one_image(img, id, threshold, ...)          -> dict      (:1428)

Differences, all deliberate and documented in DESIGN.md:
  * the letterbox resize runs on the GPU, so `preprocess_image` only computes the letterbox
    geometry; 'img_processed' is a LetterboxSpec placeholder exposing `.shape` (dicts carrying
    a real letterboxed ndarray, e.g. from the reference's own preprocessing workers, are
    accepted too);
  * in the non-classic compatibility modes the pre-resize (cv2.INTER_AREA / INTER_LINEAR to the long side) runs on
    the GPU as well; 'img_original' stays the caller's array and 'resized_shape' carries the resized size.
augment=True runs yolov5's augmented inference (three scaled / flipped passes) on the device
(mdhip_forward_tta).
An image may also arrive as a jpeg_host.CoefficientImage (the quantised DCT coefficients of a baseline JPEG, feed.py
decode='coefficients'): its pixels are rebuilt on the device (mdhip_jpeg_reconstruct), bit for bit what PIL decodes, and
never exist on the host; `jpeg_images_reconstructed` counts them.  Or as a jpeg_host.ScanImage (the compressed file and the
descriptor of its scan, feed.py decode='scan'): decode_scans() Huffman-decodes those on the device first
(mdhip_jpeg_entropy_decode; `jpeg_images_entropy_decoded` counts them) and decodes a file the GPU flags with PIL from the
bytes it holds (`jpeg_entropy_fallbacks`).
The device is driven in one way: start_batch() enqueues the groups of a batch on the detector's streams and finish_batch()
collects them; generate_detections_one_batch is the two in one call and generate_detections_for_tiles runs its chunks through
the same runner (_run_group / _collect_group), behind the windowed letterbox.
"""

import json
import os

import numpy as np

from . import weights_io
from .blur import BlurProduct
from .classify import ClassifyProduct
from .crops import CropProduct
from .preview import PreviewProduct
from .constants import (FAILURE_IMAGE_OPEN, FAILURE_INFER, DEFAULT_COMPATIBILITY_MODE)
from .jpeg_host import CoefficientImage, DeviceCoefficientImage, ScanFailure, ScanImage, check_quality
from .postprocess import letterbox_geometry, modern_geometry, format_detections


def parse_bool_string(s):
    """reference megadetector/utils/ct_utils.py:1000"""
    if isinstance(s, bool):
        return s
    s = str(s).lower().strip()
    if s in ('true', '1', 'yes', 'y'):
        return True
    if s in ('false', '0', 'no', 'n'):
        return False
    raise ValueError('Cannot convert "{}" to bool'.format(s))


class LetterboxSpec:
    """Placeholder for the letterboxed image: the pixels are produced on the GPU."""

    __slots__ = ('shape', 'geometry')

    def __init__(self, shape, geometry):
        self.shape = tuple(shape)
        self.geometry = tuple(geometry)    # (src_h, src_w, resized_h, resized_w, top, left)

    def __reduce__(self):
        return (LetterboxSpec, (self.shape, self.geometry))


def _device_ordinal(device):
    s = str(device).lower()
    if s.startswith('cuda'):
        return int(s.split(':')[1]) if ':' in s else 0
    raise ValueError('HIPDetector needs a GPU device ("cuda:N"), got {}'.format(device))


# storage type when detector_options does not name one (see HIPDetector.__init__)
DEFAULT_DTYPE = 'fp16'


class HIPDetector:

    def __init__(self, model_path, detector_options=None, verbose=False):
        """
        model_path: a YOLOv5 .pt checkpoint (md_v5a.0.0.pt ...), a YoloWeights object, or the
        string 'synthetic[:yaml_name[:seed]]' for seeded weights on the MDv5 topology.
        detector_options keys honoured: force_cpu (must be false), use_model_native_classes,
        compatibility_mode, preprocess_only, device, batch_size, max_image_size, dtype, hip_graph ('auto' | 'on' | 'off').
        dtype: storage type of activations and packed weights (accumulation is fp32 either way).  Default 'fp16':
        |d conf| against the fp32 evaluation the reference performs stays below the reference's own bar between
        environments (0.005-0.01, md_tests.py:96-100,1779) with an 8x margin on every model measured
        (profiles/r2a_accuracy_x6.txt); 'bf16' is the throughput configuration BASELINE.json names (3 % faster,
        8 significant bits); 'fp8' is BASELINE.json configs[4]: bf16 storage, the bottleneck 3x3 convs on e4m3 operands;
        its static activation scales come from `fp8_scales` (a list saved from an earlier run, HipContext.fp8_scales)
        or, without it, from the FIRST batch this detector processes (mdhip_calibrate) -- results then depend on that
        batch; a stated-tolerance throughput mode, not a reference-grade one (tests/test_gpu_fp8.py).
        """
        opts = dict(detector_options or {})
        self.use_model_native_classes = parse_bool_string(opts.get('use_model_native_classes', False))
        compat = opts.get('compatibility_mode') or DEFAULT_COMPATIBILITY_MODE
        self.compatibility_mode = compat
        preprocess_only = bool(opts.get('preprocess_only', False))
        if verbose or not preprocess_only:
            print('Loading HIP detector with compatibility mode {}'.format(compat))

        self.model_metadata = None
        if isinstance(model_path, str) and not model_path.startswith('synthetic'):
            self.model_metadata = weights_io.read_metadata_from_megadetector_model_file(model_path)
        if self.model_metadata is not None and 'image_size' in self.model_metadata:
            self.default_image_size = self.model_metadata['image_size']
            print('Loaded image size {} from model metadata'.format(self.default_image_size))
        else:
            # reference pytorch_detector.py:802-805
            if not preprocess_only:
                print('No image size available in model metadata, defaulting to 1280')
            self.default_image_size = 1280
        self.device = 'cpu'
        self.printed_image_size_warning = False
        # reference :827-845
        self.letterbox_stride = 64 if self.default_image_size == 1280 else 32
        self.half_precision = False
        self.model = None
        self._ctx = None
        self.jpeg_images_reconstructed = 0      # images whose pixels were rebuilt on the device from JPEG coefficients
        self.jpeg_images_entropy_decoded = 0    # of those: images whose scan was Huffman-decoded on the device too
        self.crop_counts = {'gpu': 0, 'host': 0, 'skipped': 0}      # crops= : encoded on the device / saved by PIL / without area
        self.blur_counts = {'gpu': 0, 'host': 0}                    # blur= : copies encoded on the device / saved by PIL
        self.render_counts = {'gpu': 0}                             # render= : video frames made on the device
        self.preview_counts = {'gpu': 0, 'host': 0, 'skipped': 0}   # preview= : encoded on the device / rendered or saved by PIL / no file
        self.classify_counts = {'gpu': 0, 'host': 0, 'skipped': 0}  # classify= : crops made by the kernel / by PIL / without a crop
        self.jpeg_entropy_fallbacks = 0         # scans the device flagged: decoded with PIL from the file's bytes instead
        if preprocess_only:
            return                      # never touches HIP: safe in forked producer processes

        if parse_bool_string(opts.get('force_cpu', False)):
            raise RuntimeError('HIPDetector has no CPU path (force_cpu requested)')
        device = opts.get('device') or 'cuda:0'
        self.device = device
        # AddaxAI parses this line from the reference (pytorch_detector.py:885)
        print('PTDetector using device {}'.format(str(self.device).lower()))

        if isinstance(model_path, str):
            if model_path.startswith('synthetic'):
                parts = model_path.split(':')
                from . import yolo_yaml
                yaml = getattr(yolo_yaml, parts[1]) if len(parts) > 1 and parts[1] else yolo_yaml.YOLOV5X6_MD
                seed = int(parts[2]) if len(parts) > 2 else 0
                weights = weights_io.synthetic_weights(yaml, seed=seed)
            else:
                weights = weights_io.load_checkpoint(model_path)
        else:
            weights = model_path
        self.weights = weights
        # YOLO11 (MDv1000-larch / -sorrel): the reference runs them through the ultralytics package -- its NMS and its
        # scale_boxes (pytorch_detector.py:395-402, :1327-1344); the library picks the NMS from the model's head
        self.anchor_free = bool(getattr(weights, 'anchor_free', False))
        # YOLOv9-C (MDv1000-cedar): the reference runs it through the yolov9 package -- its NMS (the same rule; the library's
        # anchor-free NMS) and its YOLOv5-style scale_boxes, which does NOT round the padding
        self.yolov9 = bool(getattr(weights, 'yolov9', False))
        if self.anchor_free and str(opts.get('dtype') or DEFAULT_DTYPE).lower() == 'fp8':
            raise ValueError("dtype 'fp8' is implemented for YOLOv5 models only; use 'fp16' or 'bf16' for a {} model".format(
                'YOLOv9' if self.yolov9 else 'YOLO11'))
        if weights.max_stride != self.letterbox_stride and verbose:
            print('*** Warning: model stride is {}, letterbox stride is {} ***'.format(
                weights.max_stride, self.letterbox_stride))
        # fp8 mode: where do the static activation scales come from?  Decided before anything touches the GPU, so that
        # a missing calibration is an immediate, clear error (also in the parent of a multi-GPU run)
        self._fp8_pending = False
        self._fp8_scales_file = opts.get('fp8_scales_file') or None
        fp8_scales = None
        if str(opts.get('dtype') or DEFAULT_DTYPE).lower() == 'fp8':
            fp8_scales = opts.get('fp8_scales')
            if isinstance(fp8_scales, str):                   # "a;b;c" from a key=value command line
                fp8_scales = [v for v in fp8_scales.replace(';', ' ').split() if v]
            if not fp8_scales and self._fp8_scales_file and os.path.isfile(self._fp8_scales_file):
                with open(self._fp8_scales_file, 'r') as f:
                    fp8_scales = json.load(f)['fp8_scales']
            if not fp8_scales:
                if parse_bool_string(opts.get('fp8_calibrate_on_first_batch', False)):
                    # explicit opt-in: the scales then come from whatever batch arrives first, i.e. the output depends
                    # on file order / batch size / shard; with fp8_scales_file they are saved for the next run
                    self._fp8_pending = True
                else:
                    raise ValueError(
                        "dtype 'fp8' needs its activation scales: pass detector_options['fp8_scales'] (a list saved "
                        "from HipContext.fp8_scales) or ['fp8_scales_file'] (json written by an earlier calibration), or "
                        "opt into calibrating on the first batch with ['fp8_calibrate_on_first_batch']=True -- results "
                        "then depend on that batch")
        from .hip_backend import HipContext
        self.max_batch = int(opts.get('batch_size', 1)) if int(opts.get('batch_size', 1)) > 1 else int(opts.get('max_batch', 8))
        max_size = int(opts.get('max_image_size', self.default_image_size))
        max_size = -(-max_size // weights.max_stride) * weights.max_stride
        if 'classic' not in compat:
            max_size += weights.max_stride      # the modern target shape is ceil(size / stride + 0.5) * stride
        self._ctx = HipContext(weights, device=_device_ordinal(device), dtype=opts.get('dtype') or DEFAULT_DTYPE,
                               max_batch=self.max_batch, max_h=max_size, max_w=max_size)
        self.model = self._ctx
        # launch plumbing, off by default: replaying the forward from a captured graph ('on'; 'auto' = batches <= 8) was
        # measured and changes nothing -- at batch 1 .. 8 the step is bound by its kernels, not by their launches
        self._ctx.set_graph(opts.get('hip_graph', 'off'))
        if fp8_scales:
            self._ctx.set_fp8_scales([float(v) for v in fp8_scales])

    # -----------------------------------------------------------------------------------
    def preprocess_image(self, img_original, image_id='unknown', image_size=None, verbose=False):
        """reference pytorch_detector.py:964-1119 ('classic'): geometry only, pixels stay put."""
        result = {'file': image_id}
        img_original_pil = None
        if isinstance(img_original, CoefficientImage):
            pass                                # .shape is the decoded, rotated image's; the pixels are made on the device
        elif not isinstance(img_original, np.ndarray):
            img_original_pil = img_original
            img_original = np.asarray(img_original)
        if img_original.ndim != 3 or img_original.shape[2] != 3 or img_original.dtype != np.uint8:
            raise ValueError('expected an HxWx3 uint8 RGB image, got {} {}'.format(
                img_original.shape, img_original.dtype))
        scaling_shape = img_original.shape
        if image_size is not None:
            assert isinstance(image_size, int)
            if not self.printed_image_size_warning:
                print('Using user-supplied image size {}'.format(image_size))
                self.printed_image_size_warning = True
        else:
            image_size = self.default_image_size
            self.printed_image_size_warning = False
        if 'classic' in self.compatibility_mode:
            g = letterbox_geometry(img_original.shape[:2], new_shape=image_size, stride=self.letterbox_stride,
                                   auto=True, scaleup=True)
            geometry = (img_original.shape[0], img_original.shape[1], g['new_unpad'][1], g['new_unpad'][0],
                        g['top'], g['left'], 0)
            target_shape = image_size
        else:
            # 'modern' (reference :1036-1101): resize to the long side (INTER_AREA when shrinking) and pad into the
            # target shape -- both on the device; the reference replaces img_original by the resized image, here
            # the pixels stay put and 'resized_shape' carries what the box rescaling needs
            m = modern_geometry(img_original.shape[:2], image_size, self.letterbox_stride,
                                use_ceil='use_ceil_for_resize' in self.compatibility_mode)
            g = m['letterbox']
            geometry = (img_original.shape[0], img_original.shape[1], m['resized_hw'][0], m['resized_hw'][1],
                        g['top'], g['left'], m['interp'])
            target_shape = m['target_shape']
            result['resized_shape'] = (m['resized_hw'][0], m['resized_hw'][1], 3)
        result['img_processed'] = LetterboxSpec((g['out_hw'][0], g['out_hw'][1], 3), geometry)
        result['img_original'] = img_original
        result['img_original_pil'] = img_original_pil
        result['target_shape'] = target_shape
        result['scaling_shape'] = scaling_shape
        result['letterbox_ratio'] = g['ratio']
        result['letterbox_pad'] = g['pad']
        return result

    # -----------------------------------------------------------------------------------
    supports_crops = True
    supports_blur = True
    supports_preview = True
    supports_classify = True

    def generate_detections_one_batch(self, img_original, image_id=None, detection_threshold=0.00001,
                                      image_size=None, augment=False, verbose=False, crops=None, blur=None, preview=None,
                                      classify=None, render=None):
        """reference pytorch_detector.py:1124-1252.  crops (a crops.CropOptions, default None = off): every result dict gains
        'crops', a list of (crop_id, crop_filename_relative, bytes) -- the files create_crop_folder.py writes for the
        image's detections, encoded on the device from the pixels that are resident there (mdhip_jpeg_encode).
        blur (a blur.BlurOptions, default None = off): every result dict gains 'blurred' -- None when nothing in the image is
        to be blurred, otherwise the bytes of the file separate_detections_into_folders.py --category_names_to_blur writes
        for it: a COPY of the resident image is blurred (mdhip_blur_regions) and encoded whole on the device; the pixels
        detection and crops= read are not changed, and crops are cut from the unblurred image.
        preview (a preview.PreviewOptions, default None = off): every result dict gains 'preview', a pair (bytes or None,
        leg) -- the file visualize_detector_output.py writes for the image (blurred if asked, resized with Pillow's LANCZOS
        filter, boxes and labels drawn), made on the device from the resident pixels (mdhip_blur_regions on a copy,
        mdhip_resample_lanczos, mdhip_draw_ops, mdhip_jpeg_encode); leg is 'gpu', 'host' (PIL saved or rendered it) or
        'skipped' (no file).  The resident pixels are not changed.
        classify (a classify.ClassifyOptions, default None = off): every result dict gains 'classifications', a list of
        (detection_index, [[class_id, conf], ...]) -- what classification/run_classifier.py and
        merge_classification_detection_output.py give the image's detections: the crops of a group go from the resident,
        unblurred pixels to the model's input tensor in one launch per chunk (mdhip_classifier_input), the model runs on
        the same stream, and the probabilities come back in one copy."""
        if not isinstance(img_original, list):
            raise ValueError('img_original must be a list for batch processing')
        if len(img_original) == 0:
            return []
        if isinstance(img_original[0], dict):
            for i, img in enumerate(img_original):
                if not isinstance(img, dict):
                    raise ValueError('Mixed input types in batch: item {} is not a dict, but item 0 is a dict'.format(i))
        else:
            if image_id is None:
                raise ValueError('image_id must be a list when img_original contains PIL/numpy images')
            if not isinstance(image_id, list):
                raise ValueError('image_id must be a list for batch processing')
            if len(image_id) != len(img_original):
                raise ValueError('Length mismatch: img_original has {} items, image_id has {} items'.format(
                    len(img_original), len(image_id)))
            for i_img, img in enumerate(img_original):
                if isinstance(img, dict):
                    raise ValueError('Mixed input types in batch: item {} is a dict, but item 0 is not a dict'.format(i_img))
        # one group in flight at a time: each chunk is collected before the next is enqueued, the last one here
        return self.finish_batch(self.start_batch(img_original, image_id, detection_threshold, image_size, augment, verbose,
                                                  crops=crops, blur=blur, preview=preview, classify=classify, render=render))

    def _products(self, crops, blur, preview, classify=None, render=None):
        """the products asked for (crops.Product), in the order their kernels are enqueued"""
        asked = ((CropProduct, crops, self.crop_counts), (ClassifyProduct, classify, self.classify_counts),
                 (BlurProduct, blur, self.blur_counts), (PreviewProduct, preview, self.preview_counts))
        if render is not None:                             # (process_video's annotated videos: visualize_video_output.py)
            from .visualize_video_output import RenderProduct
            asked += ((RenderProduct, render, self.render_counts),)
        return [product(options, counts) for product, options, counts in asked if options is not None]

    @staticmethod
    def _products_everywhere(results, products):
        """an image that failed has no crops, no blurred copy and no preview, as the reference's second passes give it none"""
        for product in products:
            for r in results:
                if r is not None:
                    r.setdefault(product.key, product.nothing())
        return results

    def _add_products(self, group_items, tensors, results, products, stream=0):
        """the products of the results of one group: tensors[i] holds the pixels of group_items[i] on the device.  For each
        product one round of device calls and one read-back for the group.  An image that came already letterboxed has its
        source pixels on the host only: crops are cut from the letterboxed pixels on the device, every other product is made
        from 'img_original' by its host leg."""
        for product in products:
            entries, where = [], []
            for (original_idx, info, current_id), t in zip(group_items, tensors):
                r = results[original_idx]
                if not product.selects(r):
                    continue
                if isinstance(info['img_processed'], LetterboxSpec):
                    hh, ww = info['img_original'].shape[:2]
                elif product.letterboxed_on_device:
                    hh, ww = info['img_processed'].shape[:2]
                else:
                    r[product.key] = product.of_host_image(np.asarray(info['img_original']), current_id, r['detections'])
                    continue
                entry = (t, ww, hh, current_id, r['detections'])
                # a product that wants it also gets the image as it came: a DeviceCoefficientImage's planes are still on the device
                entries.append(entry + (info['img_original'],) if getattr(product, 'wants_source', False) else entry)
                where.append(original_idx)
            if entries:
                for original_idx, value in zip(where, product.of_device_images(self._ctx, entries, stream)):
                    results[original_idx][product.key] = value

    def _prepare_batch(self, img_original, image_id, image_size, verbose):
        """per-image preprocessing with failure capture (reference :1194-1222) and grouping by processed
        shape (:1226-1233); returns (results with the failed slots filled in, {shape: [(idx, info, id)]})"""
        results = [None] * len(img_original)
        preprocessed = []
        for i_img, img in enumerate(img_original):
            try:
                if isinstance(img, dict):
                    info = img
                    current_id = info['file']
                else:
                    current_id = image_id[i_img]
                    if isinstance(img, ScanFailure):
                        raise img.error
                    info = self.preprocess_image(img, image_id=current_id, image_size=image_size, verbose=verbose)
                preprocessed.append((i_img, info, current_id))
            except Exception as e:
                current_id = image_id[i_img] if image_id else 'index_{}'.format(i_img)
                print('Warning: preprocessing failed for image {}: {}'.format(current_id, str(e)))
                results[i_img] = {'file': current_id, 'detections': None, 'failure': FAILURE_IMAGE_OPEN}
        shape_groups = {}
        for item in preprocessed:
            shape_groups.setdefault(tuple(item[1]['img_processed'].shape), []).append(item)
        return results, shape_groups

    def _check_augment(self, augment):
        if augment and getattr(self, 'anchor_free', False):
            raise ValueError('augment=True (test-time augmentation) is implemented for YOLOv5 models only, not for {}'.format(
                'YOLOv9' if getattr(self, 'yolov9', False) else 'YOLO11'))

    def _nms_iou(self):
        return 0.45 if 'classic' in self.compatibility_mode else 0.6        # reference :1318-1321

    @staticmethod
    def _group_inputs(group_items):
        images, geoms = [], []
        for _, info, _ in group_items:
            ip = info['img_processed']
            if isinstance(ip, LetterboxSpec):
                io = info['img_original']
                images.append(io if isinstance(io, CoefficientImage) else np.ascontiguousarray(io))
                geoms.append(ip.geometry)
            else:                      # an already letterboxed HWC u8 array
                ip = np.ascontiguousarray(ip)
                images.append(ip)
                geoms.append((ip.shape[0], ip.shape[1], ip.shape[0], ip.shape[1], 0, 0))
        return images, geoms

    def _format_group(self, group_items, det_all, counts, h, w, results, detection_threshold):
        for i, (original_idx, info, current_id) in enumerate(group_items):
            det = det_all[i, :counts[i]]
            modern = 'classic' not in self.compatibility_mode
            detections, max_conf = format_detections(
                det, (h, w), info.get('resized_shape', info['img_original'].shape) if modern else info['img_original'].shape,
                info['scaling_shape'], detection_threshold,
                use_model_native_classes=self.use_model_native_classes, modern=modern,
                letterbox_pad=info.get('letterbox_pad'),
                round_pad=getattr(self, 'anchor_free', False) and not getattr(self, 'yolov9', False))
            results[original_idx] = {'file': current_id, 'detections': detections,
                                     'max_detection_conf': max_conf}

    def decode_scans(self, images):
        """
        Replaces every jpeg_host.ScanImage of `images`: one upload of the compressed scans and one mdhip_jpeg_entropy_decode
        for all of them on the compute stream, the statuses read back once.  A clean file becomes a DeviceCoefficientImage
        (its planes stay on the device and go through mdhip_jpeg_reconstruct like a CoefficientImage's).  A file the
        decoder flags is decoded here from the bytes the ScanImage holds, by load_image's own statements (mode handling,
        EXIF rotation): it becomes the RGB array PIL gives or, when PIL fails too, a ScanFailure carrying that error.
        Every other entry is returned as it is.
        """
        idx = [i for i, im in enumerate(images) if isinstance(im, ScanImage)]
        if not idx:
            return images
        if self._ctx is None:
            raise RuntimeError('this HIPDetector was created with preprocess_only')
        import io
        from .feed import load_image
        pl = self._pipeline()
        torch = pl.torch
        images = list(images)
        scan_offs, coef_offs, nbytes, nvals = [], [], 0, 0
        for i in idx:
            scan_offs.append(nbytes)
            nbytes += (images[i].nbytes + 255) // 256 * 256 + 256
            coef_offs.append(nvals)
            nvals += (images[i].coef_count + 127) // 128 * 128
        host = np.zeros(nbytes, dtype=np.uint8)
        for i, off in zip(idx, scan_offs):
            host[off:off + images[i].nbytes] = images[i].scan_bytes
        comp = pl.comp_s
        with torch.cuda.device(pl.dev), torch.cuda.stream(comp):
            scans = torch.from_numpy(host).to(pl.dev)
            coefs = torch.empty(max(nvals, 1), dtype=torch.int16, device=pl.dev)
            status = self._ctx.jpeg_entropy_decode([images[i] for i in idx], [scans.data_ptr() + o for o in scan_offs],
                                                   [coefs.data_ptr() + 2 * o for o in coef_offs], stream=comp.cuda_stream)
        for i, off, st in zip(idx, coef_offs, status):
            im = images[i]
            if st == 0:
                images[i] = im.coefficient_image(DeviceCoefficientImage.Planes(coefs, off, im.coef_count))
                self.jpeg_images_entropy_decoded += 1
                continue
            self.jpeg_entropy_fallbacks += 1
            try:
                images[i] = np.asarray(load_image(io.BytesIO(im.file.tobytes())))
            except Exception as e:
                images[i] = ScanFailure(e)
        return images

    def _fp8_calibrated(self):
        self._fp8_pending = False
        if self._fp8_scales_file:
            tmp = '{}.{}.tmp'.format(self._fp8_scales_file, os.getpid())
            with open(tmp, 'w') as f:
                json.dump({'fp8_scales': [float(sc) for sc, _, _ in self._ctx.fp8_scales()]}, f)
            os.replace(tmp, self._fp8_scales_file)

    # -----------------------------------------------------------------------------------
    def generate_detections_for_tiles(self, img_original, tile_origins, tile_size, tile_ids=None,
                                      detection_threshold=0.00001, image_size=None, augment=False, verbose=False,
                                      jpeg_quality=None):
        """
        Tiled inference on one large image (the device half of run_tiled_inference.py): the image is uploaded ONCE and
        every tile is cut out of it, letterboxed and normalised by the windowed letterbox kernels
        (mdhip_preprocess_windows) -- no tile is ever materialised on the host.

        img_original: PIL image or HWC uint8 array.  tile_origins: [(x, y)] upper-left corners.  tile_size: (w, h).
        tile_ids: the 'file' of each result (default '<x>_<y>', zero-padded to four digits).
        Returns one result dict per tile, the very dicts generate_detections_one_batch returns for the list of crops
        img[y:y + h, x:x + w]: a tile counts as an image of size (h, w).  Tiles are processed in chunks of max_batch; an
        exception in a chunk marks that chunk's tiles 'inference failure'.
        Every chunk takes one of the four NMS result slots in turn, like the groups of start_batch(): with two tickets
        outstanding a call of more than two chunks reaches a slot a ticket holds, and that chunk fails.

        jpeg_quality (1 .. 100, default None = off): every tile first goes through a JPEG round trip on the device
        (mdhip_jpeg_recompress) and the detector sees what it would read from the tile FILE the reference writes with
        PIL at that quality (95 there) -- the results are those of generate_detections_one_batch for the crops after
        Image.save(quality=jpeg_quality) / Image.open, bit for bit.  No file, no host copy.
        """
        if jpeg_quality is not None:
            jpeg_quality = check_quality(jpeg_quality)
        if detection_threshold is None:
            detection_threshold = 0.0
        if self._ctx is None:
            raise RuntimeError('this HIPDetector was created with preprocess_only')
        self._check_augment(augment)
        img = img_original if isinstance(img_original, np.ndarray) else np.asarray(img_original)
        if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError('expected an HxWx3 uint8 RGB image, got {} {}'.format(img.shape, img.dtype))
        img = np.ascontiguousarray(img)
        H, W = img.shape[:2]
        tw, th = int(tile_size[0]), int(tile_size[1])
        origins = [(int(x), int(y)) for x, y in tile_origins]
        for x, y in origins:
            if x < 0 or y < 0 or tw < 1 or th < 1 or x + tw > W or y + th > H:
                raise ValueError('tile ({}, {}) of size {}x{} does not lie inside the {}x{} image'.format(x, y, tw, th, W, H))
        if tile_ids is None:
            tile_ids = ['{}_{}'.format(str(x).zfill(4), str(y).zfill(4)) for x, y in origins]
        if len(tile_ids) != len(origins):
            raise ValueError('Length mismatch: {} tile origins, {} tile ids'.format(len(origins), len(tile_ids)))
        if len(origins) == 0:
            return []
        # geometry of a tile = geometry of an image of the tile's size (the views share the parent's pixels: nothing is copied)
        views = [img[y:y + th, x:x + tw] for x, y in origins]
        results, shape_groups = self._prepare_batch(views, list(tile_ids), image_size, verbose)
        if not shape_groups:
            return results
        torch, dev = self._pipeline().torch, self._pipeline().dev
        pitch, total = W * 3, H * W * 3
        with torch.cuda.device(dev):
            parent = torch.empty(total, dtype=torch.uint8, device=dev)      # exactly the image: `readable` is exact
            parent.copy_(torch.from_numpy(img.reshape(-1)))
            torch.cuda.synchronize(dev)
            base = parent.data_ptr()
            try:
                for shape, items in shape_groups.items():                   # (one group: all tiles have one size)
                    for start in range(0, len(items), self.max_batch):
                        chunk = items[start:start + self.max_batch]
                        try:
                            if jpeg_quality is None:
                                self._process_tile_chunk(chunk, origins, base, pitch, total, results, detection_threshold, augment)
                            else:
                                self._process_tile_chunk(*self._recompress_tile_chunk(chunk, origins, base, pitch, (tw, th), jpeg_quality),
                                                         results, detection_threshold, augment)
                        except Exception as e:
                            print('Warning: tile inference failed for shape {}: {}'.format(shape, str(e)))
                            for original_idx, _, current_id in chunk:
                                results[original_idx] = {'file': current_id, 'detections': None, 'failure': FAILURE_INFER}
            finally:
                torch.cuda.synchronize(dev)                                 # nothing reads `parent` once it is released
        return results

    def _recompress_tile_chunk(self, chunk, origins, base, pitch, tile_size, quality):
        """
        The chunk's windows of the device image at `base`, after a JPEG round trip at `quality`, as tile-sized device images
        in a buffer this detector owns.  Returns the (chunk, origins, base, pitch, total) that make _process_tile_chunk
        read them: each a window that covers a whole image, one behind the other like the rows of a tw-wide strip.
        """
        pl = self._pipeline()
        tw, th = tile_size
        n = len(chunk)
        tile_bytes = th * tw * 3
        buf = getattr(self, '_tile_jpeg_buf', None)
        if buf is None or buf.numel() < n * tile_bytes:
            pl.torch.cuda.synchronize()                                     # (earlier kernels may still read the old buffer)
            self._tile_jpeg_buf = buf = pl.torch.empty(n * tile_bytes, dtype=pl.torch.uint8, device=pl.dev)
        out = buf.data_ptr()
        # on the compute stream: behind the letterbox that read `out` last and in front of the one that reads it next
        self._ctx.jpeg_recompress([base + origins[idx][1] * pitch + origins[idx][0] * 3 for idx, _, _ in chunk], [(tw, th)] * n,
                                  [pitch] * n, quality, [out + i * tile_bytes for i in range(n)], stream=pl.comp_s.cuda_stream)
        strip = {idx: (0, i * th) for i, (idx, _, _) in enumerate(chunk)}
        return chunk, strip, out, tw * 3, n * tile_bytes

    def _process_tile_chunk(self, chunk, origins, base, pitch, total, results, detection_threshold, augment):
        """the chunk's windows of the device image at `base` (row pitch `pitch`, `total` bytes): letterboxed in place on the
        compute stream, run like a dense group (_run_group) and collected at once -- tile chunks do not overlap"""
        h, w = chunk[0][1]['img_processed'].shape[:2]
        n = len(chunk)
        offs = [origins[idx][1] * pitch + origins[idx][0] * 3 for idx, _, _ in chunk]
        self._ctx.preprocess_windows([base + o for o in offs], [info['img_processed'].geometry for _, info, _ in chunk],
                                     [pitch] * n, [total - o for o in offs], h, w, stream=self._pipeline().comp_s.cuda_stream)
        self._collect_group(self._run_group(chunk, detection_threshold, augment), results, detection_threshold)

    # -----------------------------------------------------------------------------------
    # The one device path.  The device work of a group (the images of one letterboxed shape, at most max_batch of them, or a
    # chunk of tiles) is enqueued on private streams (_submit_group, _run_group) and collected later (_collect_group):
    # start_batch() returns with its last group in flight and finish_batch() waits for it and formats, so a caller that keeps
    # two tickets outstanding (the batch driver, feed.py) overlaps the copy of batch i+1 with the kernels of batch i;
    # generate_detections_one_batch is start_batch + finish_batch, one group in flight at a time.  Host images are copied
    # to the device on a copy stream into one of two staging buffers (asynchronously when they live in page-locked memory,
    # e.g. feed.SharedImageRing).  _Pipeline and _StagingSlot (below the class) hold the streams and the buffers' rules.
    # -----------------------------------------------------------------------------------
    def _pipeline(self):
        if getattr(self, '_pl', None) is None:
            self._pl = _Pipeline(self.device)
        return self._pl

    def _submit_group(self, group_items, detection_threshold, augment=False, products=()):
        """a dense group: its host images into a staging buffer, coefficient images rebuilt behind them, the letterbox, then
        _run_group; returns the handle for _collect_group"""
        pl = self._pipeline()
        torch = pl.torch
        h, w = group_items[0][1]['img_processed'].shape[:2]
        images, geoms = self._group_inputs(group_items)
        slot = pl.slots[pl.staged % 2]
        pl.staged += 1
        offs, total = [], 0
        for im in images:
            offs.append(total)
            total += (im.nbytes + 255) // 256 * 256
        # coefficient images: their pixels are rebuilt on the device, behind the copies, into the same staging buffer
        jpeg_idx = [i for i, im in enumerate(images) if isinstance(im, CoefficientImage)]
        rgb_offs = {}
        for i in jpeg_idx:
            rgb_offs[i] = total
            total += (int(np.prod(images[i].shape)) + 255) // 256 * 256
        with torch.cuda.device(pl.dev):
            stage = slot.take(total, pl.copy_s)
            with torch.cuda.stream(pl.copy_s):
                for im, off in zip(images, offs):
                    if isinstance(im, DeviceCoefficientImage):
                        continue                          # its planes are on the device already (decode_scans)
                    flat = im.coef.view(np.uint8) if isinstance(im, CoefficientImage) else im.reshape(-1)
                    if not flat.flags.writeable:          # torch warns on read-only arrays; the copy only reads
                        flat = flat.view()
                        try:
                            flat.flags.writeable = True
                        except ValueError:
                            flat = np.array(flat)
                    stage[off:off + im.nbytes].copy_(torch.from_numpy(flat), non_blocking=True)
                slot.copied.record(pl.copy_s)
            comp = pl.comp_s
            base = stage.data_ptr()
            comp.wait_event(slot.copied)
            srcs = [base + off for off in offs]
            if jpeg_idx:
                self._ctx.jpeg_reconstruct([images[i] for i in jpeg_idx],
                                           [images[i].coef.data_ptr() if isinstance(images[i], DeviceCoefficientImage) else base + offs[i]
                                            for i in jpeg_idx],
                                           [base + rgb_offs[i] for i in jpeg_idx], stream=comp.cuda_stream)
                for i in jpeg_idx:
                    srcs[i] = base + rgb_offs[i]
                self.jpeg_images_reconstructed += len(jpeg_idx)
            # (the letterbox on the copy stream next to the previous batch's forward -- mdhip_preprocess waits for that
            # forward's stem inside the library -- was measured with bench.py --pre-own-stream: 0.6 % slower, its workgroups
            # keep the 8-wave conv workgroups off their CUs; it stays on the compute stream)
            self._ctx.preprocess(srcs, geoms, h, w, stream=comp.cuda_stream)
            slot.consumed = consumed = torch.cuda.Event()
            consumed.record(comp)
            handle = self._run_group(group_items, detection_threshold, augment)
        handle['copied'], handle['images'] = slot.copied, images      # (the host arrays live until the ticket is done)
        if products:
            # the pixels stay in the staging buffer until the products are made (_collect_group): views of it, per image
            handle['products'], handle['staged'], handle['consumed'] = products, slot, consumed
            slot.owed = handle
            handle['tensors'] = [stage[rgb_offs[i]:rgb_offs[i] + int(np.prod(im.shape))] if i in rgb_offs
                                 else stage[offs[i]:offs[i] + im.nbytes] for i, im in enumerate(images)]
        return handle

    def _run_group(self, group_items, detection_threshold, augment):
        """What follows the letterbox, for a dense group and for a chunk of tiles alike: calibration if it is due, the forward on
        the compute stream, the NMS on its own stream into the next of the four result slots.  Returns the handle
        _collect_group takes."""
        pl = self._pipeline()
        torch, ctx, comp = pl.torch, self._ctx, pl.comp_s
        h, w = group_items[0][1]['img_processed'].shape[:2]
        n = len(group_items)
        nms_slot = pl.count % 4
        if pl.uncollected[nms_slot]:
            raise RuntimeError('NMS result slot {} holds a group that has not been collected: finish the outstanding tickets '
                               'before enqueueing more groups'.format(nms_slot))
        pl.count += 1
        with torch.cuda.device(pl.dev):
            if self._fp8_pending:               # fp8 mode, explicit opt-in: this batch calibrates the scales
                ctx.calibrate(n, h, w, stream=comp.cuda_stream)
                self._fp8_calibrated()
            # NMS + D2H on their own stream, next to the following batch's letterbox and first layers (the library
            # alternates between two prediction buffers; the forward that reuses a buffer waits for the NMS that read it).
            # History: own stream in round 1; in line behind the forward in rounds 2-3 (the 1024-thread NMS workgroups kept
            # the persistent conv workgroups off their CUs: 37.6 vs 37.2 ms / step); since round 4 the NMS sorts only the
            # confidence band it needs and is gone before the next forward reaches its 8-wave kernels: own stream again
            # (+0.4 .. 0.7 % at batch 32, profiles/r4_bench_nms_stream.txt).
            prev = pl.nms_done[(nms_slot - 2) % 4]                   # the group two before this one
            if prev is not None:
                comp.wait_event(prev)
            if augment:
                ctx.forward_tta(n, h, w, stream=comp.cuda_stream)    # yolov5 _forward_augment: 3 passes, concatenated predictions
            else:
                ctx.forward(n, h, w, stream=comp.cuda_stream)
            fwd_done = torch.cuda.Event()
            fwd_done.record(comp)
            pl.nms_s.wait_event(fwd_done)
            ctx.nms_enqueue(n, detection_threshold, self._nms_iou(), 300, slot=nms_slot, stream=pl.nms_s.cuda_stream)
            done = torch.cuda.Event()
            done.record(pl.nms_s)
            pl.nms_done[nms_slot], pl.uncollected[nms_slot] = done, True
        return {'items': group_items, 'h': h, 'w': w, 'slot': nms_slot}

    def _collect_group(self, handle, results, detection_threshold):
        """waits for a group's NMS, formats its results and makes the products it owes"""
        try:
            det_all, counts = self._ctx.nms_wait(slot=handle['slot'])
        finally:
            self._pipeline().uncollected[handle['slot']] = False
        self._format_group(handle['items'], det_all, counts, handle['h'], handle['w'], results, detection_threshold)
        if handle.get('tensors') is not None:
            pl = self._pipeline()
            with pl.torch.cuda.device(pl.dev):
                product_s = pl.product_stream()
                product_s.wait_event(handle['consumed'])      # copies, reconstruction and letterbox of this batch are done
                try:
                    self._add_products(handle['items'], handle['tensors'], results, handle['products'], stream=product_s.cuda_stream)
                finally:
                    handle['staged'].products_made(handle, product_s)

    def start_batch(self, img_original, image_id, detection_threshold=0.00001, image_size=None, augment=False,
                    verbose=False, crops=None, blur=None, preview=None, classify=None, render=None):
        """Enqueues a batch; returns a ticket for finish_batch(), and every ticket must be finished.  At most two tickets may
        be outstanding, and at most four groups can be in flight: every shape group of at most max_batch images takes one of
        the four NMS result slots until it is collected, and so does every chunk of the other calls.  All groups of a batch
        but the last are collected here.  The slots are taken in turn: a group whose slot is still held by an
        uncollected group fails ('inference failure').
        Same arguments as generate_detections_one_batch (augment = yolov5's three-pass augmented inference)."""
        if self._ctx is None:
            raise RuntimeError('this HIPDetector was created with preprocess_only')
        self._check_augment(augment)
        if detection_threshold is None:
            detection_threshold = 0.0
        products = self._products(crops, blur, preview, classify, render)
        img_original = self.decode_scans(img_original)
        results, shape_groups = self._prepare_batch(img_original, image_id, image_size, verbose)
        chunks = []
        for shape, items in shape_groups.items():
            for start in range(0, len(items), self.max_batch):
                chunks.append(items[start:start + self.max_batch])
        pending = None
        for ci, chunk in enumerate(chunks):
            try:
                handle = self._submit_group(chunk, detection_threshold, augment, products)
                if ci == len(chunks) - 1:
                    pending = handle                     # the last group stays in flight
                else:
                    self._collect_group(handle, results, detection_threshold)
            except Exception as e:
                print('Warning: batch inference failed for shape {}: {}'.format(chunk[0][1]['img_processed'].shape, str(e)))
                for original_idx, _, current_id in chunk:
                    results[original_idx] = {'file': current_id, 'detections': None, 'failure': FAILURE_INFER}
        return {'results': results, 'pending': pending, 'threshold': detection_threshold, 'products': products}

    def batch_inputs_consumed(self, ticket):
        """Blocks until the host images of the ticket's in-flight group have been copied to the device
        (their buffers -- e.g. shared-ring slots -- may then be reused)."""
        if ticket['pending'] is not None:
            ticket['pending']['copied'].synchronize()

    def finish_batch(self, ticket):
        results = ticket['results']
        handle = ticket['pending']
        if handle is not None:
            try:
                self._collect_group(handle, results, ticket['threshold'])
            except Exception as e:
                print('Warning: batch inference failed: {}'.format(str(e)))
                for original_idx, _, current_id in handle['items']:
                    results[original_idx] = {'file': current_id, 'detections': None, 'failure': FAILURE_INFER}
            ticket['pending'] = None
        return self._products_everywhere(results, ticket['products'])

    # -----------------------------------------------------------------------------------
    def generate_detections_one_image(self, img_original, image_id='unknown', detection_threshold=0.00001,
                                      image_size=None, augment=False, verbose=False, crops=None, blur=None, preview=None,
                                      classify=None, render=None):
        """reference pytorch_detector.py:1428-1478"""
        if isinstance(img_original, dict):
            res = self.generate_detections_one_batch([img_original], None, detection_threshold,
                                                     image_size, augment, verbose, crops=crops, blur=blur, preview=preview, classify=classify, render=render)
        else:
            res = self.generate_detections_one_batch([img_original], [image_id], detection_threshold,
                                                     image_size, augment, verbose, crops=crops, blur=blur, preview=preview, classify=classify, render=render)
        return res[0]


class _StagingSlot:
    """
    One of the pipeline's two staging buffers: a group's host images are copied into `tensor` on the copy stream (`copied`
    stands behind the copies), coefficient images are rebuilt behind them, and the letterbox reads it (`consumed` stands
    behind the last kernel that read the buffer).  `owed` is the group whose products are not made yet.
    """

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        self.tensor = None
        self.copied = torch.cuda.Event()
        self.consumed = None
        self.owed = None

    def take(self, total, copy_s):
        """the buffer with room for `total` bytes, for the next group, whose copies go onto the stream `copy_s`"""
        if self.owed is not None:
            # a group whose products are not made yet (a ticket that is still outstanding) keeps its pixels in this
            # buffer, and `consumed` stands behind its letterbox only: that group keeps the storage (its views hold
            # it) and this one gets a tensor of its own
            self.tensor = None
            self.owed = None
        if self.tensor is None or self.tensor.numel() < total:
            if self.consumed is not None:
                self.consumed.synchronize()
            self.tensor = self.torch.empty(max(total, 1), dtype=self.torch.uint8, device=self.dev)
        if self.consumed is not None:
            copy_s.wait_event(self.consumed)        # the letterbox kernel that read this buffer is done
        return self.tensor

    def products_made(self, handle, product_s):
        """While `handle`'s group owned the buffer no other group could take it (take() gives a later one a tensor of its
        own).  From here on the buffer may be reused: its `consumed` event moves behind the products' kernels, so the copy
        stream overwrites it only behind this group's last encode."""
        if self.owed is handle:
            self.owed = None
            if self.consumed is handle['consumed']:
                self.consumed = self.torch.cuda.Event()
                self.consumed.record(product_s)


class _Pipeline:
    """The streams, the two staging buffers and the four NMS result slots of a HIPDetector, made on first use.  `count` numbers
    the groups enqueued, dense groups and tile chunks alike: nms_done[count % 4] is the event behind a group's NMS and
    uncollected[count % 4] says that its results have not been fetched, so the slot must not be written.  `staged` numbers
    the dense groups alone, which alternate between the two staging buffers."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.dev = torch.device('cuda', _device_ordinal(device))
        with torch.cuda.device(self.dev):
            self.copy_s, self.comp_s, self.nms_s = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
            self.slots = [_StagingSlot(torch, self.dev), _StagingSlot(torch, self.dev)]
        self.product_s = None               # made when the first product is asked for
        self.count = self.staged = 0
        self.uncollected = [False] * 4
        self.nms_done = [None] * 4

    def product_stream(self):
        if self.product_s is None:
            with self.torch.cuda.device(self.dev):
                self.product_s = self.torch.cuda.Stream()
        return self.product_s
