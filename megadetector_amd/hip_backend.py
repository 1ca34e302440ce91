"""
Thin Python owner of one mdhip context (one GPU): turns YoloWeights into the C model
description, and exposes the hot-path stages with numpy in / numpy out.
All arithmetic happens in libmdhip.so (hand-written HIP); nothing here computes.
"""

import ctypes as C
import json
import os
from contextlib import contextmanager

import numpy as np

from . import _lib
from ._lib import HipError
from .jpeg_host import quant_tables
from .yolo_model import DETECT_TYPES, MDHIP_CBFUSE, MDHIP_DETECT_DDFL, detect_inputs


_DTYPES = {'bf16': _lib.MDHIP_DTYPE_BF16, 'fp8': _lib.MDHIP_DTYPE_FP8, 'fp16': _lib.MDHIP_DTYPE_FP16}


def model_description(weights):
    """YoloWeights -> (mdhip_model, the objects its pointers lead into: keep them for as long as the description is used)"""
    keep = []
    specs = weights.specs
    convs = []
    layers = (_lib.mdhip_layer * len(specs))()
    for i, s in enumerate(specs):
        L = layers[i]
        L.type = s.type
        frm = detect_inputs(s)                  # (DualDDetect: the inputs of the head that runs)
        L.n_from = len(frm)
        for j, f in enumerate(frm):
            L.from_[j] = f
        L.c_out = s.c_out if s.c_out is not None else 0
        L.k, L.s, L.p = s.k or 0, s.s or 1, s.p or 0
        if s.type == MDHIP_CBFUSE:              # channel offsets of the chosen splits (0 is an offset, not a default)
            L.k, L.s, L.p = s.k, s.s, s.p
        L.n = s.n or 1
        L.shortcut = s.shortcut or 0
        L.first_conv = len(convs)
        for name in s.conv_names:
            w = weights.weights[name + '.weight']
            b = weights.weights[name + '.bias']
            keep += [w, b]
            cv = _lib.mdhip_conv()
            cv.weight = w.ctypes.data_as(C.POINTER(C.c_float))
            cv.bias = b.ctypes.data_as(C.POINTER(C.c_float))
            cv.c_out, cv.c_in, cv.kh, cv.kw = w.shape
            convs.append(cv)
    conv_arr = (_lib.mdhip_conv * max(1, len(convs)))(*convs)
    m = _lib.mdhip_model()
    m.n_layers = len(specs)
    m.layers = layers
    m.n_convs = len(convs)
    m.convs = conv_arr
    m.nc = weights.nc
    m.na = weights.na
    m.nl = weights.nl
    anchors = np.ascontiguousarray(weights.anchors_px.reshape(-1), dtype=np.float32)
    strides = np.ascontiguousarray(np.asarray(weights.strides, dtype=np.float32))
    keep += [anchors, strides, layers, conv_arr]
    m.anchors_px = anchors.ctypes.data_as(C.POINTER(C.c_float)) if anchors.size else None
    m.strides = strides.ctypes.data_as(C.POINTER(C.c_float)) if strides.size else None
    return m, keep


def tuned_array(lib, entries):
    """table entries (the dicts of tuned_cfgs*.json) -> (mdhip_tuned array, count) as mdhip_set_tuned takes them"""
    ncfg = lib.mdhip_num_conv_cfgs()
    # an entry names its configuration; the id is looked up in THIS build (ids shift when a kernel family is
    # added or removed), entries without a name keep their id, entries naming an unknown configuration are dropped
    by_name = {lib.mdhip_conv_cfg_name(i).decode(): i for i in range(ncfg)}
    resolved = []
    for e in entries:
        if e.get('name'):
            if e['name'] not in by_name:
                continue
            e = dict(e, cfg=by_name[e['name']])
        if 0 <= int(e['cfg']) < ncfg:
            resolved.append(e)
    arr = (_lib.mdhip_tuned * max(1, len(resolved)))()
    for i, e in enumerate(resolved):
        arr[i].m, arr[i].n, arr[i].k = int(e['m']), int(e['n']), int(e['k'])
        arr[i].ntaps, arr[i].stride = int(e['ntaps']), int(e['stride'])
        arr[i].has_res, arr[i].cfg = int(e['has_res']), int(e['cfg'])
        arr[i].batch = int(e.get('batch', 32))
    return arr, len(resolved)


def _described(call, what):
    """the text of one of the describe calls: asked for its length first, then written"""
    lib = _lib.load()
    need = call(None, 0)
    if need >= 0:
        buf = C.create_string_buffer(need + 1)
        need = call(buf, need + 1)
    if need < 0:
        err = HipError('{} failed ({}): {}'.format(what, need, lib.mdhip_last_error(None).decode()))
        err.code = int(need)
        raise err
    return buf.value.decode()


def describe_plan(weights, dtype='bf16', max_batch=32, max_h=1280, max_w=1280):
    """
    What mdhip_create would plan for these weights, as text (mdhip_plan_describe): the ops, every tensor's place in the
    arena, the packed convs with a hash of their bytes.  Needs no GPU.  HipError (with .code) for a model the planner refuses.
    """
    lib = _lib.load()
    m, keep = model_description(weights)
    args = (C.byref(m), _DTYPES[dtype], int(max_batch), int(max_h), int(max_w))
    return _described(lambda buf, cap: lib.mdhip_plan_describe(*args, buf, cap), 'mdhip_plan_describe')


def describe_launches(weights, dtype, capacity, tuned_entries, n, h, w, fuse=True, fuse_decode=True, pair=True, isolated=False,
                      calibrating=False, augmented=False, forced=None, after_others=False, pw_stream=True):
    """
    What a forward of n images of h x w launches on a context of these weights, storage type and capacity (max_batch, max_h,
    max_w) with this tile table (the entries of tuned_cfgs*.json; None = none) and these settings, as text
    (mdhip_launches_describe): one line per op.  `forced`: {op index: configuration id or name}.  Needs no GPU.
    """
    lib = _lib.load()
    m, keep = model_description(weights)
    arr, n_tuned = tuned_array(lib, tuned_entries or [])
    flags = ((not fuse) * _lib.MDHIP_LAUNCHES_NO_FUSE | (not fuse_decode) * _lib.MDHIP_LAUNCHES_NO_FUSE_DECODE |
             (not pair) * _lib.MDHIP_LAUNCHES_NO_PAIR | bool(isolated) * _lib.MDHIP_LAUNCHES_ISOLATED |
             bool(calibrating) * _lib.MDHIP_LAUNCHES_CALIBRATING | bool(augmented) * _lib.MDHIP_LAUNCHES_AUGMENTED |
             bool(after_others) * _lib.MDHIP_LAUNCHES_AFTER_OTHERS | (not pw_stream) * _lib.MDHIP_LAUNCHES_NO_PW_STREAM)
    by_name = {lib.mdhip_conv_cfg_name(i).decode(): i for i in range(lib.mdhip_num_conv_cfgs())}
    pairs = [v for op, cfg in sorted((forced or {}).items()) for v in (int(op), by_name[cfg] if isinstance(cfg, str) else int(cfg))]
    farr = (C.c_int32 * max(1, len(pairs)))(*pairs)
    args = (C.byref(m), _DTYPES[dtype], *[int(v) for v in capacity], arr, n_tuned, int(n), int(h), int(w), flags, farr, len(pairs) // 2)
    return _described(lambda buf, cap: lib.mdhip_launches_describe(*args, buf, cap), 'mdhip_launches_describe')


def table_entries(dtype='bf16'):
    """the entries of the shipped tile table a context of this storage type loads (HipContext.load_tuned)"""
    path = HipContext.TUNED_PATH
    alt = path.replace('.json', '_{}.json'.format(dtype))
    if dtype != 'bf16' and os.path.exists(alt):
        path = alt
    return json.load(open(path)).get('entries', [])


def _window_arrays(ptrs, sizes, pitches):
    """per image or window its device address, (width, height) and bytes a row -> the pointer, width, height and pitch arrays
    the image entry points take"""
    n = len(ptrs)
    return (C.cast((C.c_void_p * n)(*[int(v) for v in ptrs]), C.POINTER(C.c_void_p)), (C.c_int32 * n)(*[int(v[0]) for v in sizes]),
            (C.c_int32 * n)(*[int(v[1]) for v in sizes]), (C.c_int64 * n)(*[int(v) for v in pitches]))


def _quant_array(quants, n):
    """per window (luma, chroma), 64 entries each -> the uint16 [n][2][64] array the sampled encoders take"""
    packed = np.zeros((max(n, 1), 2, 64), dtype=np.uint16)
    for i, pair in enumerate(quants):
        for k in (0, 1):
            table = np.asarray(pair[k]).reshape(-1)
            if table.size != 64 or table.min() < 0 or table.max() > 65535:
                raise ValueError('window {}: a quantisation table has 64 entries'.format(i))
            packed[i, k] = table
    return packed


def _letterbox_array(geoms):
    """[(src_h, src_w, resized_h, resized_w, top, left[, interp])] -> mdhip_letterbox array"""
    g = (_lib.mdhip_letterbox * len(geoms))()
    for i, q in enumerate(geoms):
        g[i].src_h, g[i].src_w, g[i].resized_h, g[i].resized_w, g[i].top, g[i].left = [int(v) for v in q[:6]]
        g[i].interp = int(q[6]) if len(q) > 6 else 0
    return g


class HipContext:

    def __init__(self, weights, device=0, dtype='bf16', max_batch=32, max_h=1280, max_w=1280):
        self.lib = _lib.load()
        self.weights = weights
        self.device = int(device)
        self.max_batch = int(max_batch)
        m, self._keep = model_description(weights)
        dt = _DTYPES[dtype]
        self.dtype = dtype
        handle = C.c_void_p()
        rc = self.lib.mdhip_create(C.byref(m), self.device, dt, int(max_batch), int(max_h), int(max_w),
                                   C.byref(handle))
        if rc != 0:
            raise HipError('mdhip_create failed ({}): {}'.format(
                rc, self.lib.mdhip_last_error(None).decode()))
        self.h = handle
        self.anchor_free = bool(getattr(weights, 'anchor_free', False))
        self.no = weights.nc + (4 if self.anchor_free else 5)      # anchor-free rows: [cx, cy, w, h, cls...]
        self.has_detect = weights.specs[-1].type in DETECT_TYPES
        self.max_stride = self.lib.mdhip_max_stride(self.h)
        self.load_tuned()

    @classmethod
    def for_images(cls, device=0):
        """
        A context without a model (include/mdhip.h: mdhip_create_images): the image calls work on it -- jpeg_*, blur_regions,
        resample_lanczos, draw_ops, classifier_input, thumbnails, change_detect, gray_count -- and every call that needs the plan or the weights
        (preprocess, forward, nms, read_*, ...) raises HipError (MDHIP_EINVAL).
        """
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self.weights = None
        self.device = int(device)
        self.max_batch = 0
        self._keep = None
        self.dtype = None
        handle = C.c_void_p()
        rc = self.lib.mdhip_create_images(self.device, C.byref(handle))
        if rc != 0:
            raise HipError('mdhip_create_images failed ({}): {}'.format(rc, self.lib.mdhip_last_error(None).decode()))
        self.h = handle
        self.anchor_free = False
        self.no = 0
        self.has_detect = False
        self.max_stride = 0
        return self

    @classmethod
    @contextmanager
    def images_or(cls, ctx, device=0):
        """`with HipContext.images_or(ctx, device) as ctx:` -- the caller's context, left open, or for None a for_images(device)
        made for the block and closed after it"""
        own = cls.for_images(device) if ctx is None else None
        try:
            yield ctx if own is None else own
        finally:
            if own is not None:
                own.close()

    TUNED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tuned_cfgs.json')

    def load_tuned(self, path=None):
        """
        Hands the measured tile choices (tools/autotune.py) to the library; returns the number of
        entries.  Shapes without an entry use the built-in heuristic, so a missing or stale file only
        costs speed.
        """
        if path is None and getattr(self, 'anchor_free', False):
            # the tables hold YOLOv5 layers; the YOLO11 layers take the built-in heuristic (an entry matched by geometry
            # from another model would pick a kernel family for them that nobody measured)
            return 0
        if path is None:
            # a table measured for this storage type, if there is one (tuned_cfgs_fp16.json), else the bf16 table
            path = self.TUNED_PATH
            alt = self.TUNED_PATH.replace('.json', '_{}.json'.format(getattr(self, 'dtype', 'bf16')))
            if getattr(self, 'dtype', 'bf16') != 'bf16' and os.path.exists(alt):
                path = alt
        if not os.path.exists(path):
            return 0
        try:
            entries = json.load(open(path)).get('entries', [])
        except Exception:
            return 0
        arr, n = tuned_array(self.lib, entries)
        self._check(self.lib.mdhip_set_tuned(self.h, arr, n), 'mdhip_set_tuned')
        return n

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise HipError('{} failed ({}): {}'.format(what, rc, self.lib.mdhip_last_error(self.h).decode()))

    def close(self):
        if getattr(self, 'h', None) is not None and self.h.value:
            self.lib.mdhip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- hot path ---------------------------------------------------------------------
    def preprocess(self, images, geoms, out_h, out_w, stream=0):
        """
        images: list of HWC uint8 RGB numpy arrays (host) or integer device pointers.
        geoms:  list of (src_h, src_w, resized_h, resized_w, top, left[, interp]); interp 0 = cv2.INTER_LINEAR
                (default), 1 = cv2.INTER_AREA.
        """
        n = len(images)
        ptrs = (C.c_void_p * n)()
        hold = []
        for i, im in enumerate(images):
            if isinstance(im, np.ndarray):
                if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                    raise ValueError('image {} must be HWC uint8 RGB'.format(i))
                im = np.ascontiguousarray(im)
                hold.append(im)
                ptrs[i] = im.ctypes.data
            else:
                ptrs[i] = int(im)
        self._check(self.lib.mdhip_preprocess(self.h, C.cast(ptrs, C.POINTER(C.c_void_p)), _letterbox_array(geoms), n,
                                              int(out_h), int(out_w), C.c_void_p(stream)), 'mdhip_preprocess')

    def preprocess_windows(self, ptrs, geoms, pitches, readable, out_h, out_w, stream=0):
        """
        preprocess() for windows of larger device images (tiles): nothing is copied, the kernels read the parent in place.
        ptrs:     integer device pointers to each window's first pixel
        geoms:    as for preprocess(); src_h / src_w are the window's size
        pitches:  bytes between two rows of each window's parent image
        readable: bytes readable from each pointer to the end of its parent allocation
        """
        n = len(ptrs)
        if not (len(geoms) == len(pitches) == len(readable) == n):
            raise ValueError('ptrs, geoms, pitches and readable must have one entry per window')
        p = (C.c_void_p * n)(*[int(v) for v in ptrs])
        pt = (C.c_int64 * n)(*[int(v) for v in pitches])
        rd = (C.c_int64 * n)(*[int(v) for v in readable])
        self._check(self.lib.mdhip_preprocess_windows(self.h, C.cast(p, C.POINTER(C.c_void_p)), _letterbox_array(geoms), pt, rd, n,
                                                      int(out_h), int(out_w), C.c_void_p(stream)), 'mdhip_preprocess_windows')

    def jpeg_reconstruct(self, images, coef_ptrs, out_ptrs, stream=0):
        """
        Rebuilds RGB images from quantised JPEG coefficients on the device (include/mdhip.h: mdhip_jpeg_reconstruct).
        images:    jpeg_host.CoefficientImage objects (geometry, sampling, tables, rotation)
        coef_ptrs: integer device pointers to each image's coefficient planes (16-byte aligned)
        out_ptrs:  integer device pointers to room for each rotated H x W x 3 image (image.shape)
        """
        n = len(images)
        if not (len(coef_ptrs) == len(out_ptrs) == n):
            raise ValueError('images, coef_ptrs and out_ptrs must have one entry per image')
        arr = (_lib.mdhip_jpeg_image * n)()
        for i, im in enumerate(images):
            a = arr[i]
            a.coef = int(coef_ptrs[i])
            a.width, a.height, a.components = im.width, im.height, im.components
            a.h_samp, a.v_samp, a.rotation = im.h_samp, im.v_samp, im.rotation
            for c in range(im.components):
                a.blocks_w[c], a.blocks_h[c] = im.blocks_w[c], im.blocks_h[c]
            q = np.ascontiguousarray(im.quant, dtype=np.uint16).reshape(3, 64)
            C.memmove(C.addressof(a.quant), q.ctypes.data, 384)
        outs = (C.c_void_p * n)(*[int(v) for v in out_ptrs])
        self._check(self.lib.mdhip_jpeg_reconstruct(self.h, arr, n, C.cast(outs, C.POINTER(C.c_void_p)), C.c_void_p(stream)),
                    'mdhip_jpeg_reconstruct')

    def jpeg_entropy_decode(self, images, scan_ptrs, coef_ptrs, subseq_bits=0, stream=0):
        """
        Huffman-decodes the scans of baseline JPEGs on the device (include/mdhip.h: mdhip_jpeg_entropy_decode).
        images:    jpeg_host.ScanImage objects (descriptor and segment offsets of mdjpeg_scan)
        scan_ptrs: integer device pointers to each file's entropy-coded bytes [scan_begin, scan_end)
        coef_ptrs: integer device pointers to room for each image's coefficient planes (16-byte aligned, coef_count int16)
        Returns the status words (int32 array): 0, or a mask of MDHIP_JPEG_* bits for a file the decoder refuses.
        """
        n = len(images)
        if not (len(scan_ptrs) == len(coef_ptrs) == n):
            raise ValueError('images, scan_ptrs and coef_ptrs must have one entry per image')
        arr = (_lib.mdhip_jpeg_scan * max(n, 1))()
        for i, im in enumerate(images):
            arr[i].scan, arr[i].coef = int(scan_ptrs[i]), int(coef_ptrs[i])
            arr[i].desc = C.addressof(im.desc)
            arr[i].seg_offsets = im.seg_offsets.ctypes.data
        status = (C.c_int32 * max(n, 1))()
        self._check(self.lib.mdhip_jpeg_entropy_decode(self.h, arr, n, int(subseq_bits), status, C.c_void_p(stream)),
                    'mdhip_jpeg_entropy_decode')
        return np.array(status[:n], dtype=np.int32)

    def jpeg_entropy_stats(self):
        """of the last jpeg_entropy_decode: {'subsequences', 'decoded_again', 'sync_launches', 'images'}"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.mdhip_jpeg_entropy_stats(self.h, out), 'mdhip_jpeg_entropy_stats')
        return dict(zip(('subsequences', 'decoded_again', 'sync_launches', 'images'), [int(v) for v in out]))

    def jpeg_recompress(self, ptrs, sizes, pitches, quality, out_ptrs, stream=0):
        """
        Gives windows of device images the pixels of Image.save(quality=quality) + Image.open, bit for bit, on the device
        (include/mdhip.h: mdhip_jpeg_recompress).
        ptrs:     integer device pointers to each window's first pixel
        sizes:    (width, height) of each window
        pitches:  bytes between two rows of each window's parent image
        quality:  Pillow's `quality`, 1 .. 100 (jpeg_host.quant_tables)
        out_ptrs: integer device pointers to room for each height x width x 3 result
        """
        n = len(ptrs)
        if not (len(sizes) == len(pitches) == len(out_ptrs) == n):
            raise ValueError('ptrs, sizes, pitches and out_ptrs must have one entry per window')
        ql, qc = quant_tables(quality)
        p, ws, hs, pt = _window_arrays(ptrs, sizes, pitches)
        o = (C.c_void_p * n)(*[int(v) for v in out_ptrs])
        self._check(self.lib.mdhip_jpeg_recompress(self.h, p, ws, hs, pt, n,
                                                   ql.ctypes.data_as(C.POINTER(C.c_uint16)), qc.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                   C.cast(o, C.POINTER(C.c_void_p)), C.c_void_p(stream)), 'mdhip_jpeg_recompress')

    def jpeg_encode(self, ptrs, sizes, pitches, quality, out_ptr, capacity, stream=0):
        """
        Entropy-coded JPEG scans of windows of device images, byte for byte those of Image.save(quality=quality)
        (include/mdhip.h: mdhip_jpeg_encode); jpeg_host.jfif_file puts the file around a scan.
        ptrs, sizes, pitches, quality: as for jpeg_recompress
        out_ptr, capacity: ONE device buffer for all scans, and its size in bytes
        Returns (fits, offsets, sizes, needed): int64 arrays of each window's scan within the buffer, and the capacity the
        call needs.  fits False (MDHIP_ECAPACITY): nothing was written beyond the capacity; call again with `needed` bytes.
        """
        n = len(ptrs)
        if not (len(sizes) == len(pitches) == n):
            raise ValueError('ptrs, sizes and pitches must have one entry per window')
        ql, qc = quant_tables(quality)
        return self._jpeg_encode('mdhip_jpeg_encode', _window_arrays(ptrs, sizes, pitches), n,
                                 (ql.ctypes.data_as(C.POINTER(C.c_uint16)), qc.ctypes.data_as(C.POINTER(C.c_uint16))), out_ptr, capacity, stream)

    def _jpeg_encode(self, name, windows, n, tables, out_ptr, capacity, stream, status=None):
        """
        What the three encode calls share.  name: the C function; windows: its arguments in front of `n` (the window arrays and,
        where it takes them, the samplings); tables: those between `n` and `out` (tables, sources, rectangles); status: the
        per-window array jpeg_encode_kept has behind `needed`.  MDHIP_ECAPACITY is a result (fits False), any other code raises.
        """
        offs, lens, need = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))(), C.c_int64(0)
        rc = getattr(self.lib, name)(self.h, *windows, n, *tables, C.c_void_p(int(out_ptr) if capacity else 0), int(capacity), offs, lens,
                                     C.byref(need), *(() if status is None else (status,)), C.c_void_p(stream))
        if rc != _lib.MDHIP_ECAPACITY:
            self._check(rc, name)
        return rc == 0, np.array(offs[:n], dtype=np.int64), np.array(lens[:n], dtype=np.int64), int(need.value)

    def jpeg_encode_sampled(self, ptrs, sizes, pitches, samplings, quants, out_ptr, capacity, stream=0):
        """
        jpeg_encode with each window's own chroma sampling and quantisation tables (include/mdhip.h:
        mdhip_jpeg_encode_sampled): byte for byte the scans of Image.save(qtables=[luma, chroma], subsampling=sampling);
        jpeg_host.sampled_file puts the file around a scan.
        samplings: per window 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), as Pillow's `subsampling`
        quants: per window (luma, chroma), 64 entries of 1 .. 255 each, natural order
        Everything else, and what is returned, as for jpeg_encode.
        """
        n = len(ptrs)
        if not (len(sizes) == len(pitches) == len(samplings) == len(quants) == n):
            raise ValueError('ptrs, sizes, pitches, samplings and quants must have one entry per window')
        windows = _window_arrays(ptrs, sizes, pitches) + ((C.c_int32 * max(n, 1))(*[int(v) for v in samplings]),)
        packed = _quant_array(quants, n)
        return self._jpeg_encode('mdhip_jpeg_encode_sampled', windows, n, (packed.ctypes.data_as(C.POINTER(C.c_uint16)),), out_ptr, capacity, stream)

    def jpeg_encode_kept(self, ptrs, sizes, pitches, samplings, quants, source_ptrs, rect_image, rects, out_ptr, capacity, stream=0):
        """
        jpeg_encode_sampled for copies in which only rectangles changed (include/mdhip.h: mdhip_jpeg_encode_kept): the blocks
        of every MCU that no rectangle touches are the source file's own coefficients.
        source_ptrs: per window the integer device pointer (16-byte aligned) to the source's quantised planes in the layout of
                     jpeg_host.decode / jpeg_entropy_decode for the window's size and sampling (whole MCUs)
        rect_image, rects: per changed rectangle the index of its window and (left, top, right, bottom), right / bottom
                     exclusive; clipped to the window by the call
        Everything else as for jpeg_encode_sampled.  Returns (fits, offsets, sizes, needed, status): status 1 marks a window
        whose merged blocks no baseline scan holds; its scan has size 0 and the caller re-encodes it whole.
        """
        n, m = len(ptrs), len(rects)
        if not (len(sizes) == len(pitches) == len(samplings) == len(quants) == len(source_ptrs) == n) or len(rect_image) != m:
            raise ValueError('one entry per window is needed in every list, and one window index per rectangle')
        windows = _window_arrays(ptrs, sizes, pitches) + ((C.c_int32 * max(n, 1))(*[int(v) for v in samplings]),)
        packed = _quant_array(quants, n)
        sources = (_lib.mdhip_jpeg_source * max(n, 1))()
        for i, ((w, h), sampling) in enumerate(zip(sizes, samplings)):
            fh, fv = {0: (1, 1), 1: (2, 1), 2: (2, 2)}.get(int(sampling), (1, 1))      # (the call refuses any other sampling)
            mx, my = (int(w) + 8 * fh - 1) // (8 * fh), (int(h) + 8 * fv - 1) // (8 * fv)
            sources[i].coef = int(source_ptrs[i])
            sources[i].blocks_w[:] = [mx * fh, mx, mx]
            sources[i].blocks_h[:] = [my * fv, my, my]
        ri = (C.c_int32 * max(m, 1))(*[int(v) for v in rect_image])
        rc4 = (C.c_int32 * max(4 * m, 1))(*[int(v) for q in rects for v in q])
        status = (C.c_int32 * max(n, 1))()
        result = self._jpeg_encode('mdhip_jpeg_encode_kept', windows, n, (packed.ctypes.data_as(C.POINTER(C.c_uint16)), sources, ri, rc4, m),
                                   out_ptr, capacity, stream, status)
        return result + (np.array(status[:n], dtype=np.int32),)

    @staticmethod
    def jpeg_encode_sampled_bound(width, height, sampling):
        """bytes the scan of a width x height window can take at the very most at that sampling (mdhip_jpeg_encode_sampled_bound)"""
        return int(_lib.load().mdhip_jpeg_encode_sampled_bound(int(width), int(height), int(sampling)))

    @staticmethod
    def jpeg_encode_bound(width, height):
        """bytes the scan of a width x height window can take at the very most (mdhip_jpeg_encode_bound)"""
        return int(_lib.load().mdhip_jpeg_encode_bound(int(width), int(height)))

    def blur_regions(self, ptrs, sizes, pitches, rect_image, rects, radius=40, stream=0):
        """
        Pillow's ImageFilter.GaussianBlur(radius) of rectangles of device images, in place and bit for bit
        (include/mdhip.h: mdhip_blur_regions).
        ptrs, sizes, pitches: per image the device address of an RGB uint8 image, its (width, height) and its bytes a row
        rect_image, rects: per rectangle the index of its image and (left, top, right, bottom), right / bottom exclusive.
        The rectangles of one image are applied in list order; a rectangle without area is skipped.  Only enqueues.
        """
        n, m = len(ptrs), len(rects)
        if not (len(sizes) == len(pitches) == n) or len(rect_image) != m:
            raise ValueError('ptrs, sizes and pitches must have one entry per image, rect_image and rects one per rectangle')
        if m == 0:
            return
        p, ws, hs, pt = _window_arrays(ptrs, sizes, pitches)
        ri = (C.c_int32 * m)(*[int(v) for v in rect_image])
        rc4 = (C.c_int32 * (4 * m))(*[int(v) for q in rects for v in q])
        self._check(self.lib.mdhip_blur_regions(self.h, p, ws, hs, pt, n, ri, rc4, m,
                                                C.c_float(float(radius)), C.c_void_p(stream)), 'mdhip_blur_regions')

    def resample_lanczos(self, src_ptrs, src_sizes, src_pitches, dst_ptrs, dst_sizes, dst_pitches, stream=0):
        """
        Pillow's Image.resize(size, LANCZOS) of device images into device images, bit for bit (include/mdhip.h:
        mdhip_resample_lanczos).  Per image the device address of an RGB uint8 image, its (width, height) and its bytes a
        row, for sources and destinations.  One launch per pass for all images.  Only enqueues.
        """
        n = len(src_ptrs)
        if not (len(src_sizes) == len(src_pitches) == len(dst_ptrs) == len(dst_sizes) == len(dst_pitches) == n):
            raise ValueError('one entry per image is needed in every list')
        if n == 0:
            return
        self._check(self.lib.mdhip_resample_lanczos(self.h, *_window_arrays(src_ptrs, src_sizes, src_pitches), n,
                                                    *_window_arrays(dst_ptrs, dst_sizes, dst_pitches), C.c_void_p(stream)),
                    'mdhip_resample_lanczos')

    def draw_ops(self, ptrs, sizes, pitches, op_image, ops, patches_ptr=0, patch_bytes=0, stream=0):
        """
        Applies each device image's ordered list of drawing operations in place, in one launch (include/mdhip.h:
        mdhip_draw_ops).  op_image: per operation the index of its image; ops: rows of 8 int32 (a solid rectangle or the
        paste of a patch); patches_ptr / patch_bytes: the packed DEVICE buffer the patch operations point into.  Only enqueues.
        """
        n, m = len(ptrs), len(ops)
        if not (len(sizes) == len(pitches) == n) or len(op_image) != m:
            raise ValueError('ptrs, sizes and pitches must have one entry per image, op_image and ops one per operation')
        if m == 0:
            return
        p, ws, hs, pt = _window_arrays(ptrs, sizes, pitches)
        oi = (C.c_int32 * m)(*[int(v) for v in op_image])
        flat = (C.c_int32 * (8 * m))(*[int(v) for q in ops for v in q])
        self._check(self.lib.mdhip_draw_ops(self.h, p, ws, hs, pt, n, oi, flat, m,
                                            C.c_void_p(int(patches_ptr) or None), int(patch_bytes), C.c_void_p(stream)), 'mdhip_draw_ops')

    def draw_ops_from(self, src_ptrs, sizes, src_pitches, dst_ptrs, dst_src, dst_pitches, op_image, ops, patches_ptr=0, patch_bytes=0,
                      stream=0, check=True):
        """
        The fan-out draw (include/mdhip.h: mdhip_draw_ops_from): destination i becomes the pixels of source dst_src[i] under
        the operations whose op_image names i, in one launch for all destinations; the sources are only read and a
        destination without operations is a copy.  ops, patches_ptr, patch_bytes: as for draw_ops.  Only enqueues.
        check=False returns the library's code instead of raising.
        """
        n, k, m = len(src_ptrs), len(dst_ptrs), len(ops)
        if not (len(sizes) == len(src_pitches) == n) or not (len(dst_src) == len(dst_pitches) == k) or len(op_image) != m:
            raise ValueError('one entry per source, per destination and per operation is needed in their lists')
        if k == 0 and m == 0:
            return 0
        p, ws, hs, pt = _window_arrays(src_ptrs, sizes, src_pitches)
        dp = C.cast((C.c_void_p * max(k, 1))(*[int(v) for v in dst_ptrs]), C.POINTER(C.c_void_p))
        ds = (C.c_int32 * max(k, 1))(*[int(v) for v in dst_src])
        dpt = (C.c_int64 * max(k, 1))(*[int(v) for v in dst_pitches])
        oi = (C.c_int32 * max(m, 1))(*[int(v) for v in op_image])
        flat = (C.c_int32 * max(8 * m, 1))(*[int(v) for q in ops for v in q])
        rc = self.lib.mdhip_draw_ops_from(self.h, p, ws, hs, pt, n, dp, ds, dpt, k, oi, flat, m,
                                          C.c_void_p(int(patches_ptr) or None), int(patch_bytes), C.c_void_p(stream))
        if check:
            self._check(rc, 'mdhip_draw_ops_from')
        return rc

    def change_detect(self, ptrs, sizes, blurred_ptrs, ready, pairs, options, mask_ptrs=None, stream=0):
        """
        Change detection between device images (include/mdhip.h: mdhip_change_detect).
        ptrs, sizes:   per image the device address of its dense RGB pixels (0 where its plane is ready) and (width, height)
        blurred_ptrs:  per image the device address of its width x height blurred gray plane; ready[i]: it is filled already
        pairs:         (previous, current) indices; options: jpeg_host.change_options()
        mask_ptrs:     None, or per pair 0 or the device address that receives the dilated mask
        Returns jpeg_host.ChangeArrays.result(): host arrays; the call has completed.
        """
        from . import jpeg_host
        n, m = len(ptrs), len(pairs)
        if not (len(sizes) == len(blurred_ptrs) == len(ready) == n):
            raise ValueError('ptrs, sizes, blurred_ptrs and ready must have one entry per image')
        p, ws, hs, pt = _window_arrays(ptrs, sizes, [3 * s[0] for s in sizes])
        bl = C.cast((C.c_void_p * max(n, 1))(*[int(v) for v in blurred_ptrs]), C.c_void_p)
        rd = (C.c_uint8 * max(n, 1))(*[1 if v else 0 for v in ready])
        pr = (C.c_int32 * max(2 * m, 1))(*[int(v) for q in pairs for v in q])
        mk = None if mask_ptrs is None else C.cast((C.c_void_p * max(m, 1))(*[int(v) or None for v in mask_ptrs]), C.c_void_p)
        out = jpeg_host.ChangeArrays(m, options.region_cap)
        self._check(self.lib.mdhip_change_detect(self.h, p, ws, hs, pt, n, bl, rd, pr, m, C.byref(options), *out.pointers(), mk,
                                                 C.c_void_p(stream)), 'mdhip_change_detect')
        return out.result(m, options.region_cap)

    def label_regions_on(self, mask, min_area=0, cap=256, stream=0):
        """the region stage of change_detect on a host mask (h, w) (include/mdhip.h: mdhip_label_regions_on) -> (labels (h, w)
        int32, n_regions, regions (min(n_regions, cap), 5), overflow)"""
        mask = np.ascontiguousarray(mask, np.uint8)
        h, w = mask.shape
        labels, n_regions, overflow = np.zeros((h, w), np.int32), C.c_int32(0), C.c_uint8(0)
        regions = np.zeros((max(cap, 1), 5), np.int32)
        self._check(self.lib.mdhip_label_regions_on(self.h, mask.ctypes.data, w, h, int(min_area), int(cap), labels.ctypes.data,
                                                    C.addressof(n_regions), regions.ctypes.data, C.addressof(overflow), C.c_void_p(stream)),
                    'mdhip_label_regions_on')
        return labels, n_regions.value, regions[:min(n_regions.value, cap)], overflow.value

    def gray_count(self, ptrs, sizes, pitches, windows, counts=None, stream=0):
        """
        The gray pixels (R == G and R == B) inside a rectangle of each device image, in one launch (include/mdhip.h:
        mdhip_gray_count).
        ptrs, sizes, pitches: per image the device address of an RGB uint8 image, its (width, height) and its bytes a row
        windows:              per image (x, y, w, h), inside the image
        counts:               None, or the uint64 array the call fills (it stays as it is when the call refuses its arguments)
        Returns the counts as Python ints; the call has completed.
        """
        n = len(ptrs)
        if not (len(sizes) == len(pitches) == len(windows) == n):
            raise ValueError('ptrs, sizes, pitches and windows must have one entry per image')
        if counts is None:
            counts = np.zeros(max(n, 1), np.uint64)
        if counts.dtype != np.uint64 or not counts.flags['C_CONTIGUOUS'] or counts.size < n:
            raise ValueError('counts: a contiguous uint64 array with one entry per image is needed')
        m = max(n, 1)
        p = C.cast((C.c_void_p * m)(*[int(v) or None for v in ptrs]), C.c_void_p)
        ws, hs = (C.c_int32 * m)(*[int(v[0]) for v in sizes]), (C.c_int32 * m)(*[int(v[1]) for v in sizes])
        pt = (C.c_int64 * m)(*[int(v) for v in pitches])
        win = (C.c_int32 * (4 * m))(*[int(v) for q in windows for v in q])
        self._check(self.lib.mdhip_gray_count(self.h, p, ws, hs, pt, win, n, counts.ctypes.data, C.c_void_p(stream)), 'mdhip_gray_count')
        return [int(v) for v in counts[:n]]

    def classifier_input(self, crops, size, out_ptr, filter=0, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), stream=0):
        """
        The input tensor of a classifier for crops of device images, in one launch (include/mdhip.h: mdhip_classifier_input).
        crops:   per crop (ptr, pitch, src_w, src_h, canvas_w, canvas_h, off_x, off_y): the device address of the first image
                 pixel that lies in the canvas, the image's bytes a row, the part of the canvas that holds pixels, the canvas,
                 where the part lies in it
        size, filter, mean, std: the side of the tensor, 0 bicubic / 1 bilinear / 2 lanczos, the normalisation
        out_ptr: device address of len(crops) x 3 x size x size floats
        Returns True; False (MDHIP_EUNSUPPORTED, nothing enqueued) when a crop is reduced more than fits on chip.  Only enqueues.
        """
        n = len(crops)
        if n == 0:
            return True
        recs = (_lib.mdhip_classifier_crop * n)(*[_lib.mdhip_classifier_crop(*[int(v) for v in q]) for q in crops])
        rc = self.lib.mdhip_classifier_input(self.h, recs, n, int(size), int(filter), (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                             C.c_void_p(int(out_ptr)), C.c_void_p(stream))
        if rc != _lib.MDHIP_EUNSUPPORTED:
            self._check(rc, 'mdhip_classifier_input')
        return rc == 0

    def thumbnails(self, tiles, filter=0, stream=0):
        """
        Tiles of device images into device sheets, in one launch (include/mdhip.h: mdhip_thumbnails): tile i is Pillow's
        image.crop(box).resize((out_w, out_h)) pasted at dst, bit for bit.
        tiles:   per tile (ptr, pitch, src_w, src_h, canvas_w, canvas_h, off_x, off_y, out_w, out_h, dst, dst_pitch): the
                 canvas as for classifier_input, the tile's size, the device address of its first pixel in its sheet and the
                 sheet's bytes a row.  The tiles of one call must not overlap.
        filter:  0 bicubic (Image.resize's default for RGB) / 1 bilinear / 2 lanczos
        Returns True; False (MDHIP_EUNSUPPORTED, nothing enqueued) when a tile is reduced more than fits on chip.  Only enqueues.
        """
        n = len(tiles)
        if n == 0:
            return True
        recs = (_lib.mdhip_thumbnail * n)(*[_lib.mdhip_thumbnail(*[int(v) for v in q]) for q in tiles])
        rc = self.lib.mdhip_thumbnails(self.h, recs, n, int(filter), C.c_void_p(stream))
        if rc != _lib.MDHIP_EUNSUPPORTED:
            self._check(rc, 'mdhip_thumbnails')
        return rc == 0

    def forward(self, n, h, w, stream=0):
        self._check(self.lib.mdhip_forward(self.h, int(n), int(h), int(w), C.c_void_p(stream)), 'mdhip_forward')

    def forward_tta(self, n, h, w, stream=0):
        """augmented inference (yolov5 _forward_augment) on the batch left by preprocess()"""
        self._check(self.lib.mdhip_forward_tta(self.h, int(n), int(h), int(w), C.c_void_p(stream)), 'mdhip_forward_tta')

    def tta_input_on(self, n, h, w, tta_pass, stream=0):
        """the network input of scaled pass 1 or 2 of forward_tta on the batch left by preprocess(), as (n, 3, oh, ow) float32 of
        the stored values (tests; include/mdhip.h: mdhip_tta_input_on).  The context's input holds the batch again afterwards."""
        oh, ow = C.c_int(), C.c_int()
        self._check(self.lib.mdhip_tta_input_on(self.h, int(n), int(h), int(w), int(tta_pass), None, C.byref(oh), C.byref(ow),
                                                C.c_void_p(stream)), 'mdhip_tta_input_on')
        out = np.empty((n, 3, oh.value, ow.value), dtype=np.float32)
        self._check(self.lib.mdhip_tta_input_on(self.h, int(n), int(h), int(w), int(tta_pass), _lib.np_ptr(out), C.byref(oh),
                                                C.byref(ow), C.c_void_p(stream)), 'mdhip_tta_input_on')
        return out

    def last_num_anchors(self):
        return self.lib.mdhip_last_num_anchors(self.h)

    # -- fp8 mode (dtype='fp8') -----------------------------------------------------------
    def calibrate(self, n, h, w, stream=0):
        """records the ranges of the e4m3 tensors on the batch left by preprocess() and derives their scales"""
        self._check(self.lib.mdhip_calibrate(self.h, int(n), int(h), int(w), C.c_void_p(stream)), 'mdhip_calibrate')

    def fp8_scales(self):
        """[(scale, model layer, op index)] of the e4m3 tensors, in execution order"""
        n = self.lib.mdhip_fp8_num_tensors(self.h)
        if n <= 0:
            return []
        sc = (C.c_float * n)()
        ly = (C.c_int32 * n)()
        op = (C.c_int32 * n)()
        self.lib.mdhip_fp8_get_scales(self.h, sc, ly, op, n)
        return [(float(sc[i]), int(ly[i]), int(op[i])) for i in range(n)]

    def set_fp8_scales(self, scales):
        arr = (C.c_float * len(scales))(*[float(v) for v in scales])
        self._check(self.lib.mdhip_fp8_set_scales(self.h, arr, len(scales)), 'mdhip_fp8_set_scales')

    def nms(self, n, conf_thres, iou_thres, max_det=300, stream=0):
        out = np.empty((n, max_det, 6), dtype=np.float32)
        counts = np.empty((n,), dtype=np.int32)
        self._check(self.lib.mdhip_nms(self.h, int(n), float(conf_thres), float(iou_thres), int(max_det),
                                       _lib.np_ptr(out), _lib.np_ptr(counts), C.c_void_p(stream)), 'mdhip_nms')
        return out, counts

    def nms_enqueue(self, n, conf_thres, iou_thres, max_det=300, slot=0, stream=0):
        """asynchronous NMS + D2H into pinned slot `slot`; pair with nms_wait(slot)"""
        self._check(self.lib.mdhip_nms_enqueue(self.h, int(n), float(conf_thres), float(iou_thres), int(max_det),
                                               int(slot), C.c_void_p(stream)), 'mdhip_nms_enqueue')
        self._slot_shape = getattr(self, '_slot_shape', {})
        self._slot_shape[slot] = (int(n), int(max_det))

    def nms_wait(self, slot=0):
        """blocks until slot is complete; returns numpy *views* of the pinned slot (valid until re-enqueued)"""
        out = C.POINTER(C.c_float)()
        cnt = C.POINTER(C.c_int32)()
        self._check(self.lib.mdhip_nms_wait(self.h, int(slot), C.byref(out), C.byref(cnt)), 'mdhip_nms_wait')
        n, max_det = self._slot_shape[slot]
        det = np.ctypeslib.as_array(out, shape=(n, max_det, 6))
        counts = np.ctypeslib.as_array(cnt, shape=(n,))
        return det, counts

    def nms_on(self, pred, conf_thres, iou_thres, max_det=300, stream=0):
        pred = np.ascontiguousarray(pred, dtype=np.float32)
        n, a, no = pred.shape
        if no != self.no:
            raise ValueError('prediction width {} != {}'.format(no, self.no))
        out = np.empty((n, max_det, 6), dtype=np.float32)
        counts = np.empty((n,), dtype=np.int32)
        self._check(self.lib.mdhip_nms_on(self.h, _lib.np_ptr(pred), n, a, float(conf_thres), float(iou_thres),
                                          int(max_det), _lib.np_ptr(out), _lib.np_ptr(counts),
                                          C.c_void_p(stream)), 'mdhip_nms_on')
        return out, counts

    # -- introspection ------------------------------------------------------------------
    def num_anchors(self, h, w):
        return self.lib.mdhip_num_anchors(self.h, int(h), int(w))

    def read_predictions(self, n, h=None, w=None, stream=0):
        out = np.empty((n, self.last_num_anchors(), self.no), dtype=np.float32)
        self._check(self.lib.mdhip_read_predictions(self.h, n, _lib.np_ptr(out), C.c_void_p(stream)),
                    'mdhip_read_predictions')
        return out

    def read_input(self, n, h, w, stream=0):
        out = np.empty((n, 3, h, w), dtype=np.float32)
        self._check(self.lib.mdhip_read_input(self.h, n, h, w, _lib.np_ptr(out), C.c_void_p(stream)), 'mdhip_read_input')
        return out

    def read_layer(self, layer, n, stream=0):
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.mdhip_read_layer(self.h, layer, n, None, C.byref(c), C.byref(h), C.byref(w),
                                              C.c_void_p(stream)), 'mdhip_read_layer')
        out = np.empty((n, c.value, h.value, w.value), dtype=np.float32)
        self._check(self.lib.mdhip_read_layer(self.h, layer, n, _lib.np_ptr(out), C.byref(c), C.byref(h),
                                              C.byref(w), C.c_void_p(stream)), 'mdhip_read_layer')
        return out

    def run_ops(self, n, h, w, first, count, stream=0):
        """ops [first, first + count) of a forward of n images of h x w, each as its own launch (mdhip_run_ops)"""
        self._check(self.lib.mdhip_run_ops(self.h, int(n), int(h), int(w), int(first), int(count), C.c_void_p(stream)), 'mdhip_run_ops')

    def read_op_tensor(self, op, which, n, stream=0):
        """a view of an op as stored, NCHW float32: which = 0 in, 1 out, 2 res, 3 out2, 4..6 fsrc (mdhip_read_op_tensor)"""
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        args = (C.byref(c), C.byref(h), C.byref(w), C.c_void_p(stream))
        self._check(self.lib.mdhip_read_op_tensor(self.h, int(op), int(which), int(n), None, *args), 'mdhip_read_op_tensor')
        out = np.empty((n, c.value, h.value, w.value), dtype=np.float32)
        self._check(self.lib.mdhip_read_op_tensor(self.h, int(op), int(which), int(n), _lib.np_ptr(out), *args), 'mdhip_read_op_tensor')
        return out

    def read_op_weights(self, op):
        """(weights [c_out][c_in][kh][kw], bias [c_out]) of a conv or depthwise op as the device holds them (mdhip_read_op_weights)"""
        dims = [C.c_int() for _ in range(4)]
        refs = [C.byref(d) for d in dims]
        self._check(self.lib.mdhip_read_op_weights(self.h, int(op), None, None, *refs), 'mdhip_read_op_weights')
        w = np.empty(tuple(d.value for d in dims), dtype=np.float32)
        b = np.empty((dims[0].value,), dtype=np.float32)
        self._check(self.lib.mdhip_read_op_weights(self.h, int(op), _lib.np_ptr(w), _lib.np_ptr(b), *refs), 'mdhip_read_op_weights')
        return w, b

    def num_ops(self):
        return self.lib.mdhip_num_ops(self.h)

    def op_infos(self):
        res = []
        for i in range(self.num_ops()):
            info = _lib.mdhip_op_info()
            self._check(self.lib.mdhip_get_op_info(self.h, i, C.byref(info)), 'mdhip_get_op_info')
            res.append(dict(op=i, name=info.name.decode(), kind=info.kind, layer=info.layer, m=info.m,
                            n=info.n, k=info.k, flops=info.flops, bytes=info.bytes, cfg=info.cfg,
                            ntaps=info.ntaps, stride=info.stride, has_res=info.has_res, variant=info.variant))
        return res

    def forward_timed(self, n, h, w, stream=0):
        ms = np.zeros((self.num_ops(),), dtype=np.float32)
        self._check(self.lib.mdhip_forward_timed(self.h, n, h, w, _lib.np_ptr(ms), C.c_void_p(stream)),
                    'mdhip_forward_timed')
        return ms

    def time_forwards(self, enable=True):
        """bracket every forward() with a HIP event pair on its stream (see forward_times)"""
        self._check(self.lib.mdhip_time_forwards(self.h, 1 if enable else 0), 'mdhip_time_forwards')

    def forward_times(self, max_n=64):
        """durations (ms) of the most recent forwards measured since time_forwards(True), oldest first"""
        ms = np.zeros((max_n,), dtype=np.float32)
        n = self.lib.mdhip_forward_times(self.h, _lib.np_ptr(ms), int(max_n))
        if n < 0:
            self._check(n, 'mdhip_forward_times')
        return ms[:n].copy()

    def set_op_cfg(self, op, cfg):
        self._check(self.lib.mdhip_set_op_cfg(self.h, op, cfg), 'mdhip_set_op_cfg')

    def set_fuse(self, on):
        """fused bottleneck launches on (default) / off (the 1x1 and the 3x3 as two launches: same bits)"""
        self._check(self.lib.mdhip_set_fuse(self.h, 1 if on else 0), 'mdhip_set_fuse')

    def set_option(self, name, value):
        """named integer switch of the context (include/mdhip.h: mdhip_set_option)"""
        self._check(self.lib.mdhip_set_option(self.h, name.encode(), int(value)), 'mdhip_set_option({})'.format(name))

    def set_graph(self, mode, max_n=0):
        """graph replay of forward(): 0 / False = off, 1 / True = every forward, 2 / 'auto' = forwards of at most max_n
        images (default 8); same kernels and arguments, bit-identical results (include/mdhip.h: mdhip_set_graph)"""
        mode = {'off': 0, 'on': 1, 'auto': 2, False: 0, True: 1}.get(mode, mode)
        self._check(self.lib.mdhip_set_graph(self.h, int(mode), int(max_n)), 'mdhip_set_graph')

    def op_supports_cfg(self, op, cfg):
        return self.lib.mdhip_op_supports_cfg(self.h, int(op), int(cfg)) == 1

    def conv_cfg_name(self, cfg):
        return self.lib.mdhip_conv_cfg_name(int(cfg)).decode()

    def cfg_is_bitwise(self, cfg):
        return self.lib.mdhip_cfg_is_bitwise(int(cfg)) == 1

    def num_conv_cfgs(self):
        return self.lib.mdhip_num_conv_cfgs()

    def time_op(self, op, n, h, w, iters=10, stream=0):
        ms = C.c_float()
        self._check(self.lib.mdhip_time_op(self.h, op, n, h, w, iters, C.byref(ms), C.c_void_p(stream)), 'mdhip_time_op')
        return ms.value
