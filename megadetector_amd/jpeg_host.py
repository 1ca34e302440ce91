"""
ctypes binding of libmdjpeg.so (C ABI: include/mdjpeg.h): the host half of the GPU JPEG feed.

parse() / decode() turn the bytes of a baseline JPEG into quantised DCT coefficients; the GPU rebuilds the pixels
(hip_backend.HipContext.jpeg_reconstruct).  Whatever the decoder does not take cleanly is reported, never guessed at: the
caller then decodes that file with PIL.

This module must stay import-light (ctypes + numpy only, like feed.py): the spawned loader processes import it, and
they may never open the GPU -- libmdjpeg.so links nothing of HIP.
"""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmdjpeg.so')

MDJPEG_OK = 0
MDJPEG_EINVAL = -1
MDJPEG_EUNSUPPORTED = -2
MDJPEG_ECORRUPT = -3
MDJPEG_ECAPACITY = -4


class mdjpeg_info(C.Structure):
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('components', C.c_int32),
                ('h_samp', C.c_int32 * 3), ('v_samp', C.c_int32 * 3), ('restart_interval', C.c_int32),
                ('mcus_x', C.c_int32), ('mcus_y', C.c_int32), ('blocks_w', C.c_int32 * 3), ('blocks_h', C.c_int32 * 3),
                ('plane_offset', C.c_int64 * 3), ('coef_count', C.c_int64), ('quant', (C.c_uint16 * 64) * 3),
                ('supported', C.c_int32), ('reason', C.c_char * 100)]


MAX_TABLES = 6


class mdjpeg_scan_info(C.Structure):
    _fields_ = [('info', mdjpeg_info), ('n_tables', C.c_int32), ('dc_table', C.c_int32 * 3), ('ac_table', C.c_int32 * 3),
                ('huff_counts', (C.c_uint8 * 16) * MAX_TABLES), ('huff_vals', (C.c_uint8 * 256) * MAX_TABLES),
                ('scan_begin', C.c_int64), ('scan_end', C.c_int64), ('n_segments', C.c_int32), ('reserved', C.c_int32)]


#: every symbol include/mdjpeg.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'mdjpeg_parse': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(mdjpeg_info)]),
    'mdjpeg_decode': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(mdjpeg_info), C.c_void_p, C.c_size_t]),
    'mdjpeg_scan': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(mdjpeg_scan_info), C.c_void_p, C.c_size_t]),
    'mdjpeg_decode_subsequences': (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(mdjpeg_info), C.c_void_p, C.c_size_t]),
    'mdjpeg_version': (C.c_char_p, []),
}

_lib = None


def load():
    """Loads libmdjpeg.so (once).  Raises RuntimeError when the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('libmdjpeg.so not found at {}: build it with `make -C megadetector_amd/csrc`'.format(LIB_PATH))
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class JpegHeader:
    """What mdjpeg_parse reports, as plain Python data."""

    def __init__(self, info, rc):
        nc = info.components if info.components in (1, 3) else 0
        self.rc = int(rc)
        self.width, self.height, self.components = info.width, info.height, info.components
        self.supported = bool(info.supported)
        self.reason = info.reason.decode('ascii', 'replace')
        self.h_samp = tuple(info.h_samp[:nc])
        self.v_samp = tuple(info.v_samp[:nc])
        self.restart_interval = info.restart_interval
        self.mcus_x, self.mcus_y = info.mcus_x, info.mcus_y
        self.blocks_w = tuple(info.blocks_w[:nc])
        self.blocks_h = tuple(info.blocks_h[:nc])
        self.plane_offset = tuple(info.plane_offset[:nc])
        self.coef_count = int(info.coef_count)
        self.quant = np.ctypeslib.as_array(info.quant).reshape(3, 64).copy()      # uint16, natural order

    def planes(self, coef):
        """views of the flat int16 coefficient buffer: one [blocks_h][blocks_w][64] array per component"""
        return [coef[o:o + bh * bw * 64].reshape(bh, bw, 64)
                for o, bh, bw in zip(self.plane_offset, self.blocks_h, self.blocks_w)]


def _as_buffer(data):
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or not data.flags.c_contiguous:
            raise ValueError('file bytes must be a contiguous uint8 array')
        return data, data.ctypes.data, data.size
    arr = np.frombuffer(data, dtype=np.uint8)
    return arr, arr.ctypes.data, arr.size


def parse(data):
    """data: the file's bytes (bytes or uint8 array).  Returns a JpegHeader; .supported says whether decode() takes it."""
    hold, ptr, n = _as_buffer(data)
    info = mdjpeg_info()
    rc = load().mdjpeg_parse(ptr, n, C.byref(info))
    return JpegHeader(info, rc)


def decode(data, out=None):
    """
    Entropy-decodes the scan.  out: a contiguous int16 array to decode into (e.g. a view of a shared-memory slot); it is
    allocated when None.  Returns (rc, header, out): rc == MDJPEG_OK and the first header.coef_count values of `out`
    hold the planes, or rc < 0 (header.reason says why) and `out` holds nothing of use.
    """
    hold, ptr, n = _as_buffer(data)
    lib = load()
    info = mdjpeg_info()
    if out is None:
        rc = lib.mdjpeg_parse(ptr, n, C.byref(info))
        if rc != MDJPEG_OK:
            return rc, JpegHeader(info, rc), None
        out = np.empty((int(info.coef_count),), dtype=np.int16)
    if out.dtype != np.int16 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError('out must be a writeable contiguous int16 array')
    rc = lib.mdjpeg_decode(ptr, n, C.byref(info), out.ctypes.data, out.size)
    return rc, JpegHeader(info, rc), out


def scan(data, seg_out=None):
    """
    The descriptor of the scan for the GPU's entropy decoder (mdjpeg_scan): no Huffman symbol is decoded.  seg_out: a
    contiguous uint32 array for the segment offsets (allocated when None).  Returns (rc, mdjpeg_scan_info, offsets): with
    rc == MDJPEG_OK the first n_segments values of `offsets` are each restart segment's first byte, counted from
    scan_begin; otherwise info.reason says why the file is left to the caller's decoder.
    """
    hold, ptr, n = _as_buffer(data)
    lib = load()
    sc = mdjpeg_scan_info()
    if seg_out is None:
        seg_out = np.empty((64,), dtype=np.uint32)
        rc = lib.mdjpeg_scan(ptr, n, C.byref(sc), seg_out.ctypes.data, seg_out.size)
        if rc != MDJPEG_ECAPACITY or sc.n_segments <= seg_out.size:
            return rc, sc, seg_out
        seg_out = np.empty((sc.n_segments,), dtype=np.uint32)
    if seg_out.dtype != np.uint32 or not seg_out.flags.c_contiguous or not seg_out.flags.writeable:
        raise ValueError('seg_out must be a writeable contiguous uint32 array')
    rc = lib.mdjpeg_scan(ptr, n, C.byref(sc), seg_out.ctypes.data, seg_out.size)
    return rc, sc, seg_out


def decode_subsequences(data, subseq_bits, out=None):
    """The host model of the GPU entropy decoder (mdjpeg_decode_subsequences): results as decode().  For tests."""
    hold, ptr, n = _as_buffer(data)
    lib = load()
    info = mdjpeg_info()
    if out is None:
        rc = lib.mdjpeg_parse(ptr, n, C.byref(info))
        if rc != MDJPEG_OK:
            return rc, JpegHeader(info, rc), None
        out = np.empty((int(info.coef_count),), dtype=np.int16)
    rc = lib.mdjpeg_decode_subsequences(ptr, n, int(subseq_bits), C.byref(info), out.ctypes.data, out.size)
    return rc, JpegHeader(info, rc), out


# ---- quantisation tables of an encoder quality (mdhip_jpeg_recompress) --------------------------------------------------
# the example tables of the JPEG standard (ITU-T T.81, Annex K.1), natural order
_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def check_quality(quality):
    """a Pillow / libjpeg `quality`: an integer from 1 to 100; anything else is a ValueError"""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError('JPEG quality must be an integer from 1 to 100, got {!r}'.format(quality))
    return int(quality)


def quant_tables(quality):
    """
    The (luminance, chrominance) quantisation tables Image.save(quality=quality) writes: the standard's tables under
    libjpeg's quality scaling (jpeg_quality_scaling, jpeg_add_quant_table with force_baseline).  uint16 [64], natural order.
    """
    quality = check_quality(quality)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(base, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16)
                 for base in (_STD_LUMA, _STD_CHROMA))


# ---- a coefficient image in a ring slot (feed.py decode='coefficients') ------------------------------------------------
# slot = [16 x int32 header][3 x 64 uint16 quantisation tables][int16 planes]
SLOT_MAGIC = 0x4D444A31
SLOT_HEADER_BYTES = 512              # 64 + 384, rounded up: the planes start 256-byte aligned within the slot
_SLOT_QUANT_OFF = 64


def decode_into_slot(data, slot_view, rotation):
    """Entropy-decodes `data` into the flat uint8 view of a slot.  Returns the code of mdjpeg_decode."""
    coef = slot_view[SLOT_HEADER_BYTES:SLOT_HEADER_BYTES + (slot_view.size - SLOT_HEADER_BYTES) // 2 * 2].view(np.int16)
    rc, h, _ = decode(data, out=coef)
    if rc != MDJPEG_OK:
        return rc
    head = slot_view[:64].view(np.int32)
    head[:] = 0
    head[0:8] = (SLOT_MAGIC, h.width, h.height, h.components, h.h_samp[0], h.v_samp[0], int(rotation), h.coef_count)
    head[8:8 + h.components] = h.blocks_w
    head[11:11 + h.components] = h.blocks_h
    slot_view[_SLOT_QUANT_OFF:_SLOT_QUANT_OFF + 384].view(np.uint16)[:] = h.quant.reshape(-1)
    return rc


class CoefficientImage:
    """
    A JPEG as the GPU takes it: quantised coefficient planes plus what reconstruction needs.  `.shape` is that of the
    RGB image mdhip_jpeg_reconstruct writes (rotated H x W x 3), which is all the letterbox geometry reads.
    coef: flat int16 (planes of Y[, Cb, Cr], each [blocks_h][blocks_w][64]); quant: [3][64] uint16, natural order.
    """

    ndim = 3
    dtype = np.dtype(np.uint8)

    def __init__(self, width, height, components, h_samp, v_samp, rotation, blocks_w, blocks_h, quant, coef):
        self.width, self.height, self.components = int(width), int(height), int(components)
        self.h_samp, self.v_samp, self.rotation = int(h_samp), int(v_samp), int(rotation)
        self.blocks_w = tuple(int(v) for v in blocks_w)
        self.blocks_h = tuple(int(v) for v in blocks_h)
        self.quant, self.coef = quant, coef
        if self.rotation in (90, 270):
            self.shape = (self.width, self.height, 3)
        else:
            self.shape = (self.height, self.width, 3)

    @property
    def nbytes(self):
        return self.coef.nbytes

    @classmethod
    def from_header(cls, header, coef, rotation=0):
        """from the results of decode()"""
        return cls(header.width, header.height, header.components, header.h_samp[0], header.v_samp[0], rotation,
                   header.blocks_w, header.blocks_h, header.quant, coef[:header.coef_count])

    @classmethod
    def from_slot(cls, slot_view, shape=None):
        """from the flat uint8 view of a ring slot written by decode_into_slot (views, nothing is copied)"""
        head = slot_view[:64].view(np.int32)
        if int(head[0]) != SLOT_MAGIC:
            raise ValueError('ring slot does not hold a coefficient image')
        nc = int(head[3])
        quant = slot_view[_SLOT_QUANT_OFF:_SLOT_QUANT_OFF + 384].view(np.uint16).reshape(3, 64)
        coef = slot_view[SLOT_HEADER_BYTES:SLOT_HEADER_BYTES + 2 * int(head[7])].view(np.int16)
        im = cls(head[1], head[2], nc, head[4], head[5], head[6], head[8:8 + nc], head[11:11 + nc], quant, coef)
        if shape is not None and tuple(shape) != im.shape:
            raise ValueError('slot holds a {} image, the queue announced {}'.format(im.shape, tuple(shape)))
        return im


class DeviceCoefficientImage(CoefficientImage):
    """A CoefficientImage whose planes are in device memory already (the GPU's entropy decoder wrote them): `.coef` is a
    Planes record instead of a host array, and nothing of it is copied."""

    class Planes:
        """count int16 values at element `offset` of a device tensor (kept alive by this record)"""

        def __init__(self, tensor, offset, count):
            self.base, self.offset, self.count = tensor, int(offset), int(count)
            self.nbytes = 0                   # bytes a host-to-device copy has to move

        def data_ptr(self):
            return self.base.data_ptr() + 2 * self.offset

        def tensor(self):
            return self.base[self.offset:self.offset + self.count]


class ScanFailure:
    """stands for a file the GPU's entropy decoder flagged and PIL could not decode either; .error is PIL's exception"""

    def __init__(self, error):
        self.error = error


# ---- a JPEG as its compressed scan in a ring slot (feed.py decode='scan') ---------------------------------------------
# slot = [16 x int32 header][mdjpeg_scan_info][uint32 segment offsets][the file's bytes]: the loader decodes no Huffman
# symbol, and the detector holds the whole file, so that it can decode a file the GPU flags with PIL itself
SCAN_SLOT_MAGIC = 0x4D444A32
_SCAN_DESC_OFF = 64
_SCAN_SEG_OFF = (_SCAN_DESC_OFF + C.sizeof(mdjpeg_scan_info) + 255) // 256 * 256


def scan_into_slot(data, slot_view, rotation):
    """Writes the descriptor of `data` (the file's bytes) and the bytes themselves into the flat uint8 view of a slot.
    Returns the code of mdjpeg_scan; MDJPEG_ECAPACITY also when the slot is too small for the file."""
    arr, _, n = _as_buffer(data)
    room = slot_view.size - _SCAN_SEG_OFF - n
    if room < 4:
        return MDJPEG_ECAPACITY
    seg = slot_view[_SCAN_SEG_OFF:_SCAN_SEG_OFF + room // 4 * 4].view(np.uint32)
    rc, sc, _ = scan(arr, seg_out=seg)
    if rc != MDJPEG_OK:
        return rc
    file_off = (_SCAN_SEG_OFF + 4 * sc.n_segments + 255) // 256 * 256
    if file_off + n > slot_view.size:
        return MDJPEG_ECAPACITY
    head = slot_view[:64].view(np.int32)
    head[:] = 0
    head[0:5] = (SCAN_SLOT_MAGIC, int(rotation), sc.n_segments, file_off, n)
    C.memmove(slot_view[_SCAN_DESC_OFF:].ctypes.data, C.addressof(sc), C.sizeof(sc))
    slot_view[file_off:file_off + n] = arr
    return rc


class ScanImage:
    """
    A JPEG as the GPU's entropy decoder takes it: the descriptor of mdjpeg_scan, the segment offsets and the file's bytes.
    `.shape` is that of the RGB image mdhip_jpeg_reconstruct writes in the end (rotated H x W x 3).
    """

    ndim = 3
    dtype = np.dtype(np.uint8)

    def __init__(self, desc, seg_offsets, file_bytes, rotation):
        self.desc, self.seg_offsets, self.file, self.rotation = desc, seg_offsets, file_bytes, int(rotation)
        info = desc.info
        self.width, self.height, self.components = int(info.width), int(info.height), int(info.components)
        self.coef_count = int(info.coef_count)
        self.shape = (self.width, self.height, 3) if self.rotation in (90, 270) else (self.height, self.width, 3)

    @property
    def scan_bytes(self):
        """view of the entropy-coded bytes [scan_begin, scan_end)"""
        return self.file[int(self.desc.scan_begin):int(self.desc.scan_end)]

    @property
    def nbytes(self):
        return int(self.desc.scan_end - self.desc.scan_begin)

    def coefficient_image(self, coef=None):
        """the CoefficientImage of this file once its planes are decoded (coef: what holds them, may stay None)"""
        i = self.desc.info
        nc = self.components
        quant = np.ctypeslib.as_array(i.quant).reshape(3, 64).copy()
        kind = DeviceCoefficientImage if isinstance(coef, DeviceCoefficientImage.Planes) else CoefficientImage
        return kind(i.width, i.height, nc, i.h_samp[0], i.v_samp[0], self.rotation, i.blocks_w[:nc], i.blocks_h[:nc], quant, coef)

    @classmethod
    def from_bytes(cls, data, rotation=0):
        """-> (rc, ScanImage or None, reason) from a file's bytes"""
        arr, _, _ = _as_buffer(data)
        rc, sc, seg = scan(arr)
        if rc != MDJPEG_OK:
            return rc, None, sc.info.reason.decode('ascii', 'replace')
        return rc, cls(sc, seg[:sc.n_segments].copy(), arr, rotation), ''

    @classmethod
    def from_slot(cls, slot_view, shape=None):
        """from the flat uint8 view of a ring slot written by scan_into_slot (the descriptor is copied, the bytes are views)"""
        head = slot_view[:64].view(np.int32)
        if int(head[0]) != SCAN_SLOT_MAGIC:
            raise ValueError('ring slot does not hold a JPEG scan')
        sc = mdjpeg_scan_info()
        C.memmove(C.addressof(sc), slot_view[_SCAN_DESC_OFF:].ctypes.data, C.sizeof(sc))
        seg = slot_view[_SCAN_SEG_OFF:_SCAN_SEG_OFF + 4 * int(head[2])].view(np.uint32)
        im = cls(sc, seg, slot_view[int(head[3]):int(head[3]) + int(head[4])], int(head[1]))
        if shape is not None and tuple(shape) != im.shape:
            raise ValueError('slot holds a {} image, the queue announced {}'.format(im.shape, tuple(shape)))
        return im
