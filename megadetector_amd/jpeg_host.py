"""
ctypes binding of libmdjpeg.so (C ABI: include/mdjpeg.h): the host half of the GPU JPEG feed -- header parser, entropy decoder
and scan descriptor (csrc/jpeg_entropy.cpp) -- and the host models the CPU suite holds the image kernels to: the entropy
encoder and the kept-block merge (csrc/jpeg_encode_host.cpp), blur, resample, drawing, classifier input and thumbnails
(csrc/image_host.cpp), repeat-detection elimination (csrc/rde_host.cpp).

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


class mdjpeg_thumbnail(C.Structure):
    _fields_ = [('src', C.c_void_p), ('pitch', C.c_int64), ('src_w', C.c_int32), ('src_h', C.c_int32),
                ('canvas_w', C.c_int32), ('canvas_h', C.c_int32), ('off_x', C.c_int32), ('off_y', C.c_int32),
                ('out_w', C.c_int32), ('out_h', C.c_int32), ('dst', C.c_void_p), ('dst_pitch', C.c_int64)]


class mdjpeg_change_options(C.Structure):
    _fields_ = [('blur_kernel_size', C.c_int32), ('threshold_type', C.c_int32), ('threshold', C.c_int32),
                ('dilate_kernel_size', C.c_int32), ('dilate_iterations', C.c_int32), ('min_area', C.c_int32),
                ('has_ignore', C.c_int32), ('region_cap', C.c_int32), ('ignore_fraction', C.c_double)]


#: every symbol include/mdjpeg.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'mdjpeg_parse': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(mdjpeg_info)]),
    'mdjpeg_decode': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(mdjpeg_info), C.c_void_p, C.c_size_t]),
    'mdjpeg_scan': (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(mdjpeg_scan_info), C.c_void_p, C.c_size_t]),
    'mdjpeg_decode_subsequences': (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(mdjpeg_info), C.c_void_p, C.c_size_t]),
    'mdjpeg_encode_subsequences': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                             C.POINTER(C.c_size_t)]),
    'mdjpeg_encode_bound': (C.c_int64, [C.c_int32, C.c_int32]),
    'mdjpeg_encode_subsequences_sampled': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]),
    'mdjpeg_encode_sampled_bound': (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    'mdjpeg_keep_merge': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int,
                                    C.POINTER(C.c_int32)]),
    'mdjpeg_blur_regions': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_float]),
    'mdjpeg_blur_regions_chunked': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int,
                                              C.c_float, C.c_int]),
    'mdjpeg_blur_weights': (C.c_int, [C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    'mdjpeg_resample': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int64]),
    'mdjpeg_draw': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int64]),
    'mdjpeg_draw_from': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int64]),
    'mdjpeg_classifier_input': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p]),
    'mdjpeg_classifier_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    'mdjpeg_thumbnails': (C.c_int, [C.POINTER(mdjpeg_thumbnail), C.c_int, C.c_int32]),
    'mdjpeg_repeat_detections': (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    'mdjpeg_change_detect': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mdjpeg_gray_count': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'mdjpeg_gray_count_walk': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
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


# ---- a JPEG file around an entropy-coded scan (mdhip_jpeg_encode) ------------------------------------------------------
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# the example Huffman tables of the standard (ITU-T T.81, K.3 - K.6) as DHT segments carry them: (class << 4 | id, codes of
# each length, symbols), in the order libjpeg writes them
_STD_HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
)
_HEADERS = {}


def _segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, 'big') + payload


def jfif_file(width, height, quality, scan_bytes):
    """
    The file Image.fromarray(rgb).save(f, 'JPEG', quality=quality) writes for a width x height RGB image whose entropy-coded
    scan is `scan_bytes` (mdhip_jpeg_encode; mdjpeg_encode_subsequences): SOI, APP0 (JFIF 1.01, no density unit, 1 x 1), the
    two DQT segments, SOF0 (three components, 4:2:0), the standard's four DHT segments, SOS, the scan, EOI.  Pillow also
    copies a COM segment of the SOURCE file (info['comment']) into what it saves; the files built here carry none.
    """
    width, height = int(width), int(height)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError('a JPEG is 1 .. 65535 pixels wide and high, got {} x {}'.format(width, height))
    quality = check_quality(quality)
    if quality not in _HEADERS:
        ql, qc = quant_tables(quality)
        zz = np.array(_ZIGZAG)
        front = b'\xff\xd8' + _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
        front += _segment(0xDB, b'\x00' + ql[zz].astype(np.uint8).tobytes()) + _segment(0xDB, b'\x01' + qc[zz].astype(np.uint8).tobytes())
        back = b''.join(_segment(0xC4, bytes((tc_th,)) + bytes(counts) + bytes(vals)) for tc_th, counts, vals in _STD_HUFFMAN)
        back += _segment(0xDA, b'\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00')
        _HEADERS[quality] = (front, back)
    front, back = _HEADERS[quality]
    sof = _segment(0xC0, b'\x08' + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + b'\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01')
    return b''.join((front, sof, back, bytes(scan_bytes), b'\xff\xd9'))


#: chroma sampling numbered as Pillow's `subsampling` (include/mdhip.h MDHIP_JPEG_H1V1 ...) -> the luma sampling factors
SAMPLING_FACTORS = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


def sampling_of(header):
    """the sampling number of a JpegHeader (parse()), or None when it is none of 4:4:4, 4:2:2 and 4:2:0 of three components"""
    if header.components != 3 or tuple(header.h_samp[1:]) != (1, 1) or tuple(header.v_samp[1:]) != (1, 1):
        return None
    for number, factors in SAMPLING_FACTORS.items():
        if (header.h_samp[0], header.v_samp[0]) == factors:
            return number
    return None


def sampled_file(width, height, quant_luma, quant_chroma, sampling, scan_bytes, exif=b'', comment=None):
    """
    The file Pillow writes around the scan `scan_bytes` (mdhip_jpeg_encode_sampled; mdjpeg_encode_subsequences_sampled) of a
    width x height RGB image for save(f, 'JPEG', qtables=[quant_luma, quant_chroma], subsampling=sampling, exif=exif) -- and so
    for save(f, exif=exif, quality='keep') of an image opened from a JPEG with these two tables and this sampling, which is
    what the reference's exif_preserving_save does: SOI, APP0 (JFIF 1.01, no density unit, 1 x 1), APP1 with `exif` (the bytes
    of Exif.tobytes(); none when empty), the COM segment Pillow copies from info['comment'] (none when empty or None), one DQT
    segment per table with 8-bit entries in zig-zag order, SOF0 with the sampling factors, the standard's four DHT segments,
    SOS, the scan, EOI.  The tables: 64 entries of 1 .. 255, natural order.
    """
    width, height = int(width), int(height)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError('a JPEG is 1 .. 65535 pixels wide and high, got {} x {}'.format(width, height))
    if sampling not in SAMPLING_FACTORS:
        raise ValueError('sampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got {!r}'.format(sampling))
    tables = [np.asarray(t, dtype=np.int64).reshape(-1) for t in (quant_luma, quant_chroma)]
    if any(t.size != 64 or t.min() < 1 or t.max() > 255 for t in tables):
        raise ValueError('a quantisation table has 64 entries of 1 .. 255')
    exif, comment = bytes(exif or b''), bytes(comment or b'')
    if len(exif) > 65533 or len(comment) > 65533:
        raise ValueError('EXIF data or comment is too long for one segment')
    zz = np.array(_ZIGZAG)
    parts = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    if exif:
        parts.append(_segment(0xE1, exif))
    if comment:
        parts.append(_segment(0xFE, comment))
    parts += [_segment(0xDB, bytes((k,)) + t[zz].astype(np.uint8).tobytes()) for k, t in enumerate(tables)]
    hs, vs = SAMPLING_FACTORS[sampling]
    parts.append(_segment(0xC0, b'\x08' + height.to_bytes(2, 'big') + width.to_bytes(2, 'big') + b'\x03\x01' + bytes((hs << 4 | vs,))
                          + b'\x00\x02\x11\x01\x03\x11\x01'))
    parts += [_segment(0xC4, bytes((tc_th,)) + bytes(counts) + bytes(vals)) for tc_th, counts, vals in _STD_HUFFMAN]
    parts += [_segment(0xDA, b'\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'), bytes(scan_bytes), b'\xff\xd9']
    return b''.join(parts)


def keep_source(path, data=None):
    """
    What exif_preserving_save(image, target, quality='keep') takes from the source file of `image`, the image the reference's
    open_image makes of `path`, read from the LAZILY opened file (Image.open parses headers and decodes no pixel): a dict with
      'size', 'rotation'  of the image open_image gives, and the angle it turned the file's pixels by
      'exif'              the bytes of getexif().tobytes() (Pillow writes them as APP1; never empty)
      'comment'           info['comment'], the source's COM segment, or None
      'format'            what Pillow calls the file
      'keep'              True when open_image returns the opened image itself, so that Pillow still calls it a JPEG and
                          re-encodes with the file's own tables and sampling; False when it made a new image (an 'L' or 'RGBA'
                          file, an EXIF rotation) or Pillow calls the file something else ('MPO'): that one is saved with the
                          quality-85 tables and 4:2:0
      'quant', 'sampling' with keep and `data` (the file's bytes): [luma, chroma] and the sampling number for sampled_file,
                          from mdjpeg_parse; None when the saved form is not one sampled_file writes -- not exactly two tables
                          of 8-bit entries, table 0 for Y and table 1 for Cb and Cr, or a sampling other than 4:4:4, 4:2:2, 4:2:0.
    Raises what opening the file raises.
    """
    from .feed import open_for_coefficients
    image, rotation = open_for_coefficients(path)
    out = {'size': (image.size[1], image.size[0]) if rotation in (90, 270) else tuple(image.size), 'rotation': rotation,
           'exif': image.getexif().tobytes(), 'comment': image.info.get('comment'), 'format': image.format,
           'keep': image.format == 'JPEG' and image.mode not in ('RGBA', 'L') and rotation == 0, 'quant': None, 'sampling': None}
    if out['keep'] and data is not None:
        header = parse(data)
        tables = getattr(image, 'quantization', None) or {}
        if header.rc == MDJPEG_OK and sorted(tables) == [0, 1] and all(len(tables[k]) == 64 and 1 <= min(tables[k]) and max(tables[k]) <= 255
                                                                        for k in (0, 1)):
            ql, qc = (np.array(tables[k], dtype=np.uint16) for k in (0, 1))          # natural order, as JpegHeader.quant
            if header.components == 3 and (header.quant[0] == ql).all() and (header.quant[1] == qc).all() and (header.quant[2] == qc).all():
                out['sampling'] = sampling_of(header)
                out['quant'] = [ql, qc] if out['sampling'] is not None else None
    return out


def with_standard_tables(data):
    """
    The file for an abbreviated stream: Motion-JPEG frames usually carry no DHT segment, because the standard's example
    tables are implied.  Returns `data` itself when every Huffman table its first scan header names is defined in front of
    that header; otherwise bytes with ONE DHT segment inserted in front of SOS that defines the named tables which are
    missing -- id 0: the standard's luminance pair, id 1: its chrominance pair (the tables jfif_file writes).  This is
    libjpeg's rule, hence Pillow's (jinit_huff_decoder fills each of DC 0, AC 0, DC 1, AC 1 that is not defined, one by
    one, and nothing else): a scan that names a missing table 2 or 3, and bytes whose segments cannot be walked up to a
    scan header, come back unchanged and stay refused by everything that refused them.
    """
    buf = data if isinstance(data, bytes) else data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    n = len(buf)
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        return data
    defined, p = set(), 2
    while True:
        if p + 4 > n or buf[p] != 0xFF:
            return data
        m = buf[p + 1]
        if m == 0xFF:                                   # fill byte
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:              # TEM, RSTn, SOI: no length
            p += 2
            continue
        if m == 0xD9:
            return data
        ln = (buf[p + 2] << 8) | buf[p + 3]
        if ln < 2 or p + 2 + ln > n:
            return data
        if m == 0xC4:
            q, end = p + 4, p + 2 + ln
            while q + 17 <= end:
                defined.add(buf[q])
                q += 17 + sum(buf[q + 1:q + 17])
            if q != end:
                return data
        elif m == 0xDA:
            ns = buf[p + 4] if ln >= 3 else 0
            if not 1 <= ns <= 4 or ln < 6 + 2 * ns:
                return data
            named = set()
            for k in range(ns):
                sel = buf[p + 6 + 2 * k]
                named.update((sel >> 4, 0x10 | (sel & 15)))
            missing = named - defined
            if not missing:
                return data
            if any((t & 15) > 1 for t in missing):
                return data
            dht = b''.join(bytes((tc_th,)) + bytes(counts) + bytes(vals) for tc_th, counts, vals in _STD_HUFFMAN if tc_th in missing)
            return buf[:p] + _segment(0xC4, dht) + buf[p:]
        p += 2 + ln


def encode_bound(width, height):
    """bytes the scan of a width x height crop can take at the very most (mdjpeg_encode_bound)"""
    return int(load().mdjpeg_encode_bound(int(width), int(height)))


def encode_bound_sampled(width, height, sampling):
    """the same for a chroma sampling (mdjpeg_encode_sampled_bound): 0 = h1v1, 1 = h2v1, 2 = h2v2, as Pillow's `subsampling`"""
    return int(load().mdjpeg_encode_sampled_bound(int(width), int(height), int(sampling)))


def encode_subsequences(coefs, sizes, chunk_bytes=64, capacity=None, samplings=None):
    """
    The host model of the GPU entropy encoder (mdjpeg_encode_subsequences), for tests.  coefs: per crop a flat int16 array in
    the layout of decode() for 4:2:0; sizes: (width, height) per crop.  Returns (rc, scans, needed, buffer): the scans as
    bytes objects when rc == MDJPEG_OK.  capacity None: as much as the call needs (asked for first).
    samplings: per crop 0 = h1v1, 1 = h2v1, 2 = h2v2 (mdjpeg_encode_subsequences_sampled), coefs in that sampling's layout.
    """
    lib = load()
    n = len(coefs)
    hold = [np.ascontiguousarray(c, dtype=np.int16) for c in coefs]
    ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in hold])
    ws = (C.c_int32 * n)(*[int(s[0]) for s in sizes])
    hs = (C.c_int32 * n)(*[int(s[1]) for s in sizes])
    offs, lens, need = (C.c_int64 * n)(), (C.c_int64 * n)(), C.c_size_t(0)
    if samplings is None:
        call = lambda out, cap: lib.mdjpeg_encode_subsequences(ptrs, ws, hs, n, int(chunk_bytes), out, cap, offs, lens, C.byref(need))
    else:
        if len(samplings) != n:
            raise ValueError('one sampling per crop is needed')
        ss = (C.c_int32 * n)(*[int(v) for v in samplings])
        call = lambda out, cap: lib.mdjpeg_encode_subsequences_sampled(ptrs, ws, hs, ss, n, int(chunk_bytes), out, cap, offs, lens,
                                                                        C.byref(need))
    if capacity is None:
        rc = call(None, 0)
        if rc != MDJPEG_ECAPACITY:
            return rc, None, int(need.value), None
        capacity = int(need.value)
    guard = 64
    buf = np.full(capacity + guard, 0xA5, dtype=np.uint8)
    rc = call(buf.ctypes.data, capacity)
    if not (buf[capacity:] == 0xA5).all():
        raise AssertionError('mdjpeg_encode_subsequences wrote beyond its capacity')
    scans = [buf[offs[i]:offs[i] + lens[i]].tobytes() for i in range(n)] if rc == MDJPEG_OK else None
    return rc, scans, int(need.value), buf[:capacity]


def keep_merge(planes, source, size, sampling, rects):
    """
    The host model of mdhip_jpeg_encode_kept's merge for one window (mdjpeg_keep_merge).  planes: the re-encoded coefficients,
    a flat int16 array in the layout of decode() for `sampling`, changed IN PLACE; source: the source file's in the same
    layout; size: (width, height); rects: (left, top, right, bottom), right and bottom exclusive.  Every block of an MCU that
    no rectangle touches becomes the source's.  Returns the status: 1 when the merged planes hold a DC difference or an AC
    value no baseline scan codes (encode_subsequences refuses them), else 0.
    """
    if planes.dtype != np.int16 or not planes.flags.c_contiguous or not planes.flags.writeable:
        raise ValueError('planes must be a writeable contiguous int16 array')
    source = np.ascontiguousarray(source, dtype=np.int16)
    width, height = int(size[0]), int(size[1])
    if sampling not in SAMPLING_FACTORS:
        raise ValueError('sampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got {!r}'.format(sampling))
    hs, vs = SAMPLING_FACTORS[sampling]
    values = ((width + 8 * hs - 1) // (8 * hs)) * ((height + 8 * vs - 1) // (8 * vs)) * (hs * vs + 2) * 64
    if planes.size != values or source.size != values:
        raise ValueError('planes and source hold {} values each for {} x {} at sampling {}'.format(values, width, height, sampling))
    flat = np.ascontiguousarray(np.asarray(rects, dtype=np.int32).reshape(-1, 4))
    status = C.c_int32(0)
    rc = load().mdjpeg_keep_merge(planes.ctypes.data, source.ctypes.data, width, height, int(sampling),
                                  flat.ctypes.data_as(C.POINTER(C.c_int32)), len(flat), C.byref(status))
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_keep_merge failed ({})'.format(rc))
    return int(status.value)


def blur_regions(rgb, rects, radius, lds_bytes=None):
    """
    Pillow's GaussianBlur(radius) of rectangles of an H x W x 3 uint8 array, IN PLACE and in the order of the list
    (mdjpeg_blur_regions: the host model of the GPU blur and the host leg of blur=).  rects: (left, top, right, bottom),
    right / bottom exclusive; rows may be strided (a view of a wider array).  lds_bytes: cut the rows into the chunks a
    device with that much on-chip memory would (mdjpeg_blur_regions_chunked; same result).  Returns the library's code.
    """
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.strides[1:] != (3, 1) or not rgb.flags.writeable:
        raise ValueError('rgb must be a writeable H x W x 3 uint8 array with contiguous rows')
    n = len(rects)
    flat = (C.c_int32 * max(4 * n, 1))(*[int(v) for q in rects for v in q])
    h, w = rgb.shape[:2]
    pitch = rgb.strides[0] if h > 1 else w * 3
    lib = load()
    if lds_bytes is None:
        return lib.mdjpeg_blur_regions(rgb.ctypes.data, w, h, pitch, flat, n, float(radius))
    return lib.mdjpeg_blur_regions_chunked(rgb.ctypes.data, w, h, pitch, flat, n, float(radius), int(lds_bytes))


def _rgb_rows(rgb, writeable):
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.strides[1:] != (3, 1) or (writeable and not rgb.flags.writeable):
        raise ValueError('an H x W x 3 uint8 array with contiguous rows is needed{}'.format(' (writeable)' if writeable else ''))
    h, w = rgb.shape[:2]
    return w, h, rgb.strides[0] if h > 1 else w * 3


def resample_lanczos(rgb, size, out=None):
    """
    Pillow's Image.resize(size, LANCZOS) of an H x W x 3 uint8 array, bit for bit (mdjpeg_resample: the host model of the GPU
    resize).  size: (width, height); rows of `rgb` and of `out` may be strided (views of wider arrays).  Returns the new array.
    """
    w, h, pitch = _rgb_rows(rgb, False)
    dw, dh = int(size[0]), int(size[1])
    if out is None:
        out = np.empty((dh, dw, 3), np.uint8)
    ow, oh, opitch = _rgb_rows(out, True)
    if (ow, oh) != (dw, dh):
        raise ValueError('out is {} x {}, not {} x {}'.format(ow, oh, dw, dh))
    rc = load().mdjpeg_resample(rgb.ctypes.data, w, h, pitch, out.ctypes.data, dw, dh, opitch)
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_resample returned {} for {} x {} -> {} x {}'.format(rc, w, h, dw, dh))
    return out


def draw_ops(rgb, ops, patches=b''):
    """
    Applies drawing operations (rows of 8 int32: include/mdhip.h mdhip_draw_ops) to an H x W x 3 uint8 array IN PLACE
    (mdjpeg_draw: the host model of the GPU drawing).  patches: the bytes the patch operations point into.  Returns the
    library's code.
    """
    w, h, pitch = _rgb_rows(rgb, True)
    flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 8))
    pbuf = np.frombuffer(bytes(patches), np.uint8) if not isinstance(patches, np.ndarray) else np.ascontiguousarray(patches, np.uint8)
    return load().mdjpeg_draw(rgb.ctypes.data, w, h, pitch, flat.ctypes.data_as(C.POINTER(C.c_int32)), len(flat),
                              pbuf.ctypes.data if pbuf.size else None, pbuf.size)


def draw_ops_from(src_ptrs, sizes, src_pitches, dst_ptrs, dst_src, dst_pitches, op_image, ops, patches=b''):
    """
    The fan-out draw on host memory (mdjpeg_draw_from: the host model of mdhip_draw_ops_from), with the arguments of
    hip_backend's draw_ops_from: ADDRESSES of the sources (with their (width, height) and bytes a row) and of the destinations
    (each with the index of its source and its bytes a row), the destination of every operation and the operations' rows
    of 8 int32.  The caller keeps the memory alive.  patches: the bytes the patch operations point into.  Returns the
    library's code.
    """
    n, k = len(src_ptrs), len(dst_ptrs)
    flat = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 8))
    oi = np.ascontiguousarray(np.asarray(op_image, dtype=np.int32).reshape(-1))
    if not (len(sizes) == len(src_pitches) == n) or not (len(dst_src) == len(dst_pitches) == k) or len(oi) != len(flat):
        raise ValueError('one entry per source, per destination and per operation is needed in their lists')
    pbuf = np.frombuffer(bytes(patches), np.uint8) if not isinstance(patches, np.ndarray) else np.ascontiguousarray(patches, np.uint8)
    i32 = C.POINTER(C.c_int32)
    return load().mdjpeg_draw_from((C.c_void_p * max(n, 1))(*[int(v) for v in src_ptrs]), (C.c_int32 * max(n, 1))(*[int(s[0]) for s in sizes]),
                                   (C.c_int32 * max(n, 1))(*[int(s[1]) for s in sizes]), (C.c_int64 * max(n, 1))(*[int(v) for v in src_pitches]), n,
                                   (C.c_void_p * max(k, 1))(*[int(v) for v in dst_ptrs]), (C.c_int32 * max(k, 1))(*[int(v) for v in dst_src]),
                                   (C.c_int64 * max(k, 1))(*[int(v) for v in dst_pitches]), k, oi.ctypes.data_as(i32), flat.ctypes.data_as(i32),
                                   len(flat), pbuf.ctypes.data if pbuf.size else None, pbuf.size)


def classifier_input(rgb, canvas, size, filter=0, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """
    The classifier input of one crop (mdjpeg_classifier_input: the host model of the GPU call): rgb, an H x W x 3 uint8 array
    whose rows may be strided, is the part of a canvas (canvas_w, canvas_h, off_x, off_y) that holds pixels; the rest of the
    canvas is 0.  Returns float32 [3][size][size], or raises ValueError with the library's code.
    """
    w, h, pitch = _rgb_rows(rgb, False)
    cw, ch, ox, oy = (int(v) for v in canvas)
    out = np.empty((3, int(size), int(size)), np.float32)
    rc = load().mdjpeg_classifier_input(rgb.ctypes.data, pitch, w, h, cw, ch, ox, oy, int(size), int(filter),
                                        (C.c_float * 3)(*mean), (C.c_float * 3)(*std), out.ctypes.data)
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_classifier_input returned {} for {} x {} in a canvas of {} x {} at size {}'.format(rc, w, h, cw, ch, size))
    return out


def thumbnails(tiles, filter=0):
    """
    Tiles into sheets (mdjpeg_thumbnails: the host model of HipContext.thumbnails): Pillow's image.crop(box).resize((out_w,
    out_h)) + sheet.paste(tile, (x, y)), bit for bit.  tiles: (rgb, canvas, sheet, x, y, out_w, out_h) each -- rgb, an H x W x 3
    uint8 array whose rows may be strided, is the part of the canvas (canvas_w, canvas_h, off_x, off_y) that holds pixels;
    sheet, a writeable H x W x 3 uint8 array, gets the tile at (x, y), which must lie inside it.  All or nothing: raises
    ValueError for an argument the library refuses, returns False when it answers MDJPEG_EUNSUPPORTED (the sizes the GPU call
    refuses), else True.
    """
    recs = (mdjpeg_thumbnail * max(len(tiles), 1))()
    for r, (rgb, canvas, sheet, x, y, out_w, out_h) in zip(recs, tiles):
        # (rgb None or without pixels: the canvas holds no image pixel -- a box wholly outside its image)
        src, (w, h, pitch) = (0, (0, 0, 0)) if rgb is None or rgb.size == 0 else (rgb.ctypes.data, _rgb_rows(rgb, False))
        sw, sh, spitch = _rgb_rows(sheet, True)
        x, y, out_w, out_h = int(x), int(y), int(out_w), int(out_h)
        if x < 0 or y < 0 or out_w < 1 or out_h < 1 or x + out_w > sw or y + out_h > sh:
            raise ValueError('a tile of {} x {} at ({}, {}) leaves its sheet of {} x {}'.format(out_w, out_h, x, y, sw, sh))
        cw, ch, ox, oy = (int(v) for v in canvas)
        r.src, r.pitch, r.src_w, r.src_h = src, pitch, w, h
        r.canvas_w, r.canvas_h, r.off_x, r.off_y = cw, ch, ox, oy
        r.out_w, r.out_h, r.dst, r.dst_pitch = out_w, out_h, sheet.ctypes.data + y * spitch + x * 3, spitch
    rc = load().mdjpeg_thumbnails(recs, len(tiles), int(filter))
    if rc == MDJPEG_EUNSUPPORTED:
        return False
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_thumbnails returned {}'.format(rc))
    return True


def change_options(blur_kernel_size=21, threshold_type=0, threshold=25, dilate_kernel_size=5, dilate_iterations=2, min_area=500,
                   ignore_fraction=None, region_cap=256):
    """the option record of mdjpeg_change_detect / mdhip_change_detect (threshold_type: 0 GLOBAL, 1 OTSU)"""
    return mdjpeg_change_options(int(blur_kernel_size), int(threshold_type), int(threshold), int(dilate_kernel_size), int(dilate_iterations),
                                 int(min_area), 0 if ignore_fraction is None else 1, int(region_cap),
                                 0.0 if ignore_fraction is None else float(ignore_fraction))


class ChangeArrays:
    """the host arrays both change-detection calls fill, and what is read out of them: per pair `counts`, `hist` (256),
    `thresholds`, `n_regions`, `regions` (cap x 5: x, y, w, h, area), `overflow`"""

    def __init__(self, n_pairs, cap):
        n = max(int(n_pairs), 1)
        self.counts = np.zeros(n, np.int64)
        self.hist = np.zeros((n, 256), np.uint32)
        self.thresholds = np.zeros(n, np.int32)
        self.n_regions = np.zeros(n, np.int32)
        self.regions = np.zeros((n, max(int(cap), 1), 5), np.int32)
        self.overflow = np.zeros(n, np.uint8)

    def pointers(self):
        return [a.ctypes.data for a in (self.counts, self.hist, self.thresholds, self.n_regions, self.regions, self.overflow)]

    def result(self, n_pairs, cap):
        return {'counts': self.counts[:n_pairs], 'hist': self.hist[:n_pairs], 'thresholds': self.thresholds[:n_pairs],
                'n_regions': self.n_regions[:n_pairs], 'regions': self.regions[:n_pairs, :cap], 'overflow': self.overflow[:n_pairs]}


def change_detect(images, pairs, options, blurred=None, want_masks=False):
    """mdjpeg_change_detect: images: per image an (h, w, 3) uint8 array, or None where blurred[i] is given; pairs: (previous,
    current) indices; options: change_options(); blurred: None, or per image None or its (h, w) uint8 blurred gray plane of an
    earlier call.  -> the ChangeArrays result plus 'blurred' (per image its plane) and 'masks' (per pair the dilated mask, or
    None).  ValueError for what the call refuses."""
    n, m = len(images), len(pairs)
    blurred = list(blurred) if blurred is not None else [None] * n
    ready = np.array([b is not None for b in blurred], np.uint8)
    rgb, sizes = [], []
    for i in range(n):
        if ready[i]:
            blurred[i] = np.ascontiguousarray(blurred[i], np.uint8)
            rgb.append(None)
            sizes.append((blurred[i].shape[1], blurred[i].shape[0]))
        else:
            a = np.ascontiguousarray(images[i], np.uint8)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError('image {}: an (h, w, 3) array is needed'.format(i))
            rgb.append(a)
            sizes.append((a.shape[1], a.shape[0]))
            blurred[i] = np.zeros((a.shape[0], a.shape[1]), np.uint8)
    pair_arr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    for a, b in pair_arr:
        if not (0 <= a < n and 0 <= b < n) or sizes[a] != sizes[b]:
            raise ValueError('a pair names no image, or two images of different sizes')
    masks = [np.zeros((sizes[a][1], sizes[a][0]), np.uint8) for a, _ in pair_arr] if want_masks else None
    out = ChangeArrays(m, options.region_cap)
    rc = load().mdjpeg_change_detect(
        (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in rgb]), (C.c_int32 * max(n, 1))(*[s[0] for s in sizes]),
        (C.c_int32 * max(n, 1))(*[s[1] for s in sizes]), (C.c_int64 * max(n, 1))(*[3 * s[0] for s in sizes]), n,
        (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in blurred]), ready.ctypes.data, pair_arr.ctypes.data, m, C.addressof(options),
        *out.pointers(), (C.c_void_p * max(m, 1))(*[k.ctypes.data for k in masks]) if want_masks else None)
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_change_detect refused its arguments ({})'.format(rc))
    res = out.result(m, options.region_cap)
    res['blurred'], res['masks'] = blurred, masks
    return res


def gray_count(images, windows=None, walk=False):
    """mdjpeg_gray_count (walk: mdjpeg_gray_count_walk, the kernel's walk of a row): images: per image an (h, w, 3) uint8 array whose
    pixels are 3 adjacent bytes -- any base address, any bytes a row (a view with strides (pitch, 3, 1) is taken as it lies);
    windows: None for the whole images, or per image (x, y, w, h).  -> per image the number of pixels of its window with
    R == G and R == B, as Python ints.  ValueError for what the call refuses."""
    n = len(images)
    for i, a in enumerate(images):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.strides[1:] != (3, 1) or (a.shape[0] > 1 and a.strides[0] < 3 * a.shape[1]):
            raise ValueError('image {}: an (h, w, 3) uint8 array with 3 adjacent bytes a pixel is needed'.format(i))
    if windows is None:
        windows = [(0, 0, a.shape[1], a.shape[0]) for a in images]
    if len(windows) != n:
        raise ValueError('one window per image is needed')
    win = np.ascontiguousarray(np.asarray(windows, np.int32).reshape(-1, 4))
    counts = np.zeros(max(n, 1), np.uint64)
    call = load().mdjpeg_gray_count_walk if walk else load().mdjpeg_gray_count
    rc = call((C.c_void_p * max(n, 1))(*[a.ctypes.data for a in images]), (C.c_int32 * max(n, 1))(*[a.shape[1] for a in images]),
              (C.c_int32 * max(n, 1))(*[a.shape[0] for a in images]),
              (C.c_int64 * max(n, 1))(*[a.strides[0] if a.shape[0] > 1 else 3 * a.shape[1] for a in images]), win.ctypes.data, n,
              counts.ctypes.data)
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_gray_count refused its arguments ({})'.format(rc))
    return [int(v) for v in counts[:n]]


def classifier_plan(canvas_w, canvas_h, size, filter=0, lds_bytes=0):
    """(output columns, output rows) a workgroup of the GPU call takes of a crop of this canvas, or None when the call
    refuses it with MDHIP_EUNSUPPORTED (mdjpeg_classifier_plan; lds_bytes 0: what the device has)"""
    plan = (C.c_int32 * 2)()
    rc = load().mdjpeg_classifier_plan(int(canvas_w), int(canvas_h), int(size), int(filter), int(lds_bytes), plan)
    if rc == MDJPEG_EUNSUPPORTED:
        return None
    if rc != MDJPEG_OK:
        raise ValueError('mdjpeg_classifier_plan returned {}'.format(rc))
    return plan[0], plan[1]


def blur_weights(radius):
    """(r, ww, fw) of Pillow's extended box filter for a Gaussian radius (mdjpeg_blur_weights)"""
    r, ww, fw = C.c_int32(0), C.c_uint32(0), C.c_uint32(0)
    rc = load().mdjpeg_blur_weights(float(radius), C.byref(r), C.byref(ww), C.byref(fw))
    if rc != MDJPEG_OK:
        raise ValueError('radius {!r} is outside 0 .. 512'.format(radius))
    return int(r.value), int(ww.value), int(fw.value)


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
