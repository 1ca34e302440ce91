"""
ctypes binding of libmdhip.so (C ABI: include/mdhip.h).

There is NO CPU fallback: if the shared library is missing or no HIP device is visible the
product path raises.  (The CPU restatement under oracle/ is test infrastructure only.)
"""

import ctypes as C
import os

import numpy as np

from .jpeg_host import mdjpeg_change_options

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmdhip.so')

MDHIP_OK = 0
MDHIP_EINVAL = -1
MDHIP_ECAPACITY = -5
MDHIP_EUNSUPPORTED = -4
MDHIP_DTYPE_BF16 = 0
MDHIP_DTYPE_FP8 = 1
MDHIP_DTYPE_FP16 = 2
#: flags of mdhip_launches_describe
MDHIP_LAUNCHES_NO_FUSE, MDHIP_LAUNCHES_NO_FUSE_DECODE, MDHIP_LAUNCHES_NO_PAIR, MDHIP_LAUNCHES_ISOLATED = 1, 2, 4, 8
MDHIP_LAUNCHES_CALIBRATING, MDHIP_LAUNCHES_AUGMENTED, MDHIP_LAUNCHES_AFTER_OTHERS, MDHIP_LAUNCHES_NO_PW_STREAM = 16, 32, 64, 128


class mdhip_conv(C.Structure):
    _fields_ = [('weight', C.POINTER(C.c_float)), ('bias', C.POINTER(C.c_float)),
                ('c_out', C.c_int32), ('c_in', C.c_int32), ('kh', C.c_int32), ('kw', C.c_int32)]


class mdhip_layer(C.Structure):
    _fields_ = [('type', C.c_int32), ('n_from', C.c_int32), ('from_', C.c_int32 * 4),
                ('c_out', C.c_int32), ('k', C.c_int32), ('s', C.c_int32), ('p', C.c_int32),
                ('n', C.c_int32), ('shortcut', C.c_int32), ('first_conv', C.c_int32)]


class mdhip_model(C.Structure):
    _fields_ = [('n_layers', C.c_int32), ('layers', C.POINTER(mdhip_layer)),
                ('n_convs', C.c_int32), ('convs', C.POINTER(mdhip_conv)),
                ('nc', C.c_int32), ('na', C.c_int32), ('nl', C.c_int32),
                ('anchors_px', C.POINTER(C.c_float)), ('strides', C.POINTER(C.c_float))]


class mdhip_letterbox(C.Structure):
    _fields_ = [('src_h', C.c_int32), ('src_w', C.c_int32), ('resized_h', C.c_int32),
                ('resized_w', C.c_int32), ('top', C.c_int32), ('left', C.c_int32), ('interp', C.c_int32)]


class mdhip_jpeg_image(C.Structure):
    _fields_ = [('coef', C.c_void_p), ('width', C.c_int32), ('height', C.c_int32), ('components', C.c_int32),
                ('h_samp', C.c_int32), ('v_samp', C.c_int32), ('blocks_w', C.c_int32 * 3), ('blocks_h', C.c_int32 * 3),
                ('rotation', C.c_int32), ('quant', (C.c_uint16 * 64) * 3)]


class mdhip_jpeg_source(C.Structure):
    _fields_ = [('coef', C.c_void_p), ('blocks_w', C.c_int32 * 3), ('blocks_h', C.c_int32 * 3)]


class mdhip_jpeg_scan(C.Structure):
    _fields_ = [('scan', C.c_void_p), ('desc', C.c_void_p), ('seg_offsets', C.c_void_p), ('coef', C.c_void_p)]


class mdhip_classifier_crop(C.Structure):
    _fields_ = [('src', C.c_void_p), ('pitch', C.c_int64), ('src_w', C.c_int32), ('src_h', C.c_int32),
                ('canvas_w', C.c_int32), ('canvas_h', C.c_int32), ('off_x', C.c_int32), ('off_y', C.c_int32)]


class mdhip_thumbnail(C.Structure):
    _fields_ = [('src', C.c_void_p), ('pitch', C.c_int64), ('src_w', C.c_int32), ('src_h', C.c_int32),
                ('canvas_w', C.c_int32), ('canvas_h', C.c_int32), ('off_x', C.c_int32), ('off_y', C.c_int32),
                ('out_w', C.c_int32), ('out_h', C.c_int32), ('dst', C.c_void_p), ('dst_pitch', C.c_int64)]


class mdhip_rde_box(C.Structure):
    _fields_ = [('x', C.c_double), ('y', C.c_double), ('w', C.c_double), ('h', C.c_double),
                ('group', C.c_int32), ('category', C.c_int32)]


mdhip_change_options = mdjpeg_change_options      # the header's typedef


class mdhip_op_info(C.Structure):
    _fields_ = [('name', C.c_char * 48), ('kind', C.c_int32), ('layer', C.c_int32),
                ('m', C.c_int32), ('n', C.c_int32), ('k', C.c_int32),
                ('flops', C.c_double), ('bytes', C.c_double), ('cfg', C.c_int32),
                ('ntaps', C.c_int32), ('stride', C.c_int32), ('has_res', C.c_int32), ('variant', C.c_int32)]


class mdhip_tuned(C.Structure):
    _fields_ = [('m', C.c_int32), ('n', C.c_int32), ('k', C.c_int32), ('ntaps', C.c_int32),
                ('stride', C.c_int32), ('has_res', C.c_int32), ('cfg', C.c_int32), ('batch', C.c_int32)]


#: every symbol include/mdhip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    'mdhip_create': (C.c_int, [C.POINTER(mdhip_model), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    'mdhip_create_images': (C.c_int, [C.c_int, C.POINTER(_P)]),
    'mdhip_destroy': (None, [_P]),
    'mdhip_last_error': (C.c_char_p, [_P]),
    'mdhip_preprocess': (C.c_int, [_P, C.POINTER(_P), C.POINTER(mdhip_letterbox), C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_preprocess_windows': (C.c_int, [_P, C.POINTER(_P), C.POINTER(mdhip_letterbox), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_forward': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_jpeg_reconstruct': (C.c_int, [_P, C.POINTER(mdhip_jpeg_image), C.c_int, C.POINTER(_P), _P]),
    'mdhip_jpeg_entropy_decode': (C.c_int, [_P, C.POINTER(mdhip_jpeg_scan), C.c_int, C.c_int, C.POINTER(C.c_int32), _P]),
    'mdhip_jpeg_entropy_stats': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    'mdhip_jpeg_recompress': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                        C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(_P), _P]),
    'mdhip_jpeg_encode': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                    C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), _P, C.c_int64, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    'mdhip_jpeg_encode_bound': (C.c_longlong, [C.c_int, C.c_int]),
    'mdhip_jpeg_encode_sampled': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint16), _P, C.c_int64, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    'mdhip_jpeg_encode_sampled_bound': (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    'mdhip_jpeg_encode_kept': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_uint16), C.POINTER(mdhip_jpeg_source),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, _P, C.c_int64, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), _P]),
    'mdhip_blur_regions': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_float, _P]),
    'mdhip_resample_lanczos': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                         C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), _P]),
    'mdhip_draw_ops': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, _P, C.c_int64, _P]),
    'mdhip_draw_ops_from': (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                      C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, _P, C.c_int64, _P]),
    'mdhip_classifier_input': (C.c_int, [_P, C.POINTER(mdhip_classifier_crop), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), _P, _P]),
    'mdhip_thumbnails': (C.c_int, [_P, C.POINTER(mdhip_thumbnail), C.c_int, C.c_int, _P]),
    'mdhip_repeat_detections': (C.c_int, [C.c_int, _P, C.c_int64, C.c_double, C.c_int, C.c_int32, C.c_int32, _P, _P, _P, C.c_int64,
                                          C.POINTER(C.c_int64)]),
    'mdhip_repeat_detections_times': (C.c_int, [C.POINTER(C.c_float)]),
    'mdhip_change_detect': (C.c_int, [_P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.POINTER(mdhip_change_options), _P, _P, _P, _P, _P,
                                      _P, _P, _P]),
    'mdhip_label_regions_on': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    'mdhip_gray_count': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _P, _P]),
    'mdhip_forward_tta': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_last_num_anchors': (C.c_int, [_P]),
    'mdhip_calibrate': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_fp8_num_tensors': (C.c_int, [_P]),
    'mdhip_fp8_get_scales': (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    'mdhip_fp8_set_scales': (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    'mdhip_f32_to_e4m3': (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_int]),
    'mdhip_nms': (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P]),
    'mdhip_nms_enqueue': (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, _P]),
    'mdhip_nms_wait': (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_int32))]),
    'mdhip_nms_on': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P, _P, _P]),
    'mdhip_num_anchors': (C.c_int, [_P, C.c_int, C.c_int]),
    'mdhip_max_stride': (C.c_int, [_P]),
    'mdhip_read_predictions': (C.c_int, [_P, C.c_int, _P, _P]),
    'mdhip_read_input': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    'mdhip_read_layer': (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    'mdhip_run_ops': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_read_op_tensor': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    'mdhip_read_op_weights': (C.c_int, [_P, C.c_int, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    'mdhip_dwconv3x3_on': (C.c_int, [_P, _P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, _P]),
    'mdhip_attention_on': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_dfl_decode_on': (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P]),
    'mdhip_adown_pool_on': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_cbfuse_on': (C.c_int, [_P, _P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    'mdhip_tta_input_on': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    'mdhip_plan_describe': (C.c_longlong, [C.POINTER(mdhip_model), C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    'mdhip_launches_describe': (C.c_longlong, [C.POINTER(mdhip_model), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(mdhip_tuned),
                                               C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_int32), C.c_int,
                                               C.c_char_p, C.c_size_t]),
    'mdhip_num_ops': (C.c_int, [_P]),
    'mdhip_get_op_info': (C.c_int, [_P, C.c_int, C.POINTER(mdhip_op_info)]),
    'mdhip_forward_timed': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P]),
    'mdhip_time_forwards': (C.c_int, [_P, C.c_int]),
    'mdhip_forward_times': (C.c_int, [_P, _P, C.c_int]),
    'mdhip_set_op_cfg': (C.c_int, [_P, C.c_int, C.c_int]),
    'mdhip_num_conv_cfgs': (C.c_int, []),
    'mdhip_op_supports_cfg': (C.c_int, [_P, C.c_int, C.c_int]),
    'mdhip_cfg_is_bitwise': (C.c_int, [C.c_int]),
    'mdhip_conv_cfg_name': (C.c_char_p, [C.c_int]),
    'mdhip_set_tuned': (C.c_int, [_P, C.POINTER(mdhip_tuned), C.c_int]),
    'mdhip_set_fuse': (C.c_int, [_P, C.c_int]),
    'mdhip_set_graph': (C.c_int, [_P, C.c_int, C.c_int]),
    'mdhip_set_option': (C.c_int, [_P, C.c_char_p, C.c_int]),
    'mdhip_time_op': (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), _P]),
    'mdhip_version': (C.c_char_p, []),
}

_lib = None


def load():
    """Loads libmdhip.so (once).  Raises RuntimeError when the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'libmdhip.so not found at {}: build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` or `make -C megadetector_amd/csrc`. There is no CPU fallback.'.format(LIB_PATH))
    # torch bundles its own libamdhip64.so.7; importing it first makes the process use ONE HIP
    # runtime (ours resolves the already-loaded SONAME).
    if os.environ.get('MDHIP_NO_TORCH_PRELOAD', '0') != '1':
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class HipError(RuntimeError):
    pass
