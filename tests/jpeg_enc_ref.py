"""
NumPy restatement of the lossy half of baseline JPEG ENCODING as libjpeg-turbo (and so Pillow's Image.save) performs it
for RGB input with default settings: three components, 4:2:0.  The CPU oracle of mdhip_jpeg_recompress; pinned against
Pillow by tests/test_tile_jpeg_cpu.py, coefficient by coefficient.  Composed with tests/jpeg_ref.py it is the whole round
trip Image.save(quality=q) -> Image.open -> RGB.  Integer arithmetic throughout:

  * colour: the 16-bit fixed-point RGB -> YCbCr tables (jccolor.c), rounding constants included;
  * edges: the right edge is replicated PIXEL-wise to whole blocks of each component (twice as far for chroma, before the
    down-sampling); below the image, luma repeats its last row and chroma repeats its last DOWN-SAMPLED row;
  * chroma: h2v2 box down-sampling with the bias alternating 1, 2 along a row (jcsample.c);
  * forward DCT: jfdctint "islow" on samples - 128: rows then columns, 13-bit constants, PASS1_BITS 2, output scaled by 8;
  * quantisation: division by 8 * table entry, rounded half away from zero;
  * blocks that only fill up an MCU (right of / below a component's own blocks) hold the DC of the previous block of
    the MCU and no AC (jccoefct.c): they are part of the file, though no decoded pixel depends on them.
"""

import numpy as np

import jpeg_ref
from megadetector_amd.jpeg_host import quant_tables

CONST_BITS, PASS1_BITS = 13, 2


def rgb_to_ycc(rgb):
    """H x W x 3 uint8 -> (y, cb, cr) int64"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_right(a, width):
    return a if a.shape[1] >= width else np.concatenate([a, np.repeat(a[:, -1:], width - a.shape[1], axis=1)], axis=1)


def _pad_bottom(a, height):
    return a if a.shape[0] >= height else np.concatenate([a, np.repeat(a[-1:], height - a.shape[0], axis=0)], axis=0)


def component_planes(rgb):
    """the samples the forward DCT reads: [Y, Cb, Cr], each a whole number of 8 x 8 blocks of the component's own size"""
    H, W = rgb.shape[:2]
    y, cb, cr = rgb_to_ycc(rgb)
    bw_y, bh_y = -(-W // 8), -(-H // 8)
    cw, ch = -(-W // 2), -(-H // 2)
    bw_c, bh_c = -(-cw // 8), -(-ch // 8)
    planes = [_pad_bottom(_pad_right(y, bw_y * 8), bh_y * 8)]
    bias = np.tile(np.array([1, 2], dtype=np.int64), bw_c * 4)[None, :]
    for c in (cb, cr):
        c = _pad_bottom(_pad_right(c, bw_c * 16), ch * 2)             # input rows: the last one once more when H is odd
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        planes.append(_pad_bottom((s + bias) >> 2, bh_c * 8))
    return planes


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one 1-D pass of jpeg_fdct_islow over the first axis of d (8 x ...)"""
    tmp0, tmp7 = d[0] + d[7], d[0] - d[7]
    tmp1, tmp6 = d[1] + d[6], d[1] - d[6]
    tmp2, tmp5 = d[2] + d[5], d[2] - d[5]
    tmp3, tmp4 = d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        o0, o4 = (tmp10 + tmp11) << PASS1_BITS, (tmp10 - tmp11) << PASS1_BITS
    else:
        o0, o4 = _descale(tmp10 + tmp11, PASS1_BITS), _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * 4433
    o2 = _descale(z1 + tmp13 * 6270, n)
    o6 = _descale(z1 + tmp12 * (-15137), n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2 = z1 * (-7373), z2 * (-20995)
    z3, z4 = z3 * (-16069) + z5, z4 * (-3196) + z5
    return np.stack([o0, _descale(tmp7 + z1 + z4, n), o2, _descale(tmp6 + z2 + z3, n),
                     o4, _descale(tmp5 + z2 + z4, n), o6, _descale(tmp4 + z1 + z3, n)])


def fdct_quantise(plane, quant):
    """plane: [bh * 8][bw * 8] samples, quant: [64] natural order -> [bh][bw][64] quantised coefficients (int64)"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.astype(np.int64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128      # [bh][bw][row y][column x]
    ws = _fdct_pass(np.moveaxis(d, 3, 0), True)                       # rows: over x -> [u][bh][bw][y]
    co = _fdct_pass(np.moveaxis(ws, 3, 0), False)                     # columns: over y -> [v][u][bh][bw]
    co = co.transpose(2, 3, 0, 1).reshape(bh, bw, 64)                 # natural order: v * 8 + u
    div = quant.astype(np.int64)[None, None, :] * 8
    q = (np.abs(co) + (div >> 1)) // div
    return np.where(co < 0, -q, q)


def _fill_mcus(co, mcus_x, mcus_y, hs, vs):
    """[bh][bw][64] of the component's own blocks -> [mcus_y * vs][mcus_x * hs][64] with libjpeg's dummy blocks"""
    bh, bw = co.shape[:2]
    out = np.zeros((mcus_y * vs, mcus_x * hs, 64), dtype=np.int64)
    out[:bh, :bw] = co
    for by in range(bh):                                              # right edge: DC of the block to the left
        for bx in range(bw, mcus_x * hs):
            out[by, bx, 0] = out[by, bx - 1, 0]
    for by in range(bh, mcus_y * vs):                                 # bottom edge: DC of the MCU's block before this row
        for m in range(mcus_x):
            out[by, m * hs:(m + 1) * hs, 0] = out[by - 1, (m + 1) * hs - 1, 0]
    return out


class EncodedImage:
    """what jpeg_ref.jpeg_ref reads of a jpeg_host.JpegHeader, for coefficients that never were a file"""

    components = 3
    h_samp, v_samp = (2, 1, 1), (2, 1, 1)

    def __init__(self, width, height, quant, planes):
        self.width, self.height = width, height
        self.quant = quant                                            # [3][64] uint16, natural order
        self._planes = planes
        self.blocks_w = tuple(p.shape[1] for p in planes)
        self.blocks_h = tuple(p.shape[0] for p in planes)

    def planes(self, coef=None):
        return self._planes


def encode(rgb, quality):
    """H x W x 3 uint8 -> EncodedImage: the quantised coefficients Image.save(quality=quality) puts into the file"""
    rgb = np.asarray(rgb)
    assert rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.dtype == np.uint8
    H, W = rgb.shape[:2]
    ql, qc = quant_tables(quality)
    quant = np.stack([ql, qc, qc]).astype(np.uint16)
    mcus_x, mcus_y = -(-W // 16), -(-H // 16)
    planes = []
    for c, p in enumerate(component_planes(rgb)):
        s = 2 if c == 0 else 1
        planes.append(_fill_mcus(fdct_quantise(p, quant[c]), mcus_x, mcus_y, s, s).astype(np.int16))
    return EncodedImage(W, H, quant, planes)


def recompress(rgb, quality):
    """np.asarray(Image.open(<Image.fromarray(rgb).save(quality=quality)>).convert('RGB')), without Pillow"""
    return jpeg_ref.jpeg_ref(encode(rgb, quality), None)
