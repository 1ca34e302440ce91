"""
NumPy restatement of the second half of baseline JPEG decoding as libjpeg-turbo (and so Pillow) performs it: the CPU
oracle of mdhip_jpeg_reconstruct, itself pinned against Pillow by tests/test_jpeg_cpu.py.

Input: the quantised coefficient planes of megadetector_amd.jpeg_host.decode.  Output: the H x W x 3 uint8 RGB pixels of
np.asarray(feed.load_image(file)).  Integer arithmetic throughout (int64 here; nothing leaves 32 bits on legal data):

  * IDCT: libjpeg's jidctint "islow" -- de-quantise, columns then rows with 13-bit constants, rounding right shifts by
    11 and 18, and SATURATION of value + 128 to 0 .. 255.  libjpeg's C code indexes a range-limit table with
    (value & 1023) instead: the same for values in [-512, 511], a wrap-around outside.  libjpeg-turbo's SIMD inverse
    DCT packs with saturation, and that is what Pillow's pixels show; a block inside the energy bound of mdjpeg_decode
    can reach +-2800, so the two differ on files the decoders accept (tests/test_jpeg_foreign_cpu.py has the probe);
  * chroma: "fancy" triangle upsampling (h2v1 / h2v2) over the component's downsampled width and height -- not over the
    block-padded plane -- with the nearest real row repeated above the first and below the last; components of at most
    two columns are replicated instead (libjpeg's rule);
  * colour: the 16-bit fixed-point YCbCr -> RGB tables; grayscale R = G = B = Y;
  * rotation: EXIF angles as PIL's rotate(angle, expand=True) turns them (counter-clockwise).
"""

import numpy as np

CONST_BITS, PASS1_BITS = 13, 2
F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865 = 2446, 3196, 4433, 6270
F_0_899976223, F_1_175875602, F_1_501321110, F_1_847759065 = 7373, 9633, 12299, 15137
F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 16069, 16819, 20995, 25172


def range_limit(x):
    """post-IDCT range limit, x = sample - 128: saturation (see the module's text)"""
    return np.clip(x + 128, 0, 255)


def range_limit_table(x):
    """libjpeg's C form, which this project does NOT follow: its table (jdmaster.c prepare_range_limit_table) indexed by
    (x & 1023).  Equal to range_limit inside [-512, 511], wrapping around outside.  Kept for the probe test that states
    which of the two the installed Pillow shows."""
    t = np.zeros(1024, dtype=np.int64)
    t[0:128] = np.arange(128, 256)
    t[128:512] = 255
    t[512:896] = 0
    t[896:1024] = np.arange(0, 128)
    return t[x & 1023]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, shift):
    """one 1-D pass of jpeg_idct_islow over the first axis of d (8 x ...), results descaled by `shift`"""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * F_0_541196100
    tmp2 = z1 + z3 * (-F_1_847759065)
    tmp3 = z1 + z2 * F_0_765366865
    z2, z3 = d[0], d[4]
    tmp0 = (z2 + z3) << CONST_BITS
    tmp1 = (z2 - z3) << CONST_BITS
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175875602
    tmp0 = tmp0 * F_0_298631336
    tmp1 = tmp1 * F_2_053119869
    tmp2 = tmp2 * F_3_072711026
    tmp3 = tmp3 * F_1_501321110
    z1 = z1 * (-F_0_899976223)
    z2 = z2 * (-F_2_562915447)
    z3 = z3 * (-F_1_961570560) + z5
    z4 = z4 * (-F_0_390180644) + z5
    tmp0 = tmp0 + z1 + z3
    tmp1 = tmp1 + z2 + z4
    tmp2 = tmp2 + z2 + z3
    tmp3 = tmp3 + z1 + z4
    return np.stack([_descale(tmp10 + tmp3, shift), _descale(tmp11 + tmp2, shift), _descale(tmp12 + tmp1, shift),
                     _descale(tmp13 + tmp0, shift), _descale(tmp13 - tmp0, shift), _descale(tmp12 - tmp1, shift),
                     _descale(tmp11 - tmp2, shift), _descale(tmp10 - tmp3, shift)])


def idct_plane(plane, quant, limit=range_limit):
    """plane: [bh][bw][64] int16 quantised, quant: [64] -> [bh * 8][bw * 8] samples (int64 in 0 .. 255)"""
    bh, bw = plane.shape[:2]
    d = plane.astype(np.int64) * quant.astype(np.int64)[None, None, :]
    d = d.reshape(bh, bw, 8, 8)                                       # [.., row v, column u]
    ws = _pass(np.moveaxis(d, 2, 0), CONST_BITS - PASS1_BITS)         # columns: over v -> [y][bh][bw][u]
    out = _pass(np.moveaxis(ws, 3, 0), CONST_BITS + PASS1_BITS + 3)   # rows: over u -> [x][y][bh][bw]
    out = limit(out)
    return out.transpose(2, 1, 3, 0).reshape(bh * 8, bw * 8)


def upsample_h2(a):
    """h2v1 fancy upsampling of the columns of a [rows][w] -> [rows][2 w]"""
    w = a.shape[1]
    if w <= 2:
        return np.repeat(a, 2, axis=1)
    left = np.concatenate([a[:, :1], a[:, :-1]], axis=1)
    right = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)
    out = np.empty((a.shape[0], 2 * w), dtype=np.int64)
    out[:, 0::2] = (3 * a + left + 1) >> 2
    out[:, 1::2] = (3 * a + right + 2) >> 2
    out[:, 0] = a[:, 0]
    out[:, -1] = a[:, -1]
    return out


def upsample_h2v2(a):
    """h2v2 fancy upsampling of a [h][w] -> [2 h][2 w]"""
    h, w = a.shape
    if w <= 2:
        return np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)
    above = np.concatenate([a[:1], a[:-1]], axis=0)
    below = np.concatenate([a[1:], a[-1:]], axis=0)
    cols = np.empty((2 * h, w), dtype=np.int64)
    cols[0::2] = 3 * a + above
    cols[1::2] = 3 * a + below
    last = np.concatenate([cols[:, :1], cols[:, :-1]], axis=1)
    nxt = np.concatenate([cols[:, 1:], cols[:, -1:]], axis=1)
    out = np.empty((2 * h, 2 * w), dtype=np.int64)
    out[:, 0::2] = (3 * cols + last + 8) >> 4
    out[:, 1::2] = (3 * cols + nxt + 7) >> 4
    out[:, 0] = (4 * cols[:, 0] + 8) >> 4
    out[:, -1] = (4 * cols[:, -1] + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    cb = cb - 128
    cr = cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def rotate(rgb, rotation):
    """PIL's rotate(angle, expand=True) for the EXIF angles: counter-clockwise quarter turns"""
    if not rotation:
        return rgb
    assert rotation in (90, 180, 270)
    return np.ascontiguousarray(np.rot90(rgb, k=rotation // 90))


def jpeg_ref(header, coef, rotation=0):
    """header: jpeg_host.JpegHeader, coef: the flat int16 buffer of jpeg_host.decode -> rotated H x W x 3 uint8"""
    W, H = header.width, header.height
    planes = header.planes(coef)
    comps = [idct_plane(p, header.quant[c]) for c, p in enumerate(planes)]
    if header.components == 1:
        y = comps[0][:H, :W]
        rgb = np.stack([y, y, y], axis=-1).astype(np.uint8)
    else:
        hs, vs = header.h_samp[0], header.v_samp[0]
        cw, ch = -(-W // hs), -(-H // vs)                     # downsampled_width / _height of the chroma components
        up = []
        for c in (1, 2):
            a = comps[c][:ch, :cw]
            if hs == 2 and vs == 2:
                a = upsample_h2v2(a)
            elif hs == 2:
                a = upsample_h2(a)
            up.append(a[:H, :W])
        rgb = ycc_to_rgb(comps[0][:H, :W], up[0], up[1])
    return rotate(rgb, rotation)
