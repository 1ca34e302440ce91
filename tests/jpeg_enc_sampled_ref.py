"""
tests/jpeg_enc_ref.py for the three chroma samplings and any pair of quantisation tables: the NumPy restatement of the lossy
half of libjpeg-turbo's encoder for Image.save(qtables=[luma, chroma], subsampling=s), s = 0 (4:4:4), 1 (4:2:2), 2 (4:2:0).
The colour conversion, the forward DCT, the quantiser and the dummy blocks are jpeg_enc_ref's own functions; what differs per
sampling is the chroma down-sampling (jcsample.c):

  * fullsize_downsample (h1v1): the samples as they are, the right edge replicated to whole blocks;
  * h2v1_downsample: the right edge replicated to 16 columns per chroma block FIRST, then pairs along a row,
    (a + b + bias) >> 1 with the bias alternating 0, 1 from the left;
  * h2v2_downsample: jpeg_enc_ref.component_planes.

Also the window matrix and the table pairs that test_encode_sampled_cpu.py and test_gpu_encode_sampled.py share.
"""

import io

import numpy as np

import jpeg_enc_ref as E
from megadetector_amd import jpeg_host as J

SAMPLINGS = (0, 1, 2)
# the right and the bottom edge at every kind of position within an MCU of each layout
SIZES = [(1, 1), (8, 8), (9, 8), (16, 8), (17, 9), (15, 17), (33, 31), (70, 50)]           # w x h


def table_pairs():
    """name -> (luma, chroma), uint16 [64] natural order: three qualities and one pair no quality gives"""
    k = np.arange(64)
    odd_luma = (1 + (k * 37 + 11) % 97).astype(np.uint16)
    odd_chroma = (255 - (k * 29) % 200).astype(np.uint16)
    odd_luma[0], odd_luma[63], odd_chroma[0], odd_chroma[1] = 3, 255, 1, 255
    pairs = {'q50': J.quant_tables(50), 'q91': J.quant_tables(91), 'q100': J.quant_tables(100), 'odd': (odd_luma, odd_chroma)}
    assert all(t.min() >= 1 and t.max() <= 255 for p in pairs.values() for t in p)
    return pairs


def window(w, h, seed, kind='random'):
    rng = np.random.default_rng(seed)
    if kind == 'flat':
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    if kind == 'saturated':
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def component_planes(rgb, sampling):
    if sampling == 2:
        return E.component_planes(rgb)
    H, W = rgb.shape[:2]
    y, cb, cr = E.rgb_to_ycc(rgb)
    bw, bh = -(-W // 8), -(-H // 8)
    planes = [E._pad_bottom(E._pad_right(y, bw * 8), bh * 8)]
    for c in (cb, cr):
        if sampling == 0:
            planes.append(E._pad_bottom(E._pad_right(c, bw * 8), bh * 8))
            continue
        bw_c = -(-(-(-W // 2)) // 8)
        c = E._pad_right(c, bw_c * 16)
        bias = np.tile(np.array([0, 1], dtype=np.int64), bw_c * 4)[None, :]
        planes.append(E._pad_bottom((c[:, 0::2] + c[:, 1::2] + bias) >> 1, bh * 8))
    return planes


def coefficients(rgb, sampling, quant_luma, quant_chroma):
    """flat int16 planes in the layout of mdjpeg_decode for this sampling: what mdjpeg_encode_subsequences_sampled takes"""
    H, W = rgb.shape[:2]
    hs, vs = J.SAMPLING_FACTORS[sampling]
    mcus_x, mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
    out = []
    for c, p in enumerate(component_planes(rgb, sampling)):
        h, v = (hs, vs) if c == 0 else (1, 1)
        q = np.asarray(quant_luma if c == 0 else quant_chroma)
        out.append(E._fill_mcus(E.fdct_quantise(p, q), mcus_x, mcus_y, h, v).astype(np.int16).reshape(-1))
    return np.concatenate(out)


def pillow_file(rgb, sampling, quant_luma, quant_chroma, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(rgb).save(bio, 'JPEG', qtables=[[int(v) for v in quant_luma], [int(v) for v in quant_chroma]], subsampling=sampling, **kw)
    return bio.getvalue()


def scan_of(data):
    """the bytes between the SOS header and EOI of a file"""
    rc, sc, _ = J.scan(data)
    assert rc == J.MDJPEG_OK
    return data[int(sc.scan_begin):int(sc.scan_end)]


def matrix():
    """[(name, rgb, sampling, pair name)]: every size x sampling x pair, and a flat and a saturated window per sampling"""
    cases = []
    for pi, pair in enumerate(table_pairs()):
        for s in SAMPLINGS:
            for si, (w, h) in enumerate(SIZES):
                cases.append(('{}x{} s{} {}'.format(w, h, s, pair), window(w, h, 1000 * pi + 100 * s + si), s, pair))
    for s in SAMPLINGS:
        cases.append(('flat s{}'.format(s), window(70, 50, 0, 'flat'), s, 'q50'))
        cases.append(('saturated s{}'.format(s), window(70, 50, 7 + s, 'saturated'), s, 'q100'))
    return cases
