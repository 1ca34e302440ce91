"""
Baseline JPEG files with an anatomy Pillow's encoder never writes, for the JPEG-feed tests: a SERIALISER (not an encoder)
after ITU-T T.81.  It takes quantised coefficient planes in mdjpeg_decode's layout and a header, and writes them behind
whatever file structure the keyword knobs ask for -- foreign component ids, no JFIF, an Adobe marker, SOF1, 16-bit
quantisation tables, table ids 0 / 3 / 1, a Huffman table per component, codes of any length up to 16, any restart
interval, fill bytes, padding segments, a trailer.  Camera firmware writes such files; libjpeg does not.

Two coefficient sources: the planes J.decode returns for a Pillow file (structural_corpus), and synthetic planes that no
8-bit image gives (spike_block, planes_with, extreme_family).

The module proves its own files before any project code is judged: foreign_file() has Pillow open the bytes and walks the
file's own segments (walk) to find every knob again.
"""

import io
import struct

import numpy as np

ZIGZAG = np.array((0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47,
                   55, 62, 63))
SAMPLING_FACTORS = {'444': (1, 1), '422': (2, 1), '420': (2, 2), 'gray': (1, 1), '440': (1, 2), '411': (4, 1)}
JFIF_PAYLOAD = b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
PAD_SEGMENTS = ((0xFE, b'a comment with \xff\xd8 and \xff\x00 inside'), (0xE5, bytes(range(256)) * 3), (0xEC, b''))

# the knobs in their plain form
PLAIN = dict(ids=(1, 2, 3), jfif=True, adobe=None, exif=b'', sof=0xC0, dqt16=False, quant_per_component=False,
             table_ids=(0, 1, 2), huff_per_component=False, shape=('flat', 1), one_dht=False, redefine=False, dri=0, fill=False,
             pad=False, trailer=b'')


class Header:
    """the fields of jpeg_host.JpegHeader a serialised file needs, for planes that come from no file"""

    def __init__(self, width, height, sampling, quant):
        """sampling: '444' / '422' / '420' / 'gray' (and '440' / '411', which the project refuses); quant: [64] or
        [components][64], natural order"""
        self.width, self.height = int(width), int(height)
        self.components = 1 if sampling == 'gray' else 3
        hs, vs = SAMPLING_FACTORS[sampling]
        self.h_samp = (hs, 1, 1)[:self.components]
        self.v_samp = (vs, 1, 1)[:self.components]
        self.mcus_x, self.mcus_y = -(-self.width // (8 * hs)), -(-self.height // (8 * vs))
        self.blocks_w = tuple(self.mcus_x * h for h in self.h_samp)
        self.blocks_h = tuple(self.mcus_y * v for v in self.v_samp)
        sizes = [w * h * 64 for w, h in zip(self.blocks_w, self.blocks_h)]
        self.plane_offset = tuple(int(v) for v in np.cumsum([0] + sizes[:-1]))
        self.coef_count = int(sum(sizes))
        self.quant = np.broadcast_to(np.asarray(quant, dtype=np.uint16).reshape(-1, 64), (3, 64)).copy()

    def planes(self, coef):
        return [coef[o:o + bh * bw * 64].reshape(bh, bw, 64) for o, bh, bw in zip(self.plane_offset, self.blocks_h, self.blocks_w)]


# ---- synthetic planes ------------------------------------------------------------------------------------------------------
def dct_basis():
    """[8][8]: row u holds the orthonormal 1-D DCT basis vector u sampled at x = 0 .. 7"""
    u, x = np.mgrid[0:8, 0:8]
    return np.where(u == 0, np.sqrt(1 / 8), np.sqrt(2 / 8) * np.cos((2 * x + 1) * u * np.pi / 16))


def spike_block(height, x0, y0, q):
    """the quantised coefficients (natural order, int16 [64]) of a block that is `height` at pixel (x0, y0) and 0 elsewhere,
    in JPEG's scaling (de-quantised coefficient = the orthonormal 2-D DCT of the level-shifted samples), every table entry q"""
    b = dct_basis()
    return np.round(height * np.outer(b[:, y0], b[:, x0]) / q).astype(np.int16).reshape(64)


def exact_idct(block, quant):
    """float64 [8][8]: the real-valued inverse DCT of one quantised block (natural order), without level shift or limit"""
    b = dct_basis()
    return b.T @ (np.asarray(block, np.float64) * np.asarray(quant, np.float64)).reshape(8, 8) @ b


def planes_with(header, block, component=0):
    """a zero coefficient buffer for `header` with `block` in the first block of `component` and -block in its last one"""
    coef = np.zeros(header.coef_count, np.int16)
    p = header.planes(coef)[component]
    p[-1, -1] = -np.asarray(block)
    p[0, 0] = block
    return coef


# ---- Huffman tables ------------------------------------------------------------------------------------------------------
def _flat_lengths(n, length):
    """every symbol on one length: max(length, what n codes need when the all-ones code stays unused)"""
    return [max(length, n.bit_length())] * n


def _ladder_lengths(n):
    """one code on every length from 1 up where the rest still fits on 16 bits afterwards, the rest on 16, the all-ones code
    unused.  One code on EACH of 1 .. 15 leaves room for a single 16-bit code, so a table of many symbols skips lengths:
    a dozen symbols climb 1 .. 12; 162 of them take 1 .. 8, 10, 11, 13 and 16; small scans reach 14 and 15 too."""
    out, free, rest = [], 2, n
    for length in range(1, 16):
        if rest and rest - 1 <= (free - 1) * (1 << (16 - length)) - 1:
            out.append(length)
            free -= 1
            rest -= 1
        free *= 2
    assert rest <= free - 1
    return out + [16] * rest


def huffman_table(frequencies, shape):
    """frequencies: {symbol: count}; shape: ('flat', L) or 'ladder' -> (counts[16], symbols in code order, {symbol: (code, length)})"""
    syms = sorted(frequencies, key=lambda s: (-frequencies[s], s)) if shape == 'ladder' else sorted(frequencies)
    lengths = _ladder_lengths(len(syms)) if shape == 'ladder' else _flat_lengths(len(syms), shape[1])
    counts, codes, code, last = [0] * 16, {}, 0, lengths[0]
    for s, length in zip(syms, lengths):
        code <<= length - last
        last = length
        assert code < (1 << length) - 1, 'the all-ones code stays unused'
        codes[s] = (code, length)
        counts[length - 1] += 1
        code += 1
    return counts, syms, codes


# ---- the scan ------------------------------------------------------------------------------------------------------------
def _category(v):
    return int(abs(int(v))).bit_length()


def _block_symbols(zz, pred):
    """[(class, symbol, extra bits, their number)] of one block in zig-zag order"""
    d = int(zz[0]) - pred
    c = _category(d)
    out = [(0, c, d if d >= 0 else d + (1 << c) - 1, c)]
    nz = np.flatnonzero(zz[1:]) + 1
    run_from = 1
    for i in nz:
        run = int(i) - run_from
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        v = int(zz[i])
        c = _category(v)
        out.append((1, (run << 4) | c, v if v >= 0 else v + (1 << c) - 1, c))
        run_from = int(i) + 1
    if run_from < 64:
        out.append((1, 0x00, 0, 0))
    return out


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _segment(marker, payload):
    return bytes((0xFF, marker)) + struct.pack('>H', len(payload) + 2) + payload


def serialise(header, coef, **knobs):
    """
    The bytes of a baseline JPEG that holds `coef` (flat int16, mdjpeg_decode's layout for `header`) exactly.  Knobs (PLAIN
    has the defaults):
      ids                  component identifiers
      jfif                 write the JFIF APP0 segment
      adobe                None, or the transform byte of an Adobe APP14 segment
      exif                 payload of an APP1 segment (Exif.tobytes()), b'' for none
      sof                  0xC0 (SOF0) or 0xC1 (SOF1)
      dqt16                16-bit quantisation table entries (Pq = 1)
      quant_per_component  a quantisation table per component instead of luma + shared chroma
      table_ids            the id of table slot 0, 1, 2 (quantisation and Huffman alike): (0, 3, 1) makes ids beyond 1 occur
                           and the order of first use differ from the order of ids
      huff_per_component   a DC and an AC Huffman table per component (six tables) instead of luma + shared chroma
      shape                ('flat', L) or 'ladder' (huffman_table)
      one_dht              all Huffman tables in ONE DHT segment instead of a segment each
      redefine             the first quantisation table and the first AC Huffman table are defined twice; the first
                           definition is wrong, the later one wins
      dri                  restart interval in MCUs, 0 for none
      fill                 a fill byte (FF) in front of every header segment's marker
      pad                  COM and APPn segments between the header segments
      trailer              bytes behind EOI
    """
    unknown = set(knobs) - set(PLAIN)
    assert not unknown, unknown
    k = dict(PLAIN, **knobs)
    nc = header.components
    planes = header.planes(np.asarray(coef))
    hs, vs = [int(v) for v in header.h_samp], [int(v) for v in header.v_samp]
    qslot = (lambda c: c) if k['quant_per_component'] else (lambda c: min(c, 1))
    hslot = (lambda c: c) if k['huff_per_component'] else (lambda c: min(c, 1))
    tid = k['table_ids']
    # symbols of the whole scan, restart markers in between
    pred, stream, freq = [0] * nc, [], {}
    for m in range(header.mcus_x * header.mcus_y):
        my, mx = divmod(m, header.mcus_x)
        if k['dri'] and m and m % k['dri'] == 0:
            pred = [0] * nc
            stream.append(None)
        for c in range(nc):
            for v in range(vs[c]):
                for h in range(hs[c]):
                    zz = planes[c][my * vs[c] + v, mx * hs[c] + h][ZIGZAG]
                    for cls, sym, bits, nbits in _block_symbols(zz, pred[c]):
                        f = freq.setdefault((cls, hslot(c)), {})
                        f[sym] = f.get(sym, 0) + 1
                        stream.append((cls, hslot(c), sym, bits, nbits))
                    pred[c] = int(zz[0])
    for (cls, _), f in freq.items():
        if cls == 0:
            for s in range(12):
                f.setdefault(s, 0)                           # the DC tables always hold the categories 0 .. 11
    tables = {key: huffman_table(f, k['shape']) for key, f in sorted(freq.items())}
    bits, rst = _BitWriter(), 0
    for item in stream:
        if item is None:
            bits.flush()
            bits.out += bytes((0xFF, 0xD0 + rst))
            rst = (rst + 1) & 7
            continue
        cls, slot, sym, extra, nbits = item
        bits.put(*tables[(cls, slot)][2][sym])
        if nbits:
            bits.put(extra, nbits)
    bits.flush()

    segs = []                                                 # header segments behind SOI
    if k['jfif']:
        segs.append(_segment(0xE0, JFIF_PAYLOAD))
    if k['exif']:
        segs.append(_segment(0xE1, bytes(k['exif'])))
    if k['adobe'] is not None:
        segs.append(_segment(0xEE, b'Adobe\x00\x64\x00\x00\x00\x00' + bytes((k['adobe'],))))

    def dqt(slot, table):
        q = np.asarray(table, np.int64).reshape(64)[ZIGZAG]
        body = b''.join(struct.pack('>H', int(v)) for v in q) if k['dqt16'] else bytes(int(v) for v in q)
        return _segment(0xDB, bytes(((16 if k['dqt16'] else 0) | tid[slot],)) + body)

    def dht(key, symbols=None):
        counts, syms, _ = tables[key]
        return bytes(((key[0] << 4) | tid[key[1]],)) + bytes(counts) + bytes(syms if symbols is None else symbols)

    if k['redefine']:
        segs.append(dqt(0, np.minimum(np.asarray(header.quant[0], np.int64) + 1, 65535 if k['dqt16'] else 255)))
    for slot in sorted({qslot(c) for c in range(nc)}):
        segs.append(dqt(slot, header.quant[[qslot(c) for c in range(nc)].index(slot)]))
    sof = bytes((8,)) + struct.pack('>HH', header.height, header.width) + bytes((nc,))
    sof += b''.join(bytes((k['ids'][c], (hs[c] << 4) | vs[c], tid[qslot(c)])) for c in range(nc))
    segs.append(_segment(k['sof'], sof))
    defs = []
    if k['redefine']:
        syms = tables[(1, 0)][1]
        defs.append(dht((1, 0), syms[1:] + syms[:1]))        # the same code lengths over the symbols rotated by one
    defs += [dht(key) for key in tables]
    segs += [_segment(0xC4, b''.join(defs))] if k['one_dht'] else [_segment(0xC4, d) for d in defs]
    if k['dri']:
        segs.append(_segment(0xDD, struct.pack('>H', k['dri'])))
    sos = bytes((nc,)) + b''.join(bytes((k['ids'][c], (tid[hslot(c)] << 4) | tid[hslot(c)])) for c in range(nc)) + b'\x00\x3f\x00'
    segs.append(_segment(0xDA, sos))
    out = bytearray(b'\xff\xd8')
    for i, s in enumerate(segs):
        if k['pad'] and i:
            out += _segment(*PAD_SEGMENTS[(i - 1) % len(PAD_SEGMENTS)])
        if k['fill']:
            out += b'\xff'
        out += s
    return bytes(out) + bytes(bits.out) + b'\xff\xd9' + bytes(k['trailer'])


# ---- the file's own account of itself ------------------------------------------------------------------------------------
def walk(data):
    """Walks the segments of `data` up to the scan and reports what the file itself says, in the words of the knobs, plus
    'sampling' ((h, v) per component), 'size', 'precision', 'quant' ({id: [64] natural order}, the definition in force),
    'huffman' ({(class, id): counts + symbols as the DHT segment holds them, the definition in force}), 'n_dht_segments',
    'n_dqt_definitions', 'n_dht_definitions', 'scan' (offset of the first entropy-coded byte) and 'eoi' (offset of EOI)."""
    assert data[:2] == b'\xff\xd8'
    r = dict(jfif=False, adobe=None, exif=b'', dri=0, fill=0, pad=[], quant={}, huffman={}, n_dht_segments=0, n_dqt_definitions=0,
             n_dht_definitions=0, dqt16=set(), sos_tables=None)
    p = 2
    while True:
        assert data[p] == 0xFF
        while data[p + 1] == 0xFF:
            r['fill'] += 1
            p += 1
        m = data[p + 1]
        ln = struct.unpack('>H', data[p + 2:p + 4])[0]
        body = data[p + 4:p + 2 + ln]
        if m == 0xE0 and body[:5] == b'JFIF\x00':
            r['jfif'] = True
        elif m == 0xE1 and body[:6] == b'Exif\x00\x00':
            r['exif'] = body
        elif m == 0xEE and body[:5] == b'Adobe':
            r['adobe'] = body[11]
        elif m == 0xFE or 0xE0 <= m <= 0xEF:
            r['pad'].append((m, body))
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, t = body[q] >> 4, body[q] & 15
                n = 128 if pq else 64
                vals = np.frombuffer(body[q + 1:q + 1 + n], '>u2' if pq else np.uint8).astype(np.uint16)
                nat = np.zeros(64, np.uint16)
                nat[ZIGZAG] = vals
                r['quant'][t] = nat
                r['dqt16'].add(bool(pq))
                r['n_dqt_definitions'] += 1
                q += 1 + n
        elif m in (0xC0, 0xC1):
            r['sof'], r['precision'] = m, body[0]
            h, w = struct.unpack('>HH', body[1:5])
            r['size'] = (w, h)
            comps = [body[6 + 3 * c:9 + 3 * c] for c in range(body[5])]
            r['ids'] = tuple(c[0] for c in comps)
            r['sampling'] = tuple((c[1] >> 4, c[1] & 15) for c in comps)
            r['quant_ids'] = tuple(c[2] for c in comps)
        elif m == 0xC4:
            r['n_dht_segments'] += 1
            q = 0
            while q < len(body):
                n = sum(body[q + 1:q + 17])
                r['huffman'][(body[q] >> 4, body[q] & 15)] = bytes(body[q + 1:q + 17 + n])
                r['n_dht_definitions'] += 1
                q += 17 + n
            assert q == len(body)
        elif m == 0xDD:
            r['dri'] = struct.unpack('>H', body)[0]
        elif m == 0xDA:
            assert tuple(body[1 + 2 * c] for c in range(body[0])) == r['ids']
            r['sos_tables'] = tuple((body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0]))
            r['scan'] = p + 2 + ln
            break
        else:
            raise AssertionError('marker {:02x}'.format(m))
        p += 2 + ln
    # the end of the scan: the first FF that is followed by neither 00 nor RSTn
    q, n_rst = r['scan'], 0
    while True:
        q = data.index(b'\xff', q)
        if data[q + 1] == 0 or 0xD0 <= data[q + 1] <= 0xD7:
            n_rst += data[q + 1] != 0
            q += 2
            continue
        break
    assert data[q + 1] == 0xD9
    r['eoi'], r['n_restart_markers'], r['trailer'] = q, n_rst, data[q + 2:]
    return r


def check_knobs(data, header, **knobs):
    """asserts that the file's own segments say what the knobs asked for"""
    k = dict(PLAIN, **knobs)
    r = walk(data)
    nc = header.components
    tid = k['table_ids']
    assert r['size'] == (header.width, header.height) and r['precision'] == 8
    assert r['ids'] == tuple(k['ids'][:nc]) and r['jfif'] == k['jfif'] and r['adobe'] == k['adobe'] and r['sof'] == k['sof']
    assert r['exif'] == bytes(k['exif']) and r['dri'] == k['dri'] and r['trailer'] == bytes(k['trailer'])
    assert r['sampling'] == tuple(zip(header.h_samp, header.v_samp))
    assert r['dqt16'] == {bool(k['dqt16'])}
    qslots = [c if k['quant_per_component'] else min(c, 1) for c in range(nc)]
    hslots = [c if k['huff_per_component'] else min(c, 1) for c in range(nc)]
    assert r['quant_ids'] == tuple(tid[s] for s in qslots) and sorted(r['quant']) == sorted({tid[s] for s in qslots})
    for c in range(nc):
        assert (r['quant'][r['quant_ids'][c]] == header.quant[c]).all(), 'the later definition of a table wins'
    assert r['sos_tables'] == tuple((tid[s], tid[s]) for s in hslots)
    n_tables = 2 * len(set(hslots))
    assert sorted(r['huffman']) == sorted((cls, tid[s]) for cls in (0, 1) for s in set(hslots))
    assert r['n_dht_definitions'] == n_tables + bool(k['redefine']) and r['n_dqt_definitions'] == len(set(qslots)) + bool(k['redefine'])
    assert r['n_dht_segments'] == (1 if k['one_dht'] else r['n_dht_definitions'])
    n_header_segments = r['jfif'] + bool(r['exif']) + (r['adobe'] is not None) + r['n_dqt_definitions'] + 1 + r['n_dht_segments'] + bool(r['dri']) + 1
    assert r['fill'] == (n_header_segments if k['fill'] else 0)
    assert len(r['pad']) == (n_header_segments - 1 if k['pad'] else 0)
    mcus = header.mcus_x * header.mcus_y
    assert r['n_restart_markers'] == ((mcus - 1) // k['dri'] if k['dri'] else 0)
    for (cls, t), body in r['huffman'].items():
        counts, syms = body[:16], body[16:]
        assert len(set(syms)) == len(syms)
        if cls == 0:
            assert set(range(12)) <= set(syms)
        lengths = [i + 1 for i, n in enumerate(counts) for _ in range(n)]
        if k['shape'] == 'ladder':
            assert lengths == _ladder_lengths(len(syms))
        else:
            assert set(lengths) == {max(k['shape'][1], len(syms).bit_length())}
    return r


def foreign_file(header, coef, **knobs):
    """serialise() + the proofs: Pillow opens and decodes the bytes at the header's size, and the file's own segments
    reproduce the knobs.  Returns the bytes."""
    from PIL import Image
    data = serialise(header, coef, **knobs)
    check_knobs(data, header, **knobs)
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == 'JPEG' and im.size == (header.width, header.height)
        im.load()
    return data


# ---- the corpora the CPU and the GPU tests share -------------------------------------------------------------------------
BASES = (('420', (37, 29)), ('444', (17, 9)), ('422', (40, 24)), ('gray', (33, 31)), ('420', (1, 1)))
FOREIGN_IDS = (0, 3, 1)


def exif_orientation(value):
    from PIL import Image
    exif = Image.Exif()
    exif[274] = value
    return exif.tobytes()


def variants(header):
    """(name, knobs): every knob alone, then three combinations as camera firmware makes them"""
    out = [('plain', {}), ('ids012', dict(ids=(0, 1, 2))), ('ids_odd', dict(ids=(10, 200, 33))), ('nojfif', dict(jfif=False)),
           ('nojfif_ids012', dict(jfif=False, ids=(0, 1, 2))), ('jfif_idsRGB', dict(ids=(82, 71, 66))),
           ('adobe1', dict(jfif=False, adobe=1)), ('exif6', dict(exif=exif_orientation(6))), ('sof1', dict(sof=0xC1)),
           ('dqt16', dict(dqt16=True)), ('quant3', dict(quant_per_component=True)), ('ids031', dict(table_ids=FOREIGN_IDS)),
           ('huff6', dict(huff_per_component=True)),
           ('six031', dict(huff_per_component=True, quant_per_component=True, table_ids=FOREIGN_IDS)),
           ('flat9', dict(shape=('flat', 9))), ('flat16', dict(shape=('flat', 16))), ('ladder', dict(shape='ladder')),
           ('one_dht', dict(one_dht=True)), ('redefine', dict(redefine=True)), ('dri1', dict(dri=1)), ('dri5', dict(dri=5)),
           ('dri60000', dict(dri=60000)), ('fill', dict(fill=True)), ('pad', dict(pad=True)),
           ('trailer', dict(trailer=b'\x00' * 37 + b'\xff\xd9xx')),
           ('camera_a', dict(jfif=False, exif=exif_orientation(6), huff_per_component=True, quant_per_component=True,
                             table_ids=FOREIGN_IDS, dri=header.mcus_x, one_dht=True, trailer=b'\x00\x00firmware')),
           ('camera_b', dict(jfif=False, adobe=1, sof=0xC1, dqt16=True, shape='ladder', dri=7, fill=True, pad=True)),
           ('camera_c', dict(ids=(0, 1, 2), shape=('flat', 16), dri=1, redefine=True, huff_per_component=True, pad=True,
                             exif=exif_orientation(8), trailer=b'\xff\xff'))]
    return out


def structural_corpus(J, tmp_dir):
    """[(name, bytes, header, coef, knobs)]: the coefficients of quality-95 noise files Pillow wrote, behind every anatomy of
    variants(); header and coef are what J.decode gave for the Pillow file"""
    import os
    import jpeg_fixtures as JF
    out = []
    for sampling, (w, h) in BASES:
        p = JF.write_jpeg(os.path.join(str(tmp_dir), 'base.jpg'), JF.content('noise', w, h), sampling, 95)
        rc, header, coef = J.decode(open(p, 'rb').read())
        assert rc == 0
        for name, knobs in variants(header):
            out.append(('{}_{}x{}_{}'.format(sampling, w, h, name), foreign_file(header, coef, **knobs), header, coef, knobs))
    return out


# blocks no 8-bit image gives, inside the energy bound of the entropy decoders (norm below 1029 with 8-bit tables of small
# entries, below 2800 at most): their samples leave [-512, 511], where a range-limit table and saturation part
SPIKE_HEIGHTS = (400, 500, 511, 520, 560, 700, 1000, 1028)
SPIKE_POSITIONS = ((0, 0), (3, 3), (7, 7))
SPIKE_TABLES = (1, 2, 16, 255)
SINGLE_INDICES = (1, 8, 9, 36, 63)
# (coefficient, table value): de-quantised values from 1900 to 2799, all but one in tables that need 16 bits
SINGLES = ((1, 1900), (1, 2000), (1, 2100), (1, 2250), (1, 2400), (1, 2600), (1, 2790), (1, 2799), (-1, 2790), (2, 1395), (3, 700),
           (3, 930), (4, 520), (4, 560), (4, 600), (4, 699), (-4, 600), (7, 300), (8, 255))
# beyond every energy bound: these must be refused by everything alike
BEYOND = ((1, 2801), (1, 40000), (11, 255), (5, 600))


def extreme_family(singles=SINGLES, spikes=True):
    """[(name, header, coef, block, table value, knobs)] over 16 x 16 files, 4:4:4 and grayscale: one-pixel spikes of
    SPIKE_HEIGHTS, both signs, at SPIKE_POSITIONS under flat tables of SPIKE_TABLES in luma; single coefficients at
    SINGLE_INDICES in luma, and at 9 and 63 in Cb too.  `block` sits in the component's first block, -block in its last."""
    out = []
    for sampling in ('444', 'gray'):
        if spikes:
            for q in SPIKE_TABLES:
                header = Header(16, 16, sampling, np.full(64, q))
                for height in SPIKE_HEIGHTS:
                    for sign in (1, -1):
                        for x0, y0 in SPIKE_POSITIONS:
                            block = spike_block(sign * height, x0, y0, q)
                            out.append(('{}_spike{:+d}_at{}{}_q{}'.format(sampling, sign * height, x0, y0, q), header,
                                        planes_with(header, block), block, q, {}))
        for v, q in singles:
            header = Header(16, 16, sampling, np.full(64, q))
            for index in SINGLE_INDICES:
                for comp in range(2 if index in (9, 63) and sampling != 'gray' else 1):
                    block = np.zeros(64, np.int16)
                    block[index] = v
                    out.append(('{}_single{:+d}x{}_at{}_c{}'.format(sampling, v, q, index, comp), header,
                                planes_with(header, block, comp), block, q, dict(dqt16=q > 255)))
    return out


def pillow_extremes(tmp_dir):
    """[(name, path)]: the hardest images 8 bits can hold -- checkerboard, one-pixel spikes, their inverse, one-pixel
    stripes -- at 40 x 24, written by Pillow in 4:4:4 / 4:2:0 / grayscale at qualities 1, 5, 25, 75 and 100: 60 files"""
    import os
    import jpeg_fixtures as JF
    yy, xx = np.mgrid[0:24, 0:40]
    spikes = ((xx % 8 == 3) & (yy % 8 == 3)) * 255
    images = {'checker': ((xx + yy) & 1) * 255, 'spike': spikes, 'invspike': 255 - spikes, 'stripes': (xx & 1) * 255}
    out = []
    for name, g in images.items():
        arr = np.stack([g, g, g], -1).astype(np.uint8)
        if name == 'checker':
            arr[..., 1] = 255 - arr[..., 1]
        for sampling in ('444', '420', 'gray'):
            for q in (1, 5, 25, 75, 100):
                tag = '{}_{}_q{}'.format(name, sampling, q)
                out.append((tag, JF.write_jpeg(os.path.join(str(tmp_dir), tag + '.jpg'), arr, sampling, q)))
    return out
