"""
AVI files for the Motion-JPEG tests, muxed at run time from JPEG frames Pillow encoded (nothing is committed as a binary):
a small RIFF writer that can produce what real writers produce -- an idx1 index or none, an interleaved audio stream, JUNK
chunks, frames grouped in LIST 'rec ', an OpenDML RIFF 'AVIX' segment, dropped (zero-length) frames -- and the JPEG surgery
the abbreviated-stream tests need (DHT segments removed, tables renumbered).
"""

import io
import struct

import numpy as np


# ---- JPEG frames ------------------------------------------------------------------------------------------------------
def jpeg_bytes(arr, sampling='422', quality=85, **extra):
    """the file Pillow writes for an h x w x 3 uint8 array; sampling: '444' | '422' | '420' | 'gray'"""
    from PIL import Image
    im = Image.fromarray(arr)
    kw = dict(quality=quality)
    if sampling == 'gray':
        im = im.convert('L')
    else:
        kw['subsampling'] = {'444': 0, '422': 1, '420': 2}[sampling]
    kw.update(extra)
    out = io.BytesIO()
    im.save(out, 'JPEG', **kw)
    return out.getvalue()


def segments(data):
    """(marker, start, end) of every segment in front of the entropy-coded data, the SOS header included"""
    p = 2
    while True:
        assert data[p] == 0xFF, 'lost the marker chain at {}'.format(p)
        m = data[p + 1]
        ln = (data[p + 2] << 8) | data[p + 3]
        yield m, p, p + 2 + ln
        if m == 0xDA:
            return
        p += 2 + ln


def _dht_tables(payload):
    """the tables of a DHT segment's payload: [(tc_th, bytes of that table)]"""
    out, q = [], 0
    while q < len(payload):
        n = 17 + sum(payload[q + 1:q + 17])
        out.append((payload[q], payload[q:q + n]))
        q += n
    return out


def strip_dht(data, drop=None):
    """`data` without its Huffman tables (drop None: all of them; else the set of tc_th bytes to drop, e.g. {0x01, 0x11}
    for the chrominance pair): what a Motion-JPEG encoder that relies on the standard's tables writes"""
    out, last = [data[:2]], 2
    for m, a, b in segments(data):
        out.append(data[last:a])
        if m == 0xC4:
            keep = b''.join(t for tc_th, t in _dht_tables(data[a + 4:b]) if drop is not None and tc_th not in drop)
            if keep:
                out.append(b'\xff\xc4' + struct.pack('>H', len(keep) + 2) + keep)
        else:
            out.append(data[a:b])
        last = b
    out.append(data[last:])
    return b''.join(out)


def renumber_tables(data, table_id):
    """`data` with every Huffman table and every selector of the scan header moved to `table_id` -- for a grayscale file,
    whose scan names one DC and one AC table"""
    d = bytearray(data)
    for m, a, b in segments(data):
        if m == 0xC4:
            tables = _dht_tables(data[a + 4:b])
            assert len(tables) == 1
            d[a + 4] = (d[a + 4] & 0xF0) | table_id
        elif m == 0xDA:
            assert d[a + 4] == 1
            d[a + 6] = (table_id << 4) | table_id
    return bytes(d)


# ---- the container ----------------------------------------------------------------------------------------------------
def chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\x00' if len(payload) & 1 else b'')


def riff_list(kind, body, tag=b'LIST'):
    return tag + struct.pack('<I', len(body) + 4) + kind + body


def _video_strl(fourcc, width, height, rate, scale, n):
    strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', fourcc, 0, 0, 0, 0, scale, rate, 0, n, 0, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack('<IiiHH4sIiiII', 40, width, height, 1, 24, fourcc, width * height * 3, 0, 0, 0, 0)
    return riff_list(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf))


def _audio_strl(n):
    strh = struct.pack('<4s4sIHHIIIIIIII4H', b'auds', b'\x00' * 4, 0, 0, 0, 0, 1, 8000, 0, n, 0, 0xFFFFFFFF, 1, 0, 0, 0, 0)
    strf = struct.pack('<HHIIHHH', 1, 1, 8000, 8000, 1, 8, 0)
    return riff_list(b'strl', chunk(b'strh', strh) + chunk(b'strf', strf))


def avi_bytes(frames, size, rate=30, scale=1, usec=None, fourcc=b'MJPG', idx1=True, audio=False, audio_first=False,
              junk=False, rec=False, avix_from=None, video=True):
    """
    frames: the video chunks' payloads in order (b'' = a dropped frame); size: (width, height).  rate / scale go into the
    stream header, usec (default: derived from them) into the main header.  audio: a second stream whose chunk follows every
    frame (audio_first: it is stream 00 and the video 01); junk: JUNK chunks in hdrl, in front of movi and between
    frames; rec: every frame (and its audio) inside a LIST 'rec '; avix_from: frames from this index on go into a RIFF
    'AVIX' segment; video=False: an audio-only file.
    """
    width, height = size
    n = len(frames)
    if usec is None:
        usec = int(round(1e6 * scale / rate)) if rate else 0
    v_id, a_id = (b'01', b'00') if (audio and audio_first) else (b'00', b'01')
    strls = []
    if video:
        strls.append(_video_strl(fourcc, width, height, rate, scale, n))
    if audio or not video:
        strls.append(_audio_strl(n))
        if audio_first or not video:
            strls.reverse()
    avih = struct.pack('<14I', usec, 0, 0, 0x10 if idx1 else 0, n, 0, len(strls), 0, width, height, 0, 0, 0, 0)
    hdrl = chunk(b'avih', avih) + b''.join(strls)
    if junk:
        hdrl += chunk(b'JUNK', b'\x00' * 13)

    def movi_body(lo, hi, index):
        body = b''
        for i in range(lo, hi):
            group, entries = b'', []
            if video:
                entries.append((v_id + b'dc', len(group), len(frames[i])))
                group += chunk(v_id + b'dc', frames[i])
            if audio or not video:
                pcm = bytes((i * 7 + k) & 0xFF for k in range(267))          # odd size: a pad byte follows
                tag = (a_id if video else b'00') + b'wb'
                entries.append((tag, len(group), len(pcm)))
                group += chunk(tag, pcm)
            if junk and i % 3 == 1:
                group += chunk(b'JUNK', b'\x00' * 5)
            head = 12 if rec else 0
            for tag, off, ln in entries:
                index.append(struct.pack('<4sIII', tag, 0x10, 4 + len(body) + head + off, ln))
            body += riff_list(b'rec ', group) if rec else group
        return body

    first = n if avix_from is None else avix_from
    index = []
    main = riff_list(b'hdrl', hdrl)
    if junk:
        main += chunk(b'JUNK', b'\x00' * 100)
    main += riff_list(b'movi', movi_body(0, first, index))
    if idx1:
        main += chunk(b'idx1', b''.join(index))
    out = riff_list(b'AVI ', main, tag=b'RIFF')
    if first < n:
        out += riff_list(b'AVIX', riff_list(b'movi', movi_body(first, n, [])), tag=b'RIFF')
    return out


def write_avi(path, frames, size, **kw):
    with open(path, 'wb') as f:
        f.write(avi_bytes(frames, size, **kw))
    return str(path)


# ---- frame content ----------------------------------------------------------------------------------------------------
def block_noise(w, h, seed, cell=4):
    """an h x w x 3 image of random cell x cell blocks: busy enough that a small scan spans several 1024-bit subsequences"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (-(-h // cell), -(-w // cell), 3), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(base, np.ones((cell, cell, 1), dtype=np.uint8))[:h, :w])


def flat(w, h, value=(90, 140, 60)):
    return np.ascontiguousarray(np.broadcast_to(np.array(value, dtype=np.uint8), (h, w, 3)))


def pil_rgb(data):
    """Pillow's decode of a stored JPEG: what every frame is pinned to"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))
