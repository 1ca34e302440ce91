"""
A reader for Motion-JPEG video in an AVI (RIFF) container: where each frame's JPEG lies in the file, and nothing else --
and a writer of the plainest such file (write_mjpeg_avi, at the end).

Plain Python (struct only, no cv2, no numpy).  The frame list is built by walking chunk headers -- seek, read 8 bytes --
through `LIST movi` of `RIFF 'AVI '` and of every `RIFF 'AVIX'` segment that follows (OpenDML); the `idx1` index is not
used, because its offsets are counted from different places by different writers.  Only the first `vids` stream is read,
and only when its BITMAPINFOHEADER says `MJPG`: every other file raises AviError with the reason, no file is guessed at.

    LIST movi holds   NNdc / NNdb   a frame of stream NN (two digits)          -> a frame
                      NNwb, ...     chunks of other streams, JUNK, ix##, ...   -> skipped
                      LIST 'rec '   a group of the above                       -> descended into
    a chunk of odd size is followed by one pad byte; a video chunk of size 0 means "frame dropped, show the previous one
    again": it keeps its frame number and read_frame gives the previous frame's bytes; a chunk that runs past the end of
    the file (a recording that was cut off) ends the frame list in front of it.
"""

import os
import struct


class AviError(ValueError):
    """the file is not a Motion-JPEG AVI this reader takes; `mjpeg` says whether it is one at all (an MJPG stream was
    found, and the file is damaged), which is what decides whether another decoder should be tried"""

    def __init__(self, reason, mjpeg=False):
        super().__init__(reason)
        self.mjpeg = mjpeg


def _children(f, begin, end):
    """(fourcc, payload offset, payload size, list type or None) of the chunks in [begin, end): headers only"""
    pos = begin
    while pos + 8 <= end:
        f.seek(pos)
        head = f.read(8)
        if len(head) < 8:
            return
        fourcc, size = head[:4], struct.unpack('<I', head[4:])[0]
        kind = None
        if fourcc in (b'LIST', b'RIFF'):
            kind = f.read(4)
            if len(kind) < 4:
                return
        yield fourcc, pos + 8, size, kind
        pos += 8 + size + (size & 1)


class AviFile:
    """
    path -> .n_frames, .frame_rate, .width, .height (of the stream's BITMAPINFOHEADER), .frames ([(offset, size)]),
    read_frame(i).  The file stays open until close(); a `with` block closes it.
    """

    def __init__(self, path):
        self.path = path
        self.file_size = os.path.getsize(path)
        self._f = open(path, 'rb')
        try:
            self._open()
        except BaseException:
            self._f.close()
            raise

    # ---- headers -----------------------------------------------------------------------------------------------------
    def _open(self):
        f, total = self._f, self.file_size
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF':
            raise AviError('not a RIFF file')
        if head[8:12] != b'AVI ':
            raise AviError('a RIFF file of type {!r}, not an AVI'.format(head[8:12]))
        usec, streams, movis = 0, [], []
        pos = 0
        while pos + 12 <= total:                              # RIFF 'AVI ', then RIFF 'AVIX' segments
            f.seek(pos)
            head = f.read(12)
            if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != (b'AVI ' if pos == 0 else b'AVIX'):
                break
            size = struct.unpack('<I', head[4:8])[0]
            end = min(pos + 8 + size, total)
            for fourcc, off, n, kind in _children(f, pos + 12, end):
                if fourcc != b'LIST':
                    continue
                if kind == b'hdrl' and pos == 0:
                    usec, streams = self._read_hdrl(off + 4, min(off + n, total))
                elif kind == b'movi':
                    movis.append((off + 4, off + n))
            pos += 8 + size + (size & 1)
        video = [(i, s) for i, s in enumerate(streams) if s['type'] == b'vids']
        if not video:
            raise AviError('the AVI has no video stream')
        number, stream = video[0]
        fourcc = stream.get('compression')
        if fourcc is None:
            raise AviError('the video stream has no format chunk (strf)')
        if fourcc.upper() != b'MJPG':
            raise AviError('the video stream is {!r}, not MJPG'.format(fourcc))
        self.width, self.height = stream['width'], abs(stream['height'])
        if stream['scale'] > 0 and stream['rate'] > 0:
            self.frame_rate = stream['rate'] / stream['scale']
        elif usec > 0:
            self.frame_rate = 1e6 / usec
        else:
            raise AviError('no usable frame rate: dwRate {} / dwScale {}, dwMicroSecPerFrame {}'.format(
                stream['rate'], stream['scale'], usec), mjpeg=True)
        prefix = '{:02d}'.format(number).encode('ascii')
        self.frames = []
        for begin, end in movis:
            if not self._walk_movi(begin, end, prefix):
                break                                         # cut off: nothing behind it is trusted
        self.n_frames = len(self.frames)

    def _read_hdrl(self, begin, end):
        f = self._f
        usec, streams = 0, []
        for fourcc, off, n, kind in _children(f, begin, end):
            if fourcc == b'avih' and n >= 4:
                f.seek(off)
                usec = struct.unpack('<I', f.read(4))[0]
            elif fourcc == b'LIST' and kind == b'strl':
                s = {'type': None, 'scale': 0, 'rate': 0}
                for c4, coff, cn, _ in _children(f, off + 4, min(off + n, end)):
                    f.seek(coff)
                    if c4 == b'strh' and cn >= 28:
                        h = f.read(28)
                        s['type'] = h[:4]
                        s['scale'], s['rate'] = struct.unpack('<II', h[20:28])
                    elif c4 == b'strf' and cn >= 20 and s['type'] == b'vids' and 'compression' not in s:
                        b = f.read(20)
                        s['width'], s['height'] = struct.unpack('<ii', b[4:12])
                        s['compression'] = b[16:20]
                streams.append(s)
        return usec, streams

    # ---- frames ------------------------------------------------------------------------------------------------------
    def _walk_movi(self, begin, end, prefix):
        """appends the video chunks of [begin, end) to self.frames; False when a chunk runs past the end of the file"""
        f, total = self._f, self.file_size
        pos, end = begin, min(end, total)
        while pos + 8 <= end:
            f.seek(pos)
            head = f.read(8)
            fourcc, size = head[:4], struct.unpack('<I', head[4:])[0]
            if fourcc == b'LIST':
                if f.read(4) == b'rec ':
                    pos += 12                                 # its chunks follow at once, and the list's end is theirs
                    continue
            elif fourcc[:2] == prefix and fourcc[2:].lower() in (b'dc', b'db'):
                if pos + 8 + size > total:
                    return False
                if size == 0:
                    if not self.frames:
                        raise AviError('the first video chunk is empty: there is no frame for it to repeat', mjpeg=True)
                    self.frames.append(self.frames[-1])
                else:
                    self.frames.append((pos + 8, size))
            pos += 8 + size + (size & 1)
        return True

    def read_frame(self, i):
        """the bytes of frame i's chunk, without the pad byte: one seek and one read"""
        if not 0 <= i < self.n_frames:
            raise IndexError('frame {} of {}'.format(i, self.n_frames))
        off, size = self.frames[i]
        self._f.seek(off)
        data = self._f.read(size)
        if len(data) != size:
            raise AviError('frame {} could not be read in full'.format(i), mjpeg=True)
        return data

    def close(self):
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the writer ------------------------------------------------------------------------------------------------------
RIFF_SIZE_LIMIT = (1 << 31) - 1                           # the size field of RIFF 'AVI ' in an AVI 1.0 file (no OpenDML)
_HEADER_BYTES = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + 12      # RIFF 'AVI ', LIST hdrl, the head of LIST movi


def frame_rate_fraction(fps):
    """(dwRate, dwScale) of a stream header for `fps` frames a second: round(fps * 1000) over 1000, in lowest terms -- exact
    for every rate with at most three decimals (30 -> 30 / 1, 12.5 -> 25 / 2, 29.97 -> 2997 / 100)"""
    from math import gcd
    rate = int(round(float(fps) * 1000))
    if rate <= 0:
        raise AviError('a frame rate of {!r} cannot be written'.format(fps))
    g = gcd(rate, 1000)
    return rate // g, 1000 // g


def riff_size(frame_lengths):
    """the size field of RIFF 'AVI ' for frames of these lengths, as write_mjpeg_avi lays the file out"""
    n = movi = 0
    for ln in frame_lengths:
        movi += 8 + ln + (ln & 1)
        n += 1
    return _HEADER_BYTES + movi + 8 + 16 * n - 8


def _headers(n, fps, width, height, largest, movi_bytes):
    rate, scale = frame_rate_fraction(fps)
    avih = struct.pack('<14I', int(round(1e6 / float(fps))), 0, 0, 0x10, n, 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, scale, rate, 0, n, largest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack('<IiiHH4sIiiII', 40, width, height, 1, 24, b'MJPG', width * height * 3, 0, 0, 0, 0)
    strl = b'LIST' + struct.pack('<I', 4 + 8 + len(strh) + 8 + len(strf)) + b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh \
        + b'strf' + struct.pack('<I', len(strf)) + strf
    hdrl = b'LIST' + struct.pack('<I', 4 + 8 + len(avih) + len(strl)) + b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + strl
    head = b'RIFF' + struct.pack('<I', _HEADER_BYTES + movi_bytes + 8 + 16 * n - 8) + b'AVI ' + hdrl \
        + b'LIST' + struct.pack('<I', 4 + movi_bytes) + b'movi'
    assert len(head) == _HEADER_BYTES
    return head


def write_mjpeg_avi(path, frames, fps, width, height):
    """
    Writes an AVI 1.0 file with one Motion-JPEG video stream.  frames: an iterable of complete JPEG files as bytes, in order
    (b'' is a dropped frame: a chunk of size 0); every frame is written as it is, as one `00dc` chunk.  Returns the number of
    frames.

        RIFF 'AVI '   LIST hdrl   avih, LIST strl (strh 'vids' / 'MJPG', strf BITMAPINFOHEADER 'MJPG', 24 bits)
                      LIST movi   00dc ...          a chunk of odd size is followed by one pad byte
                      idx1        per frame '00dc', AVIIF_KEYFRAME, the offset of the chunk's header from the 'movi' tag, its size

    dwMicroSecPerFrame is round(1e6 / fps); strh's dwRate / dwScale is frame_rate_fraction(fps).  dwTotalFrames, dwLength and
    dwSuggestedBufferSize (the largest chunk) are filled in when the last frame is written: the frames are streamed into
    `path + '.part'`, only the 16 index bytes of each stay in memory, and the finished file is renamed to `path`.  A file whose
    RIFF size would pass 2^31 - 1 bytes raises AviError and leaves nothing at `path`: for a sequence (something with len())
    the lengths are added up before the first byte is written; for an iterator the frame that would pass the limit ends the
    writing, and the partial file is removed.  OpenDML is not written.
    """
    width, height = int(width), int(height)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise AviError('a frame of {} x {} pixels cannot be written'.format(width, height))
    frame_rate_fraction(fps)
    if hasattr(frames, '__len__'):
        size = riff_size(len(f) for f in frames)
        if size > RIFF_SIZE_LIMIT:
            raise AviError('the file would take {} bytes: more than an AVI 1.0 file holds'.format(size + 8))
    part = path + '.part'
    n = largest = movi = 0
    index = []
    try:
        with open(part, 'wb') as f:
            f.write(b'\0' * _HEADER_BYTES)
            for data in frames:
                ln = len(data)
                if _HEADER_BYTES + movi + 8 + ln + (ln & 1) + 8 + 16 * (n + 1) - 8 > RIFF_SIZE_LIMIT:
                    raise AviError('frame {} would take the file past what an AVI 1.0 file holds'.format(n))
                index.append(struct.pack('<4sIII', b'00dc', 0x10, 4 + movi, ln))
                f.write(b'00dc' + struct.pack('<I', ln))
                f.write(data)
                if ln & 1:
                    f.write(b'\0')
                movi += 8 + ln + (ln & 1)
                largest = max(largest, ln)
                n += 1
            f.write(b'idx1' + struct.pack('<I', 16 * n))
            f.write(b''.join(index))
            f.seek(0)
            f.write(_headers(n, fps, width, height, largest, movi))
    except BaseException:
        if os.path.exists(part):
            os.remove(part)
        raise
    os.replace(part, path)
    return n
