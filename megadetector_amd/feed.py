"""
Host feed for real image files.

The reference moves decoded images from its loader processes to the GPU process by pickling the
arrays through a `JoinableQueue(maxsize=10)` (run_detector_batch.py:92,:124-200,:518) -- at MI355X
speeds that queue, not the GPU, sets the rate (decode is ~7 ms per 3-megapixel JPEG and core, the GPU
takes ~1 ms per image).  Here:

  * loader *processes* (spawned, never forked: a forked child of a process that has touched HIP is
    undefined behaviour) decode with PIL -- same EXIF-rotation and failure semantics as the reference's
    `load_image` (visualization_utils.py:103-175,:306) -- straight into a slot of ONE shared-memory ring;
  * only (file name, slot, shape) crosses the queue; the GPU process sees the pixels as a zero-copy
    NumPy view of the slot;
  * the ring is page-locked in the GPU process (hipHostRegister), so the host-to-device copy of a batch
    is an asynchronous DMA at PCIe rate on a copy stream, overlapped with the previous batch's kernels
    (detector.HIPDetector.start_batch / finish_batch);
  * an image that does not fit a slot falls back to travelling through the queue as an array;
  * decode='coefficients' (opt-in, run_detector_batch --gpu_jpeg): for a baseline JPEG the loader only Huffman-decodes
    (jpeg_host / libmdjpeg.so) and the slot carries quantised DCT coefficients; the GPU rebuilds the pixels PIL would
    have produced, bit for bit (mdhip_jpeg_reconstruct).  decode='scan' (run_detector_batch --gpu_jpeg_entropy) goes one
    step further: the loader only parses the headers and the slot carries the compressed file; the GPU also Huffman-decodes
    (mdhip_jpeg_entropy_decode).  Any file the entropy decoder does not take cleanly goes the
    PIL way above, per file.

This module must stay import-light (numpy + PIL, and jpeg_host's ctypes): it is what the spawned loader processes import,
and they never open the GPU.
"""

import multiprocessing as mp
import os
import queue
import traceback

import numpy as np

EXIF_IMAGE_ROTATIONS = {3: 180, 6: 270, 8: 90}                  # reference visualization_utils.py


def load_image(input_file, ignore_exif_rotation=False):
    """PIL decode to RGB with EXIF rotation (reference visualization_utils.py:103-175, :306)."""
    from PIL import Image
    image = Image.open(input_file)
    if image.mode not in ('RGBA', 'RGB', 'L', 'I;16'):
        raise AttributeError('Image {} uses unsupported mode {}'.format(input_file, image.mode))
    if image.mode in ('RGBA', 'L'):
        image = image.convert(mode='RGB')
    if not ignore_exif_rotation:
        try:
            exif = image._getexif()
            orientation = exif.get(274, None)
            if orientation is not None and orientation != 1:
                assert orientation in EXIF_IMAGE_ROTATIONS, 'Mirrored rotations are not supported'
                image = image.rotate(EXIF_IMAGE_ROTATIONS[orientation], expand=True)
        except Exception:
            pass
    image.load()
    return image


def image_metadata(image):
    """what _add_image_metadata needs from the PIL image, as plain data (reference :769-792)"""
    dt = None
    try:
        exif = image.getexif()
        dt = exif.get(36867) or exif.get(306)       # DateTimeOriginal / DateTime
    except Exception:
        pass
    return {'width': image.width, 'height': image.height, 'datetime': dt}


class ImageMeta:
    """Stands in for the PIL image where only width / height / datetime are read."""

    def __init__(self, meta):
        self.width, self.height, self._dt = meta['width'], meta['height'], meta['datetime']

    def getexif(self):
        return {36867: self._dt} if self._dt is not None else {}


def coefficient_image(ring, slot, shape):
    """the jpeg_host.CoefficientImage a loader left in `slot` (views of the ring: nothing is copied)"""
    from . import jpeg_host
    return jpeg_host.CoefficientImage.from_slot(ring.slot(slot), shape)


def scan_image(ring, slot, shape):
    """the jpeg_host.ScanImage a loader left in `slot` (the file's bytes stay views of the ring)"""
    from . import jpeg_host
    return jpeg_host.ScanImage.from_slot(ring.slot(slot), shape)


class SharedImageRing:
    """n_slots x slot_bytes of shared memory + the queue of free slot numbers."""

    def __init__(self, n_slots, slot_bytes, ctx):
        from multiprocessing import shared_memory
        self.n_slots, self.slot_bytes = int(n_slots), int(slot_bytes)
        self.shm = shared_memory.SharedMemory(create=True, size=self.n_slots * self.slot_bytes)
        self.free_q = ctx.Queue()
        for i in range(self.n_slots):
            self.free_q.put(i)
        self._registered = False
        self._all = np.ndarray((self.n_slots * self.slot_bytes,), dtype=np.uint8, buffer=self.shm.buf)

    @property
    def name(self):
        return self.shm.name

    def view(self, slot, shape):
        n = int(np.prod(shape))
        off = slot * self.slot_bytes
        return self._all[off:off + n].reshape(shape)

    def slot(self, slot):
        """the whole slot as a flat uint8 view"""
        off = slot * self.slot_bytes
        return self._all[off:off + self.slot_bytes]

    def pin(self):
        """Page-locks the ring for asynchronous H2D copies (no-op without a HIP device).  Returns bool."""
        try:
            import torch
            if not torch.cuda.is_available():
                return False
            rc = torch.cuda.cudart().cudaHostRegister(self._all.ctypes.data, self._all.nbytes, 0)
            self._registered = int(rc) == 0
        except Exception:
            self._registered = False
        return self._registered

    def release(self, slot):
        self.free_q.put(slot)

    def close(self):
        if self._registered:
            try:
                import torch
                torch.cuda.cudart().cudaHostUnregister(self._all.ctypes.data)
            except Exception:
                pass
            self._registered = False
        self._all = None
        try:
            self.shm.close()
            self.shm.unlink()
        except Exception:
            pass


def _pixels_to_ring(im_file, buf, slot_bytes, free_q, ready_q, want_meta, worker_id):
    """PIL decode of one file into a ring slot (or, too large for one, through the queue)"""
    image = load_image(im_file)
    meta = image_metadata(image) if want_meta else None
    arr = np.asarray(image)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
        raise ValueError('unexpected decoded layout {} {}'.format(arr.shape, arr.dtype))
    if arr.nbytes <= slot_bytes:
        slot = free_q.get()
        off = slot * slot_bytes
        np.copyto(buf[off:off + arr.nbytes].reshape(arr.shape), arr)
        ready_q.put(('slot', im_file, slot, arr.shape, meta, worker_id))
    else:
        ready_q.put(('array', im_file, np.ascontiguousarray(arr), arr.shape, meta, worker_id))


def open_for_coefficients(input_file):
    """
    The header half of load_image: opens the file (no pixel is decoded), applies load_image's mode check and reads the
    EXIF orientation with load_image's own statements.  Returns (image, rotation): the angle load_image would turn the
    decoded image by (0 when it would not turn it: no tag, orientation 1, a mirrored orientation whose assert fails
    inside the try, an EXIF block that raises, ignore).
    """
    from PIL import Image
    image = Image.open(input_file)
    if image.mode not in ('RGBA', 'RGB', 'L', 'I;16'):
        raise AttributeError('Image {} uses unsupported mode {}'.format(input_file, image.mode))
    rotation = 0
    try:
        # load_image converts 'RGBA' / 'L' first; what convert() returns is a plain Image, and where that has no
        # _getexif the lookup raises inside the try: such an image is never rotated
        exif = (image if image.mode not in ('RGBA', 'L') else Image.Image())._getexif()
        orientation = exif.get(274, None)
        if orientation is not None and orientation != 1:
            assert orientation in EXIF_IMAGE_ROTATIONS, 'Mirrored rotations are not supported'
            rotation = EXIF_IMAGE_ROTATIONS[orientation]
    except Exception:
        pass
    return image, rotation


def _coefficients_to_ring(im_file, buf, slot_bytes, free_q, ready_q, want_meta, worker_id):
    """
    Entropy decode of one baseline JPEG into a ring slot.  Returns False -- having put nothing on the queue -- when the
    file has to go the PIL way: not a JPEG, a kind mdjpeg_parse does not support, planes larger than a slot, or a stream
    the decoder reports as not clean.  Exceptions of the header half are load_image's own and propagate.
    """
    from . import jpeg_host
    image, rotation = open_for_coefficients(im_file)
    if image.format != 'JPEG':
        return False
    with open(im_file, 'rb') as f:
        data = f.read()
    header = jpeg_host.parse(data)
    if not header.supported or jpeg_host.SLOT_HEADER_BYTES + 2 * header.coef_count > slot_bytes:
        return False
    meta = None
    if want_meta:
        meta = image_metadata(image)
        if rotation in (90, 270):
            meta['width'], meta['height'] = meta['height'], meta['width']
    slot = free_q.get()
    try:
        off = slot * slot_bytes
        rc = jpeg_host.decode_into_slot(data, buf[off:off + slot_bytes], rotation)
    except BaseException:
        free_q.put(slot)
        raise
    if rc != jpeg_host.MDJPEG_OK:
        free_q.put(slot)
        return False
    h, w = (header.width, header.height) if rotation in (90, 270) else (header.height, header.width)
    ready_q.put(('jpeg', im_file, slot, (h, w, 3), meta, worker_id))
    return True


def _scan_to_ring(im_file, buf, slot_bytes, free_q, ready_q, want_meta, worker_id):
    """
    The compressed scan of one baseline JPEG into a ring slot, with its descriptor (jpeg_host.scan_into_slot): no Huffman
    symbol is decoded here.  Returns False -- having put nothing on the queue -- exactly where _coefficients_to_ring
    does, except that damage only symbol decoding can see is left for the GPU to flag.
    """
    from . import jpeg_host
    image, rotation = open_for_coefficients(im_file)
    if image.format != 'JPEG':
        return False
    with open(im_file, 'rb') as f:
        data = f.read()
    header = jpeg_host.parse(data)
    if not header.supported or jpeg_host.SLOT_HEADER_BYTES + 2 * header.coef_count > slot_bytes:
        return False
    meta = None
    if want_meta:
        meta = image_metadata(image)
        if rotation in (90, 270):
            meta['width'], meta['height'] = meta['height'], meta['width']
    slot = free_q.get()
    try:
        off = slot * slot_bytes
        rc = jpeg_host.scan_into_slot(data, buf[off:off + slot_bytes], rotation)
    except BaseException:
        free_q.put(slot)
        raise
    if rc != jpeg_host.MDJPEG_OK:
        free_q.put(slot)
        return False
    h, w = (header.width, header.height) if rotation in (90, 270) else (header.height, header.width)
    ready_q.put(('scan', im_file, slot, (h, w, 3), meta, worker_id))
    return True


_FAST_PATHS = {'coefficients': _coefficients_to_ring, 'scan': _scan_to_ring}


def _loader_process_main(shm_name, slot_bytes, file_q, free_q, ready_q, want_meta, worker_id, decode='pixels'):
    """Body of a loader process: file names in, (file, slot, shape) out."""
    from multiprocessing import shared_memory
    shm = shared_memory.SharedMemory(name=shm_name)
    try:
        buf = np.ndarray((shm.size,), dtype=np.uint8, buffer=shm.buf)
        while True:
            im_file = file_q.get()
            if im_file is None:
                break
            try:
                fast = _FAST_PATHS.get(decode)
                if fast is None or not fast(im_file, buf, slot_bytes, free_q, ready_q, want_meta, worker_id):
                    _pixels_to_ring(im_file, buf, slot_bytes, free_q, ready_q, want_meta, worker_id)
            except Exception as e:
                print('Producer process: image {} cannot be loaded:\n{}'.format(im_file, str(e)))
                ready_q.put(('fail', im_file, None, None, None, worker_id))
        del buf
    except Exception:
        traceback.print_exc()
    finally:
        ready_q.put(('done', None, None, None, None, worker_id))
        shm.close()


class ProcessLoader:
    """
    Spawns the loader processes and yields ('slot'|'array'|'fail'|'jpeg', file, payload, shape, meta) in
    completion order.  `payload` is the slot number (pixels: ring.view(slot, shape)) or the array.
    decode='coefficients': baseline JPEGs arrive as 'jpeg' -- the slot holds quantised DCT coefficients
    (jpeg_host.CoefficientImage.from_slot(ring.slot(slot), shape)), `shape` is that of the rotated RGB image; every
    other file arrives exactly as with decode='pixels' (the default).
    decode='scan': baseline JPEGs arrive as 'scan' -- the slot holds the file's bytes and the descriptor of its scan
    (jpeg_host.ScanImage.from_slot), no Huffman symbol decoded; the same files as with 'coefficients', plus those whose
    damage only symbol decoding can see.
    """

    def __init__(self, image_files, n_workers, n_slots, slot_bytes, want_meta=False, decode='pixels'):
        if decode not in ('pixels', 'coefficients', 'scan'):
            raise ValueError("decode must be 'pixels', 'coefficients' or 'scan', got {!r}".format(decode))
        self.ctx = mp.get_context('spawn')
        self.ring = SharedImageRing(n_slots, slot_bytes, self.ctx)
        self.file_q = self.ctx.Queue()
        self.ready_q = self.ctx.Queue()
        self.n_workers = max(1, min(int(n_workers), max(1, len(image_files))))
        for f in image_files:
            self.file_q.put(f)
        for _ in range(self.n_workers):
            self.file_q.put(None)
        self.procs = [self.ctx.Process(target=_loader_process_main,
                                       args=(self.ring.name, self.ring.slot_bytes, self.file_q, self.ring.free_q,
                                             self.ready_q, bool(want_meta), i, decode), daemon=True)
                      for i in range(self.n_workers)]
        for p in self.procs:
            p.start()

    def __iter__(self):
        finished = 0
        while finished < self.n_workers:
            try:
                item = self.ready_q.get(timeout=5.0)
            except queue.Empty:
                if not any(p.is_alive() for p in self.procs):      # all loaders died without saying so
                    break
                continue
            if item[0] == 'done':
                finished += 1
                continue
            yield item[:5]

    def close(self):
        for p in self.procs:
            p.join(timeout=5.0)
            if p.is_alive():
                p.terminate()
        self.ring.close()
