/*
 * mdhip.h -- C ABI of the MI355X-native MegaDetector v5 batch-inference hot path.
 *
 * The reference (agentmorris/MegaDetector) is pure Python and has NO FFI on this path; its
 * plugin seam is the duck-typed detector object returned by
 *   megadetector/detection/run_detector.py:601  load_detector(...)
 * i.e. the class  megadetector/detection/pytorch_detector.py:739  PTDetector.
 * This header is the C ABI that sits *under* that Python seam: each
 * entry point replaces one stage of PTDetector._process_batch_group
 * (pytorch_detector.py:1257-1426) and is bound from Python with ctypes
 * (megadetector_amd/_lib.py; the stub a maintainer would add is shown in INTEGRATION.md).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative MDHIP_E* code, never throws, never exits.  mdhip_last_error() returns a
 * human-readable message for the most recent failure on that context (or, with ctx == NULL,
 * the most recent failure of mdhip_create or of a context-free call on the calling thread).  A context is bound to one GPU
 * and is not thread-safe; use one context per (process, GPU).  The library owns all device
 * buffers and packed weights; the caller owns every pointer it passes in.
 */
#ifndef MDHIP_H
#define MDHIP_H

#include <stddef.h>
#include <stdint.h>

#include "mdjpeg.h"      /* mdjpeg_scan_info: the descriptor mdhip_jpeg_entropy_decode takes */

#ifdef __cplusplus
extern "C" {
#endif

#define MDHIP_OK            0
#define MDHIP_EINVAL       -1   /* bad argument / unsupported model description */
#define MDHIP_EHIP         -2   /* a HIP runtime call failed                     */
#define MDHIP_ENOMEM       -3   /* device arena too small for the request        */
#define MDHIP_EUNSUPPORTED -4   /* valid request this build does not implement   */
#define MDHIP_ECAPACITY    -5   /* mdhip_jpeg_encode, mdhip_repeat_detections: the output buffer is too small */

/* arithmetic type of the conv stack */
#define MDHIP_DTYPE_BF16 0
#define MDHIP_DTYPE_FP8  1      /* BASELINE.json configs[4]: bf16 storage, the 3x3 convs of the bottlenecks on e4m3
                                 * operands (W8A8, block-scaled K = 128 MFMA); needs mdhip_calibrate once */
#define MDHIP_DTYPE_FP16 2      /* fp16 storage of activations and weights (fp32 accumulate): same MFMA rate as
                                 * bf16, 3 more mantissa bits -- the accuracy mode */

/* module kinds of a YOLOv5 model description (yolov5 models/yolo.py:parse_model rows) */
#define MDHIP_CONV      0
#define MDHIP_C3        1
#define MDHIP_SPPF      2
#define MDHIP_UPSAMPLE  3
#define MDHIP_CONCAT    4
#define MDHIP_DETECT    5
/* module kinds of a YOLO11 model description (ultralytics yolo11.yaml rows, anchor-free; MDv1000-larch / -sorrel) */
#define MDHIP_C3K2       6
#define MDHIP_C2PSA      7
#define MDHIP_DETECT_DFL 8
/* module kinds of a YOLOv9-C model description (WongKinYiu yolov9 yaml rows, anchor-free; MDv1000-cedar) */
#define MDHIP_ELAN4       9     /* RepNCSPELAN4                                                                 */
#define MDHIP_ADOWN      10
#define MDHIP_CBLINEAR   11
#define MDHIP_CBFUSE     12
#define MDHIP_DETECT_DDFL 13    /* DDetect / DualDDetect                                                        */
#define MDHIP_SILENCE    14     /* identity (an alias of its input; yolov9 Silence)                             */

/* One fused (conv + folded BatchNorm) of the checkpoint: what
 * pytorch_detector.py:957  checkpoint['model'].float().fuse()  leaves in each Conv module. */
typedef struct {
    const float* weight;   /* host, fp32, OIHW: [c_out][c_in][kh][kw] */
    const float* bias;     /* host, fp32, [c_out]                      */
    int32_t c_out, c_in, kh, kw;
} mdhip_conv;

/* One row of the model (same granularity as model.model[i] in the reference's checkpoint).
 * from[] holds absolute layer indices (-1 = the network input).
 * Conv:    convs[first_conv]                        k,s,p as in the module
 * C3:      cv1, cv2, cv3, then (m[j].cv1, m[j].cv2) for j < n        -> 3 + 2n convs
 * SPPF:    cv1, cv2 ; k = pool size
 * Detect:  one 1x1 conv per input level (bias, no activation)        -> n_from convs
 * YOLO11 rows (a depthwise 3x3 conv is an mdhip_conv with c_in = 1, weight [c_out][1][3][3]; every conv carries its
 * folded BatchNorm; "no activation" below = identity, every other conv = SiLU):
 * Conv:    layer 0 may also be Conv(3->c, k=3, s=2, p=1) (the YOLO11 stem)
 * C3k2:    n inner blocks, shortcut, k = 0: Bottleneck blocks, k = 1: C3k blocks (c3k = True).  Convs:
 *          cv1, cv2, then per block j   Bottleneck: m.j.cv1 (3x3), m.j.cv2 (3x3)                          -> 2 + 2n convs
 *                                       C3k: m.j.cv1, m.j.cv2, m.j.cv3 (1x1), m.j.m.0.cv1, m.j.m.0.cv2,
 *                                            m.j.m.1.cv1, m.j.m.1.cv2 (3x3)                               -> 2 + 7n convs
 * C2PSA:   n PSA blocks; cv1, cv2, then per block j: m.j.attn.qkv (1x1, no activation), m.j.attn.proj (1x1, no
 *          activation), m.j.attn.pe (depthwise 3x3, no activation), m.j.ffn.0 (1x1), m.j.ffn.1 (1x1, no
 *          activation)                                                                             -> 2 + 5n convs
 *          (heads = c1 / 128, key_dim 32, head_dim 64: qkv has c1 / 2 + 2 * heads * 32 = c1 outputs)
 * DetectDFL (anchor-free, reg_max 16; na = 1, anchors_px unused and may be NULL), per input level l:
 *          cv2.l.0 (3x3), cv2.l.1 (3x3), cv2.l.2 (1x1, 64 box logits, bias, no activation),
 *          cv3.l.0.0 (depthwise 3x3), cv3.l.0.1 (1x1), cv3.l.1.0 (depthwise 3x3), cv3.l.1.1 (1x1),
 *          cv3.l.2 (1x1, nc class logits, bias, no activation)                                     -> 8 n_from convs
 *          Predictions are [cx, cy, w, h, cls0 .. cls(nc-1)] (4 + nc per anchor, no objectness); mdhip_nms* then apply
 *          the ultralytics rule (conf = largest class score, class offset 7680 in the IoU, 30 000 candidates at most).
 *          mdhip_forward_tta and MDHIP_DTYPE_FP8 return MDHIP_EUNSUPPORTED for such models.
 * YOLOv9-C rows (every Conv carries its folded BatchNorm and SiLU unless noted; SPPELAN is an MDHIP_SPPF row whose cv1
 * has the hidden width c3, convs cv1, cv5):
 * Silence: n_from 1, no convs; the layer's output IS its input.  A Conv whose input is the network input, directly or
 *          through Silence, is a stem (the 3x3 / s2 / p1 form above); a model may have several (yolov9-c.yaml's second
 *          stem, layer 26, reads layer 0).
 * ELAN4:   RepNCSPELAN4(c1, c2, c3, c4, n): cv1 (1x1 -> c3), then RepNCSP(c3 / 2 -> c4) cv2.0.cv1, cv2.0.cv2 (1x1 -> h),
 *          cv2.0.cv3 (1x1 2h -> c4), per j < n cv2.0.m.j.cv1 (3x3: RepConvN folded, the 1x1 branch at the centre tap),
 *          cv2.0.m.j.cv2 (3x3, + residual); cv2.1 (3x3 c4 -> c4); the same for cv3.0 (RepNCSP c4 -> c4) and cv3.1;
 *          cv4 (1x1 c3 + 2 c4 -> c2)                                                                  -> 10 + 4n convs
 *          (h = c4 / 2; lowered on ONE buffer [cv1 | cv2 | cv3] that cv4 reads)
 * ADown:   cv1 (3x3 / s2 / p1, c1 / 2 -> c2 / 2) over avg_pool2d(2, s1) of the first input half, cv2 (1x1, c1 / 2 ->
 *          c2 / 2) over max_pool2d(3, 2, 1) of avg_pool2d(2, s1) of the second half; output [cv1 | cv2] at half size
 *                                                                                                            -> 2 convs
 * CBLinear: one 1x1 conv (bias, NO activation) to the sum of the splits; c_out = that sum                  -> 1 conv
 * CBFuse:  from[0 .. n_from-2] CBLinear layers (1 to 3), from[n_from-1] the tensor they are added to; k, s, p = the
 *          channel offset of the chosen split in from[0], from[1], from[2] (the split has the channels of the last
 *          input); each split is nearest-resized to the last input's size (integer factors) and the sum is
 *          ((s0 + s1) + s2) + last in fp32, rounded once                                                 -> 0 convs
 * DetectDDFL (DDetect, reg_max 16; na = 1, anchors_px unused): n = heads in the conv table (1 DDetect, 2 DualDDetect),
 *          k = the head that runs (0 = cv2 / cv3 over the first nl inputs; yolov9's NMS keeps DualDDetect's first
 *          output), from[] = that head's nl inputs; per head h, per level l (head 1: cv4 / cv5):
 *          cv2.l.0 (3x3 -> c2), cv2.l.1 (3x3, GROUPED g = 4: weight [c2][c2 / 4][3][3]), cv2.l.2 (1x1, 64 box logits,
 *          bias, no activation), cv3.l.0 (3x3 -> c3), cv3.l.1 (3x3), cv3.l.2 (1x1, nc class logits, bias, no
 *          activation)                                                                          -> 6 nl n convs
 *          Predictions and NMS as for DetectDFL. */
typedef struct {
    int32_t type;
    int32_t n_from;
    int32_t from[4];
    int32_t c_out;
    int32_t k, s, p;
    int32_t n;
    int32_t shortcut;
    int32_t first_conv;
} mdhip_layer;

typedef struct {
    int32_t n_layers;
    const mdhip_layer* layers;
    int32_t n_convs;
    const mdhip_conv* convs;
    int32_t nc;                 /* classes (3 for MDv5)                         */
    int32_t na;                 /* anchors per level (3)                        */
    int32_t nl;                 /* detection levels (4 for YOLOv5x6)            */
    const float* anchors_px;    /* host, [nl][na][2] = Detect.anchors * stride  */
    const float* strides;       /* host, [nl]                                   */
} mdhip_model;

/* Letterbox geometry of one image, computed on the host exactly as
 * yolov5 letterbox() does (restated at pytorch_detector.py:434-454). */
typedef struct {
    int32_t src_h, src_w;           /* original image                                   */
    int32_t resized_h, resized_w;   /* new_unpad: size after cv2.resize                  */
    int32_t top, left;              /* border offsets (copyMakeBorder, value 114)       */
    int32_t interp;                 /* 0 = cv2.INTER_LINEAR (yolov5 letterbox; 'modern' growing),
                                     * 1 = cv2.INTER_AREA ('modern' shrinking, pytorch_detector.py:1048-1062) */
} mdhip_letterbox;

typedef struct mdhip_ctx mdhip_ctx;

/* Replaces PTDetector.__init__/_load_model (pytorch_detector.py:745-959): packs weights to
 * the MFMA operand layout, plans and allocates every activation buffer for up to
 * max_batch images of max_h x max_w letterboxed pixels on GPU `device`. */
int mdhip_create(const mdhip_model* model, int device, int dtype,
                 int max_batch, int max_h, int max_w, mdhip_ctx** out);
/* A context WITHOUT a model, for work that only touches images (marking a results file and writing its review folder load no
 * detector): every image entry point works on it -- mdhip_jpeg_*, mdhip_blur_regions, mdhip_resample_lanczos, mdhip_draw_ops,
 * mdhip_draw_ops_from, mdhip_classifier_input, mdhip_thumbnails, mdhip_change_detect (and its hook mdhip_label_regions_on), mdhip_gray_count -- and every entry point that needs the plan or the weights (mdhip_preprocess*,
 * the forwards, mdhip_nms*, mdhip_read_*, mdhip_calibrate and the fp8 calls, the op / cfg / tuned / fuse / option / graph /
 * timing calls, the mdhip_*_on kernel hooks) returns MDHIP_EINVAL with a text in mdhip_last_error.  It owns nothing on the
 * device until a call needs scratch.  mdhip_destroy frees it. */
int mdhip_create_images(int device, mdhip_ctx** out);
void mdhip_destroy(mdhip_ctx* ctx);
const char* mdhip_last_error(mdhip_ctx* ctx);

/* Replaces letterbox() + HWC->CHW + float() + /255 (pytorch_detector.py:1104-1109,
 * :1283-1310).  images[i]: HWC uint8 RGB, src_h x src_w, host or device memory
 * (host images are copied to a device staging area first).  Output: the context's network input,
 * n x out_h x out_w.  out_h/out_w must be multiples of the model's largest stride.
 * Device images: the kernels read whole aligned dwords, so for an image pointer (or row pitch src_w * 3) that is not a
 * multiple of 4 up to 3 bytes in front of the first and behind the last pixel are READ (never used, never written): they
 * lie in the same aligned dword as an image byte, i.e. inside any hipMalloc'ed block that holds the image, but a
 * memory checker that tracks exact extents will report them.  (MDHIP_LETTERBOX_GENERAL in the environment at
 * mdhip_create selects the byte-wise kernel for every batch.)
 * Streams: the call may be enqueued on another stream than the forwards -- it first makes its stream wait
 * (hipStreamWaitEvent, inside the library) for the last mdhip_forward / mdhip_forward_tta enqueued before it to have read
 * the network input (the stem), so the letterbox of batch i + 1 can run next to the rest of forward i; the forward of
 * batch i + 1 must then be ordered behind this call by the caller (an event), as bench.py and the detector do. */
int mdhip_preprocess(mdhip_ctx* ctx, const uint8_t* const* images, const mdhip_letterbox* geom,
                     int n, int out_h, int out_w, void* hip_stream);

/* mdhip_preprocess for sources that are WINDOWS of larger device images (tiles of an aerial image, ...): the parent image is
 * uploaded once and every tile of it is cut, resampled and normalised on the device.
 *   windows[i]   device pointer to the window's first pixel (parent + y0 * pitch + x0 * 3); a host pointer is MDHIP_EINVAL
 *   geom[i]      src_h / src_w = the WINDOW's size: geometry, and the clamping of the interpolation at the window's edge,
 *                are those of a dense image of that size (crop first, resize afterwards)
 *   pitches[i]   bytes between two rows of the parent (>= src_w * 3)
 *   readable[i]  bytes readable from windows[i] to the end of the parent allocation (>= (src_h - 1) * pitch + src_w * 3).
 *                The streaming kernels read whole aligned dwords around what they use; inside the parent that only touches
 *                neighbouring pixels, and no read reaches behind the aligned dword that holds byte readable[i] - 1.
 * Streams, the wait for the previous forward's stem and the bookkeeping for mdhip_forward are those of mdhip_preprocess;
 * the network input it leaves is the same, bit for bit, as mdhip_preprocess leaves for the contiguous copy of each window. */
int mdhip_preprocess_windows(mdhip_ctx* ctx, const uint8_t* const* windows, const mdhip_letterbox* geom,
                             const int64_t* pitches, const int64_t* readable, int n, int out_h, int out_w, void* hip_stream);

/* Replaces self.model(batch)[0] (pytorch_detector.py:1313): conv stack + Detect decode.
 * Leaves (n, n_anchors, 5+nc) fp32 predictions in a device buffer of the context (4+nc for an anchor-free model). */
int mdhip_forward(mdhip_ctx* ctx, int n, int h, int w, void* hip_stream);

/* GPU half of JPEG decoding (the reference decodes with PIL on the host, visualization_utils.py:103-175; the host half here is
 * libmdjpeg.so, include/mdjpeg.h): rebuilds from the QUANTISED DCT coefficients of a baseline JPEG the RGB pixels that
 * Pillow / libjpeg-turbo produce, bit for bit -- de-quantisation, the "islow" integer inverse DCT, "fancy" chroma
 * upsampling, fixed-point YCbCr -> RGB, and the EXIF rotation -- into device memory that mdhip_preprocess then reads.
 * The inverse DCT's results are SATURATED to 0 .. 255, as libjpeg-turbo's SIMD code packs them; libjpeg's C code indexes a
 * range-limit table with (sample - 128) & 1023 instead, which wraps around for samples outside [-512, 511].  Planes that
 * mdjpeg_decode accepts can hold such samples (its energy bound admits a block whose whole norm sits in one sample), and
 * for them the pixels are those of a Pillow whose libjpeg saturates.  quant entries may use all 16 bits.
 *   coef        DEVICE pointer, 16-byte aligned: the planes of Y[, Cb, Cr] one behind the other exactly as mdjpeg_decode
 *               writes them (plane c: [blocks_h[c]][blocks_w[c]][64], natural order within a block)
 *   width, height   of the image before rotation;  components 1 (grayscale: R = G = B = Y) or 3
 *   h_samp, v_samp  luma sampling factors: (1, 1) 4:4:4 and grayscale, (2, 1) 4:2:2, (2, 2) 4:2:0; chroma is 1 x 1
 *   blocks_w / blocks_h   plane sizes in 8x8 blocks (whole MCUs: mdjpeg_info says them)
 *   quant       quantisation table of each component, natural order
 *   rotation    0 / 90 / 180 / 270 counter-clockwise, as PIL's rotate(angle, expand = True) turns
 * out_rgb[i]: device memory for the rotated image, H x W x 3 bytes (W x H x 3 for 90 / 270), written completely.
 * The u8 component planes between the two kernels live in scratch memory of the context that grows on demand (the device
 * is synchronised when it does): keep all mdhip_jpeg_reconstruct calls of one context on ONE stream. */
typedef struct {
    const int16_t* coef;
    int32_t  width, height, components;
    int32_t  h_samp, v_samp;
    int32_t  blocks_w[3], blocks_h[3];
    int32_t  rotation;
    uint16_t quant[3][64];
} mdhip_jpeg_image;
int mdhip_jpeg_reconstruct(mdhip_ctx* ctx, const mdhip_jpeg_image* images, int n, uint8_t* const* out_rgb, void* hip_stream);

/* Entropy decoding of baseline JPEG scans on the GPU: from the compressed scan of each of n files to the quantised
 * coefficient planes mdhip_jpeg_reconstruct takes, in the layout of mdjpeg_decode (include/mdjpeg.h), so that the loaders
 * decode no Huffman symbol at all.  Self-synchronising decoding: every restart segment (or the whole scan) is cut into
 * subsequences of subseq_bits bits (0 = 1024; a multiple of 8, at least 64) that are decoded in parallel, speculatively
 * first and again until each starts where its left neighbour ended; one launch grid per pass holds the whole batch.
 *   scan         DEVICE pointer: the file's bytes [desc->scan_begin, desc->scan_end)
 *   desc         host: what mdjpeg_scan returned for the file
 *   seg_offsets  host: the desc->n_segments offsets mdjpeg_scan wrote
 *   coef         DEVICE pointer, 16-byte aligned: receives desc->info.coef_count values
 *   status[i]    host: 0, and coef holds exactly what mdjpeg_decode writes; or a mask of MDHIP_JPEG_* bits for exactly the
 *                files mdjpeg_decode answers with MDJPEG_ECORRUPT, and coef holds nothing of use (decode that file with
 *                the ordinary decoder).  Only lanes that start from verified states flag.
 * No byte outside a scan's range is read and no value outside coef_count written, whatever the bytes say.  A descriptor
 * whose ranges contradict each other, a host pointer or n < 1 is MDHIP_EINVAL.  The call returns when the planes are
 * written (it reads the statuses back).  Scratch grows on demand; stream rule as mdhip_jpeg_reconstruct. */
#define MDHIP_JPEG_ECODE      1     /* undefined Huffman code                                           */
#define MDHIP_JPEG_ECATEGORY  2     /* DC / AC magnitude category a baseline file cannot hold           */
#define MDHIP_JPEG_EINDEX     4     /* coefficient index past 63, zero run leaving the block            */
#define MDHIP_JPEG_EEARLY     8     /* data end early                                                   */
#define MDHIP_JPEG_ELEFTOVER  16    /* bytes left over in front of a marker                             */
#define MDHIP_JPEG_ECOUNT     32    /* a segment does not hold exactly its MCUs                         */
#define MDHIP_JPEG_EENERGY    64    /* block energy beyond what 8-bit samples can hold                  */
#define MDHIP_JPEG_EDC        128   /* DC value out of range                                            */
typedef struct {
    const uint8_t*          scan;
    const mdjpeg_scan_info* desc;
    const uint32_t*         seg_offsets;
    int16_t*                coef;
} mdhip_jpeg_scan;
int mdhip_jpeg_entropy_decode(mdhip_ctx* ctx, const mdhip_jpeg_scan* scans, int n, int subseq_bits, int32_t* status, void* hip_stream);
/* of the last mdhip_jpeg_entropy_decode: subsequences, subsequences decoded again in pass 2, pass-2 launches, images */
int mdhip_jpeg_entropy_stats(mdhip_ctx* ctx, int64_t out[4]);

/* JPEG recompression of windows of device images (the reference writes every tile of run_tiled_inference.py as a quality-95
 * JPEG and detects on the decoded file, run_tiled_inference.py:54,262): out_rgb[i] receives the pixels that Pillow /
 * libjpeg-turbo give for Image.save(<window i>, quality = q) followed by Image.open, bit for bit, without a file, a host
 * copy or an entropy coder.  The encoder's lossy half in libjpeg's integer arithmetic -- fixed-point RGB -> YCbCr, edges
 * replicated to whole blocks, h2v2 chroma down-sampling (three components, 4:2:0: what Pillow writes for RGB input with
 * default settings), the "islow" forward DCT, quantisation rounding half away from zero -- then mdhip_jpeg_reconstruct's
 * de-quantisation, inverse DCT, fancy upsampling and colour conversion.
 *   windows[i]   device pointer to the window's first pixel (parent + y0 * pitch + x0 * 3), as for mdhip_preprocess_windows;
 *                a host pointer is MDHIP_EINVAL.  Only bytes of the window are read: no aligned over-read, no `readable`.
 *   widths[i], heights[i]   the window's size in pixels, 1 .. 65535 each, any value (no multiple of 8 or 16 is needed)
 *   pitches[i]   bytes between two rows of the parent (>= widths[i] * 3)
 *   quant_luma, quant_chroma   HOST pointers: the encoder's tables, natural order, entries 1 .. 255 (for a Pillow quality:
 *                the standard's tables under libjpeg's quality scaling; megadetector_amd/jpeg_host.py quant_tables)
 *   out_rgb[i]   device memory of heights[i] x widths[i] x 3 bytes, written completely; it must not overlap the window
 * Scratch and streams are those of mdhip_jpeg_reconstruct (the two calls share the scratch): one stream per context. */
int mdhip_jpeg_recompress(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                          const int64_t* pitches, int n, const uint16_t quant_luma[64], const uint16_t quant_chroma[64],
                          uint8_t* const* out_rgb, void* hip_stream);

/* Entropy ENCODING of windows of device images (the reference cuts every detection out of a second PIL decode of the file and
 * saves it as a quality-95 JPEG, postprocessing/create_crop_folder.py): for each of n windows the entropy-coded scan of the
 * file Image.fromarray(window).save(f, 'JPEG', quality = q) writes, byte for byte -- every byte between the SOS header and
 * the EOI marker.  mdhip_jpeg_recompress's lossy half (same arithmetic, same statements), then a baseline Huffman encoder:
 * three components, 4:2:0, one interleaved scan without restart markers, the standard's four tables (what Pillow emits
 * without `optimize`), DC differences along the MCU order, FF bytes stuffed with 00, the last byte padded with 1-bits (and
 * stuffed when that makes it FF).  The bytes in front of and behind the scan depend on size and quality only
 * (megadetector_amd/jpeg_host.py jfif_file).  One launch grid per pass for the whole batch.
 *   windows, widths, heights, pitches, quant_luma, quant_chroma   as for mdhip_jpeg_recompress; at most 2^21 blocks a window
 *   out, capacity   ONE caller-owned DEVICE buffer of `capacity` bytes (out may be NULL when capacity is 0)
 *   offsets, sizes  HOST arrays of n values: window i's scan lies at out[offsets[i]], sizes[i] bytes; the scans lie one behind
 *                   the other in the order of the windows
 *   needed          HOST: the capacity this call needs
 * MDHIP_ECAPACITY when *needed > capacity: nothing is written at or beyond out[capacity], offsets / sizes / *needed are valid,
 * and the same call with a buffer of *needed bytes succeeds -- so a caller retries once.  mdhip_jpeg_encode_bound(w, h) is
 * a capacity that always suffices for one window, derived from the worst code lengths of the standard tables and not from
 * a trial: a block costs at most 11 + 11 bits of DC and 63 x (16 + 10) bits of AC = 1660 bits, a window pads at most 7
 * bits, and stuffing at most doubles the bytes: 8 x (52 x blocks + 1) bytes, blocks = 6 x ((w + 15) / 16) x ((h + 15) / 16);
 * -1 for a size outside 1 .. 65535.  Typical scans take a few per cent of it.
 * The call returns when the scans are written (it reads sizes and statuses back, once).  Scratch grows on demand (the
 * device is synchronised when it does): keep all mdhip_jpeg_encode calls of one context on ONE stream. */
int mdhip_jpeg_encode(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                      const int64_t* pitches, int n, const uint16_t quant_luma[64], const uint16_t quant_chroma[64], uint8_t* out,
                      int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, void* hip_stream);
long long mdhip_jpeg_encode_bound(int width, int height);

/* mdhip_jpeg_encode with the chroma sampling and the quantisation tables of EACH window (the reference's
 * exif_preserving_save(quality = 'keep') makes Pillow re-encode an RGB JPEG with the source file's own tables and its own
 * sampling, postprocessing/separate_detections_into_folders.py): window i's scan is, byte for byte, the scan of
 * Image.fromarray(window).save(f, 'JPEG', qtables = [luma, chroma], subsampling = samplings[i]).  The same kernels, the same
 * passes and the same contract as mdhip_jpeg_encode, which is this call with MDHIP_JPEG_H2V2 and one pair for all windows.
 *   samplings   HOST array of n values, numbered as Pillow's `subsampling`:
 *                 MDHIP_JPEG_H1V1 (4:4:4)  MCU  8 x 8,   3 blocks  Y Cb Cr;          chroma as it is (fullsize_downsample)
 *                 MDHIP_JPEG_H2V1 (4:2:2)  MCU 16 x 8,   4 blocks  Y0 Y1 Cb Cr;      pairs along a row, bias 0, 1, 0, 1 ...
 *                                          (h2v1_downsample), the right edge replicated before
 *                 MDHIP_JPEG_H2V2 (4:2:0)  MCU 16 x 16,  6 blocks  Y00 Y01 Y10 Y11 Cb Cr, as mdhip_jpeg_encode
 *               (libjpeg's jcsample.c, statement for statement); dummy blocks at the right and bottom edge and the DC
 *               prediction along the MCU order follow the window's own layout
 *   quant       HOST array of n pairs of tables, [n][2][64]: window i's luma table, then its chroma table, natural order,
 *               every entry 1 .. 255
 * A sampling outside 0 .. 2 or a table entry outside 1 .. 255 is MDHIP_EINVAL, and nothing is launched.
 * mdhip_jpeg_encode_sampled_bound(w, h, sampling) is a capacity that always suffices for one window, derived as
 * mdhip_jpeg_encode_bound is: 1660 bits a block at most whatever the sampling (the code lengths are the tables', not the
 * layout's), 7 bits of padding, every byte stuffed: 8 x (52 x blocks + 1) bytes with
 * blocks = (hs x vs + 2) x ((w + 8 hs - 1) / (8 hs)) x ((h + 8 vs - 1) / (8 vs)), (hs, vs) = (1, 1), (2, 1), (2, 2);
 * -1 for a size outside 1 .. 65535 or a sampling outside 0 .. 2.  For h2v2 it is mdhip_jpeg_encode_bound(w, h). */
#define MDHIP_JPEG_H1V1 0
#define MDHIP_JPEG_H2V1 1
#define MDHIP_JPEG_H2V2 2
int mdhip_jpeg_encode_sampled(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                              const int64_t* pitches, const int32_t* samplings, int n, const uint16_t* quant, uint8_t* out,
                              int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, void* hip_stream);
long long mdhip_jpeg_encode_sampled_bound(int width, int height, int sampling);

/* mdhip_jpeg_encode_sampled for copies in which only rectangles changed (boxes drawn, people blurred): the blocks of every
 * MCU that no changed rectangle touches are the SOURCE file's own quantised coefficients, so outside the rectangles the copy
 * is the source and not a re-encode of its decoded pixels.  No reference behaviour: the reference re-encodes the whole copy.
 *   sources[i]   window i's source: coef, a DEVICE pointer, 16-byte aligned, to its quantised planes in the layout of
 *                mdjpeg_decode (what mdhip_jpeg_entropy_decode leaves behind): plane c is [blocks_h[c]][blocks_w[c]][64],
 *                natural order, Y then Cb then Cr one behind the other; blocks_w / blocks_h must be the window's whole MCUs for
 *                its sampling: Y mcus_x * hs x mcus_y * vs, Cb and Cr mcus_x x mcus_y
 *   rect_image, rects, n_rects   the changed rectangles: rectangle i lies in window rect_image[i] and is rects[4 i .. 4 i + 3] =
 *                left, top, right, bottom in pixels, right and bottom exclusive (mdhip_blur_regions' convention)
 *   status       HOST array of n values: 0, or 1 for a window whose merged blocks no baseline scan holds (below)
 * Rules:
 *   clipping     a rectangle is clipped to its window; one without area after that is dropped
 *   changed MCU  the MCU is 8 hs x 8 vs pixels, (hs, vs) from the window's sampling; MCU (mx, my) is CHANGED iff some rectangle
 *                of its window has left < (mx + 1) * 8 hs, right > mx * 8 hs, top < (my + 1) * 8 vs and bottom > my * 8 vs
 *   blocks       of a changed MCU: exactly those mdhip_jpeg_encode_sampled computes from the window's pixels; of every other
 *                MCU: the source's -- Y block (my * vs + dy, mx * hs + dx), Cb and Cr block (my, mx) -- value for value, the
 *                dummy blocks of edge MCUs included (the scan codes a dummy luma block as libjpeg does whatever it holds)
 *   entropy      the passes of mdhip_jpeg_encode_sampled over the merged blocks: DC differences run along the merged planes
 * A source DC beside a recomputed one can differ by more than the 11 bits a baseline DC code holds: the decoder lets a
 * source DC d through when (d * q0)^2 stays below its energy bound, which is at least 1029^2, a black block re-encodes to
 * -1024 / q0, so with q0 = 1 a difference of 2053 > 2047 is legal input.  Such a window -- and one whose source planes hold
 * an AC value beyond 10 bits, which no decoded file does -- gets status 1 and a scan of size 0; the scans of the other
 * windows are what they are without it and lie one behind the other as always.  The caller re-encodes that copy whole.
 * MDHIP_EINVAL, and nothing is launched: a host pointer or a misaligned one for the planes, plane sizes that are not the
 * window's whole MCUs, a rectangle naming a window outside 0 .. n - 1, and everything mdhip_jpeg_encode_sampled refuses.
 * Capacity, *needed, MDHIP_ECAPACITY (status is valid then too), streams and scratch as mdhip_jpeg_encode_sampled;
 * mdhip_jpeg_encode_sampled_bound still bounds a window: a block's worst case does not depend on where its values came from. */
typedef struct {
    const int16_t* coef;
    int32_t blocks_w[3], blocks_h[3];
} mdhip_jpeg_source;
int mdhip_jpeg_encode_kept(mdhip_ctx* ctx, const uint8_t* const* windows, const int32_t* widths, const int32_t* heights,
                           const int64_t* pitches, const int32_t* samplings, int n, const uint16_t* quant,
                           const mdhip_jpeg_source* sources, const int32_t* rect_image, const int32_t* rects, int n_rects, uint8_t* out,
                           int64_t capacity, int64_t* offsets, int64_t* sizes, int64_t* needed, int32_t* status, void* hip_stream);

/* Gaussian blur of rectangles of device images, IN PLACE (the reference blurs people in the image copies it writes:
 * postprocessing/separate_detections_into_folders.py --category_names_to_blur, visualization_utils.blur_detections: per box
 * crop -> ImageFilter.GaussianBlur(40) -> paste): every rectangle becomes, bit for bit, what Pillow's GaussianBlur(radius)
 * makes of it -- three passes of an extended box filter along x, then three along y, 32-bit integers with an 8-bit
 * rounding behind every pass, the RECTANGLE's edges replicated (csrc/blur_box.h, shared with the host model
 * mdjpeg_blur_regions).  Running sums: the cost follows the pixels, not pixels x box length.
 *   images, widths, heights, pitches   n_images DEVICE images, 8 bits a sample, R G B interleaved, pitches[i] bytes a row
 *                                      (>= 3 * widths[i], any value: 3 * width is fine); every access is a single byte, so
 *                                      nothing beside a rectangle is read or written; sizes 1 .. 65535, below 2 GB
 *   rect_image, rects, n_rects         rectangle i lies in image rect_image[i] and is rects[4 i .. 4 i + 3] = left, top,
 *                                      right, bottom in pixels, right and bottom exclusive.  The rectangles of ONE image
 *                                      are applied in the order of the list, each to what the earlier ones left (so
 *                                      overlapping rectangles interact as they do in the reference); rectangles of
 *                                      different images run side by side: launch round k takes the k-th rectangle of
 *                                      every image.  A rectangle without area (right <= left or bottom <= top) is
 *                                      skipped, as Pillow pastes nothing for it; any other that leaves its image is
 *                                      MDHIP_EINVAL, and then nothing has been launched.
 *   radius                             of the Gaussian, 0 .. 512 (0 changes nothing); 40 in the reference
 * The call only enqueues (two launches per round).  Scratch -- two planes per rectangle of the largest round -- grows on
 * demand (the device is synchronised when it does): keep all mdhip_blur_regions calls of one context on ONE stream. */
int mdhip_blur_regions(mdhip_ctx* ctx, uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                       int n_images, const int32_t* rect_image, const int32_t* rects, int n_rects, float radius, void* hip_stream);

/* Annotated previews of device images (the reference's visualization/visualize_detector_output.py: resize to 1000 pixels
 * wide with Pillow's LANCZOS filter, then render_detection_bounding_boxes), from the image that is in device memory already.
 *
 * mdhip_resample_lanczos makes of every source what Pillow's Image.resize((dst_width, dst_height), LANCZOS) makes of it,
 * bit for bit (csrc/resample.h, shared with the host model mdjpeg_resample): per axis whose size changes, the horizontal one
 * first, a weighted sum of the taps within 3 max(scale, 1) samples of the output sample's centre; weights in double,
 * normalised, rounded to 22 fractional bits; 32-bit integer sums, rounded and clipped to 8 bits behind each pass.  An axis
 * whose size stays is not resampled; an image whose size stays is copied.
 *   src, widths, heights, pitches               n DEVICE images, 8 bits a sample, R G B interleaved, pitches[i] bytes a row
 *                                               (>= 3 * widths[i], any value); sizes 1 .. 65535, below 2 GB
 *   dst, dst_widths, dst_heights, dst_pitches   the n destinations, likewise; they must not overlap the sources.  Nothing
 *                                               beside the 3 * dst_widths[i] bytes of each of their rows is written.
 * One launch per pass for the whole batch.  The coefficient tables are computed here, once per distinct (in, out) pair of the
 * batch.  MDHIP_EUNSUPPORTED when the taps of one output pixel of a row do not fit on chip (a row reduced more than about
 * 1800 times); nothing has been enqueued then.  The call only enqueues.  Scratch -- tables and the 8-bit images between the
 * passes (heights[i] x dst_widths[i]) -- belongs to the context and grows on demand (the device is synchronised when it
 * does): keep all mdhip_resample_lanczos and mdhip_draw_ops calls of one context on ONE stream. */
int mdhip_resample_lanczos(mdhip_ctx* ctx, const uint8_t* const* src, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                           int n, uint8_t* const* dst, const int32_t* dst_widths, const int32_t* dst_heights, const int64_t* dst_pitches,
                           void* hip_stream);

/* mdhip_draw_ops applies to each image its ordered list of drawing operations, IN PLACE and in one launch: a pixel takes
 * the value of the LAST operation of its image's list that covers it (the host model: mdjpeg_draw).
 *   images, widths, heights, pitches   n_images DEVICE images as above
 *   op_image, ops, n_ops               operation i belongs to image op_image[i] and is the 8 int32 ops[8 i .. 8 i + 7]:
 *                                        [0, x0, y0, x1, y1, colour, 0, 0]  a solid rectangle, x0 .. x1 and y0 .. y1 INCLUSIVE,
 *                                                                           colour = R | G << 8 | B << 16
 *                                        [1, x, y, w, h, offset, 0, 0]      the paste of w x h pixels (R G B, 3 w bytes a row)
 *                                                                           that begin at byte `offset` of `patches`, their
 *                                                                           top left corner at (x, y); w, h <= 32767
 *                                      Both are clipped to the image (coordinates may be negative or beyond it).  The
 *                                      operations of one image keep the order of the list; those of different images may
 *                                      be interleaved.
 *   patches, patch_bytes               ONE packed DEVICE buffer with the pixels of all patches, and its size
 * MDHIP_EINVAL, with nothing launched and no image changed, for an operation that names an image outside 0 .. n_images - 1,
 * an unknown kind, or a patch that is not wholly inside `patches`.  The call only enqueues; see above for the stream. */
int mdhip_draw_ops(mdhip_ctx* ctx, uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                   int n_images, const int32_t* op_image, const int32_t* ops, int n_ops, const uint8_t* patches, int64_t patch_bytes,
                   void* hip_stream);

/* mdhip_draw_ops_from is the fan-out form of mdhip_draw_ops: it MAKES n_dst destination images out of n_src source images,
 * in one launch, and leaves the sources as they are -- for a source that several renderings draw on (compare_batch_results:
 * one decoded and resampled file, one rendering per comparison).  A pixel of a destination takes the value of the LAST
 * operation of the destination's list that covers it, or else its source's pixel (the host model: mdjpeg_draw_from).
 *   src, widths, heights, pitches    n_src DEVICE images as above; only read
 *   dst, dst_src, dst_pitches        n_dst DEVICE images: destination i has the size of source dst_src[i] (many destinations
 *                                    may name one source) and dst_pitches[i] bytes a row (>= 3 * width, any value).  Exactly
 *                                    the 3 * width bytes of each of its rows are written.  A destination without an
 *                                    operation is a copy of its source.
 *   op_image, ops, n_ops, patches, patch_bytes   as for mdhip_draw_ops; op_image[i] names a DESTINATION
 * MDHIP_EINVAL, with nothing launched and nothing written, for what mdhip_draw_ops refuses, for a dst_src[i] outside
 * 0 .. n_src - 1, and for a destination that shares a byte (from its first pixel to the end of its last row) with a source or
 * with another destination.  The call only enqueues; its scratch is that of mdhip_draw_ops: same stream. */
int mdhip_draw_ops_from(mdhip_ctx* ctx, const uint8_t* const* src, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                        int n_src, uint8_t* const* dst, const int32_t* dst_src, const int64_t* dst_pitches, int n_dst, const int32_t* op_image,
                        const int32_t* ops, int n_ops, const uint8_t* patches, int64_t patch_bytes, void* hip_stream);

/* The input of a species classifier for n detections of a batch, from the images that are in device memory already (the
 * reference: classification/crop_detections.py save_crop writes a crop file per detection, classification/run_classifier.py
 * reads it back and applies Resize(size, BICUBIC), CenterCrop(size), ToTensor, Normalize): ONE launch takes every crop from
 * its image to out[i] = fp32 [3][size][size], bit for bit what those steps give for the same pixels (csrc/resample.h, shared
 * with the host model mdjpeg_classifier_input).
 * A crop is a CANVAS of canvas_w x canvas_h pixels: the rectangle src_w x src_h at (off_x, off_y) holds image pixels, the
 * rest is 0 (a box that leaves its image, or one padded to a square).  The canvas is resized with Pillow's arithmetic --
 * the shorter side to `size`, the longer to int(size * longer / shorter); integer weights of 22 bits, 8 bits between the
 * horizontal and the vertical pass, an axis whose size stays is not resampled -- the size x size centre is kept (offsets
 * int(round((n - size) / 2)), a half to the even neighbour), and a byte v of channel c becomes
 * ((float)v / 255 - mean[c]) / std[c], from a table computed on the host in fp32.  Only that centre is computed, and the
 * canvas is never built: a tap outside the rectangle contributes 0.
 *   crops, n     n records (HOST memory), 0 .. 65535; the pixels they name are DEVICE memory, R G B interleaved
 *   size         1 .. 4096
 *   filter       0 bicubic (the reference), 1 bilinear, 2 LANCZOS: Pillow's filters of those names
 *   mean, std    per channel; std != 0
 *   out          DEVICE, n * 3 * size * size floats; nothing else is written, no source is changed
 * MDHIP_EINVAL, with nothing enqueued, for a host pointer, a rectangle that leaves its canvas, sizes outside the ranges, an
 * unknown filter or a std of 0.  MDHIP_EUNSUPPORTED, with nothing enqueued, when the canvas rows one output row needs do not
 * fit on chip even for a single column (a canvas reduced more than about 1800 times with LANCZOS, 2700 with bicubic); the
 * caller makes that crop on the host.  The call only enqueues.  Scratch -- the float table, the records and the
 * coefficient tables -- belongs to the context and grows on demand (the device is synchronised when it does): keep all
 * mdhip_classifier_input calls of one context on ONE stream. */
typedef struct {
    const uint8_t* src;          /* DEVICE: first image pixel that lies in the canvas           */
    int64_t  pitch;              /* bytes a row of the image (>= 3 * src_w, any value)          */
    int32_t  src_w, src_h;       /* the part of the canvas that holds image pixels, >= 1        */
    int32_t  canvas_w, canvas_h; /* 1 .. 65535                                                  */
    int32_t  off_x, off_y;       /* where that part lies in the canvas; the rest of it is 0     */
} mdhip_classifier_crop;
int mdhip_classifier_input(mdhip_ctx* ctx, const mdhip_classifier_crop* crops, int n, int size, int filter, const float mean[3],
                           const float std[3], float* out, void* hip_stream);

/* Thumbnails: n tiles go from images in device memory to their places in sheets in device memory, in ONE launch (the
 * reference: visualization_utils.render_images_with_thumbnails, which for every tile opens a file, crops, resizes and
 * pastes -- the grid of a sample of the repeat-detection review folder).  Tile i is, bit for bit, what Pillow gives for
 * image.crop(box).resize((out_w, out_h), filter) followed by sheet.paste(tile, (x, y)): the crop is a CANVAS as for
 * mdhip_classifier_input (the rectangle src_w x src_h at (off_x, off_y) holds image pixels, the rest is 0, as Image.crop fills
 * where the box leaves the image), the canvas is resized to out_w x out_h with Pillow's arithmetic (the horizontal pass
 * first, weights normalised and rounded to 22 bits, 32-bit sums clipped to 8 bits behind each pass, an axis whose size stays
 * is not resampled, a tile whose size stays is a copy), and its bytes are stored R G B interleaved at dst, dst_pitch bytes a
 * row.  The canvas is never built: a tap outside the rectangle contributes 0, but bounds and weights are the canvas's
 * (csrc/resample.h, shared with the host model mdjpeg_thumbnails).
 *   tiles, n     n records (HOST memory), 0 .. 65535; the pixels they name are DEVICE memory
 *   filter       0 bicubic (Image.resize's default for RGB), 1 bilinear, 2 LANCZOS
 * Only the 3 * out_w bytes of each of a tile's out_h rows are written; no source is changed.  The tiles of one call must not
 * overlap each other or a source (the caller's guarantee).
 * MDHIP_EINVAL, with nothing enqueued, for a host or NULL pixel pointer, a rectangle that leaves its canvas, a canvas or
 * output size outside 1 .. 65535, a dst_pitch below 3 * out_w or an unknown filter.  MDHIP_EUNSUPPORTED, with nothing
 * enqueued, when the canvas rows one output row needs do not fit on chip even for a single column (a canvas reduced more than
 * about 2700 times with bicubic); the caller makes that tile on the host.  The call only enqueues.  Scratch -- the records
 * and the coefficient tables -- belongs to the context (it shares mdhip_classifier_input's) and grows on demand (the device is
 * synchronised when it does): keep these calls of one context on ONE stream. */
typedef struct {
    const uint8_t* src;          /* DEVICE: first image pixel that lies in the canvas           */
    int64_t  pitch;              /* bytes a row of the image (>= 3 * src_w, any value)          */
    int32_t  src_w, src_h;       /* the part of the canvas that holds image pixels; either 0:   */
                                 /* none (a box wholly outside its image), src is not read      */
    int32_t  canvas_w, canvas_h; /* 1 .. 65535                                                  */
    int32_t  off_x, off_y;       /* where that part lies in the canvas; the rest of it is 0     */
    int32_t  out_w, out_h;       /* the tile, 1 .. 65535                                        */
    uint8_t* dst;                /* DEVICE: the tile's first pixel in its sheet                 */
    int64_t  dst_pitch;          /* bytes a row of the sheet (>= 3 * out_w)                     */
} mdhip_thumbnail;
int mdhip_thumbnails(mdhip_ctx* ctx, const mdhip_thumbnail* tiles, int n, int filter, void* hip_stream);

/* Repeat-detection elimination (the reference: postprocessing/repeat_detection_elimination/repeat_detections_core.py
 * _find_matches_in_directory and the "Mark suspicious locations" block of find_repeat_detections): which detections of a camera
 * sit where the same camera was boxed again and again.  CONTEXT-FREE: marking a results file needs no model, so the call takes
 * a device index, not a context; its errors are in mdhip_last_error(NULL).
 *   boxes, n     HOST: the detections that take part, of ALL locations, in processing order (images in file order, detections
 *                in list order); `group` is the index of the location, non-decreasing.  0 <= n <= 2^30
 * Boxes are taken in order.  A box MATCHES a candidate of its group when the categories are equal (or category_agnostic is
 * set) and ct_utils.get_iou(box, candidate) >= iou_threshold -- in doubles, operation for operation, the division included
 * (csrc/rde_match.h, shared with the host model mdjpeg_repeat_detections).  It becomes an instance of EVERY candidate it
 * matches; when it matches none it opens a new candidate whose first instance is itself.  Only boxes that matched nothing are
 * ever candidates.  A box get_iou raises for (x + w <= x or y + h <= y, or a NaN) matches nothing and nothing matches it.
 * A candidate with at least occurrence_threshold instances is suspicious.
 *   is_candidate[i]   HOST, n: 1 when box i opened a candidate
 *   n_instances[i]    HOST, n: the instances of the candidate box i opened (itself included), 0 for any other box
 *   pairs, capacity   HOST, capacity x 2: the instance lists of the suspicious candidates, one behind the other, each entry
 *                     (instance, candidate) as indices into boxes; sorted by candidate, then by instance -- the order of the
 *                     reference's lists.  May be NULL when capacity is 0
 *   needed            HOST: the entries this call needs
 *   chunk             boxes resolved per step, 1 .. 16384; 0 = 1024.  No result depends on it (tests put chunk edges into small
 *                     inputs with it)
 * MDHIP_ECAPACITY when *needed > capacity: is_candidate, n_instances and *needed are valid, nothing is written to pairs, and
 * the same call with room for *needed entries succeeds -- so a caller retries once.  MDHIP_EINVAL for n < 0, a group that
 * decreases, a NaN threshold, a chunk or a device outside its range; MDHIP_EHIP "no HIP device" where there is none.
 * Candidates are resolved chunk by chunk in stream order -- per chunk: its rows against the candidates so far, its rows
 * against each other (64-bit match words), one wave that walks them in order -- with no host synchronisation between chunks;
 * then the instances are counted, and written by rank.  The n x n matches are never stored: device memory is
 * O(n + chunk^2 / 8 + pairs), allocated by the call and released before it returns.  The call returns when the results are
 * in host memory. */
typedef mdjpeg_rde_box mdhip_rde_box;      /* { double x, y, w, h; int32_t group, category; } */
int mdhip_repeat_detections(int device, const mdhip_rde_box* boxes, int64_t n, double iou_threshold, int category_agnostic,
                            int32_t occurrence_threshold, int32_t chunk, uint8_t* is_candidate, int32_t* n_instances,
                            int64_t* pairs, int64_t capacity, int64_t* needed);
/* device time of this thread's last mdhip_repeat_detections, from events on its stream, in milliseconds: ms[0] resolving the
 * candidates (all chunks), ms[1] counting the instances, ms[2] writing the pairs (0 when none were written); uploads and
 * read-backs are in none of them (tools/rde_bench.py) */
int mdhip_repeat_detections_times(float ms[3]);

/* Change detection between images that lie in device memory: what the reference's detection/change_detection.py detect_motion
 * (FRAME_DIFF) computes per pair of consecutive images -- gray, region of interest, Gaussian blur, absolute difference,
 * threshold (GLOBAL or OTSU), dilation, connected regions -- with the arithmetic csrc/change_detect.h defines in integers (it is
 * the project's restatement: not verified against OpenCV, and regions are measured by pixel count and listed by label, which
 * cv2.contourArea and cv2.findContours do not do).  The host model is mdjpeg_change_detect (include/mdjpeg.h), whose comment
 * describes every argument; here
 *   ctx                       any context, one of mdhip_create_images included
 *   images, blurred, masks    point to DEVICE memory; every other array is HOST memory, inputs and results alike
 *   blurred, blurred_ready    a caller keeps the plane of a camera's last image and hands it in, ready, with the next call: every
 *                             image is converted and blurred once, not once as "current" and once as "previous"
 * One launch per stage for all images (gray + blur along x, blur along y) and for all pairs of a group (histogram for OTSU,
 * threshold + count, dilation with fused iterations, label init / merge / sums, selection in three launches), pairs of any sizes
 * side by side; a group is as many pairs as fit 1 GiB of scratch (26 bytes a pixel), which belongs to the context and grows on
 * demand.  OTSU's threshold is chosen on the host from the histogram (one extra synchronisation a group).  The call returns when
 * the results are in host memory.  MDHIP_EINVAL as mdjpeg_change_detect, and for a host pointer where device memory is due, more
 * than 65535 images or pairs; nothing is launched then. */
typedef mdjpeg_change_options mdhip_change_options;
int mdhip_change_detect(mdhip_ctx* ctx, const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                        int n_images, uint8_t* const* blurred, const uint8_t* blurred_ready, const int32_t* pairs, int n_pairs,
                        const mdhip_change_options* opt, int64_t* counts, uint32_t* hist, int32_t* thresholds, int32_t* n_regions,
                        int32_t* regions, uint8_t* overflow, uint8_t* const* masks, void* hip_stream);
/* The region stage of mdhip_change_detect in isolation (tests; host buffers, any context): the 8-connected components of the
 * non-zero pixels of mask (w x h bytes) -> labels (w x h; the smallest raster index of the pixel's component, -1 for
 * background), *n_regions (components with more than min_area pixels), the first `cap` of them by ascending label as
 * x, y, w, h, area in regions, *overflow (1: more than cap). */
int mdhip_label_regions_on(mdhip_ctx* ctx, const uint8_t* mask, int w, int h, int min_area, int cap, int32_t* labels, int32_t* n_regions,
                           int32_t* regions, uint8_t* overflow, void* hip_stream);

/* The number of gray pixels (R == G and R == B) inside a rectangle of each of n images that lie in device memory: the numerator
 * of the reference's visualization_utils.gray_scale_fraction, np.logical_and(r == g, r == b).sum(), for a whole chunk of decoded
 * files at once.  The statement and the walk of a row are csrc/gray_count.h's; the host model is mdjpeg_gray_count
 * (include/mdjpeg.h).
 *   ctx                       any context, one of mdhip_create_images included
 *   images                    per image the DEVICE address of its first pixel: RGB, 8 bits a sample, pitches[i] bytes a row, at
 *                             any alignment; widths, heights 1 .. 65535
 *   windows                   n x 4 values x, y, w, h: the rectangle that is counted, at least one pixel, inside its image (a
 *                             device image holds the pixels after the EXIF rotation, so the reference's band of rows, taken in
 *                             the stored orientation, may be a band of columns here)
 *   counts                    HOST memory, n values: per image the exact count
 * Every other array is host memory.  ONE launch for all images; only the 3 * w bytes of the h rows of a window are read.  Lane
 * counts are summed per wave and per workgroup, and each workgroup adds once, with a 64-bit atomicAdd, to its image's counter
 * in the context's scratch, which the call zeroes on the same stream first; the sums are integers, so the result does not depend
 * on the order.  The call returns when the counts are in host memory.  MDHIP_EINVAL, with nothing launched and counts left as
 * it is: a NULL pointer, n outside 1 .. 65535, a side outside 1 .. 65535, a pitch below 3 * width, an image whose last byte lies
 * 0x7fff0000 bytes or more behind its first (the limit of every image entry point), a window that is empty or leaves its
 * image, a host pointer among the images. */
int mdhip_gray_count(mdhip_ctx* ctx, const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                     const int32_t* windows, int n, uint64_t* counts, void* hip_stream);

/* Test-time augmentation: replaces mdhip_forward for `model(batch, augment=True)` (reference
 * pytorch_detector.py:1313 -> yolov5 _forward_augment): three passes over the batch that mdhip_preprocess
 * left in the context -- scale 1, scale 0.83 left-right flipped, scale 0.67 (bilinear, padded with 0.447 to
 * the model stride) -- boxes de-scaled and un-flipped, the coarsest level of the first and the finest level of
 * the last pass dropped, predictions concatenated.  mdhip_nms / mdhip_read_predictions then work on
 * mdhip_last_num_anchors(ctx) anchors per image. */
int mdhip_forward_tta(mdhip_ctx* ctx, int n, int h, int w, void* hip_stream);
/* anchors per image of the prediction the context currently holds (last forward, augmented forward or mdhip_nms_on) */
int mdhip_last_num_anchors(mdhip_ctx* ctx);

/* MDHIP_DTYPE_FP8 contexts (BASELINE.json configs[4]; the reference has no reduced precision at all --
 * pytorch_detector.py:848 hard-wires half_precision = False -- so there is no upstream call this replaces).
 * Activations and weights stay bf16 in HBM except the hidden tensor of every C3 bottleneck: its 1x1 conv writes it
 * as OCP e4m3 with one scale per tensor, its 3x3 conv runs on e4m3 operands (weights quantised per output channel at
 * mdhip_create) with the block-scaled K = 128 MFMA and fp32 accumulation.
 * mdhip_calibrate runs the batch left by mdhip_preprocess once in bf16, records the largest magnitude of every such
 * tensor and derives the scales (2x head-room); repeated calls accumulate the ranges.  mdhip_forward fails with
 * MDHIP_EINVAL until the context has scales (from mdhip_calibrate or mdhip_fp8_set_scales).  Results of an image do
 * not depend on the batch it travels in; they do depend on the calibration data.
 * mdhip_fp8_get_scales: returns the number of e4m3 tensors and fills up to max_n entries (any pointer may be NULL):
 * the scale, the model layer (C3 index) and the op index of the producing 1x1 conv, in execution order.
 * mdhip_fp8_set_scales: installs scales saved from an earlier calibration (same model, same order). */
int mdhip_calibrate(mdhip_ctx* ctx, int n, int h, int w, void* hip_stream);
int mdhip_fp8_num_tensors(mdhip_ctx* ctx);
int mdhip_fp8_get_scales(mdhip_ctx* ctx, float* scales, int32_t* layers, int32_t* ops, int max_n);
int mdhip_fp8_set_scales(mdhip_ctx* ctx, const float* scales, int n);
/* the host-side weight quantiser of the fp8 mode (OCP e4m3, round to nearest even, saturating at +-448); exported so
 * that the CPU test-suite can pin it against torch.float8_e4m3fn without a GPU */
int mdhip_f32_to_e4m3(const float* in, uint8_t* out, int n);

/* Replaces nms() (pytorch_detector.py:502-610) on the predictions of the last forward.
 * out: host, [n][max_det][6] = x1,y1,x2,y2,conf,cls in letterboxed pixels, sorted by
 * confidence (descending; ties by anchor index); counts: host, [n].  Blocks until the
 * results are in host memory. */
int mdhip_nms(mdhip_ctx* ctx, int n, float conf_thres, float iou_thres, int max_det,
              float* out, int32_t* counts, void* hip_stream);

/* Asynchronous form of mdhip_nms, for overlapping the host-side formatting of batch i
 * (pytorch_detector.py:1361-1422) with the GPU work of batch i+1: the kernel and the D2H copies
 * are enqueued on the stream and the call returns; results land in pinned host slot `slot`
 * (0 <= slot < MDHIP_NMS_SLOTS) owned by the context.  mdhip_nms_wait blocks until that slot is
 * complete and returns pointers into it ([n][max_det][6] floats, [n] counts), valid until the
 * slot is enqueued again. 
 * Every forward writes the other of two prediction buffers, so mdhip_nms_enqueue may run on another stream
 * than the forward of the next batch.  Ordering contract: the CALLER orders the enqueue behind its own forward (an
 * event recorded after mdhip_forward, waited for on the NMS stream); the LIBRARY orders the forward after next behind
 * the enqueue -- mdhip_nms_enqueue records an event for the prediction buffer it reads, and the forward that is about
 * to overwrite that buffer (mdhip_forward / mdhip_forward_tta, any stream) waits for it.  The scratch buffers of the
 * NMS kernels are shared: keep all mdhip_nms* calls of one context on ONE stream. */
#define MDHIP_NMS_SLOTS 4
int mdhip_nms_enqueue(mdhip_ctx* ctx, int n, float conf_thres, float iou_thres, int max_det,
                      int slot, void* hip_stream);
int mdhip_nms_wait(mdhip_ctx* ctx, int slot, const float** out, const int32_t** counts);

/* nms() on caller-supplied predictions (host, [n][n_anchors][5+nc] fp32); any n_anchors up to
 * the context's capacity.  Used by the parity tests against the reference's NMS vectors. */
int mdhip_nms_on(mdhip_ctx* ctx, const float* pred, int n, int n_anchors, float conf_thres,
                 float iou_thres, int max_det, float* out, int32_t* counts, void* hip_stream);

/* ---- introspection / measurement (not on the product path) ---- */

int mdhip_num_anchors(mdhip_ctx* ctx, int h, int w);                 /* anchors per image  */
int mdhip_max_stride(mdhip_ctx* ctx);
/* copy the raw predictions of the last forward to host: [n][n_anchors][5+nc] fp32 */
int mdhip_read_predictions(mdhip_ctx* ctx, int n, float* out, void* hip_stream);
/* copy the network input of the last preprocess to host as [n][3][h][w] fp32 (in [0,1]) */
int mdhip_read_input(mdhip_ctx* ctx, int n, int h, int w, float* out, void* hip_stream);
/* copy the output of model layer `layer` (last forward) to host as NCHW fp32; returns
 * c,h,w through the out-params; out may be NULL to query the shape only */
int mdhip_read_layer(mdhip_ctx* ctx, int layer, int n, float* out, int* c, int* h, int* w,
                     void* hip_stream);
/* A forward op by op (tests/op_step.py; ops are numbered as mdhip_get_op_info and mdhip_plan_describe number them).
 * mdhip_run_ops: the checks of mdhip_forward_timed, then ONE isolated pass (every op its own launch, as mdhip_time_op runs one:
 *   no fused bottleneck, no upsample read in place, no decode in a conv's epilogue; never a replayed graph) over ops
 *   [first, first + count) of a forward of n images of h x w, then a wait for the stream.  first == 0 begins a pass as
 *   mdhip_forward does (the other prediction buffer); a range that reaches the last op finishes it: from then on mdhip_read_layer
 *   and mdhip_read_predictions describe the stepped pass.  A range outside [0, mdhip_num_ops] is MDHIP_EINVAL.
 * mdhip_read_op_tensor: a view of op `op` exactly as stored, as NCHW fp32 at the size of the pass being stepped (of the last
 *   forward when none is): which = 0 in, 1 out, 2 res, 3 out2, 4..6 fsrc[0..2]; out may be NULL to query the shape only.  The
 *   fp32 logits of a Detect conv for its `out`; the stem's `in` as mdhip_read_input returns the network input.  MDHIP_EINVAL for
 *   a view the op does not have, for an e4m3 tensor (fp8 contexts) and for the decode ops.
 * mdhip_read_op_weights: what a conv or depthwise op multiplies, read back from the device: its 16-bit weights unpacked to
 *   w [c_out][c_in][kh][kw] fp32 (the stem: its 6x6 taps) and its fp32 bias b [c_out]; NULL buffers query the shape only. */
int mdhip_run_ops(mdhip_ctx* ctx, int n, int h, int w, int first, int count, void* hip_stream);
int mdhip_read_op_tensor(mdhip_ctx* ctx, int op, int which, int n, float* out, int* c, int* h, int* w, void* hip_stream);
int mdhip_read_op_weights(mdhip_ctx* ctx, int op, float* w, float* b, int* c_out, int* c_in, int* kh, int* kw);

/* the YOLO11 kernels in isolation (tests; host buffers, scratch device memory allocated per call), in the context's
 * 16-bit storage type (bf16 or fp16 bits):
 * mdhip_dwconv3x3_on: depthwise 3x3 / s1 / p1 of in [n][h][w][ld_in] -> out [n][h][w][c]; weight fp32 [c][1][3][3],
 *   bias [c]; output channel o reads input channel (o / grp) * grp_stride + grp_off + o % grp; act 1 = SiLU; res
 *   ([n][h][w][c] or NULL) is added after the activation
 * mdhip_attention_on: qkv [n][n_tokens][heads * 128] ([q 32 | k 32 | v 64] per head) -> out [n][n_tokens][heads * 64]
 * mdhip_dfl_decode_on: box logits fp32 [n][ny][nx][64], class logits fp32 [n][ny][nx][nc] -> pred [n][ny * nx][4 + nc] */
int mdhip_dwconv3x3_on(mdhip_ctx* ctx, const uint16_t* in, int ld_in, const float* weight, const float* bias, const uint16_t* res,
                       uint16_t* out, int n, int h, int w, int c, int grp, int grp_stride, int grp_off, int act, void* hip_stream);
int mdhip_attention_on(mdhip_ctx* ctx, const uint16_t* qkv, uint16_t* out, int n, int n_tokens, int heads, void* hip_stream);
int mdhip_dfl_decode_on(mdhip_ctx* ctx, const float* box, const float* cls, int nc, int n, int ny, int nx, float stride, float* pred,
                        void* hip_stream);

/* the YOLOv9 kernels in isolation (tests; host buffers, 16-bit storage of the context):
 * mdhip_adown_pool_on: in [n][h][w][c_in] -> a [n][h][w][c_in / 2] (2x2 / s1 average of the first half, last row and
 *   column zero), b [n][h / 2][w / 2][c_in / 2] (3x3 / s2 / p1 max of the 2x2 / s1 average of the second half)
 * mdhip_cbfuse_on: n_src sources src[k] [n][h / factor[k]][w / factor[k]][c] and last [n][h][w][c] -> out [n][h][w][c] */
int mdhip_adown_pool_on(mdhip_ctx* ctx, const uint16_t* in, uint16_t* a, uint16_t* b, int n, int h, int w, int c_in,
                        void* hip_stream);
int mdhip_cbfuse_on(mdhip_ctx* ctx, const uint16_t* const* src, const int32_t* factor, int n_src, const uint16_t* last,
                    uint16_t* out, int n, int h, int w, int c, void* hip_stream);

/* the network input of a scaled pass of mdhip_forward_tta in isolation (tests): pass 1 (scale 0.83, left-right flipped) or 2
 * (scale 0.67) of the batch of n images of h x w that mdhip_preprocess left in the context, computed as mdhip_forward_tta computes
 * it (the same launch, the same scratch copy of the batch, the pass geometry from the same function) and copied to host as
 * [n][3][*oh][*ow] fp32, exactly the stored values.  out may be NULL to query *oh and *ow only.  The context's input holds the
 * batch again when the call returns, and no forward state changes.  MDHIP_EUNSUPPORTED for anchor-free models, MDHIP_EINVAL for
 * another pass or without a preprocess of that batch. */
int mdhip_tta_input_on(mdhip_ctx* ctx, int n, int h, int w, int pass, float* out, int* oh, int* ow, void* hip_stream);

typedef struct {
    char    name[48];       /* e.g. "L6.m3.cv2 3x3"                           */
    int32_t kind;           /* 0 conv (implicit GEMM), 1 pool, 2 upsample, 3 decode (YOLOv5 Detect decode, or the DFL
                             * decode of an anchor-free head), 4 copy, 5 depthwise 3x3 conv, 6 C2PSA attention,
                             * 7 ADown pools, 8 CBFuse */
    int32_t layer;          /* model layer index                              */
    int32_t m, n, k;        /* GEMM view of a conv (per call, for the last n,h,w) */
    double  flops;          /* algorithmic FLOPs of the op for the last (n,h,w)   */
    double  bytes;          /* algorithmic HBM bytes (read input once + write output once + weights) */
    int32_t cfg;            /* tile configuration chosen (a decode op: -2 = done in
                             * the epilogue of the conv in front, -1 = own launch) */
    int32_t ntaps, stride, has_res;   /* conv: kh*kw of the packed kernel, stride, residual added */
    int32_t variant;        /* a conv with its own launch: which of the tile's compiled bodies ran, a number of the tile's
                             * kernel family (conv_v2: 0 general, 1 / 2 pointwise, 3 upsample read in place, 6 the streaming
                             * body of "pw_stream", 100 decoding), -1 where the family does not tell; never part of
                             * mdhip_launches_describe */
} mdhip_op_info;

/* What mdhip_create would plan for this model, dtype and capacity, as text, without touching a device: the context's sizes and
 * arena offsets, every layer view, every packed conv (shape, weight-arena offsets, element count and 64-bit FNV-1a hash of each of
 * its arrays) and every op (name, tensors, parameters), one record per line in a fixed field order.  Writes at most cap - 1
 * characters and a terminating 0 to buf (buf may be NULL with cap 0) and returns the length of the whole text; on failure the
 * negative code mdhip_create would return for the model, its text in mdhip_last_error(NULL).  tests/test_plan_cpu.py pins plans
 * with it. */
long long mdhip_plan_describe(const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w, char* buf, size_t cap);
int mdhip_num_ops(mdhip_ctx* ctx);
int mdhip_get_op_info(mdhip_ctx* ctx, int op, mdhip_op_info* out);
/* run the forward with a hipEvent pair around every op; ms[op] = duration in milliseconds */
int mdhip_forward_timed(mdhip_ctx* ctx, int n, int h, int w, float* ms, void* hip_stream);
/* live measurement for bench.py: with enable != 0 every mdhip_forward is bracketed by a hipEvent pair
 * recorded on the stream it is launched on (a ring of the 64 most recent forwards);
 * mdhip_forward_times waits for and returns the durations (ms) of the most recent min(max_n, 64,
 * forwards since enabling) forwards, oldest first, and returns how many it wrote (or a negative code). */
int mdhip_time_forwards(mdhip_ctx* ctx, int enable);
int mdhip_forward_times(mdhip_ctx* ctx, float* ms, int max_n);
/* force tile configuration `cfg` for op `op` (-1 = automatic choice); returns MDHIP_EINVAL
 * when cfg does not fit the op.  mdhip_num_conv_cfgs() = number of configurations. */
int mdhip_set_op_cfg(mdhip_ctx* ctx, int op, int cfg);
int mdhip_num_conv_cfgs(void);
/* 1 when tile configuration `cfg` can run conv op `op` (the first-generation configurations run every
 * op; the later main loops need C_in >= 64 or 32, kernels up to 3x3), 0 when not, negative on bad arguments */
int mdhip_op_supports_cfg(mdhip_ctx* ctx, int op, int cfg);
/* 1 when configuration `cfg` accumulates K in the canonical (r, s, c) order, i.e. produces bit-identical
 * results to every other such configuration; 0 for the row-patch kernel, whose K order is
 * (channel group, r, s, c) and whose results agree to fp32 summation-order rounding only */
int mdhip_cfg_is_bitwise(int cfg);
/* human-readable name of a tile configuration ("v2:160x160/2x2", ...); "" when out of range */
const char* mdhip_conv_cfg_name(int cfg);
/* measured tile choices (tools/autotune.py -> megadetector_amd/tuned_cfgs.json): a conv runs the
 * configuration of the entry with the same layer geometry (N, K, taps, stride, residual) whose
 * PER-IMAGE M (= m / batch = Ho*Wo) is equal or, failing that, nearest within a factor 4 (the same
 * layer at another image shape); everything else uses the built-in heuristic.  The choice does not
 * depend on the batch size of the call, so an image's result is bit-identical whatever batch it is
 * part of.  A configuration that does not support the op falls back to the heuristic choice. */
typedef struct {
    int32_t m, n, k;        /* GEMM view at measurement: M = batch*Ho*Wo, N = C_out, K = kh*kw*C_in */
    int32_t ntaps, stride;  /* kh*kw, conv stride */
    int32_t has_res;        /* 1 when the op adds a residual */
    int32_t cfg;
    int32_t batch;          /* batch size the entry was measured at (<= 0: taken as 32) */
} mdhip_tuned;
int mdhip_set_tuned(mdhip_ctx* ctx, const mdhip_tuned* entries, int n);
/* Fused bottlenecks (default on): a C3 block whose 3x3 convs all resolve to a strip configuration (the 80-channel block
 * of the x6 stack at batch >= 2) runs every bottleneck -- 1x1, SiLU, 3x3, SiLU, residual -- as ONE launch that keeps the
 * hidden tensor on chip; and a 1x1 conv behind Upsample + Concat reads the low-resolution tensor in place instead of its
 * 4x copy (the upsample launch is skipped).  Same arithmetic and summation order: bit-identical results.  on = 0 runs
 * the separate launches (A/B measurements, tests). */
int mdhip_set_fuse(mdhip_ctx* ctx, int on);
/* Graph replay of mdhip_forward (default off): the launches of one forward -- ~160 kernels, which at batch 1 .. 4 do a few
 * microseconds of work each -- are captured once per (batch, height, width) on an internal stream and replayed with one
 * hipGraphLaunch on the caller's stream.  mode 0 = off, 1 = every forward, 2 = forwards of at most max_n images (max_n <= 0
 * keeps the current bound, 8).  The first forward of a shape always runs eagerly; calls that change what a forward
 * launches (mdhip_set_tuned, mdhip_set_op_cfg, mdhip_set_fuse, fp8 scales) drop the captured graphs.  Same kernels, same
 * arguments: bit-identical results.  mdhip_forward_tta and the timed / per-op entry points are not replayed.
 * Replaces nothing in the reference (pytorch_detector.py:1313 runs eager PyTorch); this is launch plumbing. */
int mdhip_set_graph(mdhip_ctx* ctx, int mode, int max_n);
/* Named integer switches of a context (returns MDHIP_EINVAL for an unknown name; every change drops the captured graphs):
 *   "letterbox_general" 0 | 1   1 = mdhip_preprocess never takes the streaming-copy kernel (A/B measurements, tests;
 *                               the environment variable MDHIP_LETTERBOX_GENERAL at mdhip_create sets the same switch)
 *   "fuse_decode"       1 | 0   1 (default) = the Detect decode (yolov5 Detect.forward, pytorch_detector.py:1313) runs in the
 *                               epilogue of each level's 1x1 conv -- no fp32 logits tensor, four launches fewer -- for heads
 *                               with 8 outputs per anchor (MDv5: nc = 3) in the plain forward; the augmented forward and
 *                               other heads always use the separate decode kernel.  Same statements, bit-identical.
 *   "pw_stream"         1 | 0 | 2   1x1 / stride 1 convs with 160 input and 160 output channels, SiLU and a 16-bit output that
 *                               does not overlap their input have a second body that keeps the weights in registers and streams
 *                               pixels past them, under the tile configuration the op has anyway (the tile's name,
 *                               mdhip_launches_describe and mdhip_op_info::cfg do not change; mdhip_op_info::variant tells):
 *                               1 (default) = it runs them from the pixel count on at which it is the faster one, 0 = never,
 *                               2 = always (tests).  Same MFMA chain and epilogue per output: bit-identical.
 * Replaces nothing in the reference; the switches exist for measurements and tests. */
int mdhip_set_option(mdhip_ctx* ctx, const char* name, int value);
/* time one op in isolation: `iters` back-to-back launches bracketed by events */
int mdhip_time_op(mdhip_ctx* ctx, int op, int n, int h, int w, int iters, float* ms_avg,
                  void* hip_stream);
/* What a forward of n images of h x w would launch on such a context, as text, without touching a device: one line per op, in op
 * order -- index, name, what the op does (`launch` with the name of its tile configuration, `in_next` = runs inside the next
 * launch, `in_place` = read in place by its consumer, `in_front` = decoded in the conv in front, `plain` = its own launch
 * without a tile), whether the tile came from the table `tuned` (as mdhip_set_tuned takes it), whether the conv decodes in its
 * epilogue, and the statistics mdhip_get_op_info reports (m n k, flops and bytes as %.17g).  `flags`: the settings and the kind
 * of pass below; `forced`: n_forced pairs (op, cfg) as mdhip_set_op_cfg takes them.  Buffer, return value and errors as
 * mdhip_plan_describe.  A tile the launcher would refuse at launch (a stale table entry) is not predicted.
 * tests/test_launches_cpu.py pins launches with it. */
#define MDHIP_LAUNCHES_NO_FUSE 1          /* mdhip_set_fuse(ctx, 0) */
#define MDHIP_LAUNCHES_NO_FUSE_DECODE 2   /* mdhip_set_option(ctx, "fuse_decode", 0) */
#define MDHIP_LAUNCHES_NO_PAIR 4          /* MDHIP_PAIR=0 at mdhip_create */
#define MDHIP_LAUNCHES_ISOLATED 8         /* one op on its own, as mdhip_time_op runs it */
#define MDHIP_LAUNCHES_CALIBRATING 16     /* the 16-bit forward of mdhip_calibrate (fp8 contexts) */
#define MDHIP_LAUNCHES_AUGMENTED 32       /* a pass of mdhip_forward_tta, h x w being the size of that pass */
#define MDHIP_LAUNCHES_NO_PW_STREAM 128    /* mdhip_set_option(ctx, "pw_stream", 0): the text does not depend on it */
#define MDHIP_LAUNCHES_AFTER_OTHERS 64    /* test hook: other shapes, passes and settings are resolved on the context first and
                                             every setting is flipped and flipped back; the text must not depend on it */
long long mdhip_launches_describe(const mdhip_model* model, int dtype, int max_batch, int max_h, int max_w, const mdhip_tuned* tuned,
                                  int n_tuned, int n, int h, int w, unsigned flags, const int32_t* forced, int n_forced, char* buf,
                                  size_t cap);

const char* mdhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MDHIP_H */
