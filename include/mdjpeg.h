/*
 * mdjpeg.h -- C ABI of libmdjpeg.so: the host half of the GPU JPEG feed ("GPU JPEG reconstruction").
 *
 * A loader process parses a baseline JPEG and Huffman-decodes its scan to QUANTISED DCT coefficients; everything after
 * that (de-quantisation, inverse DCT, chroma upsampling, colour conversion, EXIF rotation) runs on the GPU
 * (mdhip_jpeg_reconstruct, include/mdhip.h).  This library is plain C++ and links nothing of HIP: the loader processes
 * never open the GPU.
 *
 * The decoder never guesses.  Whatever is not a clean stream of a supported kind is an error code, and the caller decodes
 * that file with its ordinary decoder, so every warning, failure string and partial image stays that decoder's.
 */
#ifndef MDJPEG_H
#define MDJPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDJPEG_OK            0
#define MDJPEG_EINVAL       -1   /* bad argument                                                              */
#define MDJPEG_EUNSUPPORTED -2   /* a JPEG (or not) of a kind this decoder leaves to the caller: info.reason  */
#define MDJPEG_ECORRUPT     -3   /* the stream is not clean (see mdjpeg_decode): info.reason                  */
#define MDJPEG_ECAPACITY    -4   /* the coefficient planes do not fit `capacity`                              */

typedef struct {
    int32_t  width, height;          /* image size in pixels (before any EXIF rotation)                          */
    int32_t  components;             /* 1 (grayscale) or 3 (YCbCr)                                               */
    int32_t  h_samp[3], v_samp[3];   /* sampling factors; (1, 1) for grayscale whatever the file says            */
    int32_t  restart_interval;       /* MCUs between restart markers, 0 = none                                   */
    int32_t  mcus_x, mcus_y;         /* MCUs per row / column                                                    */
    int32_t  blocks_w[3], blocks_h[3]; /* size of each component's plane in 8x8 blocks (whole MCUs)              */
    int64_t  plane_offset[3];        /* first coefficient of each plane, in int16 units from the buffer's start  */
    int64_t  coef_count;             /* int16 values mdjpeg_decode writes: sum of blocks_w * blocks_h * 64       */
    uint16_t quant[3][64];           /* quantisation table of each COMPONENT, natural (row-major) order          */
    int32_t  supported;              /* 1: mdjpeg_decode takes this file                                         */
    char     reason[100];            /* why not (supported == 0), or what the decoder met (MDJPEG_ECORRUPT)      */
} mdjpeg_info;

/* Walks the markers up to the first SOS.  Returns MDJPEG_OK with info->supported = 1, or MDJPEG_EUNSUPPORTED with
 * info->supported = 0 and info->reason set (width / height / components are filled in as far as they were read).
 * Supported: 8-bit sequential Huffman (SOF0, SOF1 with 8-bit samples), ONE interleaved scan, grayscale or three
 * components YCbCr with chroma 1x1 and luma 1x1 / 2x1 / 2x2 (4:4:4, 4:2:2, 4:2:0), with or without restart intervals,
 * any size.  Not supported: progressive, lossless and hierarchical frames, arithmetic coding, 12-bit samples, four
 * components (CMYK / YCCK), an Adobe marker with transform 0 (RGB stored as such), any other sampling (4:4:0, 4:1:1 ...),
 * several scans, anything that does not parse. */
int mdjpeg_parse(const uint8_t* data, size_t size, mdjpeg_info* info);

/* Huffman-decodes the scan into coef[0 .. info->coef_count): one plane per component, blocks in raster order, the 64
 * values of a block in natural (row-major) order, still quantised.  `capacity` counts int16 values; nothing is written at
 * or beyond coef[capacity].  Parses the file itself and fills *info as mdjpeg_parse does.
 * MDJPEG_ECORRUPT, never a guess, for: an undefined Huffman code, a DC / AC magnitude category a baseline file cannot
 * hold, a coefficient index past 63, a zero run that leaves the block, a block whose de-quantised coefficients carry
 * more energy than 64 samples of 8 bits can have (plus the quantisation error), data that end early or bytes left
 * over in front of a marker, a restart marker that is missing or out of sequence, a scan not followed by EOI at once.
 * On any error the contents of coef are unspecified. */
int mdjpeg_decode(const uint8_t* data, size_t size, mdjpeg_info* info, int16_t* coef, size_t capacity);

/* ---- the scan as a decoder that starts anywhere needs it (GPU entropy decoding: mdhip_jpeg_entropy_decode) ------------- */
#define MDJPEG_MAX_TABLES 6          /* a scan of three components names at most three DC and three AC tables           */

typedef struct {
    mdjpeg_info info;                        /* exactly what mdjpeg_parse fills in                                         */
    int32_t  n_tables;                       /* distinct Huffman tables the scan's components name, in order of first use  */
    int32_t  dc_table[3], ac_table[3];       /* which of them each component uses                                          */
    uint8_t  huff_counts[MDJPEG_MAX_TABLES][16];   /* as the file's DHT segments write them: codes of each length ...      */
    uint8_t  huff_vals[MDJPEG_MAX_TABLES][256];    /* ... and their values                                                 */
    int64_t  scan_begin, scan_end;           /* file offsets: first byte of entropy-coded data; the FF of the EOI marker   */
    int32_t  n_segments;                     /* restart segments (1 without a restart interval)                            */
    int32_t  reserved;
} mdjpeg_scan_info;

/* mdjpeg_parse's acceptance rule and info, plus the tables and the byte ranges.  Decodes no Huffman symbol: the restart
 * segments are found by a plain search for FF bytes that are not followed by 00.  seg_offsets[k] receives the offset of
 * segment k's first byte from scan_begin; segment k ends two bytes (its RSTn marker) in front of segment k + 1, the last
 * one at scan_end.  Applies the checks of mdjpeg_decode that need no symbol: MDJPEG_ECORRUPT when a restart marker is
 * missing or out of sequence, when the scan is not followed by EOI at once or when the file ends first;
 * MDJPEG_ECAPACITY (with n_segments set) when there are more segments than seg_capacity.  Never reads beyond `size`. */
int mdjpeg_scan(const uint8_t* data, size_t size, mdjpeg_scan_info* scan, uint32_t* seg_offsets, size_t seg_capacity);

/* The host model of the GPU entropy decoder, for tests: the same passes over subsequences of `subseq_bits` bits (a multiple
 * of 8 from 64 to 65536, or longer than every restart segment; anything else is MDJPEG_EINVAL), as loops over "lanes", with the per-lane decoder the kernels are compiled from (csrc/jpeg_subseq.h).  Arguments,
 * results and return codes are those of mdjpeg_decode; info->reason differs.  The loaders do not call it. */
int mdjpeg_decode_subsequences(const uint8_t* data, size_t size, int subseq_bits, mdjpeg_info* info, int16_t* coef, size_t capacity);

/* ---- entropy ENCODING (GPU: mdhip_jpeg_encode, include/mdhip.h) ------------------------------------------------------- */
/* The host model of the GPU entropy encoder, for tests: the same passes -- bit length of every block, prefix sum, bit
 * writing at the offsets, stuffing in chunks of `chunk_bytes` unstuffed bytes (any size from 1 up; the device uses 64) --
 * as loops over "lanes", with the per-block encoder, the offset arithmetic and the stuffing chunk the kernels are compiled
 * from (csrc/jpeg_encode.h).  n crops in one call, as one batch of the device.
 *   coefs[i]   crop i's quantised coefficients in the layout of mdjpeg_decode for three components, 4:2:0: the planes of
 *              Y, Cb, Cr one behind the other, whole MCUs ((w + 15) / 16 x (h + 15) / 16 MCUs, Y 2 x 2 blocks each), natural
 *              order within a block.  Luma blocks that only fill up an MCU are not read: libjpeg's rule stands in for them.
 *   out        receives the crops' scans one behind the other: crop i's at out[offsets[i]], sizes[i] bytes -- every byte
 *              between the SOS header and the EOI marker of the file Pillow / libjpeg-turbo write for these coefficients
 *              (interleaved scan, no restart markers, the standard's four Huffman tables, FF bytes stuffed, the last byte
 *              padded with 1-bits).
 * *needed is the capacity the call needs.  MDJPEG_ECAPACITY when it is more than `capacity`: nothing is written at or beyond
 * out[capacity], offsets / sizes / *needed are valid, and a second call with *needed bytes succeeds.  MDJPEG_ECORRUPT for a
 * DC difference or an AC coefficient no baseline file can hold.  mdjpeg_encode_bound: what one crop's scan can take at the
 * very most, from the worst code lengths of the tables (1660 bits a block, every byte stuffed); -1 for a size outside
 * 1 .. 65535. */
int mdjpeg_encode_subsequences(const int16_t* const* coefs, const int32_t* widths, const int32_t* heights, int n, int chunk_bytes,
                               uint8_t* out, size_t capacity, int64_t* offsets, int64_t* sizes, size_t* needed);
int64_t mdjpeg_encode_bound(int32_t width, int32_t height);
/* The same with a chroma sampling per crop (GPU: mdhip_jpeg_encode_sampled): samplings[i] 0 = h1v1 (4:4:4, MCU of 3 blocks),
 * 1 = h2v1 (4:2:2, 4 blocks), 2 = h2v2 (4:2:0, 6 blocks), numbered as Pillow's `subsampling`; anything else is
 * MDJPEG_EINVAL.  coefs[i] in the layout of mdjpeg_decode for that sampling: Y in whole MCUs ((w + 8 hs - 1) / (8 hs) x
 * (h + 8 vs - 1) / (8 vs) MCUs of hs x vs luma blocks), then Cb, then Cr, one block an MCU each.
 * mdjpeg_encode_subsequences is this call with 2 for every crop: one encoder, not two. */
int mdjpeg_encode_subsequences_sampled(const int16_t* const* coefs, const int32_t* widths, const int32_t* heights,
                                       const int32_t* samplings, int n, int chunk_bytes, uint8_t* out, size_t capacity,
                                       int64_t* offsets, int64_t* sizes, size_t* needed);
int64_t mdjpeg_encode_sampled_bound(int32_t width, int32_t height, int32_t sampling);
/* The host model of mdhip_jpeg_encode_kept's merge, for ONE window, compiled from the header the kernel is compiled from
 * (csrc/jpeg_keep.h): `planes` holds the window's re-encoded coefficients (the layout of mdjpeg_decode for `sampling`: whole
 * MCUs, Y then Cb then Cr) and `source` the source file's in the same layout; every block of an MCU that none of the
 * n_rects rectangles touches (rects: left, top, right, bottom in pixels, right and bottom exclusive; each is clipped to the
 * window and dropped when nothing is left) is overwritten with the source's, dummy blocks included.  *status: 1 when the merged
 * planes hold a DC difference beyond category 11 or an AC value beyond category 10 -- mdjpeg_encode_subsequences_sampled
 * answers MDJPEG_ECORRUPT for them, the device gives that window a scan of size 0 -- else 0.  MDJPEG_EINVAL for a NULL
 * pointer, a size outside 1 .. 65535, a sampling outside 0 .. 2 or n_rects < 0. */
int mdjpeg_keep_merge(int16_t* planes, const int16_t* source, int32_t width, int32_t height, int32_t sampling, const int32_t* rects,
                      int n_rects, int32_t* status);

/* ---- Gaussian blur of rectangles (GPU: mdhip_blur_regions, include/mdhip.h) -------------------------------------------- */
/* The host model of the GPU blur and the host leg of HIPDetector(blur=): Pillow's ImageFilter.GaussianBlur(radius) of
 * rectangles of an RGB image, bit for bit -- three passes of an extended box filter along x, then three along y, in 32-bit
 * integers with an 8-bit rounding behind every pass, the rectangle's own edges replicated -- with the weights, the line pass
 * and the chunk arithmetic the kernels are compiled from (csrc/blur_box.h).
 *   rgb, width, height, pitch   the image, 8 bits a sample, R G B interleaved, `pitch` bytes a row (>= 3 * width); changed in place
 *   rects, n_rects              n_rects x 4 values: left, top, right, bottom in pixels, right and bottom exclusive.  They are
 *                               applied in the order of the list, each to what the ones before it left (what
 *                               visualization_utils.blur_detections does: crop, blur, paste), so overlapping rectangles interact.
 *                               A rectangle without area (right <= left or bottom <= top) is skipped, as Pillow pastes
 *                               nothing for it; any other that leaves the image is MDJPEG_EINVAL, and nothing is changed.
 *   radius                      of the Gaussian, 0 .. 512 (0 changes nothing)
 * mdjpeg_blur_regions_chunked cuts the rows into the chunks (with their halo) a device with lds_bytes of on-chip memory
 * would cut them into (the device has 49152); same result.  mdjpeg_blur_weights: r, ww, fw of a radius. */
int mdjpeg_blur_regions(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects, float radius);
int mdjpeg_blur_regions_chunked(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects,
                                float radius, int lds_bytes);
int mdjpeg_blur_weights(float radius, int32_t* r, uint32_t* ww, uint32_t* fw);

/* ---- annotated previews (GPU: mdhip_resample_lanczos, mdhip_draw_ops, include/mdhip.h) ---------------------------------- */
/* The host models of the two GPU calls, compiled from the header the kernels are compiled from (csrc/resample.h).
 * mdjpeg_resample: Pillow's Image.resize((dst_width, dst_height), LANCZOS) of an 8-bit RGB image, bit for bit; `pitch` and
 * `dst_pitch` are bytes a row (>= 3 * width); sizes 1 .. 65535; the images must not overlap.
 * mdjpeg_draw: applies n_ops drawing operations of 8 int32 each (see mdhip_draw_ops) to an image in place -- a pixel takes
 * the value of the last operation that covers it; `patches` holds the pixels of the patch operations, patch_bytes bytes.
 * MDJPEG_EINVAL, and nothing is changed, for an unknown kind or a patch outside `patches`. */
int mdjpeg_resample(const uint8_t* src, int32_t width, int32_t height, int64_t pitch, uint8_t* dst, int32_t dst_width, int32_t dst_height,
                    int64_t dst_pitch);
int mdjpeg_draw(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* ops, int n_ops, const uint8_t* patches,
                int64_t patch_bytes);
/* mdjpeg_draw_from: the host model of mdhip_draw_ops_from, with the same arguments on host memory -- destination i is made
 * from source dst_src[i] (same size, dst_pitches[i] bytes a row): a pixel is the last operation of the destination's list that
 * covers it, or else the source's pixel; op_image[i] names a destination.  Only the 3 * width bytes of a destination's rows
 * are written and no source is.  MDJPEG_EINVAL, and nothing is written, for what mdjpeg_draw refuses, a dst_src[i] or
 * op_image[i] out of range, and a destination that overlaps a source or another destination. */
int mdjpeg_draw_from(const uint8_t* const* src, const int32_t* widths, const int32_t* heights, const int64_t* pitches, int n_src,
                     uint8_t* const* dst, const int32_t* dst_src, const int64_t* dst_pitches, int n_dst, const int32_t* op_image,
                     const int32_t* ops, int n_ops, const uint8_t* patches, int64_t patch_bytes);

/* ---- classifier input (GPU: mdhip_classifier_input, include/mdhip.h) ---------------------------------------------------- */
/* The host model of the GPU call for ONE crop, compiled from the header the kernel is compiled from (csrc/resample.h): the
 * canvas_w x canvas_h canvas whose rectangle src_w x src_h at (off_x, off_y) holds the pixels at `src` (`pitch` bytes a row)
 * and is 0 elsewhere, resized with Pillow's filter (0 bicubic, 1 bilinear, 2 LANCZOS) so that its shorter side is `size`,
 * the size x size centre, (v / 255 - mean) / std: out = fp32 [3][size][size], bit for bit what PIL and torchvision give.
 * mdjpeg_classifier_plan: plan[0] output columns and plan[1] output rows a workgroup takes of a crop of that canvas with
 * lds_bytes of on-chip memory (0: what the device has); MDJPEG_EUNSUPPORTED when nothing fits -- the sizes the GPU call
 * refuses. */
int mdjpeg_classifier_input(const uint8_t* src, int64_t pitch, int32_t src_w, int32_t src_h, int32_t canvas_w, int32_t canvas_h,
                            int32_t off_x, int32_t off_y, int32_t size, int32_t filter, const float mean[3], const float std[3], float* out);
int mdjpeg_classifier_plan(int32_t canvas_w, int32_t canvas_h, int32_t size, int32_t filter, int32_t lds_bytes, int32_t plan[2]);

/* ---- thumbnails (GPU: mdhip_thumbnails, include/mdhip.h) ---------------------------------------------------------------- */
/* The host model of the GPU call, compiled from the header the kernel is compiled from (csrc/resample.h), and of the same
 * record with every pointer in HOST memory: tile i is Pillow's image.crop(box).resize((out_w, out_h), filter) -- the box as a
 * canvas_w x canvas_h canvas whose rectangle src_w x src_h at (off_x, off_y) holds the pixels at `src` and is 0 elsewhere --
 * written R G B interleaved at dst, dst_pitch bytes a row, bit for bit; only the 3 * out_w bytes of its out_h rows are
 * written.  src_w or src_h of 0: the canvas holds no image pixel and src is not read.  filter: 0 bicubic, 1 bilinear,
 * 2 LANCZOS.  MDJPEG_EINVAL for a NULL pointer, a rectangle that leaves its canvas,
 * a size outside 1 .. 65535, a pitch below its row or an unknown filter, MDJPEG_EUNSUPPORTED for the sizes the GPU call
 * refuses; nothing is written in either case. */
typedef struct {
    const uint8_t* src;
    int64_t  pitch;
    int32_t  src_w, src_h;
    int32_t  canvas_w, canvas_h;
    int32_t  off_x, off_y;
    int32_t  out_w, out_h;
    uint8_t* dst;
    int64_t  dst_pitch;
} mdjpeg_thumbnail;
int mdjpeg_thumbnails(const mdjpeg_thumbnail* tiles, int n, int32_t filter);

/* ---- repeat-detection elimination (GPU: mdhip_repeat_detections, include/mdhip.h) --------------------------------------- */
/* The host model of the GPU call, compiled from the header the kernels are compiled from (csrc/rde_match.h): a plain
 * sequential restatement of the reference's rule (repeat_detections_core.py _find_matches_in_directory) -- a box is appended
 * to every earlier candidate of its group that it matches, and opens a new candidate when it matches none.  Arguments and
 * results are those of mdhip_repeat_detections without `device`; `chunk` is checked (>= 0) and otherwise has no meaning here.
 * MDJPEG_EINVAL for n < 0, a decreasing group, a NaN threshold, a negative chunk or capacity; MDJPEG_ECAPACITY when
 * *needed > capacity: is_candidate, n_instances and *needed are valid and `pairs` is untouched. */
typedef struct {
    double  x, y, w, h;      /* the detection's bbox as the results file has it                       */
    int32_t group;           /* index of its location; non-decreasing along the array                 */
    int32_t category;
} mdjpeg_rde_box;
int mdjpeg_repeat_detections(const mdjpeg_rde_box* boxes, int64_t n, double iou_threshold, int category_agnostic,
                             int32_t occurrence_threshold, int32_t chunk, uint8_t* is_candidate, int32_t* n_instances,
                             int64_t* pairs, int64_t capacity, int64_t* needed);

/* ---- change detection between images (GPU: mdhip_change_detect, include/mdhip.h) ----------------------------------------- */
/* The host model of the GPU call, compiled from the header the kernels are compiled from (csrc/change_detect.h, which defines
 * every step: gray, region of interest, blur, difference, threshold, dilation, regions).  Arguments and results are those of
 * mdhip_change_detect without the context and the stream, and every pointer is host memory:
 *   images, widths, heights, pitches, n_images   RGB images, 8 bits a sample, `pitches[i]` bytes a row; sides 1 .. 32767.
 *   blurred, blurred_ready      per image a plane of widths[i] x heights[i] bytes, dense: the blurred gray image.  ready 0: the
 *                               call computes it from images[i] and writes it there; ready 1: it holds the plane already (of an
 *                               earlier call with the same options) and images[i] is not read and may be NULL.
 *   pairs, n_pairs              n_pairs x 2 image indices (previous, current); both images of a pair have one size
 *   opt                         the options: see csrc/change_detect.h for their ranges
 *   counts                      per pair the number of non-zero pixels of the thresholded mask (after the region of interest)
 *   hist                        per pair the 256-bin histogram of the difference for threshold_type 1 (OTSU), else zeros
 *   thresholds                  per pair the threshold that was applied
 *   n_regions                   per pair the number of significant regions (area > min_area), whatever the cap
 *   regions                     per pair opt->region_cap x 5 values: x, y, w, h, area of the first region_cap significant
 *                               regions by ascending label
 *   overflow                    per pair 1 when n_regions is above region_cap (the list is cut), else 0
 *   masks                       NULL, or per pair NULL or a widths x heights plane that receives the dilated mask (0 / 255)
 * MDJPEG_EINVAL, and nothing is written, for a NULL pointer, an option or a size outside its range, a pitch below its row, a
 * pair that names an image outside 0 .. n_images - 1 or two images of different sizes, an image that is neither given nor ready. */
typedef struct {
    int32_t blur_kernel_size;    /* odd, 1 .. 127                                   */
    int32_t threshold_type;      /* 0 GLOBAL, 1 OTSU                                */
    int32_t threshold;           /* GLOBAL: 0 .. 255                                */
    int32_t dilate_kernel_size;  /* 1 .. 33                                         */
    int32_t dilate_iterations;   /* 0 .. 64                                         */
    int32_t min_area;            /* >= 0                                            */
    int32_t has_ignore;          /* 0: ignore_fraction is None                      */
    int32_t region_cap;          /* 0 .. 65536                                      */
    double  ignore_fraction;     /* -1 .. 1                                         */
} mdjpeg_change_options;
int mdjpeg_change_detect(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches, int n_images,
                         uint8_t* const* blurred, const uint8_t* blurred_ready, const int32_t* pairs, int n_pairs,
                         const mdjpeg_change_options* opt, int64_t* counts, uint32_t* hist, int32_t* thresholds, int32_t* n_regions,
                         int32_t* regions, uint8_t* overflow, uint8_t* const* masks);

/* ---- gray pixels of a rectangle (GPU: mdhip_gray_count, include/mdhip.h) ---------------------------------------------------- */
/* The host model of the GPU call, compiled from the header the kernel is compiled from (csrc/gray_count.h): per image the number
 * of pixels with R == G and R == B inside its window.  Arguments as mdhip_gray_count without the context and the stream, every
 * pointer host memory: images (RGB, 8 bits a sample, pitches[i] bytes a row, any alignment), widths, heights (1 .. 65535),
 * windows (n x 4: x, y, w, h; at least one pixel, inside the image), counts (n values).  mdjpeg_gray_count asks every pixel of
 * the window in turn; mdjpeg_gray_count_walk takes the kernel's walk of a row (head pixels byte by byte up to an aligned
 * address, four pixels at a time as three 32-bit words, the tail byte by byte) and must give the same counts.  Neither reads a
 * byte outside the 3 * w bytes of the window's rows.  MDJPEG_EINVAL, and nothing is written, for a NULL pointer, n outside
 * 1 .. 65535, a side outside 1 .. 65535, a pitch below 3 * width, an image whose last byte lies 0x7fff0000 bytes or more
 * behind its first (the GPU call's limit, kept so that both refuse the same), a window that is empty or leaves its image. */
int mdjpeg_gray_count(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                      const int32_t* windows, int n, uint64_t* counts);
int mdjpeg_gray_count_walk(const uint8_t* const* images, const int32_t* widths, const int32_t* heights, const int64_t* pitches,
                           const int32_t* windows, int n, uint64_t* counts);

const char* mdjpeg_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MDJPEG_H */
