// libmdjpeg.so: the host model of the GPU entropy ENCODER (mdjpeg_encode_subsequences, mdjpeg_encode_subsequences_sampled),
// of the kept-block merge (mdjpeg_keep_merge) and the two size bounds.  Device twin: jpeg_encode.cpp.  The encoder of a
// block, the layout of a batch and the stuffing chunk are jpeg_encode.h's, the merge's predicate and addressing jpeg_keep.h's,
// which the kernels compile too; here the passes are loops over lanes.

#include "../../include/mdjpeg.h"
#include "jpeg_encode.h"
#include "jpeg_keep.h"

#include <cstring>
#include <vector>

extern "C" {

// a crop's planes in natural order -> its blocks in MCU order, each transposed (coef: the batch's blocks, c.block0 the crop's first)
static void planes_to_mcu_order(const MdjEncCrop& c, const int16_t* planes, int16_t* coef) {
    const int64_t mcus = int64_t(c.mcus_x) * c.mcus_y;
    const int luma = c.hs * c.vs;
    const int16_t* plane[3] = {planes, planes + mcus * luma * 64, planes + mcus * (luma + 1) * 64};
    for (int64_t m = 0; m < mcus; ++m) {
        const int mx = int(m % c.mcus_x), my = int(m / c.mcus_x);
        for (int k = 0; k < c.per_mcu; ++k) {
            const int16_t* src = k < luma ? plane[0] + ((int64_t(my) * c.vs + k / c.hs) * (c.mcus_x * c.hs) + mx * c.hs + k % c.hs) * 64
                                          : plane[k - luma + 1] + m * 64;
            int16_t* dst = coef + (c.block0 + m * c.per_mcu + k) * 64;
            for (int j = 0; j < 64; ++j) dst[((j & 7) << 3) | (j >> 3)] = src[j];
        }
    }
}

// mdjpeg_encode_subsequences (samplings NULL: h2v2 for every crop) and mdjpeg_encode_subsequences_sampled
static int encode_subsequences(const int16_t* const* coefs, const int32_t* widths, const int32_t* heights, const int32_t* samplings, int n,
                               int chunk_bytes, uint8_t* out, size_t capacity, int64_t* offsets, int64_t* sizes, size_t* needed) {
    if (!coefs || !widths || !heights || !offsets || !sizes || !needed || n < 1 || chunk_bytes < MDJ_ENC_MIN_CHUNK || (!out && capacity))
        return MDJPEG_EINVAL;
    if (samplings)
        for (int i = 0; i < n; ++i)
            if (!mdj_enc_sampling_ok(samplings[i])) return MDJPEG_EINVAL;
    // the batch as the device lays it out: crops one behind the other in block order, bit buffer regions and chunks at their bounds
    std::vector<MdjEncCrop> crops(size_t(n) + 1);
    int64_t blocks = 0, words = 0, chunks = 0;
    for (int i = 0; i <= n; ++i) {
        MdjEncCrop& c = crops[size_t(i)];
        memset(&c, 0, sizeof(c));
        c.block0 = blocks;
        c.word0 = words;
        c.chunk0 = chunks;
        if (i == n) break;
        if (!coefs[i] || widths[i] < 1 || heights[i] < 1 || widths[i] > 65535 || heights[i] > 65535) return MDJPEG_EINVAL;
        const int sampling = samplings ? samplings[i] : MDJ_ENC_H2V2;
        mdj_enc_set_layout(c, widths[i], heights[i], sampling);
        const int64_t nb = mdj_enc_blocks(widths[i], heights[i], sampling);
        if (nb > MDJ_ENC_MAX_BLOCKS) return MDJPEG_EINVAL;
        blocks += nb;
        words += mdj_enc_region_words(nb);
        chunks += mdj_enc_region_chunks(nb, chunk_bytes);
    }
    // planes in natural order -> MCU order, blocks transposed
    std::vector<int16_t> coef((size_t)blocks * 64);
    for (int i = 0; i < n; ++i) planes_to_mcu_order(crops[size_t(i)], coefs[i], coef.data());
    MdjEncTables tables;
    mdj_enc_build_tables(tables);
    std::vector<uint32_t> len((size_t)blocks), bitbuf((size_t)words, 0u), count((size_t)chunks);
    std::vector<uint64_t> off((size_t)blocks + 1), start((size_t)chunks + 1);
    uint32_t errors = 0;
    for (int64_t g = 0; g < blocks; ++g) {                               // pass "bits"
        int c;
        uint32_t e;
        len[size_t(g)] = mdj_enc_lane_bits(crops.data(), n, coef.data(), tables, g, &c, &e);
        errors |= e;
    }
    if (errors) return MDJPEG_ECORRUPT;
    off[0] = 0;
    for (int64_t g = 0; g < blocks; ++g) off[size_t(g) + 1] = off[size_t(g)] + len[size_t(g)];
    for (int64_t g = 0; g < blocks; ++g)                                  // pass "write"
        mdj_enc_lane_write(crops.data(), n, coef.data(), tables, off.data(), bitbuf.data(), g);
    for (int64_t q = 0; q < chunks; ++q)                                  // pass "count"
        count[size_t(q)] = mdj_enc_lane_count(crops.data(), n, off.data(), bitbuf.data(), chunk_bytes, q);
    start[0] = 0;
    for (int64_t q = 0; q < chunks; ++q) start[size_t(q) + 1] = start[size_t(q)] + count[size_t(q)];
    for (int i = 0; i < n; ++i) {
        offsets[i] = int64_t(start[size_t(crops[size_t(i)].chunk0)]);
        sizes[i] = int64_t(start[size_t(crops[size_t(i) + 1].chunk0)]) - offsets[i];
    }
    *needed = size_t(start[size_t(chunks)]);
    for (int64_t q = 0; q < chunks; ++q)                                  // pass "stuff"
        mdj_enc_lane_stuff(crops.data(), n, off.data(), bitbuf.data(), chunk_bytes, start.data(), out, int64_t(capacity), q);
    return *needed > capacity ? MDJPEG_ECAPACITY : MDJPEG_OK;
}

int mdjpeg_encode_subsequences(const int16_t* const* coefs, const int32_t* widths, const int32_t* heights, int n, int chunk_bytes,
                               uint8_t* out, size_t capacity, int64_t* offsets, int64_t* sizes, size_t* needed) {
    return encode_subsequences(coefs, widths, heights, nullptr, n, chunk_bytes, out, capacity, offsets, sizes, needed);
}

int mdjpeg_encode_subsequences_sampled(const int16_t* const* coefs, const int32_t* widths, const int32_t* heights,
                                       const int32_t* samplings, int n, int chunk_bytes, uint8_t* out, size_t capacity,
                                       int64_t* offsets, int64_t* sizes, size_t* needed) {
    if (!samplings) return MDJPEG_EINVAL;
    return encode_subsequences(coefs, widths, heights, samplings, n, chunk_bytes, out, capacity, offsets, sizes, needed);
}

// The host model of mdhip_jpeg_encode_kept's merge for one window: the predicate and the addressing are jpeg_keep.h's, the
// status comes from the encoder's own "bits" pass over the merged blocks.
int mdjpeg_keep_merge(int16_t* planes, const int16_t* source, int32_t width, int32_t height, int32_t sampling, const int32_t* rects,
                      int n_rects, int32_t* status) {
    if (!planes || !source || !status || width < 1 || height < 1 || width > 65535 || height > 65535 || !mdj_enc_sampling_ok(sampling) ||
        n_rects < 0 || (n_rects && !rects))
        return MDJPEG_EINVAL;
    MdjEncCrop crops[2];
    memset(crops, 0, sizeof(crops));
    MdjEncCrop& c = crops[0];
    mdj_enc_set_layout(c, width, height, sampling);
    const int64_t blocks = mdj_enc_blocks(width, height, sampling);
    if (blocks > MDJ_ENC_MAX_BLOCKS) return MDJPEG_EINVAL;
    crops[1].block0 = blocks;
    std::vector<MdjKeepRect> clipped;
    for (int i = 0; i < n_rects; ++i) {
        MdjKeepRect q;
        if (mdj_keep_clip(rects + 4 * size_t(i), width, height, &q)) clipped.push_back(q);
    }
    for (int my = 0; my < c.mcus_y; ++my)
        for (int mx = 0; mx < c.mcus_x; ++mx) {
            if (mdj_keep_changed(clipped.data(), 0, int(clipped.size()), mx, my, c.hs, c.vs)) continue;
            for (int k = 0; k < c.per_mcu; ++k) {
                const int64_t o = mdj_keep_source_offset(c, mx, my, k);
                memcpy(planes + o, source + o, 128);
            }
        }
    std::vector<int16_t> coef(size_t(blocks) * 64);
    planes_to_mcu_order(c, planes, coef.data());
    MdjEncTables tables;
    mdj_enc_build_tables(tables);
    uint32_t errors = 0;
    for (int64_t g = 0; g < blocks; ++g) {
        int crop;
        uint32_t e;
        mdj_enc_lane_bits(crops, 1, coef.data(), tables, g, &crop, &e);
        errors |= e;
    }
    *status = errors ? 1 : 0;
    return MDJPEG_OK;
}

int64_t mdjpeg_encode_bound(int32_t width, int32_t height) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return -1;
    return mdj_enc_bound_bytes(width, height);
}

int64_t mdjpeg_encode_sampled_bound(int32_t width, int32_t height, int32_t sampling) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || !mdj_enc_sampling_ok(sampling)) return -1;
    return mdj_enc_bound_bytes(width, height, sampling);
}
}  // extern "C"
