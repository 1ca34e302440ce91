// The baseline Huffman ENCODER of a crop, shared by the GPU kernels (jpeg_encode.cpp) and their host model
// (mdjpeg_encode_subsequences in jpeg_encode_host.cpp): ONE encoder of a block, ONE rule for where a block's bits go, ONE
// stuffing chunk, compiled by both, so that the CPU suite and the host sanitizers exercise the very code the lanes run
// (the arrangement of jpeg_subseq.h for the decoder).
//
// What is encoded: three components, one interleaved scan without restart markers, the four example tables of the
// standard (ITU-T T.81, K.3 - K.6) -- the scan Pillow / libjpeg-turbo write for Image.save(quality = q) of an RGB image, or
// for save(qtables = ..., subsampling = ...).  The chroma sampling is a crop's own (MdjEncCrop::hs, vs: the luma sampling
// factors; chroma has 1 x 1):
//   h1v1  4:4:4  MCU  8 x 8   3 blocks  Y Cb Cr
//   h2v1  4:2:2  MCU 16 x 8   4 blocks  Y0 Y1 Cb Cr
//   h2v2  4:2:0  MCU 16 x 16  6 blocks  Y00 Y01 Y10 Y11 Cb Cr
// Block k of an MCU is luma block (k % hs, k / hs) of the MCU for k < hs * vs, then Cb, then Cr.
//
// Coefficients: the blocks of a crop in MCU ORDER (the blocks of MCU 0, then MCU 1 ...), each block TRANSPOSED
// (value (v, u) of the natural order at u * 8 + v: the column pass of the forward DCT leaves a lane one column, which it
// stores with one 16-byte store).  A luma block right of or below the component's own blocks only fills up its MCU: libjpeg
// gives it the DC of the block in front of it and no AC, so its DC difference is 0 and it costs an all-zero block's bits;
// what is stored for it is never read.
//
// Passes (each a loop over "lanes" in the host model, a launch grid over the whole batch on the device):
//   bits     lane = block: DC difference to the previous block of the component (chroma: one MCU back; luma: the last of
//            the component's own blocks in front of it), zig-zag walk, run/size symbols with ZRL
//            and EOB -> the block's bit length                                                       (mdj_enc_block, counting)
//   scan     exclusive prefix sum of the lengths; a block's offset within its crop is the difference to the crop's first
//   write    lane = block: the same walk, now writing at the offset into a zeroed buffer of 32-bit words; words a block
//            covers completely are plain stores, the first and the last are OR-ed in (atomically on the device); the last
//            block of a crop pads the last byte with 1-bits                                          (mdj_enc_block, writing)
//   count    lane = chunk of `chunk_bytes` unstuffed bytes: bytes + FF bytes = the bytes it will write
//   scan     exclusive prefix sum: where every chunk's output begins; the crops' scans lie one behind the other
//   stuff    lane = chunk: copies its bytes, a 00 behind every FF, nothing at or beyond the capacity
//
// Size of a block (MDJ_ENC_BLOCK_BITS), from the tables' worst code lengths and not from a trial: a DC code has at most 11
// bits (chroma, category 11) and 11 magnitude bits; each of the 63 AC coefficients costs at most a 16-bit code and 10
// magnitude bits (a ZRL stands for 16 zero coefficients and is shorter than one such symbol; EOB only follows a zero) --
// 22 + 63 * 26 = 1660 bits.  A crop pads at most 7 bits, and stuffing at most doubles the bytes.
#ifndef MDJPEG_ENCODE_H
#define MDJPEG_ENCODE_H

#include <stdint.h>

#include "jpeg_subseq.h"

#if defined(__HIPCC__)
#define MDJ_HD_MEMBER __host__ __device__
#else
#define MDJ_HD_MEMBER
#endif

#define MDJ_ENC_BLOCK_BITS 1660
#define MDJ_ENC_BLOCK_WORDS 52           // 1664 bits
#define MDJ_ENC_MIN_CHUNK 1              // any chunk size from one byte up is legal
#define MDJ_ENC_MAX_BLOCKS (int64_t(1) << 21)      // per crop: bit offsets within a crop stay below 2^32

#define MDJ_ENC_ERR_DC 1u                // a DC difference beyond category 11
#define MDJ_ENC_ERR_AC 2u                // an AC coefficient beyond category 10 (8-bit samples cannot give one)

// chroma sampling of a crop, numbered as Pillow's `subsampling`
#define MDJ_ENC_H1V1 0
#define MDJ_ENC_H2V1 1
#define MDJ_ENC_H2V2 2

// code and length of every symbol: table 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma; length 0 = not a symbol
struct MdjEncTables {
    uint16_t code[4][256];
    uint8_t  len[4][256];
};

// one crop of the batch; `src` / `pitch` are the device's (the host model has the coefficients already)
struct MdjEncCrop {
    const uint8_t* src;
    int64_t pitch;
    int64_t block0;                      // the crop's first block in the batch's block order
    int64_t word0;                       // the first 32-bit word of its region of the bit buffer
    int64_t chunk0;                      // its first stuffing chunk
    int32_t width, height;
    int32_t mcus_x, mcus_y;
    int32_t hs, vs;                      // luma blocks of an MCU across and down: 1 1, 2 1 or 2 2
    int32_t per_mcu;                     // blocks of an MCU: hs * vs + 2
    int32_t table;                       // its pair of quantisation tables: quant[table][2][64] (the device's)
};

MDJ_HD bool mdj_enc_sampling_ok(int sampling) { return sampling >= MDJ_ENC_H1V1 && sampling <= MDJ_ENC_H2V2; }
// width, height, sampling -> mcus_x, mcus_y, hs, vs, per_mcu of the crop
MDJ_HD void mdj_enc_set_layout(MdjEncCrop& c, int width, int height, int sampling) {
    c.width = width;
    c.height = height;
    c.hs = sampling == MDJ_ENC_H1V1 ? 1 : 2;
    c.vs = sampling == MDJ_ENC_H2V2 ? 2 : 1;
    c.per_mcu = c.hs * c.vs + 2;
    c.mcus_x = (width + 8 * c.hs - 1) / (8 * c.hs);
    c.mcus_y = (height + 8 * c.vs - 1) / (8 * c.vs);
}
MDJ_HD int64_t mdj_enc_blocks(int width, int height, int sampling = MDJ_ENC_H2V2) {
    MdjEncCrop c;
    mdj_enc_set_layout(c, width, height, sampling);
    return int64_t(c.mcus_x) * c.mcus_y * c.per_mcu;
}
// 32-bit words of a crop's region of the bit buffer: every block at its bound, and the padding bits
MDJ_HD int64_t mdj_enc_region_words(int64_t blocks) { return blocks * MDJ_ENC_BLOCK_WORDS + 1; }
MDJ_HD int64_t mdj_enc_region_chunks(int64_t blocks, int chunk_bytes) {
    return (mdj_enc_region_words(blocks) * 4 + chunk_bytes - 1) / chunk_bytes;
}
// what a crop's scan can take at most: every byte of the region an FF
MDJ_HD int64_t mdj_enc_bound_bytes(int width, int height, int sampling = MDJ_ENC_H2V2) {
    return mdj_enc_region_words(mdj_enc_blocks(width, height, sampling)) * 8;
}

// the standard's tables as DHT segments carry them: codes of each length, then the symbols
static const uint8_t MDJ_ENC_STD_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                                {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                                {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                                {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t MDJ_ENC_STD_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t MDJ_ENC_STD_AC_LUMA[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t MDJ_ENC_STD_AC_CHROMA[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// canonical codes of the four tables (T.81 Annex C); host only
inline void mdj_enc_build_tables(MdjEncTables& t) {
    memset(&t, 0, sizeof(t));
    const uint8_t* vals[4] = {MDJ_ENC_STD_DC_VALS, MDJ_ENC_STD_AC_LUMA, MDJ_ENC_STD_DC_VALS, MDJ_ENC_STD_AC_CHROMA};
    for (int k = 0; k < 4; ++k) {
        unsigned code = 0;
        int p = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < MDJ_ENC_STD_BITS[k][l - 1]; ++i, ++p) {
                t.code[k][vals[k][p]] = uint16_t(code++);
                t.len[k][vals[k][p]] = uint8_t(l);
            }
            code <<= 1;
        }
    }
}

// the crop that holds item g (a block or a chunk): the largest c with crops[c].*FIRST <= g, FIRST = &MdjEncCrop::block0 or
// &MdjEncCrop::chunk0.  crops has n + 1 entries; the last one carries the totals, so crops[n].*FIRST > g for every item.
template <int64_t MdjEncCrop::*FIRST>
MDJ_HD int mdj_enc_locate(const MdjEncCrop* crops, int n, int64_t g) {
    int lo = 0, hi = n;                  // crops[lo].first <= g < crops[hi].first
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (crops[mid].*FIRST <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// block k of MCU m is one of the component's own (chroma blocks always are)
MDJ_HD bool mdj_enc_block_real(const MdjEncCrop& c, int64_t m, int k) {
    if (k >= c.hs * c.vs) return true;
    const int kx = c.hs == 2 ? k & 1 : 0, ky = c.hs == 2 ? k >> 1 : k;
    const uint32_t my = uint32_t(m) / uint32_t(c.mcus_x), mx = uint32_t(m) - my * uint32_t(c.mcus_x);    // (at most 2^21 blocks a crop)
    const int bx = int(mx) * c.hs + kx, by = int(my) * c.vs + ky;
    return bx < (c.width + 7) / 8 && by < (c.height + 7) / 8;
}

// DC difference of block `lb` of the crop (coef: the crop's first block)
MDJ_HD int mdj_enc_dc_diff(const int16_t* coef, const MdjEncCrop& c, int64_t lb) {
    const int64_t m = int64_t(uint32_t(lb) / uint32_t(c.per_mcu));
    const int k = int(lb - m * c.per_mcu);
    if (!mdj_enc_block_real(c, m, k)) return 0;
    const int cur = coef[lb * 64];
    if (k >= c.hs * c.vs) return m == 0 ? cur : cur - coef[(lb - c.per_mcu) * 64];
    // luma: the last block of the component's own in front of this one (block 0 of an MCU always is one)
    int64_t pm = m;
    int pk = k - 1;
    if (pk < 0) {
        if (m == 0) return cur;
        pm = m - 1;
        pk = c.hs * c.vs - 1;
    }
    while (!mdj_enc_block_real(c, pm, pk)) --pk;
    return cur - coef[(pm * c.per_mcu + pk) * 64];
}

MDJ_HD int mdj_enc_bit_length(unsigned v) { return v == 0 ? 0 : 32 - __builtin_clz(v); }

// counts the bits
struct MdjEncCount {
    uint32_t bits = 0;
    MDJ_HD_MEMBER void put(uint32_t, int n) { bits += uint32_t(n); }
};

MDJ_HD void mdj_enc_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

// writes the bits from bit `pos` of the zeroed word buffer on (bit 0 = the top bit of byte 0)
struct MdjEncWriter {
    uint32_t* words;
    int64_t w;                           // the word the pending bits belong to
    uint64_t acc;                        // pending bits, right-aligned
    int nacc;                            // how many (below 32 between calls); the first word's leading bits count as zeros
    bool shared;                         // the next word to go out is the block's first: neighbours own part of it
    MDJ_HD_MEMBER MdjEncWriter(uint32_t* words_, int64_t pos) : words(words_), w(pos >> 5), acc(0), nacc(int(pos & 31)), shared(true) {}
    MDJ_HD_MEMBER void flush(uint32_t big_endian, bool last) {
        const uint32_t v = __builtin_bswap32(big_endian);
        if (shared || last) mdj_enc_or(words + w, v); else words[w] = v;
        shared = false;
        ++w;
    }
    MDJ_HD_MEMBER void put(uint32_t v, int n) {              // n <= 27
        acc = (acc << n) | v;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            flush(uint32_t(acc >> nacc), false);
            acc &= (uint64_t(1) << nacc) - 1;
        }
    }
    MDJ_HD_MEMBER void finish() {
        if (nacc > 0) flush(uint32_t(acc << (32 - nacc)), true);
    }
};

// One block: `diff` its DC difference, blk its 64 transposed coefficients (blk[0] is not read), `real` false for a block
// that only fills up its MCU.  Returns MDJ_ENC_ERR_* bits; the symbols put are valid ones whatever the values are.
template <class Sink>
MDJ_HD uint32_t mdj_enc_block(const int16_t* blk, int diff, bool real, const MdjEncTables& t, int chroma, Sink& s) {
    uint32_t err = 0;
    const uint16_t* dcc = t.code[chroma * 2];
    const uint8_t* dcl = t.len[chroma * 2];
    const uint16_t* acc = t.code[chroma * 2 + 1];
    const uint8_t* acl = t.len[chroma * 2 + 1];
    int temp = diff, temp2 = diff;
    if (temp < 0) {
        temp = -temp;
        --temp2;
    }
    int nbits = mdj_enc_bit_length(unsigned(temp));
    if (nbits > 11) {
        err |= MDJ_ENC_ERR_DC;
        nbits = 11;
    }
    s.put((uint32_t(dcc[nbits]) << nbits) | (uint32_t(temp2) & ((1u << nbits) - 1u)), dcl[nbits] + nbits);
    int run = 0;
    if (real) {
        for (int k = 1; k < 64; ++k) {
            const int zz = mdj_zigzag(k);
            const int v = blk[((zz & 7) << 3) | (zz >> 3)];
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                s.put(acc[0xF0], acl[0xF0]);
                run -= 16;
            }
            temp = v;
            temp2 = v;
            if (temp < 0) {
                temp = -temp;
                --temp2;
            }
            nbits = mdj_enc_bit_length(unsigned(temp));
            if (nbits > 10) {
                err |= MDJ_ENC_ERR_AC;
                nbits = 10;
            }
            const int sym = (run << 4) | nbits;
            s.put((uint32_t(acc[sym]) << nbits) | (uint32_t(temp2) & ((1u << nbits) - 1u)), acl[sym] + nbits);
            run = 0;
        }
    } else {
        run = 63;
    }
    if (run > 0) s.put(acc[0], acl[0]);
    return err;
}

// ---- the passes' lanes -----------------------------------------------------------------------------------------------
// bits: global block g -> its length (*err receives the block's error bits)
MDJ_HD uint32_t mdj_enc_lane_bits(const MdjEncCrop* crops, int n, const int16_t* coef, const MdjEncTables& t, int64_t g, int* crop,
                                  uint32_t* err) {
    const int c = mdj_enc_locate<&MdjEncCrop::block0>(crops, n, g);
    const MdjEncCrop& cr = crops[c];
    const int64_t lb = g - cr.block0;
    const int16_t* base = coef + cr.block0 * 64;
    MdjEncCount count;
    const int64_t m = int64_t(uint32_t(lb) / uint32_t(cr.per_mcu));
    const int k = int(lb - m * cr.per_mcu);
    *err = mdj_enc_block(base + lb * 64, mdj_enc_dc_diff(base, cr, lb), mdj_enc_block_real(cr, m, k), t, k >= cr.hs * cr.vs, count);
    *crop = c;
    return count.bits;
}

// bits of a crop, from the exclusive scan of the lengths (offsets[total] = the sum)
MDJ_HD uint64_t mdj_enc_crop_bits(const MdjEncCrop* crops, int c, const uint64_t* offsets) {
    return offsets[crops[c + 1].block0] - offsets[crops[c].block0];
}
MDJ_HD int64_t mdj_enc_crop_bytes(const MdjEncCrop* crops, int c, const uint64_t* offsets) {
    return int64_t((mdj_enc_crop_bits(crops, c, offsets) + 7) >> 3);
}

// write: global block g -> its bits in the crop's region of the bit buffer
MDJ_HD void mdj_enc_lane_write(const MdjEncCrop* crops, int n, const int16_t* coef, const MdjEncTables& t, const uint64_t* offsets,
                               uint32_t* bitbuf, int64_t g) {
    const int c = mdj_enc_locate<&MdjEncCrop::block0>(crops, n, g);
    const MdjEncCrop& cr = crops[c];
    const int64_t lb = g - cr.block0;
    const int16_t* base = coef + cr.block0 * 64;
    MdjEncWriter w(bitbuf + cr.word0, int64_t(offsets[g] - offsets[cr.block0]));
    const int64_t m = int64_t(uint32_t(lb) / uint32_t(cr.per_mcu));
    const int k = int(lb - m * cr.per_mcu);
    mdj_enc_block(base + lb * 64, mdj_enc_dc_diff(base, cr, lb), mdj_enc_block_real(cr, m, k), t, k >= cr.hs * cr.vs, w);
    if (g + 1 == crops[c + 1].block0) {                              // the crop's last block fills the last byte with 1-bits
        const int pad = int((8 - (mdj_enc_crop_bits(crops, c, offsets) & 7)) & 7);
        if (pad) w.put((1u << pad) - 1u, pad);
    }
    w.finish();
}

// the unstuffed bytes [lo, hi) of chunk j of its crop (empty behind the crop's last byte)
MDJ_HD void mdj_enc_chunk_range(const MdjEncCrop* crops, int c, const uint64_t* offsets, int64_t j, int chunk_bytes, int64_t* lo, int64_t* hi) {
    const int64_t nb = mdj_enc_crop_bytes(crops, c, offsets);
    const int64_t a = j * chunk_bytes;
    *lo = a < nb ? a : nb;
    *hi = a + chunk_bytes < nb ? a + chunk_bytes : nb;
}

// count: global chunk q -> the bytes it will write
MDJ_HD uint32_t mdj_enc_lane_count(const MdjEncCrop* crops, int n, const uint64_t* offsets, const uint32_t* bitbuf, int chunk_bytes, int64_t q) {
    const int c = mdj_enc_locate<&MdjEncCrop::chunk0>(crops, n, q);
    int64_t lo, hi;
    mdj_enc_chunk_range(crops, c, offsets, q - crops[c].chunk0, chunk_bytes, &lo, &hi);
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bitbuf + crops[c].word0);
    uint32_t count = uint32_t(hi - lo);
    for (int64_t i = lo; i < hi; ++i) count += b[i] == 0xFF;
    return count;
}

// stuff: global chunk q -> its bytes at out[starts[q] ...], a 00 behind every FF, nothing at or beyond `capacity`
MDJ_HD void mdj_enc_lane_stuff(const MdjEncCrop* crops, int n, const uint64_t* offsets, const uint32_t* bitbuf, int chunk_bytes,
                               const uint64_t* starts, uint8_t* out, int64_t capacity, int64_t q) {
    const int c = mdj_enc_locate<&MdjEncCrop::chunk0>(crops, n, q);
    int64_t lo, hi;
    mdj_enc_chunk_range(crops, c, offsets, q - crops[c].chunk0, chunk_bytes, &lo, &hi);
    const uint8_t* b = reinterpret_cast<const uint8_t*>(bitbuf + crops[c].word0);
    int64_t o = int64_t(starts[q]);
    for (int64_t i = lo; i < hi; ++i) {
        const uint8_t v = b[i];
        if (o < capacity) out[o] = v;
        ++o;
        if (v == 0xFF) {
            if (o < capacity) out[o] = 0;
            ++o;
        }
    }
}

#endif  // MDJPEG_ENCODE_H
