// The self-synchronising Huffman decoder of a baseline JPEG scan, shared by the GPU kernels (jpeg_huffman.cpp) and their
// host model (mdjpeg_decode_subsequences in jpeg_entropy.cpp): ONE decoder of a subsequence, ONE state record, ONE rule of
// synchronisation, compiled by both, so that the CPU suite and the host sanitizers exercise the very code the lanes run.
//
// A restart segment (or the whole scan) is cut into subsequences of `subseq_bits` raw bits.  A position is a raw bit offset
// into the segment's bytes, stuffing bytes (the 00 behind an FF) included but never pointed at.  A lane's state at a position
// is the block of the MCU it is in (which gives component and tables) and the zig-zag index it is at; k == 0 means "a DC
// code is next".  Decoding a subsequence from a (position, state) is a pure function, so the lanes can be run until every
// lane's start equals its left neighbour's end ("Entropy decoding on the GPU").
#ifndef MDJPEG_SUBSEQ_H
#define MDJPEG_SUBSEQ_H

#include <stdint.h>
#include <string.h>

#include "../../include/mdjpeg.h"

#if defined(__HIPCC__)
#define MDJ_HD __host__ __device__ inline
#else
#define MDJ_HD inline
#endif

#define MDJ_LOOK 9                       // bits of the first-level lookup
#define MDJ_MAX_TABLES 6
#define MDJ_MAX_SUBSEQ_BITS 65536        // a lane closes fewer than 65536 blocks (MdjState.n): a block takes at least 2 bits
#define MDJ_MIN_SUBSEQ_BITS 64           // a symbol with its magnitude bits and the stuffing in between stays below this
#define MDJ_MAX_SCAN_BYTES (int64_t(1) << 28)   // bit positions are 32 bits
#define MDJ_ENERGY_CAP (int64_t(1) << 23)   // above every energy bound (2800^2): a partial sum is cut off here

struct MdjTable {
    uint16_t look[1 << MDJ_LOOK];        // (length << 8) | symbol, 0 = longer than MDJ_LOOK bits or undefined
    int32_t  maxcode[18];                // largest code of each length, -1 = none
    int32_t  valoff[17];                 // index of the first symbol of a length minus its first code
    uint8_t  vals[256];
    uint8_t  pad[4];
};

// what the lanes of one image share; no pointers, so that it can be copied to the device and into LDS as it is
struct MdjImage {
    MdjTable tables[MDJ_MAX_TABLES];
    uint16_t quant[3][64];               // natural order
    int64_t  emax[3];                    // the energy bound of a block of each component (mdj_energy_bound)
    int64_t  plane_offset[3];
    int32_t  blocks_w[3];
    int32_t  h_samp[3], v_samp[3];
    int32_t  dc_table[3], ac_table[3];
    int32_t  components;
    int32_t  mcus_x;
    int32_t  blocks_per_mcu;
    int32_t  comp_of[8];                 // block of the MCU -> component
    int32_t  first_of[3];                // component -> its first block of the MCU
    int64_t  total_mcus;
    int64_t  interval;                   // MCUs per segment (total_mcus when the file has no restart interval)
    int32_t  subseq_bits;
    int32_t  pad;
};

struct MdjState {
    uint32_t pos;                        // raw bit offset in the segment, never inside a stuffing byte
    uint8_t  k;                          // zig-zag index that is next (0: a DC code)
    uint8_t  m;                          // block of the MCU
    uint16_t n;                          // blocks closed by the decode that ended here
};

MDJ_HD uint64_t mdj_pack(MdjState s) { return uint64_t(s.pos) | (uint64_t(s.k) << 32) | (uint64_t(s.m) << 40) | (uint64_t(s.n) << 48); }
MDJ_HD MdjState mdj_unpack(uint64_t w) { return MdjState{uint32_t(w), uint8_t(w >> 32), uint8_t(w >> 40), uint16_t(w >> 48)}; }
// what a right neighbour starts from: position and state, not the count
MDJ_HD uint64_t mdj_start_key(uint64_t w) { return w & 0x0000ffffffffffffull; }

// reasons a final lane flags (status word of an image; any bit = MDJPEG_ECORRUPT)
#define MDJ_ERR_CODE      1u    // undefined Huffman code
#define MDJ_ERR_CATEGORY  2u    // DC category above 11, AC category above 10
#define MDJ_ERR_INDEX     4u    // coefficient index past 63, zero run leaves the block, end-of-band code
#define MDJ_ERR_EARLY     8u    // data end early
#define MDJ_ERR_LEFTOVER  16u   // bytes left over in front of a marker
#define MDJ_ERR_COUNT     32u   // a segment does not hold exactly its MCUs
#define MDJ_ERR_ENERGY    64u   // block energy beyond what 8-bit samples can hold
#define MDJ_ERR_DC        128u  // DC value out of range

// natural index of zig-zag position k
#if defined(__HIPCC__)
__device__ __constant__
#endif
static const uint8_t MDJ_ZIGZAG_DEV[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t MDJ_ZIGZAG_HOST[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
MDJ_HD int mdj_zigzag(int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return MDJ_ZIGZAG_DEV[k & 63];
#else
    return MDJ_ZIGZAG_HOST[k & 63];
#endif
}

// ---- bit reader over one segment: d[0 .. nb) --------------------------------------------------------------------------
struct MdjBits {
    const uint8_t* d;
    uint32_t nb;          // bytes of the segment
    uint32_t bi;          // next raw byte to load
    uint32_t pos;         // raw bit position of the next bit
    uint64_t acc;         // next bit = bit 63; zeros behind the data
    int      n;           // bits of acc that came from the data (may go negative behind the end)
};

MDJ_HD bool mdj_is_stuffing(const uint8_t* d, uint32_t nb, uint32_t i) { return i > 0 && i < nb && d[i] == 0 && d[i - 1] == 0xFF; }

MDJ_HD void mdj_fill(MdjBits& b) {
    while (b.n <= 56 && b.bi < b.nb) {
        const unsigned v = b.d[b.bi];
        if (v == 0 && b.bi > 0 && b.d[b.bi - 1] == 0xFF) { ++b.bi; continue; }
        b.acc |= uint64_t(v) << (56 - b.n);
        b.n += 8;
        ++b.bi;
    }
}

// pos: a position as mdj_normalise gives it
MDJ_HD void mdj_seek(MdjBits& b, const uint8_t* d, uint32_t nb, uint32_t pos) {
    b.d = d; b.nb = nb; b.pos = pos; b.acc = 0; b.n = 0;
    b.bi = pos >> 3;
    if (b.bi > nb) b.bi = nb;
    mdj_fill(b);
    const int sh = int(pos & 7);
    b.acc <<= sh;
    b.n -= sh;
}

// the first position at or behind `pos` that is not inside a stuffing byte
MDJ_HD uint32_t mdj_normalise(const uint8_t* d, uint32_t nb, uint32_t pos) {
    if ((pos & 7) == 0 && mdj_is_stuffing(d, nb, pos >> 3)) return pos + 8;
    return pos;
}

MDJ_HD unsigned mdj_peek(const MdjBits& b, int k) { return unsigned(b.acc >> (64 - k)); }

// consumes k (1 .. 16) bits; the raw position steps over the stuffing bytes it meets
MDJ_HD void mdj_skip(MdjBits& b, int k) {
    b.acc <<= k;
    b.n -= k;
    uint32_t byte = b.pos >> 3;
    const uint32_t bit = (b.pos & 7) + uint32_t(k);
    for (uint32_t c = bit >> 3; c > 0; --c) {
        ++byte;
        if (mdj_is_stuffing(b.d, b.nb, byte)) ++byte;
    }
    b.pos = byte * 8 + (bit & 7);
}

// fewer than 8 data bits between pos and the end of the segment (only padding may be left)
MDJ_HD bool mdj_only_padding_left(const uint8_t* d, uint32_t nb, uint32_t pos) {
    const uint32_t total = nb * 8;
    if (pos >= total) return true;
    if (total - pos >= 24) return false;
    uint32_t left = 8 - (pos & 7);
    for (uint32_t i = (pos >> 3) + 1; i < nb; ++i)
        if (!mdj_is_stuffing(d, nb, i)) left += 8;
    return left < 8;
}

// one Huffman symbol; -1: undefined code.  The caller checks afterwards whether the position ran past the data.
MDJ_HD int mdj_symbol(MdjBits& b, const MdjTable& h) {
    const unsigned e = h.look[mdj_peek(b, MDJ_LOOK)];
    if (e) {
        mdj_skip(b, int(e >> 8));
        return int(e & 255);
    }
    const unsigned v = mdj_peek(b, 16);
    for (int len = MDJ_LOOK + 1; len <= 16; ++len) {
        const int code = int(v >> (16 - len));
        if (code <= h.maxcode[len]) {
            mdj_skip(b, len);
            return h.vals[(code + h.valoff[len]) & 255];
        }
    }
    return -1;
}

MDJ_HD int mdj_receive_extend(MdjBits& b, int s) {
    const int v = int(mdj_peek(b, s));
    mdj_skip(b, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Where a final lane puts what it decodes.  coef == nullptr: a speculative lane, which writes and flags nothing.
struct MdjSink {
    int16_t*  coef;          // the image's planes
    uint32_t* energy;        // per block of the image (index = coefficient offset / 64): AC energy, added atomically
    int64_t   first_mcu;     // of the segment
    int64_t   block;         // index, within the segment, of the block the lane is in
    int64_t   blocks;        // the segment holds exactly this many
    uint32_t  err;           // MDJ_ERR_* the lane met
};

// offset, in blocks from the buffer's start, of block `j` (decode order within the segment)
MDJ_HD int64_t mdj_block_offset(const MdjImage& im, int64_t first_mcu, int64_t j, int* comp) {
    const int64_t mcu = first_mcu + j / im.blocks_per_mcu;
    const int m = int(j % im.blocks_per_mcu);
    const int c = im.comp_of[m];
    const int sub = m - im.first_of[c];
    const int64_t my = mcu / im.mcus_x, mx = mcu % im.mcus_x;
    const int64_t by = my * im.v_samp[c] + sub / im.h_samp[c], bx = mx * im.h_samp[c] + sub % im.h_samp[c];
    *comp = c;
    return im.plane_offset[c] / 64 + by * im.blocks_w[c] + bx;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define MDJ_ENERGY_ADD(p, v) atomicAdd((p), (v))
#else
#define MDJ_ENERGY_ADD(p, v) (*(p) += (v))
#endif

// Decodes the symbols that START in [s.pos, limit) of the segment d[0 .. nb), from state s.  Returns where it ended and in
// which state, with the number of blocks it closed.  A speculative lane (sink == nullptr) decodes whatever the bits say and
// carries on behind nonsense; a final lane writes coefficients (DC as the DIFFERENCE), stops at the first error and at the
// last block of the segment, and says in sink->err what it met.
MDJ_HD MdjState mdj_decode_lane(const MdjImage& im, const MdjTable* tables, const uint8_t* d, uint32_t nb, MdjState s, uint32_t limit,
                                MdjSink* sink) {
    const uint32_t total = nb * 8;
    if (limit > total) limit = total;
    MdjBits b;
    mdj_seek(b, d, nb, s.pos);
    int k = s.k & 63, m = s.m < im.blocks_per_mcu ? s.m : 0;
    unsigned closed = 0;
    const bool fin = sink != nullptr;
    int16_t* blk = nullptr;
    uint32_t* eng = nullptr;
    const uint16_t* q = im.quant[0];
    int64_t energy = 0;
    bool have_block = false;
    if (fin && sink->block >= sink->blocks) return MdjState{s.pos, uint8_t(k), uint8_t(m), 0};
    while (b.pos < limit) {
        if (b.n < 32) mdj_fill(b);
        const int c = im.comp_of[m];
        if (fin && !have_block) {
            int cc;
            const int64_t off = mdj_block_offset(im, sink->first_mcu, sink->block, &cc);
            blk = sink->coef + off * 64;
            eng = sink->energy + off;
            q = im.quant[cc];
            have_block = true;
            energy = 0;
        }
        bool close = false;
        uint32_t err = 0;
        if (k == 0) {
            const int sz = mdj_symbol(b, tables[im.dc_table[c]]);
            if (sz < 0) { err = MDJ_ERR_CODE; if (!fin) mdj_skip(b, 1); }
            else if (sz > 11) err = MDJ_ERR_CATEGORY;
            else {
                const int v = sz ? mdj_receive_extend(b, sz) : 0;
                if (fin && b.pos <= total) blk[0] = int16_t(v);
                k = 1;
            }
        } else {
            const int rs = mdj_symbol(b, tables[im.ac_table[c]]);
            if (rs < 0) { err = MDJ_ERR_CODE; if (!fin) mdj_skip(b, 1); }
            else {
                const int r = rs >> 4, sz = rs & 15;
                if (sz) {
                    k += r;
                    if (k > 63) { err = MDJ_ERR_INDEX; close = true; }
                    else if (sz > 10) { err = MDJ_ERR_CATEGORY; }
                    else {
                        const int v = mdj_receive_extend(b, sz);
                        if (fin && b.pos <= total) {
                            const int nat = mdj_zigzag(k);
                            blk[nat] = int16_t(v);
                            const int64_t dv = int64_t(v) * q[nat];
                            energy += dv * dv;
                            if (energy > MDJ_ENERGY_CAP) energy = MDJ_ENERGY_CAP;
                        }
                        if (++k > 63) close = true;
                    }
                } else if (r == 15) {
                    k += 16;
                    if (k > 63) { err = MDJ_ERR_INDEX; close = true; }
                } else if (r == 0) {
                    close = true;
                } else {
                    err = MDJ_ERR_INDEX;
                }
            }
        }
        if (b.pos > total) {                      // the symbol ran past the data: nothing of it counts
            if (fin) sink->err |= MDJ_ERR_EARLY;
            b.pos = total;
            break;
        }
        if (fin && err) { sink->err |= err; break; }
        if (close) {
            k = 0;
            m = m + 1 < im.blocks_per_mcu ? m + 1 : 0;
            ++closed;
            if (fin) {
                if (energy) MDJ_ENERGY_ADD(eng, uint32_t(energy));
                have_block = false;
                energy = 0;
                if (++sink->block >= sink->blocks) {
                    if (!mdj_only_padding_left(d, nb, b.pos)) sink->err |= MDJ_ERR_LEFTOVER;
                    break;
                }
            }
        }
    }
    if (fin && have_block && energy) MDJ_ENERGY_ADD(eng, uint32_t(energy));
    return MdjState{b.pos, uint8_t(k), uint8_t(m), uint16_t(closed > 0xffff ? 0xffff : closed)};
}

// lanes of a segment of nb bytes (at least one: an empty segment still has to be found empty)
MDJ_HD uint32_t mdj_lanes_of(uint32_t nb, uint32_t subseq_bits) {
    const uint32_t n = uint32_t((uint64_t(nb) * 8 + subseq_bits - 1) / subseq_bits);
    return n ? n : 1;
}
MDJ_HD uint32_t mdj_lane_limit(uint32_t sub, uint32_t subseq_bits) {
    const uint64_t e = (uint64_t(sub) + 1) * subseq_bits;
    return e > 0xffffffffull ? 0xffffffffu : uint32_t(e);
}

// offset, in blocks from the buffer's start, of block `j` of component c in decode order (over the whole image)
MDJ_HD int64_t mdj_dc_block_offset(const MdjImage& im, int c, int64_t j) {
    const int per_mcu = im.h_samp[c] * im.v_samp[c];
    const int64_t mcu = j / per_mcu;
    const int sub = int(j % per_mcu);
    const int64_t by = (mcu / im.mcus_x) * im.v_samp[c] + sub / im.h_samp[c], bx = (mcu % im.mcus_x) * im.h_samp[c] + sub % im.h_samp[c];
    return im.plane_offset[c] / 64 + by * im.blocks_w[c] + bx;
}

// the start of lane `sub` of a segment before anything is known: its first bit, a DC code of the MCU's first block
MDJ_HD MdjState mdj_blind_start(const uint8_t* d, uint32_t nb, uint32_t sub, uint32_t subseq_bits) {
    return MdjState{mdj_normalise(d, nb, sub * subseq_bits), 0, 0, 0};
}

// The DC value and the energy bound of a block: `dc` is the running sum of the differences (64 bits: no sum of 11-bit
// differences leaves them), ac_energy what the final lanes added up.  Returns MDJ_ERR_* bits.
MDJ_HD uint32_t mdj_check_block(const MdjImage& im, int c, int64_t dc, uint32_t ac_energy) {
    if (dc < -32768 || dc > 32767) return MDJ_ERR_DC;
    const int64_t v0 = dc * im.quant[c][0];
    return v0 * v0 + int64_t(ac_energy) > im.emax[c] ? MDJ_ERR_ENERGY : 0u;
}

// ---- host side: tables and bounds --------------------------------------------------------------------------------------
// Builds the decoding tables of one DHT entry; false when the counts do not describe a prefix code.
inline bool mdj_build_table(MdjTable& h, const uint8_t* counts, const uint8_t* vals) {
    for (int i = 0; i < (1 << MDJ_LOOK); ++i) h.look[i] = 0;
    for (int i = 0; i < 256; ++i) h.vals[i] = 0;
    h.pad[0] = h.pad[1] = h.pad[2] = h.pad[3] = 0;
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = counts[len - 1];
        h.valoff[len] = k - code;
        if (n) {
            if (code + n > (1 << len) || k + n > 256) return false;
            for (int i = 0; i < n; ++i) h.vals[k + i] = vals[k + i];
            if (len <= MDJ_LOOK)
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (MDJ_LOOK - len);
                    for (int j = 0; j < (1 << (MDJ_LOOK - len)); ++j) h.look[first + j] = uint16_t((len << 8) | vals[k + i]);
                }
            k += n;
            code += n;
            h.maxcode[len] = code - 1;
        } else {
            h.maxcode[len] = -1;
        }
        code <<= 1;
    }
    h.valoff[0] = 0;
    h.maxcode[0] = -1;
    h.maxcode[17] = 0x7fffffff;
    return true;
}

// Parseval: the coefficients of 64 samples in [-128, 127] have a 2-norm of at most 8 * 128; quantisation moves every
// coefficient by at most half its step (mdjpeg_decode has the same bound).
inline int64_t mdj_energy_bound(const uint16_t* quant) {
    double qn = 0;
    for (int i = 0; i < 64; ++i) qn += double(quant[i]) * quant[i];
    double lim = 1024.0 + 0.5 * __builtin_sqrt(qn) + 1.0;
    if (lim > 2800.0) lim = 2800.0;
    return int64_t(lim * lim);
}

// what the lanes of an image share, from its descriptor; false when a table is not a prefix code or the descriptor is not
// one that mdjpeg_scan writes
inline bool mdj_fill_image(const mdjpeg_scan_info& sc, int subseq_bits, MdjImage& im) {
    memset(&im, 0, sizeof(im));
    const mdjpeg_info& in = sc.info;
    if ((in.components != 1 && in.components != 3) || sc.n_tables < 1 || sc.n_tables > MDJ_MAX_TABLES) return false;
    for (int t = 0; t < sc.n_tables; ++t) {
        int total = 0;
        for (int i = 0; i < 16; ++i) total += sc.huff_counts[t][i];
        if (total > 256 || !mdj_build_table(im.tables[t], sc.huff_counts[t], sc.huff_vals[t])) return false;
    }
    int m = 0;
    for (int c = 0; c < in.components; ++c) {
        if (in.h_samp[c] < 1 || in.v_samp[c] < 1 || in.h_samp[c] * in.v_samp[c] > 4 || m + in.h_samp[c] * in.v_samp[c] > 8) return false;
        if (sc.dc_table[c] < 0 || sc.dc_table[c] >= sc.n_tables || sc.ac_table[c] < 0 || sc.ac_table[c] >= sc.n_tables) return false;
        memcpy(im.quant[c], in.quant[c], sizeof(im.quant[c]));
        im.emax[c] = mdj_energy_bound(in.quant[c]);
        im.plane_offset[c] = in.plane_offset[c];
        im.blocks_w[c] = in.blocks_w[c];
        im.h_samp[c] = in.h_samp[c];
        im.v_samp[c] = in.v_samp[c];
        im.dc_table[c] = sc.dc_table[c];
        im.ac_table[c] = sc.ac_table[c];
        im.first_of[c] = m;
        for (int i = 0; i < in.h_samp[c] * in.v_samp[c]; ++i) im.comp_of[m++] = c;
    }
    for (int c = in.components; c < 3; ++c) im.h_samp[c] = im.v_samp[c] = 1;
    im.components = in.components;
    im.mcus_x = in.mcus_x;
    im.blocks_per_mcu = m;
    im.total_mcus = int64_t(in.mcus_x) * in.mcus_y;
    im.interval = in.restart_interval > 0 ? in.restart_interval : im.total_mcus;
    im.subseq_bits = subseq_bits;
    return im.total_mcus > 0;
}

#endif  // MDJPEG_SUBSEQ_H
