// libmdjpeg.so: JPEG marker parser and Huffman entropy decoder of the loader processes (C ABI: include/mdjpeg.h).
//
// Plain C++17, host compiler, no HIP: a loader process that maps this library does not open the GPU.  The output is the
// scan's QUANTISED coefficients; de-quantisation, IDCT, upsampling, colour conversion and rotation are
// mdhip_jpeg_reconstruct (jpeg_kernels.cpp).  Every irregularity is an error code -- the caller then decodes the file
// with PIL, so that no behaviour of the ordinary path (warnings, partial images, failure strings) is restated here.
//
// Decoder: 64-bit left-aligned bit buffer refilled eight bytes at a time while no 0xFF is in sight; one 11-bit look-ahead
// per symbol that yields code length and run/size together; the canonical maxcode walk for the rare longer codes.

#include "../../include/mdjpeg.h"
#include "jpeg_subseq.h"
#include "jpeg_encode.h"
#include "jpeg_keep.h"
#include "blur_box.h"
#include "resample.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

constexpr int LOOK = 11;

const uint8_t ZIGZAG[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool     defined = false;
    uint16_t look[1 << LOOK];      // (length << 8) | symbol, 0 = longer than LOOK bits or undefined
    int32_t  maxcode[18];          // largest code of each length, -1 = none
    int32_t  valoff[17];           // index of the first symbol of a length minus its first code
    uint8_t  vals[256];
    uint8_t  counts[16];           // as the file writes them (mdjpeg_scan hands them on)
};

struct Parsed {
    Huff     dc[4], ac[4];
    uint16_t qt[4][64];            // natural order
    bool     qt_defined[4] = {false, false, false, false};
    int      comp_id[4], comp_tq[4], comp_td[4], comp_ta[4];
    size_t   scan_begin = 0;       // first byte of entropy-coded data
};

int fail(mdjpeg_info* info, int code, const char* why) {
    snprintf(info->reason, sizeof(info->reason), "%s", why);
    info->supported = 0;
    return code;
}

// Builds the decoding tables of one DHT entry; false when the counts do not describe a prefix code.
bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
    memset(h.look, 0, sizeof(h.look));
    memset(h.vals, 0, sizeof(h.vals));
    memcpy(h.vals, vals, nvals);
    memcpy(h.counts, counts, 16);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        int n = counts[len - 1];
        h.valoff[len] = k - code;
        if (n) {
            if (code + n > (1 << len)) return false;
            if (len <= LOOK) {
                for (int i = 0; i < n; ++i) {
                    int first = (code + i) << (LOOK - len);
                    for (int j = 0; j < (1 << (LOOK - len)); ++j) h.look[first + j] = uint16_t((len << 8) | vals[k + i]);
                }
            }
            k += n;
            code += n;
            h.maxcode[len] = code - 1;
        } else {
            h.maxcode[len] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.defined = true;
    return true;
}

inline unsigned be16(const uint8_t* p) { return (unsigned(p[0]) << 8) | p[1]; }

int parse_headers(const uint8_t* d, size_t size, mdjpeg_info* info, Parsed& P) {
    memset(info, 0, sizeof(*info));
    if (size < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(info, MDJPEG_EUNSUPPORTED, "not a JPEG file (no SOI marker)");
    size_t p = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    for (;;) {
        if (p + 4 > size) return fail(info, MDJPEG_EUNSUPPORTED, "file ends inside the headers");
        if (d[p] != 0xFF) return fail(info, MDJPEG_EUNSUPPORTED, "bytes between marker segments");
        while (p < size && d[p] == 0xFF) ++p;                        // fill bytes in front of a marker are legal here
        if (p + 3 > size) return fail(info, MDJPEG_EUNSUPPORTED, "file ends inside the headers");
        int m = d[p++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;        // parameterless
        if (m == 0xD9) return fail(info, MDJPEG_EUNSUPPORTED, "EOI before any scan");
        if (m == 0x00) return fail(info, MDJPEG_EUNSUPPORTED, "bytes between marker segments");
        size_t len = be16(d + p);
        if (len < 2 || p + len > size) return fail(info, MDJPEG_EUNSUPPORTED, "marker segment runs past the end of the file");
        const uint8_t* s = d + p + 2;
        size_t n = len - 2;
        switch (m) {
        case 0xC0: case 0xC1: {
            if (have_sof) return fail(info, MDJPEG_EUNSUPPORTED, "more than one frame header");
            if (n < 6) return fail(info, MDJPEG_EUNSUPPORTED, "short frame header");
            int prec = s[0];
            info->height = int(be16(s + 1));
            info->width = int(be16(s + 3));
            info->components = s[5];
            if (prec != 8) return fail(info, MDJPEG_EUNSUPPORTED, "sample precision is not 8 bits");
            if (info->width < 1 || info->height < 1) return fail(info, MDJPEG_EUNSUPPORTED, "frame header without a size (DNL)");
            if (info->components == 4) return fail(info, MDJPEG_EUNSUPPORTED, "four components (CMYK / YCCK)");
            if (info->components != 1 && info->components != 3) return fail(info, MDJPEG_EUNSUPPORTED, "neither one nor three components");
            if (n != size_t(6 + 3 * info->components)) return fail(info, MDJPEG_EUNSUPPORTED, "frame header of the wrong length");
            for (int c = 0; c < info->components; ++c) {
                P.comp_id[c] = s[6 + 3 * c];
                info->h_samp[c] = s[7 + 3 * c] >> 4;
                info->v_samp[c] = s[7 + 3 * c] & 15;
                P.comp_tq[c] = s[8 + 3 * c];
                if (P.comp_tq[c] > 3 || info->h_samp[c] < 1 || info->h_samp[c] > 4 || info->v_samp[c] < 1 || info->v_samp[c] > 4)
                    return fail(info, MDJPEG_EUNSUPPORTED, "bad component specification");
            }
            have_sof = true;
            break;
        }
        case 0xC2: return fail(info, MDJPEG_EUNSUPPORTED, "progressive JPEG (SOF2)");
        case 0xC3: case 0xC5: case 0xC6: case 0xC7:
            return fail(info, MDJPEG_EUNSUPPORTED, "lossless or hierarchical JPEG");
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: case 0xCC:
            return fail(info, MDJPEG_EUNSUPPORTED, "arithmetic coding");
        case 0xC4: {                                                                 // DHT
            while (n > 0) {
                if (n < 17) return fail(info, MDJPEG_EUNSUPPORTED, "short Huffman table");
                int tc = s[0] >> 4, th = s[0] & 15, total = 0;
                for (int i = 0; i < 16; ++i) total += s[1 + i];
                if (tc > 1 || th > 3 || total > 256 || n < size_t(17 + total)) return fail(info, MDJPEG_EUNSUPPORTED, "bad Huffman table");
                if (!build_huff(tc ? P.ac[th] : P.dc[th], s + 1, s + 17, total))
                    return fail(info, MDJPEG_EUNSUPPORTED, "Huffman table is not a prefix code");
                s += 17 + total;
                n -= 17 + total;
            }
            break;
        }
        case 0xDB: {                                                                 // DQT
            while (n > 0) {
                int pq = s[0] >> 4, tq = s[0] & 15;
                size_t need = 1 + (pq ? 128 : 64);
                if (pq > 1 || tq > 3 || n < need) return fail(info, MDJPEG_EUNSUPPORTED, "bad quantisation table");
                for (int i = 0; i < 64; ++i)
                    P.qt[tq][ZIGZAG[i]] = pq ? uint16_t(be16(s + 1 + 2 * i)) : uint16_t(s[1 + i]);
                P.qt_defined[tq] = true;
                s += need;
                n -= need;
            }
            break;
        }
        case 0xDD:
            if (n != 2) return fail(info, MDJPEG_EUNSUPPORTED, "bad restart interval segment");
            info->restart_interval = int(be16(s));
            break;
        case 0xE0:
            if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) jfif = true;
            break;
        case 0xEE:
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
            break;
        case 0xDA: {                                                                 // SOS
            if (!have_sof) return fail(info, MDJPEG_EUNSUPPORTED, "scan before the frame header");
            int ns = n >= 1 ? s[0] : 0;
            if (ns != info->components) return fail(info, MDJPEG_EUNSUPPORTED, "several scans (scan does not hold every component)");
            if (n != size_t(4 + 2 * ns)) return fail(info, MDJPEG_EUNSUPPORTED, "scan header of the wrong length");
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != P.comp_id[c]) return fail(info, MDJPEG_EUNSUPPORTED, "scan components not in frame order");
                P.comp_td[c] = s[2 + 2 * c] >> 4;
                P.comp_ta[c] = s[2 + 2 * c] & 15;
                if (P.comp_td[c] > 3 || P.comp_ta[c] > 3 || !P.dc[P.comp_td[c]].defined || !P.ac[P.comp_ta[c]].defined)
                    return fail(info, MDJPEG_EUNSUPPORTED, "scan names a Huffman table that was not defined");
                if (!P.qt_defined[P.comp_tq[c]]) return fail(info, MDJPEG_EUNSUPPORTED, "component names a quantisation table that was not defined");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return fail(info, MDJPEG_EUNSUPPORTED, "scan is not a full sequential scan");
            if (ns == 3) {
                if (adobe && adobe_transform != 1) return fail(info, MDJPEG_EUNSUPPORTED, "Adobe marker with transform 0 (not YCbCr)");
                if (!adobe && !jfif && P.comp_id[0] == 'R' && P.comp_id[1] == 'G' && P.comp_id[2] == 'B')
                    return fail(info, MDJPEG_EUNSUPPORTED, "components named R, G, B (not YCbCr)");
                bool ok = info->h_samp[1] == 1 && info->v_samp[1] == 1 && info->h_samp[2] == 1 && info->v_samp[2] == 1 &&
                          ((info->h_samp[0] == 1 && info->v_samp[0] == 1) || (info->h_samp[0] == 2 && info->v_samp[0] == 1) ||
                           (info->h_samp[0] == 2 && info->v_samp[0] == 2));
                if (!ok) return fail(info, MDJPEG_EUNSUPPORTED, "chroma sampling other than 4:4:4, 4:2:2 and 4:2:0");
            } else {
                info->h_samp[0] = info->v_samp[0] = 1;             // a one-component scan is never interleaved
            }
            int mh = info->h_samp[0], mv = info->v_samp[0];
            info->mcus_x = (info->width + 8 * mh - 1) / (8 * mh);
            info->mcus_y = (info->height + 8 * mv - 1) / (8 * mv);
            int64_t off = 0;
            for (int c = 0; c < ns; ++c) {
                info->blocks_w[c] = info->mcus_x * info->h_samp[c];
                info->blocks_h[c] = info->mcus_y * info->v_samp[c];
                info->plane_offset[c] = off;
                off += int64_t(info->blocks_w[c]) * info->blocks_h[c] * 64;
                memcpy(info->quant[c], P.qt[P.comp_tq[c]], sizeof(info->quant[c]));
            }
            info->coef_count = off;
            P.scan_begin = p + len;
            info->supported = 1;
            return MDJPEG_OK;
        }
        default:
            break;                                                                   // APPn, COM, ...: skipped
        }
        p += len;
    }
}

// ---- bit reader over entropy-coded data ---------------------------------------------------------------------------
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;        // next bit = bit 63
    int      n = 0;          // valid bits in acc
    bool     stopped = false;   // a marker or the end of the data is next: nothing more to read

    inline void fill() {
        if (n > 56 || stopped) return;
        if (end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            w = __builtin_bswap64(w);
            uint64_t t = ~w;                                  // a 0xFF byte is a zero byte of t
            if (!((t - 0x0101010101010101ull) & ~t & 0x8080808080808080ull)) {
                int k = (64 - n) >> 3;
                acc |= (w >> (64 - 8 * k)) << (64 - n - 8 * k);
                p += k;
                n += 8 * k;
                return;
            }
        }
        while (n <= 56) {
            if (p >= end) { stopped = true; return; }
            unsigned b = *p;
            if (b == 0xFF) {
                if (p + 1 >= end) { stopped = true; return; }
                if (p[1] != 0) { stopped = true; return; }     // a marker: stay in front of it
                p += 2;
            } else {
                ++p;
            }
            acc |= uint64_t(b) << (56 - n);
            n += 8;
        }
    }
    inline unsigned peek(int k) const { return unsigned(acc >> (64 - k)); }
    inline void skip(int k) { acc <<= k; n -= k; }
};

struct Corrupt { const char* why; };

// one Huffman symbol; returns -1 when the code is undefined or the data end inside it
inline int decode_symbol(Bits& b, const Huff& h) {
    unsigned e = h.look[b.peek(LOOK)];
    if (e) {
        int len = int(e >> 8);
        if (len > b.n) return -1;
        b.skip(len);
        return int(e & 255);
    }
    unsigned v = b.peek(16);
    for (int len = LOOK + 1; len <= 16; ++len) {
        int code = int(v >> (16 - len));
        if (code <= h.maxcode[len]) {
            if (len > b.n) return -1;
            b.skip(len);
            return h.vals[(code + h.valoff[len]) & 255];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {
    int v = int(b.peek(s));
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

const char* decode_block(Bits& b, const Huff& dc, const Huff& ac, const uint16_t* q, int64_t emax, int& pred, int16_t* blk) {
    memset(blk, 0, 64 * sizeof(int16_t));
    if (b.n < 32) b.fill();                          // a code (<= 16 bits) and its magnitude bits (<= 11) fit 32 bits
    int s = decode_symbol(b, dc);
    if (s < 0) return "undefined DC code or data end early";
    if (s > 11) return "DC magnitude category above 11";
    if (s) {
        if (s > b.n) return "data end early";
        pred += receive_extend(b, s);
    }
    if (pred < -32768 || pred > 32767) return "DC value out of range";
    blk[0] = int16_t(pred);
    int64_t v0 = int64_t(pred) * q[0];
    int64_t energy = v0 * v0;
    for (int k = 1; k < 64;) {
        if (b.n < 32) b.fill();
        int rs = decode_symbol(b, ac);
        if (rs < 0) return "undefined AC code or data end early";
        int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return "coefficient index past 63";
            if (s > 10) return "AC magnitude category above 10";
            if (s > b.n) return "data end early";
            int v = receive_extend(b, s);
            int nat = ZIGZAG[k];
            blk[nat] = int16_t(v);
            int64_t dv = int64_t(v) * q[nat];
            energy += dv * dv;
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 63) return "zero run leaves the block";
        } else if (r == 0) {
            break;
        } else {
            return "end-of-band code in a sequential scan";
        }
    }
    if (energy > emax) return "block energy beyond what 8-bit samples can hold";
    return nullptr;
}


// ---- the scan for a decoder that starts anywhere ----------------------------------------------------------------------
// the first FF at or behind p that is not followed by 00 (a marker, or an FF the file ends on); `size` when there is none
size_t next_marker(const uint8_t* d, size_t size, size_t p) {
    while (p < size) {
        const uint8_t* f = (const uint8_t*)memchr(d + p, 0xFF, size - p);
        if (!f) return size;
        p = size_t(f - d);
        if (p + 1 >= size || d[p + 1] != 0) return p;
        p += 2;
    }
    return size;
}

int scan_file(const uint8_t* d, size_t size, mdjpeg_scan_info* sc, Parsed& P, uint32_t* seg_offsets, size_t seg_capacity) {
    mdjpeg_info* info = &sc->info;
    int rc = parse_headers(d, size, info, P);
    mdjpeg_info keep = *info;
    memset(sc, 0, sizeof(*sc));
    *info = keep;
    if (rc != MDJPEG_OK) return rc;
    int used_class[MDJPEG_MAX_TABLES], used_id[MDJPEG_MAX_TABLES];
    for (int c = 0; c < info->components; ++c)
        for (int cls = 0; cls < 2; ++cls) {
            const int id = cls ? P.comp_ta[c] : P.comp_td[c];
            int t = 0;
            while (t < sc->n_tables && !(used_class[t] == cls && used_id[t] == id)) ++t;
            if (t == sc->n_tables) {
                const Huff& h = cls ? P.ac[id] : P.dc[id];
                used_class[t] = cls;
                used_id[t] = id;
                memcpy(sc->huff_counts[t], h.counts, 16);
                memcpy(sc->huff_vals[t], h.vals, 256);
                ++sc->n_tables;
            }
            (cls ? sc->ac_table : sc->dc_table)[c] = t;
        }
    const int64_t total_mcus = int64_t(info->mcus_x) * info->mcus_y;
    const int64_t interval = info->restart_interval;
    const int64_t nseg = interval ? (total_mcus + interval - 1) / interval : 1;
    sc->scan_begin = int64_t(P.scan_begin);
    sc->n_segments = int32_t(nseg > 0x7fffffff ? 0x7fffffff : nseg);
    if (uint64_t(nseg) > uint64_t(seg_capacity)) {
        snprintf(info->reason, sizeof(info->reason), "%lld restart segments, capacity is %llu", (long long)nseg, (unsigned long long)seg_capacity);
        return MDJPEG_ECAPACITY;
    }
    size_t p = P.scan_begin;
    for (int64_t k = 0; k < nseg; ++k) {
        if (p - P.scan_begin > 0xffffffffull) {                       // (an offset that 32 bits do not hold: left to the caller's decoder)
            snprintf(info->reason, sizeof(info->reason), "scan of 4 GB or more");
            return MDJPEG_ECAPACITY;
        }
        seg_offsets[k] = uint32_t(p - P.scan_begin);
        const size_t m = next_marker(d, size, p);
        const int want = k + 1 < nseg ? 0xD0 + int(k & 7) : 0xD9;
        if (m + 2 > size || d[m + 1] != want) {
            snprintf(info->reason, sizeof(info->reason), "%s", k + 1 < nseg ? "restart marker missing or out of sequence" : "scan is not followed by EOI");
            return MDJPEG_ECORRUPT;
        }
        if (k + 1 == nseg) sc->scan_end = int64_t(m);
        p = m + 2;
    }
    return MDJPEG_OK;
}

}  // namespace

extern "C" {

int mdjpeg_parse(const uint8_t* data, size_t size, mdjpeg_info* info) {
    if (!data || !info) return MDJPEG_EINVAL;
    Parsed P;
    return parse_headers(data, size, info, P);
}

int mdjpeg_decode(const uint8_t* data, size_t size, mdjpeg_info* info, int16_t* coef, size_t capacity) {
    if (!data || !info || !coef) return MDJPEG_EINVAL;
    Parsed P;
    int rc = parse_headers(data, size, info, P);
    if (rc != MDJPEG_OK) return rc;
    if (uint64_t(info->coef_count) > uint64_t(capacity)) {
        snprintf(info->reason, sizeof(info->reason), "coefficient planes need %lld values, capacity is %llu",
                 (long long)info->coef_count, (unsigned long long)capacity);
        return MDJPEG_ECAPACITY;
    }
    const int nc = info->components;
    // Parseval: the coefficients of 64 samples in [-128, 127] have a 2-norm of at most 8 * 128; quantisation moves every
    // coefficient by at most half its step.  A block beyond that was not made from 8-bit samples.  The cap of 2800 keeps
    // the 16-bit workspace of a SIMD inverse DCT from saturating (4 * sqrt(8) * 2800 < 32768), so that such a decoder and a
    // 32-bit one agree BEFORE the range limit.  The bound does not keep samples inside [-512, 511], where libjpeg's
    // range-limit table and saturation part: a block's whole norm can sit in one sample.  The reconstruction saturates,
    // as libjpeg-turbo's SIMD code and so Pillow do ("Foreign files and the range limit").
    int64_t emax[3];
    for (int c = 0; c < nc; ++c) {
        double qn = 0;
        for (int i = 0; i < 64; ++i) qn += double(info->quant[c][i]) * info->quant[c][i];
        double lim = 1024.0 + 0.5 * __builtin_sqrt(qn) + 1.0;
        if (lim > 2800.0) lim = 2800.0;
        emax[c] = int64_t(lim * lim);
    }
    Bits b;
    b.p = data + P.scan_begin;
    b.end = data + size;
    int pred[3] = {0, 0, 0};
    const int interval = info->restart_interval;
    int to_go = interval, next_rst = 0;
    const int64_t total_mcus = int64_t(info->mcus_x) * info->mcus_y;
    int64_t done = 0;
    const char* why = nullptr;
    for (int my = 0; my < info->mcus_y && !why; ++my) {
        for (int mx = 0; mx < info->mcus_x && !why; ++mx) {
            for (int c = 0; c < nc && !why; ++c) {
                const Huff& hd = P.dc[P.comp_td[c]];
                const Huff& ha = P.ac[P.comp_ta[c]];
                const int hs = info->h_samp[c], vs = info->v_samp[c];
                for (int v = 0; v < vs && !why; ++v)
                    for (int h = 0; h < hs && !why; ++h) {
                        int64_t blk = int64_t(my * vs + v) * info->blocks_w[c] + (mx * hs + h);
                        why = decode_block(b, hd, ha, info->quant[c], emax[c], pred[c], coef + info->plane_offset[c] + blk * 64);
                    }
            }
            if (why) break;
            ++done;
            if (interval && --to_go == 0 && done < total_mcus) {
                // end of a restart interval: only padding bits may be left in front of RSTn
                b.fill();
                if (b.n >= 8 || !b.stopped) { why = "bytes left over in front of a restart marker"; break; }
                if (b.end - b.p < 2 || b.p[0] != 0xFF || b.p[1] != 0xD0 + next_rst) { why = "restart marker missing or out of sequence"; break; }
                b.p += 2;
                b.acc = 0; b.n = 0; b.stopped = false;
                next_rst = (next_rst + 1) & 7;
                to_go = interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
        }
    }
    if (!why) {
        b.fill();
        if (b.n >= 8 || !b.stopped) why = "bytes left over behind the last MCU";
        else if (b.end - b.p < 2 || b.p[0] != 0xFF || b.p[1] != 0xD9) why = "scan is not followed by EOI";
    }
    if (why) {
        snprintf(info->reason, sizeof(info->reason), "%s", why);
        return MDJPEG_ECORRUPT;
    }
    return MDJPEG_OK;
}

int mdjpeg_scan(const uint8_t* data, size_t size, mdjpeg_scan_info* scan, uint32_t* seg_offsets, size_t seg_capacity) {
    if (!data || !scan || (!seg_offsets && seg_capacity)) return MDJPEG_EINVAL;
    Parsed P;
    return scan_file(data, size, scan, P, seg_offsets, seg_capacity);
}

int mdjpeg_decode_subsequences(const uint8_t* data, size_t size, int subseq_bits, mdjpeg_info* info, int16_t* coef, size_t capacity) {
    if (!data || !info || !coef || subseq_bits < MDJ_MIN_SUBSEQ_BITS || subseq_bits % 8) return MDJPEG_EINVAL;
    Parsed P;
    mdjpeg_scan_info sc;
    int rc = parse_headers(data, size, info, P);
    if (rc != MDJPEG_OK) return rc;
    if (uint64_t(info->coef_count) > uint64_t(capacity)) {
        snprintf(info->reason, sizeof(info->reason), "coefficient planes need %lld values, capacity is %llu",
                 (long long)info->coef_count, (unsigned long long)capacity);
        return MDJPEG_ECAPACITY;
    }
    const int64_t total_mcus = int64_t(info->mcus_x) * info->mcus_y;
    const int64_t nseg = info->restart_interval ? (total_mcus + info->restart_interval - 1) / info->restart_interval : 1;
    std::vector<uint32_t> seg(size_t(nseg) + 1);
    rc = scan_file(data, size, &sc, P, seg.data(), size_t(nseg));
    *info = sc.info;
    if (rc != MDJPEG_OK) return rc;
    if (sc.scan_end - sc.scan_begin >= MDJ_MAX_SCAN_BYTES) {
        snprintf(info->reason, sizeof(info->reason), "scan too long for 32-bit bit positions");
        return MDJPEG_ECAPACITY;
    }
    seg[size_t(nseg)] = uint32_t(sc.scan_end - sc.scan_begin + 2);
    std::vector<MdjImage> imv(1);
    MdjImage& im = imv[0];
    if (!mdj_fill_image(sc, subseq_bits, im)) return fail(info, MDJPEG_EUNSUPPORTED, "Huffman table is not a prefix code");
    const uint8_t* base = data + sc.scan_begin;
    // a lane's block count is 16 bits: subsequences longer than MDJ_MAX_SUBSEQ_BITS are taken only where they give every
    // segment ONE lane, whose count nothing reads
    if (subseq_bits > MDJ_MAX_SUBSEQ_BITS)
        for (int64_t k = 0; k < nseg; ++k)
            if (uint64_t(seg[size_t(k) + 1] - 2 - seg[size_t(k)]) * 8 > uint64_t(subseq_bits)) return MDJPEG_EINVAL;
    // lanes: every segment is cut into subsequences
    struct Lane { int64_t seg; uint32_t sub; };
    std::vector<Lane> lanes;
    std::vector<size_t> first_lane(size_t(nseg) + 1);
    for (int64_t k = 0; k < nseg; ++k) {
        first_lane[size_t(k)] = lanes.size();
        const uint32_t nb = seg[size_t(k) + 1] - 2 - seg[size_t(k)];
        const uint32_t n = mdj_lanes_of(nb, uint32_t(subseq_bits));
        for (uint32_t i = 0; i < n; ++i) lanes.push_back(Lane{k, i});
    }
    first_lane[size_t(nseg)] = lanes.size();
    const size_t L = lanes.size();
    std::vector<uint64_t> end(L), start(L);
    auto seg_ptr = [&](int64_t k) { return base + seg[size_t(k)]; };
    auto seg_len = [&](int64_t k) { return uint32_t(seg[size_t(k) + 1] - 2 - seg[size_t(k)]); };
    // pass 1: every lane from its own first bit
    for (size_t l = 0; l < L; ++l) {
        const Lane& ln = lanes[l];
        const MdjState s0 = mdj_blind_start(seg_ptr(ln.seg), seg_len(ln.seg), ln.sub, uint32_t(subseq_bits));
        start[l] = mdj_start_key(mdj_pack(s0));
        end[l] = mdj_pack(mdj_decode_lane(im, im.tables, seg_ptr(ln.seg), seg_len(ln.seg), s0, mdj_lane_limit(ln.sub, uint32_t(subseq_bits)), nullptr));
    }
    // pass 2: carry every lane's end into its right neighbour until nothing changes
    for (bool changed = true; changed;) {
        changed = false;
        std::vector<uint64_t> prev = end;                    // the lanes of a round all see the round before (as the worst GPU schedule would)
        for (size_t l = 0; l < L; ++l) {
            const Lane& ln = lanes[l];
            if (ln.sub == 0) continue;
            const uint64_t key = mdj_start_key(prev[l - 1]);
            if (key == start[l]) continue;
            start[l] = key;
            end[l] = mdj_pack(mdj_decode_lane(im, im.tables, seg_ptr(ln.seg), seg_len(ln.seg), mdj_unpack(key),
                                              mdj_lane_limit(ln.sub, uint32_t(subseq_bits)), nullptr));
            changed = true;
        }
    }
    // pass 3 + 4: output positions, then the final decode
    memset(coef, 0, size_t(info->coef_count) * sizeof(int16_t));
    std::vector<uint32_t> energy(size_t(info->coef_count / 64), 0);
    uint32_t err = 0;
    for (int64_t k = 0; k < nseg; ++k) {
        int64_t block = 0;
        const int64_t first_mcu = k * im.interval;
        const int64_t mcus = total_mcus - first_mcu < im.interval ? total_mcus - first_mcu : im.interval;
        for (size_t l = first_lane[size_t(k)]; l < first_lane[size_t(k) + 1]; ++l) {
            MdjSink sink{coef, energy.data(), first_mcu, block, mcus * im.blocks_per_mcu, 0};
            const MdjState s = mdj_unpack(start[l]);
            mdj_decode_lane(im, im.tables, seg_ptr(k), seg_len(k), s, mdj_lane_limit(lanes[l].sub, uint32_t(subseq_bits)), &sink);
            err |= sink.err;
            if (l + 1 == first_lane[size_t(k) + 1] && sink.block < sink.blocks) err |= MDJ_ERR_COUNT;
            block += mdj_unpack(end[l]).n;
        }
        if (first_lane[size_t(k)] == first_lane[size_t(k) + 1]) err |= MDJ_ERR_COUNT;
    }
    // pass 5: the DC differences become values, per component, anew in every segment
    if (!err)
        for (int c = 0; c < im.components; ++c) {
            const int64_t per_mcu = int64_t(im.h_samp[c]) * im.v_samp[c];
            const int64_t nblocks = total_mcus * per_mcu;
            int64_t dc = 0;
            for (int64_t j = 0; j < nblocks; ++j) {
                if (j % (im.interval * per_mcu) == 0) dc = 0;
                const int64_t off = mdj_dc_block_offset(im, c, j);
                dc += coef[off * 64];
                err |= mdj_check_block(im, c, dc, energy[size_t(off)]);
                coef[off * 64] = int16_t(dc);
            }
        }
    if (err) {
        snprintf(info->reason, sizeof(info->reason), "the final lanes flagged 0x%x", err);
        return MDJPEG_ECORRUPT;
    }
    return MDJPEG_OK;
}

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

// the rectangles of mdjpeg_blur_regions / mdjpeg_blur_regions_chunked, one after the other; lds_bytes 0: every row in one piece
static int blur_regions(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects, float radius,
                        int lds_bytes) {
    if (!rgb || width < 1 || height < 1 || pitch < int64_t(width) * 3 || n_rects < 0 || (n_rects && !rects)) return MDJPEG_EINVAL;
    if (!(radius >= 0.0f) || radius > MD_BLUR_MAX_RADIUS) return MDJPEG_EINVAL;
    for (int i = 0; i < n_rects; ++i) {
        const int32_t* q = rects + 4 * i;
        if (q[2] <= q[0] || q[3] <= q[1]) continue;
        if (q[0] < 0 || q[1] < 0 || q[2] > width || q[3] > height) return MDJPEG_EINVAL;
    }
    const MdBlurWeights wt = md_blur_weights(radius);
    std::vector<uint8_t> s0, s1, la, lb;
    for (int i = 0; i < n_rects; ++i) {
        const int32_t* q = rects + 4 * i;
        const int w = q[2] - q[0], h = q[3] - q[1];
        if (w <= 0 || h <= 0) continue;                                  // without area: nothing is pasted
        uint8_t* img = rgb + int64_t(q[1]) * pitch + int64_t(q[0]) * 3;
        const int64_t sp = int64_t(w) * 3;
        s0.assign(size_t(sp) * h, 0);
        s1.assign(size_t(sp) * h, 0);
        MdBlurXPlan plan;
        if (lds_bytes > 0) {
            if (!md_blur_plan_x(w, wt.r, lds_bytes, &plan)) return MDJPEG_EINVAL;
        } else {
            plan.rows = 1, plan.stride = md_blur_row_stride(w), plan.chunks = 1, plan.step = w, plan.halo = 0;
        }
        la.assign(size_t(plan.stride), 0);
        lb.assign(size_t(plan.stride), 0);
        // the row stage, as a workgroup runs it: load a chunk with its halo, three passes per channel, keep the middle
        for (int y = 0; y < h; ++y)
            for (int k = 0; k < plan.chunks; ++k) {
                int o0, o1, a, b;
                md_blur_chunk(plan, w, k, &o0, &o1, &a, &b);
                const int n = b - a;
                if (size_t(n) * 3 > la.size()) return MDJPEG_EINVAL;
                memcpy(la.data(), img + int64_t(y) * pitch + int64_t(a) * 3, size_t(n) * 3);
                for (int c = 0; c < 3; ++c) md_blur_line3(la.data() + c, lb.data() + c, 3, n, wt);
                memcpy(s0.data() + int64_t(y) * sp + int64_t(o0) * 3, lb.data() + size_t(o0 - a) * 3, size_t(o1 - o0) * 3);
            }
        // the column stage, as a lane runs it: one byte column through the three passes, the last one into the image
        for (int64_t t = 0; t < sp; ++t) {
            md_blur_line(s0.data() + t, sp, s1.data() + t, sp, h, wt.r, wt.ww, wt.fw);
            md_blur_line(s1.data() + t, sp, s0.data() + t, sp, h, wt.r, wt.ww, wt.fw);
            md_blur_line(s0.data() + t, sp, img + t, pitch, h, wt.r, wt.ww, wt.fw);
        }
    }
    return MDJPEG_OK;
}

int mdjpeg_blur_regions(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects, float radius) {
    return blur_regions(rgb, width, height, pitch, rects, n_rects, radius, 0);
}

int mdjpeg_blur_regions_chunked(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* rects, int n_rects,
                                float radius, int lds_bytes) {
    if (lds_bytes < 1) return MDJPEG_EINVAL;
    return blur_regions(rgb, width, height, pitch, rects, n_rects, radius, lds_bytes);
}

int mdjpeg_blur_weights(float radius, int32_t* r, uint32_t* ww, uint32_t* fw) {
    if (!(radius >= 0.0f) || radius > MD_BLUR_MAX_RADIUS || !r || !ww || !fw) return MDJPEG_EINVAL;
    const MdBlurWeights wt = md_blur_weights(radius);
    *r = wt.r, *ww = wt.ww, *fw = wt.fw;
    return MDJPEG_OK;
}

// The host model of mdhip_resample_lanczos for one image: the passes as the workgroups run them -- the horizontal one strip
// by strip out of a copy of the strip's source run (placed as the on-chip copy is), the vertical one byte column by byte column.
int mdjpeg_resample(const uint8_t* src, int32_t width, int32_t height, int64_t pitch, uint8_t* dst, int32_t dst_width, int32_t dst_height,
                    int64_t dst_pitch) {
    if (!src || !dst || width < 1 || height < 1 || dst_width < 1 || dst_height < 1 || width > 65535 || height > 65535 ||
        dst_width > 65535 || dst_height > 65535 || pitch < int64_t(width) * 3 || dst_pitch < int64_t(dst_width) * 3)
        return MDJPEG_EINVAL;
    const bool horizontal = dst_width != width, vertical = dst_height != height;
    if (!horizontal && !vertical) {
        for (int y = 0; y < height; ++y) memcpy(dst + int64_t(y) * dst_pitch, src + int64_t(y) * pitch, size_t(width) * 3);
        return MDJPEG_OK;
    }
    std::vector<int32_t> bounds, kk;
    std::vector<double> work;
    std::vector<uint8_t> between;
    const uint8_t* in = src;
    int64_t in_pitch = pitch;
    if (horizontal) {
        const int ksize = md_resample_ksize(width, dst_width);
        bounds.assign(size_t(dst_width) * 2, 0);
        kk.assign(size_t(dst_width) * ksize, 0);
        work.assign(size_t(ksize), 0.0);
        md_resample_coeffs(width, dst_width, ksize, bounds.data(), kk.data(), work.data());
        MdResampleStrips plan;
        if (!md_resample_plan_strips(bounds.data(), dst_width, MD_RESAMPLE_LDS_BYTES, &plan)) return MDJPEG_EUNSUPPORTED;
        uint8_t* out = dst;
        int64_t out_pitch = dst_pitch;
        if (vertical) {
            between.assign(size_t(dst_width) * 3 * height, 0);
            out = between.data(), out_pitch = int64_t(dst_width) * 3;
        }
        std::vector<uint8_t> run(size_t(plan.run_bytes), 0);
        for (int y = 0; y < height; ++y)
            for (int o0 = 0; o0 < dst_width; o0 += plan.strip) {
                const int o1 = o0 + plan.strip < dst_width ? o0 + plan.strip : dst_width;
                const int first = bounds[2 * o0];
                const int nb = (bounds[2 * (o1 - 1)] + bounds[2 * (o1 - 1) + 1] - first) * 3;
                const uint8_t* line = src + int64_t(y) * pitch + int64_t(first) * 3;
                const int sh = int(uintptr_t(line) & 3);
                if (sh + nb > plan.run_bytes) return MDJPEG_EINVAL;
                memcpy(run.data() + sh, line, size_t(nb));
                for (int o = o0; o < o1; ++o)
                    for (int c = 0; c < 3; ++c)
                        out[int64_t(y) * out_pitch + int64_t(o) * 3 + c] =
                            md_resample_dot(run.data() + sh + (bounds[2 * o] - first) * 3 + c, 3, kk.data() + size_t(o) * ksize, bounds[2 * o + 1]);
            }
        in = out, in_pitch = out_pitch;
    }
    if (vertical) {
        const int ksize = md_resample_ksize(height, dst_height);
        bounds.assign(size_t(dst_height) * 2, 0);
        kk.assign(size_t(dst_height) * ksize, 0);
        work.assign(size_t(ksize), 0.0);
        md_resample_coeffs(height, dst_height, ksize, bounds.data(), kk.data(), work.data());
        for (int y = 0; y < dst_height; ++y)
            for (int x = 0; x < dst_width * 3; ++x)
                dst[int64_t(y) * dst_pitch + x] =
                    md_resample_dot(in + int64_t(bounds[2 * y]) * in_pitch + x, in_pitch, kk.data() + size_t(y) * ksize, bounds[2 * y + 1]);
    }
    return MDJPEG_OK;
}

// the host model of mdhip_draw_ops for one image: every pixel takes the value of the last operation that covers it
int mdjpeg_draw(uint8_t* rgb, int32_t width, int32_t height, int64_t pitch, const int32_t* ops, int n_ops, const uint8_t* patches,
                int64_t patch_bytes) {
    if (!rgb || width < 1 || height < 1 || pitch < int64_t(width) * 3 || n_ops < 0 || (n_ops && !ops) || patch_bytes < 0) return MDJPEG_EINVAL;
    for (int i = 0; i < n_ops; ++i) {
        const int32_t* op = ops + size_t(i) * MD_DRAW_OP_WORDS;
        if (md_draw_op_bad(op, patch_bytes)) return MDJPEG_EINVAL;
        if (op[0] == MD_DRAW_PATCH && op[3] > 0 && op[4] > 0 && !patches) return MDJPEG_EINVAL;
    }
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            uint8_t v[3];
            if (!md_draw_pixel(ops, n_ops, patches, x, y, v)) continue;
            uint8_t* p = rgb + int64_t(y) * pitch + int64_t(x) * 3;
            p[0] = v[0], p[1] = v[1], p[2] = v[2];
        }
    return MDJPEG_OK;
}

// The host model of mdhip_classifier_input for one crop: tile by tile as the workgroups run it -- the horizontal pass of the
// canvas rows a tile's vertical taps cover into an 8-bit tile of exactly that size, then the vertical pass and the lookup.
int mdjpeg_classifier_input(const uint8_t* src, int64_t pitch, int32_t src_w, int32_t src_h, int32_t canvas_w, int32_t canvas_h,
                            int32_t off_x, int32_t off_y, int32_t size, int32_t filter, const float mean[3], const float std[3], float* out) {
    if (!src || !mean || !std || !out || src_w < 1 || src_h < 1 || canvas_w < 1 || canvas_h < 1 || canvas_w > 65535 || canvas_h > 65535 ||
        pitch < int64_t(src_w) * 3 || off_x < 0 || off_y < 0 || off_x > canvas_w - src_w || off_y > canvas_h - src_h || size < 1 ||
        size > MD_CLASSIFY_MAX_SIZE || filter < MD_FILTER_BICUBIC || filter > MD_FILTER_LANCZOS)
        return MDJPEG_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f) return MDJPEG_EINVAL;
    std::vector<int32_t> table;
    std::vector<double> work;
    MdClassifyCrop d;
    memset(&d, 0, sizeof(d));
    if (!md_classify_build(filter, canvas_w, canvas_h, size, MD_CLASSIFY_LDS_BYTES, table, work, &d)) return MDJPEG_EUNSUPPORTED;
    d.src = src, d.pitch = pitch, d.src_w = src_w, d.src_h = src_h, d.off_x = off_x, d.off_y = off_y;
    std::vector<float> lut(3 * 256);
    md_classify_lut(mean, std, lut.data());
    std::vector<uint8_t> tile;
    for (int g = 0; g < d.row_tiles; ++g)
        for (int k = 0; k < d.strips; ++k)
            if (!md_classify_run_tile(d, table.data(), k, g, MD_CLASSIFY_LDS_BYTES, tile, [&](int x, int y, int c, uint8_t v) {
                    out[(size_t(c) * size + y) * size + x] = lut[size_t(c) * 256 + v];
                }))
                return MDJPEG_EINVAL;
    return MDJPEG_OK;
}

// The host model of mdhip_thumbnails: every tile is checked and planned before any is made, then made workgroup by workgroup
// with the statements the lanes run; the bytes go interleaved to their place in the sheet.
int mdjpeg_thumbnails(const mdjpeg_thumbnail* tiles, int n, int32_t filter) {
    if (n == 0) return MDJPEG_OK;
    if (!tiles || n < 0 || n > 65535 || filter < MD_FILTER_BICUBIC || filter > MD_FILTER_LANCZOS) return MDJPEG_EINVAL;
    std::vector<MdClassifyCrop> recs((size_t)n);
    std::vector<std::vector<int32_t>> tables((size_t)n);
    std::vector<double> work;
    for (int i = 0; i < n; ++i) {
        const mdjpeg_thumbnail& q = tiles[i];
        const bool empty = (q.src_w == 0 && q.src_h >= 0) || (q.src_h == 0 && q.src_w >= 0);      // no image pixel in the canvas: src is not read
        if (!q.dst || q.canvas_w < 1 || q.canvas_h < 1 || q.canvas_w > 65535 || q.canvas_h > 65535 ||
            (!empty && (!q.src || q.src_w < 1 || q.src_h < 1 || q.pitch < int64_t(q.src_w) * 3 || q.off_x < 0 || q.off_y < 0 ||
                        q.off_x > q.canvas_w - q.src_w || q.off_y > q.canvas_h - q.src_h)) ||
            q.out_w < 1 || q.out_h < 1 || q.out_w > 65535 || q.out_h > 65535 || q.dst_pitch < int64_t(q.out_w) * 3)
            return MDJPEG_EINVAL;
        MdClassifyCrop& d = recs[size_t(i)];
        memset(&d, 0, sizeof(d));
        if (!md_thumbnail_build(filter, q.canvas_w, q.canvas_h, q.out_w, q.out_h, MD_CLASSIFY_LDS_BYTES, tables[size_t(i)], work, &d))
            return MDJPEG_EUNSUPPORTED;
        if (!empty) d.src = q.src, d.pitch = q.pitch, d.src_w = q.src_w, d.src_h = q.src_h, d.off_x = q.off_x, d.off_y = q.off_y;
        d.dst = q.dst, d.dst_pitch = q.dst_pitch;
    }
    std::vector<uint8_t> tile;
    for (int i = 0; i < n; ++i) {
        const MdClassifyCrop& d = recs[size_t(i)];
        for (int g = 0; g < d.row_tiles; ++g)
            for (int k = 0; k < d.strips; ++k)
                if (!md_classify_run_tile(d, tables[size_t(i)].data(), k, g, MD_CLASSIFY_LDS_BYTES, tile, [&](int x, int y, int c, uint8_t v) {
                        d.dst[int64_t(y) * d.dst_pitch + int64_t(x) * 3 + c] = v;
                    }))
                    return MDJPEG_EINVAL;
    }
    return MDJPEG_OK;
}

// the tile a workgroup takes of a crop of this canvas: plan[0] output columns, plan[1] output rows; MDJPEG_EUNSUPPORTED when
// none fits lds_bytes (0: what the device has)
int mdjpeg_classifier_plan(int32_t canvas_w, int32_t canvas_h, int32_t size, int32_t filter, int32_t lds_bytes, int32_t plan[2]) {
    if (!plan || canvas_w < 1 || canvas_h < 1 || canvas_w > 65535 || canvas_h > 65535 || size < 1 || size > MD_CLASSIFY_MAX_SIZE ||
        filter < MD_FILTER_BICUBIC || filter > MD_FILTER_LANCZOS || lds_bytes < 0)
        return MDJPEG_EINVAL;
    std::vector<int32_t> table;
    std::vector<double> work;
    MdClassifyCrop d;
    memset(&d, 0, sizeof(d));
    if (!md_classify_build(filter, canvas_w, canvas_h, size, lds_bytes ? lds_bytes : MD_CLASSIFY_LDS_BYTES, table, work, &d)) return MDJPEG_EUNSUPPORTED;
    plan[0] = d.strip, plan[1] = d.rows;
    return MDJPEG_OK;
}

const char* mdjpeg_version(void) { return "mdjpeg 7"; }

}  // extern "C"

#ifdef MDJPEG_ASAN_MAIN
// `make asan-jpeg`: decodes every file named on the command line into a heap buffer of exactly coef_count values, so that
// the sanitizers see any access outside it.  Prints one line per file; the exit status is 0 unless a sanitizer fires.
#include <vector>
// `--blur`: mdjpeg_blur_regions and its chunked form on heap images of exactly pitch x height bytes -- the whole image, single
// rows and columns, rectangles on every border and the sizes around the box radius -- so that the sanitizers see any
// access outside an image; the two forms must agree.
static int blur_matrix() {
    const int W = 97, H = 131;
    const int64_t pitch = 393;
    std::vector<int32_t> rects = {0, 0, W, H, 50, 60, 51, 61, 0, 70, W, 71, 33, 0, 34, H, 0, 0, 30, 20, W - 30, 0, W, 25, 0, H - 20, 41, H,
                                  W - 17, H - 33, W, H, 5, 5, 5, 9, 9, 5, 5, 9};
    for (int n : {5, 39, 40, 41, 79, 80, 81}) {
        rects.insert(rects.end(), {1, 3, 1 + n, 50});
        rects.insert(rects.end(), {3, 1, 26, 1 + n});
        rects.insert(rects.end(), {2, 4, 2 + n, 4 + n});
    }
    const int n_rects = int(rects.size() / 4);
    for (float radius : {40.0f, 2.0f, 7.5f, 100.0f, 0.0f, 512.0f})
        for (int k = 0; k < n_rects; ++k) {
            const size_t bytes = size_t(pitch) * (H - 1) + size_t(W) * 3;           // the last row ends with its last pixel
            uint8_t* a = new uint8_t[bytes];
            uint8_t* b = new uint8_t[bytes];
            uint32_t seed = 12345u + uint32_t(k);
            for (size_t i = 0; i < bytes; ++i) a[i] = b[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const int ra = mdjpeg_blur_regions(a, W, H, pitch, rects.data() + 4 * k, 1, radius);
            int32_t r;
            uint32_t ww, fw;
            mdjpeg_blur_weights(radius, &r, &ww, &fw);
            const int rb = mdjpeg_blur_regions_chunked(b, W, H, pitch, rects.data() + 4 * k, 1, radius, 2 * (18 * (r + 1) + 20));
            const bool same = memcmp(a, b, bytes) == 0;
            delete[] a;
            delete[] b;
            if (ra != MDJPEG_OK || rb != MDJPEG_OK || !same) { printf("blur: rectangle %d at radius %g: %d %d %d\n", k, double(radius), ra, rb, int(same)); return 5; }
        }
    // all rectangles one after the other in one image, and rectangles that leave it
    std::vector<uint8_t> img(size_t(pitch) * H, 77);
    if (mdjpeg_blur_regions(img.data(), W, H, pitch, rects.data(), n_rects, 40.0f) != MDJPEG_OK) return 5;
    const int32_t outside[8] = {0, 0, 5, 5, 90, 100, 98, 131};
    if (mdjpeg_blur_regions(img.data(), W, H, pitch, outside, 2, 40.0f) != MDJPEG_EINVAL) return 5;
    printf("blur: %d rectangles x 6 radii\n", n_rects);
    return 0;
}

// `--preview`: mdjpeg_resample and mdjpeg_draw on heap images of exactly pitch x (height - 1) + 3 x width bytes -- reducing,
// enlarging, one axis unchanged, a single pixel, a pitch above 3 x width, runs longer than a strip -- and operations that
// leave the image on every side, so that the sanitizers see any access outside an image.
static int preview_matrix() {
    const int shapes[][6] = {{97, 61, 40, 25, 0, 0}, {333, 500, 166, 249, 0, 0}, {50, 40, 120, 96, 0, 0}, {1000, 37, 70, 2, 0, 0}, {1, 1, 5, 5, 0, 0},
                             {640, 480, 640, 479, 0, 0}, {17, 9, 8, 4, 64, 29}, {1300, 40, 100, 3, 3907, 301}, {17, 9, 17, 9, 64, 64}, {3, 2000, 2, 1, 0, 0}};
    for (const auto& q : shapes) {
        const int w = q[0], h = q[1], dw = q[2], dh = q[3];
        const int64_t pitch = q[4] ? q[4] : int64_t(w) * 3, dpitch = q[5] ? q[5] : int64_t(dw) * 3;
        const size_t bytes = size_t(pitch) * (h - 1) + size_t(w) * 3, dbytes = size_t(dpitch) * (dh - 1) + size_t(dw) * 3;
        for (int shift = 0; shift < 4; ++shift) {                        // every alignment of the first byte
            uint8_t* a = new uint8_t[bytes + shift];
            uint8_t* b = new uint8_t[dbytes];
            uint32_t seed = 777u + uint32_t(w);
            for (size_t i = 0; i < bytes + shift; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const int rc = mdjpeg_resample(a + shift, w, h, pitch, b, dw, dh, dpitch);
            delete[] a;
            delete[] b;
            if (rc != MDJPEG_OK) { printf("preview: %dx%d -> %dx%d: %d\n", w, h, dw, dh, rc); return 6; }
        }
    }
    const int W = 53, H = 31;
    const int64_t pitch = 170;
    const size_t bytes = size_t(pitch) * (H - 1) + size_t(W) * 3;
    const int pw = 20, ph = 9;
    uint8_t* patch = new uint8_t[size_t(pw) * ph * 3 + 5];
    for (size_t i = 0; i < size_t(pw) * ph * 3 + 5; ++i) patch[i] = uint8_t(i);
    const int32_t ops[] = {0, 5, 5, 20, 12, 0x0000ff, 0, 0,   0, -7, -3, 2, 200, 0x00ff00, 0, 0,   0, 40, 25, 1000, 30, 0xff0000, 0, 0,
                           0, 10, 10, 9, 20, 0x123456, 0, 0,   0, -2147483647, -2147483647, 2147483647, 0, 0x654321, 0, 0,
                           1, -5, -4, pw, ph, 5, 0, 0,   1, W - 3, H - 2, pw, ph, 0, 0, 0,   1, 7, 11, pw, ph, 0, 0, 0,
                           1, 2147483000, 2147483000, pw, ph, 0, 0, 0,   1, -2147483647, 3, pw, ph, 0, 0, 0,   1, 30, 3, 0, 0, 0, 0, 0};
    const int n_ops = int(sizeof(ops) / sizeof(ops[0]) / MD_DRAW_OP_WORDS);
    uint8_t* img = new uint8_t[bytes];
    memset(img, 9, bytes);
    int rc = mdjpeg_draw(img, W, H, pitch, ops, n_ops, patch, int64_t(pw) * ph * 3 + 5);
    const int32_t outside[] = {1, 0, 0, pw, ph, 6, 0, 0};
    const int rb = mdjpeg_draw(img, W, H, pitch, outside, 1, patch, int64_t(pw) * ph * 3 + 5);
    const int32_t unknown[] = {2, 0, 0, 1, 1, 0, 0, 0};
    const int ru = mdjpeg_draw(img, W, H, pitch, unknown, 1, patch, 0);
    delete[] img;
    delete[] patch;
    if (rc != MDJPEG_OK || rb != MDJPEG_EINVAL || ru != MDJPEG_EINVAL) { printf("preview: draw %d %d %d\n", rc, rb, ru); return 6; }
    printf("preview: %d shapes x 4 alignments, %d operations\n", int(sizeof(shapes) / sizeof(shapes[0])), n_ops);
    return 0;
}

// `--classify`: mdjpeg_classifier_input on heap images of exactly pitch x (src_h - 1) + 3 x src_w bytes and an output of
// exactly 3 x size x size floats -- reducing, enlarging, a single column, an unchanged size, more than one strip, canvases
// with zeros on every side, the three filters -- so that the sanitizers see any access outside a rectangle or the tensor.
static int classify_matrix() {
    // src_w, src_h, canvas_w, canvas_h, off_x, off_y, size, pitch (0: 3 x src_w)
    const int shapes[][8] = {{97, 61, 97, 61, 0, 0, 32, 0},     {5, 7, 5, 7, 0, 0, 32, 0},         {1, 9, 1, 9, 0, 0, 32, 0},
                             {301, 187, 301, 187, 0, 0, 32, 908}, {333, 500, 333, 500, 0, 0, 80, 0}, {80, 200, 80, 200, 0, 0, 80, 245},
                             {640, 480, 640, 480, 0, 0, 224, 0}, {1300, 40, 1300, 40, 0, 0, 32, 0}, {40, 30, 50, 50, 10, 0, 32, 0},
                             {40, 30, 50, 50, 0, 20, 32, 0},     {40, 30, 50, 50, 0, 0, 32, 121},   {21, 17, 60, 60, 20, 30, 32, 0},
                             {13, 20, 20, 20, 4, 0, 32, 0},      {2, 2, 3000, 3000, 1500, 1500, 8, 0}};
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    int runs = 0;
    for (const auto& q : shapes)
        for (int filter = 0; filter < 3; ++filter) {
            const int64_t pitch = q[7] ? q[7] : int64_t(q[0]) * 3;
            const size_t bytes = size_t(pitch) * (q[1] - 1) + size_t(q[0]) * 3;
            const int shift = runs & 3;                                  // every alignment of the first byte
            uint8_t* a = new uint8_t[bytes + shift];
            float* o = new float[size_t(3) * q[6] * q[6]];
            uint32_t seed = 99u + uint32_t(runs);
            for (size_t i = 0; i < bytes + shift; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const int rc = mdjpeg_classifier_input(a + shift, pitch, q[0], q[1], q[2], q[3], q[4], q[5], q[6], filter, mean, stdv, o);
            delete[] a;
            delete[] o;
            if (rc != MDJPEG_OK) { printf("classify: %dx%d in %dx%d at %d, filter %d: %d\n", q[0], q[1], q[2], q[3], q[6], filter, rc); return 7; }
            ++runs;
        }
    uint8_t px[3] = {1, 2, 3};
    float o1[3];
    const float zero[3] = {0.229f, 0.0f, 0.225f};
    int32_t plan[2];
    const int bad[] = {mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 1, 3, mean, stdv, o1), mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 1, 0, mean, zero, o1),
                       mdjpeg_classifier_input(px, 3, 1, 1, 4, 4, 4, 0, 1, 0, mean, stdv, o1), mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 0, 0, mean, stdv, o1)};
    for (int rc : bad)
        if (rc != MDJPEG_EINVAL) { printf("classify: a bad argument gives %d\n", rc); return 7; }
    if (mdjpeg_classifier_input(px, 3, 1, 1, 1, 1, 0, 0, 1, 0, mean, stdv, o1) != MDJPEG_OK) return 7;
    if (mdjpeg_classifier_plan(65535, 65535, 8, MD_FILTER_LANCZOS, 0, plan) != MDJPEG_EUNSUPPORTED) { printf("classify: plan\n"); return 7; }
    printf("classify: %d runs\n", runs);
    return 0;
}

// `--thumbnails`: mdjpeg_thumbnails on heap images of exactly pitch x (src_h - 1) + 3 x src_w bytes and sheets of exactly
// dst_pitch x (out_h - 1) + 3 x out_w bytes -- reducing, enlarging, one axis unchanged, a copy, a single pixel either way,
// canvases with zeros on every side and wholly of zeros, a tap run longer than a strip, the three filters -- so that the
// sanitizers see any access outside a rectangle or a tile.
static int thumbnails_matrix() {
    // src_w, src_h, canvas_w, canvas_h, off_x, off_y, out_w, out_h, pitch (0: 3 x src_w), dst_pitch (0: 3 x out_w)
    const int shapes[][10] = {{97, 61, 97, 61, 0, 0, 13, 9, 0, 0},    {9, 7, 9, 7, 0, 0, 40, 31, 0, 121},  {40, 30, 40, 30, 0, 0, 40, 11, 0, 0},
                              {40, 30, 40, 30, 0, 0, 17, 30, 127, 0}, {31, 20, 31, 20, 0, 0, 31, 20, 0, 100}, {50, 40, 50, 40, 0, 0, 1, 1, 0, 0},
                              {1, 1, 1, 1, 0, 0, 5, 5, 0, 0},         {40, 30, 50, 30, 10, 0, 20, 12, 0, 0}, {40, 30, 50, 30, 0, 0, 20, 12, 0, 0},
                              {40, 30, 40, 41, 0, 11, 20, 12, 0, 0},  {40, 30, 40, 41, 0, 0, 20, 12, 0, 67}, {1, 1, 30, 30, 29, 29, 7, 7, 0, 0},
                              {1300, 40, 1300, 40, 0, 0, 20, 3, 0, 0}, {0, 0, 12, 9, 0, 0, 5, 4, 3, 0}, {0, 5, 12, 9, 0, 0, 12, 9, 3, 0}, {8, 8, 8, 60000, 0, 29000, 3, 40, 0, 0}};
    int runs = 0;
    for (const auto& q : shapes)
        for (int filter = 0; filter < 3; ++filter) {
            const int64_t pitch = q[8] ? q[8] : int64_t(q[0]) * 3, dpitch = q[9] ? q[9] : int64_t(q[6]) * 3;
            const size_t bytes = q[0] && q[1] ? size_t(pitch) * (q[1] - 1) + size_t(q[0]) * 3 : 0, dbytes =size_t(dpitch) * (q[7] - 1) + size_t(q[6]) * 3;
            const int shift = runs & 3;                                  // every alignment of the first byte
            uint8_t* a = new uint8_t[bytes + shift];
            uint8_t* o = new uint8_t[dbytes];
            uint32_t seed = 4242u + uint32_t(runs);
            for (size_t i = 0; i < bytes + shift; ++i) a[i] = uint8_t((seed = seed * 1664525u + 1013904223u) >> 24);
            const mdjpeg_thumbnail t = {a + shift, pitch, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], o, dpitch};
            const int rc = mdjpeg_thumbnails(&t, 1, filter);
            delete[] a;
            delete[] o;
            if (rc != MDJPEG_OK) { printf("thumbnails: %dx%d in %dx%d to %dx%d, filter %d: %d\n", q[0], q[1], q[2], q[3], q[6], q[7], filter, rc); return 8; }
            ++runs;
        }
    uint8_t px[3] = {1, 2, 3}, o1[3];
    const mdjpeg_thumbnail bad[] = {{px, 3, 1, 1, 4, 4, 4, 0, 1, 1, o1, 3}, {px, 3, 1, 1, 1, 1, 0, 0, 0, 1, o1, 3}, {px, 3, 1, 1, 1, 1, 0, 0, 1, 1, o1, 2},
                                    {nullptr, 3, 1, 1, 1, 1, 0, 0, 1, 1, o1, 3}, {px, 3, 1, 1, 1, 1, 0, 0, 1, 1, nullptr, 3}};
    for (const mdjpeg_thumbnail& t : bad)
        if (mdjpeg_thumbnails(&t, 1, 0) != MDJPEG_EINVAL) { printf("thumbnails: a bad argument is accepted\n"); return 8; }
    const mdjpeg_thumbnail good = {px, 3, 1, 1, 1, 1, 0, 0, 1, 1, o1, 3}, tall = {px, 3, 1, 1, 1, 60000, 0, 0, 1, 1, o1, 3};
    if (mdjpeg_thumbnails(&good, 1, 3) != MDJPEG_EINVAL || mdjpeg_thumbnails(&good, 1, 0) != MDJPEG_OK || o1[0] != 1 || o1[2] != 3) return 8;
    if (mdjpeg_thumbnails(&tall, 1, 0) != MDJPEG_EUNSUPPORTED) { printf("thumbnails: plan\n"); return 8; }
    printf("thumbnails: %d runs\n", runs);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--thumbnails")) return thumbnails_matrix();
    if (argc == 2 && !strcmp(argv[1], "--classify")) return classify_matrix();
    if (argc == 2 && !strcmp(argv[1], "--preview")) return preview_matrix();
    if (argc == 2 && !strcmp(argv[1], "--blur")) return blur_matrix();
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("%s: cannot open\n", argv[i]); continue; }
        std::vector<uint8_t> bytes;
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
        fclose(f);
        uint8_t* exact = new uint8_t[bytes.size() ? bytes.size() : 1];          // exact extent: reads past the file are seen
        memcpy(exact, bytes.data(), bytes.size());
        mdjpeg_info info;
        int rc = mdjpeg_parse(exact, bytes.size(), &info);
        if (rc == MDJPEG_OK) {
            int16_t* coef = new int16_t[size_t(info.coef_count)];
            rc = mdjpeg_decode(exact, bytes.size(), &info, coef, size_t(info.coef_count));
            const int sampling = info.h_samp[0] == 1 && info.v_samp[0] == 1 ? 0 : info.h_samp[0] == 2 && info.v_samp[0] == 1 ? 1
                                 : info.h_samp[0] == 2 && info.v_samp[0] == 2 ? 2 : -1;
            if (rc == MDJPEG_OK && info.components == 3 && sampling >= 0) {
                // and back: the host model of the GPU entropy ENCODER on these coefficients, output buffers of the exact size
                const int16_t* planes = coef;
                for (int chunk : {1, 3, 64}) {
                    int64_t off, size;
                    size_t need = 0;
                    int re = mdjpeg_encode_subsequences_sampled(&planes, &info.width, &info.height, &sampling, 1, chunk, nullptr, 0, &off, &size, &need);
                    if (re == MDJPEG_ECAPACITY) {
                        uint8_t* scan = new uint8_t[need];
                        re = mdjpeg_encode_subsequences_sampled(&planes, &info.width, &info.height, &sampling, 1, chunk, scan, need, &off, &size, &need);
                        delete[] scan;
                    }
                    if (re != MDJPEG_OK && re != MDJPEG_ECORRUPT) { printf("%s: encoding at chunk %d gives %d\n", argv[i], chunk, re); return 4; }
                }
            }
            delete[] coef;
            // the descriptor and the host model of the GPU decoder, at two subsequence lengths, into exact buffers too
            mdjpeg_scan_info sc;
            std::vector<uint32_t> seg(1);
            int rs = mdjpeg_scan(exact, bytes.size(), &sc, seg.data(), seg.size());
            if (rs == MDJPEG_ECAPACITY && sc.n_segments > 0) {
                uint32_t* segs = new uint32_t[size_t(sc.n_segments)];
                rs = mdjpeg_scan(exact, bytes.size(), &sc, segs, size_t(sc.n_segments));
                delete[] segs;
            }
            for (int bits : {64, 1024}) {
                mdjpeg_info info2;
                int16_t* coef2 = new int16_t[size_t(info.coef_count)];
                const int r2 = mdjpeg_decode_subsequences(exact, bytes.size(), bits, &info2, coef2, size_t(info.coef_count));
                delete[] coef2;
                if (r2 != rc) { printf("%s: subsequences of %d bits give %d, mdjpeg_decode %d\n", argv[i], bits, r2, rc); return 3; }
            }
        }
        printf("%s: rc %d %s\n", argv[i], rc, info.reason);
        delete[] exact;
    }
    return 0;
}
#endif
