// libmdjpeg.so: JPEG marker parser and Huffman entropy decoder of the loader processes (C ABI: include/mdjpeg.h).
//
// Plain C++17, host compiler, no HIP: a loader process that maps this library does not open the GPU.  The output is the
// scan's QUANTISED coefficients; de-quantisation, IDCT, upsampling, colour conversion and rotation are
// mdhip_jpeg_reconstruct (jpeg_kernels.cpp).  Every irregularity is an error code -- the caller then decodes the file
// with PIL, so that no behaviour of the ordinary path (warnings, partial images, failure strings) is restated here.
//
// Decoder: 64-bit left-aligned bit buffer refilled eight bytes at a time while no 0xFF is in sight; one 11-bit look-ahead
// per symbol that yields code length and run/size together; the canonical maxcode walk for the rare longer codes.
//
// Also here, because they read the same parsed headers: the scan descriptor (mdjpeg_scan) and the host model of the GPU
// entropy decoder (mdjpeg_decode_subsequences; device twin: jpeg_huffman.cpp, shared code: jpeg_subseq.h).  The library's
// other host models are files of their own: jpeg_encode_host.cpp, image_host.cpp, rde_host.cpp.

#include "../../include/mdjpeg.h"
#include "jpeg_subseq.h"

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

const char* mdjpeg_version(void) { return "mdjpeg 7"; }

}  // extern "C"
