// Per-image non-maximum suppression on gfx950: one 1024-thread workgroup (16 wavefronts) per
// image does candidate compaction, a stable LSD radix sort by confidence and the greedy
// class-aware suppression, with wavefront ballots for every scan / match / alive-mask step.
//
// Replaces nms() at reference megadetector/detection/pytorch_detector.py:502-610 (objectness
// filter :533, xywh->xyxy :542-546, obj*cls :549, argmax class :552, confidence filter :555,
// per-class torchvision.ops.nms :569-589, sort by confidence :597, max_det :601).
//
// Exactness: per-class greedy NMS followed by a global sort and truncation to max_det is
// computed here as ONE greedy pass over all candidates in (confidence desc, anchor index asc)
// order where only same-class boxes suppress each other, stopped after max_det survivors --
// identical output, because a box's fate depends only on higher-ranked boxes of its class and
// the survivors are emitted in rank order.  All comparisons and the IoU use the same fp32
// operations as the reference (division included); compiled with -ffp-contract=off.
//
// Stage A (round 2) is its own launch spread over the chip: one CU reads 3.26 MB per image at ~15 GB/s through
// 100 barrier-separated iterations -- 0.4 of the 0.6 ms the whole NMS took at batch 32.  kScanParts workgroups per
// image compact contiguous anchor ranges into their own segment of buffer 0 (anchor order inside a segment, segments
// in anchor order: the same candidate order as before); the per-image workgroup then gathers the segments.
//
// Stages (NT = 1024 threads, image = blockIdx.x):
//   A. nms_scan_kernel: compaction in anchor order (ballot + popcount scans) -> segments of keys/vals buffer 0
//   A'. gather of the segments into buffer 1
//   S. (round 4) confidence SEGMENTS: the greedy pass stops after max_det survivors, and the benchmark's threshold
//      (1e-5, the reference's batch-mode default) lets 10^4 .. 10^5 anchors through -- sorting all of them cost 0.29 of
//      the 0.44 ms.  An 11-bit histogram of the keys' leading bits (sign, exponent, two mantissa bits) splits the
//      candidates into confidence bands; the band holding the first >= 4096 candidates is compacted (anchor order kept:
//      stable), sorted and fed to stage C; only if the kept list is still short does the next band (4x as many
//      candidates) follow.  Bands are disjoint key ranges processed in key order, so the candidate sequence stage C
//      sees is a prefix of the fully sorted one: identical output.
//   B. 4 x 8-bit stable LSD radix sort (descending confidence) of the band: every wavefront owns a
//      contiguous segment and a private 256-bin histogram in LDS; ranks inside a 64-key tile
//      come from an 8-ballot match-any
//
// Anchor-free mode (YOLO11 heads; launch_nms(..., anchor_free = true)): ultralytics non_max_suppression [3P] -- rows
// [cx, cy, w, h, cls...], no objectness, conf = the largest class score (first maximum), conf > conf_thres; only the
// kNmsMaxNmsAnchorFree highest-ranked candidates take part (max_nms); one NMS over boxes shifted by cls * 7680 (the IoU
// sees the shifted fp32 coordinates; the output boxes are re-read unshifted).  The greedy-pass argument above carries over.
// The YOLOv5 instantiation is the code as it was.
//   C. chunks of 1024 sorted candidates: filter against the kept list, then rounds of up to 64 alive candidates
//      resolved inside wavefront 0 (lane broadcasts), one barrier round per 64 instead of per kept box; stop at
//      max_det.  Measured at batch 32 (tools/nms_bench.py, 1 % / 43 % of the anchors passing): scan 0.03 ms,
//      sort 0.01 / 0.29 ms, this stage 0.15 ms, launches + D2H + sync 0.07 ms.

#include "mdhip_internal.h"

namespace mdhip {

namespace {

constexpr int NT = 1024;
constexpr int NWV = NT / 64;
constexpr int kBandBits = 11, kBandBins = 1 << kBandBits, kBandShift = 32 - kBandBits;
constexpr int kBandFirst = 4096;          // candidates the first band should hold at least (then x4 per band)

struct __attribute__((aligned(16))) NmsLds {
    float4 kept_box[kNmsMaxDet];
    float kept_conf[kNmsMaxDet];
    int kept_cls[kNmsMaxDet];
    int kept_anchor[kNmsMaxDet];          // anchor-free mode: the output box is re-read from the prediction
    union {
        uint32_t hist[NWV][256];          // stage B
        float4 chunk_box[NT];             // stage C
    } u;
    int chunk_cls[NT];
    int chunk_anchor[NT];
    float chunk_conf[NT];
    int round_nk;
    unsigned long long alive[2][NWV];
    uint32_t digit_total[256];
    uint32_t wave_cnt[NWV];
    uint32_t scan_tmp[NWV];
    uint32_t band[kBandBins];             // stage S: inclusive prefix of the candidates per leading-bits bin
    int band_end;
};

__device__ __forceinline__ unsigned long long lanemask_lt(int lane) {
    return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

__device__ __forceinline__ uint32_t sort_key_desc(float conf) {
    uint32_t u = __float_as_uint(conf);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;   // ascending-sortable
    return ~u;                                     // descending
}

__device__ __forceinline__ bool iou_gt(const float4 a, const float4 b, float thr) {
    const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y);
    const float xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float ovr = inter / (area_a + area_b - inter);
    return ovr > thr;
}

// stage A: workgroup (part, image) compacts anchors [part * per_part, (part + 1) * per_part) into keys0 / vals0 at
// offset part * per_part of the image's buffer, and stores the number of candidates it found
constexpr int NTS = 256;
template <bool AF>
__global__ void __launch_bounds__(NTS)
nms_scan_kernel(const float* __restrict__ pred_all, int n_anchors, int no, float conf_thres, int per_part,
                uint32_t* __restrict__ keys0, uint32_t* __restrict__ vals0, int cap, uint32_t* __restrict__ seg_cnt) {
    __shared__ uint32_t wave_cnt[NTS / 64];
    const int img = blockIdx.y, part = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pred = pred_all + (size_t)img * n_anchors * no;
    uint32_t* kb = keys0 + (size_t)img * cap + (size_t)part * per_part;
    uint32_t* vb = vals0 + (size_t)img * cap + (size_t)part * per_part;
    const int nc = no - (AF ? 4 : 5);
    const unsigned long long lt = lanemask_lt(lane);
    const int a_lo = part * per_part, a_hi = min(a_lo + per_part, n_anchors);
    int count = 0;
    for (int base = a_lo; base < a_hi; base += NTS) {
        const int a = base + tid;
        bool pass = false;
        uint32_t key = 0, val = 0;
        if (a < a_hi) {
            const float* p = pred + (size_t)a * no;
            if (AF) {
                // ultralytics non_max_suppression (multi_label=False): conf, j = max over the classes; conf > conf_thres
                float best = p[4];
                int bi = 0;
                for (int k = 1; k < nc; ++k) {
                    const float v = p[4 + k];
                    if (v > best) { best = v; bi = k; }
                }
                if (best > conf_thres) {
                    pass = true;
                    key = sort_key_desc(best);
                    val = (uint32_t)a | ((uint32_t)bi << 24);
                }
            } else if (p[4] > conf_thres) {
                const float obj = p[4];
                float best = p[5] * obj;
                int bi = 0;
                for (int k = 1; k < nc; ++k) {
                    const float v = p[5 + k] * obj;
                    if (v > best) { best = v; bi = k; }
                }
                if (best > conf_thres) {
                    pass = true;
                    key = sort_key_desc(best);
                    val = (uint32_t)a | ((uint32_t)bi << 24);
                }
            }
        }
        const unsigned long long bal = __ballot(pass);
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NTS / 64; ++w) {
            const uint32_t c = wave_cnt[w];
            if (w < wave) off += c;
            tot += c;
        }
        if (pass) {
            const int pos = count + (int)off + __popcll(bal & lt);
            kb[pos] = key;
            vb[pos] = val;
        }
        count += (int)tot;
        __syncthreads();
    }
    if (tid == 0) seg_cnt[(size_t)img * kNmsScanParts + part] = (uint32_t)count;
}

template <bool AF>
__global__ void __launch_bounds__(NT)
nms_image_kernel(const float* __restrict__ pred_all, int n_anchors, int no, float conf_thres,
                 float iou_thres, int max_det, int max_rank, uint32_t* keys0, uint32_t* vals0, uint32_t* keys1,
                 uint32_t* vals1, uint32_t* keys2, uint32_t* vals2, int cap, int per_part,
                 const uint32_t* __restrict__ seg_cnt, float* __restrict__ out, int* __restrict__ counts) {
    __shared__ NmsLds L;
    const int img = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const float* pred = pred_all + (size_t)img * n_anchors * no;
    // buffer 1: every candidate in anchor order (gathered below); buffers 0 and 2: the band being sorted (ping-pong)
    uint32_t* const all_k = keys1 + (size_t)img * cap;
    uint32_t* const all_v = vals1 + (size_t)img * cap;
    uint32_t* kbuf[2] = {keys0 + (size_t)img * cap, keys2 + (size_t)img * cap};
    uint32_t* vbuf[2] = {vals0 + (size_t)img * cap, vals2 + (size_t)img * cap};
    const unsigned long long lt = lanemask_lt(lane);

    // ---------------- stage A': gather the scan kernel's segments (anchor order preserved) -> buffer 1 ---------
    int count = 0;
    {
        uint32_t seg_off[kNmsScanParts + 1];
        seg_off[0] = 0;
#pragma unroll
        for (int q = 0; q < kNmsScanParts; ++q) seg_off[q + 1] = seg_off[q] + seg_cnt[(size_t)img * kNmsScanParts + q];
        count = (int)seg_off[kNmsScanParts];
#pragma unroll
        for (int q = 0; q < kNmsScanParts; ++q) {
            const int c = (int)(seg_off[q + 1] - seg_off[q]);
            const uint32_t* sk = kbuf[0] + (size_t)q * per_part;
            const uint32_t* sv = vbuf[0] + (size_t)q * per_part;
            for (int t = tid; t < c; t += NT) {
                all_k[seg_off[q] + t] = sk[t];
                all_v[seg_off[q] + t] = sv[t];
            }
        }
        __syncthreads();
    }

    // ---------------- stage S: histogram of the keys' leading bits, inclusive prefix per bin ----------------
    const int wseg = (count + NWV - 1) / NWV;                       // every wavefront owns a contiguous range of buffer 1
    const int wlo = min(wave * wseg, count), whi = min(wlo + wseg, count);
    for (int i = tid; i < kBandBins; i += NT) L.band[i] = 0;
    __syncthreads();
    for (int i = tid; i < count; i += NT) atomicAdd(&L.band[all_k[i] >> kBandShift], 1u);
    __syncthreads();
    {
        static_assert(kBandBins == 2 * NT, "two bins per thread");
        const uint32_t c0 = L.band[2 * tid], c1 = L.band[2 * tid + 1];
        uint32_t x = c0 + c1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) L.scan_tmp[wave] = x;
        __syncthreads();
        uint32_t base = 0;
        for (int w = 0; w < wave; ++w) base += L.scan_tmp[w];
        L.band[2 * tid] = base + x - c1;
        L.band[2 * tid + 1] = base + x;
        __syncthreads();
    }

    int nk = 0;
    if (max_det > kNmsMaxDet) max_det = kNmsMaxDet;
    int done = 0, b_start = 0;                                      // candidates / bins consumed by earlier bands
    uint32_t want = kBandFirst;
    // anchor-free mode: only the max_rank highest-ranked candidates take part (ultralytics max_nms); the YOLOv5 mode
    // passes max_rank >= count
    const int ranked = min(count, max_rank);
    while (done < ranked && nk < max_det) {
        // ---- this band: bins [b_start, b_end], b_end = the first bin that brings the band to `want` candidates ----
        if (tid == 0) L.band_end = kBandBins - 1;
        __syncthreads();
        {
            int mine = kBandBins;
            if (2 * tid + 1 >= b_start && L.band[2 * tid + 1] - (uint32_t)done >= want) mine = 2 * tid + 1;
            if (2 * tid >= b_start && L.band[2 * tid] - (uint32_t)done >= want) mine = 2 * tid;
            if (mine < kBandBins) atomicMin(&L.band_end, mine);
        }
        __syncthreads();
        const int b_end = L.band_end;
        const int bcount = (int)L.band[b_end] - done;
        const int bused = min(bcount, ranked - done);         // sorted candidates of this band inside the rank cut
        // ---- compaction of the band out of buffer 1 (anchor order: the sort below stays stable), wavefront ranges ----
        {
            int mine = 0;
            for (int i0 = wlo; i0 < whi; i0 += 64) {
                const int i = i0 + lane;
                const int d = i < whi ? (int)(all_k[i] >> kBandShift) : -1;
                mine += __popcll(__ballot(d >= b_start && d <= b_end));
            }
            if (lane == 0) L.wave_cnt[wave] = (uint32_t)mine;
            __syncthreads();
            int pos = 0;
            for (int w = 0; w < wave; ++w) pos += (int)L.wave_cnt[w];
            for (int i0 = wlo; i0 < whi; i0 += 64) {
                const int i = i0 + lane;
                uint32_t k = 0;
                int d = -1;
                if (i < whi) { k = all_k[i]; d = (int)(k >> kBandShift); }
                const bool in = d >= b_start && d <= b_end;
                const unsigned long long bal = __ballot(in);
                if (in) {
                    const int q = pos + __popcll(bal & lt);
                    kbuf[0][q] = k;
                    vbuf[0][q] = all_v[i];
                }
                pos += __popcll(bal);
            }
            __syncthreads();
        }

    // ---------------- stage B: stable LSD radix sort of the band, 4 passes of 8 bits ----------------
    if (bcount > 1) {
        const int seg = (bcount + NWV - 1) / NWV;
        const int lo = min(wave * seg, bcount), hi = min(lo + seg, bcount);
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = pass * 8;
            const uint32_t* sk = kbuf[pass & 1];             // the band starts in buffer 0 and is back there after 4 passes
            const uint32_t* sv = vbuf[pass & 1];
            uint32_t* dk = kbuf[(pass & 1) ^ 1];
            uint32_t* dv = vbuf[(pass & 1) ^ 1];
            for (int i = tid; i < NWV * 256; i += NT) (&L.u.hist[0][0])[i] = 0;
            __syncthreads();
            for (int i = lo + lane; i < hi; i += 64)
                atomicAdd(&L.u.hist[wave][(sk[i] >> shift) & 255], 1u);
            __syncthreads();
            // exclusive scan: digit-major, wavefront-minor
            if (tid < 256) {
                uint32_t run = 0;
#pragma unroll
                for (int w = 0; w < NWV; ++w) {
                    const uint32_t c = L.u.hist[w][tid];
                    L.u.hist[w][tid] = run;
                    run += c;
                }
                // inclusive scan of `run` over the 256 digit threads (4 wavefronts)
                uint32_t x = run;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t y = __shfl_up(x, d);
                    if (lane >= d) x += y;
                }
                if (lane == 63) L.scan_tmp[wave] = x;
                L.digit_total[tid] = x - run;      // exclusive inside the wavefront
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t base = L.digit_total[tid];
                for (int w = 0; w < wave; ++w) base += L.scan_tmp[w];
#pragma unroll
                for (int w = 0; w < NWV; ++w) L.u.hist[w][tid] += base;
            }
            __syncthreads();
            // scatter: each wavefront walks its own segment in order
            for (int i0 = lo; i0 < hi; i0 += 64) {
                const int i = i0 + lane;
                const bool valid = i < hi;
                const uint32_t k = valid ? sk[i] : 0u;
                const uint32_t v = valid ? sv[i] : 0u;
                const uint32_t d = (k >> shift) & 255u;
                unsigned long long peers = __ballot(valid);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const bool bit = (d >> b) & 1u;
                    const unsigned long long bb = __ballot(bit);
                    peers &= bit ? bb : ~bb;
                }
                const int rank = __popcll(peers & lt);
                const int cnt = __popcll(peers);
                uint32_t base = 0;
                if (valid) {
                    base = L.u.hist[wave][d];
                    dk[base + rank] = k;
                    dv[base + rank] = v;
                }
                __builtin_amdgcn_wave_barrier();
                if (valid && rank == cnt - 1) L.u.hist[wave][d] = base + (uint32_t)cnt;
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();
        }
    }
    const uint32_t* sorted_v = vbuf[0];              // four passes: back in buffer 0 (also when bcount <= 1)

    // ---------------- stage C: greedy suppression over the band's sorted candidates ----------------
    for (int c0 = 0; c0 < bused && nk < max_det; c0 += NT) {
        const int i = c0 + tid;
        const bool valid = i < bused;
        float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
        int cls = -1, anchor = -1;
        float conf = 0.f;
        if (valid) {
            const uint32_t v = sorted_v[i];
            const int a = (int)(v & 0xffffffu);
            anchor = a;
            cls = (int)(v >> 24);
            const float* p = pred + (size_t)a * no;
            const float cx = p[0], cy = p[1], w = p[2], h = p[3];
            box.x = cx - w / 2.0f;
            box.y = cy - h / 2.0f;
            box.z = cx + w / 2.0f;
            box.w = cy + h / 2.0f;
            if (AF) {
                // ultralytics: one torchvision nms over boxes + cls * max_wh (7680): the IoU sees the shifted fp32 coordinates
                const float off = (float)cls * 7680.0f;
                box.x = box.x + off; box.y = box.y + off; box.z = box.z + off; box.w = box.w + off;
                conf = p[4 + cls];
            } else {
                conf = p[5 + cls] * p[4];
            }
        }
        bool alive = valid;
        for (int k = 0; k < nk; ++k) {
            if (alive && L.kept_cls[k] == cls && iou_gt(L.kept_box[k], box, iou_thres)) alive = false;
        }
        L.u.chunk_box[tid] = box;
        L.chunk_cls[tid] = cls;
        L.chunk_conf[tid] = conf;
        L.chunk_anchor[tid] = anchor;
        {
            const unsigned long long bal = __ballot(alive);
            if (lane == 0) L.alive[0][wave] = bal;
        }
        __syncthreads();
        // Rounds of up to 64 candidates (round 2; one candidate per barrier round before: 300 rounds per image).
        // The first 64 candidates of the chunk that are still alive are resolved among themselves by wavefront 0
        // alone, in rank order, with lane broadcasts instead of barriers -- every candidate in front of the last of
        // them is either one of them or already dead, so this is exactly the sequential greedy rule -- then every
        // thread tests its candidate against the boxes kept in this round.
        while (true) {
            // (every thread reads the same words: uniform control flow)
            int total_alive = 0;
#pragma unroll
            for (int wi = 0; wi < NWV; ++wi) total_alive += __popcll(L.alive[0][wi]);
            if (total_alive == 0 || nk >= max_det) break;
            const int group = min(total_alive, 64);
            int nk_new = nk;
            // wavefront 0 clears bits of alive[0] below: every wavefront must have taken its loop-top reading of
            // those words first, or a late one could see the round's candidates already gone, leave the loop and
            // miss the barriers the others still go through
            __syncthreads();
            if (wave == 0) {
                // lane l takes the l-th alive candidate of the chunk
                int idx = -1;
                if (lane < group) {
                    int seen = 0;
                    for (int wi = 0; wi < NWV; ++wi) {
                        unsigned long long wbits = L.alive[0][wi];
                        const int c = __popcll(wbits);
                        if (lane < seen + c) {
                            for (int r = lane - seen; r > 0; --r) wbits &= wbits - 1;      // drop the r lowest set bits
                            idx = wi * 64 + __builtin_ctzll(wbits);
                            break;
                        }
                        seen += c;
                    }
                }
                float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
                int gc = -2, ga = -1;
                float gconf = 0.f;
                if (idx >= 0) { gb = L.u.chunk_box[idx]; gc = L.chunk_cls[idx]; gconf = L.chunk_conf[idx]; ga = L.chunk_anchor[idx]; }
                bool galive = idx >= 0;
                for (int k = 0; k < group; ++k) {
                    const unsigned long long am = __ballot(galive);
                    if (!((am >> k) & 1ull)) continue;                                     // uniform
                    float4 kb;
                    kb.x = __shfl(gb.x, k); kb.y = __shfl(gb.y, k); kb.z = __shfl(gb.z, k); kb.w = __shfl(gb.w, k);
                    const int kc = __shfl(gc, k);
                    if (lane > k && galive && gc == kc && iou_gt(kb, gb, iou_thres)) galive = false;
                }
                const unsigned long long km = __ballot(galive);
                const int rank = __popcll(km & lt);
                if (galive && nk + rank < max_det) {
                    L.kept_box[nk + rank] = gb;
                    L.kept_conf[nk + rank] = gconf;
                    L.kept_cls[nk + rank] = gc;
                    L.kept_anchor[nk + rank] = ga;
                }
                // the candidates of this round leave the alive set (kept or suppressed)
                if (idx >= 0) atomicAnd(&L.alive[0][idx >> 6], ~(1ull << (idx & 63)));
                if (lane == 0) L.round_nk = min(nk + (int)__popcll(km), max_det);
            }
            __syncthreads();
            nk_new = L.round_nk;
            // everybody: still alive after this round's new boxes?  (the round's own candidates were cleared above)
            const bool was = (L.alive[0][wave] >> lane) & 1ull;
            bool now = was && alive;
            if (now) {
                for (int k = nk; k < nk_new; ++k)
                    if (L.kept_cls[k] == cls && iou_gt(L.kept_box[k], box, iou_thres)) { now = false; break; }
            }
            alive = now;
            nk = nk_new;
            __syncthreads();                       // every read of alive[0] above precedes its rewrite
            const unsigned long long bal = __ballot(alive);
            if (lane == 0) L.alive[0][wave] = bal;
            __syncthreads();
        }
        __syncthreads();
    }
        // ---- next band: everything up to b_end is consumed; four times as many candidates if the kept list is still short
        done += bcount;
        b_start = b_end + 1;
        want *= 4;
        __syncthreads();
    }

    // ---------------- output ------------------------------------------------------------
    __syncthreads();
    float* o = out + (size_t)img * max_det * 6;
    for (int k = tid; k < nk; k += NT) {
        float4 b = L.kept_box[k];
        if (AF) {                                  // the unshifted box, recomputed with the same statements
            const float* p = pred + (size_t)L.kept_anchor[k] * no;
            const float cx = p[0], cy = p[1], w = p[2], h = p[3];
            b = make_float4(cx - w / 2.0f, cy - h / 2.0f, cx + w / 2.0f, cy + h / 2.0f);
        }
        o[k * 6 + 0] = b.x;
        o[k * 6 + 1] = b.y;
        o[k * 6 + 2] = b.z;
        o[k * 6 + 3] = b.w;
        o[k * 6 + 4] = L.kept_conf[k];
        o[k * 6 + 5] = (float)L.kept_cls[k];
    }
    if (tid == 0) counts[img] = nk;
}

}  // namespace

hipError_t launch_nms(const float* pred, int n, int n_anchors, int no, float conf_thres,
                      float iou_thres, int max_det, const NmsScratch& scr, float* out, int* counts,
                      hipStream_t s, bool anchor_free) {
    if (n_anchors > scr.cap || max_det > kNmsMaxDet || max_det < 1 || !scr.seg_cnt || !scr.keys[2] || !scr.vals[2]) return hipErrorInvalidValue;
    const int per_part = (n_anchors + kNmsScanParts - 1) / kNmsScanParts;
    if (anchor_free)
        hipLaunchKernelGGL(nms_scan_kernel<true>, dim3(kNmsScanParts, n), dim3(NTS), 0, s, pred, n_anchors, no, conf_thres, per_part,
                           scr.keys[0], scr.vals[0], scr.cap, scr.seg_cnt);
    else
        hipLaunchKernelGGL(nms_scan_kernel<false>, dim3(kNmsScanParts, n), dim3(NTS), 0, s, pred, n_anchors, no, conf_thres, per_part,
                           scr.keys[0], scr.vals[0], scr.cap, scr.seg_cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (anchor_free)
        hipLaunchKernelGGL(nms_image_kernel<true>, dim3(n), dim3(NT), 0, s, pred, n_anchors, no, conf_thres,
                           iou_thres, max_det, kNmsMaxNmsAnchorFree, scr.keys[0], scr.vals[0], scr.keys[1], scr.vals[1], scr.keys[2],
                           scr.vals[2], scr.cap, per_part, scr.seg_cnt, out, counts);
    else
        hipLaunchKernelGGL(nms_image_kernel<false>, dim3(n), dim3(NT), 0, s, pred, n_anchors, no, conf_thres,
                           iou_thres, max_det, 0x7fffffff, scr.keys[0], scr.vals[0], scr.keys[1], scr.vals[1], scr.keys[2],
                           scr.vals[2], scr.cap, per_part, scr.seg_cnt, out, counts);
    return hipGetLastError();
}

}  // namespace mdhip
