// mdhip_repeat_detections: repeat-detection elimination on the GPU (include/mdhip.h; DESIGN.md "Repeat-detection elimination").
//
// The rule is sequential -- a box opens a new candidate only if it matches no candidate opened before it -- so the boxes are
// resolved in chunks, in order, three launches a chunk, ordered by the stream alone:
//   rde_prior    chunk rows x the candidates earlier chunks opened in the chunk's first group (no later group has any yet):
//                one flag a row
//   rde_mask     chunk rows x chunk rows below the diagonal: the match bits, one wave64 ballot per 64 of them
//   rde_resolve  ONE wave walks the chunk's rows in order against the bits of the rows it has accepted, appends the accepted
//                rows to the compacted candidate array and leaves the new count in device memory for the next chunk
// The host synchronises once behind the last chunk.  With the candidates known the rest is parallel: rde_count counts every
// candidate's instances (integer atomics: the sum has no order), the host turns the counts into offsets, and rde_fill writes
// each suspicious candidate's instances by rank, so the order of `pairs` is fixed.  No workgroup waits for another.
// Exact rounding (rde_match.h): this file is compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <vector>

#include "mdhip_ctx.h"
#include "rde_match.h"

namespace {

constexpr int kTile = 256;        // threads of rde_prior / rde_count, and boxes of their LDS tiles
constexpr int kDefaultChunk = 1024;
constexpr int kPriorSlices = 64;  // most candidate tiles a row tile of rde_prior is split over
constexpr int kCountSlices = 32;  // row slices a candidate tile of rde_count is split over

__global__ void __launch_bounds__(kTile) rde_prepare_kernel(const mdhip_rde_box* __restrict__ boxes, const int32_t* __restrict__ gid,
                                                            int32_t n, rde_pbox* __restrict__ pb) {
    const int32_t i = blockIdx.x * kTile + threadIdx.x;
    if (i < n) pb[i] = rde_prepare(boxes[i].x, boxes[i].y, boxes[i].w, boxes[i].h, gid[i], boxes[i].category);
}

// rows r0 .. r0 + m - 1 against the candidates [*cand_lo, *n_cand): hit[local row] = 1 where one matches.  blockIdx.x: tile of
// 256 rows (one a thread); blockIdx.y strides over the candidate tiles, which go through LDS.
__global__ void __launch_bounds__(kTile) rde_prior_kernel(const rde_pbox* __restrict__ pb, int32_t r0, int32_t m,
                                                          const rde_pbox* __restrict__ cbox, const int32_t* __restrict__ cand_lo,
                                                          const int32_t* __restrict__ n_cand, double thr, int agnostic,
                                                          uint8_t* __restrict__ hit) {
    __shared__ rde_pbox tile[kTile];
    const int32_t hi = *n_cand;
    const int32_t lo = *cand_lo < 0 ? 0 : *cand_lo;
    const int32_t rl = blockIdx.x * kTile + threadIdx.x;
    rde_pbox mine;
    mine.ok = 0;
    if (rl < m) mine = pb[r0 + rl];
    bool found = false;
    for (int64_t t = lo + (int64_t)blockIdx.y * kTile; t < hi; t += (int64_t)gridDim.y * kTile) {
        const int32_t cnt = (int32_t)(hi - t < kTile ? hi - t : kTile);
        __syncthreads();
        if ((int32_t)threadIdx.x < cnt) tile[threadIdx.x] = cbox[t + threadIdx.x];
        __syncthreads();
        if (rl < m)
            for (int32_t k = 0; k < cnt; ++k) found |= rde_match(mine, tile[k], thr, agnostic);
    }
    if (found) hit[rl] = 1;       // several blocks may store the same 1
}

// Match bits of one chunk below the diagonal, word-major: bits[w * pad + row] holds, in bit j, whether local row `row` matches
// local row 64 w + j < row.  One wave a (word, 64-row tile) pair; pairs above the diagonal are skipped and never read.
__global__ void __launch_bounds__(64) rde_mask_kernel(const rde_pbox* __restrict__ pb, int32_t r0, int32_t m, int32_t pad, double thr,
                                                      int agnostic, unsigned long long* __restrict__ bits) {
    const int32_t w = blockIdx.x, rt = blockIdx.y, lane = threadIdx.x;
    if (w > rt) return;
    __shared__ rde_pbox rows[64];
    const int32_t col = w * 64 + lane, row0 = rt * 64;
    rde_pbox c;
    c.ok = 0;
    c.group = -1;
    if (col < m) c = pb[r0 + col];
    if (row0 + lane < m) rows[lane] = pb[r0 + row0 + lane];
    __syncthreads();
    unsigned long long mine = 0;
    const int32_t nrows = m - row0 < 64 ? m - row0 : 64;
    for (int32_t r = 0; r < nrows; ++r) {
        const bool bit = col < row0 + r && col < m && rde_match(rows[r], c, thr, agnostic);
        const unsigned long long b = __ballot(bit);
        if (lane == r) mine = b;
    }
    bits[(size_t)w * pad + row0 + lane] = mine;       // row0 + lane < pad: pad is a multiple of 64
}

// One wave resolves the chunk: 64 rows a step.  What the accepted rows of earlier steps say about a row is independent per
// row (a lane each); inside the step the 64 rows are walked in order against the word being built.
__global__ void __launch_bounds__(64) rde_resolve_kernel(const rde_pbox* __restrict__ pb, int32_t r0, int32_t m, int32_t pad,
                                                         const unsigned long long* __restrict__ bits, const uint8_t* __restrict__ hit,
                                                         int32_t* __restrict__ n_cand, int32_t* __restrict__ cand_row,
                                                         rde_pbox* __restrict__ cbox, int32_t* __restrict__ group_first) {
    __shared__ unsigned long long acc[RDE_MAX_CHUNK / 64];
    __shared__ unsigned long long diag[64];
    __shared__ uint8_t taken[64];
    const int32_t lane = threadIdx.x;
    const int32_t words = (m + 63) / 64;
    int32_t base = *n_cand;
    for (int32_t b = 0; b < words; ++b) {
        const int32_t rl = b * 64 + lane;
        bool t = rl >= m || hit[rl] != 0;
        for (int32_t w = 0; w < b; ++w) t |= (bits[(size_t)w * pad + rl] & acc[w]) != 0;
        diag[lane] = bits[(size_t)b * pad + rl];
        taken[lane] = t;
        __syncthreads();
        unsigned long long a = 0;
        for (int32_t l = 0; l < 64; ++l)
            if (!taken[l] && !(diag[l] & a)) a |= 1ull << l;
        if (lane == 0) acc[b] = a;
        if ((a >> lane) & 1) {
            const int32_t row = r0 + rl;
            const int32_t pos = base + __popcll(a & ((1ull << lane) - 1));
            const rde_pbox me = pb[row];
            cand_row[pos] = row;
            cbox[pos] = me;
            if (row == 0 || pb[row - 1].group != me.group) group_first[me.group] = pos;   // a group's first row is always a candidate
        }
        base += __popcll(a);
        __syncthreads();
    }
    if (lane == 0) *n_cand = base;
}

// count[p] += rows i > cand_row[p] that match candidate p.  blockIdx.x: tile of 256 candidates (one a thread); the rows from
// the tile's first candidate to the end of its last candidate's group go through LDS, split into gridDim.y slices.
__global__ void __launch_bounds__(kTile) rde_count_kernel(const rde_pbox* __restrict__ pb, const rde_pbox* __restrict__ cbox,
                                                          const int32_t* __restrict__ cand_row, int32_t n_cand,
                                                          const int32_t* __restrict__ group_end, double thr, int agnostic,
                                                          int32_t* __restrict__ count) {
    __shared__ rde_pbox tile[kTile];
    const int32_t p0 = blockIdx.x * kTile, p = p0 + threadIdx.x;
    const int32_t plast = (p0 + kTile < n_cand ? p0 + kTile : n_cand) - 1;
    const int32_t lo = cand_row[p0] + 1, hi = group_end[cbox[plast].group];
    const int32_t per = ((hi - lo + (int32_t)gridDim.y - 1) / (int32_t)gridDim.y + kTile - 1) / kTile * kTile;
    const int64_t ylo = lo + (int64_t)blockIdx.y * per;
    const int64_t yhi = ylo + per < hi ? ylo + per : hi;
    rde_pbox mine;
    mine.ok = 0;
    mine.group = -1;
    int32_t c = 0x7fffffff;
    if (p < n_cand) {
        mine = cbox[p];
        c = cand_row[p];
    }
    int32_t found = 0;
    for (int64_t t = ylo; t < yhi; t += kTile) {
        const int32_t cnt = (int32_t)(yhi - t < kTile ? yhi - t : kTile);
        __syncthreads();
        if ((int32_t)threadIdx.x < cnt) tile[threadIdx.x] = pb[t + threadIdx.x];
        __syncthreads();
        for (int32_t k = 0; k < cnt; ++k) found += (t + k > c && rde_match(tile[k], mine, thr, agnostic)) ? 1 : 0;
    }
    if (found) atomicAdd(&count[p], found);
}

// One wave a suspicious candidate: its instances (itself, then the later rows of its group that match it) in ascending order
// to pairs[offset ..], each as (instance, candidate).
__global__ void __launch_bounds__(64) rde_fill_kernel(const rde_pbox* __restrict__ pb, const rde_pbox* __restrict__ cbox,
                                                      const int32_t* __restrict__ cand_row, const int32_t* __restrict__ group_end,
                                                      const int32_t* __restrict__ susp_pos, const int64_t* __restrict__ susp_off,
                                                      double thr, int agnostic, long long* __restrict__ pairs) {
    const int32_t lane = threadIdx.x;
    const int32_t p = susp_pos[blockIdx.x];
    const rde_pbox mine = cbox[p];
    const int32_t c = cand_row[p], hi = group_end[mine.group];
    int64_t at = susp_off[blockIdx.x];
    const int64_t end = susp_off[blockIdx.x + 1];       // the count rde_count_kernel made of the same matches
    for (int64_t t = c; t < hi; t += 64) {
        const int64_t i = t + lane;
        const bool bit = i < hi && (i == c || rde_match(pb[i], mine, thr, agnostic));
        const unsigned long long b = __ballot(bit);
        if (bit) {
            const int64_t o = at + __popcll(b & ((1ull << lane) - 1));
            if (o < end) {
                pairs[2 * o] = i;
                pairs[2 * o + 1] = c;
            }
        }
        at += __popcll(b);
    }
}

// device time of the last call of this thread (mdhip_repeat_detections_times): resolution, counting, filling, in milliseconds
thread_local float g_times[3] = {0.f, 0.f, 0.f};

// device memory, the stream and the events of one call; everything is released when the call returns
struct Scratch {
    std::vector<void*> mem;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};       // around the chunks, around the count, around the fill
    int prev_device = -1;
    ~Scratch() {
        for (void* p : mem) (void)hipFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
    }
};

#define RDE_ALLOC(scr, ptr, count)                                                                  \
    do {                                                                                            \
        void* q__ = nullptr;                                                                        \
        HIP_TRY(nullptr, hipMalloc(&q__, sizeof(*(ptr)) * (size_t)((count) > 0 ? (count) : 1)));   \
        (scr).mem.push_back(q__);                                                                   \
        (ptr) = (decltype(ptr))q__;                                                                 \
    } while (0)

}  // namespace

extern "C" int mdhip_repeat_detections(int device, const mdhip_rde_box* boxes, int64_t n, double iou_threshold, int category_agnostic,
                                       int32_t occurrence_threshold, int32_t chunk, uint8_t* is_candidate, int32_t* n_instances,
                                       int64_t* pairs, int64_t capacity, int64_t* needed) {
    if (const char* what = rde_check_args(boxes, n, iou_threshold, chunk, is_candidate, n_instances, pairs, capacity, needed))
        return fail(nullptr, MDHIP_EINVAL, "mdhip_repeat_detections: %s", what);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, MDHIP_EHIP, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, MDHIP_EINVAL, "device %d outside [0,%d)", device, ndev);
    *needed = 0;
    if (n == 0) return MDHIP_OK;
    if (chunk == 0) chunk = kDefaultChunk;
    const int32_t N = (int32_t)n;

    // dense group numbers, where each group begins and ends
    std::vector<int32_t> gid(N), group_begin, group_end;
    for (int32_t i = 0; i < N; ++i) {
        if (i == 0 || boxes[i].group != boxes[i - 1].group) {
            if (i) group_end.push_back(i);
            group_begin.push_back(i);
        }
        gid[i] = (int32_t)group_begin.size() - 1;
    }
    group_end.push_back(N);
    const int32_t G = (int32_t)group_begin.size();

    Scratch scr;
    HIP_TRY(nullptr, hipGetDevice(&scr.prev_device));
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, hipStreamCreate(&scr.stream));
    hipStream_t s = scr.stream;
    for (hipEvent_t& e : scr.ev) HIP_TRY(nullptr, hipEventCreate(&e));
    g_times[0] = g_times[1] = g_times[2] = 0.f;

    const int32_t pad = (chunk + 63) / 64 * 64, max_words = pad / 64;
    mdhip_rde_box* d_boxes;
    int32_t *d_gid, *d_group_end, *d_group_first, *d_cand_row, *d_n_cand, *d_count;
    rde_pbox *d_pb, *d_cbox;
    unsigned long long* d_bits;
    uint8_t* d_hit;
    RDE_ALLOC(scr, d_boxes, N);
    RDE_ALLOC(scr, d_gid, N);
    RDE_ALLOC(scr, d_group_end, G);
    RDE_ALLOC(scr, d_group_first, G);
    RDE_ALLOC(scr, d_cand_row, N);
    RDE_ALLOC(scr, d_n_cand, 1);
    RDE_ALLOC(scr, d_count, N);
    RDE_ALLOC(scr, d_pb, N);
    RDE_ALLOC(scr, d_cbox, N);
    RDE_ALLOC(scr, d_bits, (size_t)max_words * pad);
    RDE_ALLOC(scr, d_hit, pad);
    HIP_TRY(nullptr, hipMemcpyAsync(d_boxes, boxes, sizeof(mdhip_rde_box) * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(nullptr, hipMemcpyAsync(d_gid, gid.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, s));
    HIP_TRY(nullptr, hipMemcpyAsync(d_group_end, group_end.data(), sizeof(int32_t) * (size_t)G, hipMemcpyHostToDevice, s));
    HIP_TRY(nullptr, hipMemsetAsync(d_n_cand, 0, sizeof(int32_t), s));
    HIP_TRY(nullptr, hipMemsetAsync(d_group_first, 0, sizeof(int32_t) * (size_t)G, s));
    HIP_TRY(nullptr, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)N, s));
    rde_prepare_kernel<<<dim3((N + kTile - 1) / kTile), dim3(kTile), 0, s>>>(d_boxes, d_gid, N, d_pb);

    HIP_TRY(nullptr, hipEventRecord(scr.ev[0], s));
    // candidate resolution, chunk by chunk; nothing here waits for the device
    for (int32_t r0 = 0; r0 < N; r0 += chunk) {
        const int32_t m = N - r0 < chunk ? N - r0 : chunk;
        const int32_t words = (m + 63) / 64;
        const int32_t earlier = r0 - group_begin[gid[r0]];      // rows of the chunk's first group in front of the chunk
        HIP_TRY(nullptr, hipMemsetAsync(d_hit, 0, (size_t)pad, s));
        if (earlier > 0) {
            int32_t slices = (earlier + kTile - 1) / kTile;      // candidates among them: at most that many
            if (slices > kPriorSlices) slices = kPriorSlices;
            rde_prior_kernel<<<dim3((m + kTile - 1) / kTile, slices), dim3(kTile), 0, s>>>(
                d_pb, r0, m, d_cbox, d_group_first + gid[r0], d_n_cand, iou_threshold, category_agnostic, d_hit);
        }
        rde_mask_kernel<<<dim3(words, words), dim3(64), 0, s>>>(d_pb, r0, m, pad, iou_threshold, category_agnostic, d_bits);
        rde_resolve_kernel<<<dim3(1), dim3(64), 0, s>>>(d_pb, r0, m, pad, d_bits, d_hit, d_n_cand, d_cand_row, d_cbox, d_group_first);
    }
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipEventRecord(scr.ev[1], s));
    int32_t n_cand = 0;
    HIP_TRY(nullptr, hipMemcpyAsync(&n_cand, d_n_cand, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(nullptr, hipStreamSynchronize(s));
    if (n_cand < 1 || n_cand > N) return fail(nullptr, MDHIP_EHIP, "mdhip_repeat_detections: %d candidates of %d boxes", n_cand, N);

    // instances per candidate
    HIP_TRY(nullptr, hipEventRecord(scr.ev[2], s));
    rde_count_kernel<<<dim3((n_cand + kTile - 1) / kTile, kCountSlices), dim3(kTile), 0, s>>>(
        d_pb, d_cbox, d_cand_row, n_cand, d_group_end, iou_threshold, category_agnostic, d_count);
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipEventRecord(scr.ev[3], s));
    std::vector<int32_t> cand_row(n_cand), count(n_cand);
    HIP_TRY(nullptr, hipMemcpyAsync(cand_row.data(), d_cand_row, sizeof(int32_t) * (size_t)n_cand, hipMemcpyDeviceToHost, s));
    HIP_TRY(nullptr, hipMemcpyAsync(count.data(), d_count, sizeof(int32_t) * (size_t)n_cand, hipMemcpyDeviceToHost, s));
    HIP_TRY(nullptr, hipStreamSynchronize(s));
    HIP_TRY(nullptr, hipEventElapsedTime(&g_times[0], scr.ev[0], scr.ev[1]));
    HIP_TRY(nullptr, hipEventElapsedTime(&g_times[1], scr.ev[2], scr.ev[3]));
    for (int32_t i = 0; i < N; ++i) {
        is_candidate[i] = 0;
        n_instances[i] = 0;
    }
    std::vector<int32_t> susp_pos;
    std::vector<int64_t> susp_off;
    int64_t total = 0;
    for (int32_t p = 0; p < n_cand; ++p) {
        const int32_t row = cand_row[p], k = count[p] + 1;       // the kernel counted the later rows; the first instance is the candidate
        if (row < 0 || row >= N || (p && row <= cand_row[p - 1]))
            return fail(nullptr, MDHIP_EHIP, "mdhip_repeat_detections: candidate %d names row %d", p, row);
        is_candidate[row] = 1;
        n_instances[row] = k;
        if (k >= occurrence_threshold) {
            susp_pos.push_back(p);
            susp_off.push_back(total);
            total += k;
        }
    }
    susp_off.push_back(total);
    *needed = total;
    if (total > capacity)
        return fail(nullptr, MDHIP_ECAPACITY, "mdhip_repeat_detections: %lld pairs, room for %lld", (long long)total, (long long)capacity);
    if (total == 0) return MDHIP_OK;

    // the instance lists, by rank
    int32_t* d_susp_pos;
    int64_t* d_susp_off;
    long long* d_pairs;
    RDE_ALLOC(scr, d_susp_pos, susp_pos.size());
    RDE_ALLOC(scr, d_susp_off, susp_off.size());
    RDE_ALLOC(scr, d_pairs, 2 * total);
    HIP_TRY(nullptr, hipMemcpyAsync(d_susp_pos, susp_pos.data(), sizeof(int32_t) * susp_pos.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(nullptr, hipMemcpyAsync(d_susp_off, susp_off.data(), sizeof(int64_t) * susp_off.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(nullptr, hipEventRecord(scr.ev[4], s));
    rde_fill_kernel<<<dim3((unsigned)susp_pos.size()), dim3(64), 0, s>>>(d_pb, d_cbox, d_cand_row, d_group_end, d_susp_pos, d_susp_off,
                                                                       iou_threshold, category_agnostic, d_pairs);
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipEventRecord(scr.ev[5], s));
    HIP_TRY(nullptr, hipMemcpyAsync(pairs, d_pairs, sizeof(int64_t) * 2 * (size_t)total, hipMemcpyDeviceToHost, s));
    HIP_TRY(nullptr, hipStreamSynchronize(s));
    HIP_TRY(nullptr, hipEventElapsedTime(&g_times[2], scr.ev[4], scr.ev[5]));
    return MDHIP_OK;
}

extern "C" int mdhip_repeat_detections_times(float ms[3]) {
    if (!ms) return fail(nullptr, MDHIP_EINVAL, "mdhip_repeat_detections_times: ms is NULL");
    for (int i = 0; i < 3; ++i) ms[i] = g_times[i];
    return MDHIP_OK;
}
