// Entropy decoding of baseline JPEG scans on the GPU (mdhip_jpeg_entropy_decode): the self-synchronising scheme over
// subsequences.  The decoder of one subsequence, the state record and the bounds are jpeg_subseq.h, which the host model
// (mdjpeg_decode_subsequences) compiles too; this file is the passes around it.  One launch grid per pass holds every
// image (blockIdx.y), restart segment and subsequence of the batch.  Integer code, vector memory instructions only.
//
//   zero     coefficient planes and the per-block AC energy
//   pass 1   every lane decodes its subsequence from its first bit, as if a DC code of the MCU's first block began there
//   pass 2   a lane whose left neighbour ended somewhere else than the lane began decodes again from there; a workgroup
//            repeats this over its 256 lanes until none of them moves, the host repeats the launch until no workgroup did
//   pass 3   exclusive scan of the blocks each lane closed, anew in every restart segment: the lane's output position
//   pass 4   the final decode from the now-verified starts: coefficients in natural order, DC as differences, the only
//            pass that flags
//   pass 5   DC differences -> values: per component a segmented prefix sum in decode order (chunk sums, a scan of the
//            chunks, the chunks again), with the range and energy checks that need the DC value

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "jpeg_subseq.h"

namespace mdhip {

namespace {

constexpr int LANES = 256;            // lanes of a workgroup

__device__ inline uint64_t load64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the image's shared record into LDS (it holds no pointers: a word-by-word copy)
__device__ inline void stage_image(MdjImage* dst, const MdjImage* src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (unsigned i = threadIdx.x; i < sizeof(MdjImage) / 4; i += blockDim.x) d[i] = s[i];
    __syncthreads();
}

// the segment of lane `lane`: the last k with lane0[k] <= lane
__device__ inline uint32_t segment_of(const uint32_t* lane0, uint32_t nseg, uint32_t lane) {
    uint32_t lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lane0[mid] <= lane) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void jpeg_entropy_zero_kernel(const JpegScanDev* devs) {
    const JpegScanDev& d = devs[blockIdx.y];
    uint4* c = reinterpret_cast<uint4*>(d.coef);
    const long long n16 = d.coef_count / 8;                       // coef_count is a multiple of 64
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) c[i] = z;
    const long long nb = d.coef_count / 64;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nb; i += (long long)gridDim.x * 256) d.energy[i] = 0;
}

__global__ __launch_bounds__(LANES) void jpeg_entropy_pass1_kernel(const JpegScanDev* devs) {
    __shared__ MdjImage im;
    const JpegScanDev& d = devs[blockIdx.y];
    if (blockIdx.x * LANES >= d.n_lanes) return;
    stage_image(&im, d.im);
    const uint32_t lane = blockIdx.x * LANES + threadIdx.x;
    if (lane >= d.n_lanes) return;
    const uint32_t seg = segment_of(d.seg_lane0, d.n_segments, lane);
    const uint32_t sub = lane - d.seg_lane0[seg];
    const uint8_t* p = d.scan + d.seg_off[seg];
    const uint32_t nb = d.seg_off[seg + 1] - 2 - d.seg_off[seg];
    const MdjState s0 = mdj_blind_start(p, nb, sub, uint32_t(im.subseq_bits));
    const MdjState e = mdj_decode_lane(im, im.tables, p, nb, s0, mdj_lane_limit(sub, uint32_t(im.subseq_bits)), nullptr);
    d.lane_seg[lane] = seg;
    d.lane_start[lane] = mdj_start_key(mdj_pack(s0));
    store64(&d.lane_end[lane], mdj_pack(e));
}

// counters[0]: lanes that decoded again (all launches of a call), counters[1]: != 0 when this launch moved a lane
__global__ __launch_bounds__(LANES) void jpeg_entropy_sync_kernel(const JpegScanDev* devs, unsigned long long* counters) {
    __shared__ MdjImage im;
    const JpegScanDev& d = devs[blockIdx.y];
    if (blockIdx.x * LANES >= d.n_lanes) return;
    stage_image(&im, d.im);
    const uint32_t lane = blockIdx.x * LANES + threadIdx.x;
    const bool live = lane < d.n_lanes;
    uint32_t seg = 0, sub = 0, nb = 0;
    const uint8_t* p = nullptr;
    uint64_t mine = 0;
    if (live) {
        seg = d.lane_seg[lane];
        sub = lane - d.seg_lane0[seg];
        p = d.scan + d.seg_off[seg];
        nb = d.seg_off[seg + 1] - 2 - d.seg_off[seg];
        mine = d.lane_start[lane];
    }
    unsigned moved = 0;
    for (int round = 0; round <= LANES; ++round) {                   // a change crosses the workgroup in at most LANES rounds
        int changed = 0;
        if (live && sub > 0) {
            const uint64_t key = mdj_start_key(load64(&d.lane_end[lane - 1]));
            if (key != mine) {
                mine = key;
                const MdjState e = mdj_decode_lane(im, im.tables, p, nb, mdj_unpack(key), mdj_lane_limit(sub, uint32_t(im.subseq_bits)), nullptr);
                store64(&d.lane_end[lane], mdj_pack(e));
                changed = 1;
                ++moved;
            }
        }
        __threadfence();
        if (!__syncthreads_or(changed)) break;
    }
    if (live) d.lane_start[lane] = mine;
    if (moved) {
        atomicAdd(&counters[0], (unsigned long long)moved);
        atomicOr(&counters[1], 1ull);
    }
}

// one workgroup per image: lane_block = blocks closed by the lanes in front of it in its segment
__global__ __launch_bounds__(256) void jpeg_entropy_scan_kernel(const JpegScanDev* devs) {
    __shared__ uint32_t v[256];
    __shared__ uint32_t f[256];
    const JpegScanDev& d = devs[blockIdx.x];
    const int t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < d.n_lanes; base += 256) {
        const uint32_t lane = base + t;
        uint32_t x = 0, h = 0;
        if (lane < d.n_lanes) {
            x = mdj_unpack(d.lane_end[lane]).n;
            h = d.seg_lane0[d.lane_seg[lane]] == lane;
        }
        v[t] = x;
        f[t] = h;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            uint32_t nv = v[t], nf = f[t];
            if (t >= off) {
                if (!nf) nv += v[t - off];
                nf |= f[t - off];
            }
            __syncthreads();
            v[t] = nv;
            f[t] = nf;
            __syncthreads();
        }
        const uint32_t incl = f[t] ? v[t] : v[t] + carry;
        if (lane < d.n_lanes) d.lane_block[lane] = incl - x;
        const uint32_t last = f[255] ? v[255] : v[255] + carry;
        __syncthreads();
        carry = last;
    }
}

__global__ __launch_bounds__(LANES) void jpeg_entropy_final_kernel(const JpegScanDev* devs, uint32_t* status) {
    __shared__ MdjImage im;
    const JpegScanDev& d = devs[blockIdx.y];
    if (blockIdx.x * LANES >= d.n_lanes) return;
    stage_image(&im, d.im);
    const uint32_t lane = blockIdx.x * LANES + threadIdx.x;
    if (lane >= d.n_lanes) return;
    const uint32_t seg = d.lane_seg[lane];
    const uint32_t sub = lane - d.seg_lane0[seg];
    const uint8_t* p = d.scan + d.seg_off[seg];
    const uint32_t nb = d.seg_off[seg + 1] - 2 - d.seg_off[seg];
    const int64_t first_mcu = int64_t(seg) * im.interval;
    int64_t mcus = im.total_mcus - first_mcu;
    if (mcus > im.interval) mcus = im.interval;
    if (mcus < 0) mcus = 0;
    MdjSink sink{d.coef, d.energy, first_mcu, int64_t(d.lane_block[lane]), mcus * im.blocks_per_mcu, 0};
    mdj_decode_lane(im, im.tables, p, nb, mdj_unpack(d.lane_start[lane]), mdj_lane_limit(sub, uint32_t(im.subseq_bits)), &sink);
    uint32_t err = sink.err;
    if (lane + 1 == d.seg_lane0[seg + 1] && sink.block < sink.blocks) err |= MDJ_ERR_COUNT;
    if (err) atomicOr(&status[blockIdx.y], err);
}

// ---- pass 5 ----------------------------------------------------------------------------------------------------------
constexpr int DC_CHUNK = 32;          // blocks of one component, in decode order, that one thread sums

// chunk g of the image -> component and first block
__device__ inline bool dc_chunk(const JpegScanDev& d, long long g, int* c, long long* j0, long long* j1) {
    for (int k = 0; k < 3; ++k) {
        if (g < d.dc_chunks[k]) {
            *c = k;
            *j0 = g * DC_CHUNK;
            *j1 = *j0 + DC_CHUNK < d.dc_blocks[k] ? *j0 + DC_CHUNK : d.dc_blocks[k];
            return true;
        }
        g -= d.dc_chunks[k];
    }
    return false;
}

__global__ __launch_bounds__(256) void jpeg_entropy_dc_sum_kernel(const JpegScanDev* devs) {
    const JpegScanDev& d = devs[blockIdx.y];
    const MdjImage& im = *d.im;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    int c;
    long long j0, j1;
    if (!dc_chunk(d, g, &c, &j0, &j1)) return;
    const long long seglen = im.interval * im.h_samp[c] * im.v_samp[c];
    long long sum = 0;
    uint32_t reset = 0;
    for (long long j = j0; j < j1; ++j) {
        if (j % seglen == 0) { sum = 0; reset = 1; }
        sum += d.coef[mdj_dc_block_offset(im, c, j) * 64];
    }
    d.dc_sum[g] = sum;
    d.dc_reset[g] = reset;
}

// one workgroup per (component, image): dc_sum[g] becomes the DC value in front of chunk g
__global__ __launch_bounds__(256) void jpeg_entropy_dc_scan_kernel(const JpegScanDev* devs) {
    __shared__ long long v[256];
    __shared__ uint32_t f[256];
    const JpegScanDev& d = devs[blockIdx.y];
    const int c = blockIdx.x, t = threadIdx.x;
    long long first = 0;
    for (int k = 0; k < c; ++k) first += d.dc_chunks[k];
    const long long n = d.dc_chunks[c];
    long long carry = 0;
    for (long long base = 0; base < n; base += 256) {
        const long long g = base + t;
        long long x = 0;
        uint32_t h = 0;
        if (g < n) { x = d.dc_sum[first + g]; h = d.dc_reset[first + g]; }
        v[t] = x;
        f[t] = h;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            long long nv = v[t];
            uint32_t nf = f[t];
            if (t >= off) {
                if (!nf) nv += v[t - off];
                nf |= f[t - off];
            }
            __syncthreads();
            v[t] = nv;
            f[t] = nf;
            __syncthreads();
        }
        // exclusive: what the chunk in front ended with (a chunk that resets ignores it anyway)
        const long long before = t == 0 ? carry : (f[t - 1] ? v[t - 1] : v[t - 1] + carry);
        const long long last = f[255] ? v[255] : v[255] + carry;
        __syncthreads();
        if (g < n) d.dc_sum[first + g] = before;
        carry = last;
    }
}

__global__ __launch_bounds__(256) void jpeg_entropy_dc_apply_kernel(const JpegScanDev* devs, uint32_t* status) {
    const JpegScanDev& d = devs[blockIdx.y];
    const MdjImage& im = *d.im;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    int c;
    long long j0, j1;
    if (!dc_chunk(d, g, &c, &j0, &j1)) return;
    const long long seglen = im.interval * im.h_samp[c] * im.v_samp[c];
    long long dc = d.dc_sum[g];
    uint32_t err = 0;
    for (long long j = j0; j < j1; ++j) {
        if (j % seglen == 0) dc = 0;
        const long long off = mdj_dc_block_offset(im, c, j);
        dc += d.coef[off * 64];
        err |= mdj_check_block(im, c, dc, d.energy[off]);
        d.coef[off * 64] = int16_t(dc);
    }
    if (err) atomicOr(&status[blockIdx.y], err);
}

}  // namespace

static inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per > 0 ? (n + per - 1) / per : 1); }

void launch_jpeg_entropy_front(const JpegScanDev* devs, int n, unsigned max_lanes, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_entropy_zero_kernel, dim3(64, n), dim3(256), 0, s, devs);
    hipLaunchKernelGGL(jpeg_entropy_pass1_kernel, dim3(blocks_for(max_lanes, LANES), n), dim3(LANES), 0, s, devs);
}

void launch_jpeg_entropy_sync(const JpegScanDev* devs, int n, unsigned max_lanes, unsigned long long* counters, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(blocks_for(max_lanes, LANES), n), dim3(LANES), 0, s, devs, counters);
}

void launch_jpeg_entropy_back(const JpegScanDev* devs, int n, unsigned max_lanes, long long max_chunks, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_entropy_scan_kernel, dim3(n), dim3(256), 0, s, devs);
    hipLaunchKernelGGL(jpeg_entropy_final_kernel, dim3(blocks_for(max_lanes, LANES), n), dim3(LANES), 0, s, devs, status);
    hipLaunchKernelGGL(jpeg_entropy_dc_sum_kernel, dim3(blocks_for(max_chunks, 256), n), dim3(256), 0, s, devs);
    hipLaunchKernelGGL(jpeg_entropy_dc_scan_kernel, dim3(3, n), dim3(256), 0, s, devs);
    hipLaunchKernelGGL(jpeg_entropy_dc_apply_kernel, dim3(blocks_for(max_chunks, 256), n), dim3(256), 0, s, devs, status);
}

int jpeg_entropy_dc_chunk() { return DC_CHUNK; }

}  // namespace mdhip
