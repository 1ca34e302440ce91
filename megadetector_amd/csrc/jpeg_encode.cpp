// GPU entropy ENCODING of crops (mdhip_jpeg_encode): from windows of device images to the entropy-coded scans Pillow /
// libjpeg-turbo write for Image.save(quality = q), byte for byte.  The block encoder, the offset arithmetic and the stuffing
// chunk are those of jpeg_encode.h, which libmdjpeg.so's host model compiles too; the lossy half shares its statements with
// jpeg_kernels.cpp (jpeg_dct.h).  Plain C++ and vector memory operations only.
//
// One launch grid per pass for the WHOLE batch; work is mapped by block (or chunk) number across all crops, the crop found
// by a binary search over the crops' first blocks, so a 1 x 1 crop at 4:2:0 is six lanes of a workgroup it shares with its
// neighbours and a 700 x 500 crop is 8448 lanes over 33 workgroups.  The blocks of an MCU and what each of them is are the
// crop's own (MdjEncCrop::hs, vs, per_mcu), and so is its pair of quantisation tables (MdjEncCrop::table):
//
//   jpeg_enc_coef_kernel    8 lanes per 8x8 block, 32 blocks per workgroup: colour conversion of the block's pixels (edges
//                           replicated, chroma down-sampled as the crop's sampling says: jcsample.c fullsize_downsample,
//                           h2v1_downsample or h2v2_downsample), "islow" forward DCT rows -> LDS -> columns, quantisation
//                           by the crop's own pair of tables;
//                           int16 coefficients in MCU order, a lane stores its column with one 16-byte store.
//                           mdhip_jpeg_encode_kept: a block of an MCU that no changed rectangle touches (jpeg_keep.h)
//                           skips all of that -- a lane loads row r of the SOURCE's block with one 16-byte load and the
//                           rows go through the same LDS tile to the lanes that store the columns
//   jpeg_enc_bits_kernel    lane = block: DC difference (a local read), zig-zag walk -> the block's bit length
//   scan (three kernels)    exclusive prefix sum over all blocks; a crop's own offsets are differences to its first block's
//   jpeg_enc_write_kernel   lane = block: the same walk, bits into the crop's region of the zeroed bit buffer; interior
//                           words are plain stores, the first and last word of a block's range atomicOr
//   jpeg_enc_count_kernel   lane = chunk of unstuffed bytes: bytes + FF bytes
//   scan                    where every chunk's output begins: the crops' scans lie one behind the other
//   jpeg_enc_stuff_kernel   lane = chunk: copies its bytes with a 00 behind every FF; nothing at or beyond the capacity
//   jpeg_enc_sizes_kernel   per crop offset and size, and the capacity the call needs, for ONE read by the host

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "jpeg_dct.h"
#include "jpeg_encode.h"
#include "jpeg_keep.h"

namespace mdhip {

namespace {

using namespace jpeg_dct;

constexpr int COEF_BLOCKS = 32;          // 8x8 blocks per workgroup of the coefficient kernel: 256 threads
constexpr int LANES = 256;               // workgroup of the lane-per-block / lane-per-chunk kernels
constexpr int SCAN_ITEMS = 4;            // values a thread of the scan kernels takes
constexpr int SCAN_TILE = LANES * SCAN_ITEMS;

// (8 waves a SIMD, as before the sampling became data: the three chroma branches must not cost the kernel a wave, and
// neither does the kept branch: its rectangle loop depends on the MCU alone and ends before a pixel is loaded, and a kept
// block holds 4 registers of source values where a recomputed one holds 16 of samples -- 57 VGPRs and no scratch with it as without it; 8 waves need <= 64)
__global__ __launch_bounds__(COEF_BLOCKS * 8) __attribute__((amdgpu_waves_per_eu(8, 8))) void jpeg_enc_coef_kernel(const JpegEncDev d) {
    __shared__ int lds[COEF_BLOCKS][8][9];
    const int t = threadIdx.x;
    const int lb = t >> 3, r = t & 7;
    const long long g = (long long)blockIdx.x * COEF_BLOCKS + lb;         // block number within the batch
    const bool active = g < d.blocks;
    bool real = false, keep = false;
    int chroma = 0;
    const uint16_t* quant = d.quant;                                      // the crop's pair of tables
    int v[8], ws[8];
    if (active) {
        const int ci = mdj_enc_locate<&MdjEncCrop::block0>(d.crops, d.n, g);
        const MdjEncCrop& c = d.crops[ci];
        const long long local = g - c.block0;
        const int hs = c.hs, vs = c.vs, per_mcu = c.per_mcu, luma = hs * vs;
        const unsigned m = unsigned(local) / unsigned(per_mcu);           // (a crop has at most 2^21 blocks)
        const int k = int(unsigned(local) - m * unsigned(per_mcu));
        const int my = int(m / unsigned(c.mcus_x)), mx = int(m - unsigned(my) * unsigned(c.mcus_x));
        const int W = c.width, H = c.height;
        quant = d.quant + c.table * 128;
        real = mdj_enc_block_real(c, m, k);
        keep = d.source != nullptr && !mdj_keep_changed(d.rects, d.rect0[ci], d.rect0[ci + 1], mx, my, hs, vs);
        if (keep) {                                                       // row r of the source's block, as it is (dummy blocks too)
            const uint4 row = *reinterpret_cast<const uint4*>(d.source[ci] + mdj_keep_source_offset(c, mx, my, k) + r * 8);
            lds[lb][r][0] = int(row.x & 0xffffu), lds[lb][r][1] = int(row.x >> 16);
            lds[lb][r][2] = int(row.y & 0xffffu), lds[lb][r][3] = int(row.y >> 16);
            lds[lb][r][4] = int(row.z & 0xffffu), lds[lb][r][5] = int(row.z >> 16);
            lds[lb][r][6] = int(row.w & 0xffffu), lds[lb][r][7] = int(row.w >> 16);
        } else if (k < luma) {
            if (real) {                                                   // row r of a luma block
                const int kx = hs == 2 ? k & 1 : 0, ky = hs == 2 ? k >> 1 : k;
                const int sy = min((my * vs + ky) * 8 + r, H - 1);
                const int x0 = (mx * hs + kx) * 8;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    int y, cb, cr;
                    load_ycc(c.src, c.pitch, min(x0 + i, W - 1), sy, y, cb, cr);
                    v[i] = y - 128;
                }
            }
        } else if (hs == 1) {                                             // row r of a chroma block, h1v1: 1 x 8 pixels
            chroma = 1;
            const int sy = min(my * 8 + r, H - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {                                 // fullsize_downsample: the samples as they are
                int y, cb, cr;
                load_ycc(c.src, c.pitch, min(mx * 8 + i, W - 1), sy, y, cb, cr);
                v[i] = (k == luma ? cb : cr) - 128;
            }
        } else if (vs == 1) {                                             // h2v1: 1 x 16 pixels
            chroma = 1;
            const int sy = min(my * 8 + r, H - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int sx0 = min((mx * 8 + i) * 2, W - 1), sx1 = min((mx * 8 + i) * 2 + 1, W - 1);
                int y, cb[2], cr[2];
                load_ycc(c.src, c.pitch, sx0, sy, y, cb[0], cr[0]);
                load_ycc(c.src, c.pitch, sx1, sy, y, cb[1], cr[1]);
                const int bias = i & 1;                                   // h2v1_downsample: 0 in even output columns, 1 in odd ones
                const int s = k == luma ? cb[0] + cb[1] : cr[0] + cr[1];
                v[i] = int(unsigned(s + bias) >> 1) - 128;
            }
        } else {                                                          // h2v2: 2 x 16 pixels
            chroma = 1;
            const int ch = (H + 1) >> 1;
            const int cy = min(my * 8 + r, ch - 1);                       // below the image chroma repeats its last down-sampled row
            const int sy0 = min(2 * cy, H - 1), sy1 = min(2 * cy + 1, H - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int sx0 = min((mx * 8 + i) * 2, W - 1), sx1 = min((mx * 8 + i) * 2 + 1, W - 1);
                int y, cb[4], cr[4];
                load_ycc(c.src, c.pitch, sx0, sy0, y, cb[0], cr[0]);
                load_ycc(c.src, c.pitch, sx1, sy0, y, cb[1], cr[1]);
                load_ycc(c.src, c.pitch, sx0, sy1, y, cb[2], cr[2]);
                load_ycc(c.src, c.pitch, sx1, sy1, y, cb[3], cr[3]);
                const int bias = 1 + (i & 1);                             // h2v2_downsample: 1 in even output columns, 2 in odd ones
                const int s = k == luma ? cb[0] + cb[1] + cb[2] + cb[3] : cr[0] + cr[1] + cr[2] + cr[3];
                v[i] = int(unsigned(s + bias) >> 2) - 128;
            }
        }
        if (real && !keep) {
            fdct_1d<true>(v, ws);
#pragma unroll
            for (int i = 0; i < 8; ++i) lds[lb][r][i] = ws[i];
        }
    }
    __syncthreads();
    if (!active) return;
    uint4 o = {0u, 0u, 0u, 0u};
    if (keep) {                                                           // column r of the source's block: 16-bit halves
        o.x = unsigned(lds[lb][0][r]) | (unsigned(lds[lb][1][r]) << 16);
        o.y = unsigned(lds[lb][2][r]) | (unsigned(lds[lb][3][r]) << 16);
        o.z = unsigned(lds[lb][4][r]) | (unsigned(lds[lb][5][r]) << 16);
        o.w = unsigned(lds[lb][6][r]) | (unsigned(lds[lb][7][r]) << 16);
    } else if (real) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = lds[lb][i][r];                 // column r of the workspace
        fdct_1d<false>(v, ws);                                            // coefficients (i, r), scaled by 8
        unsigned h[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned q = quant[chroma * 64 + i * 8 + r];
            const unsigned mag = quant_magnitude(ws[i], q);
            h[i] = unsigned(ws[i] < 0 ? -int(mag) : int(mag)) & 0xffffu;
        }
        o.x = h[0] | (h[1] << 16);
        o.y = h[2] | (h[3] << 16);
        o.z = h[4] | (h[5] << 16);
        o.w = h[6] | (h[7] << 16);
    }
    *reinterpret_cast<uint4*>(d.coef + g * 64 + r * 8) = o;               // transposed block: column r lies at r * 8
}

// the code tables into LDS: 3 KB that every lane indexes at random
__device__ __forceinline__ void stage_tables(MdjEncTables& t, const MdjEncTables* src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* o = reinterpret_cast<uint32_t*>(&t);
    for (unsigned i = threadIdx.x; i < sizeof(MdjEncTables) / 4; i += blockDim.x) o[i] = s[i];
    __syncthreads();
}

__global__ __launch_bounds__(LANES) void jpeg_enc_bits_kernel(const JpegEncDev d) {
    __shared__ MdjEncTables t;
    stage_tables(t, d.tables);
    const long long g = (long long)blockIdx.x * LANES + threadIdx.x;
    if (g >= d.blocks) return;
    int crop;
    uint32_t err;
    d.len[g] = mdj_enc_lane_bits(d.crops, d.n, d.coef, t, g, &crop, &err);
    if (err) atomicOr(d.status + crop, err);
}

__global__ __launch_bounds__(LANES) void jpeg_enc_write_kernel(const JpegEncDev d) {
    __shared__ MdjEncTables t;
    stage_tables(t, d.tables);
    const long long g = (long long)blockIdx.x * LANES + threadIdx.x;
    if (g >= d.blocks) return;
    mdj_enc_lane_write(d.crops, d.n, d.coef, t, d.off, d.bitbuf, g);
}

__global__ __launch_bounds__(LANES) void jpeg_enc_count_kernel(const JpegEncDev d) {
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x;
    if (q >= d.chunks) return;
    if (d.source && d.status[mdj_enc_locate<&MdjEncCrop::chunk0>(d.crops, d.n, q)]) {   // a flagged window of encode_kept: no scan
        d.count[q] = 0;
        return;
    }
    d.count[q] = mdj_enc_lane_count(d.crops, d.n, d.off, d.bitbuf, d.chunk_bytes, q);
}

__global__ __launch_bounds__(LANES) void jpeg_enc_stuff_kernel(const JpegEncDev d) {
    const long long q = (long long)blockIdx.x * LANES + threadIdx.x;
    if (q >= d.chunks) return;
    if (d.source && d.status[mdj_enc_locate<&MdjEncCrop::chunk0>(d.crops, d.n, q)]) return;
    mdj_enc_lane_stuff(d.crops, d.n, d.off, d.bitbuf, d.chunk_bytes, d.start, d.out, d.capacity, q);
}

__global__ __launch_bounds__(LANES) void jpeg_enc_sizes_kernel(const JpegEncDev d) {
    const int c = blockIdx.x * LANES + threadIdx.x;
    if (c >= d.n) return;
    const long long o = (long long)d.start[d.crops[c].chunk0];
    d.result[c] = o;
    d.result[d.n + c] = (long long)d.start[d.crops[c + 1].chunk0] - o;
    if (c == 0) d.result[2 * d.n] = (long long)d.start[d.chunks];
}

// ---- exclusive prefix sum of n uint32 values into n + 1 uint64 values (out[n] = the sum) -------------------------------
// exclusive scan of one value per thread of the workgroup; *total = the workgroup's sum
__device__ __forceinline__ uint64_t block_exclusive(uint64_t v, uint64_t* lds, uint64_t* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    uint64_t incl = v;
    for (int step = 1; step < LANES; step <<= 1) {
        const uint64_t add = t >= step ? lds[t - step] : 0;
        __syncthreads();
        incl += add;
        lds[t] = incl;
        __syncthreads();
    }
    *total = lds[LANES - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(LANES) void scan_partial_kernel(const uint32_t* __restrict__ in, long long n, uint64_t* __restrict__ partial) {
    __shared__ uint64_t lds[LANES];
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) sum += i0 + j < n ? in[i0 + j] : 0u;
    uint64_t total;
    block_exclusive(sum, lds, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: the tiles' sums -> their exclusive prefix sums, in place
__global__ __launch_bounds__(LANES) void scan_spine_kernel(uint64_t* partial, long long tiles) {
    __shared__ uint64_t lds[LANES];
    uint64_t carry = 0;
    for (long long base = 0; base < tiles; base += LANES) {
        const long long i = base + threadIdx.x;
        const uint64_t v = i < tiles ? partial[i] : 0;
        uint64_t total;
        const uint64_t excl = block_exclusive(v, lds, &total);
        if (i < tiles) partial[i] = carry + excl;
        carry += total;
    }
}

__global__ __launch_bounds__(LANES) void scan_final_kernel(const uint32_t* __restrict__ in, long long n, const uint64_t* __restrict__ partial,
                                                          uint64_t* __restrict__ out) {
    __shared__ uint64_t lds[LANES];
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = i0 + j < n ? in[i0 + j] : 0u;
        sum += v[j];
    }
    uint64_t total;
    uint64_t run = partial[blockIdx.x] + block_exclusive(sum, lds, &total);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (i0 + j < n) out[i0 + j] = run;
        run += v[j];
        if (i0 + j + 1 == n) out[n] = run;
    }
}

hipError_t scan(const uint32_t* in, long long n, uint64_t* partial, uint64_t* out, hipStream_t s) {
    const long long tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scan_partial_kernel, dim3((unsigned)tiles), dim3(LANES), 0, s, in, n, partial);
    hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(LANES), 0, s, partial, tiles);
    hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)tiles), dim3(LANES), 0, s, in, n, partial, out);
    return hipGetLastError();
}

unsigned grid_of(long long items, int per_group) { return (unsigned)((items + per_group - 1) / per_group); }

}  // namespace

long long jpeg_encode_scan_tiles(long long n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

hipError_t launch_jpeg_encode(const JpegEncDev& d, hipStream_t s) {
    hipLaunchKernelGGL(jpeg_enc_coef_kernel, dim3(grid_of(d.blocks, COEF_BLOCKS)), dim3(COEF_BLOCKS * 8), 0, s, d);
    hipLaunchKernelGGL(jpeg_enc_bits_kernel, dim3(grid_of(d.blocks, LANES)), dim3(LANES), 0, s, d);
    hipError_t e = scan(d.len, d.blocks, d.partial, d.off, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_enc_write_kernel, dim3(grid_of(d.blocks, LANES)), dim3(LANES), 0, s, d);
    hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3(grid_of(d.chunks, LANES)), dim3(LANES), 0, s, d);
    e = scan(d.count, d.chunks, d.partial, d.start, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(grid_of(d.chunks, LANES)), dim3(LANES), 0, s, d);
    hipLaunchKernelGGL(jpeg_enc_sizes_kernel, dim3(grid_of(d.n, LANES)), dim3(LANES), 0, s, d);
    return hipGetLastError();
}

}  // namespace mdhip
