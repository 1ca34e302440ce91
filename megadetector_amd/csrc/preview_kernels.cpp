// GPU kernels of the annotated previews: Pillow's LANCZOS resize of device images (mdhip_resample_lanczos), bit for bit,
// and the drawing of boxes and label patches into them (mdhip_draw_ops).  The coefficient tables, the weighted sum, the
// strip plan and the walk of a pixel through its operations are those of resample.h, which libmdjpeg.so's host models
// compile too.  Integer arithmetic, plain C++ and vector memory operations only.  No access leaves an image: a dword is
// loaded or stored only where all four of its bytes belong to the row at hand, whatever the pitch and the alignment are.
//
// One launch serves one pass over EVERY image of the batch (the image is blockIdx.y or .z):
//
//   resample_rows_kernel     the horizontal pass.  A workgroup takes one strip of output pixels of `wg_rows` rows: the
//                            source run of the strip -- from the first tap of its first output pixel to the last tap of
//                            its last -- goes to LDS once (dwords where the address allows, shifted so that the LDS stores
//                            are aligned too), then one lane per output BYTE sums its taps from LDS; neighbouring lanes
//                            write neighbouring bytes.  At scale s a strip of 64 pixels reads 64 s + 6 max(s, 1) source
//                            pixels once instead of 6 max(s, 1) per output pixel.
//   resample_columns_kernel  the vertical pass is per byte: a lane owns four neighbouring bytes of an output row and walks
//                            the taps down the source rows, one dword load a tap (a wave reads 256 contiguous bytes of a
//                            row); the weights are the same for the whole workgroup, so they come through the scalar cache.
//   draw_ops_kernel          a lane owns one pixel of the rectangle its image's operations cover and takes the value of
//                            the last operation that covers it (md_draw_pixel): order-exact without launch rounds.
//   draw_ops_from_kernel     the fan-out draw (mdhip_draw_ops_from) moves every byte of every destination: a lane owns the
//                            16 bytes of a destination row that share an aligned 16-byte line -- one dwordx4 load (of any
//                            alignment) and one aligned dwordx4 store; the runs at a row's two ends go byte by byte -- and
//                            walks the operations only for the pixels of its run inside the operations' bounding box.

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "resample.h"

namespace mdhip {

namespace {

constexpr int LANES = 256;
constexpr int DRAW_X = 64, DRAW_Y = LANES / DRAW_X;
constexpr int FROM_RUN = 16;                                             // bytes of a destination row a lane moves
constexpr int FROM_X = 64, FROM_Y = LANES / FROM_X;                      // a wave moves 1 KiB of one row

static_assert(MD_RESAMPLE_LDS_BYTES <= 64 * 1024, "static LDS of a workgroup");

__global__ __launch_bounds__(LANES) void resample_rows_kernel(const ResampleRows* __restrict__ descs, const int32_t* __restrict__ table) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[MD_RESAMPLE_LDS_BYTES];
    const ResampleRows d = descs[blockIdx.y];
    if ((int)blockIdx.x >= d.strips * d.row_groups) return;              // (uniform: the whole workgroup leaves)
    const int t = threadIdx.x;
    const int g = blockIdx.x / d.strips, k = blockIdx.x - g * d.strips;
    const int y0 = g * d.wg_rows;
    const int ny = min(d.wg_rows, d.rows - y0);
    const int o0 = k * d.strip, o1 = min(o0 + d.strip, d.out_w);
    const int32_t* bounds = table + d.bounds_off;
    const int32_t* kk = table + d.kk_off;
    const int first = bounds[2 * o0];
    const int nb = (bounds[2 * (o1 - 1)] + bounds[2 * (o1 - 1) + 1] - first) * 3;   // <= run_bytes - 3 (md_resample_plan_strips)
    for (int j = 0; j < ny; ++j) {
        const uint8_t* src = d.src + (long long)(y0 + j) * d.src_pitch + (long long)first * 3;
        const int sh = (int)((uintptr_t)src & 3);                        // byte i of the run lies at row[sh + i]
        uint8_t* row = lds + j * d.run_bytes;
        const int head = min((4 - sh) & 3, nb);
        const int body = (nb - head) >> 2;
        const int tail = nb - head - 4 * body;
        if (t < head) row[sh + t] = src[t];
        for (int i = t; i < body; i += LANES)
            *reinterpret_cast<uint32_t*>(row + sh + head + 4 * i) = *reinterpret_cast<const uint32_t*>(src + head + 4 * i);
        if (t < tail) row[sh + head + 4 * body + t] = src[head + 4 * body + t];
    }
    __syncthreads();
    const int nout = (o1 - o0) * 3;
    for (int i = t; i < ny * nout; i += LANES) {
        const int j = i / nout, b = i - j * nout;
        const int px = b / 3, c = b - px * 3;
        const int o = o0 + px;
        const long long line = (long long)(y0 + j) * d.src_pitch + (long long)first * 3;
        const int sh = (int)((uintptr_t)(d.src + line) & 3);
        const uint8_t* p = lds + j * d.run_bytes + sh + (bounds[2 * o] - first) * 3 + c;
        d.dst[(long long)(y0 + j) * d.dst_pitch + (long long)o * 3 + c] = md_resample_dot(p, 3, kk + (long long)o * d.ksize, bounds[2 * o + 1]);
    }
}

__global__ __launch_bounds__(LANES) void resample_columns_kernel(const ResampleColumns* __restrict__ descs, const int32_t* __restrict__ table) {
    const ResampleColumns d = descs[blockIdx.z];
    const int y = blockIdx.y;
    const int x = (blockIdx.x * LANES + threadIdx.x) * 4;
    if (y >= d.out_h || x >= d.row_bytes) return;
    const int nbytes = min(4, d.row_bytes - x);
    const int32_t* bounds = table + d.bounds_off;
    const int32_t* k = table + d.kk_off + (long long)y * d.ksize;
    const int ymin = bounds[2 * y], cnt = bounds[2 * y + 1];
    const uint8_t* p = d.src + (long long)ymin * d.src_pitch + x;
    uint8_t* q = d.dst + (long long)y * d.dst_pitch + x;
    uint8_t out[4] = {0, 0, 0, 0};
    if (nbytes == 4 && ((uintptr_t)p & 3) == 0 && (d.src_pitch & 3) == 0) {
        int32_t s0 = 1 << (MD_RESAMPLE_PRECISION_BITS - 1), s1 = s0, s2 = s0, s3 = s0;
        for (int i = 0; i < cnt; ++i) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(p + (long long)i * d.src_pitch);
            const int32_t w = k[i];
            s0 += (int32_t)(v & 255) * w;
            s1 += (int32_t)((v >> 8) & 255) * w;
            s2 += (int32_t)((v >> 16) & 255) * w;
            s3 += (int32_t)(v >> 24) * w;
        }
        out[0] = md_resample_clip8(s0), out[1] = md_resample_clip8(s1), out[2] = md_resample_clip8(s2), out[3] = md_resample_clip8(s3);
    } else {
        for (int b = 0; b < nbytes; ++b) out[b] = md_resample_dot(p + b, d.src_pitch, k, cnt);
    }
    if (nbytes == 4 && ((uintptr_t)q & 3) == 0) {
        *reinterpret_cast<uint32_t*>(q) = (uint32_t)out[0] | (uint32_t)out[1] << 8 | (uint32_t)out[2] << 16 | (uint32_t)out[3] << 24;
    } else {
        for (int b = 0; b < nbytes; ++b) q[b] = out[b];
    }
}

__global__ __launch_bounds__(LANES) void draw_ops_kernel(const DrawImage* __restrict__ images, const int32_t* __restrict__ ops,
                                                         const uint8_t* __restrict__ patches) {
    const DrawImage d = images[blockIdx.z];
    const int x = d.x0 + (int)blockIdx.x * DRAW_X + (int)(threadIdx.x % DRAW_X);
    const int y = d.y0 + (int)blockIdx.y * DRAW_Y + (int)(threadIdx.x / DRAW_X);
    if (x > d.x1 || y > d.y1) return;                                    // (x0 .. x1, y0 .. y1 lie inside the image: mdhip_draw_ops)
    uint8_t rgb[3];
    if (!md_draw_pixel(ops + (long long)d.op_first * MD_DRAW_OP_WORDS, d.op_count, patches, x, y, rgb)) return;
    uint8_t* p = d.img + (long long)y * d.pitch + (long long)x * 3;
    p[0] = rgb[0], p[1] = rgb[1], p[2] = rgb[2];
}

struct __attribute__((packed, aligned(1))) FromRun { uint32_t w0, w1, w2, w3; };  // 16 bytes of a row wherever they lie

// byte k (0 .. 15) of a run held in four named dwords (an array indexed by k would live in scratch memory)
__device__ __forceinline__ void from_put(uint32_t& w0, uint32_t& w1, uint32_t& w2, uint32_t& w3, int k, uint32_t v) {
    if (k < 0 || k >= FROM_RUN) return;
    const int sh = (k & 3) * 8, i = k >> 2;
    const uint32_t keep = ~(0xffu << sh), bits = v << sh;
    w0 = i == 0 ? (w0 & keep) | bits : w0;
    w1 = i == 1 ? (w1 & keep) | bits : w1;
    w2 = i == 2 ? (w2 & keep) | bits : w2;
    w3 = i == 3 ? (w3 & keep) | bits : w3;
}

// the bytes first .. first + 3 of a run that lie in lo .. hi - 1 of the row, loaded into / stored from one dword
__device__ __forceinline__ uint32_t from_load4(const uint8_t* row, int first, int lo, int hi) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (first + j >= lo && first + j < hi) w |= (uint32_t)row[first + j] << (8 * j);
    return w;
}

__device__ __forceinline__ void from_store4(uint8_t* row, int first, int lo, int hi, uint32_t w) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (first + j >= lo && first + j < hi) row[first + j] = (uint8_t)(w >> (8 * j));
}

__global__ __launch_bounds__(LANES) void draw_ops_from_kernel(const DrawFrom* __restrict__ images, const int32_t* __restrict__ ops,
                                                              const uint8_t* __restrict__ patches) {
    const DrawFrom d = images[blockIdx.z];
    const int y = (int)blockIdx.y * FROM_Y + (int)(threadIdx.x / FROM_X);
    if (y >= d.height) return;
    const uint8_t* p = d.src + (long long)y * d.src_pitch;
    uint8_t* q = d.dst + (long long)y * d.dst_pitch;
    // run c holds bytes 16 c - lead .. 16 c - lead + 15 of the row, so that a whole run is one aligned 16-byte store
    const int lead = (int)((uintptr_t)q & (FROM_RUN - 1));
    const int b0 = ((int)blockIdx.x * FROM_X + (int)(threadIdx.x % FROM_X)) * FROM_RUN - lead;
    if (b0 >= d.row_bytes) return;
    const int lo = max(b0, 0), hi = min(b0 + FROM_RUN, d.row_bytes);     // the run's bytes of the row: lo .. hi - 1
    const bool whole = hi - lo == FROM_RUN;
    uint32_t w0, w1, w2, w3;
    if (whole) {
        const FromRun v = *reinterpret_cast<const FromRun*>(p + b0);     // (all 16 bytes belong to the row; any alignment)
        w0 = v.w0, w1 = v.w1, w2 = v.w2, w3 = v.w3;
    } else {
        w0 = from_load4(p, b0, lo, hi), w1 = from_load4(p, b0 + 4, lo, hi), w2 = from_load4(p, b0 + 8, lo, hi), w3 = from_load4(p, b0 + 12, lo, hi);
    }
    if (d.x1 >= d.x0 && y >= d.y0 && y <= d.y1) {                        // the operations are looked at inside their box only
        const int xa = max(lo / 3, d.x0), xb = min((hi - 1) / 3, d.x1);
        for (int x = xa; x <= xb; ++x) {
            uint8_t rgb[3];
            if (!md_draw_pixel(ops + (long long)d.op_first * MD_DRAW_OP_WORDS, d.op_count, patches, x, y, rgb)) continue;
            const int k = x * 3 - b0;                                    // (a pixel may begin before the run or end behind it)
            from_put(w0, w1, w2, w3, k, rgb[0]), from_put(w0, w1, w2, w3, k + 1, rgb[1]), from_put(w0, w1, w2, w3, k + 2, rgb[2]);
        }
    }
    if (whole) {
        *reinterpret_cast<uint4*>(q + b0) = make_uint4(w0, w1, w2, w3);
    } else {
        from_store4(q, b0, lo, hi, w0), from_store4(q, b0 + 4, lo, hi, w1), from_store4(q, b0 + 8, lo, hi, w2), from_store4(q, b0 + 12, lo, hi, w3);
    }
}

}  // namespace

hipError_t launch_resample_rows(const ResampleRows* descs, int n, int max_blocks, const int32_t* table, hipStream_t s) {
    if (n < 1 || max_blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)max_blocks, (unsigned)n), dim3(LANES), 0, s, descs, table);
    return hipGetLastError();
}

hipError_t launch_resample_columns(const ResampleColumns* descs, int n, int max_row_bytes, int max_out_h, const int32_t* table, hipStream_t s) {
    if (n < 1 || max_row_bytes < 1 || max_out_h < 1) return hipErrorInvalidValue;
    const unsigned bx = ((unsigned)(max_row_bytes + 3) / 4 + LANES - 1) / LANES;
    hipLaunchKernelGGL(resample_columns_kernel, dim3(bx, (unsigned)max_out_h, (unsigned)n), dim3(LANES), 0, s, descs, table);
    return hipGetLastError();
}

hipError_t launch_draw_ops(const DrawImage* images, int n, int max_w, int max_h, const int32_t* ops, const uint8_t* patches, hipStream_t s) {
    if (n < 1 || max_w < 1 || max_h < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_ops_kernel, dim3((unsigned)(max_w + DRAW_X - 1) / DRAW_X, (unsigned)(max_h + DRAW_Y - 1) / DRAW_Y, (unsigned)n),
                       dim3(LANES), 0, s, images, ops, patches);
    return hipGetLastError();
}

hipError_t launch_draw_ops_from(const DrawFrom* images, int n, int max_row_bytes, int max_h, const int32_t* ops, const uint8_t* patches,
                                hipStream_t s) {
    if (n < 1 || max_row_bytes < 1 || max_h < 1) return hipErrorInvalidValue;
    // a row of b bytes that begins `lead` (0 .. 15) bytes into a 16-byte line spans (lead + b + 15) / 16 runs
    const unsigned runs = ((unsigned)max_row_bytes + 2 * FROM_RUN - 2) / FROM_RUN;
    hipLaunchKernelGGL(draw_ops_from_kernel, dim3((runs + FROM_X - 1) / FROM_X, (unsigned)(max_h + FROM_Y - 1) / FROM_Y, (unsigned)n),
                       dim3(LANES), 0, s, images, ops, patches);
    return hipGetLastError();
}

}  // namespace mdhip
