// GPU half of the JPEG feed (mdhip_jpeg_reconstruct): quantised DCT coefficients -> the RGB pixels Pillow / libjpeg-turbo
// produce, bit for bit.  Integer arithmetic only; restates tests/jpeg_ref.py, which is pinned against Pillow.
//
//   jpeg_idct_kernel      de-quantise + libjpeg's "islow" inverse DCT (jidctint: 13-bit constants, columns then rows,
//                         rounding shifts by 11 and 18, results saturated to 0 .. 255) -> u8 component planes
//   jpeg_colour_kernel    "fancy" (triangle) chroma upsampling, 16-bit fixed-point YCbCr -> RGB, EXIF rotation as an index
//                         permutation; one thread writes four neighbouring OUTPUT pixels (12 bytes, three dwords when aligned)
//
// One launch of each per image: an image's description travels by value in the kernel arguments, so nothing of a call
// lives in device memory except the component planes (scratch of the context).
//
// JPEG recompression of a window (mdhip_jpeg_recompress): the pixels Image.save(quality=q) + Image.open give, without a file.
// The encoder's lossy half in libjpeg's integer arithmetic (restates tests/jpeg_enc_ref.py, pinned against Pillow), then
// the kernels above from the planes on:
//
//   jpeg_enc_planes_kernel   16-bit fixed-point RGB -> YCbCr, edges replicated to whole blocks, h2v2 chroma down-sampling with
//                            the alternating 1 / 2 bias -> u8 component planes; one thread = 4 x 2 luma samples + 2 of each chroma
//   jpeg_requant_kernel      per 8x8 block of a plane, in place: samples - 128, "islow" forward DCT (jfdctint: rows then
//                            columns, PASS1_BITS 2), division by 8 * table entry rounded half away from zero, times the table
//                            entry, and the inverse DCT of jpeg_idct_kernel.  The quantised coefficients live in registers only.
//   jpeg_colour_kernel       as above, rotation 0

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "jpeg_dct.h"

namespace mdhip {

namespace {

using namespace jpeg_dct;

constexpr int IDCT_BLOCKS = 32;          // 8x8 blocks per workgroup: 256 threads, thread = (block, row / column)


// one 1-D pass of jpeg_idct_islow
__device__ __forceinline__ void idct_1d(const int* d, int* o, int shift) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * (-15137);
    int tmp3 = z1 + z2 * 6270;
    z2 = d[0];
    z3 = d[4];
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7];
    tmp1 = d[5];
    tmp2 = d[3];
    tmp3 = d[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * (-16069) + z5;
    z4 = z4 * (-3196) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = descale(tmp10 + tmp3, shift);
    o[7] = descale(tmp10 - tmp3, shift);
    o[1] = descale(tmp11 + tmp2, shift);
    o[6] = descale(tmp11 - tmp2, shift);
    o[2] = descale(tmp12 + tmp1, shift);
    o[5] = descale(tmp12 - tmp1, shift);
    o[3] = descale(tmp13 + tmp0, shift);
    o[4] = descale(tmp13 - tmp0, shift);
}

// post-IDCT range limit, x = sample - 128: saturation, as libjpeg-turbo's SIMD inverse DCT packs its results (and so
// Pillow's pixels).  libjpeg's C code indexes a table with (x & 1023) instead, which is the same inside [-512, 511] and
// wraps around outside it; a block within the energy bound of the entropy decoders can leave that range.
__device__ __forceinline__ unsigned range_limit(int x) {
    return unsigned(x < -128 ? 0 : (x > 127 ? 255 : x + 128));
}

__global__ __launch_bounds__(IDCT_BLOCKS * 8) void jpeg_idct_kernel(const JpegDev d) {
    __shared__ int lds[IDCT_BLOCKS][8][9];
    const int t = threadIdx.x;
    const int lb = t >> 3, r = t & 7;
    const long long g = (long long)blockIdx.x * IDCT_BLOCKS + lb;         // block number within the image, all planes
    int c = 0;
    long long b = g;
    bool active = false;
    for (int k = 0; k < d.components; ++k) {
        const long long nb = (long long)d.blocks_w[k] * d.blocks_h[k];
        if (b < nb) { c = k; active = true; break; }
        b -= nb;
    }
    if (active) {
        // row r of the block: 8 coefficients, one 16-byte load
        const int4 v = *reinterpret_cast<const int4*>(d.coef + d.coef_off[c] + b * 64 + r * 8);
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lds[lb][r][2 * i] = (int)(short)(w[i] & 0xffff) * (int)d.quant[c][r * 8 + 2 * i];
            lds[lb][r][2 * i + 1] = (w[i] >> 16) * (int)d.quant[c][r * 8 + 2 * i + 1];
        }
    }
    __syncthreads();
    int col[8], ws[8];
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) col[i] = lds[lb][i][r];               // column r
        idct_1d(col, ws, 11);
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) lds[lb][i][r] = ws[i];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) col[i] = lds[lb][r][i];               // row r of the workspace
        idct_1d(col, ws, 18);
        uint2 o;
        o.x = range_limit(ws[0]) | (range_limit(ws[1]) << 8) | (range_limit(ws[2]) << 16) | (range_limit(ws[3]) << 24);
        o.y = range_limit(ws[4]) | (range_limit(ws[5]) << 8) | (range_limit(ws[6]) << 16) | (range_limit(ws[7]) << 24);
        const int bw = d.blocks_w[c];
        const int by = (int)(b / bw), bx = (int)(b % bw);
        uint8_t* row = d.planes + d.plane_off[c] + ((long long)by * 8 + r) * ((long long)bw * 8) + bx * 8;
        *reinterpret_cast<uint2*>(row) = o;
    }
}

// chroma sample of source pixel (sx, sy): libjpeg's h2v1 / h2v2 fancy upsampling evaluated at one point; cw x ch = the
// component's downsampled size (not the padded plane), pitch = bytes per plane row
__device__ __forceinline__ int chroma_at(const uint8_t* p, int pitch, int cw, int ch, int hs, int vs, int sx, int sy) {
    if (hs == 1) return p[(long long)sy * pitch + sx];
    const int i = sx >> 1;
    if (vs == 1) {
        const uint8_t* row = p + (long long)sy * pitch;
        const int a = row[i];
        if (cw <= 2) return a;
        if (sx & 1) return i == cw - 1 ? a : (3 * a + row[i + 1] + 2) >> 2;
        return i == 0 ? a : (3 * a + row[i - 1] + 1) >> 2;
    }
    const int j = sy >> 1;
    const uint8_t* near = p + (long long)j * pitch;
    if (cw <= 2) return near[i];
    int jf = (sy & 1) ? j + 1 : j - 1;
    jf = jf < 0 ? 0 : (jf > ch - 1 ? ch - 1 : jf);
    const uint8_t* far = p + (long long)jf * pitch;
    const int cur = 3 * near[i] + far[i];
    if (sx & 1) return i == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return unsigned(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegDev d) {
    const int ow = (d.rotation == 90 || d.rotation == 270) ? d.height : d.width;
    const int oh = (d.rotation == 90 || d.rotation == 270) ? d.width : d.height;
    const int ox0 = (blockIdx.x * 16 + (threadIdx.x & 15)) * 4;
    const int oy = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (oy >= oh || ox0 >= ow) return;
    const int W = d.width, H = d.height;
    const int hs = d.h_samp, vs = d.v_samp;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const uint8_t* py = d.planes + d.plane_off[0];
    const int pitch_y = d.blocks_w[0] * 8;
    unsigned bytes[12];
    const int npix = ow - ox0 < 4 ? ow - ox0 : 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ox = ox0 + (k < npix ? k : 0);
        int sx, sy;
        if (d.rotation == 0) { sx = ox; sy = oy; }
        else if (d.rotation == 90) { sx = W - 1 - oy; sy = ox; }
        else if (d.rotation == 180) { sx = W - 1 - ox; sy = H - 1 - oy; }
        else { sx = oy; sy = H - 1 - ox; }
        const int y = py[(long long)sy * pitch_y + sx];
        if (d.components == 1) {
            bytes[3 * k] = bytes[3 * k + 1] = bytes[3 * k + 2] = unsigned(y);
        } else {
            const int pitch_c = d.blocks_w[1] * 8;
            const int cb = chroma_at(d.planes + d.plane_off[1], pitch_c, cw, ch, hs, vs, sx, sy) - 128;
            const int cr = chroma_at(d.planes + d.plane_off[2], pitch_c, cw, ch, hs, vs, sx, sy) - 128;
            bytes[3 * k] = clamp255(y + ((91881 * cr + 32768) >> 16));
            bytes[3 * k + 1] = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
            bytes[3 * k + 2] = clamp255(y + ((116130 * cb + 32768) >> 16));
        }
    }
    uint8_t* o = d.out + ((long long)oy * ow + ox0) * 3;
    if (npix == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
        o4[1] = bytes[4] | (bytes[5] << 8) | (bytes[6] << 16) | (bytes[7] << 24);
        o4[2] = bytes[8] | (bytes[9] << 8) | (bytes[10] << 16) | (bytes[11] << 24);
    } else {
        for (int k = 0; k < npix * 3; ++k) o[k] = (uint8_t)bytes[k];
    }
}

// ---- recompression: the encoder's lossy half ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void jpeg_enc_planes_kernel(const JpegDev d, const uint8_t* __restrict__ src, const long long pitch) {
    const int tx = blockIdx.x * 32 + (threadIdx.x & 31);              // two chroma columns, four luma columns
    const int cy = blockIdx.y * 8 + (threadIdx.x >> 5);               // one chroma row, two luma rows
    const int cpw = d.blocks_w[1] * 8, cph = d.blocks_h[1] * 8;       // chroma plane
    if (tx * 2 >= cpw || cy >= cph) return;
    const int W = d.width, H = d.height;
    const int ypw = d.blocks_w[0] * 8, yph = d.blocks_h[0] * 8;       // luma plane: multiples of 8, so four columns are in or out together
    const int ch = (H + 1) >> 1;
    int yv[2][4], cbv[2][4], crv[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int sy = min(2 * cy + j, H - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) load_ycc(src, pitch, min(4 * tx + k, W - 1), sy, yv[j][k], cbv[j][k], crv[j][k]);
    }
    if (4 * tx < ypw) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (2 * cy + j < yph) {
                uint8_t* row = d.planes + d.plane_off[0] + (long long)(2 * cy + j) * ypw + 4 * tx;
                *reinterpret_cast<unsigned*>(row) = unsigned(yv[j][0]) | (unsigned(yv[j][1]) << 8) | (unsigned(yv[j][2]) << 16) |
                                                    (unsigned(yv[j][3]) << 24);
            }
        }
    }
    if (cy >= ch) {                                                   // below the image chroma repeats its last down-sampled row
        int unused;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int sy = min(2 * (ch - 1) + j, H - 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) load_ycc(src, pitch, min(4 * tx + k, W - 1), sy, unused, cbv[j][k], crv[j][k]);
        }
    }
    // h2v2_downsample: the bias is 1 in even output columns and 2 in odd ones
    const unsigned cb0 = unsigned(cbv[0][0] + cbv[0][1] + cbv[1][0] + cbv[1][1] + 1) >> 2;
    const unsigned cb1 = unsigned(cbv[0][2] + cbv[0][3] + cbv[1][2] + cbv[1][3] + 2) >> 2;
    const unsigned cr0 = unsigned(crv[0][0] + crv[0][1] + crv[1][0] + crv[1][1] + 1) >> 2;
    const unsigned cr1 = unsigned(crv[0][2] + crv[0][3] + crv[1][2] + crv[1][3] + 2) >> 2;
    const long long co = (long long)cy * cpw + 2 * tx;
    *reinterpret_cast<unsigned short*>(d.planes + d.plane_off[1] + co) = (unsigned short)(cb0 | (cb1 << 8));
    *reinterpret_cast<unsigned short*>(d.planes + d.plane_off[2] + co) = (unsigned short)(cr0 | (cr1 << 8));
}

__global__ __launch_bounds__(IDCT_BLOCKS * 8) void jpeg_requant_kernel(const JpegDev d) {
    __shared__ int lds[IDCT_BLOCKS][8][9];
    const int t = threadIdx.x;
    const int lb = t >> 3, r = t & 7;
    const long long g = (long long)blockIdx.x * IDCT_BLOCKS + lb;         // block number within the image, all planes
    int c = 0;
    long long b = g;
    bool active = false;
    for (int k = 0; k < 3; ++k) {
        const long long nb = (long long)d.blocks_w[k] * d.blocks_h[k];
        if (b < nb) { c = k; active = true; break; }
        b -= nb;
    }
    uint8_t* row = nullptr;
    int v[8], ws[8];
    if (active) {
        const int bw = d.blocks_w[c];
        const int by = (int)(b / bw), bx = (int)(b % bw);
        row = d.planes + d.plane_off[c] + ((long long)by * 8 + r) * ((long long)bw * 8) + bx * 8;
        const uint2 in = *reinterpret_cast<const uint2*>(row);           // row r of the block
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = int((in.x >> (8 * i)) & 255u) - 128;
            v[4 + i] = int((in.y >> (8 * i)) & 255u) - 128;
        }
        fdct_1d<true>(v, ws);
#pragma unroll
        for (int i = 0; i < 8; ++i) lds[lb][r][i] = ws[i];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = lds[lb][i][r];                 // column r of the workspace
        fdct_1d<false>(v, ws);                                            // coefficients (i, r), scaled by 8
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned q = d.quant[c][i * 8 + r];
            const unsigned mag = quant_magnitude(ws[i], q);
            v[i] = ws[i] < 0 ? -int(mag * q) : int(mag * q);              // quantised, and de-quantised again
        }
        idct_1d(v, ws, 11);                                               // the inverse starts with the columns
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) lds[lb][i][r] = ws[i];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = lds[lb][r][i];                 // row r of the workspace
        idct_1d(v, ws, 18);
        uint2 o;
        o.x = range_limit(ws[0]) | (range_limit(ws[1]) << 8) | (range_limit(ws[2]) << 16) | (range_limit(ws[3]) << 24);
        o.y = range_limit(ws[4]) | (range_limit(ws[5]) << 8) | (range_limit(ws[6]) << 16) | (range_limit(ws[7]) << 24);
        *reinterpret_cast<uint2*>(row) = o;
    }
}

}  // namespace

hipError_t launch_jpeg_recompress(const JpegDev& d, const uint8_t* src, long long pitch, hipStream_t s) {
    const int cpw = d.blocks_w[1] * 8, cph = d.blocks_h[1] * 8;
    hipLaunchKernelGGL(jpeg_enc_planes_kernel, dim3((cpw / 2 + 31) / 32, (cph + 7) / 8), dim3(256), 0, s, d, src, pitch);
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) blocks += (long long)d.blocks_w[c] * d.blocks_h[c];
    hipLaunchKernelGGL(jpeg_requant_kernel, dim3((unsigned)((blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS)), dim3(IDCT_BLOCKS * 8), 0, s, d);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((d.width + 63) / 64, (d.height + 15) / 16), dim3(256), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_jpeg_reconstruct(const JpegDev& d, hipStream_t s) {
    long long blocks = 0;
    for (int c = 0; c < d.components; ++c) blocks += (long long)d.blocks_w[c] * d.blocks_h[c];
    const unsigned grid_a = (unsigned)((blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(grid_a), dim3(IDCT_BLOCKS * 8), 0, s, d);
    const int ow = (d.rotation == 90 || d.rotation == 270) ? d.height : d.width;
    const int oh = (d.rotation == 90 || d.rotation == 270) ? d.width : d.height;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((ow + 63) / 64, (oh + 15) / 16), dim3(256), 0, s, d);
    return hipGetLastError();
}

}  // namespace mdhip
