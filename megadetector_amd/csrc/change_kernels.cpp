// Change detection on the GPU (mdhip_change_detect): gray + blur per image, difference + threshold + dilation + regions per pair
// of images.  Every step's arithmetic is change_detect.h's, which libmdjpeg.so's host model (change_host.cpp) compiles too.
// Integer arithmetic, plain C++, vector memory operations and ordinary vector atomics only.  No kernel waits for another
// workgroup: there is no flag and no grid barrier; the order between stages is the order of the launches on one stream.
//
//   chg_gray_rows_kernel   a workgroup takes 256 pixels of one row: RGB -> gray (zero outside the region of interest) of those
//                          pixels and of the k / 2 to either side (reflected) -> LDS; then one lane per pixel sums the k taps
//                          out of LDS: the 16-bit first pass.
//   chg_columns_kernel     one lane per pixel, neighbours in x: the k taps down the column of the first pass (coalesced rows),
//                          32-bit sum, rounded.
//   chg_diff_kernel        |a - b| per pixel.  mode 0: 256-bin histogram in LDS, added to the pair's; mode 1: the thresholded
//                          mask, the region of interest, and the count by wave popcounts (one atomic a wave).
//   chg_dilate_kernel      a 64 x 16 tile with its halo in LDS, maximum along x, then along y: as many iterations fused into
//                          one launch as the halo (CHG_DILATE_HALO) allows -- change_detect.h says why that is the same.
//   chg_label_* kernels    label equivalence by smallest raster index.  init: a pixel's parent is the first pixel of its run
//                          within its wave's 64 pixels of the row (one ballot).  merge: a pixel joins the run to its left across
//                          the 64-pixel boundary and the rows above (N, or NW and NE where N is background) with the
//                          lock-free union below.  sums: every pixel finds its root and adds itself to the root's count and
//                          extremes (one atomic set a wave where the wave's pixels share a root).
//   chg_select_* kernels   the roots with count > min_area in ascending order: counted per 256 pixels, offsets by one
//                          workgroup's scan over the counts, written by rank.
//
// LOOP BOUNDS.  find(): parent links only ever point to a smaller raster index (init writes the run's first pixel, the merge
// only lowers a link with atomicMin), so a walk visits strictly decreasing indices and ends after at most w * h - 1 steps.
// unite(): an iteration either links the two roots and ends, or found that another lane lowered the link first; links only
// decrease and there are w * h of them with w * h values each, so the retries are finite for any schedule, and no iteration
// waits for a value another lane has yet to write.  chg_scan_kernel: ceil(ceil(w * h / 256) / 256) rounds.  Every other loop
// runs over the k taps, the halo'd tile or the 256 bins.

#include <hip/hip_runtime.h>

#include "mdhip_internal.h"
#include "change_detect.h"

namespace mdhip {

namespace {

constexpr int STRIP = 256;                              // pixels of a row a workgroup of the first pass takes
constexpr int TILE_X = 64, TILE_Y = 16;                 // outputs of a dilation workgroup
constexpr int HALO2 = 2 * CHG_DILATE_HALO;
constexpr uint32_t BACKGROUND = 0xffffffffu;

__global__ __launch_bounds__(256) void chg_gray_rows_kernel(const ChgImage* __restrict__ images, const ChgWeights wt) {
    __shared__ uint8_t g[STRIP + CHG_MAX_BLUR + 1];
    const ChgImage d = images[blockIdx.z];
    const int x0 = blockIdx.x * STRIP, y = blockIdx.y;
    if (x0 >= d.w || y >= d.h) return;                  // (uniform: the whole workgroup leaves)
    const int r = wt.k / 2;
    const bool kept = y >= d.y0 && y < d.y1;
    const uint8_t* row = d.rgb + (long long)y * d.pitch;
    for (int i = threadIdx.x; i < STRIP + 2 * r; i += 256) {
        uint8_t v = 0;
        if (kept && x0 - r + i < d.w + r) {             // (beyond w + r no lane of this strip reads)
            const int xx = chg_reflect101(x0 - r + i, d.w);
            v = (uint8_t)chg_gray(row[3 * xx], row[3 * xx + 1], row[3 * xx + 2]);
        }
        g[i] = v;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= d.w) return;
    uint32_t s = 0;
    for (int t = 0; t < wt.k; ++t) s += (uint32_t)wt.w[t] * g[threadIdx.x + t];
    d.first[(size_t)y * d.w + x] = (uint16_t)s;
}

__global__ __launch_bounds__(256) void chg_columns_kernel(const ChgImage* __restrict__ images, const ChgWeights wt) {
    const ChgImage d = images[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= d.w || y >= d.h) return;
    const int r = wt.k / 2;
    uint32_t s = 0;
    for (int t = 0; t < wt.k; ++t) s += (uint32_t)wt.w[t] * d.first[(size_t)chg_reflect101(y + t - r, d.h) * d.w + x];
    d.out[(size_t)y * d.w + x] = (uint8_t)((s + 32768u) >> 16);
}

__global__ __launch_bounds__(256) void chg_diff_kernel(const ChgPair* __restrict__ pairs, int mode, const int32_t* __restrict__ thr) {
    __shared__ uint32_t bins[256];
    const ChgPair d = pairs[blockIdx.y];
    const long long px = (long long)d.w * d.h, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if ((long long)blockIdx.x * 256 >= px) return;      // (uniform)
    const bool in = i < px;
    int diff = 0;
    if (in) {
        const int a = d.a[i], b = d.b[i];
        diff = a > b ? a - b : b - a;
    }
    if (mode == 0) {
        bins[threadIdx.x] = 0;
        __syncthreads();
        if (in) atomicAdd(&bins[diff], 1u);
        __syncthreads();
        if (bins[threadIdx.x]) atomicAdd(&d.hist[threadIdx.x], bins[threadIdx.x]);
        return;
    }
    const int y = in ? (int)(i / d.w) : 0;
    const bool on = in && diff > thr[blockIdx.y] && y >= d.y0 && y < d.y1;
    if (in) d.m[0][i] = on ? 255 : 0;
    const unsigned long long ballot = __ballot(on);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(d.count, (unsigned long long)__popcll(ballot));
}

// columns x - lo .. x + hi and rows y - lo .. y + hi; lo, hi <= CHG_DILATE_HALO
__global__ __launch_bounds__(256) void chg_dilate_kernel(const ChgPair* __restrict__ pairs, int sel, int lo, int hi) {
    __shared__ uint8_t in[TILE_Y + HALO2][TILE_X + HALO2];
    __shared__ uint8_t hx[TILE_Y + HALO2][TILE_X];
    const ChgPair d = pairs[blockIdx.z];
    const int bx0 = blockIdx.x * TILE_X, by0 = blockIdx.y * TILE_Y;
    if (bx0 >= d.w || by0 >= d.h) return;               // (uniform)
    const uint8_t* __restrict__ src = d.m[sel];
    uint8_t* __restrict__ dst = d.m[sel ^ 1];
    const int reach = lo + hi, rows = TILE_Y + reach, cols = TILE_X + reach;
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
        const int rr = i / cols, cc = i % cols, gx = bx0 - lo + cc, gy = by0 - lo + rr;
        in[rr][cc] = (gx >= 0 && gy >= 0 && gx < d.w && gy < d.h) ? src[(size_t)gy * d.w + gx] : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * TILE_X; i += 256) {
        const int rr = i / TILE_X, cc = i % TILE_X;
        uint8_t v = 0;
        for (int t = 0; t <= reach; ++t) v |= in[rr][cc + t];
        hx[rr][cc] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TILE_Y * TILE_X; i += 256) {
        const int rr = i / TILE_X, cc = i % TILE_X, gx = bx0 + cc, gy = by0 + rr;
        if (gx >= d.w || gy >= d.h) continue;
        uint8_t v = 0;
        for (int t = 0; t <= reach; ++t) v |= hx[rr + t][cc];
        dst[(size_t)gy * d.w + gx] = v ? 255 : 0;
    }
}

// ---- labels ------------------------------------------------------------------------------------------------------------------

// (links change while the merge runs: they are read past this compute unit's L1, at device scope)
__device__ __forceinline__ uint32_t link_of(const uint32_t* L, uint32_t i) {
    return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t find(const uint32_t* L, uint32_t i) {
    uint32_t p;
    while ((p = link_of(L, i)) != i) i = p;             // strictly decreasing: at most w * h - 1 steps
    return i;
}

__device__ void unite(uint32_t* L, uint32_t a, uint32_t b) {
    bool done = false;
    while (!done) {                                     // (bounded: see LOOP BOUNDS)
        a = find(L, a);
        b = find(L, b);
        if (a == b) break;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&L[b], a);       // b was a root when read: link it below a, unless someone was faster
        done = old == b;
        b = old;
    }
}

// workgroups of 64 x 4 lanes: a wave is 64 neighbouring pixels of one row
__global__ __launch_bounds__(256) void chg_label_init_kernel(const ChgPair* __restrict__ pairs, int sel) {
    const ChgPair d = pairs[blockIdx.z];
    const int lane = threadIdx.x, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
    if ((int)blockIdx.x * 64 >= d.w || y >= d.h) return;            // (uniform within a wave)
    const size_t i = (size_t)y * d.w + x;
    const bool fg = x < d.w && d.m[sel][i] != 0;
    const unsigned long long ballot = __ballot(fg);
    if (x >= d.w) return;
    if (!fg) {
        d.label[i] = BACKGROUND;
        return;
    }
    const unsigned long long gaps_below = ~ballot & ((1ull << lane) - 1ull);
    const int start = gaps_below ? 64 - __clzll((long long)gaps_below) : 0;     // the first lane of this pixel's run in the wave
    d.label[i] = (uint32_t)(i - (size_t)(lane - start));
    if (start == lane) {                                            // only such a pixel can end up as a root
        const size_t px = (size_t)d.w * d.h;
        d.stat[i] = 0;
        d.stat[px + i] = 0xffffffffu;
        d.stat[2 * px + i] = 0xffffffffu;
        d.stat[3 * px + i] = 0;
        d.stat[4 * px + i] = 0;
    }
}

__global__ __launch_bounds__(256) void chg_label_merge_kernel(const ChgPair* __restrict__ pairs, int sel) {
    const ChgPair d = pairs[blockIdx.z];
    const int lane = threadIdx.x, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= d.w || y >= d.h) return;
    const uint8_t* __restrict__ m = d.m[sel];
    const size_t i = (size_t)y * d.w + x;
    if (!m[i]) return;
    const bool west = x > 0 && m[i - 1];
    if (lane == 0 && west) unite(d.label, (uint32_t)i, (uint32_t)(i - 1));
    if (y == 0) return;
    const size_t up = i - (size_t)d.w;
    if (m[up]) {
        // (where W and NW are set too, W joins NW and this pixel's run holds W: nothing to add)
        if (!(west && m[up - 1])) unite(d.label, (uint32_t)i, (uint32_t)up);
    } else {
        if (x > 0 && m[up - 1]) unite(d.label, (uint32_t)i, (uint32_t)(up - 1));
        if (x + 1 < d.w && m[up + 1]) unite(d.label, (uint32_t)i, (uint32_t)(up + 1));
    }
}

__global__ __launch_bounds__(256) void chg_label_sums_kernel(const ChgPair* __restrict__ pairs, int sel) {
    const ChgPair d = pairs[blockIdx.z];
    const int lane = threadIdx.x, x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
    if ((int)blockIdx.x * 64 >= d.w || y >= d.h) return;            // (uniform within a wave)
    const size_t i = (size_t)y * d.w + x, px = (size_t)d.w * d.h;
    const bool fg = x < d.w && d.m[sel][i] != 0;
    const uint32_t root = fg ? find(d.label, (uint32_t)i) : BACKGROUND;
    if (d.label_out && x < d.w) d.label_out[i] = (int32_t)root;     // (BACKGROUND reads as -1)
    const unsigned long long ballot = __ballot(fg);
    if (!ballot) return;
    const int first = __ffsll((long long)ballot) - 1, last = 63 - __clzll((long long)ballot);
    const uint32_t first_root = (uint32_t)__shfl((int)root, first);
    const bool shared = __all(!fg || root == first_root);
    if (shared) {
        if (lane == first) {
            const int xb = blockIdx.x * 64;
            atomicAdd(&d.stat[root], (uint32_t)__popcll(ballot));
            atomicMin(&d.stat[px + root], (uint32_t)(xb + first));
            atomicMin(&d.stat[2 * px + root], (uint32_t)y);
            atomicMax(&d.stat[3 * px + root], (uint32_t)(xb + last));
            atomicMax(&d.stat[4 * px + root], (uint32_t)y);
        }
    } else if (fg) {
        atomicAdd(&d.stat[root], 1u);
        atomicMin(&d.stat[px + root], (uint32_t)x);
        atomicMin(&d.stat[2 * px + root], (uint32_t)y);
        atomicMax(&d.stat[3 * px + root], (uint32_t)x);
        atomicMax(&d.stat[4 * px + root], (uint32_t)y);
    }
}

// ---- the significant labels in ascending order -------------------------------------------------------------------------------

__device__ __forceinline__ bool significant(const ChgPair& d, long long i, long long px, int min_area) {
    return i < px && d.label[i] == (uint32_t)i && d.stat[i] > (uint32_t)min_area;
}

__global__ __launch_bounds__(256) void chg_select_count_kernel(const ChgPair* __restrict__ pairs, int min_area) {
    const ChgPair d = pairs[blockIdx.y];
    const long long px = (long long)d.w * d.h, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if ((long long)blockIdx.x * 256 >= px) return;      // (uniform)
    const int n = __syncthreads_count(significant(d, i, px, min_area));
    if (threadIdx.x == 0) d.block_count[blockIdx.x] = (uint32_t)n;
}

// one workgroup a pair: block_count[0 .. nb) -> their exclusive prefix sums behind them, the total to n_regions
__global__ __launch_bounds__(256) void chg_scan_kernel(const ChgPair* __restrict__ pairs) {
    __shared__ uint32_t part[256];
    const ChgPair d = pairs[blockIdx.x];
    const long long px = (long long)d.w * d.h;
    const int nb = (int)((px + 255) / 256);
    uint32_t running = 0;
    for (int base = 0; base < nb; base += 256) {        // ceil(nb / 256) rounds
        const int k = base + threadIdx.x;
        const uint32_t v = k < nb ? d.block_count[k] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int step = 1; step < 256; step <<= 1) {
            const uint32_t add = (int)threadIdx.x >= step ? part[threadIdx.x - step] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (k < nb) d.block_count[nb + k] = running + part[threadIdx.x] - v;
        running += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) *d.n_regions = (int32_t)running;
}

__global__ __launch_bounds__(256) void chg_select_write_kernel(const ChgPair* __restrict__ pairs, int min_area, int cap) {
    __shared__ uint32_t wave_count[4];
    const ChgPair d = pairs[blockIdx.y];
    const long long px = (long long)d.w * d.h, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if ((long long)blockIdx.x * 256 >= px) return;      // (uniform)
    const int nb = (int)((px + 255) / 256);
    const bool sig = significant(d, i, px, min_area);
    const unsigned long long ballot = __ballot(sig);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (!sig) return;
    uint32_t rank = d.block_count[nb + blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) rank += wave_count[k];
    if (rank >= (uint32_t)cap) return;
    int32_t* q = d.regions + 5 * (size_t)rank;
    const uint32_t xmin = d.stat[px + i], ymin = d.stat[2 * px + i];
    q[0] = (int32_t)xmin;
    q[1] = (int32_t)ymin;
    q[2] = (int32_t)(d.stat[3 * px + i] - xmin + 1);
    q[3] = (int32_t)(d.stat[4 * px + i] - ymin + 1);
    q[4] = (int32_t)d.stat[i];
}

}  // namespace

hipError_t launch_chg_blur(const ChgImage* images, int n, int max_w, int max_h, const ChgWeights& wt, hipStream_t s) {
    if (n < 1) return hipSuccess;
    const dim3 grid((unsigned)((max_w + STRIP - 1) / STRIP), (unsigned)max_h, (unsigned)n);
    hipLaunchKernelGGL(chg_gray_rows_kernel, grid, dim3(256), 0, s, images, wt);
    hipLaunchKernelGGL(chg_columns_kernel, grid, dim3(256), 0, s, images, wt);
    return hipGetLastError();
}

hipError_t launch_chg_diff(const ChgPair* pairs, int n, long long max_px, int mode, const int32_t* thr, hipStream_t s) {
    if (n < 1) return hipSuccess;
    hipLaunchKernelGGL(chg_diff_kernel, dim3((unsigned)((max_px + 255) / 256), (unsigned)n), dim3(256), 0, s, pairs, mode, thr);
    return hipGetLastError();
}

hipError_t launch_chg_dilate(const ChgPair* pairs, int n, int max_w, int max_h, int k, int iterations, int* sel, hipStream_t s) {
    if (n < 1 || k < 2) return hipSuccess;              // (a 1 x 1 square changes nothing)
    const int a = k / 2, b = k - 1 - a, fuse = std::max(1, CHG_DILATE_HALO / std::max(a, b));
    const dim3 grid((unsigned)((max_w + TILE_X - 1) / TILE_X), (unsigned)((max_h + TILE_Y - 1) / TILE_Y), (unsigned)n);
    while (iterations > 0) {
        const int f = std::min(fuse, iterations);
        int lo, hi;
        chg_dilate_reach(k, f, &lo, &hi);
        if (lo > CHG_DILATE_HALO || hi > CHG_DILATE_HALO) return hipErrorInvalidValue;
        hipLaunchKernelGGL(chg_dilate_kernel, grid, dim3(256), 0, s, pairs, *sel, lo, hi);
        *sel ^= 1;
        iterations -= f;
    }
    return hipGetLastError();
}

hipError_t launch_chg_regions(const ChgPair* pairs, int n, int max_w, int max_h, int sel, int min_area, int cap, hipStream_t s) {
    if (n < 1) return hipSuccess;
    const dim3 grid((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)n), block(64, 4);
    hipLaunchKernelGGL(chg_label_init_kernel, grid, block, 0, s, pairs, sel);
    hipLaunchKernelGGL(chg_label_merge_kernel, grid, block, 0, s, pairs, sel);
    hipLaunchKernelGGL(chg_label_sums_kernel, grid, block, 0, s, pairs, sel);
    const long long max_px = (long long)max_w * max_h;
    const dim3 flat((unsigned)((max_px + 255) / 256), (unsigned)n);
    hipLaunchKernelGGL(chg_select_count_kernel, flat, dim3(256), 0, s, pairs, min_area);
    hipLaunchKernelGGL(chg_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, pairs);
    hipLaunchKernelGGL(chg_select_write_kernel, flat, dim3(256), 0, s, pairs, min_area, cap);
    return hipGetLastError();
}

}  // namespace mdhip
