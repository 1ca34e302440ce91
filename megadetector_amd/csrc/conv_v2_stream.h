// The streaming body of conv_v2.cpp for 1x1 / stride 1 convs with 160 input and 160 output channels (included by that unit
// only, inside its storage-type namespace; gfx950 / MI355X).
//
// Such a launch is traffic and little else (0.13 of the matrix peak), and the tiled main loop spends most of a tile on things
// that are not traffic: three K steps behind workgroup barriers, a ring that never reaches its steady state, 51 KB of weights
// fetched again per tile for 40 .. 100 KB of activations, an epilogue in which every wave of the CU stops at once.  Here the
// weights of all ten output columns (6 k steps x 10 columns x 4 registers) and the bias are loaded ONCE per wave and launch and stay
// in registers; the wave then walks groups of 16 pixels: the activation fragments of the next D - 1 groups are in flight as
// plain 16-byte buffer loads (the MFMA operand layout: lane (pixel, quarter q) holds k = 8q .. 8q + 7 of a 32-deep step,
// what read_x delivers from LDS), the current group runs its MFMA chains, the epilogue and its stores.  No LDS, no barrier:
// waves are independent and wait only on their own counters.
//
// Same bits as the tiled instantiations: per (16 pixels x 16 channels) one accumulator, MDHIP_MFMA(weights, activations, acc)
// over the six 32-deep steps in ascending order -- the sixth (k 160 .. 191: zero activations against the zero-padded weights
// as they are packed) included --, then the statements of conv_v2_kernel's 16-bit epilogue.
//
// Memory safety as there: activations and outputs go through descriptors that start at the group's first pixel and end with
// the tensor (rows_left * ld * 2), so rows past M read zeros and drop their stores without a branch, a group past the last
// one has an empty descriptor; weights and bias through descriptors of exactly their arrays.
#pragma once

// One wave per SIMD computes all 160 output channels of its pixels: the weights take 240 registers, the in-flight groups 60, and
// every activation line is read once.  Measured against it and not kept (profiles/pw_stream.txt): two waves per SIMD that share
// a stream of pixels, 80 channels each (every line read twice: slower than the tiled kernel); a stream that walks one contiguous
// run of groups instead of every n_streams-th group (the chip's access front no longer moves through the tensor in one piece:
// 7 % slower); four groups in registers instead of three (no faster).
__global__ void __launch_bounds__(256, 1)
conv_v2_stream_kernel(const ConvArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NC = 10;                    // fragment columns (16 channels) of a wave: all of N
    constexpr int D = 3;                      // groups of a wave in registers: D - 1 in flight + the one being computed
    constexpr int KS = 6, KS_REAL = 5;        // 32-deep k steps of k_pad = 192 / of the 160 channels that exist
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int px = lane & 15, q = lane >> 4;
    const int stream = (int)(blockIdx.x * 4) + wave;
    const int n_streams = (int)(gridDim.x * 4);
    const int n_groups = (p.M + 15) >> 4;
    const int iters = (n_groups + n_streams - 1) / n_streams;       // rounds: groups per stream

    // ---- weights and bias: once per launch ----------------------------------------------------------
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.wgt, 0, p.n_rows * p.k_pad * 2, kRsrcFlags);
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.bias, 0, p.n_rows * 4, kRsrcFlags);
    frag8_t w[NC][KS];
    f32x4 bv[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const unsigned row = (unsigned)((j * 16 + px) * p.k_pad + q * 8) * 2u;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            w[j][s] = __builtin_bit_cast(frag8_t, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, (int)row + s * 64, 0, 0));
        bv[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, (j * 16 + q * 4) * 4, 0, 0));
    }
    frag8_t xz = __builtin_bit_cast(frag8_t, u32x4{0u, 0u, 0u, 0u});     // the activations of k 160 .. 191
    asm volatile("" : "+v"(xz));

    // ---- the stream -----------------------------------------------------------------------------------
    const unsigned x_off = (unsigned)(px * p.ld_in * 2 + q * 16);
    const unsigned o_pair = (unsigned)(px * p.ld_out + q * 8) * 2u;     // first of this lane's 8 channels of column pair 0
    // groups are dealt round robin (those from n_groups on, which the last rounds may name, are empty), so that the chip's access front moves through the tensor in one piece
    auto group_of = [&](int it) __attribute__((always_inline)) { return it * n_streams + stream; };
    // the descriptor of a group's rows in a tensor of pixel pitch ld: empty past the last group
    auto rows_rsrc = [&](const void* base, int ld, int grp) __attribute__((always_inline)) {
        const long long left = ((long long)p.M - (long long)grp * 16) * ld * 2;
        return __builtin_amdgcn_make_buffer_rsrc((void*)((const uint16_t*)base + (long long)grp * 16 * ld), 0,
                                                 (int)(left <= 0 ? 0LL : left > 0x7fffffffLL ? 0x7fffffffLL : left), kRsrcFlags);
    };
    u32x4 x[D][KS_REAL];
    auto load = [&](int slot, int it) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t r = rows_rsrc(p.in, p.ld_in, group_of(it));
#pragma unroll
        for (int s = 0; s < KS_REAL; ++s) x[slot][s] = __builtin_amdgcn_raw_buffer_load_b128(r, (int)x_off + s * 64, 0, 0);
    };
    auto compute = [&](int slot, int it) __attribute__((always_inline)) {
#pragma clang fp contract(off)
        f32x4 acc[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < NC; ++j)
                acc[j] = MDHIP_MFMA(w[j][s], s < KS_REAL ? __builtin_bit_cast(frag8_t, x[slot][s]) : xz, acc[j]);
        // lane holds channels n .. n + 3 of pixel px in every column: bias, SiLU, two columns per 16-byte store -- a pixel's
        // bytes leave as 64-byte runs, the wave's stores of a group cover its 16 x 320 bytes
        const __amdgpu_buffer_rsrc_t o_rsrc = rows_rsrc(p.out, p.ld_out, group_of(it));
        float v[NC][4];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            mdhip_bias4(acc[j], bv[j], v[j]);
            mdhip_silu4(v[j]);
        }
#pragma unroll
        for (int j = 0; j + 1 < NC; j += 2)
            __builtin_amdgcn_raw_buffer_store_b128(conv_pack_pair(v[j], v[j + 1]), o_rsrc, (int)(o_pair + (unsigned)(j * 32)), 0, 0);
    };
#pragma unroll
    for (int d = 0; d < D - 1; ++d) {
        load(d, d);
        MDHIP_FENCE();       // (in this order: the first wait of the loop counts the loads behind the group it needs)
    }
    for (int it = 0; it < iters; it += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            // (fenced: left alone the compiler starts the next group's MFMAs under this group's SiLU, which needs the loads
            // issued last -- and waits for every load and store in flight at the top of the loop)
            load((d + D - 1) % D, it + d + D - 1);
            MDHIP_FENCE();
            compute(d, it + d);
            MDHIP_FENCE();
        }
    }
#endif  // __HIP_DEVICE_COMPILE__
}
