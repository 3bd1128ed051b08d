// The 32 x 32 output tile of a small-batch dense product y = x w^T, as dense_small_kernel (conv_direct.hip) and the fused LSTM
// step (lstm_kernel.h) both compute it: one K loop and one four-wave sum, so the two kernels give the same bits for the same
// operands.  A workgroup of four waves owns 32 rows of x and 32 rows of w; the waves take a quarter of K each, reading both
// operands straight from global memory as float4s of 4 consecutive k through bounds-checked buffer loads (nothing is shared
// between waves, so nothing goes through LDS but the final sum of the four partial tiles).  32x32x2 MFMAs: lanes 0-31 carry k,
// lanes 32-63 carry k + 4.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DENSE_TILE_OOB = (int)0x80000000;      // a byte offset no buffer descriptor holds: the load returns 0

// row of the 32 x 32 tile that accumulator register r of this lane holds; the column is lane & 31
__device__ __forceinline__ int dense_tile_row(int r, int lane) { return 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3); }

// This wave's partial tile over its share of K.  xo / wo: byte offset of this lane's row of x / w at k = 4 * (lane >> 5), or
// DENSE_TILE_OOB for a row that does not exist.  K % 8 == 0 (host check): pairs of float4.
__device__ __forceinline__ f32x16 dense_tile_kloop(__amdgpu_buffer_rsrc_t xr, __amdgpu_buffer_rsrc_t wr, int xo, int wo, int K,
                                                   int wave) {
    constexpr int OOB = DENSE_TILE_OOB;
    const int kq = K / 4;
    const int steps = kq / 2, per_wave = (steps + 3) / 4;
    const int s0 = wave * per_wave, s1 = min(steps, s0 + per_wave);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int s = s0; s < s1; s += 4) {                     // four load pairs in flight per lane
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = s + u < s1;
            a[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xr, ok ? xo : OOB, (s + u) * 32, 0));
            b[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wr, ok ? wo : OOB, (s + u) * 32, 0));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b[u].w, acc, 0, 0, 0);
        }
    }
    return acc;
}

// The four partial tiles summed through LDS in the fixed order of waves 0, 1, 2, 3, each sum rounded on its own; the whole
// workgroup calls it (one __syncthreads inside) and wave 0's acc holds the tile afterwards.
__device__ __forceinline__ void dense_tile_sum(f32x16 &acc, float (&part)[3][32 * 32], int wave, int lane) {
    const int l31 = lane & 31;
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) part[wave - 1][dense_tile_row(r, lane) * 32 + l31] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = dense_tile_row(r, lane) * 32 + l31;
            float v = acc[r];
            v = __fadd_rn(v, part[0][at]);
            v = __fadd_rn(v, part[1][at]);
            v = __fadd_rn(v, part[2][at]);
            acc[r] = v;
        }
    }
}

}  // namespace
