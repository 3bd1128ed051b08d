// The LSTM cell of util.lstm (util.py:109-118) and the fused step kernel of pl_lstm_seq_f32 (head_ops.hip).
// The cell is one __device__ function that lstm_cell_kernel (pl_lstm_cell_f32) and the fused step both call; the fused step's
// h R^T is dense_tile.h's K loop and four-wave sum, the ones dense_small_kernel runs, so a fused step gives the bits of a
// pl_gemm_f32 + pl_lstm_cell_f32 pair wherever that GEMM is dense_small_kernel.
#pragma once
#include "dense_tile.h"

namespace {

// gates = ((x_t W^T + h R^T) + b[:4H]) + b[4H:], split i, o, f, c (ONNX order); sigmoid(i), sigmoid(f), tanh(c);
// C = f*c_prev + i*c; h = sigmoid(o) * tanh(C).  Products and sums are rounded one at a time, as numpy does them.
__device__ __forceinline__ float ref_sigmoid(float v) { return __fdiv_rn(1.f, __fadd_rn(expf(-v), 1.f)); }

// one (row, unit j) of the cell: gx[q] / gh[q] are the two GEMMs' values of gate q at column q*H + j, b the (8H) bias
__device__ __forceinline__ void lstm_cell(const float (&gx)[4], const float (&gh)[4], const float *b, int H, int j, float c_prev,
                                          float &h, float &C) {
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col = q * H + j;
        g[q] = __fadd_rn(__fadd_rn(__fadd_rn(gx[q], gh[q]), b[col]), b[4 * H + col]);
    }
    const float ig = ref_sigmoid(g[0]), fg = ref_sigmoid(g[2]), cg = tanhf(g[3]);
    C = __fadd_rn(__fmul_rn(fg, c_prev), __fmul_rn(ig, cg));
    h = __fmul_rn(ref_sigmoid(g[1]), tanhf(C));
}

struct LstmSeqArgs {
    const float *gx[2];          // per direction slot: (L*N, 4H), every step's x_t W^T
    const float *R, *bias;       // (ndir, 4H, H), (ndir, 8H)
    const float *h0, *c0;        // (ndir, N, H)
    float *Y, *c;                // (L, ndir, N, H); (ndir, N, H) cell state, updated in place
    int L, N, H;
    int step;                    // launch s of L
    int sign0;                   // +1: slot 0 runs forward, -1: reverse; slot 1 is always reverse
};

constexpr int LSTM_GATE_STRIDE = 40;     // LDS row stride of the gate tile in floats (see the exchange below)

// One time step of every direction: grid (H/8, ceil(N/32), ndir), 256 threads.  A workgroup owns 32 batch rows x 8 hidden units,
// i.e. the 32 gate columns q*H + j0 + u of R (tile column 8q + u).  A forward slot handles t = step, a reverse slot
// t = L-1-step; h_prev is Y[t -/+ 1][dir], or h0[dir] at step 0.  The only synchronisation is __syncthreads: the kernel
// boundary orders the steps.
__global__ void __launch_bounds__(256) lstm_step_fused_kernel(LstmSeqArgs p) {
    __shared__ float part[3][32 * 32];
    __shared__ float gates[32 * LSTM_GATE_STRIDE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int N = p.N, H = p.H;
    const int dir = blockIdx.z, ndir = gridDim.z;
    const int sign = dir == 0 ? p.sign0 : -1;
    const int t = sign > 0 ? p.step : p.L - 1 - p.step;
    const size_t NH = (size_t)N * H;
    const float *h_prev = p.step == 0 ? p.h0 + dir * NH : p.Y + ((size_t)(t - sign) * ndir + dir) * NH;
    const float *c_prev = (p.step == 0 ? p.c0 : p.c) + dir * NH;
    const float *bias = p.bias + (size_t)dir * 8 * H;
    const int j0 = blockIdx.x * 8, m0 = blockIdx.y * 32;

    // the cell's own operands first, so that they are in flight under the K loop: thread (row, u) = (tid / 8, tid % 8)
    const int row = threadIdx.x >> 3, u = threadIdx.x & 7;
    const int n = m0 + row, j = j0 + u;
    float gxv[4] = {0.f, 0.f, 0.f, 0.f}, cp = 0.f;
    if (n < N) {                                                        // rows >= N are neither read nor written
        const float *gx = (dir ? p.gx[1] : p.gx[0]) +((size_t)t * N + n) * 4 * H;
#pragma unroll
        for (int q = 0; q < 4; ++q) gxv[q] = gx[q * H + j];
        cp = c_prev[(size_t)n * H + j];
    }

    // gates_h tile = h_prev (N, H) times the 32 rows of R this workgroup owns; N*H*4 and 4H*H*4 are below 2^31 (host check)
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(h_prev), 0, (unsigned)(NH * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.R + (size_t)dir * 4 * H * H), 0,
                                                                       (unsigned)((size_t)4 * H * H * 4), 0x00020000);
    const int wrow = (l31 >> 3) * H + j0 + (l31 & 7);                   // < 4H: H % 8 == 0 and j0 + 7 < H
    const int xo = m0 + l31 < N ? ((m0 + l31) * H + 4 * lhi) << 2 : DENSE_TILE_OOB;
    const int wo = (wrow * H + 4 * lhi) << 2;
    f32x16 acc = dense_tile_kloop(xr, wr, xo, wo, H, wave);
    dense_tile_sum(acc, part, wave, lane);

    // the gate tile through LDS once.  ds_write_b32 / ds_read_b32 bank on (address / 4) % 32 within each 32-lane half: a half
    // writes one row of 32 consecutive floats (no conflict at any stride), and reads 4 rows x 8 units at row*stride + 8q + u,
    // which a stride of 40 = 8 mod 32 spreads over all 32 banks
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) gates[dense_tile_row(r, lane) * LSTM_GATE_STRIDE + l31] = acc[r];
    }
    __syncthreads();
    if (n < N) {
        float ghv[4], h, C;
#pragma unroll
        for (int q = 0; q < 4; ++q) ghv[q] = gates[row * LSTM_GATE_STRIDE + 8 * q + u];
        lstm_cell(gxv, ghv, bias, H, j, cp, h, C);
        p.Y[((size_t)t * ndir + dir) * NH + (size_t)n * H + j] = h;
        p.c[dir * NH + (size_t)n * H + j] = C;                          // in place: this thread alone owns (dir, n, j)
    }
}

}  // namespace
