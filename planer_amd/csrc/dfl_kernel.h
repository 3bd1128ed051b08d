// Anchor-free detection heads and prototype masks: the kernels that stand beside detect_kernel.h's for heads of
// the form (N, 4 R + C + Md, Gh, Gw) -- four box sides as distributions over R bins ("DFL"), C class logits, no objectness
// plane, Md mask coefficients -- and one prototype tensor (N, Md, Ph, Pw).
//
// decode_kernel: one lane per cell, a workgroup takes TPB consecutive cells of one image, so every plane read is coalesced.
// There is no objectness to leave on: every cell walks all C class planes, 16 and then 4 loads in flight, with the label
// kernel's argmax step (the first of equal maxima; a NaN counts as the maximum, the first NaN wins).  score = sigmoid(best); only
// a candidate, score > conf, reads the 4 R bin planes (twice: the maximum, then the sums; the second walk comes from the
// cache), and writes class and box.  Per side, with t_j the R bins:
//     m = fmax_j t_j   e_j = expf(t_j - m)   d = fl(sum_j fl(j e_j)) / fl(sum_j e_j)      (sums in ascending j)
//     x1 = fl(fl(fl(gx + 0.5) - d_l) sx)   y1 likewise (gy, d_t, sy)   x2 = fl(fl(fl(gx + 0.5) + d_r) sx)   y2 likewise
// every operation rounded on its own; not clipped.  The row is stored back to front as in detect_kernel.h.
//
// coefficients_kernel: one lane per (image, det row, coefficient).  rows[n, d] is the position in the image's row that
// nms_kernel kept for det row d, so its anchor index is row - 1 - rows[n, d]; the head that owns that index copies the cell's Md
// coefficient values, and the head at offset 0 writes +0.0 into the rows at or behind num[n].
//
// proto_masks_kernel<KS>: masks[n, d, p] = (d < num[n]) & (pixel p inside det row d's box at prototype scale)
// & (sum_k coef[n, d, k] protos[n, k, p] > 0) as bytes.  A workgroup of four waves owns TILE_PX = 256 consecutive pixels of one
// image's flattened prototype plane and all of the image's det rows; KS = the power of two >= Md / 4 is the number of
// v_mfma_f32_16x16x4_f32 K steps (steps and rows beyond Md and num are zeros in both operands: fl(acc + 0 * 0) = acc).
//   * A (coef, 16 det rows x 4 k per step) goes to LDS once, already in fragment order [row block][step][lane]: a wave reads a
//     step's fragment with one conflict-free 4-byte read per lane.
//   * B (protos): a wave owns 64 pixels as four column groups, and lane l's column in group g is pixel 4 (l % 16) + g -- the
//     groups are INTERLEAVED, so a lane's four B values of one k are one 16-byte load, and its four results of one det row are
//     four adjacent pixels: one 4-byte LDS write.  KS x 4 VGPRs, loaded once per tile.
//   * per 16-row block: KS x 4 MFMAs per wave, crop and sign, bytes into an LDS tile [16][256] (two tiles, used in turn: one
//     barrier per block), then the workgroup stores the tile, 16 bytes per lane, 256 contiguous bytes per det row.
//   * row blocks wholly at or behind num[n] skip LDS and MFMAs and store zeros.
#pragma once
#include "common.h"
#include "detect_kernel.h"
#include "device_utils.h"

namespace dfl {

constexpr int TPB = PL_STREAM_TPB;
constexpr int CLASS_WIDE = 16, CLASS_UNROLL = 4;          // class planes loaded before the first of them is compared: 16s, then 4s
constexpr int MAX_REG = PL_DFL_MAX_REG;
constexpr int MASK_MAX_DET = PL_MASK_MAX_DET;
constexpr int MASK_MAX_COEF = PL_MASK_MAX_COEF;
constexpr int TILE_PX = 256;                              // pixels of a workgroup: 64 per wave
constexpr int ROWS = 16;                                  // det rows of one MFMA row block
static_assert(TPB == 256 && TILE_PX == TPB, "four waves of 64 pixels; one 16-byte store per thread and row block");
static_assert(MASK_MAX_DET % ROWS == 0 && MASK_MAX_COEF % 4 == 0, "whole row blocks and K steps");

// one side's distance in cells from its R bin planes (plane stride HW)
__device__ __forceinline__ float side(const float *b, int R, size_t HW) {
    float m = b[0];
    for (int j = 1; j < R; ++j) m = fmaxf(m, b[(size_t)j * HW]);
    float num = 0.f, den = 0.f;
    for (int j = 0; j < R; ++j) {
        const float e = expf(__fsub_rn(b[(size_t)j * HW], m));
        num = __fadd_rn(num, __fmul_rn((float)j, e));
        den = __fadd_rn(den, e);
    }
    return __fdiv_rn(num, den);
}

// grid = N * tiles; block (n, tile) takes cells [tile * TPB, ...) of image n.  CH = 4 R + C + Md, the head's channels.
__global__ void __launch_bounds__(TPB) decode_kernel(const float *x, float *scores, int *classes, float *boxes, int R, int C,
                                                     size_t CH, int Gw, size_t HW, unsigned tiles, float sx, float sy, float conf,
                                                     size_t row, size_t off) {
    const unsigned tile = blockIdx.x % tiles;
    const size_t n = blockIdx.x / tiles;
    const size_t cell = (size_t)tile * TPB + threadIdx.x;
    if (cell >= HW) return;
    const float *t = x + n * CH * HW + cell;
    const size_t at = n * row + (row - 1 - (off + cell));                     // the row is stored back to front
    const float *cp = t + (size_t)(4 * R) * HW;
    float best = cp[0];
    int cls = 0, c = 1;
    for (; c + CLASS_WIDE <= C; c += CLASS_WIDE) {
        float v[CLASS_WIDE];
#pragma unroll
        for (int u = 0; u < CLASS_WIDE; ++u) v[u] = cp[(size_t)(c + u) * HW];
#pragma unroll
        for (int u = 0; u < CLASS_WIDE; ++u) {
            const bool take = v[u] > best || (v[u] != v[u] && best == best);
            best = take ? v[u] : best;
            cls = take ? c + u : cls;
        }
    }
    for (; c + CLASS_UNROLL <= C; c += CLASS_UNROLL) {
        float v[CLASS_UNROLL];
#pragma unroll
        for (int u = 0; u < CLASS_UNROLL; ++u) v[u] = cp[(size_t)(c + u) * HW];
#pragma unroll
        for (int u = 0; u < CLASS_UNROLL; ++u) {
            const bool take = v[u] > best || (v[u] != v[u] && best == best);
            best = take ? v[u] : best;
            cls = take ? c + u : cls;
        }
    }
    for (; c < C; ++c) {
        const float v = cp[(size_t)c * HW];
        const bool take = v > best || (v != v && best == best);
        best = take ? v : best;
        cls = take ? c : cls;
    }
    const float score = detect::sigmoid(best);
    if (!(score > conf)) {
        scores[at] = -1.f;
        return;
    }
    const size_t RHW = (size_t)R * HW;
    const float dl = side(t, R, HW), dt = side(t + RHW, R, HW), dr = side(t + 2 * RHW, R, HW), db = side(t + 3 * RHW, R, HW);
    const unsigned gy = (unsigned)(cell / (unsigned)Gw), gx = (unsigned)(cell - (size_t)gy * (unsigned)Gw);
    const float cx = __fadd_rn((float)gx, 0.5f), cy = __fadd_rn((float)gy, 0.5f);
    scores[at] = score;
    classes[at] = cls;
    float *b = boxes + at * 4;
    b[0] = __fmul_rn(__fsub_rn(cx, dl), sx);
    b[1] = __fmul_rn(__fsub_rn(cy, dt), sy);
    b[2] = __fmul_rn(__fadd_rn(cx, dr), sx);
    b[3] = __fmul_rn(__fadd_rn(cy, db), sy);
}

// grid = ceil(N max_det Md / TPB).  x is one head; first = 4 R + C, where its coefficient planes start.
__global__ void __launch_bounds__(TPB) coefficients_kernel(const float *x, const int *rows, const int *num, float *coef, size_t total,
                                                           int max_det, int Md, size_t CH, size_t first, size_t HW, long long row,
                                                           long long off) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % (unsigned)Md);
    const size_t nd = i / (unsigned)Md, n = nd / (unsigned)max_det;
    const int d = (int)(nd - n * (unsigned)max_det);
    if (d >= num[n]) {
        if (off == 0) coef[i] = 0.f;
        return;
    }
    const long long cell = row - 1 - (long long)rows[nd] - off;              // (a row outside [0, row) names no cell of any head)
    if (cell < 0 || cell >= (long long)HW || rows[nd] < 0) return;
    coef[i] = x[(n * CH + first + (size_t)k) * HW + (size_t)cell];
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// grid = N * tiles, tiles = ceil(P / TILE_PX), P = Ph Pw.  vin: protos 16-byte aligned and P % 4 == 0; vout: masks 16-byte
// aligned and P % 16 == 0 (then every 16-byte piece of a det row lies wholly inside or outside the plane).
template <int KS>
__global__ void __launch_bounds__(TPB) proto_masks_kernel(const float *det, const int *num, const float *coef, const float *protos,
                                                          int max_det, int Md, unsigned Pw, unsigned P, unsigned tiles, float kx,
                                                          float ky, bool vin, bool vout, unsigned char *masks) {
    __shared__ float a_lds[(MASK_MAX_DET / ROWS) * KS * 64];                  // [row block][step][lane]
    __shared__ float4 box_lds[MASK_MAX_DET];                                  // a det row's box at prototype scale
    __shared__ __attribute__((aligned(16))) unsigned tile_lds[2][ROWS][TILE_PX / 4];
    const unsigned tile = blockIdx.x % tiles;
    const size_t n = blockIdx.x / tiles;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 15, quad = lane >> 4;
    const int nn = min(max(num[n], 0), max_det);
    const int blocks = (max_det + ROWS - 1) / ROWS, live = (nn + ROWS - 1) / ROWS;

    for (int i = t; i < live * KS * 64; i += TPB) {
        const int l = i & 63, s = (i >> 6) % KS, rb = (i >> 6) / KS;
        const int d = rb * ROWS + (l & 15), k = 4 * s + (l >> 4);
        a_lds[i] = d < nn && k < Md ? coef[(n * (size_t)max_det + (size_t)d) * (size_t)Md + (size_t)k] : 0.f;
    }
    for (int d = t; d < live * ROWS; d += TPB) {
        float4 b = make_float4(INFINITY, INFINITY, 0.f, 0.f);                 // at or behind num: no pixel is inside
        if (d < nn) {
            const float *r = det + (n * (size_t)max_det + (size_t)d) * 6;
            b = make_float4(__fmul_rn(r[0], kx), __fmul_rn(r[1], ky), __fmul_rn(r[2], kx), __fmul_rn(r[3], ky));
        }
        box_lds[d] = b;
    }

    // the lane's four pixels p .. p + 3 (p % 4 == 0): column `col` of the wave's four interleaved column groups
    const unsigned p = tile * TILE_PX + (unsigned)wave * 64 + 4 * (unsigned)col;
    float b[KS][4], fx[4], fy[4];
    const float *pp = protos + n * (size_t)Md * P + p;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k = 4 * s + quad;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live > 0 && k < Md) {
            const float *q = pp + (size_t)k * P;
            if (vin) {
                if (p < P) v = *reinterpret_cast<const float4 *>(q);
            } else {
                v.x = p < P ? q[0] : 0.f;
                v.y = p + 1 < P ? q[1] : 0.f;
                v.z = p + 2 < P ? q[2] : 0.f;
                v.w = p + 3 < P ? q[3] : 0.f;
            }
        }
        b[s][0] = v.x, b[s][1] = v.y, b[s][2] = v.z, b[s][3] = v.w;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const unsigned y = (p + g) / Pw;
        fy[g] = (float)y, fx[g] = (float)(p + g - y * Pw);
    }
    __syncthreads();

    const int srow = t >> 4;                                                  // the store: thread t owns 16 bytes of row t / 16
    const unsigned sp = tile * TILE_PX + 16 * (unsigned)(t & 15);
    unsigned char *out = masks + n * (size_t)max_det * P;
    for (int rb = 0; rb < blocks; ++rb) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (rb < live) {                                                      // (uniform: num[n] is the workgroup's)
            f32x4 acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float a = a_lds[(rb * KS + s) * 64 + lane];
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[s][g], acc[g], 0, 0, 0);
            }
            // the accumulator's register r of lane (quad, col) is det row 4 quad + r of the block, column col
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 bx = box_lds[rb * ROWS + 4 * quad + r];
                unsigned word = 0u;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const bool on = acc[g][r] > 0.f && bx.x <= fx[g] && fx[g] < bx.z && bx.y <= fy[g] && fy[g] < bx.w;
                    word |= (on ? 1u : 0u) << (8 * g);
                }
                tile_lds[rb & 1][4 * quad + r][wave * 16 + col] = word;
            }
            __syncthreads();
            v = *reinterpret_cast<const uint4 *>(&tile_lds[rb & 1][srow][4 * (t & 15)]);
        }
        const int d = rb * ROWS + srow;
        if (d >= max_det || sp >= P) continue;
        unsigned char *o = out + (size_t)d * P + sp;
        if (vout) {
            *reinterpret_cast<uint4 *>(o) = v;
        } else {
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (sp + j < P) o[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

}  // namespace dfl
