// layer.InstanceNormalization (reference layer.py:217-226) on a channel-quad tensor [N][ceil(C/4)][HW][4], IN PLACE, with the
// tail  y = IN(x) [+ res] [relu]  in the write pass.  A "row" is one (image, channel quad): HW float4s, one pixel
// of four channels each.  Every load and store is one float4 per lane; the four components of a lane are four separate
// channels and are reduced side by side, never across -- a NaN in one channel stays in that channel's plane.
//
// Statistics are the reference's centred form.  A workgroup holds a piece of a row in registers (lane t owns pixels t, t + 256,
// ...), sums it, takes the mean, and sums (x - mean)^2 of the same registers: x is read once for both.
//   * rows of up to PL_INSTNORM_Q4_ONE_WG_PIXELS pixels: one workgroup per row owns the whole plane, so that IS mean / variance;
//     it then writes the tail from its registers (instnorm_q4_one_wg_kernel: one read, one write).
//   * longer rows: one workgroup per chunk of PL_INSTNORM_Q4_CHUNK_PIXELS pixels writes (mean, M2) of its chunk
//     (instnorm_q4_stats_kernel); the apply kernel's workgroups each merge their row's partials with Chan's pairwise update,
//     chunk 0, 1, 2, ... in that fixed order -- every workgroup of a row computes the same bits -- and stream the tail over
//     their chunks (two reads, one write).  No atomics anywhere: the result does not change from run to run.
// Which form runs depends on HW alone, so a row's bits do not depend on how many other rows the tensor has.
//
// The closing arithmetic keeps the roundings of the NCHW kernel (head_ops.hip instancenorm_kernel): dev = powf(var + eps, 0.5),
// k = s / dev, off = b - (s * mean) / dev, y = x * k + off -- each operation rounded on its own, no fused multiply-add -- then
// + res, then relu.  The padding lanes of a partial last quad are written as +0.0.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace instnorm_q4 {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int ONE_WG_REGS = PL_INSTNORM_Q4_ONE_WG_PIXELS / TPB;     // float4s a lane holds in the one-workgroup form
constexpr int CHUNK_REGS = PL_INSTNORM_Q4_CHUNK_PIXELS / TPB;       // ... and in the stats kernel
static_assert(PL_INSTNORM_Q4_ONE_WG_PIXELS % TPB == 0 && PL_INSTNORM_Q4_CHUNK_PIXELS % TPB == 0, "whole float4s per lane");
static_assert(PL_INSTNORM_Q4_ONE_WG_PIXELS >= 56 * 56, "the residual stage of a 224 x 224 input takes the one-workgroup form");
constexpr int APPLY_MAX_WG_PER_ROW = 1024;                          // the apply kernel strides over chunks beyond that

__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
__device__ __forceinline__ float4 sub4(float4 a, float4 b) {
    return make_float4(__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w));
}
__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
    return make_float4(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w));
}
__device__ __forceinline__ float4 div4(float4 a, float b) {
    return make_float4(__fdiv_rn(a.x, b), __fdiv_rn(a.y, b), __fdiv_rn(a.z, b), __fdiv_rn(a.w, b));
}

// Sum of one float4 per lane over the workgroup, per component, the same bits in every lane: xor-shuffle tree inside a wave,
// then the waves' totals from LDS in wave order.  `lds` holds WAVES float4s; two barriers, so it can be reused right away.
__device__ __forceinline__ float4 block_sum4(float4 v, float4 *lds) {
    for (int o = 32; o; o >>= 1) {
        v.x = __fadd_rn(v.x, __shfl_xor(v.x, o));
        v.y = __fadd_rn(v.y, __shfl_xor(v.y, o));
        v.z = __fadd_rn(v.z, __shfl_xor(v.z, o));
        v.w = __fadd_rn(v.w, __shfl_xor(v.w, o));
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float4 t = lds[0];
    for (int w = 1; w < WAVES; ++w) t = add4(t, lds[w]);
    __syncthreads();
    return t;
}

// The `cnt` (1 ... R * TPB) pixels at p into registers, their mean and their sum of centred squares M2.
template <int R>
__device__ __forceinline__ void load_and_centre(const float4 *p, int cnt, float4 (&v)[R], float4 &mean, float4 &m2, float4 *lds) {
    float4 s = f4(0.f);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int k = i * TPB + (int)threadIdx.x;
        v[i] = f4(0.f);
        if (k < cnt) {
            v[i] = p[k];
            s = add4(s, v[i]);
        }
    }
    mean = div4(block_sum4(s, lds), (float)cnt);
    float4 q = f4(0.f);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int k = i * TPB + (int)threadIdx.x;
        if (k < cnt) {
            const float4 d = sub4(v[i], mean);
            q = add4(q, mul4(d, d));
        }
    }
    m2 = block_sum4(q, lds);
}

struct Affine {
    float4 k, off;
    unsigned valid;       // bit j: lane component j is a real channel
};

// k = s / dev, off = b - (s * mean) / dev per component of quad `quad`; padding lanes get k = off = 0
__device__ __forceinline__ Affine make_affine(float4 mean, float4 m2, int HW, float eps, const float *s, const float *b, int quad,
                                              int C) {
    const float mv[4] = {mean.x, mean.y, mean.z, mean.w}, qv[4] = {m2.x, m2.y, m2.z, m2.w};
    float kv[4], ov[4];
    Affine a;
    a.valid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = quad * 4 + j;
        kv[j] = ov[j] = 0.f;
        if (c < C) {
            const float dev = powf(__fadd_rn(__fdiv_rn(qv[j], (float)HW), eps), 0.5f);
            const float sc = s[c];
            kv[j] = __fdiv_rn(sc, dev);
            ov[j] = __fsub_rn(b[c], __fdiv_rn(__fmul_rn(sc, mv[j]), dev));
            a.valid |= 1u << j;
        }
    }
    a.k = make_float4(kv[0], kv[1], kv[2], kv[3]);
    a.off = make_float4(ov[0], ov[1], ov[2], ov[3]);
    return a;
}

template <bool RES, bool RELU>
__device__ __forceinline__ float4 tail(float4 x, const Affine &a, float4 r) {
    float4 y = add4(mul4(x, a.k), a.off);
    if (RES) y = add4(y, r);
    if (RELU) y = make_float4(relu_ref(y.x), relu_ref(y.y), relu_ref(y.z), relu_ref(y.w));      // x * (x > 0): NaN stays
    y.x = (a.valid & 1u) ? y.x : 0.f;
    y.y = (a.valid & 2u) ? y.y : 0.f;
    y.z = (a.valid & 4u) ? y.z : 0.f;
    y.w = (a.valid & 8u) ? y.w : 0.f;
    return y;
}

// One workgroup per row (HW <= PL_INSTNORM_Q4_ONE_WG_PIXELS).  grid = rows.
template <bool RES, bool RELU>
__global__ void __launch_bounds__(TPB) instnorm_q4_one_wg_kernel(float4 *x, const float *s, const float *b, const float4 *res,
                                                                int Cq, int C, int HW, float eps) {
    __shared__ float4 lds[WAVES];
    const size_t base = (size_t)blockIdx.x * (size_t)HW;
    float4 v[ONE_WG_REGS], mean, m2;
    load_and_centre<ONE_WG_REGS>(x + base, HW, v, mean, m2, lds);
    const Affine a = make_affine(mean, m2, HW, eps, s, b, (int)(blockIdx.x % (unsigned)Cq), C);
#pragma unroll
    for (int i = 0; i < ONE_WG_REGS; ++i) {
        const int k = i * TPB + (int)threadIdx.x;
        if (k < HW) x[base + k] = tail<RES, RELU>(v[i], a, RES ? res[base + k] : f4(0.f));
    }
}

// Chunk statistics (HW > PL_INSTNORM_Q4_ONE_WG_PIXELS).  grid = rows * S; block r * S + c takes chunk c of row r and writes
// part[2 * (r * S + c)] = mean, part[2 * (r * S + c) + 1] = M2 of its pixels.
__global__ void __launch_bounds__(TPB) instnorm_q4_stats_kernel(const float4 *x, float4 *part, int S, int HW) {
    __shared__ float4 lds[WAVES];
    const unsigned row = blockIdx.x / (unsigned)S, c = blockIdx.x % (unsigned)S;
    const int first = (int)c * PL_INSTNORM_Q4_CHUNK_PIXELS;
    const int cnt = min(PL_INSTNORM_Q4_CHUNK_PIXELS, HW - first);
    float4 v[CHUNK_REGS], mean, m2;
    load_and_centre<CHUNK_REGS>(x + (size_t)row * (size_t)HW + first, cnt, v, mean, m2, lds);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = mean;
        part[2 * (size_t)blockIdx.x + 1] = m2;
    }
}

// Merge + tail.  grid = rows * A, A = min(S, APPLY_MAX_WG_PER_ROW); block r * A + j merges all S partials of row r in chunk
// order (Chan et al.: n = na + nb, d = mb - ma, m = ma + d * nb / n, M2 = M2a + M2b + d^2 * na * nb / n) and rewrites chunks
// j, j + A, ... of that row.
template <bool RES, bool RELU>
__global__ void __launch_bounds__(TPB) instnorm_q4_apply_kernel(float4 *x, const float4 *part, const float *s, const float *b,
                                                               const float4 *res, int Cq, int C, int HW, int S, int A, float eps) {
    const unsigned row = blockIdx.x / (unsigned)A, j = blockIdx.x % (unsigned)A;
    const float4 *pr = part + 2 * (size_t)row * (size_t)S;
    float4 mean = pr[0], m2 = pr[1];
    float na = (float)PL_INSTNORM_Q4_CHUNK_PIXELS;          // S >= 2 here: chunk 0 is full (counts up to 2^29 are exact in float)
    for (int c = 1; c < S; ++c) {
        const float nb = (float)min(PL_INSTNORM_Q4_CHUNK_PIXELS, HW - c * PL_INSTNORM_Q4_CHUNK_PIXELS);
        const float n = na + nb, wb = __fdiv_rn(nb, n), wab = __fmul_rn(na, wb);
        const float4 mb = pr[2 * c], qb = pr[2 * c + 1];
        const float4 d = sub4(mb, mean);
        mean = add4(mean, mul4(d, f4(wb)));
        m2 = add4(add4(m2, qb), mul4(mul4(d, d), f4(wab)));
        na = n;
    }
    const Affine a = make_affine(mean, m2, HW, eps, s, b, (int)(row % (unsigned)Cq), C);
    const size_t base = (size_t)row * (size_t)HW;
    for (int c = (int)j; c < S; c += A) {
        const int first = c * PL_INSTNORM_Q4_CHUNK_PIXELS, cnt = min(PL_INSTNORM_Q4_CHUNK_PIXELS, HW - first);
#pragma unroll
        for (int i = 0; i < CHUNK_REGS; ++i) {
            const int k = i * TPB + (int)threadIdx.x;
            if (k < cnt) {
                const size_t at = base + first + k;
                x[at] = tail<RES, RELU>(x[at], a, RES ? res[at] : f4(0.f));
            }
        }
    }
}

}  // namespace instnorm_q4
