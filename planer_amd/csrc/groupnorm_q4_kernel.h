// Group normalisation on a channel-quad tensor [N][ceil(C/4)][HW][4], IN PLACE, as the five steps an exporter writes for it --
// reshape (N, G, -1), InstanceNormalization with G scales / biases, reshape back, mul by gamma (C), add beta (C) -- with the tail
//   y = IN_g(x) [* gamma_c] [+ beta_c] [+ res] [relu]   in the write pass.
// The helpers are instnorm_q4_kernel.h's; what differs is which lanes of a float4 share their statistics.  LANES is that number:
//   * 4, "wide" (cpg = C / G a multiple of 4): a group is cpg / 4 consecutive quad planes, ONE contiguous run of L = cpg / 4 * HW
//     float4s whose four lanes all belong to it.  A "row" is that run; the float4 at position k of it lies in quad k / HW of the
//     group and takes that quad's four gamma / beta values (a chunk may straddle two planes).
//   * 2, "pair" (cpg == 2): a row is one (image, quad) plane; lanes (x, y) are one group, lanes (z, w) the next.  C is even, so
//     a partial last quad has one real pair and one padding pair.
//   * 1, "single" (cpg == 1): every lane its own group, the instance norm's geometry with the longer tail.
// The per-lane sums of a workgroup are folded across the lanes of a group (fold<LANES>) before the mean is taken, so a NaN stays
// inside its group.  Statistics are centred: the group's mean, then the sum of (x - mean)^2 over the same registers.
// Rows of up to PL_INSTNORM_Q4_ONE_WG_PIXELS float4s are held by one workgroup (one read, one write); longer ones get (mean, M2)
// per chunk of PL_INSTNORM_Q4_CHUNK_PIXELS float4s, merged by every workgroup of the apply kernel in chunk order (Chan's update).
// No atomics; the form depends on cpg and HW alone.  Every operation of the closing arithmetic is rounded on its own:
//   dev = powf(var + eps, 0.5), k = s_g / dev, off = b_g - (s_g * mean) / dev, y = x * k + off, y * gamma_c, + beta_c, + res, relu.
// Padding lanes of a partial last quad are written as +0.0.
#pragma once
#include "instnorm_q4_kernel.h"

namespace groupnorm_q4 {

using instnorm_q4::add4;
using instnorm_q4::Affine;
using instnorm_q4::APPLY_MAX_WG_PER_ROW;
using instnorm_q4::block_sum4;
using instnorm_q4::CHUNK_REGS;
using instnorm_q4::div4;
using instnorm_q4::f4;
using instnorm_q4::mul4;
using instnorm_q4::ONE_WG_REGS;
using instnorm_q4::sub4;
using instnorm_q4::TPB;
using instnorm_q4::WAVES;

// The four per-lane totals of a workgroup -> per-group totals, every lane of a group holding its group's.
template <int LANES>
__device__ __forceinline__ float4 fold(float4 t) {
    if (LANES == 4) return f4(__fadd_rn(__fadd_rn(t.x, t.y), __fadd_rn(t.z, t.w)));
    if (LANES == 2) {
        const float a = __fadd_rn(t.x, t.y), b = __fadd_rn(t.z, t.w);
        return make_float4(a, a, b, b);
    }
    return t;
}

// The `cnt` (1 ... R * TPB) float4s at p into registers; per lane its group's mean over the cnt * LANES values and their M2.
template <int R, int LANES>
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
    mean = div4(fold<LANES>(block_sum4(s, lds)), (float)(cnt * LANES));
    float4 q = f4(0.f);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int k = i * TPB + (int)threadIdx.x;
        if (k < cnt) {
            const float4 d = sub4(v[i], mean);
            q = add4(q, mul4(d, d));
        }
    }
    m2 = fold<LANES>(block_sum4(q, lds));
}

// What a row needs besides its statistics.  quad0: the row's first channel quad; r: the row's index inside its image.
struct Row {
    size_t base;
    int quad0;
};
template <int LANES>
__device__ __forceinline__ Row row_of(unsigned row, int rows_per_image, int cpg, int L) {
    const int r = (int)(row % (unsigned)rows_per_image);
    return {(size_t)row * (size_t)L, LANES == 4 ? r * (cpg / 4) : r};
}

// k = s_g / dev, off = b_g - (s_g * mean) / dev per lane, g = channel / cpg; padding lanes get k = off = 0.  n: values per group.
__device__ __forceinline__ Affine make_affine(float4 mean, float4 m2, float n, float eps, const float *gs, const float *gb, int quad0,
                                              int C, int cpg) {
    const float mv[4] = {mean.x, mean.y, mean.z, mean.w}, qv[4] = {m2.x, m2.y, m2.z, m2.w};
    float kv[4], ov[4];
    Affine a;
    a.valid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = quad0 * 4 + j;
        kv[j] = ov[j] = 0.f;
        if (c < C) {
            const int g = c / cpg;
            const float dev = powf(__fadd_rn(__fdiv_rn(qv[j], n), eps), 0.5f);
            const float sc = gs[g];
            kv[j] = __fdiv_rn(sc, dev);
            ov[j] = __fsub_rn(gb[g], __fdiv_rn(__fmul_rn(sc, mv[j]), dev));
            a.valid |= 1u << j;
        }
    }
    a.k = make_float4(kv[0], kv[1], kv[2], kv[3]);
    a.off = make_float4(ov[0], ov[1], ov[2], ov[3]);
    return a;
}

// The four per-channel values of quad `quad` (0 past C; `p` may be null: never read then)
__device__ __forceinline__ float4 quad_values(const float *p, int quad, int C) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (p) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (quad * 4 + j < C) v[j] = p[quad * 4 + j];
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

template <bool RES, bool RELU>
__device__ __forceinline__ float4 tail(float4 x, const Affine &a, bool has_gamma, float4 gam, bool has_beta, float4 bet, float4 r) {
    float4 y = add4(mul4(x, a.k), a.off);
    if (has_gamma) y = mul4(y, gam);
    if (has_beta) y = add4(y, bet);
    if (RES) y = add4(y, r);
    if (RELU) y = make_float4(relu_ref(y.x), relu_ref(y.y), relu_ref(y.z), relu_ref(y.w));      // x * (x > 0): NaN stays
    y.x = (a.valid & 1u) ? y.x : 0.f;
    y.y = (a.valid & 2u) ? y.y : 0.f;
    y.z = (a.valid & 4u) ? y.z : 0.f;
    y.w = (a.valid & 8u) ? y.w : 0.f;
    return y;
}

// One workgroup per row (L <= PL_INSTNORM_Q4_ONE_WG_PIXELS).  grid = rows; rows_per_image = G (wide) or ceil(C / 4).
template <int LANES, bool RES, bool RELU>
__global__ void __launch_bounds__(TPB) groupnorm_q4_one_wg_kernel(float4 *x, const float *gs, const float *gb, const float *gamma,
                                                                 const float *beta, const float4 *res, int rows_per_image, int C,
                                                                 int cpg, int L, FastDiv divHW, float eps) {
    __shared__ float4 lds[WAVES];
    const Row rw = row_of<LANES>(blockIdx.x, rows_per_image, cpg, L);
    float4 v[ONE_WG_REGS], mean, m2;
    load_and_centre<ONE_WG_REGS, LANES>(x + rw.base, L, v, mean, m2, lds);
    const Affine a = make_affine(mean, m2, __fmul_rn((float)L, (float)LANES), eps, gs, gb, rw.quad0, C, cpg);
    float4 gam = quad_values(gamma, rw.quad0, C), bet = quad_values(beta, rw.quad0, C);
#pragma unroll
    for (int i = 0; i < ONE_WG_REGS; ++i) {
        const int k = i * TPB + (int)threadIdx.x;
        if (k < L) {
            if (LANES == 4) {
                const int quad = rw.quad0 + (int)divHW.div((unsigned)k);
                gam = quad_values(gamma, quad, C);
                bet = quad_values(beta, quad, C);
            }
            x[rw.base + k] = tail<RES, RELU>(v[i], a, gamma != nullptr, gam, beta != nullptr, bet, RES ? res[rw.base + k] : f4(0.f));
        }
    }
}

// Chunk statistics (L > PL_INSTNORM_Q4_ONE_WG_PIXELS).  grid = rows * S; block r * S + c takes chunk c of row r and writes
// part[2 * (r * S + c)] = mean, part[2 * (r * S + c) + 1] = M2 of its values, per lane its group's.
template <int LANES>
__global__ void __launch_bounds__(TPB) groupnorm_q4_stats_kernel(const float4 *x, float4 *part, int S, int L) {
    __shared__ float4 lds[WAVES];
    const unsigned row = blockIdx.x / (unsigned)S, c = blockIdx.x % (unsigned)S;
    const int first = (int)c * PL_INSTNORM_Q4_CHUNK_PIXELS;
    const int cnt = min(PL_INSTNORM_Q4_CHUNK_PIXELS, L - first);
    float4 v[CHUNK_REGS], mean, m2;
    load_and_centre<CHUNK_REGS, LANES>(x + (size_t)row * (size_t)L + first, cnt, v, mean, m2, lds);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = mean;
        part[2 * (size_t)blockIdx.x + 1] = m2;
    }
}

// Merge + tail.  grid = rows * A, A = min(S, APPLY_MAX_WG_PER_ROW); block r * A + j merges all S partials of row r in chunk
// order (n = na + nb, d = mb - ma, m = ma + d * nb / n, M2 = M2a + M2b + d^2 * na * nb / n; counts in values, LANES per float4)
// and rewrites chunks j, j + A, ... of that row.
template <int LANES, bool RES, bool RELU>
__global__ void __launch_bounds__(TPB) groupnorm_q4_apply_kernel(float4 *x, const float4 *part, const float *gs, const float *gb,
                                                                const float *gamma, const float *beta, const float4 *res,
                                                                int rows_per_image, int C, int cpg, int L, FastDiv divHW, int S, int A,
                                                                float eps) {
    const unsigned row = blockIdx.x / (unsigned)A, j = blockIdx.x % (unsigned)A;
    const float4 *pr = part + 2 * (size_t)row * (size_t)S;
    float4 mean = pr[0], m2 = pr[1];
    float na = (float)(PL_INSTNORM_Q4_CHUNK_PIXELS * LANES);          // S >= 2 here: chunk 0 is full
    for (int c = 1; c < S; ++c) {
        const float nb = (float)(min(PL_INSTNORM_Q4_CHUNK_PIXELS, L - c * PL_INSTNORM_Q4_CHUNK_PIXELS) * LANES);
        const float n = na + nb, wb = __fdiv_rn(nb, n), wab = __fmul_rn(na, wb);
        const float4 mb = pr[2 * c], qb = pr[2 * c + 1];
        const float4 d = sub4(mb, mean);
        mean = add4(mean, mul4(d, f4(wb)));
        m2 = add4(add4(m2, qb), mul4(mul4(d, d), f4(wab)));
        na = n;
    }
    const Row rw = row_of<LANES>(row, rows_per_image, cpg, L);
    const Affine a = make_affine(mean, m2, __fmul_rn((float)L, (float)LANES), eps, gs, gb, rw.quad0, C, cpg);
    float4 gam = quad_values(gamma, rw.quad0, C), bet = quad_values(beta, rw.quad0, C);
    for (int c = (int)j; c < S; c += A) {
        const int first = c * PL_INSTNORM_Q4_CHUNK_PIXELS, cnt = min(PL_INSTNORM_Q4_CHUNK_PIXELS, L - first);
#pragma unroll
        for (int i = 0; i < CHUNK_REGS; ++i) {
            const int k = i * TPB + (int)threadIdx.x;
            if (k < cnt) {
                if (LANES == 4) {                           // the chunk may straddle two planes of the group
                    const int quad = rw.quad0 + (int)divHW.div((unsigned)(first + k));
                    gam = quad_values(gamma, quad, C);
                    bet = quad_values(beta, quad, C);
                }
                const size_t at = rw.base + first + k;
                x[at] = tail<RES, RELU>(x[at], a, gamma != nullptr, gam, beta != nullptr, bet, RES ? res[at] : f4(0.f));
            }
        }
    }
}

}  // namespace groupnorm_q4
