// Text as net output: greedy CTC decoding of a float32 sequence tensor.  Two launches: a FRAME pass that reduces
// every frame's C classes to a label (numpy's argmax) and a confidence, and a COLLAPSE pass, one workgroup per sequence, that
// merges repeats, drops blanks and writes the symbols.  The kernel boundary is the only synchronisation between workgroups,
// there is no global atomic, and everything but the softmax confidence is exact and unique.
//
// A frame's classes travel as a PARTIAL (v, i, s): v the maximum so far by numpy's rule, i its class (NONE: nothing taken yet),
// s = sum of exp(x_c - v) over the classes seen (softmax confidence only).
//   step    one more class, its index above every index the partial has seen: taken iff x > v, or x is the first NaN.  A taken
//           class rescales the sum, s = s exp(v - x) + 1; another adds exp(x - v).  exp's argument is NaN only where both values
//           are the same infinity (or one is NaN); the term is then 0, and such frames end with a NaN confidence anyway.
//   merge   two partials over disjoint classes: the NaN wins over the number, the greater number over the smaller, the lower
//           index between equal values and between two NaNs; s = s_winner + s_loser exp(v_loser - v_winner).  It is symmetric, so
//           both lanes of a butterfly pair compute the same bits.
// A partial starts as (-inf, NONE, 0); a frame whose classes are all -inf ends with i == NONE, which is class 0.
//
// frame pass, class-contiguous (st_class == 1: tnc, ntc), a row of C floats per frame:
//   the row is cut into a head of 0..3 floats up to the first 16-byte boundary, 16-byte vectors, and a tail of 0..3 floats.  Of
//   the G lanes that share a row, lane j steps head float j, then vectors j, j + G, ... (four loads in flight, the four floats of
//   a vector in order), then tail float j: a lane's indices only grow.  The lanes merge over a wave64 butterfly (32, 16, .. 1
//   apart), and where a workgroup shares the row (G = 256) wave 0's lane 0 folds the four waves' partials in wave order.
//   rows_wave_kernel   C <= ROW_WAVE_MAX: one wave per row, four rows per workgroup.
//   rows_block_kernel  above it: one workgroup per row.
// frame pass, class-strided (st_class != 1: nchw), frames adjacent in memory:
//   time_kernel  a workgroup of TIME_TPB = 1024 threads takes TIME_LANES consecutive frames of one sequence; lane l of class
//                group g (TIME_GROUPS of them, half a wave each, so a load is one 128-byte line where st_time == 1) steps classes
//                [g q, (g + 1) q) of frame l in order, q = ceil(C / TIME_GROUPS), eight loads in flight; the partials go to LDS
//                and group 0's lanes fold the groups in order.  A group past the last class hands on the start partial.  (With
//                a workgroup of 256 threads and 8 groups the pass took 152 us on (32, 6625, 1, 80): the grid is only
//                S ceil(T / 32) workgroups, so the classes' parallelism has to come from inside the workgroup.)
// A frame at or past its sequence's valid length is neither read nor written.
// collapse_kernel  one workgroup per sequence walks the frames in chunks of PL_TEXT_CHUNK, a frame per thread.  A frame reads
//                  its neighbours' labels from the frame pass's scratch, so nothing about the previous label or an open run has
//                  to cross a chunk boundary: it STARTS a symbol (label != blank and, when merging, differs from the frame in
//                  front) or ENDS one (label != blank and, when merging, differs from the frame behind, or is the last valid
//                  frame), and since runs do not overlap the end belongs to the latest start at or in front of it.  The symbol
//                  number is the inclusive scan of the start flags (wave scan, four wave totals through LDS) plus the carry of
//                  the chunks in front.  Then the count and the filler rows.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace text {

constexpr int TPB = PL_STREAM_TPB;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = PL_TEXT_CHUNK;
constexpr int ROW_WAVE_MAX = PL_TEXT_ROW_WAVE_MAX;
constexpr int TIME_LANES = PL_TEXT_TIME_LANES, TIME_GROUPS = PL_TEXT_TIME_GROUPS, TIME_TPB = TIME_LANES * TIME_GROUPS;
constexpr int NONE = 0x7fffffff;
static_assert(TPB == 256 && CHUNK == TPB, "a chunk is a frame per thread; four waves per workgroup");
static_assert(TIME_LANES == 32 && TIME_TPB == 1024, "a class group is half a wave; the largest workgroup");

// where the frames are: element (so, si, t, c) of x at so * st_outer + si * st_inner + t * st_time + c * st_class
struct Geo {
    int S_inner, T, C;
    long long st_outer, st_inner, st_time, st_class;
};

struct Partial {
    float v;
    int i;
    float s;
};

__device__ __forceinline__ Partial start_partial() { return Partial{-__builtin_huge_valf(), NONE, 0.f}; }

__device__ __forceinline__ float exp_or_zero(float d) { return d == d ? expf(d) : 0.f; }

template <bool SUM> __device__ __forceinline__ void step(Partial &p, float x, int c) {
    const bool take = x > p.v || (x != x && p.v == p.v);
    if (SUM) {
        const float e = exp_or_zero(take ? __fsub_rn(p.v, x) : __fsub_rn(x, p.v));
        p.s = take ? __fadd_rn(__fmul_rn(p.s, e), 1.f) : __fadd_rn(p.s, e);
    }
    p.v = take ? x : p.v;
    p.i = take ? c : p.i;
}

// a beats b: the NaN over the number, the greater number, the lower index between equals
__device__ __forceinline__ bool beats(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

template <bool SUM> __device__ __forceinline__ Partial merge(const Partial &a, const Partial &b) {
    const bool first = beats(a.v, a.i, b.v, b.i);
    const Partial w = first ? a : b, l = first ? b : a;
    Partial r = w;
    if (SUM) r.s = __fadd_rn(w.s, __fmul_rn(l.s, exp_or_zero(__fsub_rn(l.v, w.v))));
    return r;
}

// every lane of the wave64 leaves with the merge of all 64 partials
template <bool SUM> __device__ __forceinline__ Partial wave_merge(Partial p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Partial q;
        q.v = __shfl_xor(p.v, o);
        q.i = __shfl_xor(p.i, o);
        q.s = SUM ? __shfl_xor(p.s, o) : 0.f;
        p = merge<SUM>(p, q);
    }
    return p;
}

// mode: PL_TEXT_CONF_*.  The frame's label and confidence go to scratch.
__device__ __forceinline__ void put_frame(const Partial &p, int mode, size_t f, int *labels, float *confs) {
    labels[f] = p.i == NONE ? 0 : p.i;
    if (mode == PL_TEXT_CONF_SOFTMAX)
        confs[f] = (p.v - p.v == 0.f) ? __fdiv_rn(1.f, p.s) : __builtin_nanf("");        // (v - v: 0 iff v is finite)
    else if (mode == PL_TEXT_CONF_VALUE)
        confs[f] = p.v;
}

__device__ __forceinline__ bool frame_row(const Geo &g, const int *lengths, size_t f, const float *x, const float *&row) {
    const size_t s = f / (size_t)g.T;
    const int t = (int)(f - s * g.T);
    if (lengths && t >= lengths[s]) return false;
    const size_t so = s / (size_t)g.S_inner, si = s - so * g.S_inner;
    row = x + (long long)so * g.st_outer + (long long)si * g.st_inner + (long long)t * g.st_time;
    return true;
}

// lane `l` of the `G` that share `row` steps its part of the row's C floats (see the head of this file)
template <bool SUM, int G> __device__ __forceinline__ Partial row_partial(const float *row, int C, int l) {
    Partial p = start_partial();
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int head = min((4 - mis) & 3, C), nvec = (C - head) >> 2, tail0 = head + 4 * nvec;
    if (l < head) step<SUM>(p, row[l], l);
    const float4 *vec = reinterpret_cast<const float4 *>(row + head);
    for (int i = l; i < nvec; i += 4 * G) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * G < nvec) v[u] = vec[i + u * G];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * G < nvec) {
                const int c = head + 4 * (i + u * G);
                step<SUM>(p, v[u].x, c);
                step<SUM>(p, v[u].y, c + 1);
                step<SUM>(p, v[u].z, c + 2);
                step<SUM>(p, v[u].w, c + 3);
            }
    }
    if (tail0 + l < C) step<SUM>(p, row[tail0 + l], tail0 + l);
    return p;
}

// grid = ceil(frames / WAVES): wave w of block b takes frame b WAVES + w
template <bool SUM>
__global__ void __launch_bounds__(TPB) rows_wave_kernel(const float *x, Geo g, size_t frames, const int *lengths, int mode, int *labels, float *confs) {
    const size_t f = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const float *row;
    if (f >= frames || !frame_row(g, lengths, f, x, row)) return;                          // (wave-uniform)
    const Partial p = wave_merge<SUM>(row_partial<SUM, 64>(row, g.C, threadIdx.x & 63));
    if ((threadIdx.x & 63) == 0) put_frame(p, mode, f, labels, confs);
}

// grid = frames
template <bool SUM>
__global__ void __launch_bounds__(TPB) rows_block_kernel(const float *x, Geo g, const int *lengths, int mode, int *labels, float *confs) {
    __shared__ Partial part[WAVES];
    const size_t f = blockIdx.x;
    const float *row;
    if (!frame_row(g, lengths, f, x, row)) return;                                        // (block-uniform)
    const Partial p = wave_merge<SUM>(row_partial<SUM, TPB>(row, g.C, threadIdx.x));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial r = part[0];
        for (int w = 1; w < WAVES; ++w) r = merge<SUM>(r, part[w]);
        put_frame(r, mode, f, labels, confs);
    }
}

// grid = S * ceil(T / TIME_LANES)
template <bool SUM>
__global__ void __launch_bounds__(TIME_TPB) time_kernel(const float *x, Geo g, unsigned spans_t, const int *lengths, int mode, int *labels, float *confs) {
    __shared__ Partial part[TIME_GROUPS][TIME_LANES];
    const int l = threadIdx.x % TIME_LANES, grp = threadIdx.x / TIME_LANES;
    const size_t s = blockIdx.x / spans_t;
    const int t = (int)(blockIdx.x % spans_t) * TIME_LANES + l;
    const int len = lengths ? min(lengths[s], g.T) : g.T;
    const bool live = t < len;
    Partial p = start_partial();
    if (live) {
        const size_t so = s / (size_t)g.S_inner, si = s - so * g.S_inner;
        const float *col = x + (long long)so * g.st_outer + (long long)si * g.st_inner + (long long)t * g.st_time;
        const int q = (g.C + TIME_GROUPS - 1) / TIME_GROUPS;
        const int c0 = min(grp * q, g.C), c1 = min(c0 + q, g.C);
        for (int c = c0; c < c1; c += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c + u < c1) v[u] = col[(long long)(c + u) * g.st_class];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c + u < c1) step<SUM>(p, v[u], c + u);
        }
    }
    part[grp][l] = p;
    __syncthreads();
    if (grp == 0 && live) {
        Partial r = part[0][l];
        for (int k = 1; k < TIME_GROUPS; ++k) r = merge<SUM>(r, part[k][l]);
        put_frame(r, mode, s * (size_t)g.T + t, labels, confs);
    }
}

// grid = S.  labels, confs: the frame pass's (S, T) scratch; conf mode PL_TEXT_CONF_NONE reads no confs.
__global__ void __launch_bounds__(TPB) collapse_kernel(const int *labels, const float *confs, int T, const int *lengths, int blank, int merge_repeated,
                                                        int mode, int max_len, int *text, int *length, float *conf, int *spans) {
    __shared__ int wave_total[WAVES];
    const size_t s = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int len = lengths ? min(max(lengths[s], 0), T) : T;
    const int *lab = labels + s * (size_t)T;
    const float *cf = confs + s * (size_t)T;
    int *text_s = text + s * (size_t)max_len, *spans_s = spans + s * (size_t)max_len * 2;
    float *conf_s = conf + s * (size_t)max_len;
    int carry = 0;                                          // symbols started in the chunks in front (the same in every thread)
    for (int base = 0; base < len; base += CHUNK) {
        const int f = base + t;
        int mine = blank, start = 0, end = 0;
        if (f < len) {
            mine = lab[f];
            if (mine != blank) {
                start = !merge_repeated || f == 0 || lab[f - 1] != mine;
                end = !merge_repeated || f + 1 == len || lab[f + 1] != mine;
            }
        }
        const int inc = wave_inclusive_sum(start, lane);
        if (lane == 63) wave_total[wave] = inc;
        __syncthreads();
        int front = carry, all = carry;
        for (int w = 0; w < WAVES; ++w) {
            front += w < wave ? wave_total[w] : 0;
            all += wave_total[w];
        }
        const int k = front + inc - 1;                      // the symbol this frame starts or ends
        if (start && k < max_len) {
            text_s[k] = mine;
            conf_s[k] = mode == PL_TEXT_CONF_NONE ? 0.f : cf[f];
            spans_s[2 * k] = f;
        }
        if (end && k < max_len) spans_s[2 * k + 1] = f + 1;
        carry = all;
        __syncthreads();                                    // (wave_total is rewritten by the next chunk)
    }
    if (t == 0) length[s] = carry;
    for (int k = min(carry, max_len) + t; k < max_len; k += TPB) {
        text_s[k] = -1;
        conf_s[k] = 0.f;
        spans_s[2 * k] = 0;
        spans_s[2 * k + 1] = 0;
    }
}

}  // namespace text
