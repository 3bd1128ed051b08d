// Top-k by exact radix selection: pl_topk_select_f32, the k greatest of a row in pl_topk_f32's order (largest = 1)
// without sorting the row.  A float becomes a 32-bit KEY that is monotone in topk_before's order -- NaN 0xFFFFFFFF, -0 as +0,
// otherwise ~bits where the sign is set and bits | 0x80000000 where it is clear -- and key << 32 | index is a total order: the
// answer is the k greatest composites, descending.  A row is cut into chunks of CHUNK elements, one workgroup per chunk, and the
// launches of one call are
//   clear_kernel      zeroes the rows' histograms and candidate counters (the scratch's contents are irrelevant on entry)
//   hist_kernel<1>    counts the chunk's keys by their top 11 bits in LDS and adds the non-empty bins to the row's histogram
//   hist_kernel<2>    the next 11 bits of the keys whose top 11 equal the digit the cut falls in
//   hist_kernel<3>    the last 10 bits of the keys whose top 22 equal the two digits found
//   gather_kernel     keys above the threshold T go to the row's candidate buffer as composites, in any order; the chunk's
//                     count of keys equal to T goes to the row's tie table
//   finish_kernel     one workgroup per row sorts the c < k candidates in LDS and writes them, then fills the remaining r = k - c
//                     places with elements equal to T by descending index
// No launch has a separate "find the digit" step: find_digit is the prologue of every workgroup that needs it.  It walks the
// previous level's histogram of the row from the top bin down, a run of bins per thread and a workgroup scan over the runs'
// sums, to the bin d with above(d) < need <= above(d) + h[d], and hands need - above(d) to the next level.  After three levels
// T is exact, c = k - r keys are greater and 1 <= r <= (keys equal to T).  The histograms are integer sums, so what a workgroup
// reads does not depend on the order the atomics arrived in; the candidates' order does, and the sort removes it.  No workgroup
// waits for another inside a launch: stream order between the six launches is the only synchronisation, whatever the data.
//
// The equal keys are the case that decides the cost for detection rows (thousands of scores of -1): in the histograms a wave
// whose active lanes all hold one digit adds its population with ONE LDS atomic, and the finish pass never sorts ties -- they
// share a key, so descending index is the order of a walk from the row's end over the chunks whose tie count is not zero.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace topk_select {

constexpr int TPB = PL_STREAM_TPB;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = PL_TOPK_SELECT_CHUNK;
constexpr int MAX_K = PL_TOPK_SELECT_MAX_K;
constexpr int BINS1 = 2048, BINS2 = 2048, BINS3 = 1024;      // 11 + 11 + 10 bits
constexpr int HIST_WORDS = BINS1 + BINS2 + BINS3;
static_assert(HIST_WORDS == PL_TOPK_SELECT_HIST_WORDS, "include/planer_hip.h states the scratch size");
static_assert(TPB == 256 && CHUNK % TPB == 0 && CHUNK <= 4096, "the gather pass stages a chunk's candidates in LDS, 8 bytes each");
static_assert(MAX_K <= 4096, "the finish pass sorts up to MAX_K composites in 32 KB of LDS");

// x viewed (outer, n, inner); scratch: cand (rows, k) composites | hist (rows, HIST_WORDS) | counter (rows) | ties (rows, chunks)
struct Args {
    const float *x;
    unsigned n, inner, k, chunks;
    unsigned long long *cand;
    unsigned *hist, *counter, *ties;
    float *values;
    long long *indices;
};

__device__ __forceinline__ unsigned key_of(float v) {
    unsigned b = __float_as_uint(v);
    if (v != v) return 0xFFFFFFFFu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ const float *row_of(const Args &a, unsigned row) {
    const unsigned o = row / a.inner, in = row - o * a.inner;
    return a.x + (size_t)o * a.n * a.inner + in;
}

// The bin of h[0 .. BINS) the cut falls in, counted from the top: above(d) < need <= above(d) + h[d], and rest = need - above(d).
// Thread t owns bins BINS - 1 - t PER down to BINS - (t + 1) PER.  The whole workgroup calls; sh holds WAVES + 2 words.
template <int BINS> __device__ __forceinline__ void find_digit(const unsigned *h, unsigned need, unsigned *sh, unsigned &digit, unsigned &rest) {
    constexpr int PER = BINS / TPB;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, top = BINS - 1 - t * PER;
    unsigned v[PER], sum = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        v[u] = h[top - u];
        sum += v[u];
    }
    const unsigned inc = wave_inclusive_sum(sum, lane);
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    unsigned above = inc - sum;
    for (int w = 0; w < wave; ++w) above += sh[w];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (above < need && need <= above + v[u]) {         // (true in exactly one bin: 1 <= need <= the histogram's total)
            sh[WAVES] = (unsigned)(top - u);
            sh[WAVES + 1] = need - above;
        }
        above += v[u];
    }
    __syncthreads();
    digit = sh[WAVES];
    rest = sh[WAVES + 1];
    __syncthreads();                                         // (sh is reused by the next level)
}

// The threshold key of the row and r, the number of keys equal to it that belong to the answer.
__device__ __forceinline__ void find_threshold(const unsigned *H, unsigned k, unsigned *sh, unsigned &T, unsigned &r) {
    unsigned d1, d2, d3, need;
    find_digit<BINS1>(H, k, sh, d1, need);
    find_digit<BINS2>(H + BINS1, need, sh, d2, need);
    find_digit<BINS3>(H + BINS1 + BINS2, need, sh, d3, r);
    T = d1 << 21 | d2 << 10 | d3;
}

// f(v, i, on) for every element i of [i0, i0 + len) of the row, in no particular order; the workgroup's waves call f in
// lockstep (f holds ballots), `on` says whether the lane carries an element.  inner == 1: a head of 0..3 floats up to the first
// 16-byte boundary and a tail of 0..3 floats share one call of wave 0, the rest are 16-byte loads; otherwise strided scalars.
template <class F> __device__ __forceinline__ void visit_chunk(const float *row, unsigned inner, unsigned i0, unsigned len, F f) {
    const unsigned t = threadIdx.x;
    if (inner == 1) {
        const float *p = row + i0;
        const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
        const unsigned head = min((4 - mis) & 3, len), nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
        if (t < 64 && (head || tail0 < len)) {              // (workgroup-uniform but for t < 64, which is a whole wave)
            const bool is_head = t < head, is_tail = t >= 4 && tail0 + (t - 4) < len;
            const unsigned j = is_head ? t : tail0 + (t - 4);
            const bool on = is_head || is_tail;
            f(on ? p[j] : 0.f, i0 + j, on);
        }
        const float4 *vec = reinterpret_cast<const float4 *>(p + head);
        for (unsigned j0 = 0; j0 < nvec; j0 += TPB) {
            const unsigned j = j0 + t;
            const bool on = j < nvec;
            const float4 v = on ? vec[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            const unsigned i = i0 + head + 4 * j;
            f(v.x, i, on);
            f(v.y, i + 1, on);
            f(v.z, i + 2, on);
            f(v.w, i + 3, on);
        }
    } else {
        for (unsigned j0 = 0; j0 < len; j0 += TPB) {
            const unsigned j = j0 + t;
            const bool on = j < len;
            f(on ? row[(size_t)(i0 + j) * inner] : 0.f, i0 + j, on);
        }
    }
}

// grid-stride: the histograms and the counters are adjacent in scratch
__global__ void __launch_bounds__(TPB) clear_kernel(unsigned *p, size_t words) {
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < words; i += stride) p[i] = 0u;
}

// grid = rows * chunks, workgroup row * chunks + chunk (a grid's y extent ends at 65 535 rows)
template <int LEVEL> __global__ void __launch_bounds__(TPB) hist_kernel(Args a) {
    constexpr int BINS = LEVEL == 3 ? BINS3 : BINS1, SHIFT = LEVEL == 1 ? 21 : LEVEL == 2 ? 10 : 0;
    constexpr int OFF = LEVEL == 1 ? 0 : LEVEL == 2 ? BINS1 : BINS1 + BINS2;
    constexpr unsigned ABOVE = LEVEL == 1 ? 0u : LEVEL == 2 ? 0xFFE00000u : 0xFFFFFC00u;      // the digits already decided
    __shared__ unsigned lh[BINS];
    __shared__ unsigned sh[WAVES + 2];
    const unsigned row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks;
    unsigned *H = a.hist + (size_t)row * HIST_WORDS;
    unsigned prefix = 0, need = a.k, d;
    if (LEVEL >= 2) {
        find_digit<BINS1>(H, need, sh, d, need);
        prefix = d << 21;
    }
    if (LEVEL == 3) {
        find_digit<BINS2>(H + BINS1, need, sh, d, need);
        prefix |= d << 10;
    }
    for (int b = threadIdx.x; b < BINS; b += TPB) lh[b] = 0u;
    __syncthreads();
    const unsigned i0 = chunk * (unsigned)CHUNK, len = min((unsigned)CHUNK, a.n - i0);
    const int lane = threadIdx.x & 63;
    visit_chunk(row_of(a, row), a.inner, i0, len, [&](float v, unsigned, bool on) {
        const unsigned key = key_of(v), digit = (key >> SHIFT) & (unsigned)(BINS - 1);
        on = on && (key & ABOVE) == prefix;
        const unsigned long long m = __ballot(on);
        if (!m) return;
        const int leader = __ffsll(m) - 1;
        const unsigned d0 = __shfl(digit, leader);
        if (__ballot(on && digit != d0) == 0ull) {          // one digit in the whole wave: one atomic (rows of equal values)
            if (lane == leader) atomicAdd(&lh[d0], (unsigned)__popcll(m));
        } else if (on) {
            atomicAdd(&lh[digit], 1u);
        }
    });
    __syncthreads();
    for (int b = threadIdx.x; b < BINS; b += TPB)
        if (lh[b]) atomicAdd(&H[OFF + b], lh[b]);
}

// grid = rows * chunks.  The candidates of a chunk are staged in LDS (slots from a wave-aggregated LDS atomic), then one atomic on
// the row's counter reserves their places in the row's buffer and the workgroup copies them there.
__global__ void __launch_bounds__(TPB) gather_kernel(Args a) {
    __shared__ unsigned long long stage[CHUNK];
    __shared__ unsigned sh[WAVES + 2];
    __shared__ unsigned staged, ties, base;
    const unsigned row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks;
    unsigned T, r;
    find_threshold(a.hist + (size_t)row * HIST_WORDS, a.k, sh, T, r);
    if (threadIdx.x == 0) staged = ties = 0u;
    __syncthreads();
    const unsigned i0 = chunk * (unsigned)CHUNK, len = min((unsigned)CHUNK, a.n - i0);
    const int lane = threadIdx.x & 63;
    unsigned equal = 0;
    visit_chunk(row_of(a, row), a.inner, i0, len, [&](float v, unsigned i, bool on) {
        const unsigned key = key_of(v);
        equal += on && key == T;
        const bool take = on && key > T;
        const unsigned long long m = __ballot(take);
        if (!m) return;
        const int leader = __ffsll(m) - 1;
        unsigned at = 0;
        if (lane == leader) at = atomicAdd(&staged, (unsigned)__popcll(m));
        at = __shfl(at, leader) + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (take) stage[at] = (unsigned long long)key << 32 | i;      // (at < len <= CHUNK: a slot per element at the most)
    });
    for (int o = 32; o; o >>= 1) equal += __shfl_xor(equal, o);
    if (lane == 0 && equal) atomicAdd(&ties, equal);
    __syncthreads();
    const unsigned total = staged;
    if (threadIdx.x == 0) {
        a.ties[(size_t)row * a.chunks + chunk] = ties;
        base = total ? atomicAdd(&a.counter[row], total) : 0u;
    }
    __syncthreads();
    // all rows' keys above T number c < k, so base + j stays inside the row's k slots; the comparison only restates the bound
    for (unsigned j = threadIdx.x; j < total; j += TPB)
        if (base + j < a.k) a.cand[(size_t)row * a.k + base + j] = stage[j];
}

// grid = rows
__global__ void __launch_bounds__(TPB) finish_kernel(Args a) {
    __shared__ unsigned long long s[MAX_K];
    __shared__ unsigned sh[WAVES + 2];
    __shared__ unsigned chunk_ties[TPB];
    __shared__ unsigned wave_count[WAVES];
    const unsigned row = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned T, r;
    find_threshold(a.hist + (size_t)row * HIST_WORDS, a.k, sh, T, r);
    const unsigned c = a.k - r;
    const float *x = row_of(a, row);
    const unsigned o = row / a.inner, in = row - o * a.inner;
    const size_t out0 = (size_t)o * a.k * a.inner + in;      // place j of the row is out0 + j * inner
    // the c candidates, descending; zero is below every composite (the smallest key, -inf's, is 0x007FFFFF)
    unsigned npad = 1;
    while (npad < c) npad <<= 1;
    if (c) {
        for (unsigned j = t; j < npad; j += TPB) s[j] = j < c ? a.cand[(size_t)row * a.k + j] : 0ull;
        __syncthreads();
        for (unsigned size = 2; size <= npad; size <<= 1)
            for (unsigned step = size >> 1; step > 0; step >>= 1) {
                for (unsigned p = t; p < npad / 2; p += TPB) {
                    const unsigned lo = 2 * p - (p & (step - 1)), hi = lo + step;
                    const bool down = (lo & size) == 0;             // descending run
                    const unsigned long long u = s[lo], w = s[hi];
                    if ((u < w) == down) {
                        s[lo] = w;
                        s[hi] = u;
                    }
                }
                __syncthreads();
            }
        for (unsigned j = t; j < c; j += TPB) {
            const unsigned i = (unsigned)s[j];
            a.values[out0 + (size_t)j * a.inner] = x[(size_t)i * a.inner];
            a.indices[out0 + (size_t)j * a.inner] = (long long)i;
        }
    }
    // the r ties, by descending index: the chunks from the last one backwards, TPB tie counts at a time through LDS, and inside a
    // chunk that has ties TPB elements at a time from its end, each tie placed by a ballot and the counts of the waves in front
    unsigned placed = 0;
    for (unsigned g0 = 0; g0 < a.chunks && placed < r; g0 += TPB) {
        chunk_ties[t] = g0 + t < a.chunks ? a.ties[(size_t)row * a.chunks + (a.chunks - 1 - (g0 + t))] : 0u;
        __syncthreads();
        for (unsigned u = 0; u < TPB && placed < r; ++u) {
            if (!chunk_ties[u]) continue;
            const unsigned chunk = a.chunks - 1 - (g0 + u);
            const unsigned i0 = chunk * (unsigned)CHUNK, len = min((unsigned)CHUNK, a.n - i0);
            for (unsigned j0 = 0; j0 < len && placed < r; j0 += TPB) {
                const bool on = j0 + t < len;
                const unsigned i = i0 + len - 1 - (j0 + t);            // (used only where on)
                const float v = on ? x[(size_t)i * a.inner] : 0.f;
                const bool tie = on && key_of(v) == T;
                const unsigned long long m = __ballot(tie);
                if (lane == 0) wave_count[wave] = (unsigned)__popcll(m);
                __syncthreads();
                unsigned at = placed + (unsigned)__popcll(m & ((1ull << lane) - 1ull)), all = 0;
                for (unsigned w = 0; w < WAVES; ++w) {
                    at += w < wave ? wave_count[w] : 0u;
                    all += wave_count[w];
                }
                if (tie && at < r) {
                    a.values[out0 + (size_t)(c + at) * a.inner] = v;
                    a.indices[out0 + (size_t)(c + at) * a.inner] = (long long)i;
                }
                placed += all;
                __syncthreads();                                       // (wave_count is rewritten by the next step)
            }
        }
        __syncthreads();                                               // (chunk_ties is rewritten by the next group)
    }
}

}  // namespace topk_select
