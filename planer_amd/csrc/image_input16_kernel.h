// uint16 (and uint8) image batches -> the float32 NCHW tensor a net reads, with an optional per-image percentile scaling
// (DESIGN 4.33): y[n][c] = fl(fl(r * kk[n][c]) + bb[n][c]), r the sample of source channel s = order[c] (or util.resize's bilinear
// sample, in the uint8 kernel's order of roundings).  Without `normalise` kk, bb are the caller's k, b (kernel arguments).  With
// it, per source plane P = (n, s) of M = H W samples sorted ascending s_0 .. s_{M-1}:
//     p_q = s_j + (s_j1 - s_j) g        for q in {lo, hi}; j, j1, g from the host in float64 (struct Ranks: they depend on M alone)
//     d = p_hi - p_lo, 1 unless d > 0;  K = k[c] / d;  B = b[c] - p_lo K;  kk = fl32(K), bb = fl32(B)
// every double operation rounded on its own (the library is built with -ffp-contract=off).
//
// The four order statistics s_j of a plane are SELECTED, not sorted for: two radix levels over a 16-bit key (the sample; a uint8
// sample is the key's HIGH byte, which spreads its histogram over the bins and leaves the low level one bin).  Five launches
// whatever the data, all on the caller's stream, no host round trip, no float atomics, no waiting between workgroups:
//
//   clear      zeroes the call's 1280 counters per plane (the scratch block comes from a pool: nothing in it is assumed).
//   hist_hi    a workgroup takes a chunk of consecutive pixels of one image (chunk_pixels: CHUNK_PX, more in large images) --
//              ONE contiguous run of samples, all C channels of an interleaved source, one plane of a planar one (which is
//              handled as N C one-channel images).  The run may start
//              at any sample: the samples in front of the first 16-byte boundary and behind the last go one per lane,
//              everything between as 16-byte loads; nothing outside the run is read.  Each wave counts the high bytes in its
//              own 256 bins per channel in LDS (ds_add_u32: 4 waves x 4 channels x 256 bins = 16 KB); after one barrier the
//              waves' bins are summed and the non-zero sums added to the plane's 256 global bins.  Integer adds: any order gives
//              the same bits.  Bound: the 2 bytes per sample it reads; the LDS atomics where a wave's samples share a bin.
//   hist_lo    the same walk.  Each workgroup first re-derives, from the plane's 256 bins (256 integers out of L2, one wave scan per
//              channel, all channels in flight together), which bins hold ranks j_lo, j1_lo, j_hi, j1_hi; the ranks ascend, so
//              the FIRST rank that falls into a bin names that bin's slot (at most 4 slots per plane).  slot_of[channel][high
//              byte] (1 KB of LDS) is 0xFF for every other bin.  A sample whose high byte has a slot counts its low byte there:
//              [copy][channel][slot][256] in LDS, 32 KB, min(4, 8 / C) copies shared by the waves.  Bound: the same read; the LDS
//              atomics for a batch whose samples share one high byte (12-bit data in 16-bit words: 16 of 256 bins).
//   affine     one workgroup per image: the scan of hist_lo again (bucket and the rank left inside it), then per channel a scan
//              of the four slots' low bins; s = bucket << 8 | low byte.  Lanes 0 .. Co-1 form kk, bb in float64 and store them as
//              float2 kb[n][c].  Microseconds; bound by its barriers.
//   decode     image_input's flat and resize kernels restated for 1- or 2-byte samples, the affine read from kb[n][c] where one
//              is given and from the kernel arguments otherwise (the uint16 decode without `normalise`).  Memory-bound: 2 bytes
//              read and 4 written per element.
// Ranks are below M < 2^31, so 32-bit counters cannot wrap.  All offsets are size_t.
#pragma once
#include "common.h"
#include "device_utils.h"
#include "image_input_kernel.h"

namespace image_input16 {

using image_input::Affine;
using image_input::affine;
constexpr int TPB = PL_STREAM_TPB;
constexpr int WAVES = TPB / 64;
constexpr int LANE_PX = image_input::LANE_PX;
constexpr int TILE_PX = image_input::TILE_PX;
constexpr int MAX_C = image_input::MAX_C;
constexpr int CHUNK_PX = PL_IMAGE_NORM_CHUNK_PIXELS;
constexpr int BINS = 256;
constexpr int RANKS = 4;                                  // j_lo, j1_lo, j_hi, j1_hi
constexpr int PLANE_WORDS = PL_IMAGE_NORM_PLANE_WORDS;    // per plane: 256 high bins, then RANKS slots of 256 low bins
constexpr int LO_COPIES_X_C = 8;                          // hist_lo: copies * C <= 8 -> 32 KB of LDS
static_assert(TPB == BINS && RANKS == MAX_C, "a thread owns one bin of a scan, of up to MAX_C histograms at a time");
static_assert(PLANE_WORDS == BINS + RANKS * BINS, "the header's scratch formula");
constexpr int HIST_BLOCKS = 1024;                         // a pass's workgroups where CHUNK_PX would give more (see chunk_pixels)

// Pixels per workgroup of the histogram passes: CHUNK_PX, or the multiple of it that keeps the pass at about HIST_BLOCKS
// workgroups.  Every workgroup ends with up to 256 atomics per channel on its plane's bins, and atomics on one address are served
// one after another: at 4096 x 4096 x 1 the 4096 workgroups of CHUNK_PX pixels spent 79 us there, ten times the read.
inline size_t chunk_pixels(size_t images, size_t HW) {
    const size_t base = (HW + CHUNK_PX - 1) / CHUNK_PX, per_image = HIST_BLOCKS / images > 0 ? HIST_BLOCKS / images : 1;
    return (size_t)CHUNK_PX * ((base + per_image - 1) / per_image);
}

struct Ranks {
    unsigned j[RANKS];                                    // ascending
    double g[2];                                          // the fractions of lo and hi
};

// The samples of the run [src, src + n) to f(key, channel); the run starts at a pixel, so sample i is of channel i % C.
template <typename T, typename F> __device__ __forceinline__ void walk_run(const T *src, int n, int C, F f) {
    constexpr int PER = 16 / (int)sizeof(T), BITS = 8 * (int)sizeof(T), KEY_SHIFT = 16 - BITS;
    const int t = threadIdx.x;
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) & 15u) / sizeof(T));
    const int head = min((PER - mis) & (PER - 1), n);     // samples in front of the first 16-byte boundary
    const int body = (n - head) / PER;                    // whole 16-byte words
    const int tail0 = head + body * PER;                  // first sample behind them
    if (t < head) f((unsigned)src[t] << KEY_SHIFT, t % C);
    if (t >= 64 && t - 64 < n - tail0) f((unsigned)src[tail0 + t - 64] << KEY_SHIFT, (tail0 + t - 64) % C);
    for (int w = t; w < body; w += TPB) {
        const int i0 = head + w * PER;
        const uint4 v = *reinterpret_cast<const uint4 *>(src + i0);
        const unsigned wd[4] = {v.x, v.y, v.z, v.w};
        int c = i0 % C;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            f(((wd[e * BITS / 32] >> (e * BITS % 32)) & ((1u << BITS) - 1u)) << KEY_SHIFT, c);
            c = c + 1 == C ? 0 : c + 1;
        }
    }
}

// Thread t holds v[i], bin t of histogram i: ex[i] = the bins below it, summed.  The whole block calls; two barriers; wsum is
// free again on return.
__device__ __forceinline__ void block_exclusive_scan(const unsigned (&v)[MAX_C], unsigned (&ex)[MAX_C], unsigned (*wsum)[WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc[MAX_C];
#pragma unroll
    for (int i = 0; i < MAX_C; ++i) {
        inc[i] = wave_inclusive_sum(v[i], lane);
        if (lane == 63) wsum[i][wave] = inc[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MAX_C; ++i) {
        unsigned below = 0;
        for (int w = 0; w < wave; ++w) below += wsum[i][w];
        ex[i] = inc[i] - v[i] + below;
    }
    __syncthreads();
}

// whether sorted element `rank` lies in the bin that holds `count` elements behind `below` smaller ones
__device__ __forceinline__ bool holds(unsigned rank, unsigned below, unsigned count) { return rank >= below && rank - below < count; }

__global__ void __launch_bounds__(TPB) clear_kernel(unsigned *p, size_t words) {
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < words; i += stride) p[i] = 0u;
}

// grid = images * chunks, an image being C interleaved channels of HW pixels.  hist: [image C + channel][PLANE_WORDS].
template <typename T>
__global__ void __launch_bounds__(TPB) hist_hi_kernel(const T *x, unsigned *hist, size_t HW, int C, unsigned chunks, size_t chunk_px) {
    __shared__ unsigned h[WAVES * MAX_C * BINS];          // [wave][channel][bin]
    const int t = threadIdx.x;
    for (int i = t; i < WAVES * MAX_C * BINS; i += TPB) h[i] = 0u;
    __syncthreads();
    const unsigned chunk = blockIdx.x % chunks;
    const size_t img = blockIdx.x / chunks;
    const size_t p0 = (size_t)chunk * chunk_px;
    const int npx = (int)min(chunk_px, HW - p0);
    unsigned *mine = h + (t >> 6) * MAX_C * BINS;
    walk_run(x + (img * HW + p0) * (size_t)C, npx * C, C, [&](unsigned key, int c) { atomicAdd(&mine[c * BINS + (key >> 8)], 1u); });
    __syncthreads();
    for (int i = t; i < C * BINS; i += TPB) {
        unsigned sum = 0;
        for (int w = 0; w < WAVES; ++w) sum += h[w * MAX_C * BINS + i];
        if (sum) atomicAdd(&hist[(img * (size_t)C + (size_t)(i / BINS)) * PLANE_WORDS + (size_t)(i % BINS)], sum);
    }
}

template <typename T>
__global__ void __launch_bounds__(TPB) hist_lo_kernel(const T *x, unsigned *hist, size_t HW, int C, unsigned chunks, size_t chunk_px, Ranks rk) {
    __shared__ unsigned h[LO_COPIES_X_C * RANKS * BINS];  // [copy][channel][slot][bin]
    __shared__ unsigned wsum[MAX_C][WAVES];
    __shared__ unsigned char slot_of[MAX_C][BINS];
    const int t = threadIdx.x;
    for (int i = t; i < LO_COPIES_X_C * RANKS * BINS; i += TPB) h[i] = 0u;
    const unsigned chunk = blockIdx.x % chunks;
    const size_t img = blockIdx.x / chunks;
    unsigned *planes = hist + img * (size_t)C * PLANE_WORDS;
    unsigned v[MAX_C], ex[MAX_C];
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) v[c] = c < C ? planes[(size_t)c * PLANE_WORDS + t] : 0u;
    block_exclusive_scan(v, ex, wsum);
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) {
        unsigned char s = 0xFF;
        for (int r = RANKS - 1; r >= 0; --r)
            if (holds(rk.j[r], ex[c], v[c])) s = (unsigned char)r;
        slot_of[c][t] = s;
    }
    __syncthreads();
    const size_t p0 = (size_t)chunk * chunk_px;
    const int npx = (int)min(chunk_px, HW - p0);
    const int copies = min(WAVES, LO_COPIES_X_C / C);
    unsigned *mine = h + ((t >> 6) % copies) * C * RANKS * BINS;
    walk_run(x + (img * HW + p0) * (size_t)C, npx * C, C, [&](unsigned key, int c) {
        const unsigned s = slot_of[c][key >> 8];
        if (s != 0xFF) atomicAdd(&mine[(c * RANKS + (int)s) * BINS + (int)(key & 255u)], 1u);
    });
    __syncthreads();
    for (int i = t; i < C * RANKS * BINS; i += TPB) {
        unsigned sum = 0;
        for (int w = 0; w < copies; ++w) sum += h[w * C * RANKS * BINS + i];
        if (sum) atomicAdd(&planes[(size_t)(i / (RANKS * BINS)) * PLANE_WORDS + BINS + (size_t)(i % (RANKS * BINS))], sum);
    }
}

// grid = N; image n owns planes n C .. n C + C - 1 in either layout.  kb: [n][MAX_C].  key_shift: 8 where the samples are bytes.
__global__ void __launch_bounds__(TPB) affine_kernel(const unsigned *hist, float2 *kb, int C, int Co, Affine af, Ranks rk,
                                                     int key_shift) {
    __shared__ unsigned wsum[MAX_C][WAVES];
    __shared__ unsigned bucket[MAX_C][RANKS], left[MAX_C][RANKS], slot[MAX_C][RANKS], value[MAX_C][RANKS];
    const int t = threadIdx.x;
    const unsigned *planes = hist + (size_t)blockIdx.x * (size_t)C * PLANE_WORDS;
    if (t < MAX_C * RANKS) (&bucket[0][0])[t] = (&left[0][0])[t] = (&slot[0][0])[t] = (&value[0][0])[t] = 0u;
    unsigned v[MAX_C], ex[MAX_C];
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) v[c] = c < C ? planes[(size_t)c * PLANE_WORDS + t] : 0u;
    block_exclusive_scan(v, ex, wsum);                    // (its barriers also order the zeroes above before the stores below)
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) {
        int first = -1;
        for (int r = 0; r < RANKS; ++r)
            if (holds(rk.j[r], ex[c], v[c])) {
                if (first < 0) first = r;
                bucket[c][r] = (unsigned)t;
                left[c][r] = rk.j[r] - ex[c];
                slot[c][r] = (unsigned)first;
            }
    }
    __syncthreads();
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int r = 0; r < RANKS; ++r) v[r] = planes[(size_t)c * PLANE_WORDS + BINS + (size_t)slot[c][r] * BINS + t];
        block_exclusive_scan(v, ex, wsum);
#pragma unroll
        for (int r = 0; r < RANKS; ++r)
            if (holds(left[c][r], ex[r], v[r])) value[c][r] = (bucket[c][r] << 8 | (unsigned)t) >> key_shift;
    }
    __syncthreads();
    if (t < Co) {
        const int s = af.order[t];
        const double a0 = (double)value[s][0], a1 = (double)value[s][1], b0 = (double)value[s][2], b1 = (double)value[s][3];
        const double p_lo = __dadd_rn(a0, __dmul_rn(__dsub_rn(a1, a0), rk.g[0]));
        const double p_hi = __dadd_rn(b0, __dmul_rn(__dsub_rn(b1, b0), rk.g[1]));
        double d = __dsub_rn(p_hi, p_lo);
        if (!(d > 0.0)) d = 1.0;
        const double K = __ddiv_rn((double)af.k[t], d);
        const double B = __dsub_rn((double)af.b[t], __dmul_rn(p_lo, K));
        kb[(size_t)blockIdx.x * MAX_C + t] = make_float2((float)K, (float)B);
    }
}

// image_input::image_u8_flat_kernel for samples of type T; kb (or null: af.k, af.b) holds the affine of (n, c).
template <typename T, bool NHWC>
__global__ void __launch_bounds__(TPB) image_flat_kernel(const T *x, float *y, size_t HW, int C, int Co, unsigned tiles, Affine af,
                                                         const float2 *kb, bool vec_store) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[TILE_PX * MAX_C * sizeof(T) + 16];
    const unsigned tile = blockIdx.x % tiles;
    const size_t plane = blockIdx.x / tiles;              // NHWC: image n; else n * Co + c
    const size_t p0 = (size_t)tile * TILE_PX;
    const int npx = (int)min((size_t)TILE_PX, HW - p0);
    int oc = 0;                                           // !NHWC: this block's output channel
    size_t src0, n = plane;
    if (NHWC) {
        src0 = (plane * HW + p0) * (size_t)C;
    } else {
        n = plane / (size_t)Co;
        oc = (int)(plane - n * (size_t)Co);
        src0 = (n * (size_t)C + (size_t)af.order[oc]) * HW + p0;
    }
    const int nbytes = (NHWC ? npx * C : npx) * (int)sizeof(T);
    const unsigned char *src = reinterpret_cast<const unsigned char *>(x + src0);
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
    const int head = min((16 - mis) & 15, nbytes);        // bytes in front of the first 16-byte boundary
    const int body = (nbytes - head) >> 4;                // whole 16-byte words
    const int tail0 = head + (body << 4);                 // first byte behind them
    const int t = threadIdx.x;
    if (t < head) stage[mis + t] = src[t];
    if (t >= 16 && t - 16 < nbytes - tail0) stage[mis + tail0 + (t - 16)] = src[tail0 + (t - 16)];
    for (int i = t; i < body; i += TPB)
        *reinterpret_cast<uint4 *>(stage + mis + head + (i << 4)) = *reinterpret_cast<const uint4 *>(src + head + (i << 4));
    __syncthreads();
    const int px = t * LANE_PX;
    if (px >= npx) return;
    const int cnt = min(LANE_PX, npx - px);
    const int nout = NHWC ? Co : 1;
    const T *run = reinterpret_cast<const T *>(stage + mis);      // (mis is a multiple of sizeof(T): x is aligned to its type)
    for (int j = 0; j < nout; ++j) {
        const int c = NHWC ? j : oc;
        const float k = kb ? kb[n * MAX_C + c].x : af.k[c], b = kb ? kb[n * MAX_C + c].y : af.b[c];
        const T *s = NHWC ? run + px * C + af.order[c] : run + px;
        const int step = NHWC ? C : 1;
        float *dst = y + ((NHWC ? plane * (size_t)Co + (size_t)c : plane) * HW + p0 + (size_t)px);
        if (vec_store && cnt == LANE_PX) {
            float4 v;
            v.x = affine((float)s[0], k, b);
            v.y = affine((float)s[step], k, b);
            v.z = affine((float)s[2 * step], k, b);
            v.w = affine((float)s[3 * step], k, b);
            *reinterpret_cast<float4 *>(dst) = v;
        } else {
            for (int i = 0; i < cnt; ++i) dst[i] = affine((float)s[i * step], k, b);
        }
    }
}

// image_input::image_u8_resize_kernel for samples of type T and an affine per (n, c).
template <typename T>
__global__ void __launch_bounds__(TPB) image_resize_kernel(const T *x, float *y, size_t total, int H, int W, int C, int Co, int OH,
                                                           int OW, int groups, const int *ra, const float *rs, const int *ca,
                                                           const float *cs, Affine af, const float2 *kb, bool vec_store) {
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const size_t row = i / (size_t)groups;            // n * OH + oh
        const int ow0 = (int)(i - row * (size_t)groups) * LANE_PX;
        const size_t n = row / (size_t)OH;
        const int oh = (int)(row - n * (size_t)OH);
        const int cnt = min(LANE_PX, OW - ow0);
        const int r0 = min(max(ra[oh], 0), H - 2);
        const float fr = rs[oh], gr = __fsub_rn(1.f, fr);
        const T *top = x + (n * (size_t)H + (size_t)r0) * (size_t)W * (size_t)C;
        const T *bot = top + (size_t)W * (size_t)C;
        int c0[LANE_PX];
        float fc[LANE_PX], gc[LANE_PX];
        for (int p = 0; p < LANE_PX; ++p) {
            const int ow = min(ow0 + p, OW - 1);          // (lanes past the row repeat its last column and are not stored)
            c0[p] = min(max(ca[ow], 0), W - 2) * C;
            fc[p] = cs[ow];
            gc[p] = __fsub_rn(1.f, fc[p]);
        }
        for (int c = 0; c < Co; ++c) {
            const int sc = af.order[c];
            const float k = kb ? kb[n * MAX_C + c].x : af.k[c], b = kb ? kb[n * MAX_C + c].y : af.b[c];
            float v[LANE_PX];
            for (int p = 0; p < LANE_PX; ++p) {
                const int o = c0[p] + sc;
                const float tv = __fadd_rn(__fmul_rn((float)top[o], gc[p]), __fmul_rn((float)top[o + C], fc[p]));
                const float bv = __fadd_rn(__fmul_rn((float)bot[o], gc[p]), __fmul_rn((float)bot[o + C], fc[p]));
                v[p] = affine(__fadd_rn(__fmul_rn(tv, gr), __fmul_rn(bv, fr)), k, b);
            }
            float *dst = y + (((n * (size_t)Co + (size_t)c) * (size_t)OH + (size_t)oh) * (size_t)OW + (size_t)ow0);
            if (vec_store && cnt == LANE_PX) {
                *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int p = 0; p < cnt; ++p) dst[p] = v[p];
            }
        }
    }
}

}  // namespace image_input16
