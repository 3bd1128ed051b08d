// Keypoints as net output: the 3 x 3 local maxima above a threshold of every plane of a float32 (N, K, H, W) tensor,
// counted, and the best max_peaks of each plane as [x, y, score] rows.  Two launches; the kernel boundary is the only
// synchronisation between workgroups, there is no global atomic, and the answer is unique.
//
// A peak travels as a 64-bit KEY: the monotone uint32 image of its score (-0.0 taken as +0.0, in the key only) in the high half,
// ~p of its raster index p = y W + x in the low half.  Keys of one plane are distinct, and descending key order is the
// contract's order: score descending, equal scores by ascending p.  No peak has the key 0 (a peak is above -inf, whose image is
// 0x007fffff), so 0 is the sentinel of an unused slot and sorts behind every peak.
//
// tile_kernel   one workgroup per (plane, TILE_H x TILE_W tile): the tile and its one-pixel halo go to LDS (-inf outside the
//               plane: every comparison against it holds, as if the neighbour did not exist; 16-byte loads where W % 4 == 0),
//               a thread walks eight rows of one column with the 3 x 3 window in registers, a wave's peaks of one row are
//               compacted into the LDS key array behind one LDS counter (the order they land in does not matter: they are sorted),
//               a bitonic network over the next power of two sorts them, and the best min(count, max_peaks) keys, sentinels
//               behind them, and the count go to scratch.  A plane's best max_peaks are among its tiles' best max_peaks.
// merge_kernel  one workgroup per plane: num = the sum of the tile counts; the tiles x max_peaks candidate keys are sorted in LDS,
//               in one go where they fit MERGE_KEYS, else in rounds that keep the running best max_peaks in front and fold the
//               next MERGE_KEYS - max_peaks candidates in (a round whose candidates are all sentinels is skipped); then row j
//               is written from key j: score = the pixel's own bits, the quarter-pixel nudge from its four neighbours read from
//               x, the single rounding of the stride product; +0.0 where the key is the sentinel.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace peaks {

using u64 = unsigned long long;
constexpr int TPB = PL_STREAM_TPB;
constexpr int TILE_H = PL_PEAKS_TILE_H, TILE_W = PL_PEAKS_TILE_W, TILE_PX = TILE_H * TILE_W;
constexpr int MERGE_KEYS = PL_PEAKS_MERGE_KEYS;
constexpr int ROWS_PER_THREAD = TILE_PX / TPB;            // a thread's run of rows in its column
constexpr int LDW = TILE_W + 8;                           // LDS row: 3 unused, left halo, the tile (16-byte aligned), right halo, 3 unused
constexpr int HALO = 2 * (TILE_W + 2) + 2 * TILE_H;
static_assert(TILE_W == 64 && TPB == 256, "a wave takes one column run per lane, four waves the tile's four row groups");
static_assert(TILE_H == (TPB / 64) * ROWS_PER_THREAD && HALO <= TPB && TILE_PX / 4 % TPB == 0, "whole passes");
static_assert((MERGE_KEYS & (MERGE_KEYS - 1)) == 0 && PL_PEAKS_MAX_PEAKS < MERGE_KEYS, "a merge round folds at least one key in");

struct Geo {
    int H, W, HW, tiles_x, tiles_y;
};

__device__ __forceinline__ u64 make_key(float v, int p) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0;                          // -0.0 ties with +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (unsigned)~p;
}

// a[0 .. S) descending, S a power of two; every thread of the workgroup calls it, behind a barrier, and leaves behind one
__device__ __forceinline__ void sort_descending(u64 *a, int S, int t) {
    for (int k = 2; k <= S; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (S >> 1); i += TPB) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const u64 x = a[lo], y = a[hi];
                if ((x < y) == ((lo & k) == 0)) {
                    a[lo] = y;
                    a[hi] = x;
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ int pow2_at_least(int n) {
    int s = 1;
    while (s < n) s <<= 1;
    return s;
}

// grid = planes * tiles_y * tiles_x.  vec: W % 4 == 0 and x is 16-byte aligned, so every row start of every tile is.
__global__ void __launch_bounds__(TPB) tile_kernel(const float *x, Geo g, float threshold, int first, int max_peaks, int vec, u64 *keys,
                                                    int *counts) {
    __shared__ __attribute__((aligned(16))) float s[(TILE_H + 2) * LDW];
    __shared__ u64 key[TILE_PX];
    __shared__ int count;
    const int t = threadIdx.x;
    const unsigned tiles = (unsigned)(g.tiles_x * g.tiles_y), tile = blockIdx.x % tiles, plane = blockIdx.x / tiles;
    const int y0 = (int)(tile / (unsigned)g.tiles_x) * TILE_H, x0 = (int)(tile % (unsigned)g.tiles_x) * TILE_W;
    const float *xp = x + (size_t)plane * g.HW;
    const float ninf = -__builtin_inff();
    const bool full = y0 + TILE_H <= g.H && x0 + TILE_W <= g.W;                 // (uniform)
    if (t == 0) count = 0;
    if (vec) {
#pragma unroll
        for (int k = 0; k < TILE_PX / 4 / TPB; ++k) {
            const int f = t + k * TPB, ly = f >> 4, lx = (f & 15) * 4;
            float4 v = make_float4(ninf, ninf, ninf, ninf);
            if (full || (y0 + ly < g.H && x0 + lx < g.W))                       // (W % 4 == 0: four pixels are in or out together)
                v = *reinterpret_cast<const float4 *>(xp + (size_t)(y0 + ly) * g.W + x0 + lx);
            *reinterpret_cast<float4 *>(s + (ly + 1) * LDW + 4 + lx) = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < ROWS_PER_THREAD; ++k) {
            const int i = t + k * TPB, ly = i >> 6, lx = i & 63;
            float v = ninf;
            if (full || (y0 + ly < g.H && x0 + lx < g.W)) v = xp[(size_t)(y0 + ly) * g.W + x0 + lx];
            s[(ly + 1) * LDW + 4 + lx] = v;
        }
    }
    if (t < HALO) {                                       // top row, bottom row, left column, right column
        int ly, lx;
        if (t < 2 * (TILE_W + 2)) {
            const int top = t < TILE_W + 2;
            ly = top ? -1 : TILE_H, lx = (top ? t : t - (TILE_W + 2)) - 1;
        } else {
            const int u = t - 2 * (TILE_W + 2), left = u < TILE_H;
            ly = left ? u : u - TILE_H, lx = left ? -1 : TILE_W;
        }
        const int y = y0 + ly, xx = x0 + lx;
        float v = ninf;
        if (y >= 0 && y < g.H && xx >= 0 && xx < g.W) v = xp[(size_t)y * g.W + xx];
        s[(ly + 1) * LDW + 4 + lx] = v;
    }
    __syncthreads();
    // thread: column `col`, rows r0 .. r0 + 7; a, m, b are the rows above, at and below the pixel
    const int col = t & 63, r0 = (t >> 6) * ROWS_PER_THREAD;
    const float *w = s + r0 * LDW + 3 + col;
    float a0 = w[0], a1 = w[1], a2 = w[2], m0 = w[LDW], m1 = w[LDW + 1], m2 = w[LDW + 2];
    const bool in_x = x0 + col < g.W;
#pragma unroll
    for (int r = 0; r < ROWS_PER_THREAD; ++r) {
        const float *wb = w + (r + 2) * LDW;
        const float b0 = wb[0], b1 = wb[1], b2 = wb[2];
        const int y = y0 + r0 + r;
        bool pk = in_x && y < g.H && m1 > threshold;
        if (first)
            pk = pk && m1 > a0 && m1 > a1 && m1 > a2 && m1 > m0;
        else
            pk = pk && m1 >= a0 && m1 >= a1 && m1 >= a2 && m1 >= m0;
        pk = pk && m1 >= m2 && m1 >= b0 && m1 >= b1 && m1 >= b2;
        const u64 mask = __ballot(pk);
        if (mask) {                                       // (uniform in the wave)
            int base = 0;
            if (col == 0) base = atomicAdd(&count, __popcll(mask));
            base = __shfl(base, 0);
            if (pk) key[base + __popcll(mask & ((1ull << col) - 1))] = make_key(m1, y * g.W + x0 + col);
        }
        a0 = m0, a1 = m1, a2 = m2, m0 = b0, m1 = b1, m2 = b2;
    }
    __syncthreads();
    const int n = count, S = pow2_at_least(n);
    for (int i = n + t; i < S; i += TPB) key[i] = 0;
    __syncthreads();
    sort_descending(key, S, t);
    u64 *out = keys + (size_t)blockIdx.x * max_peaks;
    for (int i = t; i < max_peaks; i += TPB) out[i] = i < n ? key[i] : 0;
    if (t == 0) counts[blockIdx.x] = n;
}

// grid = planes
__global__ void __launch_bounds__(TPB) merge_kernel(const float *x, const u64 *keys, const int *counts, Geo g, int max_peaks, int refine,
                                                     float sy, float sx, float *peaks, int *num) {
    __shared__ u64 buf[MERGE_KEYS];
    __shared__ int part[TPB / 64];
    const int t = threadIdx.x;
    const unsigned plane = blockIdx.x;
    const int tiles = g.tiles_x * g.tiles_y;
    int c = 0;
    for (int i = t; i < tiles; i += TPB) c += counts[(size_t)plane * tiles + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((t & 63) == 0) part[t >> 6] = c;
    for (int i = t; i < max_peaks; i += TPB) buf[i] = 0;
    const size_t cand = (size_t)tiles * max_peaks;
    const u64 *kp = keys + (size_t)plane * cand;
    int base = 0;                                         // the running best in front of a later round's candidates
    for (size_t done = 0; done < cand; base = max_peaks) {
        const int take = (int)(cand - done < (size_t)(MERGE_KEYS - base) ? cand - done : (size_t)(MERGE_KEYS - base));
        const int S = pow2_at_least(base + take);         // (>= max_peaks: the first round takes a whole tile's keys at least)
        int any = 0;
        for (int i = t; i < S - base; i += TPB) {
            const u64 k = i < take ? kp[done + i] : 0;
            buf[base + i] = k;
            any |= k != 0;
        }
        if (__syncthreads_or(any)) sort_descending(buf, S, t);
        done += take;
    }
    __syncthreads();
    if (t == 0) num[plane] = part[0] + part[1] + part[2] + part[3];
    const float *xp = x + (size_t)plane * g.HW;
    float *row = peaks + (size_t)plane * max_peaks * 3;
    for (int j = t; j < max_peaks; j += TPB) {
        const u64 k = buf[j];
        float ox = 0.f, oy = 0.f, score = 0.f;
        if (k) {
            const unsigned p = ~(unsigned)k, py = p / (unsigned)g.W, px = p - py * (unsigned)g.W;
            score = xp[p];
            float dx = 0.f, dy = 0.f;
            if (refine) {
                if (px > 0 && (int)px < g.W - 1) {
                    const float l = xp[p - 1], r = xp[p + 1];
                    dx = r > l ? 0.25f : r < l ? -0.25f : 0.f;
                }
                if (py > 0 && (int)py < g.H - 1) {
                    const float u = xp[p - g.W], d = xp[p + g.W];
                    dy = d > u ? 0.25f : d < u ? -0.25f : 0.f;
                }
            }
            ox = ((float)px + dx) * sx;                   // (px + dx is exact below PL_PEAKS_MAX_EXTENT: one rounding)
            oy = ((float)py + dy) * sy;
        }
        row[3 * j] = ox, row[3 * j + 1] = oy, row[3 * j + 2] = score;
    }
}

}  // namespace peaks
