// The region table of the numbered-map heads: what components_kernel.h and flow_kernel.h share.  A map of
// numbers 1 .. num per image goes in; per number up to max_rows a row of WIDTH ints comes out, [.., area, y0, x0, y1, x1] with
// the area in column AREA, and a pair of int64 coordinate sums from which the centroid follows.  How a pixel gets its number
// stays with each chain's kernels; they call the three steps here:
//
// carry_scan / init_rows   one workgroup per image turns per-element values into running sums, and initialises the image's rows.
// Tile                     one workgroup per TILE_H x TILE_W tile: area, box and coordinate sums, tile-relative, in an LDS hash
//                          table keyed by the number, then flushed with one set of global integer atomics per (tile, number).
// centroid_row             float32(float64(sum) / float64(area)) per row, +0.0 in the unused rows.
#pragma once
#include <climits>

#include "common.h"
#include "device_utils.h"

namespace regions {

constexpr int TPB = PL_STREAM_TPB;
constexpr int TILE_H = PL_CC_TILE_H, TILE_W = PL_CC_TILE_W, TILE_PX = TILE_H * TILE_W;
constexpr int PER_THREAD = TILE_PX / TPB;
constexpr int SLOTS = TILE_PX;                            // a tile holds at most TILE_PX regions: the table never overflows
constexpr int RLX = __ATOMIC_RELAXED, AGENT = __HIP_MEMORY_SCOPE_AGENT;      // (the XCDs have private L2s)
static_assert(TILE_W == 64 && TILE_PX % TPB == 0 && (SLOTS & (SLOTS - 1)) == 0, "a wave takes one row of a tile; whole passes");
static_assert(TILE_PX <= 4096 && TILE_W * TILE_PX < (1 << 20), "Tile packs area (12 bits) over the x sum (20 bits)");

// One workgroup of STEP threads: inc = value(0) + .. + value(i) for every i < count, handed to write(i, value(i), inc) by i's
// thread, STEP elements a step.  Returns the sum of them all, in every thread.
template <int STEP, class Value, class Write> __device__ __forceinline__ int carry_scan(int count, Value value, Write write) {
    static_assert(STEP % 64 == 0 && STEP <= 1024, "whole waves of one workgroup");
    __shared__ int wtot[STEP / 64];
    __shared__ int carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int i0 = 0; i0 < count; i0 += STEP) {
        const int i = i0 + t;
        const int v = i < count ? value(i) : 0;
        const int inc = wave_inclusive_sum(v, lane);
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int before = carry_s;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        if (i < count) write(i, v, before + inc);
        __syncthreads();
        if (t == STEP - 1) carry_s = before + inc;
        __syncthreads();
    }
    return carry_s;
}

// The max_rows rows of one image (`rows` and `sums` point at its first) before any tile adds to them: zeros, and INT_MAX in the
// two min columns of the `used` first rows.  Rows at and behind `used` stay zeros for good.
template <int WIDTH, int AREA, int STEP> __device__ __forceinline__ void init_rows(int *rows, long long *sums, int max_rows, int used) {
    for (int j = threadIdx.x; j < max_rows; j += STEP) {
        int *o = rows + (size_t)j * WIDTH;
#pragma unroll
        for (int c = 0; c < WIDTH; ++c) o[c] = j < used && (c == AREA + 1 || c == AREA + 2) ? INT_MAX : 0;
        sums[(size_t)j * 2] = 0, sums[(size_t)j * 2 + 1] = 0;
    }
}

// The table of one tile, in LDS (__shared__ in the kernel): 7 SLOTS words.
struct Tile {
    int key[SLOTS], y_lo[SLOTS], x_lo[SLOTS], y_hi[SLOTS], x_hi[SLOTS];
    unsigned area_sx[SLOTS], sy[SLOTS];                   // area << 20 | sum of x; sum of y (tile-relative)

    __device__ __forceinline__ void clear() {             // (a barrier behind it)
        for (int s = threadIdx.x; s < SLOTS; s += TPB) key[s] = 0, area_sx[s] = 0u, sy[s] = 0u, y_lo[s] = INT_MAX, x_lo[s] = INT_MAX, y_hi[s] = -1, x_hi[s] = -1;
    }

    // The pixel (ly, lane) of the tile carries `number`, 0 for none; the lanes [0, inside) are in the image.  The whole wave
    // calls.  A wave whose pixels in the image all carry one number adds them with one lane.
    __device__ __forceinline__ void add(int number, int ly, int lane, int inside) {
        const int first = __shfl(number, 0);
        const bool one = first > 0 && __all(lane >= inside || number == first);
        if (!one && number == 0) return;
        if (one && lane != 0) return;
        int s = (int)(((unsigned)number * 2654435761u) >> 16) & (SLOTS - 1);
        for (;;) {
            const int old = atomicCAS(&key[s], 0, number);
            if (old == 0 || old == number) break;
            s = (s + 1) & (SLOTS - 1);
        }
        const unsigned cnt = one ? (unsigned)inside : 1u, lx = (unsigned)lane;
        atomicAdd(&area_sx[s], one ? (cnt << 20) | (cnt * (cnt - 1) / 2) : (1u << 20) | lx);
        atomicAdd(&sy[s], cnt * (unsigned)ly);
        atomicMin(&y_lo[s], ly), atomicMax(&y_hi[s], ly);
        atomicMin(&x_lo[s], lane), atomicMax(&x_hi[s], one ? inside - 1 : lane);
    }

    // (a barrier in front of it)  `rows` and `sums` point at the image's first row; (y0, x0) is the tile's corner in the image.
    template <int WIDTH, int AREA> __device__ __forceinline__ void flush(int *rows, long long *sums, int y0, int x0) const {
        for (int s = threadIdx.x; s < SLOTS; s += TPB) {
            const int number = key[s];
            if (number == 0) continue;
            int *o = rows + (size_t)(number - 1) * WIDTH + AREA;
            long long *sm = sums + (size_t)(number - 1) * 2;
            const long long area = area_sx[s] >> 20;
            __hip_atomic_fetch_add(o, (int)area, RLX, AGENT);
            __hip_atomic_fetch_min(o + 1, y0 + y_lo[s], RLX, AGENT);
            __hip_atomic_fetch_min(o + 2, x0 + x_lo[s], RLX, AGENT);
            __hip_atomic_fetch_max(o + 3, y0 + y_hi[s] + 1, RLX, AGENT);
            __hip_atomic_fetch_max(o + 4, x0 + x_hi[s] + 1, RLX, AGENT);
            __hip_atomic_fetch_add(sm, area * y0 + (long long)sy[s], RLX, AGENT);
            __hip_atomic_fetch_add(sm + 1, area * x0 + (long long)(area_sx[s] & 0xFFFFFu), RLX, AGENT);
        }
    }
};

// row r of `rows` (all images') -> its centroid (y, x)
template <int WIDTH, int AREA> __device__ __forceinline__ void centroid_row(const int *rows, const long long *sums, float *out, unsigned r) {
    const int area = rows[(size_t)r * WIDTH + AREA];
    float cy = 0.f, cx = 0.f;
    if (area > 0) {
        cy = __double2float_rn(__ddiv_rn((double)sums[(size_t)r * 2], (double)area));
        cx = __double2float_rn(__ddiv_rn((double)sums[(size_t)r * 2 + 1], (double)area));
    }
    out[(size_t)r * 2] = cy, out[(size_t)r * 2 + 1] = cx;
}

}  // namespace regions
