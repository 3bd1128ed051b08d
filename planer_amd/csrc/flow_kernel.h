// Instances as net output: a flow field (dy, dx) and a probability plane per image, every foreground pixel moved
// along the flow, and the pixels that arrive at one sink region numbered as one instance.  A chain of launches around the
// components chain (components_kernel.h); kernel boundaries are the only synchronisation between workgroups.
//
// A POINTER is the flat index n H W + y W + x of a pixel of the same image, or -1 on background; N H W < 2^31.  Trajectories
// never leave the foreground, so a pointer read through a foreground pointer is never -1.
//
// step_kernel      one float32 decision per pixel (the only kernel that reads floats): next, the pointer one step along the
//                  flow.  It also clears the hit counts and the volume table.  No operation is contracted: every product and sum
//                  is an explicit round-to-nearest intrinsic.
// double_kernel    dst[p] = src[src[p]], or twice that in one launch (src[src[src[src[p]]]]); src and dst are different
//                  buffers, so the answer on cycles and on chains longer than 2^rounds is the one the rule states.
// count_kernel     cnt[end[p]] += 1 for every foreground p: relaxed agent-scope integer atomics (the XCDs have private L2s); the
//                  lanes of a wave that hit one word add once, for the first few words of the wave.
// sink_kernel      the uint8 sink map cnt > 0, the input of pl_components_u8_i32 (connectivity 8, background 0, no table): S, nS.
// volume_kernel    vol[S[q] - 1] += cnt[q] over the sinks q: the pixel count of every raw instance, one atomic per sink pixel.
// renumber_kernel  one workgroup per image scans vol up to nS (read on the device): a kept instance (vol >= min_size) gets the
//                  next number, a dropped one 0, in place; num; and the image's table rows are initialised.
// table_kernel     one workgroup per tile: masks = the number of S[end[p]], and area, box and coordinate sums of the instances
//                  numbered up to max_instances through the tile's table (region_table.h) into the rows [area, y0, x0, y1, x1].
//                  It works from the final numbers alone: a mask need not be connected.
// centre_kernel    float32(float64(sum) / float64(area)) per row, +0.0 in the unused rows.
#pragma once
#include "common.h"
#include "device_utils.h"
#include "region_table.h"

namespace flow {

using namespace regions;                                  // TPB, the tile, RLX, AGENT

constexpr int SCAN_STEP = PL_FLOW_SCAN_STEP;              // raw instances one step of renumber_kernel's workgroup takes
constexpr int QUAD = 4;                                   // pixels a thread of the streaming kernels takes: 16-byte accesses
constexpr int COUNT_GROUPS = 6;                           // sinks a wave of count_kernel adds to with one atomic each
constexpr int ROW = 5, AREA = 0;                          // a table row: [area, y0, x0, y1, x1]

struct Geo {
    int N, H, W, HW, total;                               // total = N H W
    int tiles_x, tiles_y;
    int max_raw;                                          // ceil(H / 2) ceil(W / 2): the raw instances an image can have
    long long image_stride, pixel_stride, off_dy, off_dx, off_prob;
};

__device__ __forceinline__ int sign_of(float v) { return (v > 0.f) - (v < 0.f); }

// One thread per QUAD raster-consecutive pixels of the flat (N, H, W) range.  VEC: the three planes are dense rows of whole
// 16-byte quads (pixel_stride 1, W and every offset a multiple of 4, the base aligned), so a quad lies in one row.
template <bool VEC> __global__ void __launch_bounds__(TPB) step_kernel(const float *x, Geo g, float level, float g2, int *next, int *cnt,
                                                                      int *vol, int vol_words) {
    const unsigned f0 = (blockIdx.x * (unsigned)TPB + threadIdx.x) * (unsigned)QUAD;
    if (f0 >= (unsigned)g.total) return;
    float dy[QUAD], dx[QUAD], pr[QUAD];
    int out[QUAD];
    const int left = min(QUAD, g.total - (int)f0);
    if (VEC) {
        const unsigned n = f0 / (unsigned)g.HW, p = f0 % (unsigned)g.HW;
        const float *xi = x + (size_t)n * g.image_stride + p;
        const float4 a = *reinterpret_cast<const float4 *>(xi + g.off_dy), b = *reinterpret_cast<const float4 *>(xi + g.off_dx),
                     c = *reinterpret_cast<const float4 *>(xi + g.off_prob);
        dy[0] = a.x, dy[1] = a.y, dy[2] = a.z, dy[3] = a.w;
        dx[0] = b.x, dx[1] = b.y, dx[2] = b.z, dx[3] = b.w;
        pr[0] = c.x, pr[1] = c.y, pr[2] = c.z, pr[3] = c.w;
    }
#pragma unroll
    for (int e = 0; e < QUAD; ++e) {
        if (e >= left) break;
        const unsigned f = f0 + e, n = f / (unsigned)g.HW, p = f % (unsigned)g.HW;
        const int y = (int)(p / (unsigned)g.W), xx = (int)(p % (unsigned)g.W);
        const float *xi = x + (size_t)n * g.image_stride;
        if (!VEC) {
            const size_t at = (size_t)p * g.pixel_stride;
            dy[e] = xi[g.off_dy + at], dx[e] = xi[g.off_dx + at], pr[e] = xi[g.off_prob + at];
        }
        int to = -1;
        if (pr[e] > level) {                              // (a NaN is background)
            to = (int)f;
            const float ay = __fmul_rn(dy[e], dy[e]), ax = __fmul_rn(dx[e], dx[e]), l2 = __fadd_rn(ay, ax);
            if (l2 > g2) {                                // (a NaN does not move)
                const int sy = __fmul_rn(3.f, ay) >= ax ? sign_of(dy[e]) : 0, sx = __fmul_rn(3.f, ax) >= ay ? sign_of(dx[e]) : 0;
                const int ty = min(max(y + sy, 0), g.H - 1), tx = min(max(xx + sx, 0), g.W - 1);
                const int tp = ty * g.W + tx;
                if (xi[g.off_prob + (size_t)tp * g.pixel_stride] > level) to = (int)(n * (unsigned)g.HW) + tp;
            }
        }
        out[e] = to;
    }
    if (left == QUAD) {                                   // (next, cnt and vol are 16-byte aligned and f0 is a multiple of 4)
        *reinterpret_cast<int4 *>(next + f0) = make_int4(out[0], out[1], out[2], out[3]);
        *reinterpret_cast<int4 *>(cnt + f0) = make_int4(0, 0, 0, 0);
    } else {
        for (int e = 0; e < left; ++e) next[f0 + e] = out[e], cnt[f0 + e] = 0;
    }
    for (int e = 0; e < left; ++e)                        // vol_words = N max_raw <= total
        if ((int)f0 + e < vol_words) vol[f0 + e] = 0;
}

// dst = src o src (TWICE: o src o src).  src and dst are different buffers.
template <bool TWICE> __global__ void __launch_bounds__(TPB) double_kernel(const int *__restrict__ src, int *__restrict__ dst, int total) {
    const unsigned f0 = (blockIdx.x * (unsigned)TPB + threadIdx.x) * (unsigned)QUAD;
    if (f0 >= (unsigned)total) return;
    const int left = min(QUAD, total - (int)f0);
    int v[QUAD];
    if (left == QUAD) {
        const int4 a = *reinterpret_cast<const int4 *>(src + f0);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
        for (int e = 0; e < QUAD; ++e) v[e] = e < left ? src[f0 + e] : -1;
    }
#pragma unroll
    for (int e = 0; e < QUAD; ++e) {
        if (v[e] < 0) continue;                           // background stays -1
        v[e] = src[v[e]];
        if (TWICE) v[e] = src[src[v[e]]];
    }
    if (left == QUAD) {
        *reinterpret_cast<int4 *>(dst + f0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < left; ++e) dst[f0 + e] = v[e];
    }
}

// one thread per pixel
__global__ void __launch_bounds__(TPB) count_kernel(const int *end, int *cnt, int total) {
    const unsigned f = blockIdx.x * (unsigned)TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int q = f < (unsigned)total ? end[f] : -1;
    bool todo = q >= 0;
    // A wave's 64 raster-consecutive pixels cross a few cells, and a cell's pixels share a sink: up to COUNT_GROUPS times the
    // first lane that still has its hit takes along every lane with the same word; what is left after that adds on its own.
    // (No lane has left: every ballot and shuffle sees the whole wave.)
    for (int it = 0; it < COUNT_GROUPS; ++it) {
        const unsigned long long open = __ballot(todo);
        if (!open) break;                                 // (wave-uniform)
        const int lead = __ffsll((long long)open) - 1;
        const int word = __shfl(q, lead);
        const bool same = todo && q == word;
        const unsigned long long group = __ballot(same);
        if (lane == lead) __hip_atomic_fetch_add(cnt + word, __popcll(group), RLX, AGENT);
        todo = todo && !same;
    }
    if (todo) __hip_atomic_fetch_add(cnt + q, 1, RLX, AGENT);
}

// one thread per QUAD pixels: four bytes of the sink map in one store (the map is 4-byte aligned and padded to whole words)
__global__ void __launch_bounds__(TPB) sink_kernel(const int *cnt, unsigned char *sink, int total) {
    const unsigned f0 = (blockIdx.x * (unsigned)TPB + threadIdx.x) * (unsigned)QUAD;
    if (f0 >= (unsigned)total) return;
    const int left = min(QUAD, total - (int)f0);
    unsigned word = 0;
    if (left == QUAD) {
        const int4 c = *reinterpret_cast<const int4 *>(cnt + f0);
        word = (c.x > 0) | (c.y > 0) << 8 | (c.z > 0) << 16 | (unsigned)(c.w > 0) << 24;
    } else {
        for (int e = 0; e < left; ++e) word |= (unsigned)(cnt[f0 + e] > 0) << (8 * e);
    }
    *reinterpret_cast<unsigned *>(sink + f0) = word;
}

// one thread per pixel; S holds the sink regions' numbers, 1 .. nS per image, and 0 off the sinks
__global__ void __launch_bounds__(TPB) volume_kernel(const int *cnt, const int *S, int *vol, Geo g) {
    const unsigned f = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (f >= (unsigned)g.total) return;
    const int c = cnt[f];
    if (c <= 0) return;
    const unsigned n = f / (unsigned)g.HW;
    __hip_atomic_fetch_add(vol + (size_t)n * g.max_raw + (S[f] - 1), c, RLX, AGENT);
}

// grid = N, SCAN_STEP threads.  vol of image n -> the new numbers in place (0: dropped); num[n]; table rows of image n.
__global__ void __launch_bounds__(SCAN_STEP) renumber_kernel(int *vol, const int *raw_num, int max_raw, int min_size, int *num,
                                                             int max_instances, int *instances, long long *sums) {
    int *v = vol + (size_t)blockIdx.x * max_raw;
    const int raw = min(raw_num[blockIdx.x], max_raw);    // (nS <= max_raw by construction: the clamp only guards the table)
    const int total = carry_scan<SCAN_STEP>(raw, [v, min_size](int j) { return (int)(v[j] >= min_size); },
                                            [v](int j, int keep, int inc) { v[j] = keep ? inc : 0; });
    if (threadIdx.x == 0) num[blockIdx.x] = total;
    const size_t row = (size_t)blockIdx.x * max_instances;
    init_rows<ROW, AREA, SCAN_STEP>(instances + row * ROW, sums + row * 2, max_instances, total);
}

// grid = N * tiles_y * tiles_x.  renum = vol behind renumber_kernel.
__global__ void __launch_bounds__(TPB) table_kernel(const int *end, const int *S, const int *renum, int *masks, Geo g, int max_instances,
                                                    int *instances, long long *sums) {
    __shared__ Tile table;
    const int t = threadIdx.x, lane = t & 63;
    const unsigned tile = blockIdx.x % (unsigned)(g.tiles_x * g.tiles_y), n = blockIdx.x / (unsigned)(g.tiles_x * g.tiles_y);
    const int y0 = (int)(tile / (unsigned)g.tiles_x) * TILE_H, x0 = (int)(tile % (unsigned)g.tiles_x) * TILE_W;
    const size_t base = (size_t)n * g.HW;
    const int *rn = renum + (size_t)n * g.max_raw;
    table.clear();
    __syncthreads();
    const int inside = min(TILE_W, g.W - x0);             // columns of the tile inside the image: lanes [0, inside)
    for (int k = 0; k < PER_THREAD; ++k) {
        const int ly = (t >> 6) + k * (TPB / 64), y = y0 + ly, x = x0 + lane;
        if (y >= g.H) break;                              // (wave-uniform)
        int number = 0;
        if (lane < inside) {
            const size_t f = base + (size_t)y * g.W + x;
            const int q = end[f];
            if (q >= 0) number = rn[S[q] - 1];
            masks[f] = number;
        }
        if (number > max_instances) number = 0;           // numbered, and without a row
        table.add(number, ly, lane, inside);
    }
    __syncthreads();
    const size_t row = (size_t)n * max_instances;
    table.flush<ROW, AREA>(instances + row * ROW, sums + row * 2, y0, x0);
}

// one thread per table row
__global__ void __launch_bounds__(TPB) centre_kernel(const int *instances, const long long *sums, float *centres, unsigned rows) {
    const unsigned r = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (r >= rows) return;
    centroid_row<ROW, AREA>(instances, sums, centres, r);
}

}  // namespace flow
