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
//                  numbered up to max_instances in an LDS hash table keyed by the number (components::region_kernel's), flushed
//                  with one set of global integer atomics per (tile, instance).  It works from the final numbers alone: a mask
//                  need not be connected.
// centre_kernel    float32(float64(sum) / float64(area)) per row, +0.0 in the unused rows.
#pragma once
#include <climits>

#include "common.h"
#include "components_kernel.h"
#include "device_utils.h"

namespace flow {

constexpr int TPB = PL_STREAM_TPB;
constexpr int TILE_H = PL_CC_TILE_H, TILE_W = PL_CC_TILE_W, TILE_PX = TILE_H * TILE_W;   // table_kernel takes the components tile
constexpr int PER_THREAD = TILE_PX / TPB;
constexpr int SLOTS = TILE_PX;                            // a tile holds at most TILE_PX instances: the table never overflows
constexpr int SCAN_STEP = PL_FLOW_SCAN_STEP;              // raw instances one step of renumber_kernel's workgroup takes
constexpr int QUAD = 4;                                   // pixels a thread of the streaming kernels takes: 16-byte accesses
constexpr int COUNT_GROUPS = 6;                           // sinks a wave of count_kernel adds to with one atomic each
static_assert(TILE_W == 64 && TILE_PX % TPB == 0 && (SLOTS & (SLOTS - 1)) == 0, "a wave takes one row of a tile; whole passes");
static_assert(TILE_PX <= 4096 && TILE_W * TILE_PX < (1 << 20), "table_kernel packs area (12 bits) over the x sum (20 bits)");
static_assert(SCAN_STEP % 64 == 0 && SCAN_STEP <= 1024, "whole waves of one workgroup");

constexpr int AGENT = __HIP_MEMORY_SCOPE_AGENT;
#define PL_FLOW_RLX __ATOMIC_RELAXED

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
        if (lane == lead) __hip_atomic_fetch_add(cnt + word, __popcll(group), PL_FLOW_RLX, AGENT);
        todo = todo && !same;
    }
    if (todo) __hip_atomic_fetch_add(cnt + q, 1, PL_FLOW_RLX, AGENT);
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
    __hip_atomic_fetch_add(vol + (size_t)n * g.max_raw + (S[f] - 1), c, PL_FLOW_RLX, AGENT);
}

// grid = N, SCAN_STEP threads.  vol of image n -> the new numbers in place (0: dropped); num[n]; table rows of image n.
__global__ void __launch_bounds__(SCAN_STEP) renumber_kernel(int *vol, const int *raw_num, int max_raw, int min_size, int *num,
                                                             int max_instances, int *instances, long long *sums) {
    __shared__ int wtot[SCAN_STEP / 64];
    __shared__ int carry_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int *v = vol + (size_t)blockIdx.x * max_raw;
    const int raw = min(raw_num[blockIdx.x], max_raw);    // (nS <= max_raw by construction: the clamp only guards the table)
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int j0 = 0; j0 < raw; j0 += SCAN_STEP) {
        const int j = j0 + t;
        const int keep = j < raw && v[j] >= min_size;
        int inc = keep;
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        int before = carry_s;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        if (j < raw) v[j] = keep ? before + inc : 0;
        __syncthreads();
        if (t == SCAN_STEP - 1) carry_s = before + inc;
        __syncthreads();
    }
    const int total = carry_s;
    if (t == 0) num[blockIdx.x] = total;
    for (int j = t; j < max_instances; j += SCAN_STEP) {
        const size_t row = (size_t)blockIdx.x * max_instances + j;
        int *o = instances + row * 5;
        const bool used = j < total;
        o[0] = 0, o[1] = used ? INT_MAX : 0, o[2] = used ? INT_MAX : 0, o[3] = 0, o[4] = 0;
        sums[row * 2] = 0, sums[row * 2 + 1] = 0;
    }
}

// grid = N * tiles_y * tiles_x.  renum = vol behind renumber_kernel.
__global__ void __launch_bounds__(TPB) table_kernel(const int *end, const int *S, const int *renum, int *masks, Geo g, int max_instances,
                                                    int *instances, long long *sums) {
    __shared__ int key[SLOTS], y_lo[SLOTS], x_lo[SLOTS], y_hi[SLOTS], x_hi[SLOTS];
    __shared__ unsigned area_sx[SLOTS], sy[SLOTS];        // area << 20 | sum of x; sum of y (tile-relative)
    const int t = threadIdx.x, lane = t & 63;
    const unsigned tile = blockIdx.x % (unsigned)(g.tiles_x * g.tiles_y), n = blockIdx.x / (unsigned)(g.tiles_x * g.tiles_y);
    const int y0 = (int)(tile / (unsigned)g.tiles_x) * TILE_H, x0 = (int)(tile % (unsigned)g.tiles_x) * TILE_W;
    const size_t base = (size_t)n * g.HW;
    const int *rn = renum + (size_t)n * g.max_raw;
    for (int s = t; s < SLOTS; s += TPB) key[s] = 0, area_sx[s] = 0u, sy[s] = 0u, y_lo[s] = INT_MAX, x_lo[s] = INT_MAX, y_hi[s] = -1, x_hi[s] = -1;
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
        const int first = __shfl(number, 0);
        const bool one = first > 0 && __all(lane >= inside || number == first);
        if (!one && number == 0) continue;
        if (one && lane != 0) continue;
        int s = (int)(((unsigned)number * 2654435761u) >> 16) & (SLOTS - 1);
        for (;;) {
            const int old = atomicCAS(&key[s], 0, number);
            if (old == 0 || old == number) break;
            s = (s + 1) & (SLOTS - 1);
        }
        const unsigned c = one ? (unsigned)inside : 1u, lx = (unsigned)lane;
        atomicAdd(&area_sx[s], one ? (c << 20) | (c * (c - 1) / 2) : (1u << 20) | lx);
        atomicAdd(&sy[s], c * (unsigned)ly);
        atomicMin(&y_lo[s], ly), atomicMax(&y_hi[s], ly);
        atomicMin(&x_lo[s], lane), atomicMax(&x_hi[s], one ? inside - 1 : lane);
    }
    __syncthreads();
    for (int s = t; s < SLOTS; s += TPB) {
        const int number = key[s];
        if (number == 0) continue;
        const size_t row = (size_t)n * max_instances + (number - 1);
        int *o = instances + row * 5;
        const long long area = area_sx[s] >> 20;
        __hip_atomic_fetch_add(o, (int)area, PL_FLOW_RLX, AGENT);
        __hip_atomic_fetch_min(o + 1, y0 + y_lo[s], PL_FLOW_RLX, AGENT);
        __hip_atomic_fetch_min(o + 2, x0 + x_lo[s], PL_FLOW_RLX, AGENT);
        __hip_atomic_fetch_max(o + 3, y0 + y_hi[s] + 1, PL_FLOW_RLX, AGENT);
        __hip_atomic_fetch_max(o + 4, x0 + x_hi[s] + 1, PL_FLOW_RLX, AGENT);
        __hip_atomic_fetch_add(sums + row * 2, area * y0 + (long long)sy[s], PL_FLOW_RLX, AGENT);
        __hip_atomic_fetch_add(sums + row * 2 + 1, area * x0 + (long long)(area_sx[s] & 0xFFFFFu), PL_FLOW_RLX, AGENT);
    }
}

// one thread per table row
__global__ void __launch_bounds__(TPB) centre_kernel(const int *instances, const long long *sums, float *centres, unsigned rows) {
    const unsigned r = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (r >= rows) return;
    const int area = instances[(size_t)r * 5];
    float cy = 0.f, cx = 0.f;
    if (area > 0) {
        cy = __double2float_rn(__ddiv_rn((double)sums[(size_t)r * 2], (double)area));
        cx = __double2float_rn(__ddiv_rn((double)sums[(size_t)r * 2 + 1], (double)area));
    }
    centres[(size_t)r * 2] = cy, centres[(size_t)r * 2 + 1] = cx;
}

}  // namespace flow
