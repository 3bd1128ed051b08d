// Objects as net output: connected components of a uint8 class map (N, H, W), numbered per image by the raster
// position of their first pixel, and the region table of the first max_objects of them.  A chain of launches; kernel boundaries
// are the only synchronisation between workgroups, and no thread ever waits for another workgroup.
//
// An object's ROOT is its pixel with the smallest raster index y W + x.  `link` (int32 per pixel, scratch) holds -1 on background
// and otherwise the raster index of a pixel of the same object at or in front of the pixel itself; a root links to itself.  Links
// only ever decrease, so every walk ends.
//
// tile_kernel     one workgroup per TILE_H x TILE_W tile: class bytes to LDS (background and pixels outside the image as -1),
//                 union-find on an LDS parent array (a pixel links to its left / upper neighbour, under 8 also to the upper
//                 diagonals the other links do not already imply), then link = the raster index of the pixel's tile-local root.
//                 Plain stores, own tile only.
// seam_kernel     one thread per pixel of a tile's top row or left column: union with its equal-class neighbours across the seam
//                 (of a run of equal pairs straight across, inside one pair of tiles, only the first: the rest is implied).
//                 Every access to link is a relaxed agent-scope atomic (the XCDs have private L2s).
// resolve_kernel  every pixel walks to its root (atomics again: the walk halves the paths it passes), writes the root's index into
//                 `labels` for now, and every block of BLOCK raster-consecutive pixels counts its roots.
// scan_kernel     one workgroup per image: the counts become exclusive offsets, num is written, and the image's table rows are
//                 initialised (rows at and behind num: zeros, for good).
// rank_kernel     a root gets its number, offset + roots in front of it inside the block + 1, in `labels`.
// region_kernel   one workgroup per tile: a pixel takes its root's number (labels is final behind this), and area, box and
//                 coordinate sums of the objects numbered up to max_objects go through the tile's table (region_table.h) into
//                 the rows [class, area, y0, x0, y1, x1].  The root's thread stores the class.
// centroid_kernel float32(float64(sum) / float64(area)) per row, +0.0 in the unused rows.
//
// union (Playne & Hawick's atomicMin form): find both roots; atomicMin on the larger root's word towards the smaller; if the word
// no longer held that root, go on from the value the atomic returned (a word that was lowered past its former parent has cut
// that parent off: the next round joins it again).  The result is the unique partition, whatever order the atomics land in.
#pragma once
#include "common.h"
#include "device_utils.h"
#include "region_table.h"

namespace components {

using namespace regions;                                  // TPB, the tile, RLX, AGENT

constexpr int BLOCK = PL_CC_BLOCK;                        // raster-consecutive pixels behind one root count
constexpr int BLOCK_PER_THREAD = BLOCK / TPB;
constexpr int SCAN_STEP = PL_CC_SCAN_STEP;                // counts one step of scan_kernel's workgroup takes
constexpr int ROW = 6, AREA = 1;                          // a table row: [class, area, y0, x0, y1, x1]
static_assert(BLOCK % TPB == 0, "whole passes");

// ---- union-find on an int array; SCOPE is the HIP memory scope of every access ----
template <int SCOPE> __device__ __forceinline__ int uf_load(int *a, int i) { return __hip_atomic_load(a + i, RLX, SCOPE); }

// the root of x; words passed on the way are lowered to their grandparent (path halving)
template <int SCOPE> __device__ __forceinline__ int uf_find(int *a, int x) {
    int p = uf_load<SCOPE>(a, x);
    while (p != x) {
        const int g = uf_load<SCOPE>(a, p);
        if (g != p) __hip_atomic_fetch_min(a + x, g, RLX, SCOPE);
        x = p;
        p = g;
    }
    return x;
}

template <int SCOPE> __device__ __forceinline__ void uf_union(int *a, int x, int y) {
    for (;;) {
        x = uf_find<SCOPE>(a, x);
        y = uf_find<SCOPE>(a, y);
        if (x == y) return;
        if (x < y) {
            const int t = x;
            x = y;
            y = t;
        }
        const int old = __hip_atomic_fetch_min(a + x, y, RLX, SCOPE);
        if (old == x) return;
        x = old;
    }
}

constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;

struct Geo {
    int H, W, HW, tiles_x, tiles_y, blocks;               // blocks = ceil(HW / BLOCK)
};

// grid = N * tiles_y * tiles_x
__global__ void __launch_bounds__(TPB) tile_kernel(const unsigned char *m, int *link, Geo g, int conn8, int background) {
    __shared__ short cls[TILE_PX];
    __shared__ int parent[TILE_PX];
    const int t = threadIdx.x;
    const unsigned tile = blockIdx.x % (unsigned)(g.tiles_x * g.tiles_y), n = blockIdx.x / (unsigned)(g.tiles_x * g.tiles_y);
    const int y0 = (int)(tile / (unsigned)g.tiles_x) * TILE_H, x0 = (int)(tile % (unsigned)g.tiles_x) * TILE_W;
    const unsigned char *mi = m + (size_t)n * g.HW;
    int *li = link + (size_t)n * g.HW;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = t + k * TPB, y = y0 + (i >> 6), x = x0 + (i & 63);
        int c = -1;
        if (y < g.H && x < g.W) {
            c = mi[y * g.W + x];
            if (c == background) c = -1;
        }
        cls[i] = (short)c;
        parent[i] = i;
    }
    __syncthreads();
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = t + k * TPB, ly = i >> 6, lx = i & 63;
        const int c = cls[i];
        if (c < 0) continue;
        const bool left = lx > 0 && cls[i - 1] == c, up = ly > 0 && cls[i - TILE_W] == c;
        if (left) uf_union<WG>(parent, i, i - 1);
        if (up) uf_union<WG>(parent, i, i - TILE_W);
        if (conn8 && ly > 0 && !up) {                     // (with the upper pixel in, it carries both diagonals)
            if (!left && lx > 0 && cls[i - TILE_W - 1] == c) uf_union<WG>(parent, i, i - TILE_W - 1);
            if (lx < TILE_W - 1 && cls[i - TILE_W + 1] == c) uf_union<WG>(parent, i, i - TILE_W + 1);
        }
    }
    __syncthreads();
    for (int k = 0; k < PER_THREAD; ++k) {
        const int i = t + k * TPB, y = y0 + (i >> 6), x = x0 + (i & 63);
        if (y >= g.H || x >= g.W) continue;
        int r = -1;
        if (cls[i] >= 0) {
            r = i;
            for (int p = uf_load<WG>(parent, r); p != r; p = uf_load<WG>(parent, r)) r = p;      // (no writes in this phase)
            r = (y0 + (r >> 6)) * g.W + x0 + (r & 63);
        }
        li[y * g.W + x] = r;
    }
}

// Threads of one image: (tiles_y - 1) W pixels on the top rows of the tile rows below the first, then (tiles_x - 1) H pixels on
// the left columns of the tile columns right of the first.  A row pixel meets the three pixels above it, a column pixel the
// three to its left: every pair of neighbours that a seam separates is met, the pairs at a tile corner twice.
__global__ void __launch_bounds__(TPB) seam_kernel(const unsigned char *m, int *link, Geo g, int conn8, int background, unsigned per_image,
                                                   unsigned total) {
    const unsigned id = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (id >= total) return;
    const unsigned n = id / per_image;
    unsigned s = id % per_image;
    const unsigned rows = (unsigned)(g.tiles_y - 1) * (unsigned)g.W;
    const unsigned char *mi = m + (size_t)n * g.HW;
    int *li = link + (size_t)n * g.HW;
    int y, x, dy, dx;                                     // the pixel, and the step along the seam
    if (s < rows) {
        y = (int)(s / (unsigned)g.W + 1) * TILE_H, x = (int)(s % (unsigned)g.W), dy = 0, dx = 1;
    } else {
        s -= rows;
        x = (int)(s / (unsigned)g.H + 1) * TILE_W, y = (int)(s % (unsigned)g.H), dy = 1, dx = 0;
    }
    const int c = mi[y * g.W + x];
    if (c == background) return;
    const int p = y * g.W + x;
    const int by = y - dx, bx = x - dy;                   // the pixel straight across the seam
    const bool across = mi[by * g.W + bx] == c;
    if (across) {
        // Where the pixel in front of this one along the seam, inside the same pair of tiles, and the pixel across from that one
        // are of this class too, that thread's union joins the same two tile-local objects: only the first pair of a run works.
        const bool first = dx ? x % TILE_W == 0 : y % TILE_H == 0;
        if (first || mi[(y - dy) * g.W + x - dx] != c || mi[(by - dy) * g.W + bx - dx] != c) uf_union<AGENT>(li, p, by * g.W + bx);
        return;                                           // (the pixel across joins its own neighbours along the seam)
    }
    if (!conn8) return;
    for (int d = -1; d <= 1; d += 2) {
        const int qy = by + d * dy, qx = bx + d * dx;
        if (qy < 0 || qy >= g.H || qx < 0 || qx >= g.W) continue;
        if (mi[qy * g.W + qx] == c) uf_union<AGENT>(li, p, qy * g.W + qx);
    }
}

__device__ __forceinline__ int block_sum(int c, int *wsum) {
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) s += wsum[w];
    return s;
}

// grid = N * blocks.  labels[p] = root of p, or -1; counts[n * blocks + b] = roots among the block's pixels.
__global__ void __launch_bounds__(TPB) resolve_kernel(int *link, int *labels, int *counts, Geo g) {
    __shared__ int wsum[TPB / 64];
    const unsigned b = blockIdx.x % (unsigned)g.blocks, n = blockIdx.x / (unsigned)g.blocks;
    int *li = link + (size_t)n * g.HW, *la = labels + (size_t)n * g.HW;
    int roots = 0;
#pragma unroll
    for (int k = 0; k < BLOCK_PER_THREAD; ++k) {
        const unsigned p = b * (unsigned)BLOCK + (unsigned)(k * TPB) + threadIdx.x;
        if (p >= (unsigned)g.HW) continue;
        int r = uf_load<AGENT>(li, (int)p);
        if (r >= 0) r = uf_find<AGENT>(li, r);
        la[p] = r;
        roots += r == (int)p;
    }
    roots = block_sum(roots, wsum);
    if (threadIdx.x == 0) counts[(size_t)n * g.blocks + b] = roots;
}

// grid = N, SCAN_STEP threads.  counts of image n -> exclusive offsets in place; num[n]; table rows of image n.
__global__ void __launch_bounds__(SCAN_STEP) scan_kernel(int *counts, int blocks, int *num, int max_objects, int *objects,
                                                         long long *sums) {
    int *c = counts + (size_t)blockIdx.x * blocks;
    const int total = carry_scan<SCAN_STEP>(blocks, [c](int i) { return c[i]; }, [c](int i, int v, int inc) { c[i] = inc - v; });
    if (threadIdx.x == 0) num[blockIdx.x] = total;
    const size_t row = (size_t)blockIdx.x * max_objects;
    init_rows<ROW, AREA, SCAN_STEP>(objects + row * ROW, sums + row * 2, max_objects, total);
}

// grid = N * blocks; a thread takes BLOCK_PER_THREAD consecutive pixels.  A root (labels[p] == p) gets its number.
__global__ void __launch_bounds__(TPB) rank_kernel(int *labels, const int *offsets, Geo g) {
    __shared__ int wsum[TPB / 64];
    const unsigned b = blockIdx.x % (unsigned)g.blocks, n = blockIdx.x / (unsigned)g.blocks;
    int *la = labels + (size_t)n * g.HW;
    const unsigned base = b * (unsigned)BLOCK + threadIdx.x * (unsigned)BLOCK_PER_THREAD;
    bool f[BLOCK_PER_THREAD];
    int c = 0;
#pragma unroll
    for (int e = 0; e < BLOCK_PER_THREAD; ++e) {
        f[e] = base + e < (unsigned)g.HW && la[base + e] == (int)(base + e);
        c += f[e];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_inclusive_sum(c, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int pos = offsets[(size_t)n * g.blocks + b] + inc - c;
    for (int w = 0; w < wave; ++w) pos += wsum[w];
#pragma unroll
    for (int e = 0; e < BLOCK_PER_THREAD; ++e)
        if (f[e]) la[base + e] = ++pos;
}

// grid = N * tiles_y * tiles_x.  link tells background (-1) and roots (link[p] == p); labels holds numbers at the roots, which no
// thread of this launch writes, and root indices elsewhere, which only their own thread reads and replaces.
__global__ void __launch_bounds__(TPB) region_kernel(const unsigned char *m, const int *link, int *labels, Geo g, int max_objects,
                                                     int *objects, long long *sums) {
    __shared__ Tile table;
    const int t = threadIdx.x, lane = t & 63;
    const unsigned tile = blockIdx.x % (unsigned)(g.tiles_x * g.tiles_y), n = blockIdx.x / (unsigned)(g.tiles_x * g.tiles_y);
    const int y0 = (int)(tile / (unsigned)g.tiles_x) * TILE_H, x0 = (int)(tile % (unsigned)g.tiles_x) * TILE_W;
    const int *li = link + (size_t)n * g.HW;
    int *la = labels + (size_t)n * g.HW;
    table.clear();
    __syncthreads();
    const int inside = min(TILE_W, g.W - x0);             // columns of the tile inside the image: lanes [0, inside)
    for (int k = 0; k < PER_THREAD; ++k) {
        const int ly = (t >> 6) + k * (TPB / 64), y = y0 + ly, x = x0 + lane;
        if (y >= g.H) break;                              // (wave-uniform)
        int number = 0;
        if (lane < inside) {
            const int p = y * g.W + x, l = li[p];
            if (l == p) {
                number = la[p];
                if (number <= max_objects) objects[((size_t)n * max_objects + (number - 1)) * ROW] = m[(size_t)n * g.HW + p];
            } else if (l >= 0) {
                number = la[la[p]];
                la[p] = number;
            } else {
                la[p] = 0;
            }
        }
        if (number > max_objects) number = 0;             // numbered, and without a row
        table.add(number, ly, lane, inside);
    }
    __syncthreads();
    const size_t row = (size_t)n * max_objects;
    table.flush<ROW, AREA>(objects + row * ROW, sums + row * 2, y0, x0);
}

// one thread per table row
__global__ void __launch_bounds__(TPB) centroid_kernel(const int *objects, const long long *sums, float *centroids, unsigned rows) {
    const unsigned r = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (r >= rows) return;
    centroid_row<ROW, AREA>(objects, sums, centroids, r);
}

}  // namespace components
