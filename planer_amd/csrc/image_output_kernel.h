// A net's float32 NCHW result -> the uint8 array a caller wants: an image, y = the byte of fl(fl(v * k[c]) + b[c])
// (NaN -> 0, clamped to [0, 255], rounded to nearest even or truncated), interleaved (N, H, W, Co) or planar (N, Co, H, W); or a
// label map, y = argmax over the C planes with numpy's rules (the first of equal maxima, the first NaN before any number), for
// C == 1 the comparison x > threshold.  Memory-bound: 4 bytes read per source sample, 1 byte written per output element.
//
// The planes are flat: a workgroup takes PL_IMAGE_OUT_TILE_PIXELS consecutive pixels of one image's H W plane, a lane
// PL_IMAGE_OUT_LANE_PIXELS consecutive ones of them, loaded as one 16-byte word per source plane where the plane's floats are
// 16-byte aligned (H W % 4 == 0 and an aligned x), as single floats otherwise.  Pixels past the end of the plane are neither read
// nor written.
//
// Planar and label output: a lane's LANE_PX bytes are one 32-bit store where their address is 4-byte aligned, single bytes
// otherwise (y may start at any byte).  Interleaved output: the tile's bytes are ONE contiguous run of npx * Co bytes that may
// start at any byte, so the run is staged through LDS (image_input_kernel.h in reverse): LDS byte i + (address of the run mod 16)
// holds byte i of the run; the bytes up to the first 16-byte boundary and behind the last one go one byte per lane, everything
// between as aligned 16-byte stores -- nothing outside the run is written.
//
// The label kernel walks the planes with a running (max, index) pair per pixel, LABEL_UNROLL plane loads in flight per lane.
//
// k, b and order are kernel arguments (struct Affine): no upload, no allocation per call.  All offsets are size_t.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace image_output {

constexpr int TPB = PL_STREAM_TPB;
constexpr int LANE_PX = PL_IMAGE_OUT_LANE_PIXELS;
constexpr int TILE_PX = PL_IMAGE_OUT_TILE_PIXELS;
static_assert(TILE_PX == TPB * LANE_PX, "one lane owns LANE_PX pixels of a tile");
static_assert(LANE_PX == 4, "a lane loads one float4 per source plane and stores one 32-bit word per output plane");
constexpr int MAX_CO = 4;
constexpr int MAX_LABELS = 256;
constexpr int STAGE_BYTES = TILE_PX * MAX_CO + 16;      // the longest run + its offset from a 16-byte boundary
constexpr int LABEL_UNROLL = 4;                         // source planes loaded before the first of them is compared

struct Affine {
    float k[MAX_CO], b[MAX_CO];
    int order[MAX_CO];
};

// LANE_PX consecutive floats of one plane; `vec` only where all of them exist and p is 16-byte aligned
__device__ __forceinline__ void load_px(const float *p, int cnt, bool vec, float (&v)[LANE_PX]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < LANE_PX; ++i) v[i] = i < cnt ? p[i] : 0.f;
    }
}

__device__ __forceinline__ void store_px(unsigned char *d, int cnt, const unsigned (&q)[LANE_PX]) {
    if (cnt == LANE_PX && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
        *reinterpret_cast<unsigned *>(d) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
        for (int i = 0; i < cnt; ++i) d[i] = (unsigned char)q[i];
    }
}

// every operation rounded on its own; NaN -> 0 before the clamp
__device__ __forceinline__ unsigned quantise(float v, float k, float b, bool trunc) {
    float t = __fadd_rn(__fmul_rn(v, k), b);
    t = t != t ? 0.f : t;
    t = fminf(fmaxf(t, 0.f), 255.f);
    return (unsigned)(int)(trunc ? t : rintf(t));       // (t >= 0: the conversion truncates)
}

// grid = N * tiles, block (n, t) reads Co source planes of image n and writes pixels [p0, p0 + npx) of every output channel.
template <bool NHWC>
__global__ void __launch_bounds__(TPB) image_f32_u8_kernel(const float *x, unsigned char *y, size_t HW, int C, int Co,
                                                           unsigned tiles, Affine af, bool vec_load, bool trunc) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[NHWC ? STAGE_BYTES : 16];
    const unsigned tile = blockIdx.x % tiles;
    const size_t n = blockIdx.x / tiles;
    const size_t p0 = (size_t)tile * TILE_PX;
    const int npx = (int)min((size_t)TILE_PX, HW - p0);
    const int t = threadIdx.x;
    const int px = t * LANE_PX;
    const int cnt = min(LANE_PX, npx - px);               // <= 0: a lane past the end of the plane
    unsigned char *run = y + (n * HW + p0) * (size_t)Co;  // NHWC: the tile's bytes
    const int mis = (int)(reinterpret_cast<uintptr_t>(run) & 15u);
    if (cnt > 0) {
        float v[MAX_CO][LANE_PX];
#pragma unroll
        for (int c = 0; c < MAX_CO; ++c)
            if (c < Co) load_px(x + ((n * (size_t)C + (size_t)af.order[c]) * HW + p0 + (size_t)px), cnt, vec_load, v[c]);
#pragma unroll
        for (int c = 0; c < MAX_CO; ++c) {
            if (c >= Co) break;
            unsigned q[LANE_PX];
#pragma unroll
            for (int i = 0; i < LANE_PX; ++i) q[i] = quantise(v[c][i], af.k[c], af.b[c], trunc);
            if (NHWC) {
                unsigned char *s = stage + mis + px * Co + c;
                for (int i = 0; i < cnt; ++i) s[i * Co] = (unsigned char)q[i];
            } else {
                store_px(y + ((n * (size_t)Co + (size_t)c) * HW + p0 + (size_t)px), cnt, q);
            }
        }
    }
    if (!NHWC) return;
    __syncthreads();
    const int nbytes = npx * Co;
    const int head = min((16 - mis) & 15, nbytes);        // bytes in front of the first 16-byte boundary
    const int body = (nbytes - head) >> 4;                // whole 16-byte words
    const int tail0 = head + (body << 4);                 // first byte behind them
    if (t < head) run[t] = stage[mis + t];
    if (t >= 16 && t - 16 < nbytes - tail0) run[tail0 + (t - 16)] = stage[mis + tail0 + (t - 16)];
    for (int i = t; i < body; i += TPB)                   // (at most TILE_PX * MAX_CO / 16 = TPB words: one trip)
        *reinterpret_cast<uint4 *>(run + head + (i << 4)) = *reinterpret_cast<const uint4 *>(stage + mis + head + (i << 4));
}

// numpy's argmax step: a later value wins only if it is greater, or the first NaN
__device__ __forceinline__ void label_step(float (&best)[LANE_PX], unsigned (&idx)[LANE_PX], const float (&v)[LANE_PX], unsigned c) {
#pragma unroll
    for (int i = 0; i < LANE_PX; ++i) {
        const bool take = v[i] > best[i] || (v[i] != v[i] && best[i] == best[i]);
        best[i] = take ? v[i] : best[i];
        idx[i] = take ? c : idx[i];
    }
}

// grid = N * tiles, block (n, t) reads pixels [p0, p0 + npx) of the C planes of image n and writes their labels.
__global__ void __launch_bounds__(TPB) labels_f32_u8_kernel(const float *x, unsigned char *y, size_t HW, int C, unsigned tiles,
                                                            float threshold, bool vec_load) {
    const unsigned tile = blockIdx.x % tiles;
    const size_t n = blockIdx.x / tiles;
    const size_t p0 = (size_t)tile * TILE_PX;
    const int npx = (int)min((size_t)TILE_PX, HW - p0);
    const int px = threadIdx.x * LANE_PX;
    const int cnt = min(LANE_PX, npx - px);
    if (cnt <= 0) return;
    const float *src = x + (n * (size_t)C * HW + p0 + (size_t)px);
    float best[LANE_PX];
    unsigned idx[LANE_PX] = {0, 0, 0, 0};
    load_px(src, cnt, vec_load, best);
    if (C == 1) {
#pragma unroll
        for (int i = 0; i < LANE_PX; ++i) idx[i] = best[i] > threshold ? 1u : 0u;
    } else {
        int c = 1;
        for (; c + LABEL_UNROLL <= C; c += LABEL_UNROLL) {
            float v[LABEL_UNROLL][LANE_PX];
#pragma unroll
            for (int u = 0; u < LABEL_UNROLL; ++u) load_px(src + (size_t)(c + u) * HW, cnt, vec_load, v[u]);
#pragma unroll
            for (int u = 0; u < LABEL_UNROLL; ++u) label_step(best, idx, v[u], (unsigned)(c + u));
        }
        for (; c < C; ++c) {
            float v[LANE_PX];
            load_px(src + (size_t)c * HW, cnt, vec_load, v);
            label_step(best, idx, v, (unsigned)c);
        }
    }
    store_px(y + (n * HW + p0 + (size_t)px), cnt, idx);
}

}  // namespace image_output
