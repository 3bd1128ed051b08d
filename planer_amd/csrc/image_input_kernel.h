// uint8 image batches -> the float32 NCHW tensor a net reads: y[n][c] = fl(fl(r * k[c]) + b[c]), r the byte of
// source channel order[c] (or util.resize's bilinear sample of those bytes, util.py:253-269, in its own order of roundings).
// A memory-bound re-layout: 1 byte read and 4 bytes written per output element.
//
// Without resize the planes are flat: a workgroup takes PL_IMAGE_U8_TILE_PIXELS consecutive pixels of one image (interleaved
// source, "nhwc") or of one channel plane (planar source, "nchw").  Their source bytes are ONE contiguous run that may start at
// any byte (3 W bytes per row; views into larger buffers), so the run is staged through LDS: the bytes up to the first 16-byte
// boundary and behind the last one go one byte per lane, everything between as 16-byte loads -- nothing outside the run is
// read.  LDS byte i + (address of the run mod 16) holds byte i of the run, which keeps the 16-byte LDS stores aligned.  Each
// lane then owns PL_IMAGE_U8_LANE_PIXELS consecutive pixels: per output channel it picks its bytes out of LDS and stores one
// float4 into that channel's plane where the plane's floats are 16-byte aligned (H W % 4 == 0 and an aligned y), single
// floats otherwise.  Pixels past the end of the plane are neither read nor written.
//
// With resize (interleaved source only) a lane owns PL_IMAGE_U8_LANE_PIXELS consecutive output columns of one output row and
// gathers the 2 x 2 source bytes of every sample from global memory (the source is a quarter of the output's bytes and its rows
// are re-read out of L2); columns first, then rows, every product and sum rounded on its own.  Table entries are clamped to
// [0, H - 2] / [0, W - 2], the range util.resize's own index rule gives, so a bad table cannot read outside the image.
//
// k, b and order are kernel arguments (struct Affine): no upload, no allocation per call.  All offsets are size_t.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace image_input {

constexpr int TPB = PL_STREAM_TPB;
constexpr int LANE_PX = PL_IMAGE_U8_LANE_PIXELS;
constexpr int TILE_PX = PL_IMAGE_U8_TILE_PIXELS;
static_assert(TILE_PX == TPB * LANE_PX, "one lane owns LANE_PX pixels of a tile");
static_assert(LANE_PX == 4, "a lane stores one float4 per channel plane");
constexpr int MAX_C = 4;
constexpr int STAGE_BYTES = TILE_PX * MAX_C + 16;       // the longest run + its offset from a 16-byte boundary

struct Affine {
    float k[MAX_C], b[MAX_C];
    int order[MAX_C];
};

__device__ __forceinline__ float affine(float r, float k, float b) { return __fadd_rn(__fmul_rn(r, k), b); }

// NHWC: grid = N * tiles, block (n, t) reads bytes [(n HW + p0) C, +npx C) and writes Co planes.
// !NHWC: grid = N * Co * tiles, block (n, c, t) reads bytes [((n C + order[c]) HW + p0), +npx) and writes plane (n, c).
template <bool NHWC>
__global__ void __launch_bounds__(TPB) image_u8_flat_kernel(const unsigned char *x, float *y, size_t HW, int C, int Co,
                                                            unsigned tiles, Affine af, bool vec_store) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[STAGE_BYTES];
    const unsigned tile = blockIdx.x % tiles;
    const size_t plane = blockIdx.x / tiles;              // NHWC: image n; else n * Co + c
    const size_t p0 = (size_t)tile * TILE_PX;
    const int npx = (int)min((size_t)TILE_PX, HW - p0);
    int oc = 0;                                           // !NHWC: this block's output channel
    size_t src0;
    if (NHWC) {
        src0 = (plane * HW + p0) * (size_t)C;
    } else {
        const size_t n = plane / (size_t)Co;
        oc = (int)(plane - n * (size_t)Co);
        src0 = (n * (size_t)C + (size_t)af.order[oc]) * HW + p0;
    }
    const int nbytes = NHWC ? npx * C : npx;
    const unsigned char *src = x + src0;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
    const int head = min((16 - mis) & 15, nbytes);        // bytes in front of the first 16-byte boundary
    const int body = (nbytes - head) >> 4;                // whole 16-byte words
    const int tail0 = head + (body << 4);                 // first byte behind them
    const int t = threadIdx.x;
    if (t < head) stage[mis + t] = src[t];
    if (t >= 16 && t - 16 < nbytes - tail0) stage[mis + tail0 + (t - 16)] = src[tail0 + (t - 16)];
    for (int i = t; i < body; i += TPB)                   // (at most TILE_PX * MAX_C / 16 = TPB words: one trip)
        *reinterpret_cast<uint4 *>(stage + mis + head + (i << 4)) = *reinterpret_cast<const uint4 *>(src + head + (i << 4));
    __syncthreads();
    const int px = t * LANE_PX;
    if (px >= npx) return;
    const int cnt = min(LANE_PX, npx - px);
    const int nout = NHWC ? Co : 1;
    for (int j = 0; j < nout; ++j) {
        const int c = NHWC ? j : oc;
        const float k = af.k[c], b = af.b[c];
        const unsigned char *s = NHWC ? stage + mis + px * C + af.order[c] : stage + mis + px;
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

// One lane per (n, oh, group of LANE_PX output columns); groups = ceil(OW / LANE_PX); total = N * OH * groups.
__global__ void __launch_bounds__(TPB) image_u8_resize_kernel(const unsigned char *x, float *y, size_t total, int H, int W, int C,
                                                              int Co, int OH, int OW, int groups, const int *ra, const float *rs,
                                                              const int *ca, const float *cs, Affine af, bool vec_store) {
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const size_t row = i / (size_t)groups;            // n * OH + oh
        const int ow0 = (int)(i - row * (size_t)groups) * LANE_PX;
        const size_t n = row / (size_t)OH;
        const int oh = (int)(row - n * (size_t)OH);
        const int cnt = min(LANE_PX, OW - ow0);
        const int r0 = min(max(ra[oh], 0), H - 2);
        const float fr = rs[oh], gr = __fsub_rn(1.f, fr);
        const unsigned char *top = x + (n * (size_t)H + (size_t)r0) * (size_t)W * (size_t)C;
        const unsigned char *bot = top + (size_t)W * (size_t)C;
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
            const float k = af.k[c], b = af.b[c];
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

}  // namespace image_input
