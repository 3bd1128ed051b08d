// Tiled whole-image inference around a plan (Net.tiled): the windows of one H x W x C image cut into the float32
// (S, Co, h, w) NCHW batch a plan reads, and the plan's (n, Co, oh, ow) window results blended into the whole output.  One
// launch each; both memory-bound.
//
// tile_windows_kernel: a lane owns LANE_PX consecutive pixels of ONE output plane's flat h w pixels (so consecutive lanes write
// consecutive floats of a plane: one float4 per lane and channel where the planes' floats are 16-byte aligned, h w % 4 == 0 and
// an aligned y, single floats otherwise) and walks the output channels.  Slot s shows window min(s, n - 1).  Window pixel (r, c)
// is working pixel (r0 + r, c0 + c), clamped into the working image: the source pixel itself, or -- with util.resize's sampling
// tables for the WHOLE working image -- its bilinear sample of the source in image_u8_resize_kernel's order of roundings, table
// entries clamped to [0, H - 2] / [0, W - 2].  Whatever the origins hold, nothing outside the image is read.  A window row's
// source is a contiguous run of w C bytes (floats) at an arbitrary offset: lanes read their own bytes (consecutive lanes,
// consecutive bytes), the source is at most a quarter of the bytes written.  uint8: y = fl(fl(r * k[c]) + b[c]) of source
// channel order[c] (image_input::Affine); float32: a copy, channel c of C == Co.
//
// tile_blend_kernel, in gather form: a lane owns LANE_PX consecutive columns of one output row and, per group of CHUNK planes,
// visits the windows that cover each of its pixels in grid order (row-major over gr x gc): acc = fl(v w) for window 0 of the
// grid, acc = fl(acc + fl(v w)) from acc = +0.0 for the others, count = the integer sum of w, result fl(acc / (float)count) -- the
// reference's loop (util.py:327-344: window 0 assigned, the others added to a zeroed buffer, one division), so a -0.0 stays -0.0
// under window 0 alone and becomes +0.0 elsewhere, as it does there.
// w = min(distance to the window's nearest edge, ramp) + 1.  The covering grid rows and columns are found by one scan of the
// origins per lane (first and last that cover), every window inside that range is tested on its own: any number of windows may
// cover a pixel, origins need not be evenly spaced.  No atomics, no zero-fill, no weight plane: every output element is written
// once.  A pixel no window covers gets 0 / 0 (the host refuses such grids).  Output forms: float32 (OH, OW, Co); uint8 through
// image_output::quantise, (OH, OW, Co') or (Co', OH, OW); uint8 labels through image_output::label_step (C == 1: > threshold).
//
// All offsets are size_t.
#pragma once
#include "common.h"
#include "device_utils.h"
#include "image_input_kernel.h"
#include "image_output_kernel.h"

namespace tile {

constexpr int TPB = PL_STREAM_TPB;
constexpr int LANE_PX = 4;
constexpr int CHUNK = 4;                                 // planes blended per visit of the covering windows
static_assert(image_output::LANE_PX == LANE_PX && image_output::MAX_CO == CHUNK, "label_step / store_px / Affine are shared");

enum { OUT_F32 = 0, OUT_U8_NHWC = 1, OUT_U8_NCHW = 2, OUT_LABELS = 3 };

struct Tables {
    const int *ra;
    const float *rs;
    const int *ca;
    const float *cs;
};

// One lane per (slot, group of LANE_PX plane pixels); groups = ceil(h w / LANE_PX); total = S * groups.
template <typename T, bool TABLES>
__global__ void __launch_bounds__(TPB) tile_windows_kernel(const T *x, float *y, size_t total, int H, int W, int C, int Co, int h, int w,
                                                           int WH, int WW, const int *R0, const int *C0, int n, unsigned groups,
                                                           Tables tb, image_input::Affine af, bool vec_store) {
    constexpr bool U8 = sizeof(T) == 1;
    const size_t stride = (size_t)gridDim.x * TPB;
    const size_t hw = (size_t)h * (size_t)w;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const size_t s = i / (size_t)groups;
        const size_t p0 = (i - s * (size_t)groups) * LANE_PX;
        const int cnt = (int)min((size_t)LANE_PX, hw - p0);
        const int win = (int)min(s, (size_t)(n - 1));
        const int r0 = R0[win], c0 = C0[win];
        int r = (int)(p0 / (size_t)w), c = (int)(p0 - (size_t)r * (size_t)w);
        size_t o00[LANE_PX];                              // offset of the (top left) source pixel's channel 0
        float fr[LANE_PX], fc[LANE_PX];
#pragma unroll
        for (int p = 0; p < LANE_PX; ++p) {               // (pixels past the plane: clamped like any other, not stored)
            const int rr = min(max(r0 + r, 0), WH - 1), cc = min(max(c0 + c, 0), WW - 1);
            if (TABLES) {
                const int a = min(max(tb.ra[rr], 0), H - 2), b = min(max(tb.ca[cc], 0), W - 2);
                o00[p] = ((size_t)a * (size_t)W + (size_t)b) * (size_t)C;
                fr[p] = tb.rs[rr], fc[p] = tb.cs[cc];
            } else {
                o00[p] = ((size_t)min(rr, H - 1) * (size_t)W + (size_t)min(cc, W - 1)) * (size_t)C;
                fr[p] = fc[p] = 0.f;
            }
            if (++c == w) c = 0, ++r;
        }
        const size_t down = (size_t)W * (size_t)C;
        for (int ch = 0; ch < Co; ++ch) {
            const int sc = U8 ? af.order[ch & (image_input::MAX_C - 1)] : ch;
            float v[LANE_PX];
#pragma unroll
            for (int p = 0; p < LANE_PX; ++p) {
                const T *q = x + o00[p] + (size_t)sc;
                if (TABLES) {
                    const float gc = __fsub_rn(1.f, fc[p]), gr = __fsub_rn(1.f, fr[p]);
                    const float tv = __fadd_rn(__fmul_rn((float)q[0], gc), __fmul_rn((float)q[C], fc[p]));
                    const float bv = __fadd_rn(__fmul_rn((float)q[down], gc), __fmul_rn((float)q[down + C], fc[p]));
                    v[p] = __fadd_rn(__fmul_rn(tv, gr), __fmul_rn(bv, fr[p]));
                } else {
                    v[p] = (float)q[0];
                }
                if (U8) v[p] = image_input::affine(v[p], af.k[ch & (image_input::MAX_C - 1)], af.b[ch & (image_input::MAX_C - 1)]);
            }
            float *dst = y + ((s * (size_t)Co + (size_t)ch) * hw + p0);
            if (vec_store && cnt == LANE_PX) {
                *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int p = 0; p < cnt; ++p) dst[p] = v[p];
            }
        }
    }
}

struct Blend {
    int n, C, oh, ow, gr, gc, OH, OW, ramp;
    int Co;                                               // output channels (OUT_U8_*), else C
    unsigned groups;                                      // ceil(OW / LANE_PX)
    float threshold;
    bool trunc;
};

// One lane per (output row, group of LANE_PX columns); total = OH * groups.
template <int MODE>
__global__ void __launch_bounds__(TPB) tile_blend_kernel(const float *x, void *yv, size_t total, const int *R0, const int *C0, Blend g,
                                                         image_output::Affine af) {
    constexpr bool IMAGE = MODE == OUT_U8_NHWC || MODE == OUT_U8_NCHW;
    const size_t stride = (size_t)gridDim.x * TPB;
    const size_t plane = (size_t)g.oh * (size_t)g.ow;
    const size_t OHW = (size_t)g.OH * (size_t)g.OW;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const int orow = (int)(i / (size_t)g.groups);
        const int col0 = (int)(i - (size_t)orow * (size_t)g.groups) * LANE_PX;
        const int cnt = min(LANE_PX, g.OW - col0);
        const int colN = col0 + cnt - 1;                  // the last column this lane stores
        // the grid rows / columns that can cover this lane's pixels: first and last whose extent meets them
        int gi0 = g.gr, gi1 = 0, gj0 = g.gc, gj1 = 0;
        for (int gi = 0; gi < g.gr; ++gi) {
            const int a = R0[(size_t)gi * (size_t)g.gc];
            if (orow >= a && orow - a < g.oh) gi0 = min(gi0, gi), gi1 = gi + 1;
        }
        for (int gj = 0; gj < g.gc; ++gj) {
            const int a = C0[gj];
            if (colN >= a && col0 - a < g.ow) gj0 = min(gj0, gj), gj1 = gj + 1;
        }
        float best[LANE_PX] = {0.f, 0.f, 0.f, 0.f};       // OUT_LABELS: the running maximum and its plane
        unsigned idx[LANE_PX] = {0, 0, 0, 0};
        const int planes = IMAGE ? g.Co : g.C;
        for (int cb = 0; cb < planes; cb += CHUNK) {
            const int nch = min(CHUNK, planes - cb);
            float acc[CHUNK][LANE_PX];
            int count[LANE_PX] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < CHUNK; ++j)
#pragma unroll
                for (int p = 0; p < LANE_PX; ++p) acc[j][p] = 0.f;
            for (int gi = gi0; gi < gi1; ++gi) {
                for (int gj = gj0; gj < gj1; ++gj) {
                    const size_t win = (size_t)gi * (size_t)g.gc + (size_t)gj;
                    const int r = orow - R0[win], wc0 = C0[win];
                    if (r < 0 || r >= g.oh) continue;
                    const int dr = min(r, g.oh - 1 - r);
#pragma unroll
                    for (int p = 0; p < LANE_PX; ++p) {
                        const int c = col0 + p - wc0;
                        if (p >= cnt || c < 0 || c >= g.ow) continue;
                        const int wi = min(min(dr, min(c, g.ow - 1 - c)), g.ramp) + 1;
                        const float wt = (float)wi;
                        const bool first = win == 0;          // (the reference assigns window 0 and adds the others to zeros)
                        count[p] += wi;
#pragma unroll
                        for (int j = 0; j < CHUNK; ++j) {
                            if (j >= nch) break;
                            const int sp = IMAGE ? af.order[j] : cb + j;
                            const float prod = __fmul_rn(x[(win * (size_t)g.C + (size_t)sp) * plane + (size_t)r * (size_t)g.ow + (size_t)c], wt);
                            acc[j][p] = first ? prod : __fadd_rn(acc[j][p], prod);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < CHUNK; ++j)
#pragma unroll
                for (int p = 0; p < LANE_PX; ++p) acc[j][p] = __fdiv_rn(acc[j][p], (float)count[p]);
            const size_t pix = (size_t)orow * (size_t)g.OW + (size_t)col0;
            if (MODE == OUT_F32) {
                float *y = reinterpret_cast<float *>(yv);
                for (int p = 0; p < cnt; ++p)
                    for (int j = 0; j < nch; ++j) y[(pix + (size_t)p) * (size_t)g.C + (size_t)(cb + j)] = acc[j][p];
            } else if (IMAGE) {
                unsigned char *y = reinterpret_cast<unsigned char *>(yv);
#pragma unroll
                for (int j = 0; j < CHUNK; ++j) {
                    if (j >= nch) break;
                    unsigned q[LANE_PX];
#pragma unroll
                    for (int p = 0; p < LANE_PX; ++p) q[p] = image_output::quantise(acc[j][p], af.k[j], af.b[j], g.trunc);
                    if (MODE == OUT_U8_NCHW) {
                        image_output::store_px(y + ((size_t)j * OHW + pix), cnt, q);
                    } else {
                        for (int p = 0; p < cnt; ++p) y[(pix + (size_t)p) * (size_t)g.Co + (size_t)j] = (unsigned char)q[p];
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < CHUNK; ++j) {
                    if (j >= nch) break;
                    if (cb + j == 0) {
#pragma unroll
                        for (int p = 0; p < LANE_PX; ++p) best[p] = acc[0][p];
                    } else {
                        image_output::label_step(best, idx, acc[j], (unsigned)(cb + j));
                    }
                }
            }
        }
        if (MODE == OUT_LABELS) {
            if (g.C == 1) {
#pragma unroll
                for (int p = 0; p < LANE_PX; ++p) idx[p] = best[p] > g.threshold ? 1u : 0u;
            }
            image_output::store_px(reinterpret_cast<unsigned char *>(yv) + (size_t)orow * (size_t)g.OW + (size_t)col0, cnt, idx);
        }
    }
}

}  // namespace tile
