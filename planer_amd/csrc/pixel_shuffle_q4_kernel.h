// Pixel shuffle / unshuffle (depth-to-space / space-to-depth) on channel-quad tensors.
//
// The NARROW side is (N, C, H, W), the WIDE side (N, C r^2, H/r, W/r); a shuffle goes wide -> narrow, an unshuffle back.
//   CRD (PyTorch PixelShuffle):  wide channel c r^2 + i r + j  <->  narrow channel c at pixel (h r + i, w r + j)
//   DCR (ONNX DepthToSpace):     wide channel (i r + j) C + c  <->  the same pixel                     (C % 4 == 0 only)
// CRD: the 4 r^2 wide channels of narrow quad Q are the wide quads Q r^2 .. Q r^2 + r^2 - 1, whatever C is, so the thread that
// owns (small pixel, narrow quad Q) holds r^2 float4 of one side, permutes them in registers (all indices static: r is a
// template parameter) and writes r^2 float4 of the other.  DCR with C % 4 == 0: narrow quad Q at block position (i, j) IS wide
// quad (i r + j) C/4 + Q, the same thread moves the same r^2 float4 without the permutation.
// With C % 4 != 0 the wide side has ceil(C r^2 / 4) quads: the slots past that do not exist -- never read, never written --
// and every lane of the output that stands for a channel >= C (narrow) or >= C r^2 (wide) is written as +0 whatever the input
// holds there.  Both conditions are one: narrow lane cl of quad Q is live iff 4 Q + cl < C.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace pixel_shuffle_q4 {

constexpr int TPB = PL_STREAM_TPB;

struct Geom {
    int C, Cq, CqW;      // narrow channels, narrow quads, wide quads
    int Hs, Ws;          // the wide side's map (H / r, W / r)
    FastDiv divWs, divHs, divCq;
};

// slot k (0 .. r^2 - 1) of narrow quad Q -> its wide quad
template <int R, int ORDER>
__device__ __forceinline__ unsigned wide_quad(unsigned Q, int k, int Cq) {
    return ORDER == 0 ? Q * (unsigned)(R * R) + (unsigned)k : (unsigned)k * (unsigned)Cq + Q;
}

// element (narrow lane cl, block position i, j) -> its place 4 k + l among the thread's 4 r^2 wide floats
template <int R, int ORDER>
__device__ __forceinline__ constexpr int wide_pos(int cl, int i, int j) {
    return ORDER == 0 ? cl * R * R + i * R + j : 4 * (i * R + j) + cl;
}

// One thread per (image, narrow quad, small pixel).  INVERSE 0: x wide, y narrow; 1: x narrow, y wide.  NCHW (shuffles only):
// y is the plain (N, C, H, W) tensor, r contiguous floats per (channel, row) and thread, padding channels not written.
template <int R, int ORDER, bool INVERSE, bool NCHW>
__global__ void __launch_bounds__(TPB) pixel_shuffle_q4_kernel(const float4 *x, float *yf, unsigned total, Geom g) {
    constexpr int R2 = R * R;
    float4 *y = (float4 *)yf;
    const int H = g.Hs * R, W = g.Ws * R;
    const unsigned stride = gridDim.x * TPB;
    for (unsigned t = blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {        // t = ((n Cq + Q) Hs + hs) Ws + ws
        unsigned row, ws, nq, hs, n, Q;
        g.divWs.divmod(t, row, ws);
        g.divHs.divmod(row, nq, hs);
        g.divCq.divmod(nq, n, Q);
        const int live = g.C - (int)(4 * Q);                     // narrow lanes 0 .. live - 1 hold channels
        const size_t wide_img = (size_t)n * g.CqW, narrow_plane = (size_t)n * g.Cq + Q;
        float v[4 * R2];                                          // wide order: v[4 k + l] = lane l of slot k
        if (!INVERSE) {
#pragma unroll
            for (int k = 0; k < R2; ++k) {
                const unsigned wq = wide_quad<R, ORDER>(Q, k, g.Cq);
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                if (wq < (unsigned)g.CqW) a = x[((wide_img + wq) * g.Hs + hs) * g.Ws + ws];
                v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                if (NCHW) {
#pragma unroll
                    for (int cl = 0; cl < 4; ++cl) {
                        if (cl >= live) break;
                        float *p = yf + (((size_t)n * g.C + 4 * Q + cl) * H + hs * R + i) * W + (size_t)ws * R;
                        if (R == 2) {                             // W is even and y 16-byte aligned: 8-byte aligned
                            *(float2 *)p = make_float2(v[wide_pos<R, ORDER>(cl, i, 0)], v[wide_pos<R, ORDER>(cl, i, 1)]);
                        } else if (R == 4) {
                            *(float4 *)p = make_float4(v[wide_pos<R, ORDER>(cl, i, 0)], v[wide_pos<R, ORDER>(cl, i, 1)],
                                                       v[wide_pos<R, ORDER>(cl, i, R - 2)], v[wide_pos<R, ORDER>(cl, i, R - 1)]);
                        } else {
#pragma unroll
                            for (int j = 0; j < R; ++j) p[j] = v[wide_pos<R, ORDER>(cl, i, j)];
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < R; ++j) {
                        float4 o;
                        o.x = live > 0 ? v[wide_pos<R, ORDER>(0, i, j)] : 0.f;
                        o.y = live > 1 ? v[wide_pos<R, ORDER>(1, i, j)] : 0.f;
                        o.z = live > 2 ? v[wide_pos<R, ORDER>(2, i, j)] : 0.f;
                        o.w = live > 3 ? v[wide_pos<R, ORDER>(3, i, j)] : 0.f;
                        y[(narrow_plane * H + hs * R + i) * W + (size_t)ws * R + j] = o;
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float4 a = x[(narrow_plane * H + hs * R + i) * W + (size_t)ws * R + j];
                    v[wide_pos<R, ORDER>(0, i, j)] = live > 0 ? a.x : 0.f;
                    v[wide_pos<R, ORDER>(1, i, j)] = live > 1 ? a.y : 0.f;
                    v[wide_pos<R, ORDER>(2, i, j)] = live > 2 ? a.z : 0.f;
                    v[wide_pos<R, ORDER>(3, i, j)] = live > 3 ? a.w : 0.f;
                }
#pragma unroll
            for (int k = 0; k < R2; ++k) {
                const unsigned wq = wide_quad<R, ORDER>(Q, k, g.Cq);
                if (wq < (unsigned)g.CqW)
                    y[((wide_img + wq) * g.Hs + hs) * g.Ws + ws] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
            }
        }
    }
}

}  // namespace pixel_shuffle_q4
