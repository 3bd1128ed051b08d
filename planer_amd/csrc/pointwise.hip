// HBM-bound kernels of planer's forward pass: BatchNorm, ReLU, LeakyReLU,
// Sigmoid, Add, Maxpool/AveragePool, nearest UpSample, Concat copies, global
// average pool and the split-K combine.  Each moves its algorithmic bytes
// once: 16-byte vector loads/stores, grid capped near 8 blocks per CU with a
// grid-stride loop, wave64 shuffles for the one reduction.
#include "common.h"
#include "device_utils.h"
#include "instnorm_q4_kernel.h"
#include "groupnorm_q4_kernel.h"
#include "pixel_shuffle_q4_kernel.h"
#include "image_input_kernel.h"
#include "image_output_kernel.h"
#include "detect_kernel.h"
#include "components_kernel.h"
#include "flow_kernel.h"
#include "text_kernel.h"
#include "peaks_kernel.h"
#include "tile_kernel.h"

namespace {

constexpr int TPB = PL_STREAM_TPB;

inline unsigned stream_grid(pl_ctx *ctx, size_t work_items) { return pl_stream_grid(ctx->cu_count, work_items); }
inline bool loop32_ok(pl_ctx *ctx, size_t total) { return pl_loop32_ok(ctx->cu_count, total); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- unary / binary elementwise -----------------------------------------
struct OpRelu {
    __device__ float operator()(float x) const { return relu_ref(x); }
};
struct OpLeaky {
    float a, b;
    __device__ float operator()(float x) const { return leaky_ref(x, a, b); }
};
struct OpSigmoid {
    // 1/(1+exp(-x)) with an accurate expf; exp overflow gives inf -> result 0
    __device__ float operator()(float x) const { return __fdiv_rn(1.f, __fadd_rn(expf(-x), 1.f)); }
};

template <class Op>
__global__ void __launch_bounds__(TPB) unary_vec4(const float4 *x, float4 *y, size_t n4, Op op) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
        float4 v = x[i];
        v.x = op(v.x); v.y = op(v.y); v.z = op(v.z); v.w = op(v.w);
        y[i] = v;
    }
}

template <class Op>
__global__ void __launch_bounds__(TPB) unary_scalar(const float *x, float *y, size_t n, Op op) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) y[i] = op(x[i]);
}

template <class Op>
int launch_unary(pl_ctx *ctx, const float *x, float *y, size_t n, Op op) {
    PL_REQUIRE(ctx && (n == 0 || (x && y)), PL_EINVAL, "elementwise: null argument");
    if (!n) return PL_OK;
    CtxGuard g(ctx);
    size_t n4 = 0;
    if (aligned16(x) && aligned16(y)) {
        n4 = n / 4;
        if (n4) unary_vec4<<<stream_grid(ctx, n4), TPB, 0, ctx->stream>>>((const float4 *)x, (float4 *)y, n4, op);
    }
    size_t done = n4 * 4;
    if (done < n) unary_scalar<<<stream_grid(ctx, n - done), TPB, 0, ctx->stream>>>(x + done, y + done, n - done, op);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

__global__ void __launch_bounds__(TPB) add_vec4(const float4 *a, const float4 *b, float4 *y, size_t n4) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n4; i += stride) {
        float4 u = a[i], v = b[i];
        y[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    }
}

__global__ void __launch_bounds__(TPB) add_scalar(const float *a, const float *b, float *y, size_t n) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) y[i] = a[i] + b[i];
}

// ---- per-channel affine (BatchNorm) and channel-broadcast add -------------
// x viewed as (outer, C, inner); one block row per (outer, c) plane chunk so
// the channel lookup is uniform per block instead of a division per element.
template <bool HAS_SCALE>
__global__ void __launch_bounds__(TPB) affine_plane(const float *x, float *y, const float *scale,
                                                    const float *shift, int C, int inner, FastDiv divC) {
    // blockIdx.y = plane (outer*C + c), blockIdx.x strides over the plane
    const unsigned plane = blockIdx.y;
    const unsigned c = plane - divC.div(plane) * (unsigned)C;
    const float s = HAS_SCALE ? scale[c] : 1.f;
    const float t = shift ? shift[c] : 0.f;
    const float *xp = x + (size_t)plane * inner;
    float *yp = y + (size_t)plane * inner;
    // unsigned: inner < 2^31 and the stride is about inner / 4, so i + stride stays below 2^32 (a signed i overflowed)
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < (unsigned)inner; i += stride) {
        float v = xp[i];
        if (HAS_SCALE) v = __fmul_rn(v, s);
        yp[i] = __fadd_rn(v, t);
    }
}

// flat form for small planes (e.g. 7x7): 4 consecutive elements per thread
template <bool HAS_SCALE>
__global__ void __launch_bounds__(TPB) affine_flat(const float *x, float *y, const float *scale,
                                                   const float *shift, size_t n, int C, FastDiv divInner,
                                                   FastDiv divC) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        unsigned plane = divInner.div((unsigned)i);
        unsigned c = plane - divC.div(plane) * (unsigned)C;
        float v = x[i];
        if (HAS_SCALE) v = __fmul_rn(v, scale[c]);
        y[i] = __fadd_rn(v, shift ? shift[c] : 0.f);
    }
}

template <bool HAS_SCALE>
int launch_affine(pl_ctx *ctx, const float *x, float *y, const float *scale, const float *shift,
                  int outer, int C, int inner) {
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "affine: null argument");
    PL_REQUIRE(outer >= 0 && C > 0 && inner > 0, PL_EINVAL, "affine: bad shape");
    size_t n = (size_t)outer * C * inner;
    if (!n) return PL_OK;
    PL_REQUIRE(n < (1ull << 32), PL_EUNSUPPORTED, "affine: tensor too large");
    CtxGuard g(ctx);
    size_t planes = (size_t)outer * C;
    if (inner >= 1024 && planes <= 65535) {
        dim3 grid(cdiv(inner, TPB * 4) ? cdiv(inner, TPB * 4) : 1, (unsigned)planes);
        affine_plane<HAS_SCALE><<<grid, TPB, 0, ctx->stream>>>(x, y, scale, shift, C, inner, FastDiv(C));
    } else {
        affine_flat<HAS_SCALE><<<stream_grid(ctx, n), TPB, 0, ctx->stream>>>(x, y, scale, shift, n, C,
                                                                         FastDiv(inner), FastDiv(C));
    }
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// ---- pooling ---------------------------------------------------------------
// util.pool (util.py:79-92): zero padding; max accumulator starts at -1e4.
template <int MODE>
__global__ void __launch_bounds__(TPB) pool2d_kernel(const float *x, float *y, unsigned total, int H, int W,
                                                     int Ho, int Wo, int kh, int kw, int sh, int sw, int pt,
                                                     int pl, FastDiv divWo, FastDiv divHo) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ow, nc, oh;
        divWo.divmod(i, row, ow);
        divHo.divmod(row, nc, oh);
        const float *xp = x + (size_t)nc * H * W;
        float acc = MODE == 0 ? -1e4f : 0.f;
        int h0 = (int)oh * sh - pt, w0 = (int)ow * sw - pl;
        for (int r = 0; r < kh; ++r) {
            int hi = h0 + r;
            bool hok = (unsigned)hi < (unsigned)H;
            for (int q = 0; q < kw; ++q) {
                int wi = w0 + q;
                float v = (hok && (unsigned)wi < (unsigned)W) ? xp[(size_t)hi * W + wi] : 0.f;
                acc = MODE == 0 ? max_nan(v, acc) : acc + v;
            }
        }
        if (MODE == 1) acc = __fdiv_rn(acc, (float)(kh * kw));
        y[i] = acc;
    }
}

// 3x3 / stride 2 / pad 1 on an even-sized map (ResNet's stem pool): one thread
// produces 4 neighbouring outputs from 3 rows x (two aligned float4 + one scalar),
// 9 load instructions instead of 36, one float4 store.  Same semantics as above:
// padding contributes 0, accumulator starts at -1e4 (util.py:88,95).
__global__ void __launch_bounds__(TPB) maxpool_k3s2p1_x4(const float *x, float *y, unsigned total4, int H, int W,
                                                         int Ho, int Wo4, FastDiv divWo4, FastDiv divHo) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total4; i += stride) {
        unsigned row, q, nc, oh;
        divWo4.divmod(i, row, q);
        divHo.divmod(row, nc, oh);
        const int wi0 = (int)q * 8;                         // first input column of the aligned pair
        const float *xp = x + (size_t)nc * H * W + wi0;
        float4 acc = make_float4(-1e4f, -1e4f, -1e4f, -1e4f);
        const bool top_pad = oh == 0;                       // row -1 is padding
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int hi = (int)oh * 2 - 1 + r;
            if (hi < 0) continue;
            const float *rp = xp + (size_t)hi * W;
            const float4 a = *reinterpret_cast<const float4 *>(rp);
            const float4 b = *reinterpret_cast<const float4 *>(rp + 4);
            const float l = q ? rp[-1] : 0.f;               // column -1 is padding
            acc.x = max_nan(acc.x, max_nan(l, max_nan(a.x, a.y)));
            acc.y = max_nan(acc.y, max_nan(a.y, max_nan(a.z, a.w)));
            acc.z = max_nan(acc.z, max_nan(a.w, max_nan(b.x, b.y)));
            acc.w = max_nan(acc.w, max_nan(b.y, max_nan(b.z, b.w)));
        }
        if (top_pad) {
            acc.x = max_nan(acc.x, 0.f); acc.y = max_nan(acc.y, 0.f); acc.z = max_nan(acc.z, 0.f); acc.w = max_nan(acc.w, 0.f);
        }
        *reinterpret_cast<float4 *>(y + (size_t)row * (Wo4 * 4) + q * 4) = acc;
    }
}

// ---- nearest upsample --------------------------------------------------------
__global__ void __launch_bounds__(TPB) upsample_kernel(const float *x, float *y, unsigned total, int H, int W,
                                                       int OH, int OW, FastDiv divOW, FastDiv divOH,
                                                       FastDiv divFh, FastDiv divFw) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ow, nc, oh;
        divOW.divmod(i, row, ow);
        divOH.divmod(row, nc, oh);
        y[i] = x[((size_t)nc * H + divFh.div(oh)) * W + divFw.div(ow)];
    }
}

// ---- strided row copy (concat) -------------------------------------------------
__global__ void __launch_bounds__(TPB) copy2d_vec4(float4 *dst, size_t dst_pitch4, const float4 *src,
                                                   size_t src_pitch4, unsigned width4, unsigned total4,
                                                   FastDiv divW) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total4; i += stride) {
        unsigned r, c;
        divW.divmod(i, r, c);
        dst[(size_t)r * dst_pitch4 + c] = src[(size_t)r * src_pitch4 + c];
    }
}

__global__ void __launch_bounds__(TPB) copy2d_scalar(float *dst, size_t dst_pitch, const float *src,
                                                     size_t src_pitch, unsigned width, unsigned total,
                                                     FastDiv divW) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned r, c;
        divW.divmod(i, r, c);
        dst[(size_t)r * dst_pitch + c] = src[(size_t)r * src_pitch + c];
    }
}

// ---- global average pool: one wave64 per (n,c) row ------------------------------
__global__ void __launch_bounds__(TPB) gap_kernel(const float *x, float *y, int rows, int inner, float inv) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * TPB + threadIdx.x) >> 6;
    const unsigned nwaves = (gridDim.x * TPB) >> 6;
    for (unsigned r = wave; r < (unsigned)rows; r += nwaves) {      // unsigned: rows <= 2^31 - 1, so r + nwaves cannot wrap
        const float *xp = x + (size_t)r * inner;
        float s = 0.f;
        for (unsigned i = lane; i < (unsigned)inner; i += 64) s += xp[i];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) y[r] = s * inv;
    }
}

// ---- split-K combine + fused conv tail ---------------------------------------------
__global__ void __launch_bounds__(TPB) splitk_reduce_kernel(const float *ws, int splits, size_t slab, float *y,
                                                            unsigned total, int C, FastDiv divInner,
                                                            FastDiv divC, Epilogue ep) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        float v = ws[i];
        for (int z = 1; z < splits; ++z) v += ws[(size_t)z * slab + i];
        unsigned plane = divInner.div(i);
        unsigned c = plane - divC.div(plane) * (unsigned)C;
        y[i] = apply_epilogue(ep, v, (int)c, i);
    }
}

// ---- channel-quad (Q4) variants ---------------------------------------------------
// Same semantics as the kernels above on tensors stored [N][C/4][H][W][4] (include/planer_hip.h):
// every thread handles one pixel of one channel quad, i.e. one float4 per tap.  Padding lanes of
// the last quad stay zero: max(-1e4, 0, ...) = 0, 0-sums, and the affine kernel writes them as 0.
__device__ __forceinline__ float4 f4max(float4 a, float4 b) {
    return make_float4(max_nan(a.x, b.x), max_nan(a.y, b.y), max_nan(a.z, b.z), max_nan(a.w, b.w));
}
__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

template <int MODE>
__global__ void __launch_bounds__(TPB) pool2d_q4_kernel(const float4 *x, float4 *y, unsigned total, int H, int W,
                                                        int Ho, int Wo, int kh, int kw, int sh, int sw, int pt,
                                                        int pl, FastDiv divWo, FastDiv divHo) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ow, nc, oh;
        divWo.divmod(i, row, ow);
        divHo.divmod(row, nc, oh);
        const float4 *xp = x + (size_t)nc * H * W;
        const float init = MODE == 0 ? -1e4f : 0.f;
        float4 acc = make_float4(init, init, init, init);
        const int h0 = (int)oh * sh - pt, w0 = (int)ow * sw - pl;
        for (int r = 0; r < kh; ++r) {
            const int hi = h0 + r;
            const bool hok = (unsigned)hi < (unsigned)H;
            for (int q = 0; q < kw; ++q) {
                const int wi = w0 + q;
                const float4 v = (hok && (unsigned)wi < (unsigned)W) ? xp[(size_t)hi * W + wi] : make_float4(0.f, 0.f, 0.f, 0.f);
                acc = MODE == 0 ? f4max(v, acc) : f4add(acc, v);
            }
        }
        if (MODE == 1) {
            const float d = (float)(kh * kw);
            acc = make_float4(__fdiv_rn(acc.x, d), __fdiv_rn(acc.y, d), __fdiv_rn(acc.z, d), __fdiv_rn(acc.w, d));
        }
        y[i] = acc;
    }
}

// 3x3 / stride 2 / pad 1 max pool (ResNet's stem pool) on Q4: a thread owns TWO vertically adjacent outputs and
// reads its 5x3 input window once (15 float4 instead of 18; an input row is fetched for 2 output rows instead of
// 1.5) while consecutive lanes stay consecutive output columns -- the generic kernel above re-read 23 % of its input
// from HBM (profiles/r01_hbm_traffic.md).  Same zero padding, -1e4 start and per-output accumulation order as
// pool2d_q4_kernel<0> (util.py:79-95), so results are bit-identical.
__global__ void __launch_bounds__(TPB) maxpool_q4_k3s2p1_2x1(const float4 *x, float4 *y, unsigned total, int H, int W,
                                                             int Ho, int Wo, int Hb, unsigned x_bytes, FastDiv divWo,
                                                             FastDiv divHb) {
    const unsigned stride = gridDim.x * TPB;
    // the zero padding comes from the buffer's range check (an out-of-window lane gets an out-of-range offset):
    // all 15 loads of a thread are in flight together, no branch per element
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(x), 0, x_bytes, 0x00020000);
    constexpr int OOB = (int)0x80000000;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {      // i = (nc*Hb + a)*Wo + ow
        unsigned row, ow, nc, a;
        divWo.divmod(i, row, ow);
        divHb.divmod(row, nc, a);
        const int h0 = 4 * (int)a - 1, w0 = 2 * (int)ow - 1;
        const int base = (int)nc * H * W;                                            // in float4s; < 2^27 (host check)
        float4 v[5][3];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int hi = h0 + r;
            const bool hok = (unsigned)hi < (unsigned)H;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int wi = w0 + q;
                const bool ok = hok && (unsigned)wi < (unsigned)W;
                v[r][q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, ok ? (base + hi * W + wi) << 4 : OOB, 0, 0));
            }
        }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int oh = 2 * (int)a + dy;
            if (oh >= Ho) continue;
            float4 acc = make_float4(-1e4f, -1e4f, -1e4f, -1e4f);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc = f4max(v[2 * dy + r][q], acc);
            y[((size_t)nc * Ho + oh) * Wo + ow] = acc;
        }
    }
}

__global__ void __launch_bounds__(TPB) upsample_q4_kernel(const float4 *x, float4 *y, unsigned total, int H, int W,
                                                          int OH, int OW, FastDiv divOW, FastDiv divOH,
                                                          FastDiv divFh, FastDiv divFw) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ow, nc, oh;
        divOW.divmod(i, row, ow);
        divOH.divmod(row, nc, oh);
        y[i] = x[((size_t)nc * H + divFh.div(oh)) * W + divFw.div(ow)];
    }
}

// Pixel-phase re-layout of a channel-quad tensor.  A tensor "folded by (dh, dw)" holds the (N, C, H, W) activation
// as N*dh*dw images of ceil(H/dh) x ceil(W/dw) pixels: image (n*dh + i)*dw + j, pixel (r, c) = x[n, :, r*dh + i, c*dw + j], zero
// where that coordinate lies outside H x W.  One output quad per lane, consecutive lanes store consecutive quads; the gather is
// on the read side (a 16-byte store at a 64-byte stride runs at a third of a contiguous one's rate, profiles/r04_pointwise_gbs.md).
// Every output quad is written, the zero-fill cells included; a coordinate inside H x W never maps to a zero-fill cell of the
// input, so those -- junk behind a conv -- are never read.
__global__ void __launch_bounds__(TPB) refold_q4_kernel(const float4 *x, float4 *y, unsigned total, int Cq, int H, int W, int Hi,
                                                        int Wi, int dih, int diw, int doh, int dow, FastDiv divWo, FastDiv divHo,
                                                        FastDiv divCq, FastDiv divDow, FastDiv divDoh, FastDiv divDih,
                                                        FastDiv divDiw) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {      // i = ((m*Cq + q)*Ho + r)*Wo + c
        unsigned row, c, mq, r, m, q, t, jo, n, io;
        divWo.divmod(i, row, c);
        divHo.divmod(row, mq, r);
        divCq.divmod(mq, m, q);
        divDow.divmod(m, t, jo);
        divDoh.divmod(t, n, io);
        const unsigned py = r * (unsigned)doh + io, px = c * (unsigned)dow + jo;      // the unfolded pixel
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (py < (unsigned)H && px < (unsigned)W) {
            unsigned ri, ii, ci, ji;
            divDih.divmod(py, ri, ii);
            divDiw.divmod(px, ci, ji);
            const size_t mi = ((size_t)n * dih + ii) * diw + ji;
            v = x[((mi * Cq + q) * Hi + ri) * Wi + ci];
        }
        y[i] = v;
    }
}

// layer.Concatenate (layer.py:90-91) of TWO channel-quad tensors along channels in one launch, the first one optionally
// nearest-upsampled by (fh, fw) on the way (layer.UpSample, layer.py:80-82 -> util.upsample_nearest): the route layers of
// a detection net -- upsample -> concat -- are one pass over the output instead of three kernels.
__global__ void __launch_bounds__(TPB) concat2_q4_kernel(const float4 *a, const float4 *b, float4 *y, unsigned total, int qa,
                                                         int qb, int H, int W, int Ha, int Wa, FastDiv divHW, FastDiv divQ,
                                                         FastDiv divW, FastDiv divFh, FastDiv divFw) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {      // i = (n*(qa+qb) + q)*H*W + pix
        unsigned r, pix, n, q;
        divHW.divmod(i, r, pix);
        divQ.divmod(r, n, q);
        if ((int)q < qa) {
            unsigned oh, ow;
            divW.divmod(pix, oh, ow);
            y[i] = a[(((size_t)n * qa + q) * Ha + divFh.div(oh)) * Wa + divFw.div(ow)];
        } else {
            y[i] = b[((size_t)n * qb + (q - qa)) * (size_t)(H * W) + pix];
        }
    }
}

// global average pool: one wave64 per (n, channel quad); output is plain [N][C]
__global__ void __launch_bounds__(TPB) gap_q4_kernel(const float4 *x, float *y, int rows, int Cq, int C, int inner,
                                                     float inv) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * TPB + threadIdx.x) >> 6;
    const unsigned nwaves = (gridDim.x * TPB) >> 6;
    for (unsigned r = wave; r < (unsigned)rows; r += nwaves) {      // unsigned: rows <= 2^31 - 1, so r + nwaves cannot wrap
        const float4 *xp = x + (size_t)r * inner;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (unsigned i = lane; i < (unsigned)inner; i += 64) s = f4add(s, xp[i]);
        for (int off = 32; off > 0; off >>= 1) {
            s.x += __shfl_down(s.x, off, 64); s.y += __shfl_down(s.y, off, 64);
            s.z += __shfl_down(s.z, off, 64); s.w += __shfl_down(s.w, off, 64);
        }
        if (lane == 0) {
            const int n = (int)(r / (unsigned)Cq), cq = (int)(r - (unsigned)n * (unsigned)Cq);
            float *yp = y + (size_t)n * C + cq * 4;
            const int left = C - cq * 4;
            yp[0] = s.x * inv;
            if (left > 1) yp[1] = s.y * inv;
            if (left > 2) yp[2] = s.z * inv;
            if (left > 3) yp[3] = s.w * inv;
        }
    }
}

// BatchNorm (layer.py:125-127) on a Q4 tensor: y = x*scale[c] + shift[c], two roundings
__global__ void __launch_bounds__(TPB) affine_q4_kernel(const float4 *x, float4 *y, const float *scale,
                                                        const float *shift, unsigned total, int C, int Cq,
                                                        FastDiv divInner, FastDiv divCq) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        const unsigned plane = divInner.div(i);
        const int cq = (int)(plane - divCq.div(plane) * (unsigned)Cq);
        const float4 v = x[i];
        float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = cq * 4 + e;
            r[e] = c < C ? __fadd_rn(__fmul_rn(r[e], scale[c]), shift[c]) : 0.f;
        }
        y[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// ---- second-wave operators -----------------------------------
struct OpMath {
    int op;       // 0 exp 1 log 2 tanh 3 sqrt 4 reciprocal 5 hardsigmoid 6 clip
    float p0, p1;
    __device__ float operator()(float x) const {
        switch (op) {
            case 0: return expf(x);
            case 1: return logf(x);
            case 2: return tanhf(x);
            case 3: return sqrtf(x);   // correctly rounded (hipcc default)
            case 4: return __fdiv_rn(1.f, x);
            case 5: return max_nan(min_nan(__fadd_rn(__fmul_rn(x, p0), p1), 1.f), 0.f);   // layer.py:66-69
            default: return max_nan(min_nan(x, p1), p0);                                     // layer.py:250-251
        }
    }
};

__device__ __forceinline__ float bin_op(int op, float a, float b) {
    switch (op) {
        case 0: return __fadd_rn(a, b);
        case 1: return __fsub_rn(a, b);
        case 2: return __fmul_rn(a, b);
        case 3: return __fdiv_rn(a, b);
        default: return powf(a, b);
    }
}

// y = a (op) b with each operand either full-size, one value per channel, or a single value
__global__ void __launch_bounds__(TPB) binary_kernel(const float *a, const float *b, float *y, size_t n, int C, int op,
                                                     int amode, int bmode, FastDiv divInner, FastDiv divC) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        unsigned c = 0;
        if (amode == 1 || bmode == 1) {
            const unsigned plane = divInner.div((unsigned)i);
            c = plane - divC.div(plane) * (unsigned)C;
        }
        const float av = amode == 0 ? a[i] : amode == 1 ? a[c] : a[0];
        const float bv = bmode == 0 ? b[i] : bmode == 1 ? b[c] : b[0];
        y[i] = bin_op(op, av, bv);
    }
}

// y = a (op) b under numpy broadcasting (layer.py:93-111): the result's index, axis by axis, addresses each operand
// through its own strides -- 0 on an axis the operand is broadcast over.
struct BcastArgs {
    int ndim;
    unsigned shape[6];
    long long sa[6], sb[6];
};

__global__ void __launch_bounds__(TPB) binary_bcast_kernel(const float *a, const float *b, float *y, size_t n, int op,
                                                           BcastArgs p) {
    size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += stride) {
        unsigned rem = (unsigned)i;
        long long ia = 0, ib = 0;
        for (int d = p.ndim - 1; d >= 0; --d) {
            const unsigned q = rem / p.shape[d], t = rem - q * p.shape[d];
            rem = q;
            ia += (long long)t * p.sa[d];
            ib += (long long)t * p.sb[d];
        }
        y[i] = bin_op(op, a[ia], b[ib]);
    }
}

// layer.UpSample / Resize, mode "linear", integer factors (util.py:121-153 upsample_blinear): the map is
// edge-replicated by one pixel, every 2 x 2 neighbourhood (i, j) of it yields an fh x fw block
//   lt*w[0][a][b] + rt*w[1][a][b] + lb*w[2][a][b] + rb*w[3][a][b]
// and the result is that field cropped by fh/2, fw/2.  The weights are the reference's float16 table, handed in
// by the host as floats.  With a factor of 1 on one axis only the other axis is interpolated (two terms).
struct UpLinArgs {
    int H, W, fh, fw, terms;   // terms: 4 both axes, 2 one axis
    float w[4 * 64];
};

// Where output pixel (oy, ox) of the integer-factor map samples: clamped rows r0 / r1, columns c0 / c1 and the offset of its
// weights in the (terms, fh, fw) table.  Shared by the NCHW kernel and its channel-quad twin.
struct UpLinTap {
    int r0, r1, c0, c1, wofs;
};

__device__ __forceinline__ UpLinTap uplin_tap(const UpLinArgs &p, int oy, int ox) {
    UpLinTap t;
    t.r0 = oy; t.r1 = oy; t.c0 = ox; t.c1 = ox;
    int a = 0, b = 0;
    if (p.fh > 1) {
        const int Y = oy + p.fh / 2, q = Y / p.fh;
        a = Y - q * p.fh;
        t.r0 = max(q - 1, 0);
        t.r1 = min(q, p.H - 1);
    }
    if (p.fw > 1) {
        const int X = ox + p.fw / 2, q = X / p.fw;
        b = X - q * p.fw;
        t.c0 = max(q - 1, 0);
        t.c1 = min(q, p.W - 1);
    }
    t.wofs = a * p.fw + b;
    return t;
}

// One component of the integer-factor interpolation.  The chain starts from +0 like the oracle's matrix product: an all -0
// neighbourhood gives +0, not -0.  Four terms: lt, rt, lb, rb; two terms: (a, b) are the two samples of the one axis.
__device__ __forceinline__ float uplin4(float lt, float rt, float lb, float rb, const float *w, int kk) {
    float v = __fmaf_rn(lt, w[0], 0.f);
    v = __fmaf_rn(rt, w[kk], v);
    v = __fmaf_rn(lb, w[2 * kk], v);
    return __fmaf_rn(rb, w[3 * kk], v);
}

__device__ __forceinline__ float uplin2(float a, float b, const float *w, int kk) {
    return __fmaf_rn(b, w[kk], __fmaf_rn(a, w[0], 0.f));
}

// One component of the fractional interpolation: columns first, a*(1-fc) + b*fc, then rows on those -- the reference's order of
// roundings.
__device__ __forceinline__ float resize_lerp(float lt, float rt, float lb, float rb, float fc, float gc, float fr, float gr) {
    const float top = __fadd_rn(__fmul_rn(lt, gc), __fmul_rn(rt, fc));
    const float bot = __fadd_rn(__fmul_rn(lb, gc), __fmul_rn(rb, fc));
    return __fadd_rn(__fmul_rn(top, gr), __fmul_rn(bot, fr));
}

__global__ void __launch_bounds__(TPB) upsample_linear_kernel(const float *x, float *y, unsigned total, UpLinArgs p,
                                                              FastDiv divOW, FastDiv divOH) {
    const unsigned stride = gridDim.x * TPB;
    const int kk = p.fh * p.fw;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ox, plane, oy;
        divOW.divmod(i, row, ox);
        divOH.divmod(row, plane, oy);
        const float *xp = x + (size_t)plane * p.H * p.W;
        const UpLinTap t = uplin_tap(p, (int)oy, (int)ox);
        const float *w = p.w + t.wofs;
        float v;
        if (p.terms == 4)
            v = uplin4(xp[(size_t)t.r0 * p.W + t.c0], xp[(size_t)t.r0 * p.W + t.c1], xp[(size_t)t.r1 * p.W + t.c0],
                       xp[(size_t)t.r1 * p.W + t.c1], w, kk);
        else if (p.fw > 1)
            v = uplin2(xp[(size_t)t.r0 * p.W + t.c0], xp[(size_t)t.r0 * p.W + t.c1], w, kk);
        else
            v = uplin2(xp[(size_t)t.r0 * p.W + t.c0], xp[(size_t)t.r1 * p.W + t.c0], w, kk);
        y[i] = v;
    }
}

// layer.UpSample / Resize, mode "linear", fractional factors (util.py:194-219 upsample_size) on (planes, H, W):
// columns first, a*(1-cs) + b*cs, then rows on those -- the reference's order of roundings.  Sample positions
// come from the host (float32 linspace, clip, floor).
__global__ void __launch_bounds__(TPB) resize_planes_kernel(const float *x, float *y, unsigned total, int H, int W,
                                                            const int *ra, const float *rs, const int *ca,
                                                            const float *cs, FastDiv divOW, FastDiv divOH) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ox, plane, oy;
        divOW.divmod(i, row, ox);
        divOH.divmod(row, plane, oy);
        const int r0 = ra[oy], c0 = ca[ox];
        const float fr = rs[oy], fc = cs[ox];
        const float gc = __fsub_rn(1.f, fc), gr = __fsub_rn(1.f, fr);
        const float *p0 = x + ((size_t)plane * H + r0) * W + c0, *p1 = p0 + W;
        y[i] = resize_lerp(p0[0], p0[1], p1[0], p1[1], fc, gc, fr, gr);
    }
}

// The channel-quad twins: one output quad per lane, i = ((n*Cq + q)*OH + oy)*OW + ox, consecutive lanes store
// consecutive quads; the gather is on the read side, where the fh*fw outputs of a neighbourhood hit the same four input quads in
// cache.  Per component the arithmetic is the NCHW kernel's (the helpers above), so zero lanes stay +0.  `res`, where given, is
// added in the write pass as a rounding of its own -- never contracted into the last fma -- so the step equals the upsample
// followed by an add bit for bit.
__device__ __forceinline__ float4 q4_add_res(float4 v, const float4 *res, unsigned i) {
    if (res) {
        const float4 r = res[i];
        v.x = __fadd_rn(v.x, r.x); v.y = __fadd_rn(v.y, r.y); v.z = __fadd_rn(v.z, r.z); v.w = __fadd_rn(v.w, r.w);
    }
    return v;
}

__global__ void __launch_bounds__(TPB) upsample_linear_q4_kernel(const float4 *x, float4 *y, const float4 *res, unsigned total,
                                                                 UpLinArgs p, FastDiv divOW, FastDiv divOH) {
    const unsigned stride = gridDim.x * TPB;
    const int kk = p.fh * p.fw;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ox, plane, oy;
        divOW.divmod(i, row, ox);
        divOH.divmod(row, plane, oy);
        const float4 *xp = x + (size_t)plane * p.H * p.W;
        const UpLinTap t = uplin_tap(p, (int)oy, (int)ox);
        const float *w = p.w + t.wofs;
        float4 v;
        if (p.terms == 4) {
            const float4 lt = xp[(size_t)t.r0 * p.W + t.c0], rt = xp[(size_t)t.r0 * p.W + t.c1];
            const float4 lb = xp[(size_t)t.r1 * p.W + t.c0], rb = xp[(size_t)t.r1 * p.W + t.c1];
            v.x = uplin4(lt.x, rt.x, lb.x, rb.x, w, kk); v.y = uplin4(lt.y, rt.y, lb.y, rb.y, w, kk);
            v.z = uplin4(lt.z, rt.z, lb.z, rb.z, w, kk); v.w = uplin4(lt.w, rt.w, lb.w, rb.w, w, kk);
        } else {
            const float4 a = xp[(size_t)t.r0 * p.W + t.c0];
            const float4 b = p.fw > 1 ? xp[(size_t)t.r0 * p.W + t.c1] : xp[(size_t)t.r1 * p.W + t.c0];
            v.x = uplin2(a.x, b.x, w, kk); v.y = uplin2(a.y, b.y, w, kk);
            v.z = uplin2(a.z, b.z, w, kk); v.w = uplin2(a.w, b.w, w, kk);
        }
        y[i] = q4_add_res(v, res, i);
    }
}

__global__ void __launch_bounds__(TPB) resize_linear_q4_kernel(const float4 *x, float4 *y, const float4 *res, unsigned total,
                                                               int H, int W, const int *ra, const float *rs, const int *ca,
                                                               const float *cs, FastDiv divOW, FastDiv divOH) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned row, ox, plane, oy;
        divOW.divmod(i, row, ox);
        divOH.divmod(row, plane, oy);
        const int r0 = ra[oy], c0 = ca[ox];
        const float fr = rs[oy], fc = cs[ox];
        const float gc = __fsub_rn(1.f, fc), gr = __fsub_rn(1.f, fr);
        const float4 *p0 = x + ((size_t)plane * H + r0) * W + c0, *p1 = p0 + W;
        const float4 lt = p0[0], rt = p0[1], lb = p1[0], rb = p1[1];
        float4 v;
        v.x = resize_lerp(lt.x, rt.x, lb.x, rb.x, fc, gc, fr, gr); v.y = resize_lerp(lt.y, rt.y, lb.y, rb.y, fc, gc, fr, gr);
        v.z = resize_lerp(lt.z, rt.z, lb.z, rb.z, fc, gc, fr, gr); v.w = resize_lerp(lt.w, rt.w, lb.w, rb.w, fc, gc, fr, gr);
        y[i] = q4_add_res(v, res, i);
    }
}

// softmax / logsoftmax over the last axis, one wave64 per row (layer.py:141-153):
// y = x - max; s = sum(exp(y)); out = exp(y - log s)  (or y - log s)
__global__ void __launch_bounds__(TPB) softmax_kernel(const float *x, float *y, int rows, int cols, int logmode) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = (gridDim.x * TPB) >> 6;
    for (unsigned r = wave; r < (unsigned)rows; r += nwaves) {      // unsigned: rows <= 2^31 - 1, so r + nwaves cannot wrap
        const float *xp = x + (size_t)r * cols;
        float *yp = y + (size_t)r * cols;
        float m = -INFINITY;
        for (unsigned i = lane; i < (unsigned)cols; i += 64) m = fmaxf(m, xp[i]);
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        float s = 0.f;
        for (unsigned i = lane; i < (unsigned)cols; i += 64) s += expf(__fsub_rn(xp[i], m));
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const float ls = logf(s);
        for (unsigned i = lane; i < (unsigned)cols; i += 64) {
            const float t = __fsub_rn(__fsub_rn(xp[i], m), ls);
            yp[i] = logmode ? t : expf(t);
        }
    }
}

// reduce over the trailing `cols` elements of each row: 0 sum, 1 mean, 2 max, 3 min
__global__ void __launch_bounds__(TPB) reduce_rows_kernel(const float *x, float *y, int rows, int cols, int op) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = (gridDim.x * TPB) >> 6;
    for (unsigned r = wave; r < (unsigned)rows; r += nwaves) {      // unsigned: rows <= 2^31 - 1, so r + nwaves cannot wrap
        const float *xp = x + (size_t)r * cols;
        float v = op == 2 ? -INFINITY : op == 3 ? INFINITY : 0.f;
        for (unsigned i = lane; i < (unsigned)cols; i += 64) {
            const float t = xp[i];
            v = op == 2 ? max_nan(v, t) : op == 3 ? min_nan(v, t) : v + t;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float t = __shfl_xor(v, off, 64);
            v = op == 2 ? max_nan(v, t) : op == 3 ? min_nan(v, t) : v + t;
        }
        if (lane == 0) y[r] = op == 1 ? __fdiv_rn(v, (float)cols) : v;
    }
}

// general permutation of up to 6 axes: out[idx_out] = in[idx_in]
struct PermArgs {
    int ndim;
    unsigned oshape[6];     // output shape
    unsigned istride[6];    // input stride (elements) of the axis that feeds output axis d
};
__global__ void __launch_bounds__(TPB) transpose_kernel(const float *x, float *y, unsigned total, PermArgs p) {
    unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned rem = i;
        size_t src = 0;
        for (int d = p.ndim - 1; d >= 0; --d) {
            const unsigned q = rem / p.oshape[d], r = rem - q * p.oshape[d];
            src += (size_t)r * p.istride[d];
            rem = q;
        }
        y[i] = x[src];
    }
}

// General strided map of up to 6 axes: output index o_d reads input index
//     t = o_d*step_d + start_d;  wrap_d = 1: t mod extent_d, 2: t clamped to the axis, 3 / 4: t mirrored at the borders without /
//     with the border sample (np.pad's 'wrap', 'edge', 'reflect', 'symmetric');  div_d > 1: needs t % div_d == 0, t /= div_d
// and takes `fill` whenever an axis lands outside [0, extent_d).  One kernel covers Slice (start /
// step, negative steps), constant Pad (negative start), Tile (wrap), Expand (stride 0), Split, the
// zero-stuffing of ConvTranspose2d (div = stride) and its filter flip + transpose (step -1,
// permuted strides).
struct MapArgs {
    int ndim;
    unsigned oshape[6];
    long long istride[6];
    int start[6], step[6], div[6], extent[6], wrap[6];
    float fill;
};
__global__ void __launch_bounds__(TPB) strided_map_kernel(const float *x, float *y, size_t total, MapArgs p) {
    const size_t stride = (size_t)gridDim.x * TPB;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        size_t rem = i;
        long long src = 0;
        bool ok = true;
        for (int d = p.ndim - 1; d >= 0; --d) {
            const size_t q = rem / p.oshape[d];
            const int o = (int)(rem - q * p.oshape[d]);
            rem = q;
            int t = o * p.step[d] + p.start[d];
            const int n = p.extent[d];
            if (p.wrap[d] == 1) {                      // modulo (Tile, np.pad 'wrap')
                t %= n;
                if (t < 0) t += n;
            } else if (p.wrap[d] == 2) {               // clamp (np.pad 'edge')
                t = min(max(t, 0), n - 1);
            } else if (p.wrap[d] >= 3) {               // mirror: 3 without the border sample ('reflect'), 4 with it ('symmetric')
                const int period = p.wrap[d] == 3 ? max(2 * (n - 1), 1) : 2 * n;
                t %= period;
                if (t < 0) t += period;
                if (t >= n) t = (p.wrap[d] == 3 ? period : period - 1) - t;
            }
            if (p.div[d] > 1) {
                ok = ok && t % p.div[d] == 0;
                t /= p.div[d];
            }
            ok = ok && t >= 0 && t < p.extent[d];
            src += (long long)t * p.istride[d];
        }
        y[i] = ok ? x[src] : p.fill;
    }
}

// ---- tiled large-image inference (util.tile, util.py:291-348) -----------------------------------
// util.resize (util.py:253-269) on an H x W x C image: separable bilinear with the reference's
// order of roundings -- columns first: a*(1-cs) + b*cs, then rows on those.  The sample positions
// (ra, rs, ca, cs) are computed on the host exactly like the reference's float32 linspace.
__global__ void __launch_bounds__(TPB) resize_hwc_kernel(const float *x, float *y, unsigned total, int W, int C,
                                                         int OW, const int *ra, const float *rs, const int *ca,
                                                         const float *cs, FastDiv divC, FastDiv divOW) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned pix, ch, oh, ow;
        divC.divmod(i, pix, ch);
        divOW.divmod(pix, oh, ow);
        const int r0 = ra[oh], c0 = ca[ow];
        const float fr = rs[oh], fc = cs[ow];
        const float gc = __fsub_rn(1.f, fc), gr = __fsub_rn(1.f, fr);
        const float *p0 = x + ((size_t)r0 * W + c0) * C + ch, *p1 = p0 + (size_t)W * C;
        const float top = __fadd_rn(__fmul_rn(p0[0], gc), __fmul_rn(p0[C], fc));
        const float bot = __fadd_rn(__fmul_rn(p1[0], gc), __fmul_rn(p1[C], fc));
        y[i] = __fadd_rn(__fmul_rn(top, gr), __fmul_rn(bot, fr));
    }
}

// One window's result into the blend buffers (util.py:333-343): weight = distance to the window
// border + 1, capped at m + 1;  buf += rst * weight, count += weight.  Launches for overlapping
// windows are ordered by the stream.
__global__ void __launch_bounds__(TPB) tile_accumulate_kernel(const float *rst, float *buf, float *count, unsigned total,
                                                              int h, int w, int C, int r0, int c0, int OW, int m,
                                                              FastDiv divC, FastDiv divW) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) {
        unsigned pix, ch, r, c;
        divC.divmod(i, pix, ch);
        divW.divmod(pix, r, c);
        const int dr = min((int)r, h - 1 - (int)r), dc = min((int)c, w - 1 - (int)c);
        const float wt = (float)(min(min(dr, dc), m) + 1);
        const size_t o = (size_t)(r0 + (int)r) * OW + (c0 + (int)c);
        buf[o * C + ch] = __fadd_rn(buf[o * C + ch], __fmul_rn(rst[i], wt));
        if (ch == 0) count[o] = __fadd_rn(count[o], wt);
    }
}

__global__ void __launch_bounds__(TPB) tile_normalise_kernel(float *buf, const float *count, unsigned total, FastDiv divC) {
    const unsigned stride = gridDim.x * TPB;
    for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < total; i += stride) buf[i] = __fdiv_rn(buf[i], count[divC.div(i)]);
}

// one launch of pixel_shuffle_q4_kernel.h for (r, order), the form picked by direction and output layout
template <int R, int ORDER>
void launch_pixel_shuffle_q4(pl_ctx *ctx, const float *xq, float *y, unsigned total, const pixel_shuffle_q4::Geom &g, int inverse,
                                    int nchw_out) {
    namespace ps = pixel_shuffle_q4;
    const unsigned grid = stream_grid(ctx, total);
    if (inverse) ps::pixel_shuffle_q4_kernel<R, ORDER, true, false><<<grid, TPB, 0, ctx->stream>>>((const float4 *)xq, y, total, g);
    else if (nchw_out) ps::pixel_shuffle_q4_kernel<R, ORDER, false, true><<<grid, TPB, 0, ctx->stream>>>((const float4 *)xq, y, total, g);
    else ps::pixel_shuffle_q4_kernel<R, ORDER, false, false><<<grid, TPB, 0, ctx->stream>>>((const float4 *)xq, y, total, g);
}

}  // namespace

unsigned pl_stream_grid(int cu_count, size_t work_items) {
    size_t blocks = (work_items + PL_STREAM_TPB - 1) / PL_STREAM_TPB;
    size_t cap = (size_t)(cu_count > 0 ? cu_count : 256) * 8;
    if (blocks > cap) blocks = cap;
    return blocks ? (unsigned)blocks : 1u;
}

bool pl_loop32_ok(int cu_count, size_t total) {
    return total < (1ull << 32) && total + (size_t)pl_stream_grid(cu_count, total) * PL_STREAM_TPB <= (1ull << 32);
}

extern "C" {

// pl_loop32_ok for (total, cu_count); cu_count <= 0 stands for the 256 CUs assumed before a context exists.  A host query (tests).
int pl_stream_loop32_ok(size_t total, int cu_count, int *ok) {
    PL_REQUIRE(ok, PL_EINVAL, "pl_stream_loop32_ok: null argument");
    *ok = pl_loop32_ok(cu_count, total) ? 1 : 0;
    return PL_OK;
}

int pl_resize_hwc_f32(pl_ctx *ctx, const float *x, float *y, int H, int W, int C, int OH, int OW, const int *ra,
                      const float *rs, const int *ca, const float *cs) {
    PL_REQUIRE(ctx && x && y && ra && rs && ca && cs, PL_EINVAL, "pl_resize_hwc_f32: null argument");
    PL_REQUIRE(H > 1 && W > 1 && C > 0 && OH > 0 && OW > 0, PL_EINVAL, "pl_resize_hwc_f32: bad shape (needs H, W >= 2)");
    const size_t total = (size_t)OH * OW * C;
    PL_REQUIRE(loop32_ok(ctx, total) && (size_t)H * W * C < (1ull << 32), PL_EUNSUPPORTED, "resize: image too large");
    CtxGuard g(ctx);
    resize_hwc_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, (unsigned)total, W, C, OW, ra, rs, ca, cs,
                                                                     FastDiv(C), FastDiv(OW));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// uint8 image batch -> float32 NCHW (image_input_kernel.h).  Every refusal comes before any launch.
int pl_image_u8_nchw_f32(pl_ctx *ctx, const unsigned char *x, float *y, int N, int H, int W, int C, int nhwc, int Co,
                         const int *order, int OH, int OW, const int *ra, const float *rs, const int *ca, const float *cs,
                         const float *k, const float *b) {
    namespace ii = image_input;
    PL_REQUIRE(ctx && k && b, PL_EINVAL, "pl_image_u8_nchw_f32: null argument");
    PL_REQUIRE(N >= 0 && H > 0 && W > 0 && OH > 0 && OW > 0, PL_EINVAL, "pl_image_u8_nchw_f32: bad shape");
    PL_REQUIRE(C >= 1 && C <= ii::MAX_C && Co >= 1 && Co <= ii::MAX_C, PL_EUNSUPPORTED,
               "pl_image_u8_nchw_f32: 1 to 4 channels, got C = %d, Co = %d", C, Co);
    PL_REQUIRE(order || Co == C, PL_EINVAL, "pl_image_u8_nchw_f32: no channel order given and Co != C");
    ii::Affine af;
    for (int c = 0; c < ii::MAX_C; ++c) {
        af.k[c] = c < Co ? k[c] : 0.f;
        af.b[c] = c < Co ? b[c] : 0.f;
        af.order[c] = c < Co ? (order ? order[c] : c) : 0;
        PL_REQUIRE(af.order[c] >= 0 && af.order[c] < C, PL_EINVAL, "pl_image_u8_nchw_f32: order[%d] = %d is no source channel", c,
                   af.order[c]);
    }
    const bool tables = ra || rs || ca || cs;
    PL_REQUIRE(!tables || (ra && rs && ca && cs), PL_EINVAL, "pl_image_u8_nchw_f32: all four sampling tables or none");
    PL_REQUIRE(tables || (OH == H && OW == W), PL_EINVAL, "pl_image_u8_nchw_f32: OH x OW != H x W needs sampling tables");
    PL_REQUIRE(!tables || nhwc, PL_EUNSUPPORTED, "pl_image_u8_nchw_f32: resize takes the (N, H, W, C) layout only");
    PL_REQUIRE(!tables || (H >= 2 && W >= 2), PL_EINVAL, "pl_image_u8_nchw_f32: resize needs H, W >= 2");
    const size_t HWo = (size_t)OH * OW;
    PL_REQUIRE((size_t)N * H * W * C < (1ull << 31) && (size_t)N * Co * HWo < (1ull << 31), PL_EUNSUPPORTED,
               "pl_image_u8_nchw_f32: 2^31 or more source bytes or output floats");
    if (N == 0) return PL_OK;
    PL_REQUIRE(x && y, PL_EINVAL, "pl_image_u8_nchw_f32: null argument");
    CtxGuard g(ctx);
    if (tables) {
        const int groups = (OW + ii::LANE_PX - 1) / ii::LANE_PX;
        const size_t total = (size_t)N * OH * groups;
        ii::image_u8_resize_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, H, W, C, Co, OH, OW, groups, ra,
                                                                                 rs, ca, cs, af, aligned16(y) && OW % 4 == 0);
    } else {
        const unsigned tiles = cdiv(HWo, ii::TILE_PX);
        const bool vec = aligned16(y) && HWo % 4 == 0;
        if (nhwc) ii::image_u8_flat_kernel<true><<<(unsigned)N * tiles, TPB, 0, ctx->stream>>>(x, y, HWo, C, Co, tiles, af, vec);
        else ii::image_u8_flat_kernel<false><<<(unsigned)N * Co * tiles, TPB, 0, ctx->stream>>>(x, y, HWo, C, Co, tiles, af, vec);
    }
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// float32 NCHW -> uint8 images and label maps (image_output_kernel.h).  Every refusal comes before any launch.
namespace {
// whether n * c * hw (each below 2^31, so no product of two wraps) stays below 2^31
inline bool below_2_31(size_t n, size_t c, size_t hw) { return n * c < (1ull << 31) && n * c * hw < (1ull << 31); }
}  // namespace

int pl_image_f32_u8(pl_ctx *ctx, const float *x, unsigned char *y, int N, int C, int H, int W, int Co, const int *order, int nhwc,
                    const float *k, const float *b, int trunc) {
    namespace io = image_output;
    PL_REQUIRE(ctx && x && y && k && b, PL_EINVAL, "pl_image_f32_u8: null argument");
    PL_REQUIRE(N >= 0 && C >= 1 && H >= 0 && W >= 0, PL_EINVAL, "pl_image_f32_u8: bad shape (%d, %d, %d, %d)", N, C, H, W);
    PL_REQUIRE(Co >= 1 && Co <= io::MAX_CO, PL_EUNSUPPORTED, "pl_image_f32_u8: 1 to 4 output channels, got Co = %d", Co);
    PL_REQUIRE(order || Co == C, PL_EINVAL, "pl_image_f32_u8: no channel order given and Co = %d != C = %d", Co, C);
    io::Affine af;
    for (int c = 0; c < io::MAX_CO; ++c) {
        af.k[c] = c < Co ? k[c] : 0.f;
        af.b[c] = c < Co ? b[c] : 0.f;
        af.order[c] = c < Co ? (order ? order[c] : c) : 0;
        PL_REQUIRE(af.order[c] >= 0 && af.order[c] < C, PL_EINVAL, "pl_image_f32_u8: order[%d] = %d is no source plane", c,
                   af.order[c]);
    }
    const size_t HW = (size_t)H * W;
    PL_REQUIRE(HW < (1ull << 31) && below_2_31(N, C, HW) && below_2_31(N, Co, HW), PL_EUNSUPPORTED,
               "pl_image_f32_u8: 2^31 or more source floats or output bytes");
    if (N == 0 || HW == 0) return PL_OK;
    CtxGuard g(ctx);
    const unsigned tiles = cdiv(HW, io::TILE_PX);
    const bool vec = aligned16(x) && HW % 4 == 0;
    if (nhwc) io::image_f32_u8_kernel<true><<<(unsigned)N * tiles, TPB, 0, ctx->stream>>>(x, y, HW, C, Co, tiles, af, vec, trunc != 0);
    else io::image_f32_u8_kernel<false><<<(unsigned)N * tiles, TPB, 0, ctx->stream>>>(x, y, HW, C, Co, tiles, af, vec, trunc != 0);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_labels_f32_u8(pl_ctx *ctx, const float *x, unsigned char *y, int N, int C, int H, int W, double threshold) {
    namespace io = image_output;
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "pl_labels_f32_u8: null argument");
    PL_REQUIRE(N >= 0 && C >= 1 && H >= 0 && W >= 0, PL_EINVAL, "pl_labels_f32_u8: bad shape (%d, %d, %d, %d)", N, C, H, W);
    PL_REQUIRE(C <= io::MAX_LABELS, PL_EUNSUPPORTED, "pl_labels_f32_u8: at most 256 planes fit a byte, got C = %d", C);
    const size_t HW = (size_t)H * W;
    PL_REQUIRE(HW < (1ull << 31) && below_2_31(N, C, HW), PL_EUNSUPPORTED, "pl_labels_f32_u8: 2^31 or more source floats");
    if (N == 0 || HW == 0) return PL_OK;
    CtxGuard g(ctx);
    const unsigned tiles = cdiv(HW, io::TILE_PX);
    io::labels_f32_u8_kernel<<<(unsigned)N * tiles, TPB, 0, ctx->stream>>>(x, y, HW, C, tiles, (float)threshold,
                                                                          aligned16(x) && HW % 4 == 0);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// YOLO heads -> detections (detect_kernel.h).  Every refusal comes before any launch.
int pl_yolo_decode_f32(pl_ctx *ctx, const float *x, int N, int A, int C, int Gh, int Gw, const float *anchors, double sx, double sy,
                       double conf, int row, int offset, float *scores, int *classes, float *boxes) {
    namespace dt = detect;
    PL_REQUIRE(ctx && x && anchors && scores && classes && boxes, PL_EINVAL, "pl_yolo_decode_f32: null argument");
    PL_REQUIRE(N >= 0 && A >= 0 && Gh >= 0 && Gw >= 0 && row >= 0, PL_EINVAL, "pl_yolo_decode_f32: bad shape (%d, %d x (5 + %d), %d, %d), row %d",
               N, A, C, Gh, Gw, row);
    PL_REQUIRE(C >= 1, PL_EINVAL, "pl_yolo_decode_f32: at least one class, got C = %d", C);
    const size_t HW = (size_t)Gh * Gw;
    PL_REQUIRE(offset >= 0 && HW < (1ull << 31) && (size_t)A * HW <= (size_t)row && (size_t)offset <= (size_t)row - (size_t)A * HW,
               PL_EINVAL, "pl_yolo_decode_f32: %d x %d x %d anchors at offset %d do not fit a row of %d", A, Gh, Gw, offset, row);
    PL_REQUIRE(A <= dt::MAX_ANCHORS, PL_EUNSUPPORTED, "pl_yolo_decode_f32: at most %d anchors per head, got A = %d", dt::MAX_ANCHORS, A);
    const size_t planes = (size_t)A * (5 + (size_t)C);      // (A <= 8: below 2^35)
    PL_REQUIRE(planes < (1ull << 31) && below_2_31(N, planes, HW) && below_2_31(N, 4, row), PL_EUNSUPPORTED,
               "pl_yolo_decode_f32: 2^31 or more floats in a tensor");
    if (N == 0 || A == 0 || HW == 0) return PL_OK;
    dt::Anchors an;
    for (int a = 0; a < dt::MAX_ANCHORS; ++a) {
        an.w[a] = a < A ? anchors[2 * a] : 0.f;
        an.h[a] = a < A ? anchors[2 * a + 1] : 0.f;
    }
    CtxGuard g(ctx);
    const unsigned tiles = cdiv(HW, dt::TPB);
    dt::decode_kernel<<<(unsigned)N * (unsigned)A * tiles, dt::TPB, 0, ctx->stream>>>(x, scores, classes, boxes, A, C, Gw, HW, tiles, an, (float)sx,
                                                                                      (float)sy, (float)conf, (size_t)row, (size_t)offset);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_nms_f32(pl_ctx *ctx, const float *boxes, const int *classes, const float *sorted_scores, const long long *order, int N, int R,
               int K, double floor, double iou, int class_aware, int max_det, float *det, int *num) {
    namespace dt = detect;
    PL_REQUIRE(ctx && boxes && sorted_scores && order && det && num, PL_EINVAL, "pl_nms_f32: null argument");
    PL_REQUIRE(N >= 0 && R >= 0 && K >= 0 && max_det >= 0, PL_EINVAL, "pl_nms_f32: bad shape N = %d, R = %d, K = %d, max_det = %d", N, R, K,
               max_det);
    PL_REQUIRE(K <= R, PL_EINVAL, "pl_nms_f32: K = %d entries of %d rows", K, R);
    PL_REQUIRE(K <= dt::NMS_MAX_K, PL_EUNSUPPORTED, "pl_nms_f32: at most %d entries per image, got K = %d", dt::NMS_MAX_K, K);
    PL_REQUIRE(max_det <= K, PL_EUNSUPPORTED, "pl_nms_f32: max_det = %d exceeds K = %d", max_det, K);
    PL_REQUIRE(below_2_31(N, 4, R) && below_2_31(N, 6, max_det), PL_EUNSUPPORTED, "pl_nms_f32: 2^31 or more floats in a tensor");
    if (N == 0) return PL_OK;
    CtxGuard g(ctx);
    const size_t lds = dt::nms_lds_bytes(K);
    if (lds > 48 * 1024)
        PL_HIP(hipFuncSetAttribute((const void *)dt::nms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dt::nms_kernel<<<(unsigned)N, dt::TPB, lds, ctx->stream>>>(boxes, classes, sorted_scores, order, R, K, (float)floor, (float)iou,
                                                               class_aware != 0, max_det, det, num);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// uint8 class map -> objects (components_kernel.h).  Every refusal comes before any launch.
int pl_components_u8_i32(pl_ctx *ctx, const unsigned char *m, int N, int H, int W, int connectivity, int background, int max_objects,
                         void *scratch, int *labels, int *num, int *objects, float *centroids) {
    namespace cc = components;
    PL_REQUIRE(ctx && m && scratch && labels && num && (max_objects <= 0 || (objects && centroids)), PL_EINVAL,
               "pl_components_u8_i32: null argument");
    PL_REQUIRE(N >= 0 && H >= 0 && W >= 0 && max_objects >= 0, PL_EINVAL, "pl_components_u8_i32: bad shape (%d, %d, %d), max_objects = %d", N,
               H, W, max_objects);
    PL_REQUIRE(connectivity == 4 || connectivity == 8, PL_EINVAL, "pl_components_u8_i32: connectivity is 4 or 8, got %d", connectivity);
    PL_REQUIRE(background >= -1 && background <= 255, PL_EINVAL, "pl_components_u8_i32: background is a class 0..255 or -1, got %d",
               background);
    const size_t HW = (size_t)H * W;
    PL_REQUIRE(HW < (1ull << 31) && (size_t)N * HW < (1ull << 31), PL_EUNSUPPORTED, "pl_components_u8_i32: 2^31 or more pixels");
    PL_REQUIRE(max_objects <= PL_CC_MAX_OBJECTS, PL_EUNSUPPORTED, "pl_components_u8_i32: at most %d table rows per image, got max_objects = %d",
               PL_CC_MAX_OBJECTS, max_objects);
    if (N == 0 || HW == 0) return PL_OK;
    cc::Geo g;
    g.H = H, g.W = W, g.HW = (int)HW;
    g.tiles_x = (int)cdiv(W, cc::TILE_W), g.tiles_y = (int)cdiv(H, cc::TILE_H), g.blocks = (int)cdiv(HW, cc::BLOCK);
    const size_t tiles = (size_t)N * g.tiles_x * g.tiles_y;
    PL_REQUIRE(tiles < (1ull << 31) && (size_t)N * max_objects * 6 < (1ull << 31), PL_EUNSUPPORTED,
               "pl_components_u8_i32: 2^31 or more tiles or table entries");
    // scratch: the int64 coordinate sums in front (8-byte aligned), then link, then the per-block root counts
    long long *sums = reinterpret_cast<long long *>(scratch);
    int *link = reinterpret_cast<int *>(sums + (size_t)N * max_objects * 2);
    int *counts = link + (size_t)N * HW;
    const int conn8 = connectivity == 8;
    CtxGuard guard(ctx);
    cc::tile_kernel<<<(unsigned)tiles, cc::TPB, 0, ctx->stream>>>(m, link, g, conn8, background);
    const size_t per_image = (size_t)(g.tiles_y - 1) * W + (size_t)(g.tiles_x - 1) * H;      // (below H W)
    if (per_image)
        cc::seam_kernel<<<cdiv(N * per_image, cc::TPB), cc::TPB, 0, ctx->stream>>>(m, link, g, conn8, background, (unsigned)per_image,
                                                                                 (unsigned)(N * per_image));
    const unsigned nblocks = (unsigned)N * (unsigned)g.blocks;
    cc::resolve_kernel<<<nblocks, cc::TPB, 0, ctx->stream>>>(link, labels, counts, g);
    cc::scan_kernel<<<(unsigned)N, cc::SCAN_STEP, 0, ctx->stream>>>(counts, g.blocks, num, max_objects, objects, sums);
    cc::rank_kernel<<<nblocks, cc::TPB, 0, ctx->stream>>>(labels, counts, g);
    cc::region_kernel<<<(unsigned)tiles, cc::TPB, 0, ctx->stream>>>(m, link, labels, g, max_objects, objects, sums);
    if (max_objects)
        cc::centroid_kernel<<<cdiv((size_t)N * max_objects, cc::TPB), cc::TPB, 0, ctx->stream>>>(objects, sums, centroids,
                                                                                              (unsigned)N * (unsigned)max_objects);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// flow field and probability planes -> instance masks (flow_kernel.h).  Every refusal comes before any launch.
int pl_flow_instances_f32(pl_ctx *ctx, const float *x, int N, int H, int W, long long image_stride, long long pixel_stride,
                          long long off_dy, long long off_dx, long long off_prob, double level, double min_flow, int rounds, int min_size,
                          int max_instances, void *scratch, int *masks, int *num, int *instances, float *centres) {
    namespace fl = flow;
    PL_REQUIRE(ctx && x && scratch && masks && num && (max_instances <= 0 || (instances && centres)), PL_EINVAL,
               "pl_flow_instances_f32: null argument");
    PL_REQUIRE(N >= 0 && H >= 0 && W >= 0 && max_instances >= 0, PL_EINVAL, "pl_flow_instances_f32: bad shape (%d, %d, %d), max_instances = %d",
               N, H, W, max_instances);
    PL_REQUIRE(rounds >= 0 && min_size >= 0, PL_EINVAL, "pl_flow_instances_f32: rounds = %d and min_size = %d are counts >= 0", rounds,
               min_size);
    PL_REQUIRE(image_stride > 0 && pixel_stride > 0 && off_dy >= 0 && off_dx >= 0 && off_prob >= 0, PL_EINVAL,
               "pl_flow_instances_f32: strides are positive and plane offsets are not negative");
    PL_REQUIRE(level == level && min_flow == min_flow, PL_EINVAL, "pl_flow_instances_f32: level or min_flow is NaN");
    const size_t HW = (size_t)H * W;
    PL_REQUIRE(HW < (1ull << 31) && (size_t)N * HW < (1ull << 31), PL_EUNSUPPORTED, "pl_flow_instances_f32: 2^31 or more pixels");
    PL_REQUIRE(rounds <= PL_FLOW_MAX_ROUNDS, PL_EUNSUPPORTED, "pl_flow_instances_f32: at most %d pointer doublings, got rounds = %d",
               PL_FLOW_MAX_ROUNDS, rounds);
    PL_REQUIRE(max_instances <= PL_FLOW_MAX_INSTANCES, PL_EUNSUPPORTED,
               "pl_flow_instances_f32: at most %d table rows per image, got max_instances = %d", PL_FLOW_MAX_INSTANCES, max_instances);
    PL_REQUIRE((size_t)N * max_instances * 5 < (1ull << 31), PL_EUNSUPPORTED, "pl_flow_instances_f32: 2^31 or more table entries");
    if (N == 0 || HW == 0) return PL_OK;
    fl::Geo g;
    g.N = N, g.H = H, g.W = W, g.HW = (int)HW, g.total = (int)(N * HW);
    g.tiles_x = (int)cdiv(W, fl::TILE_W), g.tiles_y = (int)cdiv(H, fl::TILE_H);
    g.max_raw = (int)PL_FLOW_MAX_RAW(H, W);
    g.image_stride = image_stride, g.pixel_stride = pixel_stride, g.off_dy = off_dy, g.off_dx = off_dx, g.off_prob = off_prob;
    // scratch, from its first 16-byte boundary on: the int64 coordinate sums, two pointer buffers, the hit counts, the sink
    // labels, the volume table, the sink regions per image, the sink map, and the components chain's own scratch
    char *at = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(scratch) + 15) / 16 * 16);
    auto take = [&at](size_t bytes) {
        char *p = at;
        at += PL_FLOW_ALIGN(bytes);
        return p;
    };
    const size_t total = (size_t)g.total;
    long long *sums = reinterpret_cast<long long *>(take((size_t)N * max_instances * 16));
    int *buf[2] = {reinterpret_cast<int *>(take(total * 4)), reinterpret_cast<int *>(take(total * 4))};
    int *cnt = reinterpret_cast<int *>(take(total * 4)), *S = reinterpret_cast<int *>(take(total * 4));
    int *vol = reinterpret_cast<int *>(take((size_t)N * g.max_raw * 4)), *raw_num = reinterpret_cast<int *>(take((size_t)N * 4));
    unsigned char *sink = reinterpret_cast<unsigned char *>(take(total));
    void *cc_scratch = at;
    const float lv = (float)level, mf = (float)min_flow, g2 = mf * mf;      // (one product: nothing to contract)
    const bool vec = pixel_stride == 1 && W % 4 == 0 && image_stride % 4 == 0 && off_dy % 4 == 0 && off_dx % 4 == 0 && off_prob % 4 == 0 &&
                     reinterpret_cast<uintptr_t>(x) % 16 == 0;
    const unsigned quads = cdiv(total, (size_t)fl::QUAD * fl::TPB), pixels = cdiv(total, fl::TPB);
    CtxGuard guard(ctx);
    if (vec)
        fl::step_kernel<true><<<quads, fl::TPB, 0, ctx->stream>>>(x, g, lv, g2, buf[0], cnt, vol, N * g.max_raw);
    else
        fl::step_kernel<false><<<quads, fl::TPB, 0, ctx->stream>>>(x, g, lv, g2, buf[0], cnt, vol, N * g.max_raw);
    int cur = 0;
    for (int r = 0; r < rounds; cur ^= 1) {
        if (rounds - r >= 2) {
            fl::double_kernel<true><<<quads, fl::TPB, 0, ctx->stream>>>(buf[cur], buf[cur ^ 1], g.total);
            r += 2;
        } else {
            fl::double_kernel<false><<<quads, fl::TPB, 0, ctx->stream>>>(buf[cur], buf[cur ^ 1], g.total);
            r += 1;
        }
    }
    const int *end = buf[cur];
    fl::count_kernel<<<pixels, fl::TPB, 0, ctx->stream>>>(end, cnt, g.total);
    fl::sink_kernel<<<quads, fl::TPB, 0, ctx->stream>>>(cnt, sink, g.total);
    PL_LAUNCH_CHECK();
    const int rc = pl_components_u8_i32(ctx, sink, N, H, W, 8, 0, 0, cc_scratch, S, raw_num, nullptr, nullptr);
    if (rc != PL_OK) return rc;
    fl::volume_kernel<<<pixels, fl::TPB, 0, ctx->stream>>>(cnt, S, vol, g);
    fl::renumber_kernel<<<(unsigned)N, fl::SCAN_STEP, 0, ctx->stream>>>(vol, raw_num, g.max_raw, min_size, num, max_instances, instances, sums);
    const size_t tiles = (size_t)N * g.tiles_x * g.tiles_y;                  // (below 2^31: pl_components_u8_i32 took them)
    fl::table_kernel<<<(unsigned)tiles, fl::TPB, 0, ctx->stream>>>(end, S, vol, masks, g, max_instances, instances, sums);
    if (max_instances)
        fl::centre_kernel<<<cdiv((size_t)N * max_instances, fl::TPB), fl::TPB, 0, ctx->stream>>>(instances, sums, centres,
                                                                                            (unsigned)N * (unsigned)max_instances);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// float32 heat maps -> peaks per plane (peaks_kernel.h).  Every refusal comes before any launch.
int pl_peaks_f32(pl_ctx *ctx, const float *x, int N, int K, int H, int W, double threshold, int ties, int max_peaks, int refine,
                 double sy, double sx, void *scratch, float *peaks, int *num) {
    namespace pk = peaks;
    PL_REQUIRE(ctx && x && scratch && peaks && num, PL_EINVAL, "pl_peaks_f32: null argument");
    PL_REQUIRE(N >= 0 && K >= 0 && H >= 0 && W >= 0 && max_peaks >= 1, PL_EINVAL, "pl_peaks_f32: bad shape (%d, %d, %d, %d), max_peaks = %d",
               N, K, H, W, max_peaks);
    PL_REQUIRE(ties == PL_PEAKS_TIES_ALL || ties == PL_PEAKS_TIES_FIRST, PL_EINVAL, "pl_peaks_f32: ties is 0 (all) or 1 (first), got %d", ties);
    PL_REQUIRE(refine == PL_PEAKS_REFINE_NONE || refine == PL_PEAKS_REFINE_QUARTER, PL_EINVAL,
               "pl_peaks_f32: refine is 0 (none) or 1 (quarter), got %d", refine);
    PL_REQUIRE(threshold == threshold && sy == sy && sx == sx, PL_EINVAL, "pl_peaks_f32: threshold or stride is NaN");
    PL_REQUIRE(max_peaks <= PL_PEAKS_MAX_PEAKS, PL_EUNSUPPORTED, "pl_peaks_f32: at most %d rows per plane, got max_peaks = %d",
               PL_PEAKS_MAX_PEAKS, max_peaks);
    PL_REQUIRE(H <= PL_PEAKS_MAX_EXTENT && W <= PL_PEAKS_MAX_EXTENT, PL_EUNSUPPORTED, "pl_peaks_f32: a plane of at most %d x %d, got %d x %d",
               PL_PEAKS_MAX_EXTENT, PL_PEAKS_MAX_EXTENT, H, W);
    const size_t HW = (size_t)H * W, planes = (size_t)N * K;
    PL_REQUIRE(HW < (1ull << 31) && planes < (1ull << 31) && planes * HW < (1ull << 31), PL_EUNSUPPORTED,
               "pl_peaks_f32: 2^31 or more pixels");
    PL_REQUIRE(3 * planes * max_peaks < (1ull << 31), PL_EUNSUPPORTED, "pl_peaks_f32: 2^31 or more output floats");
    if (planes == 0) return PL_OK;
    pk::Geo g;
    g.H = H, g.W = W, g.HW = (int)HW;
    g.tiles_x = (int)cdiv(W, pk::TILE_W), g.tiles_y = (int)cdiv(H, pk::TILE_H);
    const size_t tiles = planes * g.tiles_x * g.tiles_y;  // (a tile holds a pixel at least: below 2^31)
    // scratch: every tile's best max_peaks keys in front (8-byte aligned), then every tile's count
    pk::u64 *keys = reinterpret_cast<pk::u64 *>(scratch);
    int *counts = reinterpret_cast<int *>(keys + tiles * max_peaks);
    const int vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    CtxGuard guard(ctx);
    if (tiles)
        pk::tile_kernel<<<(unsigned)tiles, pk::TPB, 0, ctx->stream>>>(x, g, (float)threshold, ties == PL_PEAKS_TIES_FIRST, max_peaks, vec, keys,
                                                                     counts);
    pk::merge_kernel<<<(unsigned)planes, pk::TPB, 0, ctx->stream>>>(x, keys, counts, g, max_peaks, refine == PL_PEAKS_REFINE_QUARTER, (float)sy,
                                                                   (float)sx, peaks, num);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// float32 sequence tensor -> greedy CTC text (text_kernel.h).  Every refusal comes before any launch.
int pl_ctc_greedy_f32(pl_ctx *ctx, const float *x, int S_outer, int S_inner, int T, int C, long long st_outer, long long st_inner,
                      long long st_time, long long st_class, const int *lengths, int blank, int merge_repeated, int confidence,
                      int max_len, void *scratch, int *text, int *length, float *conf, int *spans) {
    namespace tx = text;
    PL_REQUIRE(ctx && x && scratch && text && length && conf && spans, PL_EINVAL, "pl_ctc_greedy_f32: null argument");
    PL_REQUIRE(S_outer >= 0 && S_inner >= 0 && T >= 0 && C >= 1, PL_EINVAL, "pl_ctc_greedy_f32: bad shape: %d x %d sequences, %d frames, %d classes",
               S_outer, S_inner, T, C);
    PL_REQUIRE(blank >= 0 && blank < C, PL_EINVAL, "pl_ctc_greedy_f32: blank = %d is no class of %d", blank, C);
    PL_REQUIRE(max_len >= 1, PL_EINVAL, "pl_ctc_greedy_f32: max_len = %d is below 1", max_len);
    PL_REQUIRE(confidence == PL_TEXT_CONF_NONE || confidence == PL_TEXT_CONF_SOFTMAX || confidence == PL_TEXT_CONF_VALUE, PL_EINVAL,
               "pl_ctc_greedy_f32: confidence is 0 (none), 1 (softmax) or 2 (value), got %d", confidence);
    PL_REQUIRE(max_len <= PL_TEXT_MAX_LEN, PL_EUNSUPPORTED, "pl_ctc_greedy_f32: at most %d symbols per sequence, got max_len = %d",
               PL_TEXT_MAX_LEN, max_len);
    PL_REQUIRE(T <= PL_TEXT_MAX_FRAMES, PL_EUNSUPPORTED, "pl_ctc_greedy_f32: at most %d frames, got %d", PL_TEXT_MAX_FRAMES, T);
    const size_t S = (size_t)S_outer * S_inner, frames = S * T;
    PL_REQUIRE(S < (1ull << 31) && frames < (1ull << 31) && frames * C < (1ull << 31), PL_EUNSUPPORTED,
               "pl_ctc_greedy_f32: 2^31 or more sequences, frames or elements");
    if (S == 0) return PL_OK;
    tx::Geo g;
    g.S_inner = S_inner, g.T = T, g.C = C;
    g.st_outer = st_outer, g.st_inner = st_inner, g.st_time = st_time, g.st_class = st_class;
    int *labels = reinterpret_cast<int *>(scratch);
    float *confs = reinterpret_cast<float *>(labels + frames);
    const bool sum = confidence == PL_TEXT_CONF_SOFTMAX;
    CtxGuard guard(ctx);
    if (frames) {
        if (st_class == 1 && C <= tx::ROW_WAVE_MAX) {
            const unsigned grid = (unsigned)cdiv(frames, (size_t)tx::WAVES);
            if (sum)
                tx::rows_wave_kernel<true><<<grid, tx::TPB, 0, ctx->stream>>>(x, g, frames, lengths, confidence, labels, confs);
            else
                tx::rows_wave_kernel<false><<<grid, tx::TPB, 0, ctx->stream>>>(x, g, frames, lengths, confidence, labels, confs);
        } else if (st_class == 1) {
            if (sum)
                tx::rows_block_kernel<true><<<(unsigned)frames, tx::TPB, 0, ctx->stream>>>(x, g, lengths, confidence, labels, confs);
            else
                tx::rows_block_kernel<false><<<(unsigned)frames, tx::TPB, 0, ctx->stream>>>(x, g, lengths, confidence, labels, confs);
        } else {
            const unsigned spans_t = (unsigned)cdiv(T, tx::TIME_LANES), grid = (unsigned)(S * spans_t);   // (below 2^31: no more than frames)
            if (sum)
                tx::time_kernel<true><<<grid, tx::TIME_TPB, 0, ctx->stream>>>(x, g, spans_t, lengths, confidence, labels, confs);
            else
                tx::time_kernel<false><<<grid, tx::TIME_TPB, 0, ctx->stream>>>(x, g, spans_t, lengths, confidence, labels, confs);
        }
    }
    tx::collapse_kernel<<<(unsigned)S, tx::TPB, 0, ctx->stream>>>(labels, confs, T, lengths, blank, merge_repeated != 0, confidence, max_len, text,
                                                                 length, conf, spans);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_tile_accumulate_f32(pl_ctx *ctx, const float *rst, float *buf, float *count, int h, int w, int C, int r0, int c0,
                           int OH, int OW, int margin) {
    PL_REQUIRE(ctx && rst && buf && count, PL_EINVAL, "pl_tile_accumulate_f32: null argument");
    PL_REQUIRE(h > 0 && w > 0 && C > 0 && r0 >= 0 && c0 >= 0 && r0 + h <= OH && c0 + w <= OW && margin >= 0, PL_EINVAL,
               "pl_tile_accumulate_f32: window outside the output");
    const size_t total = (size_t)h * w * C;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "tile: window too large");
    CtxGuard g(ctx);
    tile_accumulate_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(rst, buf, count, (unsigned)total, h, w, C, r0,
                                                                          c0, OW, margin, FastDiv(C), FastDiv(w));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_tile_normalise_f32(pl_ctx *ctx, float *buf, const float *count, int OH, int OW, int C) {
    PL_REQUIRE(ctx && buf && count && OH > 0 && OW > 0 && C > 0, PL_EINVAL, "pl_tile_normalise_f32: bad argument");
    const size_t total = (size_t)OH * OW * C;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "tile: image too large");
    CtxGuard g(ctx);
    tile_normalise_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(buf, count, (unsigned)total, FastDiv(C));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// Net.tiled's window gather and blend (tile_kernel.h).  Every refusal comes before any launch.
extern "C++" {        // (a template among the C entry points)
namespace {
template <typename T>
int launch_tile_windows(pl_ctx *ctx, const char *who, const T *x, float *y, int H, int W, int C, int Co, const int *r0, const int *c0,
                        int n, int S, int h, int w, int WH, int WW, const int *ra, const float *rs, const int *ca, const float *cs,
                        const image_input::Affine &af) {
    PL_REQUIRE(ctx && r0 && c0, PL_EINVAL, "%s: null argument", who);
    PL_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0 && WH > 0 && WW > 0 && S >= 0 && n >= 1, PL_EINVAL,
               "%s: bad shape (image %d x %d, working %d x %d, window %d x %d, %d windows, %d slots)", who, H, W, WH, WW, h, w, n, S);
    PL_REQUIRE(h <= WH && w <= WW, PL_EINVAL, "%s: a %d x %d window does not fit the %d x %d working image", who, h, w, WH, WW);
    const bool tables = ra || rs || ca || cs;
    PL_REQUIRE(!tables || (ra && rs && ca && cs), PL_EINVAL, "%s: all four sampling tables or none", who);
    PL_REQUIRE(tables || (WH == H && WW == W), PL_EINVAL, "%s: a working size other than H x W needs sampling tables", who);
    PL_REQUIRE(!tables || (H >= 2 && W >= 2), PL_EINVAL, "%s: resampling needs H, W >= 2", who);
    const size_t hw = (size_t)h * w;
    PL_REQUIRE((size_t)H * W < (1ull << 31) && below_2_31(H, W, C) && hw < (1ull << 31) && below_2_31(S, Co, hw), PL_EUNSUPPORTED,
               "%s: 2^31 or more source elements or output floats", who);
    if (S == 0) return PL_OK;
    PL_REQUIRE(x && y, PL_EINVAL, "%s: null argument", who);
    CtxGuard g(ctx);
    const unsigned groups = cdiv(hw, tile::LANE_PX);
    const size_t total = (size_t)S * groups;
    const bool vec = aligned16(y) && hw % 4 == 0;
    const tile::Tables tb = {ra, rs, ca, cs};
    if (tables)
        tile::tile_windows_kernel<T, true><<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, H, W, C, Co, h, w, WH, WW, r0, c0, n,
                                                                                         groups, tb, af, vec);
    else
        tile::tile_windows_kernel<T, false><<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, H, W, C, Co, h, w, WH, WW, r0, c0, n,
                                                                                          groups, tb, af, vec);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// the checks the three blend entry points share; fills `g` (Co, threshold and trunc are the caller's)
int blend_geometry(pl_ctx *ctx, const char *who, const void *x, const void *y, int n, int C, int oh, int ow, const int *R0, const int *C0,
                   int gr, int gc, int OH, int OW, int ramp, tile::Blend &g) {
    PL_REQUIRE(ctx && x && y && R0 && C0, PL_EINVAL, "%s: null argument", who);
    PL_REQUIRE(n >= 1 && C >= 1 && oh > 0 && ow > 0 && gr >= 1 && gc >= 1 && OH >= 0 && OW >= 0 && ramp >= 0, PL_EINVAL,
               "%s: bad shape (%d windows (%d, %d, %d), grid %d x %d, output %d x %d, ramp %d)", who, n, C, oh, ow, gr, gc, OH, OW, ramp);
    PL_REQUIRE((size_t)gr * gc == (size_t)n, PL_EINVAL, "%s: a %d x %d grid is not %d windows", who, gr, gc, n);
    PL_REQUIRE(oh <= OH && ow <= OW, PL_EINVAL, "%s: a %d x %d window result does not fit the %d x %d output", who, oh, ow, OH, OW);
    PL_REQUIRE((size_t)oh * ow < (1ull << 31) && below_2_31(n, C, (size_t)oh * ow) && (size_t)OH * OW < (1ull << 31), PL_EUNSUPPORTED,
               "%s: 2^31 or more window floats or output pixels", who);
    g.n = n, g.C = C, g.oh = oh, g.ow = ow, g.gr = gr, g.gc = gc, g.OH = OH, g.OW = OW, g.ramp = ramp;
    g.Co = C, g.groups = cdiv((size_t)OW, tile::LANE_PX), g.threshold = 0.f, g.trunc = false;
    return PL_OK;
}
}  // namespace
}  // extern "C++"

int pl_tile_windows_u8_nchw_f32(pl_ctx *ctx, const unsigned char *x, float *y, int H, int W, int C, int Co, const int *order,
                                const int *r0, const int *c0, int n, int S, int h, int w, int WH, int WW, const int *ra, const float *rs,
                                const int *ca, const float *cs, const float *k, const float *b) {
    namespace ii = image_input;
    PL_REQUIRE(ctx && k && b, PL_EINVAL, "pl_tile_windows_u8_nchw_f32: null argument");
    PL_REQUIRE(C >= 1 && C <= ii::MAX_C && Co >= 1 && Co <= ii::MAX_C, PL_EUNSUPPORTED,
               "pl_tile_windows_u8_nchw_f32: 1 to 4 channels, got C = %d, Co = %d", C, Co);
    PL_REQUIRE(order || Co == C, PL_EINVAL, "pl_tile_windows_u8_nchw_f32: no channel order given and Co != C");
    ii::Affine af;
    for (int c = 0; c < ii::MAX_C; ++c) {
        af.k[c] = c < Co ? k[c] : 0.f;
        af.b[c] = c < Co ? b[c] : 0.f;
        af.order[c] = c < Co ? (order ? order[c] : c) : 0;
        PL_REQUIRE(af.order[c] >= 0 && af.order[c] < C, PL_EINVAL, "pl_tile_windows_u8_nchw_f32: order[%d] = %d is no source channel", c,
                   af.order[c]);
    }
    return launch_tile_windows(ctx, "pl_tile_windows_u8_nchw_f32", x, y, H, W, C, Co, r0, c0, n, S, h, w, WH, WW, ra, rs, ca, cs, af);
}

int pl_tile_windows_f32_nchw_f32(pl_ctx *ctx, const float *x, float *y, int H, int W, int C, const int *r0, const int *c0, int n, int S,
                                 int h, int w, int WH, int WW, const int *ra, const float *rs, const int *ca, const float *cs) {
    PL_REQUIRE(C >= 1, PL_EINVAL, "pl_tile_windows_f32_nchw_f32: at least one channel, got C = %d", C);
    image_input::Affine af = {};
    return launch_tile_windows(ctx, "pl_tile_windows_f32_nchw_f32", x, y, H, W, C, C, r0, c0, n, S, h, w, WH, WW, ra, rs, ca, cs, af);
}

int pl_tile_blend_f32(pl_ctx *ctx, const float *x, float *y, int n, int C, int oh, int ow, const int *R0, const int *C0, int gr, int gc,
                      int OH, int OW, int ramp) {
    tile::Blend g;
    if (int rc = blend_geometry(ctx, "pl_tile_blend_f32", x, y, n, C, oh, ow, R0, C0, gr, gc, OH, OW, ramp, g)) return rc;
    PL_REQUIRE(below_2_31(OH, OW, C), PL_EUNSUPPORTED, "pl_tile_blend_f32: 2^31 or more output floats");
    const size_t total = (size_t)OH * g.groups;
    if (!total) return PL_OK;
    CtxGuard guard(ctx);
    tile::tile_blend_kernel<tile::OUT_F32><<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, R0, C0, g, image_output::Affine{});
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_tile_blend_u8(pl_ctx *ctx, const float *x, unsigned char *y, int n, int C, int oh, int ow, const int *R0, const int *C0, int gr,
                     int gc, int OH, int OW, int ramp, int Co, const int *order, int nhwc, const float *k, const float *b, int trunc) {
    namespace io = image_output;
    tile::Blend g;
    PL_REQUIRE(k && b, PL_EINVAL, "pl_tile_blend_u8: null argument");
    if (int rc = blend_geometry(ctx, "pl_tile_blend_u8", x, y, n, C, oh, ow, R0, C0, gr, gc, OH, OW, ramp, g)) return rc;
    PL_REQUIRE(Co >= 1 && Co <= io::MAX_CO, PL_EUNSUPPORTED, "pl_tile_blend_u8: 1 to 4 output channels, got Co = %d", Co);
    PL_REQUIRE(order || Co == C, PL_EINVAL, "pl_tile_blend_u8: no channel order given and Co = %d != C = %d", Co, C);
    io::Affine af;
    for (int c = 0; c < io::MAX_CO; ++c) {
        af.k[c] = c < Co ? k[c] : 0.f;
        af.b[c] = c < Co ? b[c] : 0.f;
        af.order[c] = c < Co ? (order ? order[c] : c) : 0;
        PL_REQUIRE(af.order[c] >= 0 && af.order[c] < C, PL_EINVAL, "pl_tile_blend_u8: order[%d] = %d is no source plane", c, af.order[c]);
    }
    g.Co = Co, g.trunc = trunc != 0;
    const size_t total = (size_t)OH * g.groups;
    if (!total) return PL_OK;
    CtxGuard guard(ctx);
    if (nhwc) tile::tile_blend_kernel<tile::OUT_U8_NHWC><<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, R0, C0, g, af);
    else tile::tile_blend_kernel<tile::OUT_U8_NCHW><<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, R0, C0, g, af);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_tile_blend_labels_u8(pl_ctx *ctx, const float *x, unsigned char *y, int n, int C, int oh, int ow, const int *R0, const int *C0,
                            int gr, int gc, int OH, int OW, int ramp, double threshold) {
    tile::Blend g;
    if (int rc = blend_geometry(ctx, "pl_tile_blend_labels_u8", x, y, n, C, oh, ow, R0, C0, gr, gc, OH, OW, ramp, g)) return rc;
    PL_REQUIRE(C <= image_output::MAX_LABELS, PL_EUNSUPPORTED, "pl_tile_blend_labels_u8: at most 256 planes fit a byte, got C = %d", C);
    g.threshold = (float)threshold;
    const size_t total = (size_t)OH * g.groups;
    if (!total) return PL_OK;
    CtxGuard guard(ctx);
    tile::tile_blend_kernel<tile::OUT_LABELS><<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, R0, C0, g, image_output::Affine{});
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_strided_map_f32(pl_ctx *ctx, const float *x, float *y, int ndim, const int *out_shape,
                       const long long *in_stride, const int *start, const int *step, const int *div,
                       const int *extent, const int *wrap, double fill) {
    PL_REQUIRE(ctx && y && out_shape && in_stride && start && step && div && extent && wrap, PL_EINVAL,
               "pl_strided_map_f32: null argument");
    PL_REQUIRE(ndim >= 1 && ndim <= 6, PL_EUNSUPPORTED, "pl_strided_map_f32: 1..6 axes supported, got %d", ndim);
    MapArgs p;
    p.ndim = ndim;
    p.fill = (float)fill;
    size_t total = 1;
    for (int d = 0; d < ndim; ++d) {
        PL_REQUIRE(out_shape[d] >= 0 && extent[d] >= 0 && div[d] >= 1, PL_EINVAL, "pl_strided_map_f32: bad axis %d", d);
        PL_REQUIRE(wrap[d] >= 0 && wrap[d] <= 4, PL_EINVAL, "pl_strided_map_f32: boundary mode %d of axis %d (0 fill, 1 wrap, 2 edge, 3 reflect, 4 symmetric)", wrap[d], d);
        PL_REQUIRE(!wrap[d] || extent[d] > 0, PL_EINVAL, "pl_strided_map_f32: wrap on an empty axis");
        p.oshape[d] = (unsigned)out_shape[d];
        p.istride[d] = in_stride[d];
        p.start[d] = start[d]; p.step[d] = step[d]; p.div[d] = div[d]; p.extent[d] = extent[d]; p.wrap[d] = wrap[d];
        total *= (size_t)out_shape[d];
    }
    if (!total) return PL_OK;
    PL_REQUIRE(x, PL_EINVAL, "pl_strided_map_f32: null input");
    PL_REQUIRE(total < (1ull << 32), PL_EUNSUPPORTED, "pl_strided_map_f32: tensor too large");
    CtxGuard g(ctx);
    strided_map_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, total, p);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_unary_f32(pl_ctx *ctx, const float *x, float *y, size_t n, int op, double p0, double p1) {
    PL_REQUIRE(op >= 0 && op <= 6, PL_EINVAL, "pl_unary_f32: bad op %d", op);
    return launch_unary(ctx, x, y, n, OpMath{op, (float)p0, (float)p1});
}

int pl_binary_f32(pl_ctx *ctx, const float *a, const float *b, float *y, int outer, int C, int inner, int op,
                  int a_mode, int b_mode) {
    PL_REQUIRE(ctx && a && b && y, PL_EINVAL, "pl_binary_f32: null argument");
    PL_REQUIRE(op >= 0 && op <= 4 && a_mode >= 0 && a_mode <= 2 && b_mode >= 0 && b_mode <= 2, PL_EINVAL,
               "pl_binary_f32: bad op / broadcast mode");
    PL_REQUIRE(outer >= 0 && C > 0 && inner > 0, PL_EINVAL, "pl_binary_f32: bad shape");
    const size_t n = (size_t)outer * C * inner;
    if (!n) return PL_OK;
    PL_REQUIRE(n < (1ull << 32), PL_EUNSUPPORTED, "binary op: tensor too large");
    CtxGuard g(ctx);
    binary_kernel<<<stream_grid(ctx, n), TPB, 0, ctx->stream>>>(a, b, y, n, C, op, a_mode, b_mode, FastDiv(inner),
                                                              FastDiv(C));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_binary_bcast_f32(pl_ctx *ctx, const float *a, const float *b, float *y, int ndim, const int *shape,
                        const long long *a_stride, const long long *b_stride, int op) {
    PL_REQUIRE(ctx && shape && a_stride && b_stride, PL_EINVAL, "pl_binary_bcast_f32: null argument");
    PL_REQUIRE(ndim >= 1 && ndim <= 6, PL_EUNSUPPORTED, "pl_binary_bcast_f32: 1..6 axes supported, got %d", ndim);
    PL_REQUIRE(op >= 0 && op <= 4, PL_EINVAL, "pl_binary_bcast_f32: bad op %d", op);
    BcastArgs p;
    p.ndim = ndim;
    size_t n = 1;
    for (int d = 0; d < ndim; ++d) {
        PL_REQUIRE(shape[d] >= 0 && a_stride[d] >= 0 && b_stride[d] >= 0, PL_EINVAL, "pl_binary_bcast_f32: bad axis %d", d);
        p.shape[d] = (unsigned)shape[d];
        p.sa[d] = a_stride[d];
        p.sb[d] = b_stride[d];
        n *= (size_t)shape[d];
    }
    if (!n) return PL_OK;
    PL_REQUIRE(a && b && y, PL_EINVAL, "pl_binary_bcast_f32: null tensor");
    PL_REQUIRE(n < (1ull << 32), PL_EUNSUPPORTED, "binary op: tensor too large");
    CtxGuard g(ctx);
    binary_bcast_kernel<<<stream_grid(ctx, n), TPB, 0, ctx->stream>>>(a, b, y, n, op, p);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_upsample_linear_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W, int fh, int fw,
                           const float *weights) {
    PL_REQUIRE(ctx && x && y && weights, PL_EINVAL, "pl_upsample_linear_f32: null argument");
    PL_REQUIRE(NC >= 0 && H > 0 && W > 0 && fh > 0 && fw > 0, PL_EINVAL, "pl_upsample_linear_f32: bad shape");
    PL_REQUIRE(fh * fw > 1, PL_EINVAL, "pl_upsample_linear_f32: factors 1 x 1 are the identity");
    PL_REQUIRE(fh * fw <= 64, PL_EUNSUPPORTED, "pl_upsample_linear_f32: fh * fw <= 64 supported, got %d", fh * fw);
    const size_t total = (size_t)NC * H * fh * W * fw;
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "upsample: tensor too large");
    UpLinArgs p;
    p.H = H; p.W = W; p.fh = fh; p.fw = fw;
    p.terms = (fh > 1 && fw > 1) ? 4 : 2;
    for (int i = 0; i < 4 * 64; ++i) p.w[i] = i < p.terms * fh * fw ? weights[i] : 0.f;
    CtxGuard g(ctx);
    upsample_linear_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, (unsigned)total, p, FastDiv(W * fw),
                                                                         FastDiv(H * fh));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_resize_linear_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W, int OH, int OW, const int *ra,
                         const float *rs, const int *ca, const float *cs) {
    PL_REQUIRE(ctx && x && y && ra && rs && ca && cs, PL_EINVAL, "pl_resize_linear_f32: null argument");
    PL_REQUIRE(NC >= 0 && H > 1 && W > 1 && OH > 0 && OW > 0, PL_EINVAL, "pl_resize_linear_f32: bad shape (needs H, W >= 2)");
    const size_t total = (size_t)NC * OH * OW;
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total) && (size_t)NC * H * W < (1ull << 32), PL_EUNSUPPORTED, "resize: tensor too large");
    CtxGuard g(ctx);
    resize_planes_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, (unsigned)total, H, W, ra, rs, ca, cs,
                                                                       FastDiv(OW), FastDiv(OH));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_softmax_f32(pl_ctx *ctx, const float *x, float *y, int rows, int cols, int log_softmax) {
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "pl_softmax_f32: null argument");
    PL_REQUIRE(rows >= 0 && cols > 0, PL_EINVAL, "pl_softmax_f32: bad shape");
    if (!rows) return PL_OK;
    CtxGuard g(ctx);
    softmax_kernel<<<stream_grid(ctx, (size_t)rows * 64), TPB, 0, ctx->stream>>>(x, y, rows, cols, log_softmax);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_reduce_f32(pl_ctx *ctx, const float *x, float *y, int rows, int cols, int op) {
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "pl_reduce_f32: null argument");
    PL_REQUIRE(rows >= 0 && cols > 0 && op >= 0 && op <= 3, PL_EINVAL, "pl_reduce_f32: bad argument");
    if (!rows) return PL_OK;
    CtxGuard g(ctx);
    reduce_rows_kernel<<<stream_grid(ctx, (size_t)rows * 64), TPB, 0, ctx->stream>>>(x, y, rows, cols, op);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_transpose_f32(pl_ctx *ctx, const float *x, float *y, int ndim, const int *shape, const int *perm) {
    PL_REQUIRE(ctx && x && y && shape && perm, PL_EINVAL, "pl_transpose_f32: null argument");
    PL_REQUIRE(ndim >= 1 && ndim <= 6, PL_EUNSUPPORTED, "pl_transpose_f32: 1..6 axes");
    size_t istr[6], total = 1;
    for (int d = ndim - 1; d >= 0; --d) {
        PL_REQUIRE(shape[d] >= 0 && perm[d] >= 0 && perm[d] < ndim, PL_EINVAL, "pl_transpose_f32: bad shape/perm");
        istr[d] = total;
        total *= (size_t)shape[d];
    }
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "transpose: tensor too large");
    PermArgs p;
    p.ndim = ndim;
    for (int d = 0; d < ndim; ++d) {
        p.oshape[d] = (unsigned)shape[perm[d]];
        p.istride[d] = (unsigned)istr[perm[d]];
    }
    CtxGuard g(ctx);
    transpose_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, (unsigned)total, p);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_relu_f32(pl_ctx *ctx, const float *x, float *y, size_t n) { return launch_unary(ctx, x, y, n, OpRelu{}); }

int pl_leakyrelu_f32(pl_ctx *ctx, const float *x, float *y, size_t n, double alpha) {
    // layer.py:49: a = array(alpha, f32), b = array(1-alpha, f32)
    return launch_unary(ctx, x, y, n, OpLeaky{(float)alpha, (float)(1.0 - alpha)});
}

int pl_sigmoid_f32(pl_ctx *ctx, const float *x, float *y, size_t n) { return launch_unary(ctx, x, y, n, OpSigmoid{}); }

int pl_add_f32(pl_ctx *ctx, const float *a, const float *b, float *y, size_t n) {
    PL_REQUIRE(ctx && (n == 0 || (a && b && y)), PL_EINVAL, "pl_add_f32: null argument");
    if (!n) return PL_OK;
    CtxGuard g(ctx);
    size_t n4 = 0;
    if (aligned16(a) && aligned16(b) && aligned16(y)) {
        n4 = n / 4;
        if (n4) add_vec4<<<stream_grid(ctx, n4), TPB, 0, ctx->stream>>>((const float4 *)a, (const float4 *)b, (float4 *)y, n4);
    }
    size_t done = n4 * 4;
    if (done < n) add_scalar<<<stream_grid(ctx, n - done), TPB, 0, ctx->stream>>>(a + done, b + done, y + done, n - done);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_scale_shift_f32(pl_ctx *ctx, const float *x, float *y, const float *scale, const float *shift,
                       int outer, int C, int inner) {
    PL_REQUIRE(scale, PL_EINVAL, "pl_scale_shift_f32: null scale");
    return launch_affine<true>(ctx, x, y, scale, shift, outer, C, inner);
}

int pl_add_channel_f32(pl_ctx *ctx, const float *a, const float *b_c, float *y, int outer, int C, int inner) {
    PL_REQUIRE(b_c, PL_EINVAL, "pl_add_channel_f32: null b");
    return launch_affine<false>(ctx, a, y, nullptr, b_c, outer, C, inner);
}

int pl_pool2d_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W, int kh, int kw, int sh, int sw,
                  int pt, int pl, int pb, int pr, int mode) {
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "pl_pool2d_f32: null argument");
    PL_REQUIRE(NC >= 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0, PL_EINVAL, "pl_pool2d_f32: bad shape");
    PL_REQUIRE(mode == 0 || mode == 1, PL_EINVAL, "pl_pool2d_f32: mode must be 0 (max) or 1 (avg)");
    // util.pad grows each side by pads[0]/pads[1] only (util.py:8)
    PL_REQUIRE(pt == pb && pl == pr, PL_EUNSUPPORTED, "asymmetric pads are undefined in the reference (util.py:8)");
    int Ho = (H + pt + pb - kh + sh) / sh, Wo = (W + pl + pr - kw + sw) / sw;  // util.py:84-85
    PL_REQUIRE(Ho > 0 && Wo > 0, PL_EINVAL, "pl_pool2d_f32: empty output");
    size_t total = (size_t)NC * Ho * Wo;
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total) && (size_t)NC * H * W < (1ull << 32), PL_EUNSUPPORTED, "pool: tensor too large");
    CtxGuard g(ctx);
    if (mode == 0 && kh == 3 && kw == 3 && sh == 2 && sw == 2 && pt == 1 && pl == 1 && H == 2 * Ho && W == 2 * Wo &&
        Wo % 4 == 0 && aligned16(x) && aligned16(y)) {
        const unsigned total4 = (unsigned)(total / 4);
        maxpool_k3s2p1_x4<<<stream_grid(ctx, total4), TPB, 0, ctx->stream>>>(x, y, total4, H, W, Ho, Wo / 4,
                                                                         FastDiv(Wo / 4), FastDiv(Ho));
        PL_LAUNCH_CHECK();
        return PL_OK;
    }
    unsigned grid = stream_grid(ctx, total);
    if (mode == 0)
        pool2d_kernel<0><<<grid, TPB, 0, ctx->stream>>>(x, y, (unsigned)total, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl, FastDiv(Wo), FastDiv(Ho));
    else
        pool2d_kernel<1><<<grid, TPB, 0, ctx->stream>>>(x, y, (unsigned)total, H, W, Ho, Wo, kh, kw, sh, sw, pt, pl, FastDiv(Wo), FastDiv(Ho));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_upsample_nearest_f32(pl_ctx *ctx, const float *x, float *y, int NC, int H, int W, int fh, int fw) {
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "pl_upsample_nearest_f32: null argument");
    PL_REQUIRE(NC >= 0 && H > 0 && W > 0 && fh > 0 && fw > 0, PL_EINVAL, "pl_upsample_nearest_f32: bad shape");
    size_t total = (size_t)NC * H * fh * W * fw;
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "upsample: tensor too large");
    CtxGuard g(ctx);
    upsample_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(x, y, (unsigned)total, H, W, H * fh, W * fw,
                                                                  FastDiv(W * fw), FastDiv(H * fh), FastDiv(fh), FastDiv(fw));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_copy2d_f32(pl_ctx *ctx, float *dst, size_t dst_pitch, const float *src, size_t src_pitch, size_t width,
                  size_t rows) {
    PL_REQUIRE(ctx && (width * rows == 0 || (dst && src)), PL_EINVAL, "pl_copy2d_f32: null argument");
    PL_REQUIRE(dst_pitch >= width && src_pitch >= width, PL_EINVAL, "pl_copy2d_f32: pitch < width");
    size_t total = width * rows;
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "copy2d: tensor too large");
    CtxGuard g(ctx);
    if (aligned16(dst) && aligned16(src) && width % 4 == 0 && dst_pitch % 4 == 0 && src_pitch % 4 == 0) {
        unsigned w4 = (unsigned)(width / 4), t4 = (unsigned)(total / 4);
        copy2d_vec4<<<stream_grid(ctx, t4), TPB, 0, ctx->stream>>>((float4 *)dst, dst_pitch / 4, (const float4 *)src,
                                                                 src_pitch / 4, w4, t4, FastDiv(w4));
    } else {
        copy2d_scalar<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(dst, dst_pitch, src, src_pitch, (unsigned)width,
                                                                     (unsigned)total, FastDiv((unsigned)width));
    }
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_gap_f32(pl_ctx *ctx, const float *x, float *y, int rows, int inner) {
    PL_REQUIRE(ctx && x && y, PL_EINVAL, "pl_gap_f32: null argument");
    PL_REQUIRE(rows >= 0 && inner > 0, PL_EINVAL, "pl_gap_f32: bad shape");
    if (!rows) return PL_OK;
    CtxGuard g(ctx);
    gap_kernel<<<stream_grid(ctx, (size_t)rows * 64), TPB, 0, ctx->stream>>>(x, y, rows, inner, 1.f / (float)inner);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_pool2d_q4_f32(pl_ctx *ctx, const float *xq, float *yq, int N, int C, int H, int W, int kh, int kw, int sh,
                     int sw, int pt, int pl, int pb, int pr, int mode) {
    PL_REQUIRE(ctx && xq && yq, PL_EINVAL, "pl_pool2d_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0, PL_EINVAL,
               "pl_pool2d_q4_f32: bad shape");
    PL_REQUIRE(mode == 0 || mode == 1, PL_EINVAL, "pl_pool2d_q4_f32: mode must be 0 (max) or 1 (avg)");
    PL_REQUIRE(pt == pb && pl == pr, PL_EUNSUPPORTED, "asymmetric pads are undefined in the reference (util.py:8)");
    PL_REQUIRE(aligned16(xq) && aligned16(yq), PL_EINVAL, "pl_pool2d_q4_f32: Q4 tensors must be 16-byte aligned");
    const int Ho = (H + pt + pb - kh + sh) / sh, Wo = (W + pl + pr - kw + sw) / sw;  // util.py:84-85
    PL_REQUIRE(Ho > 0 && Wo > 0, PL_EINVAL, "pl_pool2d_q4_f32: empty output");
    const size_t NC = (size_t)N * ((C + 3) / 4), total = NC * Ho * Wo;
    if (!total) return PL_OK;
    PL_REQUIRE(total < (1ull << 30) && NC * H * W < (1ull << 30), PL_EUNSUPPORTED, "pool: tensor too large");
    CtxGuard g(ctx);
    if (mode == 0 && kh == 3 && kw == 3 && sh == 2 && sw == 2 && pt == 1 && pl == 1 && !getenv("PLANER_HIP_POOL_GENERIC") &&
        (size_t)N * ((C + 3) / 4) * H * W < (1ull << 27)) {
        const int Hb = (Ho + 1) / 2;
        const size_t blocks = total / ((size_t)Ho * Wo) * Hb * Wo;
        maxpool_q4_k3s2p1_2x1<<<stream_grid(ctx, blocks), TPB, 0, ctx->stream>>>((const float4 *)xq, (float4 *)yq, (unsigned)blocks, H, W,
                                                                                Ho, Wo, Hb, (unsigned)((size_t)N * ((C + 3) / 4) * H * W * 16),
                                                                                FastDiv(Wo), FastDiv(Hb));
        PL_LAUNCH_CHECK();
        return PL_OK;
    }
    const unsigned grid = stream_grid(ctx, total);
    if (mode == 0)
        pool2d_q4_kernel<0><<<grid, TPB, 0, ctx->stream>>>((const float4 *)xq, (float4 *)yq, (unsigned)total, H, W, Ho, Wo,
                                                         kh, kw, sh, sw, pt, pl, FastDiv(Wo), FastDiv(Ho));
    else
        pool2d_q4_kernel<1><<<grid, TPB, 0, ctx->stream>>>((const float4 *)xq, (float4 *)yq, (unsigned)total, H, W, Ho, Wo,
                                                         kh, kw, sh, sw, pt, pl, FastDiv(Wo), FastDiv(Ho));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_upsample_nearest_q4_f32(pl_ctx *ctx, const float *xq, float *yq, int N, int C, int H, int W, int fh, int fw) {
    PL_REQUIRE(ctx && xq && yq, PL_EINVAL, "pl_upsample_nearest_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && fh > 0 && fw > 0, PL_EINVAL, "pl_upsample_nearest_q4_f32: bad shape");
    PL_REQUIRE(aligned16(xq) && aligned16(yq), PL_EINVAL, "pl_upsample_nearest_q4_f32: Q4 tensors must be 16-byte aligned");
    const size_t total = (size_t)N * ((C + 3) / 4) * H * fh * W * fw;
    if (!total) return PL_OK;
    PL_REQUIRE(total < (1ull << 30), PL_EUNSUPPORTED, "upsample: tensor too large");
    CtxGuard g(ctx);
    upsample_q4_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(
        (const float4 *)xq, (float4 *)yq, (unsigned)total, H, W, H * fh, W * fw, FastDiv(W * fw), FastDiv(H * fh),
        FastDiv(fh), FastDiv(fw));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// The channel-quad twin of pl_upsample_linear_f32: same host weight table, same two-term forms, same limits.  `resq`: NULL or a
// Q4 tensor of the output's shape, added in the write pass (a rounding of its own).
int pl_upsample_linear_q4_f32(pl_ctx *ctx, const float *xq, float *yq, const float *resq, int N, int C, int H, int W, int fh,
                              int fw, const float *weights) {
    PL_REQUIRE(ctx && xq && yq && weights, PL_EINVAL, "pl_upsample_linear_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && fh > 0 && fw > 0, PL_EINVAL, "pl_upsample_linear_q4_f32: bad shape");
    PL_REQUIRE(fh * fw > 1, PL_EINVAL, "pl_upsample_linear_q4_f32: factors 1 x 1 are the identity");
    PL_REQUIRE(fh <= 64 && fw <= 64 && fh * fw <= 64, PL_EUNSUPPORTED, "pl_upsample_linear_q4_f32: fh * fw <= 64 supported, got %d",
               fh * fw);
    PL_REQUIRE(aligned16(xq) && aligned16(yq) && aligned16(resq), PL_EINVAL,
               "pl_upsample_linear_q4_f32: Q4 tensors must be 16-byte aligned");
    PL_REQUIRE(xq != yq, PL_EINVAL, "pl_upsample_linear_q4_f32: cannot run in place");
    const size_t total = (size_t)N * ((C + 3) / 4) * H * fh * W * fw;
    if (!total) return PL_OK;
    PL_REQUIRE(total < (1ull << 30), PL_EUNSUPPORTED, "upsample: tensor too large");
    UpLinArgs p;
    p.H = H; p.W = W; p.fh = fh; p.fw = fw;
    p.terms = (fh > 1 && fw > 1) ? 4 : 2;
    for (int i = 0; i < 4 * 64; ++i) p.w[i] = i < p.terms * fh * fw ? weights[i] : 0.f;
    CtxGuard g(ctx);
    upsample_linear_q4_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(
        (const float4 *)xq, (float4 *)yq, (const float4 *)resq, (unsigned)total, p, FastDiv(W * fw), FastDiv(H * fh));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// The channel-quad twin of pl_resize_linear_f32: same device position tables (ra, rs: OH entries; ca, cs: OW entries).
int pl_resize_linear_q4_f32(pl_ctx *ctx, const float *xq, float *yq, const float *resq, int N, int C, int H, int W, int OH,
                            int OW, const int *ra, const float *rs, const int *ca, const float *cs) {
    PL_REQUIRE(ctx && xq && yq && ra && rs && ca && cs, PL_EINVAL, "pl_resize_linear_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && H > 1 && W > 1 && OH > 0 && OW > 0, PL_EINVAL,
               "pl_resize_linear_q4_f32: bad shape (needs H, W >= 2)");
    PL_REQUIRE(aligned16(xq) && aligned16(yq) && aligned16(resq), PL_EINVAL,
               "pl_resize_linear_q4_f32: Q4 tensors must be 16-byte aligned");
    PL_REQUIRE(xq != yq, PL_EINVAL, "pl_resize_linear_q4_f32: cannot run in place");
    const size_t total = (size_t)N * ((C + 3) / 4) * OH * OW;
    if (!total) return PL_OK;
    PL_REQUIRE(total < (1ull << 30) && (size_t)N * ((C + 3) / 4) * H * W < (1ull << 30), PL_EUNSUPPORTED, "resize: tensor too large");
    CtxGuard g(ctx);
    resize_linear_q4_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(
        (const float4 *)xq, (float4 *)yq, (const float4 *)resq, (unsigned)total, H, W, ra, rs, ca, cs, FastDiv(OW), FastDiv(OH));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// Q4 tensor folded by (dh_in, dw_in) -> the same activation folded by (dh_out, dw_out); (1, 1) is the unfolded tensor, so this
// folds, unfolds and goes from one fold to another.  N, C, H, W: the UNFOLDED logical shape.
int pl_refold_q4_f32(pl_ctx *ctx, const float *xq, float *yq, int N, int C, int H, int W, int dh_in, int dw_in, int dh_out,
                     int dw_out) {
    PL_REQUIRE(ctx && xq && yq, PL_EINVAL, "pl_refold_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, PL_EINVAL, "pl_refold_q4_f32: bad shape");
    PL_REQUIRE(dh_in > 0 && dw_in > 0 && dh_out > 0 && dw_out > 0, PL_EINVAL, "pl_refold_q4_f32: a fold is at least 1");
    PL_REQUIRE(aligned16(xq) && aligned16(yq), PL_EINVAL, "pl_refold_q4_f32: Q4 tensors must be 16-byte aligned");
    PL_REQUIRE(xq != yq, PL_EINVAL, "pl_refold_q4_f32: not an in-place operation");
    const int Cq = (C + 3) / 4;
    // quads of the tensor folded by (dh, dw), saturating at 2^29: every factor is checked before the next multiplication
    auto quads = [&](int dh, int dw, int &Hf, int &Wf) {
        const size_t lim = 1ull << 29;
        Hf = (H + dh - 1) / dh;
        Wf = (W + dw - 1) / dw;
        size_t t = (size_t)N;
        for (size_t f : {(size_t)dh, (size_t)dw, (size_t)Cq, (size_t)Hf, (size_t)Wf}) {
            if (t >= lim) return lim;
            t *= f;                                             // t < 2^29, f < 2^31
        }
        return t < lim ? t : lim;
    };
    int Hi, Wi, Ho, Wo;
    const size_t in_total = quads(dh_in, dw_in, Hi, Wi), total = quads(dh_out, dw_out, Ho, Wo);
    PL_REQUIRE(in_total < (1ull << 29) && total < (1ull << 29) && loop32_ok(ctx, total), PL_EUNSUPPORTED,
               "pl_refold_q4_f32: Q4 tensor of 2^29 pixel quads (8 GiB) or more");
    if (!total) return PL_OK;
    CtxGuard g(ctx);
    refold_q4_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(
        (const float4 *)xq, (float4 *)yq, (unsigned)total, Cq, H, W, Hi, Wi, dh_in, dw_in, dh_out, dw_out, FastDiv(Wo), FastDiv(Ho),
        FastDiv(Cq), FastDiv(dw_out), FastDiv(dh_out), FastDiv(dh_in), FastDiv(dw_in));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// Pixel shuffle / unshuffle of a Q4 tensor (pixel_shuffle_q4_kernel.h).  N, C, H, W: the NARROW side -- a shuffle's
// output, an unshuffle's input; the other side is (N, C r^2, H / r, W / r).
int pl_pixel_shuffle_q4_f32(pl_ctx *ctx, const float *xq, float *y, int N, int C, int H, int W, int r, int order, int inverse,
                            int nchw_out) {
    namespace ps = pixel_shuffle_q4;
    PL_REQUIRE(ctx && xq && y, PL_EINVAL, "pl_pixel_shuffle_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, PL_EINVAL, "pl_pixel_shuffle_q4_f32: bad shape");
    PL_REQUIRE(order == 0 || order == 1, PL_EINVAL, "pl_pixel_shuffle_q4_f32: order is 0 (CRD) or 1 (DCR)");
    PL_REQUIRE(r >= 2 && r <= 4, PL_EUNSUPPORTED, "pl_pixel_shuffle_q4_f32: r = 2, 3, 4 supported, got %d", r);
    PL_REQUIRE(H % r == 0 && W % r == 0, PL_EINVAL, "pl_pixel_shuffle_q4_f32: H and W (the narrow side's) must be multiples of r");
    PL_REQUIRE(order == 0 || C % 4 == 0, PL_EUNSUPPORTED, "pl_pixel_shuffle_q4_f32: DCR order needs C %% 4 == 0, got C = %d", C);
    PL_REQUIRE(!(nchw_out && inverse), PL_EINVAL, "pl_pixel_shuffle_q4_f32: nchw_out goes with a shuffle (inverse = 0) only");
    PL_REQUIRE(aligned16(xq) && aligned16(y), PL_EINVAL, "pl_pixel_shuffle_q4_f32: tensors must be 16-byte aligned");
    PL_REQUIRE(xq != y, PL_EINVAL, "pl_pixel_shuffle_q4_f32: not an in-place operation");
    const size_t lim = 1ull << 29;
    // quads of one side, saturating at 2^29: every factor is checked before the next multiplication
    auto quads = [&](size_t cq, size_t h, size_t w) {
        size_t t = (size_t)N;
        for (size_t f : {cq, h, w}) {
            if (t >= lim) return lim;
            t *= f;                                             // t < 2^29, f < 2^33
        }
        return t < lim ? t : lim;
    };
    ps::Geom g;
    g.C = C;
    g.Cq = (C + 3) / 4;
    const size_t cqw = ((size_t)C * r * r + 3) / 4;              // C < 2^31, r^2 <= 16
    g.Hs = H / r;
    g.Ws = W / r;
    const size_t narrow = quads((size_t)g.Cq, (size_t)H, (size_t)W), wide = quads(cqw, (size_t)g.Hs, (size_t)g.Ws);
    const size_t total = quads((size_t)g.Cq, (size_t)g.Hs, (size_t)g.Ws);       // one thread per (narrow quad, small pixel)
    PL_REQUIRE(narrow < lim && wide < lim && loop32_ok(ctx, total), PL_EUNSUPPORTED,
               "pl_pixel_shuffle_q4_f32: Q4 tensor of 2^29 pixel quads (8 GiB) or more");
    if (!total) return PL_OK;
    g.CqW = (int)cqw;                                            // wide < 2^29 and total > 0: cqw < 2^29
    g.divWs = FastDiv(g.Ws); g.divHs = FastDiv(g.Hs); g.divCq = FastDiv(g.Cq);
    CtxGuard guard(ctx);
    const unsigned n = (unsigned)total;
    switch (r * 2 + order) {
    case 4: launch_pixel_shuffle_q4<2, 0>(ctx, xq, y, n, g, inverse, nchw_out); break;
    case 5: launch_pixel_shuffle_q4<2, 1>(ctx, xq, y, n, g, inverse, nchw_out); break;
    case 6: launch_pixel_shuffle_q4<3, 0>(ctx, xq, y, n, g, inverse, nchw_out); break;
    case 7: launch_pixel_shuffle_q4<3, 1>(ctx, xq, y, n, g, inverse, nchw_out); break;
    case 8: launch_pixel_shuffle_q4<4, 0>(ctx, xq, y, n, g, inverse, nchw_out); break;
    default: launch_pixel_shuffle_q4<4, 1>(ctx, xq, y, n, g, inverse, nchw_out); break;
    }
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_concat2_q4_f32(pl_ctx *ctx, const float *aq, const float *bq, float *yq, int N, int Ca, int Cb, int H, int W, int fh,
                      int fw) {
    PL_REQUIRE(ctx && aq && bq && yq, PL_EINVAL, "pl_concat2_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && Ca > 0 && Cb > 0 && H > 0 && W > 0 && fh > 0 && fw > 0 && Ca % 4 == 0 && Cb % 4 == 0 && H % fh == 0 &&
                   W % fw == 0, PL_EINVAL, "pl_concat2_q4_f32: bad shape (channel counts must be multiples of 4, H, W of the factors)");
    PL_REQUIRE(aligned16(aq) && aligned16(bq) && aligned16(yq), PL_EINVAL, "pl_concat2_q4_f32: Q4 tensors must be 16-byte aligned");
    const size_t total = (size_t)N * ((Ca + Cb) / 4) * H * W;
    if (!total) return PL_OK;
    PL_REQUIRE(total < (1ull << 30), PL_EUNSUPPORTED, "concat: tensor too large");
    CtxGuard g(ctx);
    concat2_q4_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(
        (const float4 *)aq, (const float4 *)bq, (float4 *)yq, (unsigned)total, Ca / 4, Cb / 4, H, W, H / fh, W / fw,
        FastDiv(H * W), FastDiv((Ca + Cb) / 4), FastDiv(W), FastDiv(fh), FastDiv(fw));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_gap_q4_f32(pl_ctx *ctx, const float *xq, float *y, int N, int C, int HW) {
    PL_REQUIRE(ctx && xq && y, PL_EINVAL, "pl_gap_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && HW > 0, PL_EINVAL, "pl_gap_q4_f32: bad shape");
    PL_REQUIRE(aligned16(xq), PL_EINVAL, "pl_gap_q4_f32: Q4 tensor must be 16-byte aligned");
    const int Cq = (C + 3) / 4;
    const size_t rows = (size_t)N * Cq;
    if (!rows) return PL_OK;
    PL_REQUIRE(rows < (1ull << 31), PL_EUNSUPPORTED, "gap: tensor too large");
    CtxGuard g(ctx);
    gap_q4_kernel<<<stream_grid(ctx, rows * 64), TPB, 0, ctx->stream>>>((const float4 *)xq, y, (int)rows, Cq, C, HW,
                                                                     1.f / (float)HW);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

int pl_scale_shift_q4_f32(pl_ctx *ctx, const float *xq, float *yq, const float *scale, const float *shift, int N,
                          int C, int HW) {
    PL_REQUIRE(ctx && xq && yq && scale && shift, PL_EINVAL, "pl_scale_shift_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && HW > 0, PL_EINVAL, "pl_scale_shift_q4_f32: bad shape");
    PL_REQUIRE(aligned16(xq) && aligned16(yq), PL_EINVAL, "pl_scale_shift_q4_f32: Q4 tensors must be 16-byte aligned");
    const int Cq = (C + 3) / 4;
    const size_t total = (size_t)N * Cq * HW;
    if (!total) return PL_OK;
    PL_REQUIRE(total < (1ull << 30), PL_EUNSUPPORTED, "scale_shift: tensor too large");
    CtxGuard g(ctx);
    affine_q4_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>((const float4 *)xq, (float4 *)yq, scale, shift,
                                                                   (unsigned)total, C, Cq, FastDiv(HW), FastDiv(Cq));
    PL_LAUNCH_CHECK();
    return PL_OK;
}

// layer.InstanceNormalization on a Q4 tensor, in place, y = IN(x) [+ res] [relu] (instnorm_q4_kernel.h).  The form
// depends on HW alone: one workgroup per (image, quad) up to PL_INSTNORM_Q4_ONE_WG_PIXELS pixels, chunk statistics into a pool
// block + merge-and-apply above.
int pl_instancenorm_q4_f32(pl_ctx *ctx, float *xq, const float *scale, const float *bias, const float *resq, int N, int C, int HW,
                           double eps, int act) {
    namespace iq = instnorm_q4;
    PL_REQUIRE(ctx && xq && scale && bias, PL_EINVAL, "pl_instancenorm_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && HW >= 0, PL_EINVAL, "pl_instancenorm_q4_f32: bad shape");
    PL_REQUIRE(act == PL_ACT_NONE || act == PL_ACT_RELU, PL_EINVAL, "pl_instancenorm_q4_f32: act must be 0 (none) or 1 (relu)");
    PL_REQUIRE(aligned16(xq) && aligned16(resq), PL_EINVAL, "pl_instancenorm_q4_f32: Q4 tensors must be 16-byte aligned");
    const int Cq = (C + 3) / 4;
    const size_t rows = (size_t)N * Cq, total = rows * (size_t)HW;
    if (!total) return PL_OK;
    PL_REQUIRE(total <= (1ull << 29), PL_EUNSUPPORTED, "instancenorm: tensor too large");
    CtxGuard g(ctx);
    float4 *x = (float4 *)xq;
    const float4 *res = (const float4 *)resq;
    const float e = (float)eps;
    const int tail_id = (resq ? 2 : 0) | (act == PL_ACT_RELU ? 1 : 0);
    if (HW <= PL_INSTNORM_Q4_ONE_WG_PIXELS) {
        const dim3 grid((unsigned)rows), block(iq::TPB);
        switch (tail_id) {
        case 0: iq::instnorm_q4_one_wg_kernel<false, false><<<grid, block, 0, ctx->stream>>>(x, scale, bias, res, Cq, C, HW, e); break;
        case 1: iq::instnorm_q4_one_wg_kernel<false, true><<<grid, block, 0, ctx->stream>>>(x, scale, bias, res, Cq, C, HW, e); break;
        case 2: iq::instnorm_q4_one_wg_kernel<true, false><<<grid, block, 0, ctx->stream>>>(x, scale, bias, res, Cq, C, HW, e); break;
        default: iq::instnorm_q4_one_wg_kernel<true, true><<<grid, block, 0, ctx->stream>>>(x, scale, bias, res, Cq, C, HW, e); break;
        }
        PL_LAUNCH_CHECK();
        ctx->last_plan = "instnorm-q4 one-wg";
        return PL_OK;
    }
    // rows * S <= total / CHUNK + rows < 2^19: one-dimensional grids
    const int S = (HW + PL_INSTNORM_Q4_CHUNK_PIXELS - 1) / PL_INSTNORM_Q4_CHUNK_PIXELS;
    const int A = S < iq::APPLY_MAX_WG_PER_ROW ? S : iq::APPLY_MAX_WG_PER_ROW;
    float4 *part = nullptr;
    int rc = pl_alloc(ctx, rows * S * 2 * sizeof(float4), (void **)&part);
    if (rc != PL_OK) return rc;
    iq::instnorm_q4_stats_kernel<<<dim3((unsigned)(rows * S)), dim3(iq::TPB), 0, ctx->stream>>>(x, part, S, HW);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) {
        const dim3 grid((unsigned)(rows * A)), block(iq::TPB);
        switch (tail_id) {
        case 0: iq::instnorm_q4_apply_kernel<false, false><<<grid, block, 0, ctx->stream>>>(x, part, scale, bias, res, Cq, C, HW, S, A, e); break;
        case 1: iq::instnorm_q4_apply_kernel<false, true><<<grid, block, 0, ctx->stream>>>(x, part, scale, bias, res, Cq, C, HW, S, A, e); break;
        case 2: iq::instnorm_q4_apply_kernel<true, false><<<grid, block, 0, ctx->stream>>>(x, part, scale, bias, res, Cq, C, HW, S, A, e); break;
        default: iq::instnorm_q4_apply_kernel<true, true><<<grid, block, 0, ctx->stream>>>(x, part, scale, bias, res, Cq, C, HW, S, A, e); break;
        }
        le = hipGetLastError();
    }
    pl_free(ctx, part);  // stream-ordered: safe to recycle after the enqueue
    if (le != hipSuccess) {
        pl_set_error("pl_instancenorm_q4_f32: kernel launch -> %s", hipGetErrorString(le));
        return PL_EHIP;
    }
    ctx->last_plan = "instnorm-q4 chunks=" + std::to_string(S);
    return PL_OK;
}

int pl_splitk_reduce_f32(pl_ctx *ctx, const float *ws, int splits, float *y, int N, int C, int inner,
                         const float *bias, const float *scale, const float *shift, const float *res, int act,
                         double alpha) {
    PL_REQUIRE(ctx && ws && y && splits >= 1, PL_EINVAL, "pl_splitk_reduce_f32: bad argument");
    size_t total = (size_t)N * C * inner;
    if (!total) return PL_OK;
    PL_REQUIRE(loop32_ok(ctx, total), PL_EUNSUPPORTED, "splitk reduce: tensor too large");
    CtxGuard g(ctx);
    Epilogue ep = make_epilogue(bias, scale, shift, res, act, alpha);
    splitk_reduce_kernel<<<stream_grid(ctx, total), TPB, 0, ctx->stream>>>(ws, splits, total, y, (unsigned)total, C,
                                                                        FastDiv(inner), FastDiv(C), ep);
    PL_LAUNCH_CHECK();
    return PL_OK;
}

}  // extern "C"

// Group normalisation on a Q4 tensor, in place: y = IN_g(x) [* gamma] [+ beta] [+ res] [relu] (groupnorm_q4_kernel.h).
// The form depends on cpg = C / G and HW alone: wide (cpg % 4 == 0: a group is one run of cpg / 4 * HW float4s), pair (cpg == 2)
// or single (cpg == 1) rows; one workgroup per row up to PL_INSTNORM_Q4_ONE_WG_PIXELS float4s, chunk statistics into a pool block +
// merge-and-apply above.
template <int LANES>
static hipError_t groupnorm_q4_launch(pl_ctx *ctx, float4 *x, float4 *part, const float *gs, const float *gb, const float *gamma,
                                      const float *beta, const float4 *res, size_t rows, int rpi, int C, int cpg, int L, int HW, int S,
                                      float e, int tail_id) {
    namespace gq = groupnorm_q4;
    const dim3 block(gq::TPB);
    const FastDiv divHW((unsigned)HW);
    if (!part) {
        const dim3 grid((unsigned)rows);
        switch (tail_id) {
        case 0: gq::groupnorm_q4_one_wg_kernel<LANES, false, false><<<grid, block, 0, ctx->stream>>>(x, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, e); break;
        case 1: gq::groupnorm_q4_one_wg_kernel<LANES, false, true><<<grid, block, 0, ctx->stream>>>(x, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, e); break;
        case 2: gq::groupnorm_q4_one_wg_kernel<LANES, true, false><<<grid, block, 0, ctx->stream>>>(x, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, e); break;
        default: gq::groupnorm_q4_one_wg_kernel<LANES, true, true><<<grid, block, 0, ctx->stream>>>(x, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, e); break;
        }
        return hipGetLastError();
    }
    const int A = S < gq::APPLY_MAX_WG_PER_ROW ? S : gq::APPLY_MAX_WG_PER_ROW;
    gq::groupnorm_q4_stats_kernel<LANES><<<dim3((unsigned)(rows * S)), block, 0, ctx->stream>>>(x, part, S, L);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return le;
    const dim3 grid((unsigned)(rows * A));
    switch (tail_id) {
    case 0: gq::groupnorm_q4_apply_kernel<LANES, false, false><<<grid, block, 0, ctx->stream>>>(x, part, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, S, A, e); break;
    case 1: gq::groupnorm_q4_apply_kernel<LANES, false, true><<<grid, block, 0, ctx->stream>>>(x, part, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, S, A, e); break;
    case 2: gq::groupnorm_q4_apply_kernel<LANES, true, false><<<grid, block, 0, ctx->stream>>>(x, part, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, S, A, e); break;
    default: gq::groupnorm_q4_apply_kernel<LANES, true, true><<<grid, block, 0, ctx->stream>>>(x, part, gs, gb, gamma, beta, res, rpi, C, cpg, L, divHW, S, A, e); break;
    }
    return hipGetLastError();
}

extern "C" int pl_groupnorm_q4_f32(pl_ctx *ctx, float *xq, const float *gscale, const float *gbias, const float *gamma, const float *beta,
                                   const float *resq, int N, int C, int HW, int G, double eps, int act) {
    PL_REQUIRE(ctx && xq && gscale && gbias, PL_EINVAL, "pl_groupnorm_q4_f32: null argument");
    PL_REQUIRE(N >= 0 && C > 0 && HW >= 0 && G > 0, PL_EINVAL, "pl_groupnorm_q4_f32: bad shape");
    PL_REQUIRE(C % G == 0, PL_EINVAL, "pl_groupnorm_q4_f32: the group count must divide the channel count");
    PL_REQUIRE(act == PL_ACT_NONE || act == PL_ACT_RELU, PL_EINVAL, "pl_groupnorm_q4_f32: act must be 0 (none) or 1 (relu)");
    PL_REQUIRE(aligned16(xq) && aligned16(resq), PL_EINVAL, "pl_groupnorm_q4_f32: Q4 tensors must be 16-byte aligned");
    const int cpg = C / G;
    PL_REQUIRE(cpg % 4 == 0 || cpg == 2 || cpg == 1, PL_EUNSUPPORTED,
               "pl_groupnorm_q4_f32: %d channels per group split a channel quad unevenly (1, 2 or a multiple of 4 have a Q4 form)", cpg);
    const int Cq = (C + 3) / 4;
    const size_t total = (size_t)N * Cq * (size_t)HW;
    if (!total) return PL_OK;
    PL_REQUIRE(total <= (1ull << 29), PL_EUNSUPPORTED, "groupnorm: tensor too large");
    CtxGuard g(ctx);
    const int lanes = cpg % 4 == 0 ? 4 : cpg;
    const int rpi = lanes == 4 ? G : Cq;                                  // rows per image
    const size_t rows = (size_t)N * rpi;
    const int L = (int)(total / rows);                                    // float4s per row: cpg / 4 * HW, or HW
    const int tail_id = (resq ? 2 : 0) | (act == PL_ACT_RELU ? 1 : 0);
    const bool chunked = L > PL_INSTNORM_Q4_ONE_WG_PIXELS;
    // rows * S <= total / CHUNK + rows < 2^30: one-dimensional grids
    const int S = chunked ? (L + PL_INSTNORM_Q4_CHUNK_PIXELS - 1) / PL_INSTNORM_Q4_CHUNK_PIXELS : 1;
    float4 *part = nullptr;
    if (chunked) {
        int rc = pl_alloc(ctx, rows * S * 2 * sizeof(float4), (void **)&part);
        if (rc != PL_OK) return rc;
    }
    float4 *x = (float4 *)xq;
    const float4 *res = (const float4 *)resq;
    const float e = (float)eps;
    hipError_t le;
    if (lanes == 4) le = groupnorm_q4_launch<4>(ctx, x, part, gscale, gbias, gamma, beta, res, rows, rpi, C, cpg, L, HW, S, e, tail_id);
    else if (lanes == 2) le = groupnorm_q4_launch<2>(ctx, x, part, gscale, gbias, gamma, beta, res, rows, rpi, C, cpg, L, HW, S, e, tail_id);
    else le = groupnorm_q4_launch<1>(ctx, x, part, gscale, gbias, gamma, beta, res, rows, rpi, C, cpg, L, HW, S, e, tail_id);
    if (part) pl_free(ctx, part);  // stream-ordered: safe to recycle after the enqueue
    if (le != hipSuccess) {
        pl_set_error("pl_groupnorm_q4_f32: kernel launch -> %s", hipGetErrorString(le));
        return PL_EHIP;
    }
    ctx->last_plan = std::string("groupnorm-q4 ") + (lanes == 4 ? "wide" : lanes == 2 ? "pair" : "single") +
                     (chunked ? " chunks=" + std::to_string(S) : std::string(" one-wg"));
    return PL_OK;
}
