// Depthwise convolution (group == Cin == Cout: one filter plane per channel) on the vector ALUs -- included by conv_direct.hip
// inside its anonymous namespace.  Reference semantics: layer.Conv2d (layer.py:22-26) -> util.conv_for (util.py:17-44) with
// Cin/group == 1, i.e. y[n,c] = sum_taps x[n,c](shifted) * K[c,0,ky,kx], then the plan's fused tail.
//
// Why a kernel of its own: the implicit-GEMM kernels see a depthwise conv as C GEMMs of ONE output row and K = kh*kw, so at
// least 31 of the 32 MFMA rows of their smallest tile are padding.  The operation itself does 2*kh*kw FLOP per 8 compulsory
// bytes (read x once, write y once): it is bound by HBM traffic, and fp32 FMAs on the VALU are more than enough.
//
// One workgroup = one (image, channel or channel quad, output tile).  Its filter plane is uniform across the workgroup and is
// read with scalar loads.  The input window of the tile -- tile rows plus the halo rows and columns the taps reach, zero where
// the window hangs over the padding -- is staged in LDS once, so each input byte comes from HBM about once.  A lane then owns
// one output pixel at a time (consecutive lanes = consecutive pixels of a row, so the stores of a wave are contiguous):
//   * T = float4 (channel-quad tensors [N][C/4][H][W][4], filter [C/4][kh*kw][4]): one 16-byte LDS read and four FMAs per tap,
//     16-byte stores;
//   * T = float (NCHW tensors, OIHW filter [C][1][kh][kw]): one 4-byte read and one FMA per tap.
// Taps are summed in (ky, kx) order as one fmaf chain per output; the epilogue is the shared fused tail (apply_epilogue /
// apply_epilogue4).  Windows too large for the LDS budget (huge dilations or rows) take the STAGED = false form, which reads
// every tap straight from global memory with a bounds check.
struct DwArgs {
    const float *x, *w;
    float *y;
    Epilogue ep;
    int planes;                      // channels (float) or channel quads (float4) per image
    int chans;                       // logical channel count (masks the padding lanes of a partial last quad)
    int H, W, Ho, Wo;
    int kh, kw, sh, sw, dh, dw, pt, pl;
    int tile_rows, tile_cols;        // output tile of a workgroup
    int in_rows, in_cols;            // its staged input window
    int tiles_x;                     // column tiles per plane
    FastDiv div_cols, div_in_cols;   // by tile_cols, in_cols
};

__device__ __forceinline__ float dw_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ float4 dw_fma(float4 a, float4 b, float4 c) {
    return make_float4(__fmaf_rn(a.x, b.x, c.x), __fmaf_rn(a.y, b.y, c.y), __fmaf_rn(a.z, b.z, c.z), __fmaf_rn(a.w, b.w, c.w));
}
template <class T> __device__ __forceinline__ T dw_zero();
template <> __device__ __forceinline__ float dw_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 dw_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// KH = KW = 0: filter extents from the arguments (any kh x kw); otherwise compile-time extents, whose taps are loaded into
// (scalar) registers before the first store.
template <class T, int KH, int KW, bool STAGED>
__global__ void __launch_bounds__(256) conv_dw_kernel(const DwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    T *win = reinterpret_cast<T *>(smem);                                    // [in_rows][in_cols]
    const int kh = KH ? KH : p.kh, kw = KW ? KW : p.kw;
    const int c = blockIdx.y, n = blockIdx.z;
    const int ty = (int)blockIdx.x / p.tiles_x, tx = (int)blockIdx.x - ty * p.tiles_x;
    const int oy0 = ty * p.tile_rows, ox0 = tx * p.tile_cols;
    const int iy0 = oy0 * p.sh - p.pt, ix0 = ox0 * p.sw - p.pl;
    const size_t plane = (size_t)n * p.planes + c;
    const T *xp = reinterpret_cast<const T *>(p.x) + plane * p.H * p.W;
    T *yp = reinterpret_cast<T *>(p.y) + plane * p.Ho * p.Wo;
    const T *wp = reinterpret_cast<const T *>(p.w) + (size_t)c * kh * kw;

    constexpr int KK = KH * KW > 0 ? KH * KW : 1;
    T wr[KK];
    if constexpr (KH > 0) {
#pragma unroll
        for (int t = 0; t < KK; ++t) wr[t] = wp[t];
    }
    // per-channel parameters of the fused tail (uniform)
    float4 bs4, sc4, sh4;
    if constexpr (sizeof(T) == 16) {
        float b[4], s[4], h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) load_chan_params(p.ep, min(c * 4 + e, p.chans - 1), b[e], s[e], h[e]);
        bs4 = make_float4(b[0], b[1], b[2], b[3]);
        sc4 = make_float4(s[0], s[1], s[2], s[3]);
        sh4 = make_float4(h[0], h[1], h[2], h[3]);
    }

    if constexpr (STAGED) {
        // the input window -> LDS, four requests in flight per thread before the first LDS write
        const int total = p.in_rows * p.in_cols, step = blockDim.x;
        for (int base = threadIdx.x; base < total; base += 4 * step) {
            T v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = base + j * step;
                v[j] = dw_zero<T>();
                if (e < total) {
                    unsigned r, col;
                    p.div_in_cols.divmod((unsigned)e, r, col);
                    const int gy = iy0 + (int)r, gx = ix0 + (int)col;
                    if ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) v[j] = xp[(size_t)gy * p.W + gx];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (base + j * step < total) win[base + j * step] = v[j];
        }
        __syncthreads();
    }

    const int npix = p.tile_rows * p.tile_cols;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        unsigned r, col;
        p.div_cols.divmod((unsigned)i, r, col);
        const int oy = oy0 + (int)r, ox = ox0 + (int)col;
        if (oy >= p.Ho || ox >= p.Wo) continue;
        T acc = dw_zero<T>();
        for (int ky = 0; ky < kh; ++ky) {
#pragma unroll
            for (int kx = 0; kx < kw; ++kx) {
                T wv, xv;
                if constexpr (KH > 0) wv = wr[ky * KW + kx];
                else wv = wp[ky * kw + kx];
                if constexpr (STAGED) {
                    xv = win[((int)r * p.sh + ky * p.dh) * p.in_cols + (int)col * p.sw + kx * p.dw];
                } else {
                    const int gy = oy * p.sh - p.pt + ky * p.dh, gx = ox * p.sw - p.pl + kx * p.dw;
                    xv = ((unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) ? xp[(size_t)gy * p.W + gx] : dw_zero<T>();
                }
                acc = dw_fma(xv, wv, acc);
            }
        }
        const size_t o = (size_t)oy * p.Wo + ox;
        if constexpr (sizeof(T) == 16) {
            const size_t idx4 = plane * p.Ho * p.Wo + o;
            const float4 rs = p.ep.res ? reinterpret_cast<const float4 *>(p.ep.res)[idx4] : make_float4(0.f, 0.f, 0.f, 0.f);
            yp[o] = apply_epilogue4(p.ep, bs4, sc4, sh4, rs, min(4, p.chans - c * 4), acc);
        } else {
            yp[o] = apply_epilogue(p.ep, acc, c, plane * p.Ho * p.Wo + o);
        }
    }
}

// OIHW [C][1][kh][kw] -> [C/4][kh*kw][4], zero-padded quads (pl_conv2d_prepare_dw_q4_f32)
__global__ void pack_filter_dw_q4_kernel(const float *__restrict__ w, float *__restrict__ out, unsigned total, int C, int taps) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned e = i & 3u, qt = i >> 2, q = qt / (unsigned)taps, t = qt - q * (unsigned)taps;
        const unsigned ch = q * 4u + e;
        out[i] = ch < (unsigned)C ? w[(size_t)ch * taps + t] : 0.f;
    }
}
