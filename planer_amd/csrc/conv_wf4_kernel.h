// Fully fused Winograd F(4x4,3x3) convolution on channel-quad tensors -- included by conv_winograd.hip inside its
// anonymous namespace (uses Epilogue, FastDiv, apply_epilogue4).
//
// For 3x3 / stride 1 / pad 1 / group 1 convs (util.conv_for, util.py:17-44, with the fused tail of layer.py:125-127,
// 93-95, 44-51).  The staged pipeline (input transform -> 36 grouped GEMMs -> output transform) needs 4x fewer
// multiplies than the direct conv but moves V and M -- 2.25x the activation each, written and read -- through
// memory; the fused 1-D kernel (conv_w1d4_kernel) moves nothing extra but only halves the multiplies.  Here ONE
// workgroup carries a block of tiles x 64 output channels through all 36 frequencies:
//   * A wave owns 16 output channels x 16 tiles as 36 accumulator blocks of v_mfma_f32_16x16x4_f32 (144 of its 256
//     registers, amdgpu_waves_per_eu(2,2)): lane (i = lane % 16, rg = lane / 16) ends up holding, for ITS tile i and ITS channel
//     quad 4 rg .. 4 rg + 3, all 36 frequencies -- so the output transform A^T m A is lane-local; the fused tail and the stores
//     go through a wave-private LDS exchange that turns (tile, quad) lanes into (tile, pixel) lanes: one store covers a
//     contiguous 1 KB run.  M never exists.  (The first version had 4 waves x 288 accumulators: 67 us against 48 us -- the
//     compiler shuffled through AGPRs.)
//   * What ships: BLOCKS OF 16 TILES ON FOUR WAVES (template parameter HALF).  Wave wm owns output channels [16 wm, 16 wm + 16)
//     x the 16 tiles.  A workgroup holds half the registers of a CU, so two of them -- or one and another kernel's workgroups
//     -- share a CU with barriers of their own: one's prologue, store tail and barrier waits run under the other's K loop.
//     Layer2 conv of ResNet-18 at batch 32: 43.7 against 62.1 us alone (224 instead of 112 workgroups), bench.py 58.1-58.4 k
//     against 55.9-56.2 k img/s (profiles/r06_ab_wf4_half_blocks.txt).
//   * The oracle: BLOCKS OF 32 TILES ON EIGHT WAVES, two per SIMD (PLANER_HIP_EXPERIMENT=wf4_half=0).  Wave (wm, wn) = (wave / 2,
//     wave % 2) owns channels [16 wm, 16 wm + 16) x tiles [16 wn, 16 wn + 16).  One workgroup owns the CU.
//   * K runs over input channel quads (one quad = one chunk = one MFMA K step of 4), one barrier per chunk.  Per chunk the
//     workgroup holds in LDS, double buffered: the input patch P of the block's tiles -- (4 BR + 2) x (4 BC + 2) pixels per
//     image, halo shared between neighbouring tiles, stored [row][x mod 4][x div 4] as 16-byte cells (by LDS-DMA straight from
//     the activation, zero fill by the range check; 512 cells = 8 KB for 16 tiles, 1024 = 16 KB for 32) -- and the transformed
//     patch V[wn][4 k][16 tiles][36] (9.2 KB per 16 tiles) that wave-items compute from P (B^T d B, a channel pair per lane,
//     packed arithmetic): V never leaves the CU.  LDS per workgroup: 34.8 KB with 16 tiles (36.9 KB woven, see below), 69.6 KB
//     with 32.  In iteration c the waves request chunk c + 2's patch (one request behind each of the first MFMA groups) and
//     transform P[(c+1)&1] into V[(c+1)&1]; every buffer written in an interval was last read in the previous one.
//   * The filter never touches LDS: it is laid out [cout block][chunk][16-channel block][group of 4 frequencies][lane][4]
//     (wf4_filter_kernel), so the fragment a wave needs for one group of four MFMAs is ONE 16-byte load per lane over a
//     contiguous 1 KB, global -> registers, requested WF4_GA_AHEAD = five groups ahead into a ring of WF4_GA_SLOTS = six register
//     slots (profiles/r06_wf4_stalls.md: 39.2 / 60.2 against 40.3 / 62.6 us per layer1 / layer2 conv with the slice staged in LDS,
//     110 KB less LDS traffic per K step, 69.6 instead of 143 KB of LDS for the 32-tile block).
//   * The 16-tile block's K step is WOVEN (template parameter WEAVE): no transform phase in front of the MFMAs -- every wave
//     carries a two-row item of chunk c + 1 in pieces behind single MFMAs of chunk c (mma_weave: reads, first stage column by
//     column, second stage, V writes; scheduling barriers pin the pieces).  One branch-free instruction stream for all four
//     waves: an item's kind is per-wave DATA (row bases, coefficients; the three-row kind reads its fourth row out of 1 KB of
//     -0.0 behind the patch buffer), wave 0 repeats wave 1's item.  No scratch.  Per conv alone /
//     per 32 images at batch 256: layer1 37.0 / 30.3 against 38.7 / 31.9 us, layer2 41.1 / 26.7 against 44.0 / 27.6 us
//     (profiles/wf4_weave.md).
//   * The PHASED K step (mma_ga; PLANER_HIP_EXPERIMENT=wf4_weave=0, and the 32-tile block always): the transform is a phase of
//     its own.  16 tiles: three TWO-ROW wave-items (wf4_transform_2rows: lane = row of a pair x tile x channel pair) on waves 1-3
//     in front of their MFMAs.  32 tiles: six one-row items (wf4_transform_row2: lane = tile x channel pair) -- waves 4-7 rows
//     0-3 BEFORE their 36 MFMAs of chunk c, waves 0-1 rows 4-5 after theirs, so that the two waves of a SIMD alternate on its
//     matrix pipe.  The woven step is bit-identical to the phased one (tests/test_gpu_wf4_weave.py).
//   * HEAD AND TAIL of the 16-tile block (a layer1 block issues as many vector instructions outside its 16 K steps as inside,
//     beside the sibling workgroup's K loop; profiles/wf4_head_tail.md): the accumulators are never cleared -- K step 0 is a copy
//     of the step that multiplies into a literal zero; after the loop the first stage of A^T m A runs ONCE over the
//     accumulators, in place (wf4_column_sums: 156 packed operations where the row-by-row form of the 32-tile block spends 204),
//     which frees the registers that used to spill in the output rows: 238-244 registers, no scratch anywhere; the four store
//     offsets of output row 0 are computed once and rows 1-3 add the row pitch (no multiply, no branch inside the rows); scale
//     and shift of the straight-line tail come by one range-checked 16-byte load each.  The last K step still carries its
//     transform item: peeling it as well makes the register allocator copy the accumulators (240-510 spilled registers).
//     The 32-tile block keeps the head and tail these replaced, value for value the same.
//   * Fragment reads of V are conflict free by layout: a lane's 36 frequencies of one (k, tile) are 144 consecutive bytes.
//   * What a K step of the 32-tile block with the filter in LDS cost (profiles/r04_wf4_knockout.md): 1.00 us of MFMAs + 0.36
//     fragment reads + 0.38 transform + 0.13 both LDS-DMA streams = 1.61 us; fp32 MFMAs do not overlap with the other vector
//     instructions of their SIMD.  The 16-tile form's table: profiles/wf4_weave.md.
// Executed MFMA work = 36/16 of a GEMM per output pixel = 4x fewer multiplies than the direct conv (tile and
// channel padding aside); HBM traffic = x + y (+ residual) + the filter.
// Forms measured and dropped (filter slice staged in LDS, patch stored channel plane by channel plane, register-staged operands, every wave multiplying
// first): DESIGN.md, the fused F(4x4,3x3) items, and profiles/r06_wf4_stalls.md.

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Wf4Args {
    const float *x;        // [N][Cq][H][W][4]
    const float *u;        // [cout block of 64][chunk = cin/4][wm = 16-channel block][g = 4 frequencies][lane = 16 k + i][4]   (pl_conv2d_prepare_wf4_f32)
    float *y;              // [N][Coq][H][W][4]
    int N, Cq, Coq, H, W, th, tw;
    int nchunks;           // Cin / 4
    int lBR, lBC;          // log2(tile rows), log2(tile columns) of a block; images per block NB = 32 >> (lBR + lBC)
    int R, S;              // patch rows 4 BR + 2; 16-byte cells per x phase BC + 1
    int cells;             // NB * R * 4 * S cells of one patch
    int rblocks, cblocks, cout_blocks;
    // PACK: the block's spare slot columns (BC - tw of them, one image per block, one column block) carry tiles of a DONOR image --
    // of every G = tw / sc + 1 images the last one is cut into (th / BR) x (tw / sc) groups of BR x sc tiles, one per block of the
    // other G - 1: no padding slots (a 56-pixel map: 196 real tiles in 7 blocks of 32 per image -> 49 blocks per 8 images instead of 56)
    int pack_sc, pack_g, pack_gc;      // spare columns, images per group, donor groups per tile row (tw / sc); 0: off
    unsigned x_bytes, u_bytes, y_bytes;
    FastDiv divPlane, div4S, divS, divCoB, divCb, divRb;
    Epilogue ep;
};

// probe builds only (tools/wf4_knock.sh): bit 0 unused (it dropped the filter's LDS-DMA while the filter slice was staged in
// LDS; the numbering stays so that profiles/r04_wf4_knockout.md reads as written), 1 no patch LDS-DMA, 2 no patch transform,
// 3 no MFMAs, 4 no fragment reads, 5 no output rows -- results are garbage, the time tells what a K step's parts cost.  Bits 2-4
// act on both forms of the K step (phased, woven).
#ifndef WF4_KNOCK
#define WF4_KNOCK 0
#endif
// the filter fragments' rolling prefetch: WF4_GA_AHEAD MFMA groups deep into a ring of WF4_GA_SLOTS register slots
#ifndef WF4_GA_AHEAD
#define WF4_GA_AHEAD 5
#endif
#ifndef WF4_GA_SLOTS
#define WF4_GA_SLOTS 6
#endif
// probe builds only (-DWF4_STAMP, tools/wf4_stamp.py): s_memtime of wave 0 / wave 4 of every block at kernel entry, after chunk 0
// has landed, after the prologue, after the K loop and after the last output row
#ifdef WF4_STAMP
__device__ unsigned long long wf4_stamps[4096 * 2 * 8];
#define WF4_MARK(i)                                                                                          \
    do {                                                                                                     \
        if ((wave == 0 || wave == 4) && lane == 0 && blockIdx.x < 4096)                                       \
            wf4_stamps[(blockIdx.x * 2 + (wave >> 2)) * 8 + (i)] = __builtin_amdgcn_s_memtime();             \
    } while (0)
// ... and inside K steps 6 and 7 of every block, per wave: step entry, transform_first done, MFMAs done, transform_last done,
// barrier passed
__device__ unsigned long long wf4_step_stamps[512 * 8 * 2 * 8];
#define WF4_STEP_MARK(c, i)                                                                                  \
    do {                                                                                                     \
        if (((c) == 6 || (c) == 7) && lane == 0 && blockIdx.x < 512)                                          \
            wf4_step_stamps[((blockIdx.x * 8 + wave) * 2 + ((c) - 6)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define WF4_MARK(i)
#define WF4_STEP_MARK(c, i)
#endif
constexpr int WF4_A_FLOATS = 36 * 256;                  // one (cout block, chunk) of the prepared filter: 64 channels x 4 k x 36 frequencies
constexpr int WF4_V_FLOATS = 2 * 36 * 64, WF4_P_PASSES = 2;      // V of 32 tiles; patch passes of one cell per thread
constexpr int WF4_P_CELLS = 1024, WF4_P_FLOATS = WF4_P_CELLS * 4;      // patch of 32 tiles (16 tiles: half of each)

// One transform wave-item of the 32-tile block: row A of B^T d B for TWO channels per lane -- every value is a channel pair out
// of one 8-byte LDS read and every operation a packed one, no operand shuffling.  Lanes = 32 tiles x 2 channel pairs (pair
// fastest: consecutive lanes read consecutive 8 bytes).  All the patch values the row needs are requested before the first is
// used; the rows of d with a zero coefficient in row A of B^T are never read (the compiler drops those loads).
typedef float wf4_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ wf4_v2 wf4_fma2(float a, wf4_v2 b, wf4_v2 c) { return __builtin_elementwise_fma((wf4_v2){a, a}, b, c); }
__device__ __forceinline__ void wf4_bt2(const wf4_v2 (&d)[6], wf4_v2 (&o)[6]) {
    const wf4_v2 s = d[4] - d[2], t = d[3] - d[1];
    o[0] = wf4_fma2(4.f, d[0], wf4_fma2(-5.f, d[2], d[4]));
    o[1] = wf4_fma2(-4.f, d[1] + d[2], d[3] + d[4]);
    o[2] = wf4_fma2(4.f, d[1] - d[2], d[4] - d[3]);
    o[3] = wf4_fma2(2.f, t, s);
    o[4] = wf4_fma2(-2.f, t, s);
    o[5] = wf4_fma2(4.f, d[1], wf4_fma2(-5.f, d[3], d[5]));
}
template <int A>
__device__ __forceinline__ wf4_v2 wf4_bt_row2(const wf4_v2 (&d)[6]) {
    if constexpr (A == 0) return wf4_fma2(4.f, d[0], wf4_fma2(-5.f, d[2], d[4]));
    else if constexpr (A == 1) return wf4_fma2(-4.f, d[1] + d[2], d[3] + d[4]);
    else if constexpr (A == 2) return wf4_fma2(4.f, d[1] - d[2], d[4] - d[3]);
    else if constexpr (A == 3) return wf4_fma2(2.f, d[3] - d[1], d[4] - d[2]);
    else if constexpr (A == 4) return wf4_fma2(-2.f, d[3] - d[1], d[4] - d[2]);
    else return wf4_fma2(4.f, d[1], wf4_fma2(-5.f, d[3], d[5]));
}
// pbase: float index of the pair's first value in the tile's first patch cell; vbase: float index of V[half][even channel][i][0]
// (the odd channel's row is 16 x 36 floats further on); rs = floats per patch row, ps = floats per x phase
template <int A, int rs, int ps>
__device__ __forceinline__ void wf4_transform_row2(const float *P, float *V, int pbase, int vbase) {
    wf4_v2 d[6][6];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const float *col = P + pbase + (b & 3) * ps + (b >> 2) * 4;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            constexpr bool used[6][6] = {{1, 0, 1, 0, 1, 0}, {0, 1, 1, 1, 1, 0}, {0, 1, 1, 1, 1, 0},
                                         {0, 1, 1, 1, 1, 0}, {0, 1, 1, 1, 1, 0}, {0, 1, 0, 1, 0, 1}};
            d[b][k] = used[A][k] ? *reinterpret_cast<const wf4_v2 *>(col + k * rs) : (wf4_v2){0.f, 0.f};
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    wf4_v2 m[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) m[b] = wf4_bt_row2<A>(d[b]);
    wf4_v2 o[6];
    wf4_bt2(m, o);
    float *v0 = V + vbase + A * 6, *v1 = v0 + 16 * 36;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        v0[j] = o[j].x;
        v1[j] = o[j].y;
    }
}

// TWO rows of B^T d B per wave-item, for blocks of 16 tiles (HALF): lane = [row select r][tile, 4 bits][channel pair].  The rows of a
// pair share their loads up to a per-lane base (KIND 0: rows 0 / 5 read patch rows r, r + 2, r + 4) or read the same four patch
// rows with per-lane coefficients (KIND 1: rows 1 / 2, KIND 2: rows 3 / 4 -- each is c1 d1 + c2 d2 + c3 d3 + d4): three wave-items
// transform a 16-tile block where the one-row form would need six half-empty ones.  pbase: as for wf4_transform_row2, plus r rows
// for KIND 0; vbase: float index of V[even channel][tile][6 A(r)].
template <int KIND, int rs, int ps>
__device__ __forceinline__ void wf4_transform_2rows(const float *P, float *V, int pbase, int vbase, int r) {
    constexpr int NR = KIND == 0 ? 3 : 4;
    wf4_v2 d[6][NR];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const float *col = P + pbase + (b & 3) * ps + (b >> 2) * 4;
#pragma unroll
        for (int k = 0; k < NR; ++k)
            d[b][k] = *reinterpret_cast<const wf4_v2 *>(col + (KIND == 0 ? 2 * k : k + 1) * rs);
    }
    __builtin_amdgcn_sched_barrier(0);
    wf4_v2 m[6];
    if constexpr (KIND == 0) {
#pragma unroll
        for (int b = 0; b < 6; ++b) m[b] = wf4_fma2(4.f, d[b][0], wf4_fma2(-5.f, d[b][1], d[b][2]));
    } else {
        // rows 1 / 2: (-4, -4, 1) / (4, -4, -1);  rows 3 / 4: (-2, -1, 2) / (2, -1, -2)
        const float c1 = KIND == 1 ? (r ? 4.f : -4.f) : (r ? 2.f : -2.f);
        const float c2 = KIND == 1 ? -4.f : -1.f;
        const float c3 = KIND == 1 ? (r ? -1.f : 1.f) : (r ? -2.f : 2.f);
#pragma unroll
        for (int b = 0; b < 6; ++b) m[b] = wf4_fma2(c1, d[b][0], wf4_fma2(c2, d[b][1], wf4_fma2(c3, d[b][2], d[b][3])));
    }
    wf4_v2 o[6];
    wf4_bt2(m, o);
    float *v0 = V + vbase, *v1 = v0 + 16 * 36;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        v0[j] = o[j].x;
        v1[j] = o[j].y;
    }
}

// A^T m A on channel PAIRS (the accumulator's registers 0-1 and 2-3 are natural pairs): packed arithmetic throughout, the
// operations and their order are those of w4_at4_row / w4_at4.
template <int A>
__device__ __forceinline__ wf4_v2 wf4_at_row2(const wf4_v2 (&m)[6]) {
    if constexpr (A == 0) return (m[0] + (m[1] + m[2])) + (m[3] + m[4]);
    else {
        const wf4_v2 q = m[1] - m[2], t = m[3] - m[4], pp = m[1] + m[2], r = m[3] + m[4];
        if constexpr (A == 1) return q + 2.f * t;
        else if constexpr (A == 2) return pp + 4.f * r;
        else return (q + 8.f * t) + m[5];
    }
}
__device__ __forceinline__ void wf4_at2(const wf4_v2 (&m)[6], wf4_v2 (&o)[4]) {
    const wf4_v2 pp = m[1] + m[2], q = m[1] - m[2], r = m[3] + m[4], t = m[3] - m[4];
    o[0] = (m[0] + pp) + r;
    o[1] = q + 2.f * t;
    o[2] = pp + 4.f * r;
    o[3] = (q + 8.f * t) + m[5];
}
// Coalesced form of the row for the tail the convolutions of a residual net carry (per-channel scale and shift, [residual,]
// ReLU, no bias).  In the MFMA's C layout a lane owns one tile x one channel quad, so a 16-byte
// store instruction scatters 64 pieces at 64-byte strides over four channel planes -- the end-of-kernel store burst of all
// workgroups ran at ~2 TB/s.  Here the row goes through a wave-private LDS buffer [b][quad][tile] (68-cell rows: the padding
// makes the read-back conflict-free) and comes back as lane = (tile, pixel b of the tile's row): one instruction then writes
// (and, for the residual, reads) 16 tiles x 4 pixels = one contiguous 1 KB run of a channel plane.  Scale and shift are applied
// before the exchange (a lane knows its quad's parameters there), residual and ReLU after it: the same operations in the same
// order on every value.
// PLAIN: that tail written straight (packed operations, no per-element option selects); otherwise the general fused tail in
// the same two halves -- bias / scale / shift before the exchange, residual / activation / late residual after it.
// second half of an output row: the six column sums s[b] (pairs lo / hi of the lane's channel quad) -> the row's four pixels,
// tail, exchange, stores
template <bool RES, bool PLAIN>
__device__ __forceinline__ void wf4_row_finish(const Wf4Args &p, const wf4_v2 (&slo)[6], const wf4_v2 (&shi)[6], int cqc, float4 scale,
                                               float4 shift, float4 *xb, int wr_cell, int rd_cell,
                                               const __amdgpu_buffer_rsrc_t yrsrc, const __amdgpu_buffer_rsrc_t rrsrc,
                                               const int (&off)[4]) {
    float4 rs[4];
    if constexpr (RES) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rs[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, off[q], 0, 0));
    }
    wf4_v2 olo[4], ohi[4];
    wf4_at2(slo, olo);
    wf4_at2(shi, ohi);
    if constexpr (PLAIN) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            olo[b] = olo[b] * (wf4_v2){scale.x, scale.y} + (wf4_v2){shift.x, shift.y};
            ohi[b] = ohi[b] * (wf4_v2){scale.z, scale.w} + (wf4_v2){shift.z, shift.w};
        }
    }
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // (the general form fetches its quad's parameters here, row by row: twelve more registers held across the whole epilogue
    //  would spill beside the accumulators)
    float4 gbias = z4, gscale = z4, gshift = z4;
    if constexpr (!PLAIN) {
        if (p.ep.bias) gbias = reinterpret_cast<const float4 *>(p.ep.bias)[cqc];
        if (p.ep.scale) gscale = reinterpret_cast<const float4 *>(p.ep.scale)[cqc];
        if (p.ep.shift) gshift = reinterpret_cast<const float4 *>(p.ep.shift)[cqc];
    }
    Epilogue affine = p.ep, rest = p.ep;          // the general tail's two halves (apply_epilogue4 skips what is null / 0)
    affine.res = nullptr; affine.act = 0;
    rest.bias = rest.scale = rest.shift = nullptr;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float4 o = make_float4(olo[b].x, olo[b].y, ohi[b].x, ohi[b].y);
        if constexpr (!PLAIN) o = apply_epilogue4(affine, gbias, gscale, gshift, z4, 4, o);
        xb[b * 68 + wr_cell] = o;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = xb[rd_cell + q * 16];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                   // the next row overwrites the buffer
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 o;
        if constexpr (PLAIN) {
            wf4_v2 lo = (wf4_v2){v[q].x, v[q].y}, hi = (wf4_v2){v[q].z, v[q].w};
            if constexpr (RES) {
                lo = lo + (wf4_v2){rs[q].x, rs[q].y};
                hi = hi + (wf4_v2){rs[q].z, rs[q].w};
            }
            const wf4_v2 zl = lo * 0.f, zh = hi * 0.f;     // relu_ref: x > 0 ? x : x * 0
            o = make_float4(lo.x > 0.f ? lo.x : zl.x, lo.y > 0.f ? lo.y : zl.y, hi.x > 0.f ? hi.x : zh.x, hi.y > 0.f ? hi.y : zh.y);
        } else {
            o = apply_epilogue4(rest, z4, z4, z4, RES ? rs[q] : z4, 4, v[q]);
        }
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, o),
                                               yrsrc, off[q], 0, 0);
    }
}

template <int A, bool RES, bool PLAIN>
__device__ __forceinline__ void wf4_output_row_coalesced(const Wf4Args &p, const f32x4 (&acc)[36], int cqc, float4 scale,
                                                         float4 shift, float4 *xb, int wr_cell, int rd_cell,
                                                         const __amdgpu_buffer_rsrc_t yrsrc, const __amdgpu_buffer_rsrc_t rrsrc,
                                                         const int (&off)[4]) {
    wf4_v2 slo[6], shi[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        wf4_v2 m[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) m[a] = __builtin_shufflevector(acc[a * 6 + b], acc[a * 6 + b], 0, 1);
        slo[b] = wf4_at_row2<A>(m);
#pragma unroll
        for (int a = 0; a < 6; ++a) m[a] = __builtin_shufflevector(acc[a * 6 + b], acc[a * 6 + b], 2, 3);
        shi[b] = wf4_at_row2<A>(m);
    }
    wf4_row_finish<RES, PLAIN>(p, slo, shi, cqc, scale, shift, xb, wr_cell, rd_cell, yrsrc, rrsrc, off);
}

// 16-tile blocks: the column sums of A^T m A ONCE for all four output rows, in place -- wf4_at2 over acc[a * 6 + b], a = 0 .. 5, per
// column b and channel pair, its four results back into acc[A * 6 + b], A = 0 .. 3.  wf4_at2's expressions are those of
// wf4_at_row2<0 .. 3>, so every value is what the row-by-row form computes (which redoes m1 +- m2 and m3 +- m4 in each of the four
// rows: 204 packed operations against 156); rows 4 and 5 of the accumulators are free afterwards.
__device__ __forceinline__ void wf4_column_sums(f32x4 (&acc)[36]) {
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        wf4_v2 m[6], lo[4], hi[4];
#pragma unroll
        for (int a = 0; a < 6; ++a) m[a] = __builtin_shufflevector(acc[a * 6 + b], acc[a * 6 + b], 0, 1);
        wf4_at2(m, lo);
#pragma unroll
        for (int a = 0; a < 6; ++a) m[a] = __builtin_shufflevector(acc[a * 6 + b], acc[a * 6 + b], 2, 3);
        wf4_at2(m, hi);
#pragma unroll
        for (int A = 0; A < 4; ++A) acc[A * 6 + b] = (f32x4){lo[A].x, lo[A].y, hi[A].x, hi[A].y};
        // column by column: all six at once keep some forty temporaries alive beside the 144 accumulators, and the kernel spills.
        // (An empty statement that "uses" this column's results and "defines" the next column's inputs: nothing is emitted, and it
        // is what keeps the order -- a scheduling barrier does not bind plain arithmetic before instruction selection.)
        if (b < 5)
            asm volatile("" : "+v"(acc[b]), "+v"(acc[6 + b]), "+v"(acc[12 + b]), "+v"(acc[18 + b]),
                              "+v"(acc[b + 1]), "+v"(acc[6 + b + 1]), "+v"(acc[12 + b + 1]), "+v"(acc[18 + b + 1]),
                              "+v"(acc[24 + b + 1]), "+v"(acc[30 + b + 1]));
    }
}
// output row A from the sums wf4_column_sums left in acc[A * 6 + b]
template <int A, bool RES, bool PLAIN>
__device__ __forceinline__ void wf4_output_row_summed(const Wf4Args &p, const f32x4 (&acc)[36], int cqc, float4 scale, float4 shift,
                                                      float4 *xb, int wr_cell, int rd_cell, const __amdgpu_buffer_rsrc_t yrsrc,
                                                      const __amdgpu_buffer_rsrc_t rrsrc, const int (&off)[4]) {
    wf4_v2 slo[6], shi[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        slo[b] = __builtin_shufflevector(acc[A * 6 + b], acc[A * 6 + b], 0, 1);
        shi[b] = __builtin_shufflevector(acc[A * 6 + b], acc[A * 6 + b], 2, 3);
    }
    wf4_row_finish<RES, PLAIN>(p, slo, shi, cqc, scale, shift, xb, wr_cell, rd_cell, yrsrc, rrsrc, off);
}

// Variants (compile-time; the launcher picks one per block width, so that every patch read is base + immediate): PACK -- spare
// slot columns carry a donor image's tiles (Wf4Args); HALF -- 16 tiles on four waves instead of 32 on eight; WEAVE -- the woven
// K step instead of the phased one.
template <int LBC, bool PACK = false, bool HALF = false, bool WEAVE = false>
__device__ __forceinline__ void conv_wf4_body(const Wf4Args &p) {
    constexpr int NT = HALF ? 256 : 512, LT = HALF ? 4 : 5;          // threads, log2(tiles) of a block
    static_assert(!WEAVE || HALF, "woven K step: 16-tile blocks only");
    constexpr int S = (1 << LBC) + 1 + (PACK ? 1 : 0);      // 16-byte cells per x phase: compile time, so every patch read is base + immediate
    // four separate LDS objects (not one dynamic array): the compiler orders LDS-DMA against later LDS accesses object by
    // object, so a DMA into P0 does not hold up the reads of P1 / V0 and the writes of V1
    // (HALF: one tile half of V, 512 patch cells -- 34.8 KB a workgroup, so that what else runs on the CU keeps its LDS)
    __shared__ __attribute__((aligned(16))) float Vs0[WF4_V_FLOATS / (HALF ? 2 : 1)], Vs1[WF4_V_FLOATS / (HALF ? 2 : 1)];      // [wn][4 k][16 i][36 f]
    // (WEAVE: 1 KB of -0.0 behind each patch buffer -- the "fourth patch row" of the waves whose item reads three, see wv_p3)
    constexpr int P_TAIL = WEAVE ? 256 : 0, P_BODY = WF4_P_FLOATS / (HALF ? 2 : 1);
    __shared__ __attribute__((aligned(16))) float Ps0[P_BODY + P_TAIL], Ps1[P_BODY + P_TAIL];      // [cells][4]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = HALF ? wave : wave >> 1, wn = HALF ? 0 : wave & 1;       // 16 output channels x 16 tiles per wave
    const int li = lane & 15, lk = lane >> 4;      // MFMA: operand row / column i, k index (A, B) or row group (C)

    // ---- which block: cout block fastest (blocks that share input pixels are neighbours), then columns, rows, images ----
    unsigned t1, coutblk, t2, colblk, ngrp, rowblk;
    p.divCoB.divmod(blockIdx.x, t1, coutblk);
    p.divCb.divmod(t1, t2, colblk);
    p.divRb.divmod(t2, ngrp, rowblk);
    const int BRm = (1 << p.lBR) - 1, BCm = (1 << LBC) - 1, lT = p.lBR + LBC;
    int n0 = (int)ngrp << (LT - lT);
    const int ty0 = (int)rowblk << p.lBR, tx0 = (int)colblk << LBC;
    // PACK: ngrp counts the RECEIVING images (G - 1 of every G); the donor's tile group of this block: (dgr, dgc)
    int dn = 0, dgr = 0, dgc = 0;
    if constexpr (PACK) {
        const int grp = (int)ngrp / (p.pack_g - 1), i = (int)ngrp - grp * (p.pack_g - 1);
        n0 = grp * p.pack_g + i;
        dn = grp * p.pack_g + p.pack_g - 1;
        const int id = i * p.rblocks + (int)rowblk;
        dgr = id / p.pack_gc;
        dgc = id - dgr * p.pack_gc;
    }
    const int HW = p.H * p.W;

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.u), 0, p.u_bytes, 0x00020000);
    constexpr int OOB = (int)0x80000000;
    typedef __attribute__((address_space(3))) float lds_float;

    // ---- patch cells this thread fetches every chunk (16 bytes = the 4 channels of a pixel; the channel quad rides in the
    //      scalar offset) ----
    int pvoff[WF4_P_PASSES];
#pragma unroll
    for (int ps = 0; ps < WF4_P_PASSES; ++ps) {
        const unsigned ci = (unsigned)(ps * NT + tid);
        pvoff[ps] = OOB;
        if (ci < (unsigned)p.cells) {
            unsigned nb, rem, r_, rem2, m, s;
            p.divPlane.divmod(ci, nb, rem);
            p.div4S.divmod(rem, r_, rem2);
            p.divS.divmod(rem2, m, s);
            int n = n0 + (int)nb, h = 4 * ty0 + (int)r_ - 1, w = 4 * tx0 + (int)(4 * s + m) - 1;
            if constexpr (PACK) {
                // plane columns from 4 (tw + 1) on hold the donor group's patch (one cell right of where the spare slots would
                // read by themselves: the main image's last tile column shares its two halo columns with nobody)
                const int pc = (int)(4 * s + m) - 4 * (p.tw + 1);
                if (pc >= 0) {
                    n = dn;
                    h = (4 * dgr << p.lBR) + (int)r_ - 1;
                    w = 4 * p.pack_sc * dgc + pc - 1;
                    if (pc > 4 * p.pack_sc + 1) n = p.N;           // (past the donor patch: nothing)
                }
            }
            if (n < p.N && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W)
                pvoff[ps] = (int)(((unsigned)(n * p.Cq) * (unsigned)HW + (unsigned)(h * p.W + w)) << 4);
        }
    }
    // 16-byte cells land lane-linear: LDS-DMA writes them directly
    auto load_p = [&](int c, int buf) {
        const int soff = (c * HW) << 4;
        float *Pb = buf ? Ps1 : Ps0;
#pragma unroll
        for (int ps = 0; ps < WF4_P_PASSES; ++ps)
            if (ps * NT < p.cells && ps * NT + tid < p.cells)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_float *)(Pb + (ps * NT + tid - lane) * 4), 16, pvoff[ps], soff, 0, 0);
    };
    // one piece (1 KB per wave) of the patch after next: the K step issues them BETWEEN its MFMA groups, so that the ~100 issue
    // cycles an LDS-DMA instruction costs a wave are spent while the matrix pipe is busy (all in a row before the first MFMA
    // left the pipe idle at the head of every step: 40.9 -> 39.8 us per layer1 conv)
    auto load_p_piece = [&](int c, int buf, int ps) {
        const int soff = (c * HW) << 4;
        float *Pb = buf ? Ps1 : Ps0;
        if constexpr (WF4_KNOCK & 2) return;
        if (ps * NT < p.cells && ps * NT + tid < p.cells)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_float *)(Pb + (ps * NT + tid - lane) * 4), 16, pvoff[ps], soff, 0, 0);
    };

    // ---- transform.  32 tiles: a lane takes a channel PAIR of one of the block's tiles (wf4_transform_row2), so a whole row of
    //      B^T d B is ONE wave-item: six per step -- waves 4-7 rows 0-3, waves 0-1 rows 4-5.  16 tiles: three two-row items
    //      (wf4_transform_2rows) on waves 1-3, or the same items woven into every wave's MFMAs ----
    constexpr int rs = 16 * S, psz = 4 * S;                      // floats per patch row, per x phase
    int pb2 = 0, vb2 = 0;
    const int hr = lane >> 5;                                    // HALF: which row of its pair this lane transforms
    if constexpr (HALF) {
        const int tj = (lane >> 1) & 15, cp = lane & 1;
        const int t_nb = tj >> lT, t_r = (tj >> LBC) & BRm;
        int t_c = tj & BCm;
        if (PACK && t_c >= p.tw) t_c += 1;
        pb2 = 2 * cp + (((t_nb * p.R + 4 * t_r) * 4) * S + t_c) * 4;
        vb2 = ((2 * cp * 16) + tj) * 36;
    } else {
        const int tj = lane >> 1, cp = lane & 1;
        const int t_nb = tj >> lT, t_r = (tj >> LBC) & BRm;
        int t_c = tj & BCm;
        if (PACK && t_c >= p.tw) t_c += 1;                       // spare slots read the donor patch, one cell further right
        pb2 = 2 * cp + (((t_nb * p.R + 4 * t_r) * 4) * S + t_c) * 4;
        vb2 = ((((tj >> 4) * 4 + 2 * cp) * 16) + (tj & 15)) * 36;
    }
    // WEAVE: the wave's item as DATA, so that one instruction stream serves every wave.  Each column's first stage is
    //     m = c1 d0 + (c2 d1 + (c3 d2 + d3))        (fused multiply-adds, innermost first)
    // over four patch rows.  Waves 2 / 3 (wf4_transform_2rows' KIND 1 / 2): patch rows 1-4, coefficients of rows 1 / 2
    // (-4, -4, 1) / (4, -4, -1) and rows 3 / 4 (-2, -1, 2) / (2, -1, -2).  Waves 0 / 1 (KIND 0, rows 0 / 5 = 4 d0 - 5 d2 + d4 of patch
    // rows r, r + 2, r + 4): coefficients (4, -5, 1), and their d3 is read out of the -0.0 tail of the patch buffer --
    // fma(1, x, -0.0) is x for every x, signed zeros and infinities included, so the value that enters the c2 stage is the one
    // KIND 0 feeds it: bit-identical.  (d3 selected in registers instead, two v_cndmask per column: 1-2 % slower per conv.)
    // Bases (float index in the patch buffer): rows 1 and 3 of kinds 1 / 2 share wv_p13 with row 1 of kind 0.
    const bool wv_k0 = wave < 2;
    const int wv_p13 = wv_k0 ? pb2 + hr * rs : pb2;
    const int wv_p0 = wv_k0 ? pb2 + hr * rs : pb2 + rs;
    const int wv_p2 = wv_k0 ? pb2 + (hr + 4) * rs : pb2 + 3 * rs;
    const int wv_p3 = wv_k0 ? P_BODY : pb2 + 4 * rs;
    static_assert(!WEAVE || 3 * psz + 6 <= P_TAIL, "the -0.0 tail must cover every column offset");
    if constexpr (WEAVE) {
        if (tid < P_TAIL) Ps0[P_BODY + tid] = Ps1[P_BODY + tid] = -0.f;          // (published by the prologue's first barrier)
    }
    const int wv_vb = vb2 + (wv_k0 ? hr * 30 : wave == 2 ? 6 + hr * 6 : 18 + hr * 6);
    const float wv_c1 = wv_k0 ? 4.f : wave == 2 ? (hr ? 4.f : -4.f) : (hr ? 2.f : -2.f);
    const float wv_c2 = wv_k0 ? -5.f : wave == 2 ? -4.f : -1.f;
    const float wv_c3 = wv_k0 ? 1.f : wave == 2 ? (hr ? -1.f : 1.f) : (hr ? -2.f : 2.f);
    auto transform_first = [&](int pbuf, int vbuf) {           // waves 4-7: a whole row each
        if constexpr (WF4_KNOCK & 4) return;
        const float *Pb = pbuf ? Ps1 : Ps0;
        float *Vb = vbuf ? Vs1 : Vs0;
        if constexpr (HALF) {                                     // waves 1-3: rows 0 / 5, 1 / 2, 3 / 4
            if (wave == 1) wf4_transform_2rows<0, rs, psz>(Pb, Vb, pb2 + hr * rs, vb2 + hr * 30, hr);
            else if (wave == 2) wf4_transform_2rows<1, rs, psz>(Pb, Vb, pb2, vb2 + 6 + hr * 6, hr);
            else if (wave == 3) wf4_transform_2rows<2, rs, psz>(Pb, Vb, pb2, vb2 + 18 + hr * 6, hr);
        } else {
            if (wave == 4) wf4_transform_row2<0, rs, psz>(Pb, Vb, pb2, vb2);
            else if (wave == 5) wf4_transform_row2<1, rs, psz>(Pb, Vb, pb2, vb2);
            else if (wave == 6) wf4_transform_row2<2, rs, psz>(Pb, Vb, pb2, vb2);
            else if (wave == 7) wf4_transform_row2<3, rs, psz>(Pb, Vb, pb2, vb2);
        }
    };
    auto transform_last = [&](int pbuf, int vbuf) {            // waves 0-1: rows 4 and 5 (32-tile blocks)
        if constexpr (WF4_KNOCK & 4 || HALF) return;
        const float *Pb = pbuf ? Ps1 : Ps0;
        float *Vb = vbuf ? Vs1 : Vs0;
        if (wave == 0) wf4_transform_row2<4, rs, psz>(Pb, Vb, pb2, vb2);
        else if (wave == 1) wf4_transform_row2<5, rs, psz>(Pb, Vb, pb2, vb2);
    };

    // 16-tile blocks never clear the accumulators: their first K step multiplies into a literal zero (FIRST below)
    f32x4 acc[36];
    if constexpr (!HALF) {
#pragma unroll
        for (int f = 0; f < 36; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int b_off = ((wn * 4 + lk) * 16 + li) * 36;      // this lane's 36 frequencies of V[k = lk][tile 16 wn + li]
    // filter fragments: u[cout block][chunk][wm][g = 4 frequencies][lane][4] -- group g of chunk c for this wave is ONE load
    // instruction over a contiguous 1 KB; a ring of AHEAD + 1 register slots, the load for group G + AHEAD goes out when group
    // G's MFMAs do (G counts groups across K steps: 9 per step, two steps unrolled -> 18 = 3 rings of 6)
    constexpr int GA_D = WF4_GA_AHEAD, GA_SLOTS = WF4_GA_SLOTS;
    static_assert(18 % GA_SLOTS == 0, "two K steps (18 groups) must be whole turns of the ring");
    static_assert(GA_D >= 1 && GA_D < GA_SLOTS, "prefetch depth must leave one slot for the group in use");
    float4 ga[GA_SLOTS];
    const int ga_voff = lane << 4;
    auto ga_load = [&](auto slot, int c, int g) {           // (past the last chunk: the range check returns zeros, nothing uses them)
        const int soff = (int)((((unsigned)coutblk * (unsigned)p.nchunks + (unsigned)c) * 36u + (unsigned)(wm * 9 + g)) << 10);
        ga[decltype(slot)::value] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(ursrc, ga_voff, soff, 0));
    };
    // the phased K step's MFMAs: 9 groups of 4, chunk c + 2's patch requests behind the first groups
    auto mma_ga = [&](auto parity, auto first, int c, bool more2) {
        constexpr int par = decltype(parity)::value;
        constexpr bool FIRST = decltype(first)::value;
        constexpr bool NOFRAG = (WF4_KNOCK & 16) != 0, NOMMA = (WF4_KNOCK & 8) != 0;
        auto cin = [&](int f) -> f32x4 {             // FIRST: the step multiplies into a literal zero, acc is written before it is read
            if constexpr (FIRST) return (f32x4){0.f, 0.f, 0.f, 0.f};
            else return acc[f];
        };
        if constexpr (NOMMA && FIRST) {
#pragma unroll
            for (int f = 0; f < 36; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const float4 *Vp = reinterpret_cast<const float4 *>((par ? Vs1 : Vs0) + b_off);
        float4 fb[3];
        if constexpr (NOFRAG) {
            fb[0] = fb[1] = fb[2] = make_float4(1.f, 2.f, 3.f, (float)lane);
        } else {
            fb[0] = Vp[0];
            fb[1] = Vp[1];
        }
#pragma unroll
        for (int g = 0; g < 9; ++g) {
            if (!NOFRAG && g + 2 < 9) fb[(g + 2) % 3] = Vp[g + 2];
            {
                const int gn = g + GA_D;                    // the group AHEAD: same chunk or the next one
                auto issue = [&](auto sl) { ga_load(sl, gn < 9 ? c : c + 1, gn < 9 ? gn : gn - 9); };
                switch ((9 * par + g + GA_D) % GA_SLOTS) {
                case 0: issue(std::integral_constant<int, 0>{}); break;
                case 1: issue(std::integral_constant<int, 1>{}); break;
                case 2: issue(std::integral_constant<int, 2>{}); break;
                case 3: issue(std::integral_constant<int, 3>{}); break;
                case 4: issue(std::integral_constant<int, 4>{}); break;
                case 5: issue(std::integral_constant<int, 5 % GA_SLOTS>{}); break;
                case 6: issue(std::integral_constant<int, 6 % GA_SLOTS>{}); break;
                case 7: issue(std::integral_constant<int, 7 % GA_SLOTS>{}); break;
                default: issue(std::integral_constant<int, 8 % GA_SLOTS>{}); break;
                }
            }
            const float4 a = ga[(9 * par + g) % GA_SLOTS], b = fb[g % 3];
            if constexpr (NOMMA) {
                acc[4 * g + 0].x += a.x * b.x; acc[4 * g + 1].x += a.y * b.y; acc[4 * g + 2].x += a.z * b.z; acc[4 * g + 3].x += a.w * b.w;
            } else {
            acc[4 * g + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, cin(4 * g + 0), 0, 0, 0);
            acc[4 * g + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, cin(4 * g + 1), 0, 0, 0);
            acc[4 * g + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, cin(4 * g + 2), 0, 0, 0);
            acc[4 * g + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, cin(4 * g + 3), 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (g < WF4_P_PASSES) {
                if (more2) load_p_piece(c + 2, par, g);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // WEAVE: the same K step with the wave's two-row transform item of chunk c + 1 cut into pieces that ride BEHIND single MFMAs of
    // chunk c: slot s = 4 g + h follows MFMA h of group g.  A vector instruction issued by the wave that owns the matrix pipe costs
    // 3-4 cycles of matrix time, the same instruction from the sibling wave ~20 (profiles/r04_mfma_valu.txt).
    //   slots 0, 2 .. 10    patch column b = s / 2: its four 8-byte reads (P[nxt] landed a step ago)
    //   slots 5, 7 .. 15    first stage of column b = (s - 5) / 2 -- at most three columns (24 registers) are in flight
    //   slots 17 .. 22      second stage (wf4_bt2's operations in wf4_bt2's order), the V[nxt] writes behind their values
    // (measured: the item 4 or 8 slots later, or 3 / 7 slots between a column's reads and its first stage, all within +-1 %)
    // ONE branch-free instruction stream for all four waves and all steps; the item kinds differ in DATA (wv_* above).  Two other
    // forms were compiled and dropped: a stream per item kind (the register allocator copies the 144 accumulators at the joins:
    // 850 spilled registers) and scalar branches around the pieces (each piece becomes a basic block of its own and the
    // compiler sinks the patch reads into the block that uses them: read, wait, multiply -- the latency the weave is there to
    // hide).  So wave 0 repeats wave 1's item (same values to the same cells) and the last step transforms a patch nobody
    // multiplies (V[nxt] is free until the epilogue's barrier).  Every slot ends in a scheduling barrier, so the pieces stay where
    // they are put; the step's closing barrier publishes V[nxt] as before.
    auto mma_weave = [&](auto parity, auto first, int c, bool more2) {
        constexpr int par = decltype(parity)::value;
        constexpr bool FIRST = decltype(first)::value;
        constexpr bool NOFRAG = (WF4_KNOCK & 16) != 0, NOMMA = (WF4_KNOCK & 8) != 0, ITEM = (WF4_KNOCK & 4) == 0;
        auto cin = [&](int f) -> f32x4 {
            if constexpr (FIRST) return (f32x4){0.f, 0.f, 0.f, 0.f};
            else return acc[f];
        };
        if constexpr (NOMMA && FIRST) {
#pragma unroll
            for (int f = 0; f < 36; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const float4 *Vp = reinterpret_cast<const float4 *>((par ? Vs1 : Vs0) + b_off);
        const float *Pn = par ? Ps0 : Ps1;
        float *v0 = (par ? Vs0 : Vs1) + wv_vb, *v1 = v0 + 16 * 36;
        wf4_v2 d[6][4], m[6], o[6], s2, t2;
        auto item_slot = [&](int s) {
            constexpr int R0 = 0, S1 = R0 + 5, S2 = S1 + 12;
            if (!ITEM || s < R0 || s > S2 + 5) return;
            if (s < R0 + 12 && ((s - R0) & 1) == 0) {
                const int b = (s - R0) >> 1, co = (b & 3) * psz + (b >> 2) * 4;
                d[b][0] = *reinterpret_cast<const wf4_v2 *>(Pn + wv_p0 + co);
                d[b][1] = *reinterpret_cast<const wf4_v2 *>(Pn + wv_p13 + co + 2 * rs);
                d[b][2] = *reinterpret_cast<const wf4_v2 *>(Pn + wv_p2 + co);
                d[b][3] = *reinterpret_cast<const wf4_v2 *>(Pn + wv_p3 + co);
            }
            if (s >= S1 && s < S1 + 12 && ((s - S1) & 1) == 0) {
                const int b = (s - S1) >> 1;
                m[b] = wf4_fma2(wv_c1, d[b][0], wf4_fma2(wv_c2, d[b][1], wf4_fma2(wv_c3, d[b][2], d[b][3])));
            }
            if (s == S2) {
                s2 = m[4] - m[2];
                t2 = m[3] - m[1];
                o[0] = wf4_fma2(4.f, m[0], wf4_fma2(-5.f, m[2], m[4]));
            }
            if (s == S2 + 1) o[1] = wf4_fma2(-4.f, m[1] + m[2], m[3] + m[4]);
            if (s == S2 + 2) o[2] = wf4_fma2(4.f, m[1] - m[2], m[4] - m[3]);
            if (s == S2 + 3) {
                o[3] = wf4_fma2(2.f, t2, s2);
                o[4] = wf4_fma2(-2.f, t2, s2);
            }
            if (s == S2 + 4) o[5] = wf4_fma2(4.f, m[1], wf4_fma2(-5.f, m[3], m[5]));
            if (s == S2 + 2 || s == S2 + 4 || s == S2 + 5) {
                const int j = s == S2 + 2 ? 0 : s == S2 + 4 ? 2 : 4;
                v0[j] = o[j].x;
                v0[j + 1] = o[j + 1].x;
                v1[j] = o[j].y;
                v1[j + 1] = o[j + 1].y;
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        float4 fb[3];
        if constexpr (NOFRAG) {
            fb[0] = fb[1] = fb[2] = make_float4(1.f, 2.f, 3.f, (float)lane);
        } else {
            fb[0] = Vp[0];
            fb[1] = Vp[1];
        }
#pragma unroll
        for (int g = 0; g < 9; ++g) {
            if (!NOFRAG && g + 2 < 9) fb[(g + 2) % 3] = Vp[g + 2];
            {
                const int gn = g + GA_D;
                auto issue = [&](auto sl) { ga_load(sl, gn < 9 ? c : c + 1, gn < 9 ? gn : gn - 9); };
                switch ((9 * par + g + GA_D) % GA_SLOTS) {
                case 0: issue(std::integral_constant<int, 0>{}); break;
                case 1: issue(std::integral_constant<int, 1>{}); break;
                case 2: issue(std::integral_constant<int, 2>{}); break;
                case 3: issue(std::integral_constant<int, 3>{}); break;
                case 4: issue(std::integral_constant<int, 4>{}); break;
                case 5: issue(std::integral_constant<int, 5 % GA_SLOTS>{}); break;
                case 6: issue(std::integral_constant<int, 6 % GA_SLOTS>{}); break;
                case 7: issue(std::integral_constant<int, 7 % GA_SLOTS>{}); break;
                default: issue(std::integral_constant<int, 8 % GA_SLOTS>{}); break;
                }
            }
            const float4 a = ga[(9 * par + g) % GA_SLOTS], b = fb[g % 3];
            if constexpr (NOMMA) {
                acc[4 * g + 0].x += a.x * b.x; acc[4 * g + 1].x += a.y * b.y; acc[4 * g + 2].x += a.z * b.z; acc[4 * g + 3].x += a.w * b.w;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int h = 0; h < 4; ++h) item_slot(4 * g + h);
            } else {
                acc[4 * g + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, cin(4 * g + 0), 0, 0, 0);
                item_slot(4 * g + 0);
                acc[4 * g + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, cin(4 * g + 1), 0, 0, 0);
                item_slot(4 * g + 1);
                acc[4 * g + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, cin(4 * g + 2), 0, 0, 0);
                item_slot(4 * g + 2);
                acc[4 * g + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, cin(4 * g + 3), 0, 0, 0);
                item_slot(4 * g + 3);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (g < WF4_P_PASSES) {
                if (more2) load_p_piece(c + 2, par, g);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // ---- prologue: chunk 0's patch in LDS and transformed, its first filter fragments and chunk 1's patch requested ----
    WF4_MARK(0);
    load_p(0, 0);
    {
        auto first = [&](auto sl) { ga_load(sl, 0, decltype(sl)::value); };      // groups 0 .. AHEAD - 1 of chunk 0
        first(std::integral_constant<int, 0>{});
        if (GA_D > 1) first(std::integral_constant<int, 1>{});
        if (GA_D > 2) first(std::integral_constant<int, 2>{});
        if (GA_D > 3) first(std::integral_constant<int, 3>{});
        if (GA_D > 4) first(std::integral_constant<int, 4>{});
        if (GA_D > 5) first(std::integral_constant<int, 5 % GA_SLOTS>{});
        if (GA_D > 6) first(std::integral_constant<int, 6 % GA_SLOTS>{});
        if (GA_D > 7) first(std::integral_constant<int, 7 % GA_SLOTS>{});
    }
    __syncthreads();
    WF4_MARK(1);
    if (p.nchunks > 1) load_p(1, 1);
    transform_first(0, 0);
    transform_last(0, 0);
    __syncthreads();
    WF4_MARK(2);
    // (cache policy of the LDS-DMA requests, measured: non-temporal patch / filter / both 41.6 / 41.3 / 42.5 us against 39.0 us for
    //  the default policy -- neighbouring workgroups share halo pixels and every workgroup the filter -- sc0 39.2 us)
    // one K step; the buffer parity is a compile-time constant, so the compiler can tell the LDS-DMA destination (P[cur]) from
    // what the step reads and writes (V[cur], P[nxt], V[nxt]) and lets the DMA fly
    // FIRST (16-tile blocks; a compile-time copy of the step): the block's first step multiplies into a literal zero instead of
    // cleared accumulators -- fma(a, b, +0) either way.
    auto kstep = [&](auto parity, int c, auto first) {
        constexpr int cur = decltype(parity)::value, nxt = cur ^ 1;
        const bool more = c + 1 < p.nchunks, more2 = c + 2 < p.nchunks;
        // P[cur] was last read by the transform of chunk c: free for the whole step.  Phased: waves 4-7 (16 tiles: 1-3) transform
        // BEFORE they request their share of the next patch (the patch they read landed a step ago; an LDS-DMA instruction holds
        // a wave's issue slot ~100 cycles and would delay the transform their MFMAs wait for): 38.2 -> 37.6 us
        WF4_STEP_MARK(c, 0);
        if (!WEAVE && more) transform_first(nxt, nxt);
        WF4_STEP_MARK(c, 1);
        if constexpr (WEAVE) {
            mma_weave(parity, first, c, more2);           // every wave carries its item of chunk c + 1 inside its own MFMA stream
        } else {
            mma_ga(parity, first, c, more2);
        }
        WF4_STEP_MARK(c, 2);
        if (more) transform_last(nxt, nxt);
        WF4_STEP_MARK(c, 3);
        __syncthreads();
        WF4_STEP_MARK(c, 4);
    };
    // 32-tile blocks: static priority for the waves that multiply first (0-3; their SIMD partners 4-7 open every step with the
    // patch transform): 39.2 -> 38.5-38.8 us per layer1 conv; the other half at priority 1 instead: 41.3 us
    if (!HALF && wave < 4) __builtin_amdgcn_s_setprio(1);
    {
        constexpr std::integral_constant<int, 0> even{};
        constexpr std::integral_constant<int, 1> odd{};
        constexpr std::false_type no{};
        constexpr std::true_type yes{};
        if constexpr (HALF) {
            // step c keeps parity c & 1 (the filter ring's slots and the buffers are the unpeeled loop's): step 0 on its own, then
            // pairs (odd, even).  (The last step peeled as well, without its item: the register allocator copies the accumulators
            // at the joins, 240-510 spilled registers in either loop form tried -- profiles/wf4_head_tail.md.)
            kstep(even, 0, yes);
            for (int c = 1; c < p.nchunks; c += 2) {
                kstep(odd, c, no);
                if (c + 1 < p.nchunks) kstep(even, c + 1, no);
            }
        } else {
            for (int c = 0; c < p.nchunks; c += 2) {
                kstep(even, c, no);
                if (c + 1 < p.nchunks) kstep(odd, c + 1, no);
            }
        }
    }

    // ---- lane-local output transform; fused tail and stores through the wave's exchange buffer ----
    WF4_MARK(3);
    const int coq = (int)coutblk * 16 + wm * 4 + lk;
    const int cqc = min(coq, p.Coq - 1);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.ep.res), 0, p.ep.res ? p.y_bytes : 0u, 0x00020000);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f), one4 = make_float4(1.f, 1.f, 1.f, 1.f);
    const bool plain = !p.ep.bias && p.ep.scale && p.ep.shift && p.ep.act == 1 && !(p.ep.res && p.ep.res_post);
    float4 scale, shift;                       // the straight-line tail's parameters, held in registers
    if constexpr (HALF) {
        // one range-checked 16-byte load each, no branch: only the straight-line tail reads them, and elsewhere the empty range
        // gives zeros without touching memory
        const unsigned par_bytes = plain ? (unsigned)p.Coq * 16u : 0u;
        const __amdgpu_buffer_rsrc_t scrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.ep.scale), 0, par_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t shrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.ep.shift), 0, par_bytes, 0x00020000);
        scale = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(scrsrc, cqc << 4, 0, 0));
        shift = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(shrsrc, cqc << 4, 0, 0));
    } else {
        scale = plain ? reinterpret_cast<const float4 *>(p.ep.scale)[cqc] : one4;
        shift = plain ? reinterpret_cast<const float4 *>(p.ep.shift)[cqc] : z4;
    }
    // the K loop is over: V (and, for 16-tile blocks, P) is free -- 4.25 KB of exchange buffer per wave
    float4 *xb = HALF ? reinterpret_cast<float4 *>(wave == 0 ? Vs0 : wave == 1 ? Vs1 : wave == 2 ? Ps0 : Ps1)
                      : reinterpret_cast<float4 *>(wave < 4 ? Vs0 : Vs1) + (wave & 3) * (4 * 68);
    const int te = lane >> 2, be = lane & 3;
    const int oj2 = wn * 16 + te;
    int n2 = n0 + (oj2 >> lT), ty2 = ty0 + ((oj2 >> LBC) & BRm), tx2 = tx0 + (oj2 & BCm);
    if constexpr (PACK) {
        if ((oj2 & BCm) >= p.tw) {                               // a spare slot: the donor image's tile
            n2 = dn;
            ty2 = (dgr << p.lBR) + ((oj2 >> LBC) & BRm);
            tx2 = p.pack_sc * dgc + (oj2 & BCm) - p.tw;
        }
    }
    const int x2 = tx2 * 4 + be, cq0 = (int)coutblk * 16 + wm * 4;
    const bool ok2 = n2 < p.N && ty2 < p.th && tx2 < p.tw && x2 < p.W;
    // 16-tile blocks: the first stage of A^T m A once, and row 0's four store offsets once -- row A adds A row pitches and selects
    // the out-of-range offset where the row is off the map (an out-of-range offset stays one with three pitches added: the
    // tensor is below 2 GB), no branch inside the rows
    int off0[4] = {OOB, OOB, OOB, OOB};
    if constexpr (HALF) {
        wf4_column_sums(acc);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (ok2 && cq0 + q < p.Coq)
                off0[q] = (int)((((unsigned)(n2 * p.Coq + cq0 + q) * (unsigned)p.H + (unsigned)(ty2 * 4)) * (unsigned)p.W + (unsigned)x2) << 4);
    }
    auto row = [&](auto first, auto res, auto pl) {
        constexpr int A = decltype(first)::value;
        const int yy = ty2 * 4 + A;
        int off[4];
        if constexpr (HALF) {
            const bool in = yy < p.H;
#pragma unroll
            for (int q = 0; q < 4; ++q) off[q] = in ? (int)((unsigned)off0[q] + (unsigned)(A * p.W) * 16u) : OOB;
            wf4_output_row_summed<A, decltype(res)::value, decltype(pl)::value>(p, acc, cqc, scale, shift, xb, lk * 16 + li,
                                                                               be * 68 + te, yrsrc, rrsrc, off);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                off[q] = (ok2 && yy < p.H && cq0 + q < p.Coq)
                             ? (int)((((unsigned)(n2 * p.Coq + cq0 + q) * (unsigned)p.H + (unsigned)yy) * (unsigned)p.W + (unsigned)x2) << 4) : OOB;
            wf4_output_row_coalesced<A, decltype(res)::value, decltype(pl)::value>(p, acc, cqc, scale, shift, xb, lk * 16 + li,
                                                                                  be * 68 + te, yrsrc, rrsrc, off);
        }
    };
    auto rows = [&](auto res, auto pl) {
        row(std::integral_constant<int, 0>{}, res, pl);
        row(std::integral_constant<int, 1>{}, res, pl);
        row(std::integral_constant<int, 2>{}, res, pl);
        row(std::integral_constant<int, 3>{}, res, pl);
    };
    // the tail is the same for the whole launch: scalar branches pick the straight-line form where it applies and whether a
    // residual is fetched
    if (plain) {
        if (p.ep.res) rows(std::true_type{}, std::true_type{});
        else rows(std::false_type{}, std::true_type{});
    } else {
        if (p.ep.res) rows(std::true_type{}, std::false_type{});
        else rows(std::false_type{}, std::false_type{});
    }
    WF4_MARK(4);
#ifdef WF4_STAMP
    __builtin_amdgcn_s_waitcnt(0);             // (probe: when have this wave's stores left?)
    WF4_MARK(5);
#endif
}

template <int LBC, bool PACK = false, bool HALF = false, bool WEAVE = false>
__global__ void __launch_bounds__(HALF ? 256 : 512) __attribute__((amdgpu_waves_per_eu(2, 2))) conv_wf4_kernel(const Wf4Args p) {
    conv_wf4_body<LBC, PACK, HALF, WEAVE>(p);
}

// filter: OIHW 3x3 -> u[cout block][chunk][wm][g][lane = 16 kk + i][f & 3] = (G g G^T)[f = 4 g + (f & 3)] of channel
// (64 blk + 16 wm + i, 4 chunk + kk); zero beyond Cout
__global__ void __launch_bounds__(256) wf4_filter_kernel(const float *w, float *u, unsigned total, int Cin, int Cout) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;   // (co, c) pair
    if (i >= total) return;
    const int co = (int)(i / (unsigned)Cin), c = (int)(i - (unsigned)co * Cin);
    const float *g = w + (size_t)i * 9;
    float t[6][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float g0 = g[j], g1 = g[3 + j], g2 = g[6 + j];
        t[0][j] = g0 * 0.25f;
        t[1][j] = -(g0 + g1 + g2) * (1.f / 6.f);
        t[2][j] = (-g0 + g1 - g2) * (1.f / 6.f);
        t[3][j] = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
        t[4][j] = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
        t[5][j] = g2;
    }
    const int nchunks = Cin / 4;
    float f[36];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const float g0 = t[a][0], g1 = t[a][1], g2 = t[a][2];
        f[a * 6 + 0] = g0 * 0.25f;
        f[a * 6 + 1] = -(g0 + g1 + g2) * (1.f / 6.f);
        f[a * 6 + 2] = (-g0 + g1 - g2) * (1.f / 6.f);
        f[a * 6 + 3] = g0 * (1.f / 24.f) + g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
        f[a * 6 + 4] = g0 * (1.f / 24.f) - g1 * (1.f / 12.f) + g2 * (1.f / 6.f);
        f[a * 6 + 5] = g2;
    }
    float *blk = u + ((size_t)(co >> 6) * nchunks + (c >> 2)) * WF4_A_FLOATS;
    // [wm = 16-channel block][g = 4 frequencies][lane = k * 16 + channel][4]: what one wave loads for one MFMA group is contiguous
    float *up = blk + (((co >> 4) & 3) * 9 * 64 + (c & 3) * 16 + (co & 15)) * 4;
#pragma unroll
    for (int q = 0; q < 36; ++q) up[(q >> 2) * 256 + (q & 3)] = f[q];
}
