// Stem convolution + max-pool as a polyphase 1-D Winograd F(4,4) along W -- a second form of conv_stem_pool_kernel<7, true>
// (conv_stem_pool_kernel.h, included in front of this file: StemPoolArgs, the strips, the NCHW rows by LDS-DMA, the zero / -1e4
// pool semantics, max_nan, the fused tail and the ring of horizontally pooled rows are the same).  What changes is the
// arithmetic of a conv row: with stride 2, conv column j reads padded columns 2 j + v, so the taps v = 0, 2, 4, 6 are a 4-tap
// stride-1 correlation over the even columns of the row and v = 1, 3, 5 (+ one zero tap) one over its odd columns.  Both go
// through F(4,4) on the nodes 0, 1, -1, 2, -2, 1/2, inf: 7 frequencies per tile of 4 conv columns, products summed in the
// frequency domain over k = (filter row, channel, phase) -- K = 7 x 3 x 2 = 42, padded to 11 k-quads -- and ONE output
// transform.  Per 16 output channels and conv-row pair that is 4 tile blocks x 7 frequencies x 11 = 308 MFMAs
// (v_mfma_f32_16x16x4_f32) where the direct form issues 2 x 7 x 37 = 518.
//
// V, the transformed input, is a RING OF K-QUADS: V[f][ring quad][tile slot][4].  With a the input row counted from the strip's
// first (2 c0 - 3 in the image) and rho = 3 a + c a staged (input row, channel) row, k = 2 rho + phase = 6 a + 2 c + phase is
// absolute over the strip, and quad Q = k / 4 sits at ring position Q mod 20.  Step t (conv rows 2 t, 2 t + 1 of the strip, one
// pooled row) reads input rows a = 4 t .. 4 t + 8 = quads 6 t .. 6 t + 13; its conv row r multiplies k = 24 t + 12 r .. + 43, which
// starts on a quad, so filter quad j (0 .. 10) meets ring position (6 t + 3 r + j) mod 20 and the filter in registers is the same
// in every step: nothing rotates.  A step adds 4 input rows = 12 staged rows = 6 quads (6 t + 13, upper half, .. 6 t + 19, lower
// half); 14 + 6 = 20, so the quads step t + 1 adds are not among those step t reads.
//
// A step of the persistent workgroup (8 waves; wave (mb, r) = 16 output channels x conv row r of the pair):
//   1. top barrier: V of step t is whole and the 12 staged rows that step t + 1 adds have landed in X by LDS-DMA;
//   2. the MFMAs run in two halves of one tile block (16 tiles) x 7 frequencies = 28 accumulator registers each.  A B fragment
//      is one ds_read_b128: lane (tile li, quarter kk) reads quad 4 u + kk of its tile, 4 MFMAs; with 128 tile slots' worth of
//      bytes between quads the two lane quarters of a b128 group cover the 16 slots of a bank row (conflict-free, wherever the
//      quad sits in the ring).  The last 3 quads are one MFMA each (ds_read_b32, element kk).  k = 42, 43 of a conv row lie under
//      zero filter values, but in the ring they are another row's values -- stale, or being written -- so every wave multiplies
//      zeros there (`cut`), or an inf of a row the conv row never reads would come out as inf x 0.  The FILTER never enters LDS: a
//      lane's 77 A values (7 f x 11 quads, one channel) are loaded once per workgroup and stay in registers.  Frequencies run
//      4 (then 3) abreast, so two MFMAs on one accumulator are 3-4 issues apart;
//   3. TRANSFORM of step t + 1, LDS -> LDS, riding in half 0's MFMAs: item (staged row, tile) = thread tid < 12 x 28 = 336 reads
//      floats 8 tile .. + 15 of its row (4 x ds_read_b128, behind MFMA group 3), applies B^T to the even and to the odd phase and
//      writes the 7 x 2 values at k = 2 rho + phase (7 x ds_write_b64, behind group 4).  The 5 input rows a step shares with the
//      one before are not transformed again.  Behind the mid-step barrier X is empty and the rows of step t + 2 are requested.
//      Step 0 alone transforms its 9 input rows (27 staged rows, 756 items) in a phase of its own, staged in the pooled-row ring,
//      which is idle until then;
//   4. the output transform A^T is lane-local (7 accumulators -> 4 conv pixels x 4 channels), then the fused tail, the
//      horizontal 3-max -- pooled column 2 t takes pixel 4 t - 1 from the neighbouring lane (DPP), 2 t + 1 is lane-local -- and
//      two 16-byte cells per lane into the ring of pooled rows.  It rides in the other half's MFMAs: half 0 carries the tail of
//      the previous step's half 1, the hand-over barrier and the pooled row, half 1 the tail of this step's half 0.
// LDS (of 160 KB): V 7 f x 20 quads x 32 slots x 16 B = 70.0 KB, X 12.0 KB, the ring of pooled rows 4 x 16 x 56 x 16 B = 56.0 KB:
// 138 KB.  With the filter in LDS (77 KB per 64 channels) V could not stay whole; 32-channel workgroups would repeat the transform
// and the input traffic.  Registers: 77 filter + 2 x 28 accumulators + 2 x 16 fragments + 16 of the transform item.
// Width: one chunk of up to 112 conv columns = 28 tiles in 32 slots (slots 28 .. 31 hold zeros); wider maps are cut into chunks as
// in the direct form.  Non-finite inputs spread over their tile (and, within it, over the conv rows that read the input row).
constexpr int SW_F = 7, SW_KQ = 11, SW_K = 42;      // frequencies, filter k-quads, real k values
constexpr int SW_VQ = 20, SW_TS = 32;               // ring quads of V (a step reads 14: 9 rows x 3 channels x 2 phases = 54 -> 56, the next adds 6), tile slots
constexpr int SW_TILES = 28;                        // tiles per chunk
constexpr int SW_XROWS0 = 27, SW_XROWS = 12;        // staged (input row, channel) rows: the 9 input rows of step 0, the 4 new ones of a step
constexpr int SW_XROW = 244;                        // floats per staged row: 4 left + 2 per conv column + the last tile's reach, 61 cells
constexpr int sw_x_floats(int rows) { return (rows * (SW_XROW / 4) + 63) / 64 * 256; }
constexpr int SW_FQ = SW_VQ * SW_TS * 4;            // floats of V per frequency
constexpr int SW_PC = 56, SW_HP_CELLS = 16 * SW_PC;
// G of F(4,4) on the nodes 0, 1, -1, 2, -2, 1/2, inf (row f, tap a)
__device__ const float sw_G[SW_F * 4] = {
    -1.f / 2, 0.f, 0.f, 0.f,
    -1.f / 3, -1.f / 3, -1.f / 3, -1.f / 3,
    1.f / 9, -1.f / 9, 1.f / 9, -1.f / 9,
    1.f / 36, 1.f / 18, 1.f / 9, 2.f / 9,
    -1.f / 60, 1.f / 30, -1.f / 15, 2.f / 15,
    32.f / 45, 16.f / 45, 8.f / 45, 4.f / 45,
    0.f, 0.f, 0.f, 1.f};
// k order: k = 6 fr + 2 c + phase; tap a of it is filter column kw = 2 a + phase (phase 1, a = 3: the zero tap).
// -> index into the OIHW filter of one output channel, or -1
__host__ __device__ constexpr int sw_k_tap(int k, int a) {
    const int fr = k / 6, c = (k % 6) / 2, kw = 2 * a + (k & 1);
    return (k < SW_K && kw < 7) ? (c * SP_KH + fr) * 7 + kw : -1;
}

// B^T d of F(4,4) on these nodes
__device__ __forceinline__ void sw_bt(const float d0, const float d1, const float d2, const float d3, const float d4, const float d5,
                                      const float d6, float (&o)[SW_F]) {
    o[0] = fmaf(-2.f, d0, fmaf(4.f, d1, fmaf(2.5f, d2, fmaf(-5.f, d3, fmaf(-0.5f, d4, d5)))));
    o[1] = fmaf(2.f, d1 - d2, fmaf(-4.5f, d3, fmaf(0.5f, d4, d5)));
    o[2] = fmaf(-2.f, d1, fmaf(6.f, d2, fmaf(-3.5f, d3, fmaf(-1.5f, d4, d5))));
    o[3] = fmaf(1.5f, d4 - d2, fmaf(-2.f, d3, d1 + d5));
    o[4] = fmaf(2.5f, d2 - d4, d5 - d1);
    o[5] = fmaf(4.f, d1, fmaf(-5.f, d3, d5));
    o[6] = fmaf(-2.f, d1, fmaf(4.f, d2, fmaf(2.5f, d3, fmaf(-5.f, d4, fmaf(-0.5f, d5, d6)))));
}

__global__ void __launch_bounds__(512) conv_stem_wino_kernel(const StemPoolArgs p) {
    __shared__ __attribute__((aligned(16))) float V[SW_F * SW_FQ];
    __shared__ __attribute__((aligned(16))) float X[sw_x_floats(SW_XROWS)];
    __shared__ __attribute__((aligned(16))) float4 HP[4 * SW_HP_CELLS];
    static_assert(sw_x_floats(SW_XROWS0) <= 16 * SW_HP_CELLS, "the rows of step 0 are staged in the pooled-row ring");
    float *X0 = reinterpret_cast<float *>(HP);              // step 0 only: nothing enters the ring before its transform is done
    typedef __attribute__((address_space(3))) float lds_float;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mb = wave & 3, rsel = wave >> 2;              // 16-channel block, conv row of the pair
    const int li = lane & 15, kk = lane >> 4;

    unsigned t1, t2, cob, n, strip, chunk;
    cob = blockIdx.x % (unsigned)p.cout_blocks;
    t1 = blockIdx.x / (unsigned)p.cout_blocks;
    chunk = t1 % (unsigned)p.chunks;
    t2 = t1 / (unsigned)p.chunks;
    n = t2 / (unsigned)p.strips;
    strip = t2 - n * (unsigned)p.strips;
    const int q0 = (int)chunk * p.pq;                       // first pooled column this workgroup stores
    const int x0 = chunk ? 2 * q0 - 2 : 0;                  // its first conv column; local pooled column l is global x0 / 2 + l
    const int lskip = chunk ? 1 : 0, qend = min(q0 + p.pq, p.Wq);
    const int p0 = (int)strip * p.prows;                    // first pooled row of the strip
    const int c0 = 2 * p0 - 1;                              // first conv row: the one above the first window's centre
    const int co0 = (int)cob * 64;

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.xp), 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq), 0, p.w_bytes, 0x00020000);
    constexpr int OOB = (int)0x80000000;

    // ---- the filter: [7 f][11 quads][Cout][4]; this lane's channel, quads 4 u + kk whole (u = 0, 1), element kk of quads 8 .. 10 ----
    float4 fw4[SW_F][2];
    float fwt[SW_F][3];
    {
        const int co = co0 + mb * 16 + li;
#pragma unroll
        for (int f = 0; f < SW_F; ++f) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int off = co < p.Cout ? (int)(((unsigned)(f * SW_KQ + 4 * u + kk) * (unsigned)p.Cout + (unsigned)co) << 4) : OOB;
                fw4[f][u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 0));
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int off = co < p.Cout ? (int)((((unsigned)(f * SW_KQ + 8 + j) * (unsigned)p.Cout + (unsigned)co) << 4) + 4u * (unsigned)kk) : OOB;
                fwt[f][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wrsrc, off, 0, 0));
            }
        }
    }
    // V starts as zeros: the tile slots 28 .. 31 are never written
    for (int i = tid; i < SW_F * SW_FQ / 4; i += 512) reinterpret_cast<float4 *>(V)[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- staged rows: ROWS (input row, channel) rows of 61 cells from absolute row rho0 = 3 a + c on (a: input row of the strip,
    // 2 c0 - 3 + a in the image; step t reads a = 4 t .. 4 t + 8); cell j = input columns 2 x0 - 4 + 4 j .. + 3
    auto load_rows = [&](auto rows, float *buf, int rho0) {
        constexpr int CPR = SW_XROW / 4, CELLS = decltype(rows)::value * CPR;
        for (int pc = wave; pc * 64 < CELLS; pc += 8) {
            const int idx = pc * 64 + lane;
            const int rr = idx / CPR, j = idx - rr * CPR;
            const int a = (rho0 + rr) / 3, c = rho0 + rr - 3 * a;
            const int h = 2 * c0 - 3 + a, xin = 2 * x0 - 4 + 4 * j;
            const bool ok = idx < CELLS && (unsigned)h < (unsigned)p.H && xin >= 0 && xin + 3 < p.W;
            const int off = ok ? (int)(((((unsigned)n * 3u + (unsigned)c) * (unsigned)p.H + (unsigned)h) * (unsigned)p.W + (unsigned)xin) << 2) : OOB;
            if (idx < CELLS) __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_float *)(buf + pc * 256), 16, off, 0, 0, 0);
        }
    };
    // the rows step t adds to the 5 it shares with step t - 1: a = 4 t + 5 .. 4 t + 8
    auto load_step = [&](int t) { load_rows(std::integral_constant<int, SW_XROWS>{}, X, 12 * t + 15); };
    load_rows(std::integral_constant<int, SW_XROWS0>{}, X0, 0);

    // ---- staged rows -> V: conv column 4 t + jj, tap v sits at float 8 t + 2 jj + v + 1 of its row: the even phase is the odd
    // floats.  Row rho is k = 2 rho, 2 rho + 1: half of quad rho / 2, at ring position (rho / 2) mod SW_VQ.  An item is staged row
    // rr of the buffer (absolute row rho0 + rr) x tile tt, in two parts: 4 x ds_read_b128, then B^T and 7 x ds_write_b64 ----
    auto item_load = [&](const float *buf, int it, float4 (&s)[4]) {
        const int rr = it / SW_TILES, tt = it - rr * SW_TILES;
        const float4 *src = reinterpret_cast<const float4 *>(buf + rr * SW_XROW + 8 * tt);
        s[0] = src[0]; s[1] = src[1]; s[2] = src[2]; s[3] = src[3];
    };
    auto item_store = [&](int rho0, int it, const float4 (&s)[4]) {
        const int rr = it / SW_TILES, tt = it - rr * SW_TILES, rho = rho0 + rr;
        const float4 a = s[0], b = s[1], c = s[2], d = s[3];
        float ev[SW_F], od[SW_F];
        sw_bt(a.y, a.w, b.y, b.w, c.y, c.w, d.y, ev);
        sw_bt(a.z, b.x, b.z, c.x, c.z, d.x, d.z, od);
        const int q = (rho0 >> 1) % SW_VQ + (((rho0 & 1) + rr) >> 1);                // (rho / 2) mod SW_VQ: the first term is wave-uniform
        float *dst = V + ((q >= SW_VQ ? q - SW_VQ : q) * SW_TS + tt) * 4 + 2 * (rho & 1);
#pragma unroll
        for (int f = 0; f < SW_F; ++f) *reinterpret_cast<float2 *>(dst + f * SW_FQ) = make_float2(ev[f], od[f]);
    };

    // tail parameters of this lane's channel quad (a lane of the 16x16 C layout holds rows 4 (lane / 16) .. + 3 of its column)
    const int cq = (int)cob * 16 + mb * 4 + kk;
    const int cqc = min(cq, p.Coq - 1);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f), one4 = make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 bias = p.ep.bias ? reinterpret_cast<const float4 *>(p.ep.bias)[cqc] : z4;
    const float4 scale = p.ep.scale ? reinterpret_cast<const float4 *>(p.ep.scale)[cqc] : one4;
    const float4 shift = p.ep.shift ? reinterpret_cast<const float4 *>(p.ep.shift)[cqc] : z4;
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(p.y, 0, p.y_bytes, 0x00020000);
    const bool plain = !p.ep.bias && p.ep.scale && p.ep.shift && p.ep.act == 1;

    sp_f32x4 accA[SW_F], accB[SW_F];                            // tile block 0 / 1 of the wave's conv row
    float4 vprev = z4;                                           // last pixel of tile block 0 after the tail (its lane 15 is a neighbour)
    const float4 lo4 = make_float4(-1e4f, -1e4f, -1e4f, -1e4f);

    // tile block tb of conv row k (of the strip): A^T, fused tail, horizontal 3-max, two pooled columns per tile -> the ring
    auto tail_block = [&](const sp_f32x4 (&acc)[SW_F], int tb, int k) {
        const bool row_in = (unsigned)(c0 + k) < (unsigned)p.Ho;         // rows outside the map are the pool's zero padding
        const int tile = 16 * tb + li, col0 = x0 + 4 * tile;
        float px[4][4];                                                   // [pixel of the tile][channel of the quad]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float s12 = acc[1][e] + acc[2][e], d12 = acc[1][e] - acc[2][e];
            const float s34 = acc[3][e] + acc[4][e], d34 = acc[3][e] - acc[4][e];
            const float h = acc[5][e];
            px[0][e] = ((acc[0][e] + s12) + s34) + h;
            px[1][e] = fmaf(0.5f, h, fmaf(2.f, d34, d12));
            px[2][e] = fmaf(0.25f, h, fmaf(4.f, s34, s12));
            px[3][e] = fmaf(0.125f, h, fmaf(8.f, d34, d12)) + acc[6][e];
        }
        float4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (plain) {
                // scale, shift, ReLU without bias, as in the direct form: separate roundings, the ReLU behind the pooling
                typedef float sp_v2 __attribute__((ext_vector_type(2)));
                const sp_v2 lo = (sp_v2){px[i][0], px[i][1]} * (sp_v2){scale.x, scale.y} + (sp_v2){shift.x, shift.y};
                const sp_v2 hi = (sp_v2){px[i][2], px[i][3]} * (sp_v2){scale.z, scale.w} + (sp_v2){shift.z, shift.w};
                v[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
            } else {
                v[i] = apply_epilogue4(p.ep, bias, scale, shift, z4, 4, make_float4(px[i][0], px[i][1], px[i][2], px[i][3]));
            }
            if (!row_in || col0 + i >= p.Wo) v[i] = z4;                   // (columns past the map's edge: zero padding too)
        }
        // pooled column 2 t: pixels 4 t - 1 (pixel 3 of lane li - 1 by row_shr:1, whose lane 0 keeps `old` = lane 15 of tile block 0
        // or the zero padding), 4 t, 4 t + 1; pooled column 2 t + 1: pixels 4 t + 1, 4 t + 2, 4 t + 3
        float4 m0, m1;
        float *mo0 = reinterpret_cast<float *>(&m0), *mo1 = reinterpret_cast<float *>(&m1);
        const float *pv = reinterpret_cast<const float *>(&vprev);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v0 = reinterpret_cast<const float *>(&v[0])[e], v1 = reinterpret_cast<const float *>(&v[1])[e];
            const float v2 = reinterpret_cast<const float *>(&v[2])[e], v3 = reinterpret_cast<const float *>(&v[3])[e];
            const int prev15 = tb > 0 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, pv[e]), 0x121, 0xf, 0xf, false) : 0;   // row_ror:1
            const float left = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(prev15, __builtin_bit_cast(int, v3), 0x111, 0xf, 0xf, false));   // row_shr:1
            mo0[e] = max_nan(max_nan(left, v0), v1);
            mo1[e] = max_nan(max_nan(v1, v2), v3);
        }
        vprev = v[3];
        if (tile < SW_TILES) {
            float4 *hp = HP + (k & 3) * SW_HP_CELLS + (mb * 4 + kk) * SW_PC + 2 * tile;
            hp[0] = m0;
            hp[1] = m1;
        }
    };
    // half of pooled row j (cells i = tid + 512 * half): rows 2 j, 2 j + 1, 2 j + 2 of the ring, running maximum from -1e4
    auto pool_half = [&](int j, int half) {
        const int prow = p0 + j, i = tid + 512 * half;
        if (i < SW_HP_CELLS && prow < p.Hq) {
            const float4 *r0 = HP + ((2 * j) & 3) * SW_HP_CELLS, *r1 = HP + ((2 * j + 1) & 3) * SW_HP_CELLS,
                         *r2 = HP + ((2 * j + 2) & 3) * SW_HP_CELLS;
            const int c = i / SW_PC, ql = i - c * SW_PC, q = (x0 >> 1) + ql;
            float4 m = sp_max4(sp_max4(sp_max4(lo4, r0[i]), r1[i]), r2[i]);
            if (plain) m = make_float4(relu_ref(m.x), relu_ref(m.y), relu_ref(m.z), relu_ref(m.w));
            const int cqo = (int)cob * 16 + c;
            const int off = (cqo < p.Coq && ql >= lskip && q < qend)
                                ? (int)(((((unsigned)n * (unsigned)p.Coq + (unsigned)cqo) * (unsigned)p.Hq + (unsigned)prow) * (unsigned)p.Wq + (unsigned)q) << 4)
                                : OOB;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned, m), yrsrc, off, 0, 0);
        }
    };
    auto lds_barrier = [&]() {          // orders LDS traffic only: __syncthreads() also waits for the wave's global stores (vmcnt)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    };

    // the MFMAs of one tile block: 6 groups G = 3 b + g -- frequencies 4 b .. (4 abreast, then 3), g = 0, 1: quads 4 g + kk
    // (4 MFMAs per frequency), g = 2: quads 8 .. 10 (3).  Fragments one group ahead in two register sets; ride(G) is what
    // rides along behind group G.
    auto mma_half = [&](auto tbc, int t, sp_f32x4 (&acc)[SW_F], auto &&ride) {
        constexpr int tb = decltype(tbc)::value;
        // filter quad j of the wave's conv row is absolute quad 6 t + 3 rsel + j: ring position (qb + j) mod SW_VQ
        const int qb = (6 * t + 3 * rsel) % SW_VQ;
        auto at = [&](int j) { return V + ((qb + j >= SW_VQ ? qb + j - SW_VQ : qb + j) * SW_TS + 16 * tb + li) * 4; };
        const float *vb[2] = {at(kk), at(4 + kk)};                                   // + f SW_FQ
        // k = 42, 43 of the last quad lie under zero filter values, but in the ring they are another row's values -- the other
        // conv row's, stale ones, or those the riding transform is writing: multiply zeros, and do not even read them (the lanes
        // kk >= 2 load k = 40, 41 again, which nothing writes during the step, and drop them)
        const bool cut = kk >= 2;
        const float *vt[3] = {at(8) + kk, at(9) + kk, at(10) + (kk & 1)};            // + f SW_FQ
#pragma unroll
        for (int f = 0; f < SW_F; ++f) acc[f] = (sp_f32x4){0.f, 0.f, 0.f, 0.f};
        float4 fb[2][4];
        auto fetch = [&](int G, int set) {
            const int b = G / 3, g = G - 3 * b;
#pragma unroll
            for (int fi = 0; fi < 4; ++fi) {
                const int f = 4 * b + fi;
                if (f >= SW_F) continue;
                if (g < 2) {
                    fb[set][fi] = *reinterpret_cast<const float4 *>(vb[g] + f * SW_FQ);
                } else {
                    fb[set][fi].x = vt[0][f * SW_FQ];
                    fb[set][fi].y = vt[1][f * SW_FQ];
                    const float last = vt[2][f * SW_FQ];
                    fb[set][fi].z = cut ? 0.f : last;
                }
            }
        };
        fetch(0, 0);
#pragma unroll
        for (int G = 0; G < 6; ++G) {
            const int set = G & 1, b = G / 3, g = G - 3 * b;
            if (G + 1 < 6) fetch(G + 1, set ^ 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (g == 2 && j == 3) continue;
#pragma unroll
                for (int fi = 0; fi < 4; ++fi) {
                    const int f = 4 * b + fi;
                    if (f >= SW_F) continue;
                    const float av = g < 2 ? reinterpret_cast<const float *>(&fw4[f][g])[j] : fwt[f][j];
                    const float bv = reinterpret_cast<const float *>(&fb[set][fi])[j];
                    acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[f], 0, 0, 0);
                }
            }
            ride(G);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // step 0: all 9 input rows, a phase of its own
    if (p.steps > 1) load_step(1);
    __syncthreads();                                     // the rows of steps 0 and 1 have landed (vmcnt)
    {
        float4 s[4];
        for (int it = tid; it < SW_XROWS0 * SW_TILES; it += 512) {
            item_load(X0, it, s);
            item_store(0, it, s);
        }
    }
    float4 xs[4];                                        // thread tid < 336 transforms item tid of step t + 1 while step t multiplies
    for (int t = 0; t < p.steps; ++t) {
        __syncthreads();                                 // V of step t is whole; the rows of step t + 1 have landed (vmcnt)
        const bool more = t + 1 < p.steps && tid < SW_XROWS * SW_TILES;
        // half 0 carries the tail of the previous step's half 1, the barrier that completes ring rows 2 t - 2, 2 t - 1, the pooled
        // row, and the transform of step t + 1: its 6 ring quads are not among the 14 this step reads
        mma_half(std::integral_constant<int, 0>{}, t, accA, [&](int G) {
            if (t >= 1) {
                if (G == 0) tail_block(accB, 1, 2 * (t - 1) + rsel);
                if (G == 1) lds_barrier();
                if (t >= 2 && (G == 2 || G == 3)) pool_half(t - 2, G - 2);
            }
            if (G == 3 && more) item_load(X, tid, xs);
            if (G == 4 && more) item_store(12 * t + 27, tid, xs);
        });
        lds_barrier();                                   // the pooled row has been read: its ring rows take rows 2 t, 2 t + 1; X is free
        if (t + 2 < p.steps) load_step(t + 2);
        mma_half(std::integral_constant<int, 1>{}, t, accB, [&](int G) {
            if (G == 0) tail_block(accA, 0, 2 * t + rsel);
        });
    }
    // drain: half 1 of the last step, last pooled row
    tail_block(accB, 1, 2 * (p.steps - 1) + rsel);
    lds_barrier();
    pool_half(p.prows - 1, 0);
    pool_half(p.prows - 1, 1);
}

// OIHW stem filter [Cout][3][7][7] -> G g in the kernel's k order: [7 f][11 quads][Cout][4], element e of quad q is k = 4 q + e
// (sw_k_tap; k = 42, 43 are zeros)
__global__ void __launch_bounds__(256) pack_filter_stem_wino_kernel(const float *w, float4 *out, unsigned total, int Cout) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const int fq = (int)(i / (unsigned)Cout), co = (int)(i - (unsigned)fq * (unsigned)Cout);
    const int f = fq / SW_KQ, q = fq - f * SW_KQ;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int tap = sw_k_tap(4 * q + e, a);
            if (tap >= 0) s = fmaf(sw_G[4 * f + a], w[co * 147 + tap], s);
        }
        v[e] = s;
    }
    out[i] = make_float4(v[0], v[1], v[2], v[3]);
}
