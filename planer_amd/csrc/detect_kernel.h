// Detections as net output: the two kernels around pl_topk_f32 that turn YOLO-style head tensors into
// (N, max_det, 6) rows [x1, y1, x2, y2, score, class] and their count.
//
// decode_kernel: head h is float32 (N, A (5 + C), Gh, Gw).  One lane takes one cell of one anchor, so every plane read is
// coalesced; a workgroup takes TPB consecutive cells of one (image, anchor).  The lane reads the objectness plane t4 first and
// leaves, score -1, unless sigmoid(t4) > conf (the score is that times a sigmoid <= 1, and rounding is monotonic, so it could not
// exceed conf; a NaN objectness fails the comparison).  Only then does it walk the C class planes, CLASS_UNROLL loads in flight,
// with the label kernel's argmax step (the first of equal maxima; a NaN counts as the maximum, the first NaN wins), and only a
// candidate, score = fl(sigmoid(t4) * sigmoid(t[5 + class])) > conf, reads the four box planes and writes class and box:
//     cx = fl(fl(sigmoid(t0) + gx) * sx)   w = fl(exp(t2) * aw)   box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2)
// every operation rounded on its own.  A non-candidate's class and box are NOT written.  Anchors travel as kernel arguments.
// An image's row is stored BACK TO FRONT, anchor index i at position row - 1 - i: pl_topk_f32 (largest) orders equal scores by
// DESCENDING position (it reads a stable ascending sort from its end), which is then ascending anchor index, the contract's order.
//
// nms_kernel: one workgroup per image.  Entry j of the image's K sorted (score, index) pairs is a candidate iff its score > floor
// and its index names a row of the image (anything else is dead from the start, so nothing outside boxes / classes is read).
// The candidates' boxes, areas and classes are gathered into dynamic LDS (24 K bytes), one alive bit per entry beside them.
// Then, until max_det boxes are kept: every wave finds the first alive entry at or behind the cursor with one ballot over the
// (at most 64) mask words; all lanes sweep the entries behind it, each wave owning whole mask words, and clear the bits of those
// it suppresses,
//     iw = max(0, min(x2i, x2j) - max(x1i, x1j))   inter = iw ih   union = (area_i + area_j) - inter   inter > iou union
// in float32, every operation rounded on its own, no division: a zero union or a NaN suppresses nothing.  One barrier per KEPT
// box.  A slower wave that still searches while a faster one already clears bits finds the same entry: only bits behind it
// change.  The kept entries are a second bit mask; at the end every lane writes the rows of the kept entries it owns (row =
// number of kept bits in front), the other rows as +0.0, and lane 0 the count: det and num are written completely.
#pragma once
#include "common.h"
#include "device_utils.h"

namespace detect {

constexpr int TPB = PL_STREAM_TPB;
constexpr int WAVES = TPB / 64;
constexpr int MAX_ANCHORS = PL_YOLO_MAX_ANCHORS;
constexpr int NMS_MAX_K = PL_NMS_MAX_CANDIDATES;
constexpr int CLASS_UNROLL = 4;                           // class planes loaded before the first of them is compared
static_assert(NMS_MAX_K <= 64 * 64, "one ballot covers the alive mask: at most 64 words of 64 bits");

struct Anchors {
    float w[MAX_ANCHORS], h[MAX_ANCHORS];
};

// the reference's sigmoid, 1 / (1 + exp(-v)), as pl_sigmoid_f32 computes it
__device__ __forceinline__ float sigmoid(float v) { return __fdiv_rn(1.f, __fadd_rn(expf(-v), 1.f)); }

// grid = N * A * tiles; block (n, a, tile) takes cells [tile * TPB, ...) of anchor a of image n.  row = A_total, off = where this
// head's anchors start in an image's row.
__global__ void __launch_bounds__(TPB) decode_kernel(const float *x, float *scores, int *classes, float *boxes, int A, int C,
                                                     int Gw, size_t HW, unsigned tiles, Anchors an, float sx, float sy,
                                                     float conf, size_t row, size_t off) {
    const unsigned tile = blockIdx.x % tiles;
    const unsigned na = blockIdx.x / tiles;               // n * A + a
    const int a = (int)(na % (unsigned)A);
    const size_t n = na / (unsigned)A;
    const size_t cell = (size_t)tile * TPB + threadIdx.x;
    if (cell >= HW) return;
    const float *t = x + ((size_t)na * (size_t)(5 + C)) * HW + cell;
    const size_t at = n * row + (row - 1 - (off + (size_t)a * HW + cell));    // the row is stored back to front (see above)
    const float obj = sigmoid(t[4 * HW]);
    if (!(obj > conf)) {
        scores[at] = -1.f;
        return;
    }
    const float *cp = t + 5 * HW;
    float best = cp[0];
    int cls = 0, c = 1;
    for (; c + CLASS_UNROLL <= C; c += CLASS_UNROLL) {
        float v[CLASS_UNROLL];
#pragma unroll
        for (int u = 0; u < CLASS_UNROLL; ++u) v[u] = cp[(size_t)(c + u) * HW];
#pragma unroll
        for (int u = 0; u < CLASS_UNROLL; ++u) {
            const bool take = v[u] > best || (v[u] != v[u] && best == best);
            best = take ? v[u] : best;
            cls = take ? c + u : cls;
        }
    }
    for (; c < C; ++c) {
        const float v = cp[(size_t)c * HW];
        const bool take = v > best || (v != v && best == best);
        best = take ? v : best;
        cls = take ? c : cls;
    }
    const float score = __fmul_rn(obj, sigmoid(best));
    if (!(score > conf)) {
        scores[at] = -1.f;
        return;
    }
    const float t0 = t[0], t1 = t[HW], t2 = t[2 * HW], t3 = t[3 * HW];
    const unsigned gy = (unsigned)(cell / (unsigned)Gw), gx = (unsigned)(cell - (size_t)gy * (unsigned)Gw);
    const float cx = __fmul_rn(__fadd_rn(sigmoid(t0), (float)gx), sx);
    const float cy = __fmul_rn(__fadd_rn(sigmoid(t1), (float)gy), sy);
    const float hw = __fmul_rn(__fmul_rn(expf(t2), an.w[a]), 0.5f);
    const float hh = __fmul_rn(__fmul_rn(expf(t3), an.h[a]), 0.5f);
    scores[at] = score;
    classes[at] = cls;
    float *b = boxes + at * 4;
    b[0] = __fsub_rn(cx, hw);
    b[1] = __fsub_rn(cy, hh);
    b[2] = __fadd_rn(cx, hw);
    b[3] = __fadd_rn(cy, hh);
}

// dynamic LDS of nms_kernel for K entries: x1, y1, x2, y2, area, class (K words each), then the alive and the kept mask
__host__ __device__ constexpr int nms_words(int K) { return (K + 63) / 64; }
__host__ __device__ constexpr size_t nms_lds_bytes(int K) { return (size_t)K * 24 + (size_t)nms_words(K) * 16; }

// The first set bit at or behind `cur` in the `words` 64-bit words of `mask`, or -1.  Every lane of the wave gets the answer.
__device__ __forceinline__ int first_alive(const unsigned long long *mask, int words, int cur, int lane) {
    const int cw = cur >> 6;
    unsigned long long m = lane < words && lane >= cw ? mask[lane] : 0ull;
    if (lane == cw) m &= ~0ull << (cur & 63);
    const unsigned long long any = __ballot(m != 0ull);
    if (!any) return -1;
    const int w = __ffsll((long long)any) - 1;
    unsigned long long mw = mask[w];
    if (w == cw) mw &= ~0ull << (cur & 63);
    if (!mw) return -1;                                   // (cannot happen: bits at or in front of the answer never change)
    return (w << 6) + __ffsll((long long)mw) - 1;
}

// grid = N.  boxes (N, R, 4), classes (N, R) or null, sorted (N, K) descending scores, order (N, K) their rows in [0, R).
__global__ void __launch_bounds__(TPB) nms_kernel(const float *boxes, const int *classes, const float *sorted,
                                                  const long long *order, int R, int K, float low, float iou, bool class_aware,
                                                  int max_det, float *det, int *num) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_smem[];
    float *x1 = reinterpret_cast<float *>(nms_smem), *y1 = x1 + K, *x2 = y1 + K, *y2 = x2 + K, *area = y2 + K;
    int *cls = reinterpret_cast<int *>(area + K);
    const int words = nms_words(K);
    // (24 K bytes in front: 8-byte aligned whatever K is)
    unsigned long long *alive = reinterpret_cast<unsigned long long *>(nms_smem + (size_t)K * 24), *keep = alive + words;
    const size_t n = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float *sc = sorted + n * (size_t)K;
    const long long *ord = order + n * (size_t)K;

    for (int base = wave * 64; base < K; base += TPB) {
        const int j = base + lane;
        bool ok = false;
        if (j < K) {
            const long long r = ord[j];
            ok = sc[j] > low && r >= 0 && r < (long long)R;
            if (ok) {
                const float *b = boxes + (n * (size_t)R + (size_t)r) * 4;
                const float bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
                x1[j] = bx1, y1[j] = by1, x2[j] = bx2, y2[j] = by2;
                area[j] = __fmul_rn(__fsub_rn(bx2, bx1), __fsub_rn(by2, by1));
                cls[j] = classes ? classes[n * (size_t)R + (size_t)r] : 0;
            }
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) alive[base >> 6] = m, keep[base >> 6] = 0ull;
    }
    __syncthreads();

    int kept = 0, cur = 0;
    while (kept < max_det) {
        const int i = first_alive(alive, words, cur, lane);
        if (i < 0) break;
        if (t == 0) keep[i >> 6] |= 1ull << (i & 63);
        ++kept;
        cur = i + 1;
        if (kept == max_det) break;
        const float ix1 = x1[i], iy1 = y1[i], ix2 = x2[i], iy2 = y2[i], ia = area[i];
        const int ic = cls[i];
        for (int base = (i & ~63) + wave * 64; base < K; base += TPB) {
            const int j = base + lane;
            const unsigned long long word = alive[base >> 6];
            bool sup = false;
            if (j > i && j < K && ((word >> lane) & 1ull)) {
                const float iw = fmaxf(0.f, __fsub_rn(fminf(ix2, x2[j]), fmaxf(ix1, x1[j])));
                const float ih = fmaxf(0.f, __fsub_rn(fminf(iy2, y2[j]), fmaxf(iy1, y1[j])));
                const float inter = __fmul_rn(iw, ih);
                const float uni = __fsub_rn(__fadd_rn(ia, area[j]), inter);
                sup = inter > __fmul_rn(iou, uni) && (!class_aware || cls[j] == ic);
            }
            const unsigned long long s = __ballot(sup);
            if (lane == 0 && s) alive[base >> 6] = word & ~s;
        }
        __syncthreads();
    }
    __syncthreads();

    float *d = det + n * (size_t)max_det * 6;
    for (int base = wave * 64; base < K; base += TPB) {
        const int j = base + lane, w = base >> 6;
        const unsigned long long kw = keep[w];
        if (j < K && ((kw >> lane) & 1ull)) {
            int rowi = __popcll(kw & ((1ull << lane) - 1ull));
            for (int q = 0; q < w; ++q) rowi += __popcll(keep[q]);
            float *o = d + (size_t)rowi * 6;
            o[0] = x1[j], o[1] = y1[j], o[2] = x2[j], o[3] = y2[j], o[4] = sc[j], o[5] = (float)cls[j];
        }
    }
    for (int e = kept * 6 + t; e < max_det * 6; e += TPB) d[e] = 0.f;
    if (t == 0) num[n] = kept;
}

}  // namespace detect
