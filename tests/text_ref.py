"""The numpy mirror of pl_ctc_greedy_f32 (include/planer_hip.h, csrc/text_kernel.h): greedy CTC decoding of a float32 sequence
tensor, and the float64 reference and error bound of its softmax confidence, in the pattern of tests/ref64_ops.py.

Everything but the softmax confidence is exact, so `ctc_greedy` is held to the kernel bit for bit.  The softmax confidence of a
frame is 1 / S, S = sum_c exp(x_c - m); the kernels read each class once and keep a running (max, sum), so a term's way into S is

    exp(x_c - m_1) * exp(m_1 - m_2) * ... * exp(m_k - m)        (m_1 <= m_2 <= ... <= m: the maxima its partial sum lived under)

with one float32 addition per later term of its lane and per merge level.  The differences telescope, so the roundings of the
exponents add up to at most u |x_c - m| relative error of the term (u = 2^-24).  Each factor carries ULP["exp"] ulps (2u
relative each), each product and each addition u; a term passes at most K(C) such stages,

    rows form   (class-contiguous):  K = 4 ceil(ceil(C / 4) / G) + 2 lane steps + 6 butterfly levels (+ 3 wave folds where the
                                     row is a workgroup's, G = 256; G = 64 up to PL_TEXT_ROW_WAVE_MAX classes)
    time form   (class-strided):     K = ceil(C / 32) lane steps + 31 group folds

and the division is correctly rounded (u).  At lam = 1 the relative bound on 1 / S is therefore

    u * ( sum_c exp(x_c - m) |x_c - m| / S  +  K (2 ULP["exp"] + 2)  +  1 )

LAM_TEXT is 4x the worst err / (bound at lam = 1) of the float32 emulations of the kernels' order of operations (`emulate_rows`,
`emulate_time`) over `calibration_cases`, rounded up; tests/test_text_ref.py checks that it still covers them.  The bound is
compared against the float64 value, never against the kernel.
"""
import math

import numpy as np

from tests.ref64_ops import U, ULP

F32, I32 = np.float32, np.int32
ROW_WAVE_MAX, TIME_GROUPS = 1024, 32         # include/planer_hip.h PL_TEXT_ROW_WAVE_MAX, PL_TEXT_TIME_GROUPS
NONE = 0x7FFFFFFF
# worst emulated ratios (tests/test_text_ref.py): rows 0.0424, time 0.0227
LAM_TEXT = 0.2


# ---- the mirror ---------------------------------------------------------------------------------------------------------------
def frames_of(x, layout):
    """(lead, x as (S, T, C)) of a sequence tensor in `layout`: "tnc", "ntc", or "nchw" with a line per (n, h) and time along W."""
    x = np.asarray(x, F32)
    if layout == "tnc":
        return (x.shape[1],), x.transpose(1, 0, 2)
    if layout == "ntc":
        return (x.shape[0],), x
    n, c, h, w = x.shape
    return (n, h), x.transpose(0, 2, 3, 1).reshape(n * h, w, c)


def frame_labels(rows):
    """numpy's argmax of every row of (R, C), spelt out: the first NaN, else the first position that equals the maximum."""
    rows = np.asarray(rows, F32)
    nan = np.isnan(rows)
    with np.errstate(invalid="ignore"):
        top = np.where(nan, -np.inf, rows).max(-1, keepdims=True)
    return np.where(nan.any(-1), nan.argmax(-1), (rows == top).argmax(-1)).astype(I32)


def frame_conf64(rows):
    """1 / sum_c exp(x_c - m) of every row of (R, C) in float64; NaN where the maximum m is not finite."""
    x = np.asarray(rows, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(-1, keepdims=True)                        # (NaN-propagating)
        good = np.isfinite(m[:, 0])
        s = np.exp(np.where(good[:, None], x - np.where(good[:, None], m, 0.0), 0.0)).sum(-1)
    return np.where(good, 1.0 / s, np.nan)


def frame_conf(rows, labels, confidence):
    rows = np.asarray(rows, F32)
    if confidence == "softmax":
        return frame_conf64(rows).astype(F32)
    if confidence == "value":
        return rows[np.arange(rows.shape[0]), labels]
    return np.zeros(rows.shape[0], F32)


def ctc_greedy(x, layout="tnc", blank=0, merge_repeated=True, confidence="softmax", max_len=64, lengths=None):
    """(text, length, conf, spans) as pl_ctc_greedy_f32 defines them; conf in softmax mode is the float64 value rounded."""
    lead, seq = frames_of(x, layout)
    S, T, C = seq.shape
    labels = frame_labels(seq.reshape(S * T, C)).reshape(S, T)
    confs = frame_conf(seq.reshape(S * T, C), labels.reshape(-1), confidence).reshape(S, T)
    valid = np.full(S, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64).reshape(S), 0, T)
    text, length = np.full((S, max_len), -1, I32), np.zeros(S, I32)
    conf, spans = np.zeros((S, max_len), F32), np.zeros((S, max_len, 2), I32)
    for s in range(S):
        k, t, n = 0, 0, int(valid[s])
        while t < n:
            lab, end = labels[s, t], t + 1
            if merge_repeated:
                while end < n and labels[s, end] == lab:
                    end += 1
            if lab != blank:
                if k < max_len:
                    text[s, k], conf[s, k], spans[s, k] = lab, confs[s, t], (t, end)
                k += 1
            t = end
        length[s] = k
    return text.reshape(lead + (max_len,)), length.reshape(lead), conf.reshape(lead + (max_len,)), spans.reshape(lead + (max_len, 2))


# ---- the softmax confidence's bound ---------------------------------------------------------------------------------------------
def stages(C, form):
    """K(C) of the module docstring."""
    if form == "time":
        return math.ceil(C / TIME_GROUPS) + TIME_GROUPS - 1
    G = 64 if C <= ROW_WAVE_MAX else 256
    return 4 * math.ceil(math.ceil(C / 4) / G) + 2 + 6 + (3 if G == 256 else 0)


def conf_bound(rows, form, lam=None):
    """Absolute bound per row of finite (R, C) on the softmax confidence against `frame_conf64`."""
    lam = LAM_TEXT if lam is None else lam
    x = np.asarray(rows, np.float64)
    d = x - x.max(-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(-1)
    with np.errstate(invalid="ignore"):
        spread = np.where(e > 0, e * np.abs(d), 0.0).sum(-1) / s          # (a class at -inf adds nothing)
    return lam * U * (spread + stages(x.shape[-1], form) * (2 * ULP["exp"] + 2) + 1) / s


# ---- float32 emulations of the kernels' order of operations ---------------------------------------------------------------------
def _exp32(d):
    """A correctly rounded expf; 0 where the argument is NaN (text_kernel.h exp_or_zero)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(d), F32(0), np.exp(d.astype(np.float64)).astype(F32)).astype(F32)


def _step(p, x, c, live):
    """text_kernel.h step on the lanes where `live`: p = (v, i, s) arrays, x the class values, c their indices."""
    v, i, s = p
    with np.errstate(invalid="ignore", over="ignore"):
        take = live & ((x > v) | (np.isnan(x) & ~np.isnan(v)))
        e = _exp32(np.where(take, v - x, x - v).astype(F32))
        s2 = np.where(take, ((s * e).astype(F32) + F32(1)).astype(F32), (s + e).astype(F32))
    return np.where(take, x, v).astype(F32), np.where(take, c, i), np.where(live, s2, s).astype(F32)


def _merge(a, b):
    """text_kernel.h merge of two partials."""
    (av, ai, as_), (bv, bi, bs) = a, b
    an, bn = np.isnan(av), np.isnan(bv)
    with np.errstate(invalid="ignore", over="ignore"):
        first = np.where(an | bn, an & (~bn | (ai < bi)), (av > bv) | ((av == bv) & (ai < bi)))
        wv, wi, ws = np.where(first, av, bv), np.where(first, ai, bi), np.where(first, as_, bs)
        lv, ls = np.where(first, bv, av), np.where(first, bs, as_)
        s = (ws + (ls * _exp32((lv - wv).astype(F32))).astype(F32)).astype(F32)
    return wv.astype(F32), wi, s


def _start(shape):
    return np.full(shape, -np.inf, F32), np.full(shape, NONE, np.int64), np.zeros(shape, F32)


def _finish(p):
    v, i, s = p
    with np.errstate(invalid="ignore", divide="ignore"):
        conf = np.where(np.isfinite(v), (F32(1) / s).astype(F32), F32(np.nan)).astype(F32)
    return np.where(i == NONE, 0, i).astype(I32), conf


def _run(rows, schedule, lanes):
    """Every lane steps the classes `schedule` gives it: a list of (lanes,) index arrays, -1 for a lane without one."""
    R = rows.shape[0]
    p = _start((R, lanes))
    for idx in schedule:
        live = np.broadcast_to(idx >= 0, (R, lanes))
        p = _step(p, rows[:, np.maximum(idx, 0)], np.broadcast_to(idx, (R, lanes)), live)
    return p


def emulate_rows(rows, mis=0):
    """rows_wave_kernel / rows_block_kernel on (R, C) whose rows start `mis` floats behind a 16-byte boundary -> (labels, conf)."""
    rows = np.asarray(rows, F32)
    R, C = rows.shape
    G = 64 if C <= ROW_WAVE_MAX else 256
    lane = np.arange(G)
    head = min((4 - mis) & 3, C)
    nvec = (C - head) // 4
    tail0 = head + 4 * nvec
    schedule = [np.where(lane < head, lane, -1)]
    for k in range(math.ceil(nvec / G)):
        for e in range(4):
            schedule.append(np.where(lane + k * G < nvec, head + 4 * (lane + k * G) + e, -1))
    schedule.append(np.where(tail0 + lane < C, tail0 + lane, -1))
    p = tuple(a.reshape(R, G // 64, 64) for a in _run(rows, schedule, G))
    off = 32
    while off:
        p = _merge(tuple(a[..., :off] for a in p), tuple(a[..., off:2 * off] for a in p))
        off >>= 1
    r = tuple(a[:, 0, 0] for a in p)
    for w in range(1, G // 64):
        r = _merge(r, tuple(a[:, w, 0] for a in p))
    return _finish(r)


def emulate_time(rows):
    """time_kernel on (R, C): the classes in TIME_GROUPS contiguous shares, folded in order -> (labels, conf)."""
    rows = np.asarray(rows, F32)
    R, C = rows.shape
    q = math.ceil(C / TIME_GROUPS)
    c0 = np.minimum(np.arange(TIME_GROUPS) * q, C)
    c1 = np.minimum(c0 + q, C)
    p = _run(rows, [np.where(c0 + k < c1, c0 + k, -1) for k in range(q)], TIME_GROUPS)
    r = tuple(a[:, 0] for a in p)
    for g in range(1, TIME_GROUPS):
        r = _merge(r, tuple(a[:, g] for a in p))
    return _finish(r)


def spread_rows(rng, rows, C, spread):
    """Finite logits: normal with standard deviation `spread` / 3, a few rows stretched over +-`spread`."""
    x = rng.standard_normal((rows, C)) * (spread / 3)
    x[::3] = rng.uniform(-spread, spread, (len(x[::3]), C))
    return x.astype(F32)


def calibration_cases():
    """(name, form, mis, rows) over the class counts where the kernels change their path and over narrow to wide logits."""
    rng = np.random.default_rng(29)
    for C in (1, 5, 37, 257, 1024, 1025, 6625):
        for spread in (1.0, 8.0, 30.0):
            x = spread_rows(rng, 12, C, spread)
            for mis in range(4):
                yield "rows C=%d spread=%g mis=%d" % (C, spread, mis), "rows", mis, x
            yield "time C=%d spread=%g" % (C, spread), "time", 0, x


def emulated_ratio(form, mis, rows):
    """The worst |emulation - float64| / (bound at lam = 1) over the rows."""
    conf = (emulate_rows(rows, mis) if form == "rows" else emulate_time(rows))[1]
    return float((np.abs(conf.astype(np.float64) - frame_conf64(rows)) / conf_bound(rows, form, lam=1.0)).max())
