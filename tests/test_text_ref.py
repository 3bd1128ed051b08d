"""tests/text_ref.py, the mirror pl_ctc_greedy_f32 is held to, against an independent restatement -- `np.argmax` and
`itertools.groupby` -- and against the rules of include/planer_hip.h for NaN and the infinities; and the calibration of the
softmax confidence's bound."""
import itertools
import math

import numpy as np
import pytest

from tests import text_ref as R

F32, I32 = np.float32, np.int32


def restated(x, layout, blank, merge_repeated, max_len, lengths):
    """Greedy CTC as a caller writes it: argmax(-1), groupby, drop the blanks.  -> (text, length, spans, first frames)"""
    seq = {"tnc": lambda a: a.transpose(1, 0, 2), "ntc": lambda a: a,
           "nchw": lambda a: a.transpose(0, 2, 3, 1).reshape(-1, a.shape[3], a.shape[1])}[layout](x)
    S, T, _ = seq.shape
    best = np.argmax(seq, -1)
    text, length, spans = np.full((S, max_len), -1, I32), np.zeros(S, I32), np.zeros((S, max_len, 2), I32)
    firsts = np.full((S, max_len), -1, np.int64)
    for s in range(S):
        n = T if lengths is None else max(0, min(int(np.asarray(lengths).reshape(-1)[s]), T))
        frames = list(enumerate(best[s, :n]))
        groups = itertools.groupby(frames, key=lambda f: f[1]) if merge_repeated else ((f[1], [f]) for f in frames)
        runs = [(lab, [t for t, _ in run]) for lab, run in groups]
        symbols = [(lab, ts[0], ts[-1] + 1) for lab, ts in runs if lab != blank]
        length[s] = len(symbols)
        for k, (lab, t0, t1) in enumerate(symbols[:max_len]):
            text[s, k], spans[s, k], firsts[s, k] = lab, (t0, t1), t0
    return text, length, spans, firsts, seq


CASES = [  # layout, shape, blank, merge, max_len, lengths
    ("tnc", (12, 5, 4), 0, True, 64, None),
    ("tnc", (12, 5, 4), 3, True, 64, None),
    ("ntc", (5, 12, 4), 1, False, 64, None),
    ("ntc", (6, 30, 3), 0, True, 4, None),                  # length > max_len
    ("ntc", (6, 30, 3), 2, False, 7, [0, 31, 30, 1, 17, -3]),
    ("tnc", (9, 4, 2), 0, True, 1, [9, 0, 100, 5]),
    ("nchw", (2, 5, 3, 11), 0, True, 8, None),
    ("nchw", (2, 5, 3, 11), 4, True, 8, np.arange(6).reshape(2, 3) * 3),
    ("nchw", (1, 1, 2, 7), 0, True, 3, None),               # one class: every frame is the blank
    ("tnc", (0, 3, 4), 0, True, 5, None),                   # no frame
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("confidence", ["softmax", "value", "none"])
def test_mirror_against_the_restatement(case, confidence):
    layout, shape, blank, merge, max_len, lengths = CASES[case]
    rng = np.random.default_rng(100 + case)
    x = rng.integers(-2, 3, shape).astype(F32)              # small integers: ties in most frames
    text, length, conf, spans = R.ctc_greedy(x, layout, blank, merge, confidence, max_len, lengths)
    wt, wl, ws, firsts, seq = restated(x, layout, blank, merge, max_len, lengths)
    lead = (shape[0], shape[2]) if layout == "nchw" else (shape[1] if layout == "tnc" else shape[0],)
    assert text.shape == lead + (max_len,) and length.shape == lead and conf.shape == lead + (max_len,) and spans.shape == lead + (max_len, 2)
    assert (text.dtype, length.dtype, conf.dtype, spans.dtype) == (I32, I32, F32, I32)
    assert np.array_equal(text.reshape(wt.shape), wt) and np.array_equal(length.reshape(-1), wl)
    assert np.array_equal(spans.reshape(ws.shape), ws)
    conf = conf.reshape(firsts.shape)
    for s, k in np.ndindex(firsts.shape):
        t = firsts[s, k]
        if t < 0:
            assert conf[s, k] == 0 and not np.signbit(conf[s, k])
        elif confidence == "softmax":
            row = seq[s, t].astype(np.float64)
            assert conf[s, k] == F32(1 / np.exp(row - row.max()).sum())
        elif confidence == "value":
            assert conf[s, k] == seq[s, t].max()
        else:
            assert conf[s, k] == 0
    if case == 3:
        assert (length > max_len).any()


def test_special_values():
    nan, inf = np.nan, np.inf
    rows = np.array([[1, nan, 5, nan],          # the first NaN wins over any number
                     [nan, 9, 9, 9],
                     [-inf, -inf, -inf, -inf],    # all equal: the first
                     [0, inf, inf, 1],            # the first of equal maxima
                     [-1, -0.0, 0.0, -2],         # -0.0 ties with +0.0
                     [-1, 0.0, -0.0, -2],
                     [-inf, 3, -inf, 3],
                     [2, 1, -inf, 0]], F32)
    assert R.frame_labels(rows).tolist() == [1, 0, 0, 1, 1, 1, 1, 0]
    assert np.array_equal(R.frame_labels(rows), np.argmax(rows, -1))
    c = R.frame_conf64(rows)
    assert np.isnan(c[:4]).all() and np.isfinite(c[4:]).all()          # NaN when the maximum is NaN, -inf or +inf
    assert c[6] == 0.5 and c[7] == 1 / (1 + math.exp(-1) + math.exp(-2))
    v = R.frame_conf(rows, R.frame_labels(rows), "value")
    assert np.isnan(v[:2]).all() and v[2] == -inf and v[3] == inf
    assert np.signbit(v[4]) and not np.signbit(v[5])                    # the bits of x at the argmax
    assert not R.frame_conf(rows, R.frame_labels(rows), "none").any()
    # through the decode: conf is NaN exactly on the symbols whose first frame's maximum is not finite
    x = rows.reshape(1, 8, 4)
    text, length, conf, spans = R.ctc_greedy(x, "ntc", blank=0, max_len=8)
    assert length.tolist() == [2] and text[0, :3].tolist() == [1, 1, -1] and spans[0, :2].tolist() == [[0, 1], [3, 7]]
    assert np.isnan(conf[0, :2]).all() and not conf[0, 2:].any()
    text, length, conf, spans = R.ctc_greedy(x, "ntc", blank=2, merge_repeated=False, max_len=8)
    assert text[0].tolist() == [1, 0, 0, 1, 1, 1, 1, 0] and np.isnan(conf[0, :4]).all() and np.isfinite(conf[0, 4:]).all()
    text, length, conf, spans = R.ctc_greedy(x, "ntc", blank=2, max_len=8)
    assert text[0].tolist() == [1, 0, 1, 0, -1, -1, -1, -1] and spans[0, :4].tolist() == [[0, 1], [1, 3], [3, 7], [7, 8]]
    assert np.isnan(conf[0, :3]).all() and conf[0, 3] == F32(c[7]) and not conf[0, 4:].any()


def test_emulations_pick_the_mirrors_labels():
    """The float32 emulations of the kernels' lane orders and merges give numpy's argmax, ties, NaNs and -inf rows included."""
    rng = np.random.default_rng(5)
    for C in (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1025):
        x = rng.integers(-2, 3, (24, C)).astype(F32)
        x[::5, rng.integers(0, C)] = np.nan
        x[1::7] = -np.inf
        x[2::9, rng.integers(0, C)] = np.inf
        want = np.argmax(x, -1)
        assert np.array_equal(R.frame_labels(x), want)
        for mis in range(4):
            assert np.array_equal(R.emulate_rows(x, mis)[0], want), (C, mis)
        assert np.array_equal(R.emulate_time(x)[0], want), C
        nan = np.isnan(R.frame_conf64(x))
        assert np.array_equal(np.isnan(R.emulate_rows(x, 1)[1]), nan) and np.array_equal(np.isnan(R.emulate_time(x)[1]), nan)


def test_calibration_constant_covers_the_emulations():
    worst = {"rows": 0.0, "time": 0.0}
    for name, form, mis, rows in R.calibration_cases():
        ratio = R.emulated_ratio(form, mis, rows)
        assert 4 * ratio <= R.LAM_TEXT, (name, ratio)
        worst[form] = max(worst[form], ratio)
    print("worst emulated ratios: rows %.4f, time %.4f; LAM_TEXT %.3g" % (worst["rows"], worst["time"], R.LAM_TEXT))
    assert R.LAM_TEXT <= 8 * max(worst.values())             # (and is not slack by more than its rounding up)
    assert R.stages(37, "rows") == 4 + 8 and R.stages(1025, "rows") == 8 + 8 + 3 and R.stages(6625, "time") == 208 + 31


def test_mutations_of_the_emulation_miss_the_bound():
    """The bound is tight enough to see a sloppy exp: 2^-12 relative error per call is far outside it."""
    rows = R.spread_rows(np.random.default_rng(11), 6, 257, 8.0)
    keep = R._exp32
    try:
        R._exp32 = lambda d: (keep(d) * F32(1 + 2.0 ** -12)).astype(F32)
        conf = R.emulate_rows(rows)[1]
    finally:
        R._exp32 = keep
    assert (np.abs(conf.astype(np.float64) - R.frame_conf64(rows)) > R.conf_bound(rows, "rows")).any()
    conf = R.emulate_rows(rows)[1]
    assert (np.abs(conf.astype(np.float64) - R.frame_conf64(rows)) <= R.conf_bound(rows, "rows")).all()
