"""Text as net output on a real MI355X: pl_ctc_greedy_f32, util.ctc_decode, util.TextSpec.

Labels, lengths and spans equal tests/text_ref.py's bit for bit, and so does the confidence in value and none mode; the softmax
confidence is held to the float64 value within the bound text_ref derives, and is NaN exactly where the mirror's is.  The launches
write into outputs framed by sentinel words that must survive, from a framed scratch block; one pass over a long case list runs
with the pool in hygiene mode.  Shapes come from what the kernels do at them: rows shorter than a vector and a wave and one past
each, misaligned for 16-byte loads, on either side of the wave / workgroup threshold; class counts that leave lane groups of the
class-strided form empty; sequences around the collapse pass's chunk."""
import functools

import numpy as np
import pytest

from tests import head_kit as K
from tests import text_ref as R
from tests.head_kit import EINVAL, EUNSUPPORTED, F32, I32, OK, Framed

pytestmark = pytest.mark.gpu

NAMES = ("text", "length", "conf", "spans")
CONF = {"none": 0, "softmax": 1, "value": 2}
MODES = ("softmax", "value", "none")

_C = K.header_constants("PL_TEXT_")
CHUNK, MAX_LEN, MAX_FRAMES, ROW_WAVE_MAX = (_C["PL_TEXT_" + k] for k in ("CHUNK", "MAX_LEN", "MAX_FRAMES", "ROW_WAVE_MAX"))


@pytest.fixture(scope="module")
def pa():
    import planer_amd
    planer_amd.hip.context()
    return planer_amd


def form_of(layout):
    return "time" if layout == "nchw" else "rows"


def chain(pa, x, layout, blank, merge, confidence, max_len, lengths=None, off=0):
    """pl_ctc_greedy_f32 through the C interface on framed outputs and a framed scratch block, x starting `off` floats into its
    allocation.  -> (status, (text, length, conf, spans), every frame intact)."""
    ctx = pa.hip.context()
    lead, n, inner, t, c, st = pa.util.TextSpec(layout, blank, merge, confidence, max_len).geometry(x.shape)
    s = n * inner
    dev = pa.hip.empty((x.size + off + 1,), F32)
    if x.size:
        dev.set(np.concatenate([np.full(off, np.nan, F32), x.ravel(), np.full(1, np.nan, F32)]))
    lens = None if lengths is None else pa.hip.asarray(np.asarray(lengths, I32).reshape(-1))
    text, length, conf, spans = Framed(pa, s * max_len), Framed(pa, s), Framed(pa, s * max_len), Framed(pa, s * max_len * 2)
    scratch = Framed(pa, s * t * 2)
    rc = pa._lib.load().pl_ctc_greedy_f32(ctx.handle, dev.ptr + 4 * off, n, inner, t, c, st[0], st[1], st[2], st[3],
                                          None if lens is None else lens.ptr, blank, int(merge), CONF[confidence], max_len, scratch.ptr,
                                          text.ptr, length.ptr, conf.ptr, spans.ptr)
    got = [f.get(d, lead + tail) for f, d, tail in ((text, I32, (max_len,)), (length, I32, ()), (conf, F32, (max_len,)), (spans, I32, (max_len, 2)))]
    return rc, tuple(g[0] for g in got), all(g[1] for g in got) and scratch.get()[1]


def softmax_ratio(conf, ref, x, layout, what):
    """The softmax confidences of the symbols against float64: NaN exactly where that is, else inside text_ref's bound; +0.0
    behind the symbols.  -> worst err / tol."""
    _, seq = R.frames_of(x, layout)
    S, _, C = seq.shape
    m = ref[0].shape[-1]
    length, spans, conf = ref[1].reshape(S), ref[3].reshape(S, m, 2), conf.reshape(S, m)
    used = np.arange(m)[None, :] < np.minimum(length, m)[:, None]
    assert not conf[~used].view(np.uint32).any(), what
    si, ki = np.nonzero(used)
    if not si.size:
        return 0.0
    rows = seq[si, spans[si, ki, 0]]
    want, got = R.frame_conf64(rows), conf[si, ki].astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    if nan.all():
        return 0.0
    ratio = np.abs(got[~nan] - want[~nan]) / R.conf_bound(rows[~nan], form_of(layout))
    assert ratio.max() <= 1, "%s: softmax confidence off by %.3g of its bound" % (what, ratio.max())
    return float(ratio.max())


def check(got, ref, x, layout, confidence, what):
    if confidence == "softmax":
        K.same((got[0], got[1], got[3]), (ref[0], ref[1], ref[3]), ("text", "length", "spans"), what)
        assert got[2].shape == ref[2].shape and got[2].dtype == F32, what
        return softmax_ratio(got[2], ref, x, layout, what)
    K.same(got, ref, NAMES, what)
    return 0.0


def run_case(pa, case, off=0):
    what, x, layout, blank, merge, confidence, max_len, lengths, ref = case
    rc, got, intact = chain(pa, x, layout, blank, merge, confidence, max_len, lengths, off)
    assert rc == OK and intact, what
    return check(got, ref, x, layout, confidence, what)


def make_case(what, x, layout, blank=0, merge=True, confidence="softmax", max_len=8, lengths=None):
    ref = R.ctc_greedy(x, layout, blank, merge, confidence, max_len, lengths)
    for a in (x,) + ref:
        a.setflags(write=False)
    return ("%s %s %s blank %d merge %d %s max_len %d lengths %s" % (what, layout, x.shape, blank, merge, confidence, max_len,
                                                                     None if lengths is None else np.asarray(lengths).ravel().tolist()[:6]),
            x, layout, blank, merge, confidence, max_len, lengths, ref)


# ---- class-contiguous boundaries ------------------------------------------------------------------------------------------------
ROW_C = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1025)


def plants(C):
    """Where a row's maximum goes: first, last, interior, and pairs of equal maxima on either side of a vector and a lane
    boundary of every alignment (vectors begin 0..3 floats into the row) and of the 64th and 256th vector."""
    single = [(0,), (C - 1,), (C // 2,)]
    pairs = [(p, p + 1) for p in (0, 1, 2, 3, 4, 6, 7, 63, 64, 65, 255, 256, 257, 258, 259, 1022, 1023) if p + 1 < C]
    far = [(p, q) for p, q in ((0, C - 1), (1, C - 2), (3, 260), (64, 256)) if p < q < C]
    return single + pairs + far


@functools.lru_cache(maxsize=None)
def row_cases(C):
    rng = np.random.default_rng(C)
    where = plants(C)
    out = []
    for v in range(-(-len(where) // 6) + 1):
        x = rng.integers(-2, 3, (2, 3, C)).astype(F32)                        # six frames; ties are the rule
        if v:
            for j in range(6):
                x[j // 3, j % 3, list(where[((v - 1) * 6 + j) % len(where)])] = 9
        layout = ("ntc", "tnc")[v % 2]
        out.append(make_case("rows %d" % v, x, layout, blank=(0, C - 1)[v % 2], merge=v % 3 != 1, confidence=MODES[v % 3], max_len=4))
    return out


@pytest.mark.parametrize("C", ROW_C)
def test_class_contiguous_boundaries(pa, C):
    cases = row_cases(C)
    assert len(cases) >= 2
    for i, case in enumerate(cases):
        for off in (0, 1, 2, 3):                                               # every alignment of the first row
            run_case(pa, case, off)


# ---- time-contiguous boundaries -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def time_cases(W, H):
    out = []
    for i, C in enumerate((1, 3, 65, 257)):
        rng = np.random.default_rng(W * 1000 + H * 10 + i)
        x = rng.integers(-2, 3, (2, C, H, W)).astype(F32)
        lengths = None if i % 2 == 0 else rng.integers(-1, W + 3, (2, H))
        out.append(make_case("time", x, "nchw", blank=(0, C - 1)[i % 2], merge=i != 2, confidence=MODES[(i + W) % 3], max_len=(6, 1, 70)[i % 3],
                             lengths=lengths))
    return out


@pytest.mark.parametrize("H", (1, 3))
@pytest.mark.parametrize("W", (1, 63, 64, 65, 130))
def test_time_contiguous_boundaries(pa, W, H):
    for case in time_cases(W, H):
        run_case(pa, case)
        run_case(pa, case, off=1)


# ---- collapse boundaries --------------------------------------------------------------------------------------------------------
def one_hot(labels, C):
    """Logits whose argmax is `labels` (S, T): 5 at the label, small integers below it elsewhere."""
    S, T = labels.shape
    x = np.random.default_rng(S * 7 + T).integers(-2, 3, (S, T, C)).astype(F32)
    x[np.arange(S)[:, None], np.arange(T)[None, :], labels] = 5
    return x


def collapse_labels(T, C, blank, symbols):
    """Four lines of T frames: random runs; all blank; a run across the chunk boundary and a repeat on either side of it; and
    exactly `symbols` symbols (a label, a blank, a label, ...) as far as T allows."""
    rng = np.random.default_rng(T * 10 + C)
    other = [c for c in range(C) if c != blank]
    lab = np.full((4, T), blank, np.int64)
    lab[0] = np.repeat(rng.integers(0, C, T), rng.integers(1, 4, T))[:T]
    if T > CHUNK:
        lab[2, CHUNK - 3:min(CHUNK + 3, T)] = other[0]                        # one run over the boundary
        lab[2, CHUNK - 5] = other[-1]
        if CHUNK + 4 < T:
            lab[2, CHUNK + 4] = other[0]
    elif T:
        lab[2, T // 2:] = other[0]                                            # a run that ends with the line
    if T >= 2 * CHUNK + 1:
        lab[2, 2 * CHUNK - 1:2 * CHUNK + 1] = other[-1]                       # a repeat whose frames sit on either side
    n = min(symbols, (T + 1) // 2)
    lab[3, 0:2 * n:2] = [other[k % len(other)] for k in range(n)]
    return lab


@functools.lru_cache(maxsize=None)
def collapse_cases(T):
    out, C, i = [], 4, 0
    for blank in (0, C - 1):
        for merge in (True, False):
            for max_len, symbols in ((5, 4), (5, 5), (5, 6), (1, 3), (MAX_LEN, 40)):
                lab = collapse_labels(T, C, blank, symbols)
                mid = T // 2 + 1                                              # (inside line 2's run)
                for lengths in (None, [0, T + 9, mid, T], [T, 1, max(T - 1, 0), min(2 * symbols - 1, T)]):
                    if lengths is not None and (i + max_len) % 2:
                        continue
                    i += 1
                    out.append(make_case("collapse", one_hot(lab, C), "ntc", blank, merge, MODES[i % 3], max_len, lengths))
    return out


@pytest.mark.parametrize("T", (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1))
def test_collapse_boundaries(pa, T):
    cases = collapse_cases(T)
    for case in cases:
        run_case(pa, case)
    if T == 2 * CHUNK + 1:                                                    # the list holds what it claims
        lengths = {(c[6], int(c[8][1].reshape(-1)[3])) for c in cases if c[4] and c[7] is None}
        assert {(5, 4), (5, 5), (5, 6), (1, 3), (MAX_LEN, 40)} <= lengths, lengths
        merged = next(c for c in cases if c[4] and c[7] is None and c[3] == 0)
        spans = merged[8][3][2]
        assert [CHUNK - 3, CHUNK + 3] in spans.tolist() and [2 * CHUNK - 1, 2 * CHUNK + 1] in spans.tolist()
        assert not merged[8][1][1] and (merged[8][0][1] == -1).all()          # the all-blank line


def test_more_symbols_than_the_largest_max_len(pa):
    """max_len 1024 filled to the last row: 1025 frames, none blank, none merged."""
    T = 4 * CHUNK + 1
    lab = (np.arange(T)[None, :] % 2 + 1) * np.ones((2, 1), np.int64)
    lab[1, 5] = 0
    case = make_case("full", one_hot(lab, 3), "ntc", 0, False, "value", MAX_LEN)
    assert case[8][1].tolist() == [T, T - 1] and (case[8][0] >= 0).all()
    run_case(pa, case)
    run_case(pa, make_case("full, merged", one_hot(lab, 3), "ntc", 0, True, "none", MAX_LEN))


# ---- special values -------------------------------------------------------------------------------------------------------------
def special_rows(C):
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(C)
    x = rng.integers(-2, 3, (12, C)).astype(F32)
    last, mid = C - 1, C // 2
    x[0, mid] = nan                                                           # NaN later than larger numbers
    x[0, 0] = 7
    x[1, [0, last]] = nan                                                     # NaN first, and again at the end
    x[2] = -inf                                                               # all -inf: class 0
    x[3, [mid, last]] = inf                                                   # +inf twice: the first
    x[4] = 0
    x[4, ::2] = -0.0                                                          # -0.0 and +0.0 tie: class 0 and its sign
    x[5] = -0.0
    x[5, 1::2] = 0.0
    x[6] = -inf
    x[6, [mid, last]] = 3                                                     # numbers among -inf: a finite confidence
    x[7, mid], x[7, last] = inf, nan                                          # a NaN behind +inf still wins
    x[8, 0], x[8, last] = -inf, -inf
    x[9] = nan
    x[10, last] = 9
    x[[8, 11], mid] = 8                                                       # (no row's label is class 1, the tests' blank)
    return x


@pytest.mark.parametrize("C", (4, 70, ROW_WAVE_MAX + 7))
def test_special_values_in_both_forms(pa, C):
    rows = special_rows(C)
    assert np.array_equal(R.frame_labels(rows), np.argmax(rows, -1))
    for confidence in MODES:
        for merge in (False, True):
            x = np.ascontiguousarray(rows.reshape(2, 6, C))
            run_case(pa, make_case("special", x, "ntc", blank=1, merge=merge, confidence=confidence, max_len=6), off=C % 3)
            x = np.ascontiguousarray(rows.reshape(2, 1, 6, C).transpose(0, 3, 1, 2))
            case = make_case("special", x, "nchw", blank=1, merge=merge, confidence=confidence, max_len=6)
            run_case(pa, case)
            if confidence == "softmax" and not merge:
                conf = case[8][2].reshape(12)
                assert np.isnan(conf[[0, 1, 2, 3, 7, 9]]).all() and np.isfinite(conf[[4, 5, 6, 8, 10]]).all()


# ---- confidence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (37, 257, ROW_WAVE_MAX + 1, 2000))
def test_softmax_confidence_inside_its_bound(pa, C):
    worst = {}
    for spread in (1.0, 8.0, 30.0):
        x = R.spread_rows(np.random.default_rng(int(C + spread)), 24, C, spread).reshape(2, 12, C)
        x[0, 0, ::3] = -np.inf                                                # classes at -inf add nothing
        for layout, xs in (("ntc", x), ("tnc", np.ascontiguousarray(x.transpose(1, 0, 2))),
                           ("nchw", np.ascontiguousarray(x.reshape(2, 1, 12, C).transpose(0, 3, 1, 2)))):
            case = make_case("confidence", xs, layout, blank=C - 1, merge=False, confidence="softmax", max_len=12)
            assert (case[8][1] >= 10).all()
            form = form_of(layout)
            worst[form] = max(worst.get(form, 0.0), run_case(pa, case, off=0 if layout == "nchw" else 3))
    print("softmax confidence, C = %d: worst err / tol rows %.3f, time %.3f" % (C, worst["rows"], worst["time"]))


def test_value_and_none_confidence(pa):
    x = R.spread_rows(np.random.default_rng(3), 20, 300, 8.0).reshape(4, 5, 300)
    for layout, xs in (("ntc", x), ("nchw", np.ascontiguousarray(x.reshape(4, 1, 5, 300).transpose(0, 3, 1, 2)))):
        case = make_case("value", xs, layout, blank=0, merge=False, confidence="value", max_len=5)
        assert np.array_equal(case[8][2].reshape(4, 5), x.max(-1))
        run_case(pa, case)
        case = make_case("none", xs, layout, blank=0, merge=False, confidence="none", max_len=5)
        assert not case[8][2].view(np.uint32).any() and case[8][1].all()
        run_case(pa, case)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(pa):
    ctx = pa.hip.context()
    lib = pa._lib.load()
    x = pa.hip.asarray(np.random.default_rng(1).integers(-2, 3, (2, 3, 7, 5)).astype(F32))    # 6 sequences of 7 frames, 5 classes
    lens = pa.hip.asarray(np.array([7, 0, 3, 9, 1, 7], I32))
    text, length, conf, spans = Framed(pa, 6 * 4), Framed(pa, 6), Framed(pa, 6 * 4), Framed(pa, 6 * 4 * 2)
    scratch = Framed(pa, 6 * 7 * 2)
    ok = dict(x=x.ptr, S_outer=2, S_inner=3, T=7, C=5, st_outer=105, st_inner=35, st_time=5, st_class=1, lengths=lens.ptr, blank=0, merge=1,
              confidence=1, max_len=4, scratch=scratch.ptr, text=text.ptr, length=length.ptr, conf=conf.ptr, spans=spans.ptr)
    bad = [(dict(x=None), EINVAL), (dict(scratch=None), EINVAL), (dict(text=None), EINVAL), (dict(length=None), EINVAL),
           (dict(conf=None), EINVAL), (dict(spans=None), EINVAL), (dict(S_outer=-1), EINVAL), (dict(S_inner=-1), EINVAL), (dict(T=-1), EINVAL),
           (dict(C=0), EINVAL), (dict(C=-4), EINVAL), (dict(blank=-1), EINVAL), (dict(blank=5), EINVAL), (dict(max_len=0), EINVAL),
           (dict(max_len=-2), EINVAL), (dict(confidence=3), EINVAL), (dict(confidence=-1), EINVAL),
           (dict(max_len=MAX_LEN + 1), EUNSUPPORTED), (dict(T=MAX_FRAMES + 1, S_outer=1, S_inner=1), EUNSUPPORTED),
           (dict(S_outer=1 << 11, S_inner=1 << 10, T=1 << 10, C=1), EUNSUPPORTED), (dict(S_outer=1 << 16, S_inner=1 << 15, T=0), EUNSUPPORTED),
           (dict(S_outer=1, S_inner=1, T=1 << 16, C=1 << 15, blank=0), EUNSUPPORTED)]
    for change, code in bad:
        args = dict(ok, **change)
        assert lib.pl_ctc_greedy_f32(ctx.handle, *args.values()) == code, change
        assert lib.pl_last_error(), change
    assert lib.pl_ctc_greedy_f32(None, *ok.values()) == EINVAL
    for change in (dict(S_outer=0), dict(S_inner=0), dict(S_outer=0, T=0)):     # nothing to do: PL_OK without a launch
        assert lib.pl_ctc_greedy_f32(ctx.handle, *dict(ok, **change).values()) == OK, change
    ctx.synchronize()
    assert all(f.untouched() for f in (text, length, conf, spans, scratch))
    # no frame: length = 0 and the filler rows, written; the scratch is not touched
    assert lib.pl_ctc_greedy_f32(ctx.handle, *dict(ok, T=0).values()) == OK
    t, ok_t = text.get(I32)
    n, ok_n = length.get(I32)
    c, ok_c = conf.get()
    s, ok_s = spans.get()
    assert ok_t and ok_n and ok_c and ok_s and (t == -1).all() and not n.any() and not c.any() and not s.any() and scratch.untouched()
    assert lib.pl_ctc_greedy_f32(ctx.handle, *ok.values()) == OK                # ... and the arguments they were derived from run
    assert length.get(I32)[0].any() and length.get(I32)[1]


# ---- hygiene, capture, the layouts ----------------------------------------------------------------------------------------------
def test_hygiene_pass_over_many_cases(pa):
    """util.ctc_decode with the pool in hygiene mode: fresh blocks are poisoned and guarded.  The confidences in softmax mode
    are compared as bits to the value- and none-mode cases only; the softmax cases take their labels, lengths and spans."""
    cases = [c for C in (3, 65, 257, 1025) for c in row_cases(C)] + [c for W in (1, 65, 130) for c in time_cases(W, 3)]
    cases += collapse_cases(CHUNK + 1)[::3]
    exact = [c for c in cases if c[5] != "softmax"]
    K.hygiene_pass(pa, exact, lambda x, layout, blank, merge, confidence, max_len, lengths: pa.util.ctc_decode(
        pa.hip.asarray(x), layout, blank, merge, confidence, max_len, lengths), NAMES, 15)
    soft = [c[:8] + ((c[8][0], c[8][1], c[8][3]),) for c in cases if c[5] == "softmax"]

    def without_conf(x, layout, blank, merge, confidence, max_len, lengths):
        text, length, conf, spans = pa.util.ctc_decode(pa.hip.asarray(x), layout, blank, merge, confidence, max_len,
                                                       None if lengths is None else pa.hip.asarray(np.asarray(lengths, I32).reshape(-1)))
        return text, length, spans

    K.hygiene_pass(pa, soft, without_conf, ("text", "length", "spans"), 8)


def test_chain_replays_from_a_captured_graph(pa):
    """No host wait and no host-computed value: the launches captured once answer for whatever is in their input at launch."""
    T, N, C, m = CHUNK + 9, 3, 70, 40
    rng = np.random.default_rng(8)
    inputs = [rng.integers(-2, 3, (T, N, C)).astype(F32), np.zeros((T, N, C), F32), one_hot(collapse_labels(T, C, 0, 30)[:3], C).transpose(1, 0, 2).copy()]
    x = pa.hip.empty((T, N, C), F32)
    outs = (pa.hip.empty((N, m), I32), pa.hip.empty((N,), I32), pa.hip.empty((N, m), F32), pa.hip.empty((N, m, 2), I32))
    scratch = pa.hip.empty((N * T,), np.int64)
    K.replay_from_captured_graph(
        pa, lambda: pa._lib.load().pl_ctc_greedy_f32(pa.hip.context().handle, x.ptr, N, 1, T, C, C, 0, N * C, 1, None, 0, 1, CONF["value"], m,
                                                     scratch.ptr, *[a.ptr for a in outs]),
        x, outs, inputs, lambda host: R.ctc_greedy(host, "tnc", 0, True, "value", m), NAMES)


def test_the_three_layouts_agree(pa):
    T, N, C = 70, 3, 41
    x = np.random.default_rng(12).integers(-2, 3, (T, N, C)).astype(F32)
    lengths = [70, 33, 0]
    views = {"tnc": x, "ntc": np.ascontiguousarray(x.transpose(1, 0, 2)), "nchw": np.ascontiguousarray(x.transpose(1, 2, 0)[:, :, None, :])}
    got = {}
    for layout, xs in views.items():
        case = make_case("layouts", xs, layout, blank=2, merge=True, confidence="value", max_len=32, lengths=lengths)
        run_case(pa, case)
        text, length, conf, spans = K.host(pa.util.ctc_decode(pa.hip.asarray(xs), layout, 2, True, "value", 32, lengths))
        got[layout] = (text.reshape(N, 32), length.reshape(N), conf.reshape(N, 32), spans.reshape(N, 32, 2))
    assert got["tnc"][1].tolist()[2] == 0 and got["tnc"][1][0] > got["tnc"][1][1] > 0
    for layout in ("ntc", "nchw"):
        K.same(got[layout], got["tnc"], NAMES, layout + " against tnc")
    assert pa.util.ctc_decode(pa.hip.asarray(views["nchw"]), "nchw")[0].shape == (N, 1, 64)
    # no frame, no sequence: the filler rows without a launch
    text, length, conf, spans = K.host(pa.util.ctc_decode(pa.hip.empty((0, 3, 5), F32), max_len=3))
    assert (text == -1).all() and text.shape == (3, 3) and not length.any() and not conf.view(np.uint32).any() and not spans.any()
    assert pa.util.ctc_decode(pa.hip.empty((4, 0, 5), F32))[3].shape == (0, 64, 2)
