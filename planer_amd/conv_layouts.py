"""Convolution filter layouts: the one table of `w_layout` codes.

A conv step's `w_layout` says how its filter was prepared and which kernel runs it.  The codes are a persisted format
(planer_amd/tuned/*.algo.json stores picks by code, run reports print them, PLANER_HIP_CONV_ALGO forces one), so their
values never change.  Every other module asks this one: what a code is called, its filter-key suffix, the function that
prepares its filter, when it applies, and which code a conv step gets (`choose`).  DESIGN.md section 4.
"""
import collections
import ctypes
import os

from . import _lib
from .hip import _f32, empty

IGEMM_NCHW, TAP_NCHW, DIRECT_Q4, WINO2_NCHW, WINO2_Q4 = 0, 1, 2, 3, 4
ROWPACK_Q4, WINO4_Q4, W1D4_Q4, WF4_Q4, STEM_POOL, WINO43_Q4, STEM_POOL_NCHW, DW_Q4, CONVT_Q4 = 6, 7, 8, 9, 10, 11, 12, 13, 14


# ---- filter packing ------------------------------------------------------------------------------------------------------
def _packer(name, dims, check=None, count=None, elems=None, same_1x1=False):
    """-> prepare(K, ...): the filter in the layout pl_conv2d_prepare_<name>_f32(ctx, K, *dims(K.shape, ...), out) writes,
    made once per model.  The allocation holds pl_conv2d_<elems or name>_filter_elems(*dims) floats, or `count(K.shape)`
    without a query; the returned array keeps the logical shape of K.  `check(K.shape)` raises ValueError on filters the
    layout cannot hold; `same_1x1`: a 1x1 filter is the same in this layout and is returned as is."""
    def prepare(K, *args, **kw):
        _f32(K)
        if check is not None:
            check(K.shape)
        if same_1x1 and K.shape[2] * K.shape[3] == 1:
            return K
        d = dims(K.shape, *args, **kw)
        if count is None:
            n = ctypes.c_size_t()
            _lib.call("pl_conv2d_%s_filter_elems" % (elems or name), *d, ctypes.byref(n))
        out = empty((count(K.shape) if count is not None else n.value,), ctx=K.ctx)
        _lib.call("pl_conv2d_prepare_%s_f32" % name, K.ctx.handle, K.ptr, *d, out.ptr)
        out.shape = K.shape
        return out
    return prepare


def _oihw(s, **_):
    return s[0], s[1], s[2], s[3]


def _cout_cin(s, **_):
    return s[0], s[1]


def _refuse(test, msg):
    def check(s):
        if not test(*s):
            raise ValueError(msg)
    return check


_wino_check = _refuse(lambda cout, cin, kh, kw: (kh, kw) == (3, 3) and cin % 4 == 0 and cout % 4 == 0,
                      "winograd Q4 filters need 3x3 kernels, Cin % 4 == 0 and Cout % 4 == 0")

# OIHW -> tap-major [Cout][kh*kw][Cin/g] (the bytes permuted; 1x1 filters are the same in both layouts)
prepare_conv_weights = _packer("weights", _oihw, _refuse(lambda co, ci, kh, kw: ci % 16 == 0, "tap-major filters need Cin/group % 16 == 0"),
                               count=lambda s: s[0] * s[1] * s[2] * s[3], same_1x1=True)
# OIHW 3x3 -> Winograd F(2x2,3x3) domain U[16][Cout][Cin]
prepare_winograd_weights = _packer("winograd", _cout_cin, _refuse(lambda co, ci, kh, kw: (kh, kw) == (3, 3) and ci % 16 == 0,
                                                                  "winograd filters need 3x3 kernels and Cin % 16 == 0"),
                                   count=lambda s: 16 * s[0] * s[1])
# OIHW -> wq[group][tap*ceil(Cin_g/4) + cin/4][Cout/group][4] (zero padded)
prepare_q4_weights = _packer("q4", lambda s, group=1, **_: (s[0], s[1], s[2], s[3], int(group)))
# OIHW 3x3 -> Winograd-domain Q4 filters [16][k-quad][Cout][4]
prepare_winograd_q4_weights = _packer("winograd_q4", _cout_cin, _wino_check)
# OIHW with Cin < 4 -> row-packed [kh*ceil(kw*Cin/4)][Cout][4]
prepare_rowpack_weights = _packer("rowpack", _oihw)
# OIHW 3x3 -> Winograd F(4x4,3x3) Q4 filters [36][k-quad][Cout][4]
prepare_winograd4_q4_weights = _packer("winograd4_q4", _cout_cin, _wino_check)
# OIHW 3x3 -> fused 1-D Winograd F(4,3) filters [6][row*Cin/4 + cin/4][Cout][4]
prepare_w1d4_q4_weights = _packer("w1d4_q4", _cout_cin, _refuse(lambda co, ci, kh, kw: (kh, kw) == (3, 3) and ci % 4 == 0,
                                                                "1-D winograd filters need 3x3 kernels and Cin % 4 == 0"))
# OIHW 3x3 -> fully fused F(4x4,3x3) filters [Cout/64][Cin/4][4 blocks of 16 channels][9 groups of 4 frequencies][4 k x 16 channels][4]
prepare_wf4_q4_weights = _packer("wf4", _cout_cin, _wino_check)
# OIHW 3x3 -> mixed-tile Winograd filters [121][k-quad][Cout][4]
prepare_winograd43_q4_weights = _packer("winograd43_q4", _cout_cin, _wino_check)
# OIHW stem filters [Cout][3][7][7] -> [48][Cout][4] in the k order of the stem + max-pool kernel that reads the NCHW input
prepare_stem_nchw_weights = _packer("stem_nchw", lambda s, **_: (s[0],),
                                    _refuse(lambda co, ci, kh, kw: (ci, kh, kw) == (3, 7, 7), "the NCHW stem kernel takes [Cout][3][7][7] filters"))
# OIHW stem filters [Cout][3][7][7] -> G g of the polyphase F(4,4) form of that kernel, [7][11][Cout][4] (csrc/conv_stem_wino_kernel.h).
# The form has no w_layout code of its own: q4.ConvPoolQ4 runs it on w_layout 12 with wino=44 (STEM_WINO), or where the step's
# filter carries one (q4.attach_stem_wino)
prepare_stem_wino_weights = _packer("stem_wino", lambda s, **_: (s[0],),
                                    _refuse(lambda co, ci, kh, kw: (ci, kh, kw) == (3, 7, 7), "the F(4,4) stem kernel takes [Cout][3][7][7] filters"))
STEM_WINO = 44
# OIHW depthwise filters [C][1][kh][kw] -> [ceil(C/4)][kh*kw][4] with zero-padded quads
prepare_dw_q4_weights = _packer("dw_q4", lambda s, **_: (s[0], s[2], s[3]),
                                _refuse(lambda c, ci, kh, kw: ci == 1, "depthwise filters have one input channel per group"),
                                count=lambda s: (s[0] + 3) // 4 * s[2] * s[3] * 4)
# ConvTranspose filters [Cin][Cout][kh][kw] -> one stride-1 sub-filter per output phase in the channel-quad form; the packing
# depends on the strides
prepare_convt_weights = _packer("convt_q4", lambda s, strides=(2, 2), **_: (s[0], s[1], s[2], s[3], int(strides[0]), int(strides[1])),
                                elems="convt")


# ---- where each layout applies -------------------------------------------------------------------------------------------
def _conv3x3_s1(k_shape, group, strides, dilations, pads):
    """3x3 / stride 1 / pad 1 / no dilation / no groups."""
    return (k_shape[2] == 3 and k_shape[3] == 3 and group == 1 and list(strides) == [1, 1] and list(dilations) == [1, 1]
            and list(pads) == [1, 1, 1, 1])


def _symmetric(pads):
    pads = list(pads)
    return len(pads) == 4 and pads[0] == pads[2] and pads[1] == pads[3]


def q4_conv_eligible(k_shape, group=1, **_):
    """The direct channel-quad kernel: groups that do not split a channel quad."""
    cout, cin_g = k_shape[0], k_shape[1]
    return len(k_shape) == 4 and (group == 1 or (cin_g % 4 == 0 and (cout // group) % 4 == 0))


def winograd_eligible(k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """NCHW F(2x2,3x3): 3x3 / stride 1 / pad 1 / no dilation / no groups, Cin % 16 == 0."""
    return k_shape[1] % 16 == 0 and _conv3x3_s1(k_shape, group, strides, dilations, pads)


def w1d_q4_eligible(k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """Fused 1-D F(4,3): 3x3 / stride 1 / pad 1 / no dilation / no groups, Cin % 4 == 0."""
    return k_shape[1] % 4 == 0 and _conv3x3_s1(k_shape, group, strides, dilations, pads)


def winograd_q4_eligible(k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """3x3 / stride 1 / pad 1 / no dilation / no groups, Cin and Cout multiples of 4."""
    return k_shape[0] % 4 == 0 and w1d_q4_eligible(k_shape, group, strides, dilations, pads)


def winograd43_eligible(x_shape, k_shape, min_columns=0, **para):
    """Mixed-tile Winograd (csrc/wino43_kernels.h): a 3x3 / stride 1 / pad 1 / group 1 conv on a map whose sides are 7, 14 or 21.
    `min_columns`: the plan compiler only offers it where each of the 121 per-frequency GEMMs has that many tile columns
    (N * (H / 7) * (W / 7)): its filters are 3.4x those of F(4x4,3x3), and with few columns per filter the GEMM lives on filter
    bandwidth -- ResNet-18's layer4 at batch 32 (32 columns, 127 MB of filters per conv) wins 4 us per conv in isolation and
    loses 2 % of the pipelined rate, layer3 (128 columns) wins both ways."""
    return (len(x_shape) == 4 and x_shape[2] in (7, 14, 21) and x_shape[3] in (7, 14, 21) and winograd_q4_eligible(k_shape, **para)
            and x_shape[0] * (x_shape[2] // 7) * (x_shape[3] // 7) >= min_columns)


def rowpack_eligible(k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """Convs on 1..3 input channels (the stem): group 1, no dilation, symmetric pads."""
    return group == 1 and k_shape[1] < 4 and list(dilations) == [1, 1] and _symmetric(pads)


def dw_q4_eligible(k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """Depthwise conv with channel multiplier 1 (group == Cin == Cout, OIHW filter [C][1][kh][kw]), kh / kw up to 7, symmetric
    pads: the VALU kernel of csrc/conv_dw_kernel.h.  Any stride and dilation."""
    return (len(k_shape) == 4 and k_shape[1] == 1 and k_shape[0] == group and 1 <= k_shape[2] <= 7 and 1 <= k_shape[3] <= 7
            and (len(list(pads)) != 4 or _symmetric(pads)))


def convt_phase_eligible(k_shape, group=1, strides=(2, 2), dilations=(1, 1), pads=(0, 0, 0, 0), output_padding=(0, 0), **_):
    """A transposed conv the phase-decomposed kernel runs (pl_conv2d_convt_q4_f32): 4-D filter [Cin][Cout][kh][kw], group 1,
    dilation 1, pads within the kernel reach.  Any stride, kh != kw, asymmetric pads and output_padding."""
    if len(k_shape) != 4 or int(group) != 1 or [int(d) for d in dilations] != [1, 1] or len(list(pads)) != 4:
        return False
    kh, kw = k_shape[2:]
    p, op = [int(v) for v in pads], [int(v) for v in output_padding]
    return min(int(s) for s in strides) >= 1 and min(kh - 1 - p[0], kh - 1 - p[2] + op[0], kw - 1 - p[1], kw - 1 - p[3] + op[1]) >= 0


def _supported(entry, x_shape, k_shape, strides, pads):
    cout, cin, kh, kw = k_shape
    ok = ctypes.c_int()
    _lib.call(entry, int(cin), int(x_shape[2]), int(x_shape[3]), int(cout), int(kh), int(kw),
              int(strides[0]), int(strides[1]), int(pads[0]), int(pads[1]), ctypes.byref(ok))
    return bool(ok.value)


def stem_pool_eligible(x_shape, k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """Whether the row-packed conv + maxpool(3x3 / s2 / p1) kernel (csrc/conv_stem_pool_kernel.h) takes this conv."""
    if len(x_shape) != 4 or int(group) != 1 or list(dilations) != [1, 1] or not _symmetric(pads):
        return False
    return _supported("pl_conv2d_rowpacked_pool_supported", x_shape, k_shape, strides, pads) and x_shape[1] == k_shape[1]


def stem_pool_nchw_eligible(x_shape, k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """Whether the stem + max-pool kernel can read this NCHW input itself (W % 4 == 0 on top of stem_pool_eligible)."""
    return (stem_pool_eligible(x_shape, k_shape, group, strides, dilations, pads)
            and _supported("pl_conv2d_stem_pool_nchw_supported", x_shape, k_shape, strides, pads))


def stem_pool_wino_eligible(x_shape, k_shape, group=1, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), **_):
    """Whether the polyphase F(4,4) form of the NCHW stem + max-pool kernel takes this conv (csrc/conv_stem_wino_kernel.h).
    PLANER_HIP_EXPERIMENT=stem_wino=0 or 1 switches the pick (Net's `stem_pool` callback)."""
    return (stem_pool_nchw_eligible(x_shape, k_shape, group, strides, dilations, pads)
            and _supported("pl_conv2d_stem_pool_wino_supported", x_shape, k_shape, strides, pads))


def experiment(key, default):
    """PLANER_HIP_EXPERIMENT="key=value,key=value" as the native code reads it (csrc/common.h pl_experiment)."""
    for item in os.environ.get("PLANER_HIP_EXPERIMENT", "").split(","):
        k, _, v = item.partition("=")
        if k.strip() == key:
            try:
                return int(v)
            except ValueError:
                return default
    return default


# ---- the table -----------------------------------------------------------------------------------------------------------
# name: what run reports print.  suffix: appended to the filter's init name to key the prepared copy (formatted with the conv's
# `group` and `strides`).  prepare(K, **para).  eligible(k_shape, x_shape, **para).  kernel: the ConvQ4 entry of the codes
# that share one signature.  staged: the stage-kind prefix of a Winograd conv the plan runs as explicit stages
# (plan.chain_winograd).  switch: the environment variable that takes a timed candidate out (=0).
Layout = collections.namedtuple("Layout", "name suffix prepare eligible kernel staged switch", defaults=(None,) * 6)

LAYOUTS = {
    IGEMM_NCHW: Layout("igemm-nchw"),
    TAP_NCHW: Layout("tap-nchw", "@tap", prepare_conv_weights, lambda k, x=None, **p: k[1] % 16 == 0),
    DIRECT_Q4: Layout("direct-q4 (conv_q4_kernel)", "@q4g%(group)d", prepare_q4_weights, lambda k, x=None, **p: q4_conv_eligible(k, **p)),
    WINO2_NCHW: Layout("wino2x2-nchw", "@wino", prepare_winograd_weights, lambda k, x=None, **p: winograd_eligible(k, **p)),
    WINO2_Q4: Layout("wino2x2-q4 (transforms + grouped conv_q4_kernel)", "@winoq4", prepare_winograd_q4_weights,
                     lambda k, x=None, **p: winograd_q4_eligible(k, **p), kernel="pl_conv2d_winograd_q4_f32"),
    ROWPACK_Q4: Layout("rowpack-q4 (nchw_to_rowpack + conv_q4_kernel)", "@rowpack", prepare_rowpack_weights,
                       lambda k, x=None, **p: rowpack_eligible(k, **p)),
    WINO4_Q4: Layout("wino4x4-q4 (transforms + grouped conv_q4_kernel)", "@wino4q4", prepare_winograd4_q4_weights,
                     lambda k, x=None, **p: winograd_q4_eligible(k, **p), "pl_conv2d_winograd4_q4_f32", "wino4", "PLANER_HIP_WINOGRAD4"),
    W1D4_Q4: Layout("w1d4 F(4,3) (conv_w1d4_kernel)", "@w1d4q4", prepare_w1d4_q4_weights, lambda k, x=None, **p: w1d_q4_eligible(k, **p),
                    "pl_conv2d_w1d4_q4_f32"),
    WF4_Q4: Layout("wf4 fused F(4x4,3x3) (conv_wf4_kernel)", "@wf4q4", prepare_wf4_q4_weights, lambda k, x=None, **p: winograd_q4_eligible(k, **p),
                   "pl_conv2d_wf4_q4_f32", switch="PLANER_HIP_WF4"),
    STEM_POOL: Layout("stem + maxpool (conv_stem_pool_kernel)", "@rowpack", prepare_rowpack_weights,
                      lambda k, x=None, **p: x is not None and stem_pool_eligible(x, k, **p)),
    WINO43_Q4: Layout("wino43-q4 (mixed F(4,3) x F(3,3) tiles: transforms + 121 grouped conv_q4_kernel)", "@wino43q4",
                      prepare_winograd43_q4_weights, lambda k, x=None, **p: x is not None and winograd43_eligible(x, k, **p),
                      "pl_conv2d_winograd43_q4_f32", "wino43", "PLANER_HIP_WINOGRAD43"),
    # (the kernel reads the NCHW batch itself)
    STEM_POOL_NCHW: Layout("stem + maxpool (conv_stem_pool_kernel)", "@stemnchw", prepare_stem_nchw_weights,
                           lambda k, x=None, **p: x is not None and stem_pool_nchw_eligible(x, k, **p)),
    DW_Q4: Layout("depthwise-q4 (conv_dw_kernel)", "@dwq4", prepare_dw_q4_weights, lambda k, x=None, **p: dw_q4_eligible(k, **p)),
    CONVT_Q4: Layout("convt-q4 (phase-decomposed convt_q4_kernel)", "@convt%(sh)dx%(sw)d", prepare_convt_weights,
                     lambda k, x=None, **p: convt_phase_eligible(k, **p)),
}
# w_layout -> stage-kind prefix (plan.chain_winograd): staged F(4x4,3x3), and the mixed-tile form for maps of 7 / 14 / 21 a side
STAGED_LAYOUTS = {code: lay.staged for code, lay in LAYOUTS.items() if lay.staged}

# what Net._pick_conv_algo times, in order: the first candidate is the fallback and wins ties.  Direct, fused 1-D F(4,3) along W,
# 2-D Winograd pipelines with separate transform kernels, fully fused F(4x4,3x3), mixed F(4,3) x F(3,3) tiles (staged).
Q4_CANDIDATES = (DIRECT_Q4, W1D4_Q4, WINO2_Q4, WINO4_Q4, WF4_Q4, WINO43_Q4)
NCHW_CANDIDATES = (TAP_NCHW, WINO2_NCHW)
# the mixed-tile form is offered where each per-frequency GEMM has this many tile columns (winograd43_eligible)
WINO43_MIN_COLUMNS = 64
CONV_KINDS, CONVT_KINDS = ("conv", "conv_fused"), ("convt_q4", "convt_fused", "convtranspose")


def conv_para(para):
    """The geometry of a conv step's parameters (what the predicates take)."""
    return {k: v for k, v in para.items() if k in ("group", "strides", "dilations", "pads")}


def suffix(code, para):
    """The filter-key suffix of `code` for a conv with these parameters."""
    strides = para.get("strides", (2, 2))
    return LAYOUTS[code].suffix % {"group": int(para.get("group", 1)), "sh": int(strides[0]), "sw": int(strides[1])}


def candidates(q4, k_shape, para, x_shape):
    """The w_layouts a conv can be timed on, in the order of Q4_CANDIDATES / NCHW_CANDIDATES.  The first is the step's own
    (its kind chose it) and is always there."""
    order, geo = (Q4_CANDIDATES if q4 else NCHW_CANDIDATES), conv_para(para)
    x_shape = tuple(x_shape) if x_shape is not None else None
    return [order[0]] + [c for c in order[1:] if os.environ.get(LAYOUTS[c].switch or "", "1") != "0"
                        and LAYOUTS[c].eligible(k_shape, x_shape, min_columns=WINO43_MIN_COLUMNS, **geo)]


def choose(kind, k_shape, para, x_shape, rowpack, pick):
    """-> (w_layout, filter-key suffix) of a conv step of `kind` on a filter of shape `k_shape`, or None where the step keeps its
    filter as it is.  conv_q4: the row-packed stem (`rowpack`: the plan feeds it the NCHW input), depthwise, else the Q4
    candidates.  conv / conv_fused: the NCHW candidates.  Transposed convs: the phase-decomposed packing.  Where more than one
    candidate applies and the input shape `x_shape` is known, `pick(candidates)` chooses (Net._pick_conv_algo times them;
    PLANER_HIP_WINOGRAD=0 keeps the first)."""
    geo = conv_para(para)
    if kind in CONVT_KINDS:
        code = CONVT_Q4 if convt_phase_eligible(k_shape, **para) else None
    elif kind == "conv_q4" and rowpack and rowpack_eligible(k_shape, **geo):
        code = ROWPACK_Q4
    elif kind == "conv_q4" and dw_q4_eligible(k_shape, **geo):
        code = DW_Q4
    elif kind == "conv_q4" or (kind in CONV_KINDS and len(k_shape) == 4 and LAYOUTS[TAP_NCHW].eligible(k_shape)):
        cands = candidates(kind == "conv_q4", k_shape, para, x_shape)
        code = cands[0]
        if len(cands) > 1 and x_shape is not None and os.environ.get("PLANER_HIP_WINOGRAD", "1") != "0":
            code = pick(cands)
    else:
        code = None
    return None if code is None else (code, suffix(code, para))
