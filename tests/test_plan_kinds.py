"""plan.KINDS, the one table of what a kind does to its operands: the lists the passes use are read off it and hold what they
held when each was a literal of its own, and every kind a plan can hold has a row -- so a kind added without saying whether it
writes in place fails here, on the host."""
import ast
import os

from planer_amd import plan
from planer_amd.layer import layer_map

try:
    from planer_amd import q4
except Exception:                      # no built library on this host: q4.register is read as source below
    q4 = None

# the lists as they stood before the table
BEFORE = {
    "_IN_PLACE": ("relu", "relu_q4", "clip", "clip_q4", "erf", "instancenormalization", "instancenormalization_q4", "groupnorm",
                  "groupnorm_q4"),
    "_PURE_READERS": ("conv_q4", "convt_q4", "wino4_in", "wino4_gemm", "wino4_out", "wino4_chain", "wino43_in", "wino43_gemm",
                      "wino43_out", "wino43_chain", "conv1x1_wino_in", "conv_q4_pair", "add_q4", "maxpool_q4", "averagepool_q4",
                      "gap_q4", "upsample_q4", "concat_q4", "upconcat_q4", "batchnorm_q4", "leakyrelu_q4", "sigmoid_q4", "from_q4",
                      "pad_q4", "refold_q4", "resize_q4", "upsample_add_q4", "resize_add_q4", "pixelshuffle_q4"),
    "_FOLD_POINTWISE": ("relu_q4", "leakyrelu_q4", "clip_q4", "sigmoid_q4", "batchnorm_q4", "add_q4", "concat_q4"),
    "_FOLD_IN_PLACE": ("relu_q4", "clip_q4", "instancenormalization_q4"),
    "Q4_POINTWISE": ("maxpool", "averagepool", "gap", "upsample", "batchnorm", "relu", "leakyrelu", "sigmoid", "add", "concat",
                     "clip", "instancenormalization", "pad", "resize", "pixelshuffle", "groupnorm"),
    "INSTNORM_Q4_KINDS": ("instancenormalization", "pad"),
    "LINEAR_Q4_KINDS": ("resize",),
}


def _registered_kinds():
    """The plan-internal kinds q4.register adds to a layer map -- by calling it, or from its source where q4 does not import."""
    if q4 is not None:
        added = {}
        q4.register(added)
        return set(added)
    with open(os.path.join(os.path.dirname(plan.__file__), "q4.py")) as f:
        tree = ast.parse(f.read())
    register = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "register")
    literal = next(n for n in ast.walk(register) if isinstance(n, ast.Dict))
    return {k.value for k in literal.keys} | {k + "_q4" for k in plan.Q4_POINTWISE}


def test_the_derived_lists_hold_what_the_literals_held():
    for name, before in BEFORE.items():
        got = getattr(plan, name)
        assert isinstance(got, tuple) and len(got) == len(set(got)), name
        assert set(got) == set(before), name
    assert plan.Q4_POINTWISE == BEFORE["Q4_POINTWISE"]            # q4_pointwise_kinds() hands this order out


def test_every_kind_a_plan_can_hold_has_a_row():
    kinds = set(layer_map) | _registered_kinds()
    assert {"conv_q4", "wino43_chain", "groupnorm_q4"} <= kinds    # (the plan-internal kinds were found)
    assert kinds - set(plan.KINDS) == set()
    assert set(plan.KINDS) - kinds == set()                       # and no row for a kind that does not exist


def test_rows_are_consistent():
    traits = {plan.W, plan.R, plan.F, plan.Q, plan.QI, plan.QL}
    for kind, row in plan.KINDS.items():
        assert set(row) <= traits and len(row) == len(set(row)), kind
        assert not (plan.W in row and plan.R in row), kind        # a kind that rewrites its input is no pure reader
        if kind in plan.Q4_POINTWISE:
            assert kind + "_q4" in plan.KINDS, kind


def test_q4_layers_are_the_kinds_with_a_q4_form():
    if q4 is not None:
        assert set(q4.Q4_LAYERS) == set(plan.Q4_POINTWISE)
    else:
        assert {k + "_q4" for k in plan.Q4_POINTWISE} <= set(plan.KINDS)
