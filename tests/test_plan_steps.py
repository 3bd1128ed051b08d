"""plan.Steps, the view every pass takes of a program: steps one layer each, readers and writers, the two predicates that make
moving a read sound, and the shared epilogue."""
from planer_amd.plan import Steps

BODY = [["c", "conv", {}], ["b", "batchnorm", {}], ["r", "relu", {}], ["s", "sigmoid", {}], ["a", "add", {}], ["sp", "split", {}]]
FLOW = [[["x", "K"], ["c", "b"], "y"],          # a chained step: c writes y, b reads y and writes y
        ["x", "r", "x2"],                       # in place on x
        [["y", "y"], ["a"], "z"],               # reads y twice
        ["z", ["sp"], ["p", "q"]],
        ["p", ["s"], "x"]]                      # writes x again


def test_steps_readers_and_writers():
    v = Steps(BODY, FLOW)
    assert v.steps == [[["x", "K"], "c", "y"], [["y"], "b", "y"], [["x"], "r", "x2"], [["y", "y"], "a", "z"],
                       [["z"], "sp", ["p", "q"]], [["p"], "s", "x"]]
    assert v.readers == {"x": [0, 2], "K": [0], "y": [1, 3], "z": [4], "p": [5]}            # each reading step once
    assert v.writers == {"y": [0, 1], "x2": [2], "x": [5], "z": [3], "p": [4], "q": [4]}
    assert [v.kind(i) for i in range(6)] == ["conv", "batchnorm", "relu", "add", "split", "sigmoid"]
    assert v.step(3) == (["y", "y"], "a", "add", {}, "z") and v.each()[3] == v.step(3)


def test_only_reader():
    v = Steps(BODY, FLOW)
    assert v.only_reader(3, "z") == 4
    assert v.only_reader(4, "z") is None            # the reader does not come later
    assert v.only_reader(0, "y") is None            # two writers, two readers
    assert v.only_reader(4, "p") == 5
    assert v.only_reader(4, "q") is None            # no reader
    assert v.only_reader(4, ["p", "q"]) is None     # not one tensor


def test_clobbered_and_its_rules():
    v = Steps(BODY, FLOW)
    assert v.clobbers(2, "x") and not v.clobbers(0, "x")                 # relu rewrites x; conv only reads it
    assert v.clobbers(5, "x") and not v.clobbers(5, "x", writes=False)   # sigmoid writes x
    assert v.clobbers(0, "x", in_place=None, writes=False)               # any reader
    assert not v.clobbers(2, "x", in_place=(), writes=False)
    assert v.clobbered("x", 0, 4) and not v.clobbered("x", 2, 5)         # strictly between
    assert not v.clobbered("x", 0, 4, skip=(2,))
    assert not v.clobbered("x", 0, 5, in_place=()) and v.clobbered("x", 0, 6, in_place=())
    assert v.clobbered("p", 0, 6) and not v.clobbered("q", 4, 6)         # one of several outputs


def test_spliced_and_emit():
    v = Steps(BODY + [["r2", "relu", {}]], FLOW + [["x", ["r"], "x"]])
    out = v.spliced({1: (["x", "K"], "c+", "conv_fused", {"act": 0}, "y")}, dropped=(0, 1, 2))
    body, flow = v.emit(out)
    assert flow == [[["x", "K"], ["c+"], "y"], [["y", "y"], ["a"], "z"], [["z"], ["sp"], ["p", "q"]], [["p"], ["s"], "x"],
                    [["x"], ["r"], "x"]]
    # each layer once, in the order of first use; layers no step uses are gone
    assert body == [["c+", "conv_fused", {"act": 0}], ["a", "add", {}], ["sp", "split", {}], ["s", "sigmoid", {}], ["r", "relu", {}]]
