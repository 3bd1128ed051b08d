"""pl_topk_select_f32 without a GPU: the routing rule with its three switch values, the Python mirror of the
scratch size against the header's macro, the declaration and the export."""
import re
import subprocess

import pytest

from planer_amd import _lib, layer, util
from tests.test_abi import HEADER, _built, header_functions

BIG = 1 << 31
# rows, n, inner, k, largest -> eligible with the switch unset, "0", "force"
TABLE = [
    ((1, 16385, 1, 2, 1), (True, False, True)),
    ((8, 25200, 1, 1024, 1), (True, False, True)),
    ((21, 65537, 7, 4096, 1), (True, False, True)),
    ((1, 16385, 1, 1, 1), (False, False, True)),            # one selection round is already one pass
    ((1, 16384, 1, 1, 1), (True, False, True)),             # ... the LDS sort is not
    ((8, 10647, 1, 1024, 1), (True, False, True)),
    ((1, 4096, 1, 4096, 1), (True, False, True)),
    ((1, 4095, 1, 300, 1), (False, False, True)),           # short rows stay with the one-launch sort by default
    ((300, 10, 1, 10, 1), (False, False, True)),
    ((1, 20000, 1, 4097, 1), (False, False, False)),        # above PL_TOPK_SELECT_MAX_K
    ((1, 20000, 1, 0, 1), (False, False, False)),
    ((1, 20000, 1, 300, 0), (False, False, False)),         # largest = 0 stays with pl_topk_f32
    ((3, 100, 1, 101, 1), (False, False, False)),
    ((BIG, 1, 1, 1, 1), (False, False, False)),
    ((1 << 11, 1 << 20, 1, 5, 1), (False, False, False)),   # 2^31 elements
    ((0, 20000, 1, 5, 1), (False, False, False)),
]


@pytest.mark.parametrize("switch, column", [(None, 0), ("0", 1), ("force", 2), ("1", 0)])
def test_eligibility_table(monkeypatch, switch, column):
    if switch is None:
        monkeypatch.delenv("PLANER_HIP_TOPK_SELECT", raising=False)
    else:
        monkeypatch.setenv("PLANER_HIP_TOPK_SELECT", switch)
    assert layer.topk_select_enabled() is (switch != "0")
    for args, want in TABLE:
        assert layer.topk_select_eligible(*args) is want[column], (args, switch)


def test_scratch_size_is_the_headers_macro():
    text = open(HEADER).read().replace("\\\n", " ")
    consts = {k: int(v) for k, v in re.findall(r"#define (PL_TOPK_SELECT_[A-Z_]+) (\d+)", text)}
    assert consts == dict(PL_TOPK_SELECT_CHUNK=_lib.TOPK_SELECT_CHUNK, PL_TOPK_SELECT_MAX_K=_lib.TOPK_SELECT_MAX_K,
                          PL_TOPK_SELECT_HIST_WORDS=_lib.TOPK_SELECT_HIST_WORDS)
    body = re.search(r"#define PL_TOPK_SELECT_SCRATCH_BYTES\(rows, n, k\)\s+(.*)", text).group(1)
    macro = eval("lambda rows, n, k: " + body.replace("(size_t)", "").replace("/", "//"), dict(consts))
    for (rows, n, _, k, _), _ in TABLE:
        assert util._topk_select_scratch_bytes(rows, n, max(k, 0)) == macro(rows, n, max(k, 0)), (rows, n, k)
    c = _lib.TOPK_SELECT_CHUNK
    assert util._topk_select_scratch_bytes(1, c, 1) + 4 == util._topk_select_scratch_bytes(1, c + 1, 1)
    assert util._topk_select_scratch_bytes(3, 2 * c, 7) == 3 * (7 * 8 + 5120 * 4 + 4 + 2 * 4)


def test_declared_with_a_signature_and_a_thunk():
    assert "pl_topk_select_f32" in header_functions() and len(_lib.SIGNATURES["pl_topk_select_f32"]) == 9
    proto = re.search(r"\bint pl_topk_select_f32\(([^;]*)\);", open(HEADER).read()).group(1)
    assert [p.strip().split()[-1].lstrip("*") for p in proto.split(",")] == ["ctx", "x", "outer", "n", "inner", "k", "scratch", "values", "indices"]
    inc = open(HEADER.replace("include/planer_hip.h", "planer_amd/csrc/plan_dispatch.inc")).read()
    assert '{"pl_topk_select_f32", 9, &thunk_pl_topk_select_f32}' in inc


@pytest.mark.skipif(not _built(), reason="libplaner_hip.so not built")
def test_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT pl_topk_select_f32$", out, flags=re.M)
