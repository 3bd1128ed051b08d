"""pl_lstm_seq_f32 without a GPU: the entry is declared in the header, the ctypes table and the plan dispatch table
with one argument count, layer.LSTM's eligibility rule and switch, and the (step, slot) -> time index map the kernel runs."""
import os
import re

import pytest

from tests.conftest import ROOT

NARGS = 14      # ctx, gates_x0, gates_x1, R, bias, h0, c0, Y, c, L, N, H, ndir, sign0


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_signature_table_and_dispatch_agree():
    from planer_amd import _lib
    m = re.search(r"\nint pl_lstm_seq_f32\(([^;]*)\);", _read("include", "planer_hip.h"))
    assert m, "include/planer_hip.h does not declare pl_lstm_seq_f32"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == NARGS
    assert params[0] == "pl_ctx *ctx" and [p.split()[-1].lstrip("*") for p in params[1:]] == [
        "gates_x0", "gates_x1", "R", "bias", "h0", "c0", "Y", "c", "L", "N", "H", "ndir", "sign0"]
    sig = _lib.SIGNATURES["pl_lstm_seq_f32"]
    assert len(sig) == NARGS
    assert sig[:9] == [_lib.c_void_p] * 9 and sig[9:] == [_lib.c_int] * 5
    # pointers in the header where the table has pointers
    assert [("*" in p) for p in params] == [t is _lib.c_void_p for t in sig]


def test_plan_dispatch_has_the_thunk():
    inc = _read("planer_amd", "csrc", "plan_dispatch.inc")
    assert "static int thunk_pl_lstm_seq_f32(const PlArg *a) {" in inc
    assert '{"pl_lstm_seq_f32", %d, &thunk_pl_lstm_seq_f32},' % NARGS in inc
    call = re.search(r"&pl_lstm_seq_f32\)\((.*)\);", inc).group(1)
    assert call.count("(void *)a[") == 9 and call.count("(int)a[") == 5


def test_both_kernels_call_the_shared_tile():
    """dense_small_kernel and the fused step take their K loop and four-wave sum from dense_tile.h."""
    direct, step = _read("planer_amd", "csrc", "conv_direct.hip"), _read("planer_amd", "csrc", "lstm_kernel.h")
    body = direct.split("void __launch_bounds__(256) dense_small_kernel(")[1].split('extern "C"')[0]
    for text in (body, step):
        assert "dense_tile_kloop(" in text and "dense_tile_sum(" in text


@pytest.mark.parametrize("H, ok", [(0, False), (4, False), (8, True), (12, False), (64, True), (72, True)])
@pytest.mark.parametrize("L", [0, 1])
def test_eligibility_truth_table(H, ok, L):
    from planer_amd.layer import lstm_fused_eligible
    for ndir in (1, 2):
        for N in (1, 33):
            assert lstm_fused_eligible(L, N, H, ndir) is (ok and L >= 1)
            assert lstm_fused_eligible(L, N, H, ndir, aligned=False) is False
    assert lstm_fused_eligible(L, 1, H, 0) is False and lstm_fused_eligible(L, 1, H, 3) is False


def test_eligibility_mirrors_the_descriptor_range():
    from planer_amd.layer import lstm_fused_eligible
    assert lstm_fused_eligible(1, 64, 4096, 1) and lstm_fused_eligible(1, 64, 11584, 1)      # 4 H H = 2^29 - 1.2e5
    assert not lstm_fused_eligible(1, 64, 11592, 1)                                          # 4 H H >= 2^29
    assert lstm_fused_eligible(1, 65535 * 32, 8, 1) and not lstm_fused_eligible(1, 65535 * 32 + 1, 8, 1)      # 65535 row blocks
    assert lstm_fused_eligible(1, (1 << 20) - 1, 128, 1) and not lstm_fused_eligible(1, 1 << 20, 128, 1)      # N 4H = 2^29
    assert not lstm_fused_eligible(1, -1, 8, 1)


def _step_times(L, step, sign):
    """The kernel's index arithmetic (lstm_kernel.h) restated: launch `step` of a slot of direction `sign` writes Y[t] and reads
    the h of t_prev = t - sign; None at step 0, where it reads h0."""
    t = step if sign > 0 else L - 1 - step
    return t, (None if step == 0 else t - sign)


def _walk(L, sign):
    """One slot: the order in which the launches write Y[t] and what each reads."""
    return [_step_times(L, s, sign) for s in range(L)]


def test_step_to_time_map():
    assert _walk(1, +1) == [(0, None)] and _walk(1, -1) == [(0, None)]
    assert _walk(2, +1) == [(0, None), (1, 0)] and _walk(2, -1) == [(1, None), (0, 1)]
    assert _walk(3, +1) == [(0, None), (1, 0), (2, 1)] and _walk(3, -1) == [(2, None), (1, 2), (0, 1)]
    for L in (1, 2, 3):
        for sign in (+1, -1):
            seq = _walk(L, sign)
            assert sorted(t for t, _ in seq) == list(range(L))                   # every step written once
            assert [t for t, _ in seq] == list(range(L))[::sign]                 # in the per-step program's order
            assert all(prev == seq[s - 1][0] for s, (_, prev) in enumerate(seq) if s)      # reads what the last launch wrote
            assert seq[-1][0] == (L - 1 if sign > 0 else 0)                      # where the final h is


def test_switch_parses(monkeypatch):
    from planer_amd.layer import lstm_fused_enabled
    monkeypatch.delenv("PLANER_HIP_LSTM_FUSED", raising=False)
    assert lstm_fused_enabled() is True
    for value, want in (("0", False), ("1", True), ("", True), ("off", True)):
        monkeypatch.setenv("PLANER_HIP_LSTM_FUSED", value)
        assert lstm_fused_enabled() is want                                      # read at call time
