"""The checks of the row-kernel edge tests (tests/rows_check.py) checked on the CPU: the fp32 stand-in -- the kernels' arithmetic in
torch float32, in their summation order where that is cheap to state -- passes every bound of every case, so the counted bounds are
reachable before anything runs on a device; each planted fault, of the kind these kernels can have without the whole-tensor L2 ratio
of tests/test_ops_gpu.py noticing, fails a case that is named here; and the case tables hold every value they were given."""
import pytest
import torch

import rows_check as rc
from rows_check import CONV_CASES, FINALIZE_CASES, LN_CASES, REDUCE_CASES, RMS_BWD_CASES, RMS_FWD_CASES, SCAN_CASES, RmsFwdCase, ScanCase


def _fails(fn, what):
    with pytest.raises(AssertionError, match=what):
        fn()


def _by_name(cases, name):
    return next(c for c in cases if c.name == name)


# ------------------------------------------------------------------------------------------------ the tables hold what they claim
def test_rms_fwd_table():
    cs = RMS_FWD_CASES
    assert {c.D for c in cs} >= {4, 252, 260, 508, 512, 516, 1024, 1028, 1668, 2044, 2048}
    ranges = {(2, 9, 2, 4), (3, 7, 3, 3), (1, 1, 0, 1), (3, 5, 0, 5)}
    assert {(c.B, c.Np, c.n0, c.rpb) for c in cs} >= ranges
    for D in {c.D for c in cs} - {8}:  # every width: every row range, adaptive and shared
        assert {((c.B, c.Np, c.n0, c.rpb), c.adaptive) for c in cs if c.D == D and not c.zero} == {(r, a) for r in ranges for a in (True, False)}
    assert any(c.B * c.rpb > 16384 and c.D == 8 for c in cs)
    assert any(c.zero and c.adaptive for c in cs) and any(c.zero and not c.adaptive for c in cs)
    assert len({c.name for c in cs}) == len(cs)


def test_rms_bwd_table():
    cs = RMS_BWD_CASES
    assert {c.D for c in cs} == {4, 260, 512, 516, 1024, 1028, 1668, 2048}
    for D in {c.D for c in cs}:
        mine = [c for c in cs if c.D == D]
        assert {c.rpb for c in mine} >= {1, 7, 8, 9, 15, 16, 17, 33}
        assert {c.ptrs for c in mine} == set(rc.PTRS) and {c.B for c in mine} == {1, 3} and {c.n0 for c in mine} == {0, 3}
        assert {c.adaptive for c in mine} == {True, False}
    assert all(c.Np > c.n0 + c.rpb for c in cs)
    assert any(c.zero and c.D == 512 for c in cs) and any(c.zero and c.D != 512 for c in cs)
    assert len({c.name for c in cs}) == len(cs)


def test_reduce_ln_tables():
    for kind in ("norm", "col"):
        assert {c.chunks for c in REDUCE_CASES if c.kind == kind} == {1, 2, 65}
    assert {c.sum_batch for c in REDUCE_CASES if c.kind == "norm"} == {0, 1} and any(c.pad for c in REDUCE_CASES)
    assert {c.D for c in LN_CASES} >= {4, 260, 512, 516, 1024, 1028, 1668, 2048}
    for D in (4, 260, 512, 516, 1024, 1028, 1668, 2048):
        mine = [c for c in LN_CASES if c.D == D and not c.const]
        assert {c.Np for c in mine} == {1, 8, 9, 16, 17} and {c.resid for c in mine} == {True, False}
    assert any(c.B * c.Np == 16389 and c.D == 8 for c in LN_CASES) and any(c.const for c in LN_CASES)
    assert len({c.name for c in LN_CASES}) == len(LN_CASES) and len({c.name for c in REDUCE_CASES}) == len(REDUCE_CASES)


def test_scan_table():
    assert {c.Np for c in SCAN_CASES} == {1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025}
    assert {c.D for c in SCAN_CASES} == {1, 31, 32, 33, 96} and {c.B for c in SCAN_CASES} == {1, 2}
    assert {(c.B, c.Np, c.D) for c in SCAN_CASES if c.gates == "normal"} == {(c.B, c.Np, c.D) for c in SCAN_CASES if c.gates == "long"}
    assert 12 <= len(SCAN_CASES) // 2 <= 16
    c = ScanCase(1, 1025, 96, "long")
    a = rc.scan_inputs(c)["qkva"][..., 2 * c.D:].double().sigmoid()
    assert 0.95 < float(a.min()) and float(a.max()) < 0.9991
    x = rc.sweep_logits()
    assert float(x[0]) == rc.SWEEP[0] and float(x[-1]) == rc.SWEEP[1]


def test_conv_table():
    cs = CONV_CASES
    assert {c.N for c in cs} == {1, 15, 16, 63, 64, 65, 129} and {c.D for c in cs} == {1, 40, 64, 72, 128}
    assert {c.ks for c in cs} == {1, 3, 31} and {c.R for c in cs} == {0, 16} and {c.B for c in cs} == {1, 3}
    assert {c.mask for c in cs} == set(rc.MASKS) and 14 <= len(cs) <= 18
    assert any(c.ks == 31 and c.N == 1 for c in cs) and any(c.ks == 31 and c.N == 15 for c in cs)
    assert any(c.mask == "hole" and c.N >= 66 for c in cs)  # the whole hole 62..65
    assert any(c.R and c.dreg_null for c in cs) and any(c.R and not c.dreg_null for c in cs)
    assert [f[0] for f in FINALIZE_CASES] == [1, 3, 4, 5, 9]
    assert len({c.name for c in cs}) == len(cs)


# ------------------------------------------------------------------------------------------------ the stand-in passes every bound
@pytest.mark.parametrize("c", RMS_FWD_CASES, ids=lambda c: c.name)
def test_standin_passes_rms_fwd(c):
    rc.check_rms_fwd(c, rc.standin_rms_fwd(c))


@pytest.mark.parametrize("c", RMS_BWD_CASES, ids=lambda c: c.name)
def test_standin_passes_rms_bwd(c):
    rc.check_rms_bwd(c, rc.standin_rms_bwd(c))


@pytest.mark.parametrize("c", REDUCE_CASES, ids=lambda c: c.name)
def test_standin_passes_reduce(c):
    rc.check_reduce(c, rc.standin_reduce(c))


@pytest.mark.parametrize("c", LN_CASES, ids=lambda c: c.name)
def test_standin_passes_ln(c):
    rc.check_ln(c, rc.standin_ln(c))


@pytest.mark.parametrize("c", SCAN_CASES, ids=lambda c: c.name)
def test_standin_passes_scan(c):
    rc.check_scan(c, rc.standin_scan(c))


@pytest.mark.parametrize("c", CONV_CASES, ids=lambda c: c.name)
def test_standin_passes_conv(c):
    rc.check_conv(c, rc.standin_conv(c))


@pytest.mark.parametrize("f", FINALIZE_CASES, ids=rc.finalize_name)
def test_standin_passes_finalize(f):
    rc.check_finalize(f, rc.standin_finalize(f))


# ------------------------------------------------------------------------------------------------ planted faults
LONG = ScanCase(1, 1025, 96, "long")


def test_fault_scan_carry_dropped_at_one_seam():
    _fails(lambda: rc.check_scan(LONG, rc.standin_scan(LONG, "seam")), r"scan-B1-Np1025-D96-long: s \[scan_s\].*hstate \[scan_h\]")
    short = ScanCase(1, 33, 33, "long")  # T = 2: the seam in front of frame 16
    _fails(lambda: rc.check_scan(short, rc.standin_scan(short, "seam")), r"scan-B1-Np33-D33-long: s \[scan_s\]")


def test_fault_scan_carry_passes_the_l2_ratio_with_short_memory_and_fails_here():
    """Why the whole-tensor ratio cannot see one dropped carry: with gates from N(0, 1) it changes a handful of frames of 1025."""
    c = ScanCase(1, 1025, 96, "normal")
    good, bad = rc.standin_scan(c), rc.standin_scan(c, "seam")
    rows = c.B * c.Np
    assert float((bad["s"][:rows] - good["s"][:rows]).norm() / good["s"][:rows].norm()) < 0.1
    _fails(lambda: rc.check_scan(c, bad), r"scan-B1-Np1025-D96-normal: s \[scan_s\]")


def test_fault_scan_bwd_gate_of_the_wrong_frame():
    _fails(lambda: rc.check_scan(LONG, rc.standin_scan(LONG, "an")), r"scan-B1-Np1025-D96-long: dkv \[scan_dkv\].*da \[scan_da\]")


def test_fault_conv_taps_across_the_tile_seam():
    c = _by_name(CONV_CASES, "conv-B3-N129-D128-ks3-R0-row")
    _fails(lambda: rc.check_conv(c, rc.standin_conv(c, "seam")), r"conv-B3-N129-D128-ks3-R0-row: xs\[:, R:\] \[conv_fwd\]")
    c = _by_name(CONV_CASES, "conv-B1-N129-D40-ks31-R0-hole")
    _fails(lambda: rc.check_conv(c, rc.standin_conv(c, "seam")), r"conv-B1-N129-D40-ks31-R0-hole: xs\[:, R:\] \[conv_fwd\]")


def test_fault_conv_mask_on_the_residual():
    c = _by_name(CONV_CASES, "conv-B3-N65-D40-ks31-R16-hole")
    _fails(lambda: rc.check_conv(c, rc.standin_conv(c, "mask_e")), r"conv-B3-N65-D40-ks31-R16-hole: xs\[:, R:\] \[conv_fwd\]")


def test_fault_conv_bias_gradient_slot():
    c = _by_name(CONV_CASES, "conv-B1-N64-D128-ks31-R0-none")
    _fails(lambda: rc.check_conv(c, rc.standin_conv(c, "bias_slot")), r"conv-B1-N64-D128-ks31-R0-none: wpart \[conv_wpart\]")


def test_fault_n0_ignored():
    c = RmsFwdCase(512, 2, 9, 2, 4, True)
    _fails(lambda: rc.check_rms_fwd(c, rc.standin_rms_fwd(c, "n0")), r"rmsfwd-D512-B2-Np9-n2-r4-ada: y bf16 \[rms_fwd_bf16\]")
    b = next(c for c in RMS_BWD_CASES if c.D == 1024 and c.n0 == 3)
    _fails(lambda: rc.check_rms_bwd(b, rc.standin_rms_bwd(b, "n0")), b.name + r": dx_out \[rms_bwd_dx\]")


def test_fault_gamma_of_batch_0():
    c = RmsFwdCase(1024, 3, 7, 3, 3, True)
    _fails(lambda: rc.check_rms_fwd(c, rc.standin_rms_fwd(c, "gamma0")), r"rmsfwd-D1024-B3-Np7-n3-r3-ada: y bf16 \[rms_fwd_bf16\]")
    b = next(c for c in RMS_BWD_CASES if c.D == 512 and c.B == 3 and c.adaptive)
    _fails(lambda: rc.check_rms_bwd(b, rc.standin_rms_bwd(b, "gamma0")), b.name + r": dx_out \[rms_bwd_dx\]")


def test_fault_last_record_takes_the_row_past_the_range():
    b = next(c for c in RMS_BWD_CASES if c.D == 512 and c.rpb == 17)
    _fails(lambda: rc.check_rms_bwd(b, rc.standin_rms_bwd(b, "rowpast")), b.name + r": part\[..\]\[0\] \(gamma\) \[rms_bwd_part\]")


def test_fault_last_float4_dropped():
    c = RmsFwdCase(260, 3, 5, 0, 5, False)
    _fails(lambda: rc.check_rms_fwd(c, rc.standin_rms_fwd(c, "float4")), r"rmsfwd-D260-B3-Np5-n0-r5-shared: y bf16 \[rms_fwd_bf16\]")
    b = next(c for c in RMS_BWD_CASES if c.D == 516)
    _fails(lambda: rc.check_rms_bwd(b, rc.standin_rms_bwd(b, "float4")), b.name + r": dx_out \[rms_bwd_dx\]")


def test_fault_beta_ignored():
    c = RmsFwdCase(2048, 3, 5, 0, 5, True)
    _fails(lambda: rc.check_rms_fwd(c, rc.standin_rms_fwd(c, "beta")), r"rmsfwd-D2048-B3-Np5-n0-r5-ada: y bf16 \[rms_fwd_bf16\]")


def test_fault_layernorm_divides_by_d_minus_1():
    c = next(c for c in LN_CASES if c.D == 1668 and c.Np == 9)  # the widest: 1 / (D - 1) is 6e-4 off
    _fails(lambda: rc.check_ln(c, rc.standin_ln(c, "dm1")), c.name + r": y \[ln_fwd\]")
    c = next(c for c in LN_CASES if c.D == 4 and not c.fwd_only)
    _fails(lambda: rc.check_ln(c, rc.standin_ln(c, "dm1")), c.name + r": y \[ln_fwd\].*ds \[ln_bwd_ds\]")


def test_one_wrong_element_passes_the_l2_ratio_and_fails_here():
    """One completely wrong element of a large output is about 5e-4 of the whole-tensor norm: under the 4e-3 of the L2 test."""
    c = RMS_FWD_CASES[[x.name for x in RMS_FWD_CASES].index("rmsfwd-D8-B1-Np16389-n0-r16389-ada")]
    got = rc.standin_rms_fwd(c)
    ref = got["f32"][: c.B * c.rpb].clone()
    j = int((ref[777].abs() - 0.5).abs().argmin())  # an element of ordinary size, lost
    assert 0.25 < abs(float(ref[777, j])) < 1.0
    got["bf16"][777, j] = 0
    assert float((got["bf16"][: c.B * c.rpb].float() - ref).norm() / ref.norm()) < 4e-3
    _fails(lambda: rc.check_rms_fwd(c, got), r"y bf16 \[rms_fwd_bf16\] error / bound at \(777, %d\)" % j)


def test_half_ulp():
    assert float(rc.half_ulp(torch.tensor([1.0]), rc.BF16)) == 2.0 ** -8 and float(rc.half_ulp(torch.tensor([1.99]), rc.BF16)) == 2.0 ** -8
    assert float(rc.half_ulp(torch.tensor([2.0]), rc.F16)) == 2.0 ** -10 and float(rc.half_ulp(torch.tensor([0.0]), rc.F16)) == 2.0 ** -25
    x = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20])
    assert abs(float(x.to(rc.BF16)) - float(x)) <= float(rc.half_ulp(x, rc.BF16))
    assert rc.U == torch.finfo(torch.float32).eps / 2
