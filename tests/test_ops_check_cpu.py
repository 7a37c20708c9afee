"""The checks of the conditioning and loss kernel edge tests (tests/ops_check.py) checked on the CPU: the fp32 stand-in -- the kernels'
arithmetic in torch float32 -- passes every bound of every case, so the counted bounds are reachable before anything runs on a
device; each planted fault, of the kind these kernels can have without the whole-tensor L2 ratio of tests/test_ops_gpu.py noticing,
fails a case that is named here; and the case tables hold every value they were given."""
import pytest
import torch

import ops_check as oc
from ops_check import (ADA_BWD_CASES, ADA_FWD_CASES, AXPY_N, CFM_CASES, COLSUM_CASES, DTEMB_CASES, GEGLU_CASES, MSE_CASES, SELECT_CASES,
                       SUM_ROWS_CASES, AdaFwdCase)


def _fails(fn, what):
    with pytest.raises(AssertionError, match=what):
        fn()


def _by_name(cases, name):
    return next(c for c in cases if c.name == name)


# ------------------------------------------------------------------------------------------------ the tables hold what they claim
def test_ada_fwd_table():
    m = [c for c in ADA_FWD_CASES if c.kernel == "mfma"]
    s = [c for c in ADA_FWD_CASES if c.kernel == "scalar"]
    assert {(c.B, c.Th) for c in m} >= {(B, Th) for B in (1, 4, 5, 12, 13, 16) for Th in (32, 256, 288, 544)}
    assert {c.J for c in m if not c.group} == set(oc.ADA_J) and {(c.J, c.group) for c in m if c.group} == set(oc.ADA_GROUPS)
    assert {c.Th for c in m if c.small} == {32, 256, 288, 544}
    assert {(c.B, c.Th, c.J) for c in s if not c.group} == {(B, Th, J) for B, Th in ((17, 32), (3, 8), (3, 264), (9, 40), (16, 24), (8, 4104))
                                                            for J in (1, 17, 64, 65)}
    assert {(c.J, c.group) for c in s if c.group} == set(oc.ADA_GROUPS)
    assert all(oc.fwd_kernel(c.B, c.Th) == c.kernel for c in ADA_FWD_CASES)
    assert len({c.name for c in ADA_FWD_CASES}) == len(ADA_FWD_CASES)


def test_ada_bwd_dtemb_tables():
    v2 = [c for c in ADA_BWD_CASES if c.kernel == "v2"]
    v1 = [c for c in ADA_BWD_CASES if c.kernel == "v1"]
    assert {c.J for c in v2} == {1, 4, 127, 129, 516, 1100, 8192} and {c.per for c in v2} == {1, 2, 5, 9, 64}
    assert {c.Th for c in v2} == {8, 264, 2056} and {c.B for c in v2} == {1, 8, 9, 11}
    assert {(c.dw, c.acc) for c in v2} == {(d, a) for d in (True, False) for a in (0, 1)}
    assert {(c.B, c.Th) for c in v1} == {(B, Th) for B in (1, 8, 9) for Th in (8, 264)} | {(1, 2056)} and {c.J for c in v1} == {8196}
    assert {c.dw for c in v1} == {True, False} and {c.acc for c in v1} == {0, 1}
    assert all(oc.bwd_kernel(c.J) == c.kernel for c in ADA_BWD_CASES)
    assert {c.rows for c in DTEMB_CASES} >= {1, 2, 27, 32, 33, 97, 128, 129, 161}
    assert {(c.L, c.J) for c in DTEMB_CASES} >= {(L, J) for L in (1, 3) for J in (4, 64, 65, 516)}
    assert {(c.B, c.Th) for c in DTEMB_CASES} >= {(B, Th) for B in (1, 8, 9, 11) for Th in (8, 264, 2056)}
    for cs in (ADA_BWD_CASES, DTEMB_CASES):
        assert len({c.name for c in cs}) == len(cs)


def test_other_tables():
    assert {(c.rows, c.cols) for c in SUM_ROWS_CASES} == {(r, cl) for r in (1, 4, 5, 12, 13, 16, 17, 33) for cl in (1, 63, 64, 65)}
    assert {(c.pad > 0, c.acc) for c in SUM_ROWS_CASES} == {(p, a) for p in (True, False) for a in (0, 1)}
    assert {(c.M, c.Fp) for c in GEGLU_CASES if c.colsum} == {(M, Fp) for Fp in (64, 192, 512, 576) for M in (1, 3, 5, 511, 512, 513, 1025)}
    assert any(c.M * c.Fp // 8 > oc.GRID_CAP and c.Fp == 64 for c in GEGLU_CASES)
    bf = [c for c in COLSUM_CASES if c.kind == "bf16" and not c.rowmap]
    assert {(c.M, c.C) for c in bf} == {(M, C) for C in (8, 512, 520) for M in (1, 5, 127, 128, 129, 257)} and {c.pad for c in bf} == {0, 8}
    assert {(c.Fd, c.C // 2) for c in COLSUM_CASES if c.rowmap} == {(60, 64), (170, 192)} and any(c.out_len for c in COLSUM_CASES)
    assert {c.C for c in COLSUM_CASES if c.kind == "f32"} == {4, 256, 260}
    assert {(c.N, c.D) for c in MSE_CASES} >= {(N, D) for N in (1, 4, 255, 256, 257, 513) for D in (4, 252, 256, 260)}
    assert {c.B for c in MSE_CASES} == {1, 3} and {c.mask for c in MSE_CASES} == set(oc.MSE_MASKS)
    assert {c.outs for c in MSE_CASES} == set(oc.MSE_OUTS) and {c.gscale for c in MSE_CASES} == {True, False}
    assert any(c.mask == "late" and c.N > 256 for c in MSE_CASES) and any(c.B * c.N * c.D // 4 > oc.GRID_CAP for c in MSE_CASES)
    assert {(c.per, c.sigma) for c in CFM_CASES} >= {(p, s) for p in (1, 7, 1030) for s in (0.0, oc.SIGMA_01)}
    assert any(c.B * c.per > oc.GRID_CAP for c in CFM_CASES) and AXPY_N[2] // 4 > oc.GRID_CAP
    assert {(c.L, c.B, c.G) for c in SELECT_CASES} == {(L, B, G) for L in (1, 3) for B in (1, 5) for G in (4, 520)}
    for cs in (SUM_ROWS_CASES, GEGLU_CASES, COLSUM_CASES, MSE_CASES, CFM_CASES, SELECT_CASES):
        assert len({c.name for c in cs}) == len(cs)


# ------------------------------------------------------------------------------------------------ the stand-in passes every bound
@pytest.mark.parametrize("c", ADA_FWD_CASES, ids=lambda c: c.name)
def test_standin_passes_ada_fwd(c):
    oc.check_ada_fwd(c, oc.standin_ada_fwd(c))


@pytest.mark.parametrize("c", ADA_BWD_CASES, ids=lambda c: c.name)
def test_standin_passes_ada_bwd(c):
    oc.check_ada_bwd(c, oc.standin_ada_bwd(c))


@pytest.mark.parametrize("c", DTEMB_CASES, ids=lambda c: c.name)
def test_standin_passes_dtemb(c):
    oc.check_dtemb(c, oc.standin_dtemb(c))


@pytest.mark.parametrize("c", SUM_ROWS_CASES, ids=lambda c: c.name)
def test_standin_passes_sum_rows(c):
    oc.check_sum_rows(c, oc.standin_sum_rows(c))


@pytest.mark.parametrize("c", GEGLU_CASES, ids=lambda c: c.name)
def test_standin_passes_geglu(c):
    oc.check_geglu(c, oc.standin_geglu(c))


@pytest.mark.parametrize("c", COLSUM_CASES, ids=lambda c: c.name)
def test_standin_passes_colsum(c):
    oc.check_colsum(c, oc.standin_colsum(c))


@pytest.mark.parametrize("c", MSE_CASES, ids=lambda c: c.name)
def test_standin_passes_mse(c):
    oc.check_mse(c, oc.standin_mse(c))


@pytest.mark.parametrize("c", CFM_CASES, ids=lambda c: c.name)
def test_standin_passes_cfm(c):
    oc.check_cfm(c, oc.standin_cfm(c))


@pytest.mark.parametrize("n", AXPY_N[:2])
def test_standin_passes_axpy(n):
    oc.check_axpy(n, oc.standin_axpy(n))


@pytest.mark.parametrize("c", SELECT_CASES, ids=lambda c: c.name)
def test_standin_passes_select(c):
    oc.check_select(c, oc.standin_select(c))


@pytest.mark.parametrize("name", list(oc.MR_SETS), ids=str)
def test_standin_passes_multi_reduce(name):
    ks = oc.MR_SETS[name]
    oc.check_mr(name, ks, [oc.standin_mr(k) for k in ks])


@pytest.mark.parametrize("c", oc.TIME_CASES, ids=lambda c: c.name)
def test_standin_passes_time(c):
    oc.check_time(c, oc.standin_time(c))


def test_time_and_multi_reduce_tables():
    cs = oc.TIME_CASES
    assert {(c.D, c.Th) for c in cs} == {(D, Th) for D in (2, 62, 64, 66, 130) for Th in (1, 3, 31, 32, 33, 65)} and {c.B for c in cs} == {1, 3, 9}
    for B in (1, 3, 9):
        t = oc.time_inputs(next(c for c in cs if c.B == B))["times"]
        assert float(t[0]) == 1.0 and (B == 1 or float(t[1]) == 0.0)
    c = next(c for c in cs if c.D == 130)
    assert float((oc.time_inputs(c)["wsin"].abs() * oc.time_inputs(c)["times"].max()).max()) > 2  # an argument of several turns
    js = oc.MR_JOBS
    assert len(js) == oc.VBX_MR_MAX == 48
    assert {(j.rows, j.cols) for j in js} >= {(r, cl) for r in (1, 15, 16, 17, 49, 64, 65, 113) for cl in (1, 63, 64, 65)}
    assert {j.batches for j in js} == {1, 3} and any(j.dst_len and not j.rowmap for j in js) and sum(j.rowmap for j in js) == 2
    assert all(j.b_pad and j.d_pad for j in js if j.batches > 1) and any(j.row_pad for j in js)
    assert {len(v) for v in oc.MR_SETS.values()} == {1, 2, 48}
    sw = oc.time_sweep_inputs()
    f = oc.f_arg32(sw["times"], sw["wsin"])
    assert float(f.abs().max()) <= oc.F_SWEEP and float(f.abs().max()) > oc.F_SWEEP - 0.01 and float(f.min()) < -31
    assert float(sw["b1"][0]) == -oc.P_SWEEP and float(sw["b1"][-1]) == oc.P_SWEEP


def test_fault_time():
    c = next(c for c in oc.TIME_CASES if c.D == 66 and c.B == 9)
    _fails(lambda: oc.check_time(c, oc.standin_time(c, "swap")), c.name + r": four \[time_four\]")
    _fails(lambda: oc.check_time(c, oc.standin_time(c, "db1")), c.name + r": .*db1 \[time_db1\]")
    c = next(c for c in oc.TIME_CASES if c.D == 2 and c.B == 3)
    _fails(lambda: oc.check_time(c, oc.standin_time(c, "db1")), c.name + r": .*db1 \[time_db1\]")


def test_fault_multi_reduce_reads_a_padding_row():
    got = oc.standin_mr(13)
    got[0] += oc.mr_input(13)[1][oc.MR_JOBS[13].cols]  # the first padding column of the operand
    _fails(lambda: oc.check_mr("n1-job13", (13,), [got]), r"multireduce-n1-job13: job 13 \[multi_reduce\]")


def test_counter():
    t = oc.new_counter()
    t[1] += 3
    oc.check_counter(t, 3)
    _fails(lambda: oc.check_counter(oc.new_counter(), 3), "counter-add-3")


# ------------------------------------------------------------------------------------------------ planted faults
def test_fault_ada_fwd_rows_of_the_upper_lane_quads():
    for B in (5, 16):
        c = AdaFwdCase("mfma", B, 288, 72, 24)
        _fails(lambda: oc.check_ada_fwd(c, oc.standin_ada_fwd(c, "rowshift")), c.name + r": ada \[ada_fwd_mfma\]")


def test_fault_ada_fwd_partial_k_round_dropped():
    for Th in (288, 544):
        c = next(c for c in ADA_FWD_CASES if c.kernel == "mfma" and c.Th == Th and not c.small)
        _fails(lambda: oc.check_ada_fwd(c, oc.standin_ada_fwd(c, "kround")), c.name + r": ada \[ada_fwd_mfma\]")


def test_fault_ada_fwd_group_of_the_waves_first_output():
    for J, g in ((72, 24), (136, 8)):
        c = AdaFwdCase("mfma", 5, 288, J, g)
        _fails(lambda: oc.check_ada_fwd(c, oc.standin_ada_fwd(c, "group_first")), c.name + r": ada \[ada_fwd_mfma\]")
    c = AdaFwdCase("mfma", 5, 288, 512, 128)  # a multiple of 16: the fault is invisible at the only group size tested before
    oc.check_ada_fwd(c, oc.standin_ada_fwd(c, "group_first"))


@pytest.mark.parametrize("fault", ["no_lo", "flush_lo"])
def test_fault_ada_fwd_lo_half_and_the_tightness_of_the_bound(fault):
    """On the small-magnitude temb (every lo an fp16 subnormal) the stand-in stays below half the bound and losing lo -- altogether, or
    to a flush of subnormals -- exceeds it, already at Th = 32."""
    c = AdaFwdCase("mfma", 13, oc.SMALL_TH, 65, small=True)
    assert c in ADA_FWD_CASES and oc.SMALL_TH == 32
    ck = oc.check_ada_fwd(c, oc.standin_ada_fwd(c))
    worst = max(v for n, v, b in ck.seen if "error / bound" in n)
    assert worst < 0.5, worst
    _fails(lambda: oc.check_ada_fwd(c, oc.standin_ada_fwd(c, fault)), c.name + r": ada \[ada_fwd_mfma_small\]")
    for Th in (256, 288, 544):
        c = AdaFwdCase("mfma", 13, Th, 65, small=True)
        _fails(lambda: oc.check_ada_fwd(c, oc.standin_ada_fwd(c, fault)), r"ada \[ada_fwd_mfma_small\]")


def test_fault_ada_fwd_no_lo_on_ordinary_magnitudes():
    c = next(c for c in ADA_FWD_CASES if c.kernel == "mfma" and c.Th == 256 and not c.small)
    _fails(lambda: oc.check_ada_fwd(c, oc.standin_ada_fwd(c, "no_lo")), c.name + r": ada \[ada_fwd_mfma\]")


def test_fault_ada_bwd():
    c = _by_name(ADA_BWD_CASES, "adabwd-v2-B9-Th264-J129-dw-acc1")
    _fails(lambda: oc.check_ada_bwd(c, oc.standin_ada_bwd(c, "tail")), c.name + r": scratch \[ada_bwd_scratch\].*dtemb \[ada_bwd_dtemb\]")
    _fails(lambda: oc.check_ada_bwd(c, oc.standin_ada_bwd(c, "acc")), c.name + r": dtemb \[ada_bwd_dtemb\]")
    _fails(lambda: oc.check_ada_bwd(c, oc.standin_ada_bwd(c, "dbias8")), c.name + r": dbias \[ada_bwd_dbias\]")
    c = next(c for c in ADA_BWD_CASES if c.kernel == "v1" and c.B == 9 and c.Th == 264)
    _fails(lambda: oc.check_ada_bwd(c, oc.standin_ada_bwd(c, "tail")), c.name + r": scratch \[ada_bwd_scratch\]")
    _fails(lambda: oc.check_ada_bwd(c, oc.standin_ada_bwd(c, "dbias8")), c.name + r": dbias \[ada_bwd_dbias\]")


def test_fault_dtemb_rows_past_the_slice_carry_a_weight():
    for c in (c for c in DTEMB_CASES if c.J in (65, 516, 4)):
        _fails(lambda: oc.check_dtemb(c, oc.standin_dtemb(c, "clamp")), c.name + r": scratch \[dtemb_scratch\]")


def test_fault_geglu():
    c = _by_name(GEGLU_CASES, "geglu-M513-Fp192")
    _fails(lambda: oc.check_geglu(c, oc.standin_geglu(c, "swap")), c.name + r": dh1 \[geglu_dh1\]")
    _fails(lambda: oc.check_geglu(c, oc.standin_geglu(c, "rec32")), c.name + r": slab records \[geglu_rec\]")
    _fails(lambda: oc.check_geglu(c, oc.standin_geglu(c, "trunc")), c.name + r": dh1 \[geglu_dh1\]")
    c = _by_name(GEGLU_CASES, "geglu-M1-Fp64")
    _fails(lambda: oc.check_geglu(c, oc.standin_geglu(c, "rec32")), c.name + r": slab records \[geglu_rec\]")


def test_fault_colsum():
    c = _by_name(COLSUM_CASES, "colsum-bf16-M257-C520-pad8-map0-F0-len0")
    _fails(lambda: oc.check_colsum(c, oc.standin_colsum(c, "lastrow")), c.name + r": slab records \[colsum_rec\]")
    _fails(lambda: oc.check_colsum(c, oc.standin_colsum(c, "pad")), c.name + r": slab records \[colsum_rec\]")
    c = next(c for c in COLSUM_CASES if c.rowmap and c.Fd == 170 and not c.out_len and c.M == 129)
    _fails(lambda: oc.check_colsum(c, oc.standin_colsum(c, "mapblock")), c.name + r": out \[colsum_out\]")
    c = next(c for c in COLSUM_CASES if c.kind == "f32" and c.M == 257 and c.pad)
    _fails(lambda: oc.check_colsum(c, oc.standin_colsum(c, "pad")), c.name + r": slab records \[colsum_rec\]")


def test_fault_mse():
    late = _by_name(MSE_CASES, "mse-B3-N513-D260-late-gs-both")
    _fails(lambda: oc.check_mse(late, oc.standin_mse(late, "late")), late.name + r": .*split counts failed")
    ones = next(c for c in MSE_CASES if c.N == 513 and c.mask == "ones")
    _fails(lambda: oc.check_mse(ones, oc.standin_mse(ones, "late")), ones.name + r": split numerators \[mse_split\]")
    empty = _by_name(MSE_CASES, "mse-B3-N513-D4-empty-gs-both")
    _fails(lambda: oc.check_mse(empty, oc.standin_mse(empty, "noclamp")), empty.name + r": .*denominators failed")
    _fails(lambda: oc.check_mse(late, oc.standin_mse(late, "nogscale")), late.name + r": dpred \[mse_dpred\].*dpb \[mse_dpb\]")
    _fails(lambda: oc.check_mse(late, oc.standin_mse(late, "d4")), late.name + r": split numerators \[mse_split\]")


def test_fault_cfm_and_select():
    c = _by_name(CFM_CASES, f"cfm-B3-per7-sigma{oc.SIGMA_01:.3g}")
    _fails(lambda: oc.check_cfm(c, oc.standin_cfm(c, "x1")), c.name + r": flow \[cfm_flow\]")
    c = SELECT_CASES[0]
    _fails(lambda: oc.check_select(c, oc.standin_select(c, "slot")), c.name + ": ada is the selected row")


def test_one_wrong_row_passes_the_l2_ratio_and_fails_here():
    """One batch row of thirteen off by 1e-5 relative is under the 1e-5 whole-tensor ratio of tests/test_ops_gpu.py, and is found here
    at its row."""
    c = next(c for c in ADA_FWD_CASES if c.kernel == "mfma" and c.B == 13 and c.Th == 288 and c.J == 130)
    got = oc.standin_ada_fwd(c)
    ref = got["ada"][: c.B].clone()
    got["ada"][7] *= 1 + 1e-5
    assert float((got["ada"][: c.B] - ref).norm() / ref.norm()) < 1e-5
    _fails(lambda: oc.check_ada_fwd(c, got), r"ada \[ada_fwd_mfma\] error / bound at \(7, ")
