"""The checks of the sampler kernel edge tests (tests/ode_check.py) checked on the CPU: the fp32 stand-in -- the kernels' arithmetic
in torch float32, a product and then a sum -- passes every check of every case, so the bit comparisons and the counted bounds are
reachable before anything runs on a device; each planted fault, of the kind these kernels can have while every sample still comes
out right at 2e-3, fails a case that is named here; and the case tables hold every value they were given."""
import math

import pytest
import torch

import ode_check as oc
from ode_check import (COMBINE_CASES, COMMIT_CASES, COPY_COLS_CASES, DENSE_CASES, NORM_CASES, PACK_CASES, STACK_CASES, TIME_CASES, UNET_CASES,
                       ZERO_TAIL_CASES)


def _fails(fn, what):
    with pytest.raises(AssertionError, match=what):
        fn()


def _ids(c):
    return getattr(c, "name", None) or "-".join(map(str, c))


# ------------------------------------------------------------------------------------------------ the tables hold what they claim
def test_combine_and_time_tables():
    t = [c for c in COMBINE_CASES if c.form == "table"]
    d = [c for c in COMBINE_CASES if c.form != "table"]
    for cs in (t, d):
        assert {(c.n, c.S) for c in cs} >= {(n, S) for n in oc.SMALL_N for S in range(1, 8)}
        assert {(c.S, c.inplace) for c in cs} >= {(S, ip) for S in (1, 7) for ip in (False, True)}
    assert {(c.n, c.S) for c in COMBINE_CASES if c.n > 4 * oc.GRID_CAP} == {(oc.N_CAP, 1), (oc.N_CAP, 7)} and oc.N_CAP == 4096 * 256 * 4 + 12
    forms = {(c.ld - c.S, c.stride, c.row, c.counter) for c in t if c.S == 3}
    assert forms == {(dl, st, r, ctr) for dl in (0, 3) for st in (1, 3, 5) for r in (0, st - 1) for ctr in (0, 5)}
    assert {c.form for c in d} == {"dt", "h0"}
    for form, v in oc.SLOT_VALUE.items():
        assert oc.f32(v) != v
        b = torch.tensor(oc.C01[form][:1], dtype=oc.F64).float()
        assert float(oc.step_coefs(b, v)) != float(oc.step_coefs(b, v, "nocast"))
    for c in COMBINE_CASES:  # the table holds NaN outside the addressed row, the state outside the addressed slot
        ops = oc.combine_operands(c)
        if c.form == "table":
            assert int((~torch.isnan(ops["table"])).sum()) == c.S and ops["table"].numel() > (c.counter * c.stride + c.row) * c.ld + c.S
        else:
            assert int((~torch.isnan(ops["state"][: oc.DP_STATE])).sum()) == 1
    assert {c.B for c in TIME_CASES} == set(oc.TIME_B) == {1, 63, 64, 65, 130}
    assert {(c.B, c.which) for c in TIME_CASES if c.mode == "end"} == {(B, w) for B in oc.TIME_B for w in oc.TIME_ENDS}
    assert {c.mode for c in TIME_CASES} == {"table", "stage", "probe", "end"}
    ends = {w: T + DT for w, (T, DT) in oc.TIME_ENDS.items()}
    assert ends["one"] == 1.0 and ends["half"] == 0.5 and ends["zero"] == 0.0 and ends["negative"] < 0 and ends["min_normal"] == 2.0 ** -126
    assert oc.f32(ends["rounds_up"]) > ends["rounds_up"]
    assert float(oc.time_value(oc.TimeCase("end", 1, "zero"))) == -(2.0 ** -149)
    assert float(oc.time_value(oc.TimeCase("end", 1, "min_normal"))) == 2.0 ** -126 - 2.0 ** -149
    for cs in (COMBINE_CASES, TIME_CASES):
        assert len({c.name for c in cs}) == len(cs)


def test_norm_table():
    plain = [c for c in NORM_CASES if c.shape is None and c.data == "rand"]
    assert {(c.mode, c.n) for c in plain} >= {(m, n) for m in range(3) for n in oc.SMALL_N + (oc.N_SLAB, oc.N_NORM_CAP)}
    assert oc.N_SLAB == 257 * 1024 + 8 and oc.NormCase(0, oc.N_SLAB).nb == 258 and oc.N_NORM_CAP == 1024 * 256 * 4 + 20
    lens = [c for c in NORM_CASES if c.shape is not None]
    assert {c.shape for c in lens} >= {(3, 37, 12), (2, 9, 4)} and {c.mode for c in lens if c.n < oc.NORM_CAP} == {0, 1, 2}
    assert any(0 in c.lens and c.shape[1] in c.lens and any(0 < l < c.shape[1] for l in c.lens) for c in lens)
    big = next(c for c in lens if c.n > 4 * oc.NORM_CAP)
    B, N, D = big.shape
    edge = (N + big.lens[1]) * D // 4  # the float4 at which row 1 turns into padding: inside the second trip
    assert oc.NORM_CAP < edge < big.n // 4 and big.shape[2] == 4
    assert {c.data for c in NORM_CASES if c.mode == oc.NORM_ERROR} == set(oc.CTRL) | {"rand"}
    assert {(c.data, c.nfe) for c in NORM_CASES if c.data in oc.CTRL} == {(d, m) for d in oc.CTRL for m in (1, 2)}
    assert {(c.mode, c.nfe) for c in NORM_CASES} == {(mode, m) for mode in range(3) for m in (1, 2)}
    assert {(c.mode, c.data) for c in NORM_CASES if c.mode} == {(m, d) for m in (1, 2) for d in oc.INIT_DATA}
    # the arms of the initial step are the ones taken
    arms = set()
    for c in NORM_CASES:
        if c.mode == oc.NORM_INIT1:
            st = oc.norm_inputs(c)["st"]
            dt = float(oc.standin_norm(c)["state"][oc.DP_DT])
            arms.add((st["H0"] == oc.f32(1e-6), st["D1"] <= 1e-15, dt == float(torch.tensor(100.0) * torch.tensor(st["H0"], dtype=oc.F64).float())))
    assert arms == {(False, False, False), (True, False, True), (True, True, False)}
    # the constructed ratios are what the fp64 sum of the element terms gives
    for name, (q, T, dt, TEND) in oc.CTRL.items():
        if name in oc.CTRL_RATIO:
            assert math.sqrt(math.fsum(v * v for v in q) / 4) == oc.CTRL_RATIO[name], name
    assert oc.CTRL_RATIO["above1_f64"] == math.nextafter(1.0, 2.0) and oc.CTRL_RATIO["above1_f32"] == float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))
    assert oc.CTRL_RATIO["clamp10"] < (0.9 / 10) ** 5 and oc.CTRL_RATIO["clamp02"] > (0.9 / 0.2) ** 5
    assert len({c.name for c in NORM_CASES}) == len(NORM_CASES)


def test_other_tables():
    assert {(c.n, c.last, c.done) for c in COMMIT_CASES} == {(n, l, d) for n in oc.SMALL_N for l in (0, 1) for d in (0, 1)} | {(oc.N_CAP, 1, 0)}
    assert {(c.n, c.at) for c in DENSE_CASES} == {(n, a) for n in oc.SMALL_N for a in ("inside", "t1", "t0")} | {(oc.N_CAP, "inside")}
    for at in ("inside", "t1", "t0"):
        st = oc.dense_inputs(oc.DenseCase(4, at))["st"]
        assert (st["T0"] < st["TEND"] < st["T1"]) if at == "inside" else st["TEND"] == st["T1" if at == "t1" else "T0"]
    assert {c.D for c in ZERO_TAIL_CASES} == {1, 3, 4, 12} and sum(c.B * c.N * c.D > oc.GRID_CAP for c in ZERO_TAIL_CASES) == 1
    assert any(0 in c.lens and c.N in c.lens and any(0 < l < c.N for l in c.lens) for c in ZERO_TAIL_CASES)
    assert {(c.D, c.mask, c.bf) for c in PACK_CASES} >= {(D, m, b) for D in (8, 24, 512) for m in (False, True) for b in (False, True)}
    assert sum(c.B * c.N * c.D // 4 > oc.GRID_CAP for c in PACK_CASES) == 1
    assert {(c.R, c.D) for c in STACK_CASES} == {(R, D) for R in (0, 1, 16) for D in (4, 512)}
    cat = [c for c in UNET_CASES if c.kind == "cat"]
    assert {(c.f16, c.bf) for c in cat} == {(1, 0), (0, 1), (1, 1)} and {c.scale for c in cat} == set(oc.UNET_SCALES) == {1.0, 2.0 ** -0.5, 0.5}
    assert {c.bf for c in UNET_CASES if c.kind == "split"} == {False, True} and {c.bf for c in UNET_CASES if c.kind == "addskip"} == {False, True}
    assert all(ld > cols for _, cols, ld in COPY_COLS_CASES)
    x = torch.tensor(oc.SPECIAL, dtype=oc.F64).float()
    h = oc.to_f16_sat(x).float()
    assert float(h[~torch.isnan(h)].abs().max()) == 65504.0 and bool(torch.isinf(x).any()) and bool(torch.isnan(h).any())
    assert bool(((h != 0) & (h.abs() < 2.0 ** -14)).any()) and bool(torch.isinf(oc.to_f16_sat(x, "nosat").float()).any())
    for cs in (COMMIT_CASES, DENSE_CASES, ZERO_TAIL_CASES, PACK_CASES, STACK_CASES, UNET_CASES):
        assert len({c.name for c in cs}) == len(cs)


# ------------------------------------------------------------------------------------------------ the stand-in passes every check
@pytest.mark.parametrize("c", COMBINE_CASES, ids=_ids)
def test_standin_passes_combine(c):
    oc.check_combine(c, oc.standin_combine(c))


@pytest.mark.parametrize("c", TIME_CASES, ids=_ids)
def test_standin_passes_time(c):
    oc.check_time(c, oc.standin_time(c))


@pytest.mark.parametrize("c", NORM_CASES, ids=_ids)
def test_standin_passes_norm(c):
    oc.check_norm(c, oc.standin_norm(c))


@pytest.mark.parametrize("c", COMMIT_CASES, ids=_ids)
def test_standin_passes_commit(c):
    oc.check_commit(c, oc.standin_commit(c))


@pytest.mark.parametrize("c", DENSE_CASES, ids=_ids)
def test_standin_passes_dense(c):
    oc.check_dense(c, oc.standin_dense(c))


@pytest.mark.parametrize("c", ZERO_TAIL_CASES, ids=_ids)
def test_standin_passes_zero_tail(c):
    oc.check_zero_tail(c, oc.standin_zero_tail(c))


@pytest.mark.parametrize("c", PACK_CASES, ids=_ids)
def test_standin_passes_pack(c):
    oc.check_pack(c, oc.standin_pack(c))


@pytest.mark.parametrize("c", STACK_CASES, ids=_ids)
def test_standin_passes_stack(c):
    oc.check_stack(c, oc.standin_stack(c))


@pytest.mark.parametrize("c", UNET_CASES, ids=_ids)
def test_standin_passes_unet(c):
    oc.check_unet(c, oc.standin_unet(c))


@pytest.mark.parametrize("c", COPY_COLS_CASES, ids=_ids)
def test_standin_passes_copy_cols(c):
    oc.check_copy_cols(c, oc.standin_copy_cols(c))


def test_pow_sweep_construction():
    m = oc.pow_sweep_values()
    assert float(m[0]) == 2.0 ** -24 and float(m[-1]) == 2.0 ** 24 and m.numel() == 385
    assert oc.pow_sweep_error(m[7], torch.tensor(0.01) / m[7]) > 0.1  # a wrong power is seen
    want = (float(torch.tensor(0.01) / m[7])) ** float(torch.tensor(1.0) / torch.tensor(5.0))
    assert oc.pow_sweep_error(m[7], torch.tensor(want, dtype=oc.F64).float()) <= oc.U


# ------------------------------------------------------------------------------------------------ planted faults
def test_fault_a_stage_order_reversed():
    """(a): every case of three stages and more tells the order (at two the sum commutes)"""
    for c in (c for c in COMBINE_CASES if c.S >= 3 and c.n < oc.N_CAP):
        _fails(lambda: oc.check_combine(c, oc.standin_combine(c, "reversed")), c.name + ": out is the fp32 sum of fp32 products by bits")
    c = next(c for c in COMBINE_CASES if c.S == 7 and c.n == oc.N_CAP)
    _fails(lambda: oc.check_combine(c, oc.standin_combine(c, "reversed")), c.name + ": out is the fp32 sum of fp32 products by bits")


def test_fault_b_fused_multiply_add():
    """(b): every combine case and the STAGE time fail on a fused product-sum"""
    for c in (c for c in COMBINE_CASES if c.n < oc.N_CAP):
        _fails(lambda: oc.check_combine(c, oc.standin_combine(c, "fma")), c.name + ": out is the fp32 sum of fp32 products by bits")
    c = next(c for c in COMBINE_CASES if c.S == 1 and c.n == oc.N_CAP)
    _fails(lambda: oc.check_combine(c, oc.standin_combine(c, "fma")), c.name + ": out is the fp32 sum of fp32 products by bits")
    for c in (c for c in TIME_CASES if c.mode == "stage"):
        _fails(lambda: oc.check_time(c, oc.standin_time(c, "fma")), c.name + ": times")


def test_fault_c_elements_past_the_grid_cap_skipped():
    for c in (c for c in COMBINE_CASES if c.n == oc.N_CAP):
        _fails(lambda: oc.check_combine(c, oc.standin_combine(c, "cap")), c.name + r": out is the fp32 sum of fp32 products by bits failed")
    c = COMMIT_CASES[-1]
    _fails(lambda: oc.check_commit(c, oc.standin_commit(c, "cap")), c.name + ": y is y1 failed; k1 is k7 failed")
    c = DENSE_CASES[-1]
    _fails(lambda: oc.check_dense(c, oc.standin_dense(c, "cap")), c.name + r": out \[dense\]")
    c = ZERO_TAIL_CASES[-1]
    _fails(lambda: oc.check_zero_tail(c, oc.standin_zero_tail(c, "cap")), c.name + ": dropped elements are")
    c = PACK_CASES[-1]
    _fails(lambda: oc.check_pack(c, oc.standin_pack(c, "cap")), c.name + ": f16 is")
    for c in (c for c in NORM_CASES if c.n > 4 * oc.NORM_CAP):
        kind = ("error", "init0", "init1")[c.mode]
        _fails(lambda: oc.check_norm(c, oc.standin_norm(c, "cap")), c.name + rf": slab lane 0 against the fp64 sum of the fp32 terms \[norm_{kind}_sum\]")


def test_fault_d_slab_entries_from_256_on_dropped():
    """(d): 1032 of 263176 elements lie in workgroups 256 and 257"""
    for c, slot in zip((c for c in NORM_CASES if c.n == oc.N_SLAB), ("RATIO", "D1", "DT")):
        kind = ("error", "init0", "init1")[c.mode]
        _fails(lambda: oc.check_norm(c, oc.standin_norm(c, "slab256")), c.name + rf": .*state {slot} \[norm_{kind}_{slot}\]")
    c = next(c for c in NORM_CASES if c.n == oc.SMALL_N[-1] and c.data == "rand" and c.shape is None)
    oc.check_norm(c, oc.standin_norm(c, "slab256"))  # two workgroups: the fault is invisible at the sizes tested before


def test_fault_e_lens_off_by_one_frame():
    for c in (c for c in NORM_CASES if c.lens is not None and any(l < c.shape[1] for l in c.lens)):
        _fails(lambda: oc.check_norm(c, oc.standin_norm(c, "lens")), c.name + ": ")
    c = ZERO_TAIL_CASES[0]
    _fails(lambda: oc.check_zero_tail(c, oc.standin_zero_tail(c, "lens")), c.name + ": dropped elements are")


def test_fault_f_prev_float_omitted():
    for c in (c for c in TIME_CASES if c.mode == "end"):
        _fails(lambda: oc.check_time(c, oc.standin_time(c, "noprev")), c.name + ": times")


def test_fault_g_dt_without_the_fp32_cast():
    for c in (c for c in COMBINE_CASES if c.form != "table" and c.n < oc.N_CAP):
        _fails(lambda: oc.check_combine(c, oc.standin_combine(c, "nocast")), c.name + ": out is the fp32 sum of fp32 products by bits")


def test_fault_h_accept_tested_with_less():
    for m in (1, 2):
        c = oc.NormCase(oc.NORM_ERROR, 4, m, data="one")
        assert c in NORM_CASES
        _fails(lambda: oc.check_norm(c, oc.standin_norm(c, "less")), c.name + ": state T .*accepted / rejected, DONE and BAD as constructed failed")
    c = oc.NormCase(oc.NORM_ERROR, 4, 1, data="interior")
    oc.check_norm(c, oc.standin_norm(c, "less"))


def test_fault_i_commit_copies_when_done():
    for n in oc.SMALL_N:
        c = oc.CommitCase(n, 1, 1)
        assert c in COMMIT_CASES
        _fails(lambda: oc.check_commit(c, oc.standin_commit(c, "done")), c.name + ": y keeps its bits .*k1 keeps its bits")


def test_fault_j_fp16_store_not_saturating():
    for c in PACK_CASES[:-1]:
        _fails(lambda: oc.check_pack(c, oc.standin_pack(c, "nosat")), c.name + ": f16 is")
    for c in (c for c in UNET_CASES if c.kind == "cat" and c.f16):
        _fails(lambda: oc.check_unet(c, oc.standin_unet(c, "nosat")), c.name + ": f16")


def test_fault_copies():
    c = next(c for c in STACK_CASES if c.R == 16)
    _fails(lambda: oc.check_stack(c, oc.standin_stack(c, "reg0")), c.name + ": xs is")
    c = COPY_COLS_CASES[0]
    _fails(lambda: oc.check_copy_cols(c, oc.standin_copy_cols(c, "ld")), "copycols-r5-c7-ld10: ")


def test_one_dropped_element_of_a_million_fails_the_sum():
    """A dropped element moves the sum by about 1e-6 relative: far under every end-to-end bound, far over (n + 2) 2^-53."""
    c = next(c for c in NORM_CASES if c.n == oc.N_NORM_CAP and c.mode == oc.NORM_ERROR)
    got = oc.standin_norm(c)
    a, b = oc.norm_sums(c, oc.norm_inputs(c))
    p, _ = oc.norm_terms32(c, oc.norm_inputs(c))
    got["slab"][2 * 5] -= float(p[5 * 1024 + 3]) ** 2
    rel = float(p[5 * 1024 + 3]) ** 2 / float(a.sum())
    assert rel < 1e-5
    _fails(lambda: oc.check_norm(c, got), c.name + r": slab lane 0 against the fp64 sum of the fp32 terms \[norm_error_sum\]")


def test_an_unwritten_slab_entry_fails_where_the_sum_is_not_finite():
    for d in ("nan", "inf"):
        c = oc.NormCase(oc.NORM_ERROR, 4, 1, data=d)
        got = oc.standin_norm(c)
        oc.check_norm(c, got)
        got["slab"][1] = oc.sent64(1)[0]
        _fails(lambda: oc.check_norm(c, got), c.name + ": every slab entry is written failed")
