"""The checks of the optimizer edge tests (tests/optim_check.py) checked on the CPU: the fp32 stand-in -- the kernels' arithmetic in
torch float32 -- passes every bound of every case, so the counted bounds are reachable before anything runs on a device; and each
planted fault, of the kind these kernels can have without a model-level test noticing, fails a case that is named here."""
import pytest
import torch

import optim_check as oc
from optim_check import (CHAIN_STEPS, CLIP_CASES, EXPAND_SHAPES, FACTOR_CASES, GRAM_CASES, PACKED_CASES, RANGES_CASES, SUMSQ_CASES, TABLES,
                         FactorCase, PackedCase)


def _fails(fn, what):
    with pytest.raises(AssertionError, match=what):
        fn()


# ------------------------------------------------------------------------------------------------ the cases cover what they claim
def test_tables_hold_every_form_and_both_arms():
    segs = [s for t in TABLES.values() for s in t.segs]
    packed = [s for s in segs if s["dst_bf16"] or s["dst_f16"] or s["dst_f32"]]

    def vec(s):
        return s["off"] % 4 == 0 and (s not in packed or (s["cols"] % 4 == 0 and s["dst_ld"] % 4 == 0))

    counts = {s["count"] for s in segs if s not in packed}
    assert {2 * 2048 + 1, 1024, 1028, 7} <= counts
    assert any(s["count"] == 7 and s["off"] % 2 == 1 for s in segs)
    for shape, ld in (((5, 12), 16), ((5, 10), 12), ((5, 8), 10)):
        assert any(s["cols"] == shape[1] and s["count"] == shape[0] * shape[1] and s["dst_ld"] == ld and s["dst_bf16"] and s["dst_f16"] for s in packed)
    # each condition of the vector arm fails on its own somewhere, and the arm itself runs with and without copies
    assert any(vec(s) for s in packed) and any(vec(s) for s in segs if s not in packed)
    assert any(s["off"] % 4 and s["cols"] % 4 == 0 and s["dst_ld"] % 4 == 0 for s in packed)
    assert any(s["off"] % 4 == 0 and s["cols"] % 4 and s["dst_ld"] % 4 == 0 for s in packed)
    assert any(s["off"] % 4 == 0 and s["cols"] % 4 == 0 and s["dst_ld"] % 4 for s in packed)
    kinds = {(bool(s["dst_bf16"]), bool(s["dst_f16"]), bool(s["dst_f32"])) for s in packed if s["rowmap"] != 2}
    assert kinds == {(True, True, False), (True, False, False), (False, True, False), (False, False, True)}
    assert any(s["rowmap"] == 1 and s["cols"] == 8 and s["F"] == 70 and s["count"] == 140 * 8 for s in packed)
    assert any(s["rowmap"] == 1 and s["cols"] == 1 and s["dst_f32"] for s in packed)  # the GEGLU bias
    assert any(s["rowmap"] == 1 and s["count"] > 2048 and vec(s) for s in packed)
    assert any(s["dst_f32"] and s["cols"] == s["count"] == 37 for s in packed)
    assert any(s["dst_ld"] > s["cols"] and vec(s) for s in packed) and any(s["dst_ld"] > s["cols"] and not vec(s) for s in packed)
    for t in TABLES.values():  # a zero-block entry in the middle and at the end
        z = [i for i, s in enumerate(t.segs) if s["rowmap"] == 2]
        assert z and z[-1] == len(t.segs) - 1 and z[0] < len(t.segs) - 1
        assert t.segs[-1]["block0"] == t.total_blocks and t.segs[z[0]]["block0"] == t.segs[z[0] + 1]["block0"]
        assert not t.covered()[: t.n].all()  # gaps
        t.dst_map()  # no destination element mapped twice, every guard row free
    # the one-row piece dp.filter_adam_segments cut: odd offset, shifted destination, cols = b - a
    e = TABLES["edges"]
    piece = [s for s in e.segs if s["dst_f32"] and s["cols"] == 20]
    assert len(piece) == 1 and piece[0]["off"] % 2 == 1 and piece[0]["count"] == 20 and e.resolve(piece[0]["dst_f32"])[1] == 21
    assert any(s["dst_f32"] and s["cols"] == 3 and e.resolve(s["dst_f32"]) == e.resolve(piece[0]["dst_f32"] - 21 * 4) for s in e.segs)


def test_block_numbering_is_the_filter_s_own():
    from voicebox_pytorch_amd.dp import filter_adam_segments

    for t in TABLES.values():
        same, blocks = filter_adam_segments([dict(s) for s in t.segs], [])
        assert blocks == t.total_blocks and [s["block0"] for s in same] == [s["block0"] for s in t.segs]


def test_interleave_restatement():
    """64 rows of the first half, then 64 of the second, per 128; F = 70 needs 256 destination rows and pads 116 of them"""
    F = 70
    rows = [oc.dest_row(r, 1, F) for r in range(2 * F)]
    assert rows[:64] == list(range(64)) and rows[64:70] == list(range(128, 134))
    assert rows[70:134] == list(range(64, 128)) and rows[134:] == list(range(192, 198))
    assert len(set(rows)) == 2 * F and max(rows) < 256


def test_sum_geometry():
    assert oc.sumsq_k(4 * 256 * 1024 + 3, 0) == 4 and oc.sumsq_k(1031, 1) == 1 and oc.sumsq_k(1, 0) == 1
    by = {c.name: c for c in RANGES_CASES}
    assert oc.ranges_k(by["ranges-across-x0"]) == 1 and oc.ranges_k(by["ranges-empties-x5000"]) == 6
    assert sum(hi - lo for lo, hi in by["ranges-under256-x0"].ranges) < 4 * 256
    assert {c.n_extra for c in RANGES_CASES} == {0, 1, 1023, 1025, 4097, 5000}
    assert len({c.name for c in RANGES_CASES}) == len(RANGES_CASES) and all(len(c.ranges) <= 64 for c in RANGES_CASES)


# ------------------------------------------------------------------------------------------------ the stand-in passes every bound
@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: c.name)
def test_standin_passes_packed(case):
    inp = oc.packed_inputs(case)
    z = (inp["g"] == 0) & (inp["m"] == 0) & (inp["v"] == 0)
    assert int(z.sum()) > 100 and int(((inp["v"] == 0) & (inp["g"] != 0)).sum()) > 100  # the planted zeros are there
    oc.check_packed(case, oc.standin_packed(case))


@pytest.mark.parametrize("case", FACTOR_CASES, ids=lambda c: c.name)
def test_standin_passes_factor(case):
    oc.check_factor(case, oc.standin_factor(case))


@pytest.mark.parametrize("sh", EXPAND_SHAPES, ids=oc.expand_name)
def test_standin_passes_expand(sh):
    oc.check_expand(sh, oc.standin_expand(sh))


@pytest.mark.parametrize("n,off", SUMSQ_CASES)
def test_standin_passes_sumsq(n, off):
    oc.check_sumsq(n, off, oc.standin_sumsq(n, off))


@pytest.mark.parametrize("case", RANGES_CASES, ids=lambda c: c.name)
def test_standin_passes_ranges(case):
    oc.check_ranges(case, oc.standin_ranges(case))


@pytest.mark.parametrize("sh", GRAM_CASES, ids=oc.gram_name)
def test_standin_passes_gram(sh):
    oc.check_gram(sh, oc.standin_gram(*oc.gram_inputs(sh)))


@pytest.mark.parametrize("case", CLIP_CASES, ids=oc.clip_name)
def test_standin_passes_clip(case):
    oc.check_clip(case, oc.standin_clip(*case))


def _run_chain(fault=None, upto=CHAIN_STEPS):
    state = oc.chain_initial()
    for step in range(1, upto + 1):
        got = oc.standin_chain_step(step, state, fault)
        oc.check_chain_step(step, state, got)
        state = {k: got[k] for k in "pmv"}


def test_standin_passes_the_chain():
    _run_chain()


# ------------------------------------------------------------------------------------------------ planted faults
GS = oc.GSCALES[1]


def test_fault_gscale_ignored():
    c = PackedCase("edges", 2, GS)
    _fails(lambda: oc.check_packed(c, oc.standin_packed(c, "gscale")), r"packed-edges-step2-gs: .*m \[adam_m\].*v \[adam_v\]")
    f = FactorCase(2, 3, 13, 1028, 2, GS, "all")
    _fails(lambda: oc.check_factor(f, oc.standin_factor(f, "gscale")), r"factor-L2-B3-J13-Th1028-step2-gs-dst_all: .*\[factor_m\]")
    # step 1 from m = v = 0, p alone: the scale cancels -- the chain sees it in m and v
    _fails(lambda: _run_chain("gscale", 1), r"chain-step1: .*m \[adam_m\].*v \[adam_v\]")


def test_fault_gscale_passes_the_one_step_update_metric_and_fails_here():
    """Why the model-level comparison (one step from m = v = 0, the update's Frobenius ratio under 2e-2 per tensor) cannot see the clip
    coefficient: with the coefficient ignored the update differs by 1.2e-4 -- the scale cancels up to eps -- while m and v are off by
    the coefficient and its square."""
    state = oc.chain_initial()
    good, bad = oc.standin_chain_step(1, state), oc.standin_chain_step(1, state, "gscale")
    cov = oc.chain_covered()
    upd, upd_bad = (good["p"] - state["p"])[cov].double(), (bad["p"] - state["p"])[cov].double()
    assert float((upd_bad - upd).norm() / upd.norm()) < 2e-2  # that test's bound: accepted
    _fails(lambda: oc.check_chain_step(1, state, bad), r"m \[adam_m\] error / bound at \(\d+,\) = \d\.\d+e\+0[5-9]")


def test_fault_bc2_from_beta1():
    c = PackedCase("forms", 2, None)
    _fails(lambda: oc.check_packed(c, oc.standin_packed(c, "bc2")), r"packed-forms-step2-nogs: p \[adam_p\]")
    f = FactorCase(3, 9, 8, 260, 2, None, "all")
    _fails(lambda: oc.check_factor(f, oc.standin_factor(f, "bc2")), r"factor-L3-B9-J8-Th260-step2-nogs-dst_all: .*\[factor_p\]")


def test_fault_ragged_tail_left_unupdated():
    c = PackedCase("edges", 1, None)
    _fails(lambda: oc.check_packed(c, oc.standin_packed(c, "tail")), r"packed-edges-step1-nogs: p \[adam_p\]")


def test_fault_rowmap_row_off_by_one():
    c = PackedCase("forms", 1, GS)
    _fails(lambda: oc.check_packed(c, oc.standin_packed(c, "rowmap")), r"packed-forms-step1-gs: s\d+\.bf16 is round-to-nearest-even of the stored p failed")


def test_fault_copy_truncated():
    c = PackedCase("edges", 1000, GS)
    _fails(lambda: oc.check_packed(c, oc.standin_packed(c, "trunc")), r"packed-edges-step1000-gs: s\d+\.bf16 is round-to-nearest-even of the stored p failed")


def test_fault_last_batch_row_dropped():
    f = FactorCase(2, 3, 13, 1028, 1, None, "all")
    _fails(lambda: oc.check_factor(f, oc.standin_factor(f, "lastb")), r"factor-L2-B3-J13-Th1028-step1-nogs-dst_all: .*\[factor_m\]")
    sh = (17, 9, 8)
    _fails(lambda: oc.check_expand(sh, oc.standin_expand(sh, "lastb")), r"expand-B17-J9-Th8: dw \[expand_dw\]")


def test_fault_last_float4_of_a_range_skipped():
    c = next(c for c in RANGES_CASES if c.name == "ranges-r64-x0")
    _fails(lambda: oc.check_ranges(c, oc.standin_ranges(c, "float4")), r"ranges-r64-x0: sum \[sumsq_ranges\]")


def test_fault_one_extra_term_dropped():
    c = next(c for c in RANGES_CASES if c.name == "ranges-empties-x4097")
    _fails(lambda: oc.check_ranges(c, oc.standin_ranges(c, "extra")), r"ranges-empties-x4097: sum \[sumsq_ranges\]")


def test_fault_clip_without_1e_6():
    c = CLIP_CASES[-1]  # (at a norm of 2 the term is 5e-7 of the coefficient, 8 u: inside the margin; here it is a tenth)
    _fails(lambda: oc.check_clip(c, oc.standin_clip(*c, fault="1e-6")), r"clip-ss1e-10-max1e-06-iw1: coef\[0\] \[clip_coef\]")


def test_fault_inv_world_applied_twice():
    c = next(c for c in CLIP_CASES if c[2] == 0.125 and c[1] > 0)
    _fails(lambda: oc.check_clip(c, oc.standin_clip(*c, fault="inv_world")), r"clip-ss64-max0.5-iw0.125: coef\[0\] \[clip_coef\]")


def test_fault_one_write_into_a_gap():
    c = PackedCase("edges", 1, None)
    _fails(lambda: oc.check_packed(c, oc.standin_packed(c, "gap")), r"packed-edges-step1-nogs: p outside every segment keeps its bits failed")


def test_segment_table_check_sees_an_overlap_and_a_wrong_block0():
    t = TABLES["forms"]
    segs = [dict(s) for s in t.segs]
    n = segs[-1]["off"] + segs[-1]["count"]
    fb = [(s["off"], s["off"] + s["count"]) for s in segs if s["rowmap"] == 2]
    _fails(lambda: oc.check_segment_table(segs, t.total_blocks, n, fb, (0, 1 << 40)), "tile")  # this synthetic table has gaps
    tiled, cur = [], 0
    for s in segs:  # filled as the builder fills them
        if s["off"] > cur:
            tiled.append(dict(off=cur, count=s["off"] - cur, dst_bf16=0, dst_f16=0, dst_f32=0, cols=1, dst_ld=0, rowmap=0, F=0, block0=0))
        tiled.append(s)
        cur = s["off"] + s["count"]
    blocks = oc.number_blocks(tiled)
    oc.check_segment_table(tiled, blocks, n, fb, (0, 1 << 40))
    bad = [dict(s) for s in tiled]
    bad[3]["block0"] += 1
    _fails(lambda: oc.check_segment_table(bad, blocks, n, fb, (0, 1 << 40)), "block0 consistent")
    bad = [dict(s) for s in tiled]
    i = next(i for i, s in enumerate(bad) if s["dst_bf16"] and bad[i + 1]["dst_bf16"])
    bad[i + 1]["dst_bf16"] = bad[i]["dst_bf16"] + 2
    _fails(lambda: oc.check_segment_table(bad, blocks, n, fb, (0, 1 << 40)), "destination extents disjoint")


def test_roundings():
    assert oc.U == torch.finfo(torch.float32).eps / 2
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20])  # above the midpoint: nearest is up, truncation is down
    assert float(x.to(torch.bfloat16)) == 1.0 + 2.0 ** -7 and float(oc.truncate_bf16(x)) == 1.0
