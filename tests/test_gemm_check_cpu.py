"""The checks of the GEMM edge tests (tests/gemm_check.py) checked on the CPU: a correct result -- an fp32 product of the same operands
through the epilogue in fp32, rounded once -- passes every bound of every case, so the bounds are reachable before anything runs on a
device; planted faults fail; and the two faults a ragged tile typically produces pass the global rel_err bound of
tests/test_ops_gpu.py::test_gemm_nt_bf16_f32 at one of its own shapes, which is why these checks exist."""
import pytest
import torch

import gemm_check as gc
from gemm_check import CASES, GROUPED_JOBS, Case

ALL = CASES + GROUPED_JOBS
# the faults are planted in every case of up to 2^18 output elements: every kernel, mode and epilogue of the table, both layouts
SMALL = [c for c in ALL if c.M * c.N <= 1 << 18]


def test_the_table_reaches_every_kernel_and_epilogue_with_ragged_edges():
    """Every kernel has, per epilogue it serves, a case with a ragged M, a ragged N and a K tail at its own tile."""
    tile = {gc.BM64: (64, 128, 32), gc.BM128: (128, 128, 32), gc.BM160: (160, 128, 64), gc.GEMM3: (256, 256, 64), gc.GEMM4: (128, 256, 32)}
    serves = {k: {gc.EPI_BF16, gc.EPI_F32, gc.EPI_QKV, gc.EPI_GEGLU} for k in tile}
    for k in (gc.BM64, gc.BM128, gc.BM160):
        serves[k] = serves[k] | {gc.EPI_GELU}
    serves[gc.BM128] = serves[gc.BM128] | {gc.EPI_SPLITK}
    serves[gc.GEMM3] = serves[gc.GEMM3] | {gc.EPI_SPLITK}
    for k, (bm, bn, bk) in tile.items():
        for e in serves[k]:
            mine = [c for c in CASES if c.kernel == k and c.epi == e]
            kt = (lambda c: c.K % 64) if e == gc.EPI_SPLITK else (lambda c: c.K % bk)
            whole_n = bn == 128 and e in (gc.EPI_QKV, gc.EPI_GEGLU)  # N is a multiple of 384 / 128 by the epilogue's own layout
            assert any(c.M % bm and (c.N % bn or whole_n) and kt(c) for c in mine), (k, e)
            assert {c.strided for c in mine} == {False, True}, (k, e)
    for e in (gc.EPI_BF16, gc.EPI_QKV, gc.EPI_GEGLU):  # gemm5: K is 512; ragged 32-row blocks, a last panel with idle waves
        mine = [c for c in CASES if c.kernel == gc.GEMM5 and c.epi == e]
        assert any(c.M % 32 and (c.N // 64) % 4 for c in mine) and {c.cu_limit for c in mine} == {0, 1, 2}
    assert len({c.name for c in ALL}) == len(ALL)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_a_correct_result_passes_every_bound(case):
    built = gc.build(case)
    gc.check(built, gc.fill(built, gc.standin(case)))


def _target(built):
    """The output the faults are planted in: the first linear output, or a fused case's first fp16 output (C otherwise)."""
    for n, spec in built.outs.items():
        if spec.dtype == torch.float16:
            return n
    return next(iter(built.outs))


def _fails(built, res, what):
    with pytest.raises(AssertionError, match=what):
        gc.check(built, res, label="planted")


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_planted_faults_fail(case):
    built = gc.build(case)
    good = gc.fill(built, gc.standin(case))
    ref, S = gc.reference(case)
    n = _target(built)
    spec = built.outs[n]
    linear = S is not None

    def fresh():
        res = {k: v.clone() for k, v in good.items()}
        return res, spec.view(res[n])

    # one row of the last partial tile scaled by 1.01.  A block check sees 0.01 / sqrt(rows of the block): above the fp16 tolerance
    # for any block, above the bf16 one (beside ~2e-3 of rounding) only in a tail block of one or two rows
    tail_rows = (case.M - 1) % gc.BLOCK_ROWS + 1
    if linear or spec.dtype == torch.float16 or tail_rows <= 2:
        res, v = fresh()
        row = case.M - 1 if linear else spec.rows - 1  # (split-K: the last row of the first slab, never an empty one)
        v[row] = (v[row].float() * 1.01).to(spec.dtype)
        _fails(built, res, rf"{n} \[")
    # one 8-column tail zeroed (GEGLU: the last 8 columns that carry weights; those behind them are zero anyway)
    res, v = fresh()
    hi = gc.geglu_fd(case) if case.epi == gc.EPI_GEGLU else spec.cols
    v[:, max(hi - 8, 0):hi] = 0
    _fails(built, res, rf"{n} \[")
    # one element of a 16-bit linear output off by 4 of its ulps (an fp32 output may legitimately differ by that: summation order)
    n16 = next((k for k, s in built.outs.items() if s.dtype != torch.float32), None)
    if linear and n16:
        res, _ = fresh()
        s16 = built.outs[n16]
        i = int(ref[n16].abs().argmax())
        res[n16].view(torch.int16)[(i // s16.cols) * s16.ld + i % s16.cols] += 4  # sign-magnitude: four ulps away from zero
        _fails(built, res, rf"{n16} \[")
    # one sentinel element overwritten: the row after the last, and a column between N and ldc where there is one
    res, _ = fresh()
    res[n][-1] = 0
    _fails(built, res, f"{n} sentinel")
    if spec.ld > spec.cols:
        res, _ = fresh()
        res[n][spec.cols] = 0
        _fails(built, res, f"{n} sentinel")
    # one NaN inside the extent
    res, v = fresh()
    v[0, 0] = float("nan")
    _fails(built, res, f"{n} finite")
    # an empty split's slab left as it was allocated
    if case.epi == gc.EPI_SPLITK:
        for s, (kb, ke) in enumerate(gc.split_ranges(case.K, case.splits)):
            if ke == kb:
                res, _ = fresh()
                slab = built.outs["slabs"]
                slab.view(res["slabs"])[s * case.M:(s + 1) * case.M] = slab.view(slab.new())[:case.M]
                _fails(built, res, "slabs finite")


def test_some_case_has_an_empty_split():
    assert any(ke == kb for c in ALL if c.epi == gc.EPI_SPLITK for kb, ke in gc.split_ranges(c.K, c.splits))
    assert gc.split_ranges(72, 3) == [(0, 64), (64, 72), (72, 72)]


@pytest.fixture(scope="module")
def old_shape():
    """(8200, 512, 64) of test_ops_gpu.py::test_gemm_nt_bf16_f32: bf16 output with a bias, checked there by rel_err < 4e-3."""
    case = Case(gc.BM64, 0, gc.NT, gc.EPI_BF16, 8200, 512, 64, bias=True)
    built = gc.build(case)
    return case, built, gc.fill(built, gc.standin(case)), gc.reference(case)[0]["C"]


def test_a_wrong_tail_row_passes_the_old_metric_and_fails_here(old_shape):
    case, built, good, ref = old_shape
    res = {"C": good["C"].clone()}
    v = built.outs["C"].view(res["C"])
    v[case.M - 1] = (v[case.M - 1].float() * 1.01).to(torch.bfloat16)  # the one row of the last 128-row tile (8200 = 64 x 128 + 8 ...)
    assert gc.rel_err(v, ref) < 4e-3  # test_gemm_nt_bf16_f32's bound: accepted
    _fails(built, res, r"C \[bf16\] error / bound at \(8199, ")


def test_a_missing_tail_store_passes_the_old_metric_and_fails_here(old_shape):
    case, built, good, ref = old_shape
    res = {"C": good["C"].clone()}
    v = built.outs["C"].view(res["C"])
    v[case.M - 1, case.N - 8:] = 0  # one 16-byte store of the last row's 8-column tail never made
    assert gc.rel_err(v, ref) < 4e-3
    _fails(built, res, r"C \[bf16\] error / bound at \(8199, 5")


def test_block_errors_rules():
    """The floor, exact-zero and NaN rules of attn_check.tile_errors, in two dimensions."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(70, 130, generator=g, dtype=torch.float64)
    ref[:, 128:] = 0  # a block whose reference is exactly zero
    e = gc.block_errors(ref, ref)
    assert e.shape == (3, 3) and float(e.max()) == 0.0
    got = ref.clone()
    got[64:, :64] *= 1.5
    e = gc.block_errors(got, ref)
    assert abs(float(e[2, 0]) - 0.5) < 1e-12 and float(e.sum()) == float(e[2, 0])
    got = ref.clone()
    got[3, 129] = 1e-30
    assert float(gc.block_errors(got, ref)[0, 2]) == float("inf")
    got[40, 70] = float("nan")
    e = gc.block_errors(got, ref)
    assert bool(torch.isnan(e[1, 1])) and float(e[0, 2]) == float("inf")
    tiny = ref.clone()
    tiny[:32, :64] *= 1e-9  # a nearly-zero block is measured against the floor, not against itself
    got = tiny.clone()
    got[:32, :64] *= 2
    assert float(gc.block_errors(got, tiny)[0, 0]) < 1e-5


def test_unit_roundoffs():
    for dt, u in gc.U_OUT.items():
        assert u == torch.finfo(dt).eps / 2  # round to nearest: half the spacing above 1
    one = torch.tensor(1.0)
    assert float((one + 2.0 ** -8).to(torch.bfloat16)) == 1.0 and float((one + 1.5 * 2.0 ** -8).to(torch.bfloat16)) == 1.0 + 2.0 ** -7
