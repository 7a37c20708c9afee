"""The block-gradient checks bite (tests/block_check.py; no GPU): the "device" here is the bf16-backward stand-in run in fp32, which
must pass every bound of its case against the fp64 reference, and planted faults of the kinds a backward can have -- a wrong tile, a
dropped tail, swapped slabs, a batch row or a layer read from the wrong place -- must fail the block bound.

What a fault does to the whole-tensor error is geometry: a block scaled by 1 + e adds e * sqrt(its share of the tensor's energy), a
zeroed block sqrt(its share), two swapped blocks of unrelated content about sqrt(2 * their share).  HIDDEN faults are planted in
tensors large enough that this footprint lies under the whole-tensor bound 8 * S_case (3.5 - 4.3 % here): there the test asserts BOTH
that the block bound catches the fault and that the whole-tensor bound does not -- the gap this suite closes.  The footprints:
  one 16 x 64 block x 1.3 of >= 256 blocks: <= 0.3 / 16 = 1.9 %;   one 7 x 64 tail block of x's 567 x 1024 gradient zeroed: 2.8 % (at
  dim 512 it would be 3.9 %, over the bound: the case is the dim-1024 one);   the 16 x 21 / 16 x 42 column tail of ff.3's weight
  gradient zeroed: sqrt(336 / (512 * 1365)) = 2.2 % / 1.6 %, the 10-row tail of ff.0's: 2.1 %;   two blocks of ff.0's 5460 x 1024 weight gradient swapped: sqrt(4 / 5472) =
  2.7 % (at dim 512, 1368 blocks: 5.4 %, over the bound; to_qkv at dim 1024, 3072 blocks: 3.6 %, under the model path's 4.3 %).
GROSS faults (a batch row of dx, a layer's whole weight gradient, a tensor of one block) move the whole tensor too; for them the test
asserts what is new, that the block bound fails and names the tensor."""
import functools

import pytest
import torch

import block_check as bc

CASES = {c.name: c for c in (
    bc.Case("stack", 512, 3, 189, True),
    bc.Case("stack", 1024, 3, 189, True),
    bc.Case("stack", 512, 1, 8, False),
    bc.Case("model", 512, 3, 189, True),
    bc.Case("model", 1024, 3, 189, True),
)}
S512, S1024, M512, M1024 = "stack-dim512-3x189-masked", "stack-dim1024-3x189-masked", "model-dim512-3x189-masked", "model-dim1024-3x189-masked"


@functools.lru_cache(maxsize=None)
def _reference(name):
    return bc.reference(CASES[name])


@functools.lru_cache(maxsize=None)
def _device(name):
    """the stand-in in fp32: (forward, gradients)"""
    return bc.oracle_grads(CASES[name], dtype=torch.float32, standin=True)


@pytest.mark.parametrize("name", list(CASES))
def test_condition_s_case_is_under_the_cap(name):
    r = _reference(name)
    print(f"{name}: s_case {r.s_case:.5f} S_case {r.S_case:.5f} oracle + stand-in {r.seconds:.1f} s")
    assert 0 < r.s_case <= bc.S_CASE_CAP, (name, r.s_case)  # no block bound exceeds 10 %
    assert r.S_case > 0


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_standin_passes_every_bound(name):
    case, r = CASES[name], _reference(name)
    fwd, got = _device(name)
    bc.check(name, bc.errors(got, r.grads), r.s_case, r.S_case)
    if case.path == "stack":
        assert bc.rel(fwd, r.forward) < bc.Y_REL
    else:
        assert abs(float(fwd) - bc.loss32_emulated(case)) < bc.LOSS_ABS


def test_every_gradient_is_covered():
    """every floating-point parameter of the state dict (null_cond aside, which no unconditional loss reaches) has a reference gradient
    that is not zero, and the stack path adds x and cond"""
    for name in (S512, M512):
        case, r = CASES[name], _reference(name)
        want = {k for k, v in bc.inputs(case)["state"].items() if v.is_floating_point() and k != "null_cond" and not k.endswith("inv_freq")}  # (the rotary table is a buffer)
        want |= {"x", "cond"} if case.path == "stack" else set()
        assert set(r.grads) == want, (name, set(r.grads) ^ want)
        assert all(float(g.norm()) > 0 for g in r.grads.values())
        assert {bc.tensor_class(k) for k in r.grads} == set(bc.CLASSES) - ({"embed", "head"} if case.path == "stack" else {"x", "cond"})


# ----------------------------------------------------------------------------- planted faults
def _blk(t, i, j):
    """view of block (i, j) of a tensor seen as rows x last dimension (negative indices count from the end)"""
    m = t.reshape(1, -1) if t.ndim <= 1 else t.reshape(-1, t.shape[-1])
    nr, nc = -(-m.shape[0] // bc.BLOCK_ROWS), -(-m.shape[1] // bc.BLOCK_COLS)
    i, j = i % nr, j % nc
    return m[i * bc.BLOCK_ROWS:(i + 1) * bc.BLOCK_ROWS, j * bc.BLOCK_COLS:(j + 1) * bc.BLOCK_COLS]


def _interior(t):
    m = bc.as_rows(t)
    return (-(-m.shape[0] // bc.BLOCK_ROWS)) // 2, (-(-m.shape[1] // bc.BLOCK_COLS)) // 2


def scale_interior_block(t):
    _blk(t, *_interior(t)).mul_(1.3)


def zero_last_row_tail(t):
    b = _blk(t, -1, 1)
    assert b.shape[0] < bc.BLOCK_ROWS  # a tail
    b.zero_()


def zero_last_col_tail(t):
    b = _blk(t, 1, -1)
    assert b.shape[1] < bc.BLOCK_COLS
    b.zero_()


def swap_two_row_blocks(t):
    i, j = _interior(t)
    a, b = _blk(t, i, j), _blk(t, i + 1, j)
    tmp = a.clone()
    a.copy_(b)
    b.copy_(tmp)


def _l(case_name, key):
    return "transformer." + key if CASES[case_name].path == "model" and key.startswith("layers.") else key


HIDDEN = [
    # (fault, case, tensor): one interior block x 1.3 over a representative tensor of every class with a tensor of >= 256 blocks
    (scale_interior_block, S512, "layers.0.3.to_qkv.weight"),
    (scale_interior_block, S1024, "layers.1.3.to_out.weight"),
    (scale_interior_block, S512, "layers.0.5.0.weight"),
    (scale_interior_block, S1024, "layers.1.5.3.weight"),
    (scale_interior_block, S512, "x"),
    (scale_interior_block, M512, "layers.1.2.to_gamma.weight"),
    (scale_interior_block, M1024, "layers.0.4.to_beta.weight"),
    (scale_interior_block, M512, "layers.1.3.to_qkv.weight"),
    (scale_interior_block, M512, "to_embed.weight"),
    (scale_interior_block, M512, "sinu_pos_emb.1.weight"),
    (scale_interior_block, M512, "to_pred.weight"),
    # one tail block zeroed: the last rows of x's gradient, the last 21 (dim 512) / 42 (dim 1024) columns of ff.3's weight gradient
    # (inner width 1365 / 2730: the columns the kernels pad to 1408 / 2752), the last 10 rows of ff.0's
    (zero_last_row_tail, S1024, "x"),
    (zero_last_col_tail, S512, "layers.0.5.3.weight"),
    (zero_last_col_tail, M1024, "layers.1.5.3.weight"),
    (zero_last_row_tail, M512, "layers.0.5.0.weight"),
    # two row blocks of a weight gradient swapped
    (swap_two_row_blocks, S1024, "layers.0.5.0.weight"),
    (swap_two_row_blocks, M1024, "layers.1.5.0.weight"),
    (swap_two_row_blocks, M1024, "layers.0.3.to_qkv.weight"),
]


@pytest.mark.parametrize("fault,name,key", HIDDEN, ids=[f"{f.__name__}-{n}-{k}" for f, n, k in HIDDEN])
def test_hidden_fault_fails_the_block_bound_and_only_that(fault, name, key):
    r = _reference(name)
    key = key if key in ("x", "cond") else _l(name, key)
    got = _device(name)[1][key].clone()
    fault(got)
    e = bc.tensor_err(got, r.grads[key])
    print(f"{fault.__name__} {name} {key}: block {e.worst:.3f} at {e.where} (bound {bc.FACTOR * r.s_case:.3f}), "
          f"whole {e.whole:.4f} (bound {bc.FACTOR * r.S_case:.4f})")
    assert e.worst > bc.FACTOR * r.s_case, "the block bound misses the fault"
    assert e.whole < bc.FACTOR * r.S_case, "the fault is not hidden from the whole-tensor bound: the wrong tensor for this test"
    bad = bc.violations({key: e}, r.s_case, r.S_case)
    assert [b[:2] for b in bad] == [("block", key)]


def batch_row_1_from_row_0(g):
    g["x"][1].copy_(g["x"][0])
    return "x"


def layer_0_qkv_from_layer_1(g):
    k0 = next(k for k in g if k.endswith("layers.0.3.to_qkv.weight"))
    g[k0].copy_(g[k0.replace("layers.0.", "layers.1.")])
    return k0


def scale_q_norm_gamma(g):
    k = next(k for k in g if k.endswith("layers.1.3.q_norm.gamma"))
    g[k].mul_(1.3)
    return k


def scale_one_block_of_a_bias(g):
    k = next(k for k in g if k.endswith("layers.0.4.to_gamma.bias"))
    _blk(g[k], 0, 3).mul_(1.3)
    return k


def zero_registers_column_block(g):
    k = next(k for k in g if k.endswith("register_tokens"))
    _blk(g[k], 0, -1).zero_()
    return k


GROSS = [(batch_row_1_from_row_0, S512), (batch_row_1_from_row_0, S1024), (layer_0_qkv_from_layer_1, S512), (layer_0_qkv_from_layer_1, M1024),
         (scale_q_norm_gamma, S512), (scale_q_norm_gamma, M512), (scale_one_block_of_a_bias, M512), (zero_registers_column_block, M1024),
         (scale_q_norm_gamma, "stack-dim512-1x8")]


@pytest.mark.parametrize("fault,name", GROSS, ids=[f"{f.__name__}-{n}" for f, n in GROSS])
def test_gross_fault_fails_the_block_bound(fault, name):
    r = _reference(name)
    got = {k: v.clone() for k, v in _device(name)[1].items()}
    key = fault(got)
    bad = bc.violations(bc.errors(got, r.grads), r.s_case, r.S_case)
    print(f"{fault.__name__} {name}: {[(b[0], b[1], b[2], round(b[3], 3)) for b in bad]}")
    assert ("block", key) in [b[:2] for b in bad]
    assert {b[1] for b in bad} == {key}  # and it names that tensor alone
    with pytest.raises(AssertionError):
        bc.check(name, bc.errors(got, r.grads), r.s_case, r.S_case, verbose=False)


# ----------------------------------------------------------------------------- the metric itself
def test_block_metric_on_known_tensors():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(40, 150, generator=g, dtype=torch.float64)  # 3 x 3 blocks: 16 / 16 / 8 rows, 64 / 64 / 22 columns
    assert bc.block_numel(40, 150).tolist() == [[1024., 1024., 352.], [1024., 1024., 352.], [512., 512., 176.]]
    e = bc.tensor_err(ref, ref)
    assert e.blocks.shape == (3, 3) and e.worst == 0 and e.whole == 0
    got = ref.clone()
    got[32:, 128:] *= 1.3  # the corner tail, 8 x 22
    e = bc.tensor_err(got, ref)
    assert e.where == (2, 2) and abs(e.worst - 0.3) < 1e-12 and float(e.blocks.sum()) == e.worst
    # a block that is legitimately near zero is measured against half a typical block of ITS size, not against nothing
    ref2 = ref.clone()
    ref2[32:, 128:] = 0
    got2 = ref2.clone()
    got2[32:, 128:] = 1e-3
    e = bc.tensor_err(got2, ref2)
    rms = float(ref2.norm()) / ref2.numel() ** 0.5
    assert abs(e.worst - 1e-3 * 176 ** 0.5 / (0.5 * rms * 176 ** 0.5)) < 1e-12
    # 1-D: one row, blocks of 1 x 64; 3-D: rows x last dimension
    assert bc.tensor_err(torch.ones(130), torch.ones(130)).blocks.shape == (1, 3)
    assert bc.tensor_err(torch.ones(16, 1, 64), torch.ones(16, 1, 64)).blocks.shape == (1, 1)
    assert bc.tensor_err(torch.ones(3, 189, 512), torch.ones(3, 189, 512)).blocks.shape == (36, 8)
    # an all-zero reference: zero passes, anything else cannot
    assert bc.tensor_err(torch.zeros(5), torch.zeros(5)).worst == 0
    assert bc.tensor_err(torch.full((5,), 1e-9), torch.zeros(5)).worst == float("inf")
    with pytest.raises(AssertionError):
        bc.tensor_err(torch.full((5,), float("nan")), torch.ones(5))
    with pytest.raises(AssertionError):
        bc.errors({}, {"w": torch.ones(5)})


def test_yardstick_restores_the_oracle_and_leaves_the_forward_alone():
    from oracle import restate

    orig = restate._op
    with pytest.raises(RuntimeError):
        with bc.bf16_backward():
            assert restate._op is not orig
            raise RuntimeError
    assert restate._op is orig
    case = CASES["stack-dim512-1x8"]
    y_ref, g_ref = bc.oracle_grads(case)
    y_std, g_std = bc.oracle_grads(case, standin=True)
    assert torch.equal(y_ref, y_std)  # the forward is untouched
    assert any(not torch.equal(g_ref[k], g_std[k]) for k in g_ref)
    # `reference` back-propagates ONE graph twice, the rounding points passing the gradient through the first time: that is the plain
    # oracle's backward bit for bit, and its yardstick is the separate stand-in pass's
    r = bc.reference(case)
    assert set(r.grads) == set(g_ref) and all(torch.equal(r.grads[k], g_ref[k]) for k in g_ref)
    assert torch.equal(r.forward, y_ref) and (r.s_case, r.S_case) == bc.yardstick(g_std, g_ref)
    assert bc._ROUND["on"]
    x = torch.randn(4, 4, dtype=torch.float64, requires_grad=True)
    with bc.bf16_backward():
        (restate._op(x) * torch.full((4, 4), 1.001, dtype=torch.float64)).sum().backward()
    assert torch.equal(x.grad, torch.full((4, 4), 1.0, dtype=torch.float64))  # bf16(1.001) = 1
