"""CPU side of the Aligner network: the fp64 restatement of tests/aligner_ref.py (forward and hand-written backward) against an
independent construction from nn.Conv1d, the broadcast difference, softmax and autograd; the planted faults and the tolerance the
GPU tests take from them; the direct-form contract of the sum of squares with its two planted faults; and the host logic of
voicebox_pytorch_amd.Aligner / aligner_attention / DurationPredictor that needs no device."""
import pytest
import torch

import aligner_ref as R

import voicebox_pytorch_amd as vbx
from voicebox_pytorch_amd import _lib

TAU = 0.0005
CASES = [(3, 1, 1), (3, 2, 3), (2, 5, 1), (3, 21, 9)]  # B, T, K: the 3-tap edges at T = 1 and 2


def _case(B, T, K, seed=5, dims=(16, 24, 8)):
    sd = R.init_state(*dims, seed, TAU)
    queries, keys = R.make_inputs(B, T, K, dims[0], dims[1], seed + 1)
    return sd, queries, keys


def _torch_module(sd, dims):
    m = R.torch_module(*dims).double()
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    return m


@pytest.mark.parametrize("B,T,K", CASES)
def test_restatement_equals_the_torch_construction(B, T, K):
    dims = (16, 24, 8)
    sd, queries, keys = _case(B, T, K)
    m = _torch_module(sd, dims)
    for variant in R.variants(B) + [None]:
        if variant is None:
            klens, qlens, mask = [K] * B, [T] * B, None
        else:
            klens, qlens = R.lengths(B, T, K, variant)
            mask = R.mask_of(klens, K)
        attn, lp = R.forward(sd, queries, keys, mask, TAU)
        with torch.no_grad():
            ta, tl = R.torch_forward(m, queries.double(), keys.double(), mask, TAU)
        assert float((attn - ta).abs().max()) <= 1e-12
        assert float((lp - tl).abs().max()) <= 1e-12 * max(1.0, float(tl.abs().max()))
        if mask is not None:
            assert float(attn[~mask[:, None, None, :].expand_as(attn) & mask.any(1)[:, None, None, None]].abs().sum()) == 0.0
            dead = ~mask.any(1)
            if bool(dead.any()):
                assert torch.equal(attn[dead], torch.full_like(attn[dead], 1.0 / K))
        # the hand-written backward against autograd through torch's own layers
        mine = R.reference(sd, queries, keys, klens, qlens, TAU)
        auto = R.reference_autograd(sd, queries, keys, klens, qlens, TAU, module=m)
        assert abs(float(mine["loss"] - auto["loss"])) <= 1e-12 * max(1.0, abs(float(auto["loss"])))
        for n, g in auto["grads"].items():
            assert mine["grads"][n].shape == g.shape, n
            assert R.rel_l2(mine["grads"][n], g) <= 1e-12, (n, R.rel_l2(mine["grads"][n], g))


def test_attention_backward_by_hand_equals_autograd():
    g = torch.Generator().manual_seed(2)
    B, T, K, A = 3, 9, 7, 8
    q, k = torch.randn(B, T, A, generator=g, dtype=torch.float64), torch.randn(B, K, A, generator=g, dtype=torch.float64)
    mask = R.mask_of([7, 4, 0], K)
    ga, gl = torch.randn(B, 1, T, K, generator=g, dtype=torch.float64), torch.randn(B, 1, T, K, generator=g, dtype=torch.float64)
    for use_a, use_l in ((True, True), (True, False), (False, True)):
        qq, kk = q.clone().requires_grad_(), k.clone().requires_grad_()
        attn, lp = R.attention(qq, kk, mask, 0.3)
        obj = (attn * ga).sum() * use_a + (lp * gl).sum() * use_l
        aq, ak = torch.autograd.grad(obj, (qq, kk))
        dq, dk, _ = R.attention_backward(q, k, mask, 0.3, attn.detach(), ga if use_a else None, gl if use_l else None)
        assert R.rel_l2(dq, aq) <= 1e-12 and R.rel_l2(dk, ak) <= 1e-12


def test_planted_faults_move_the_result_ten_tolerances():
    mv, tol = R.planted_movements(), R.tolerance()
    assert set(mv) == set(R.FAULTS) and len(mv) == 9
    for f, (a, b) in mv.items():
        assert max(a, b) >= 10 * tol, (f, a, b, tol)
    # the tolerance is of use only above what the device's operand formats cost: bf16 operands (2^-9 each, two per product)
    assert tol > 4 * 2.0 ** -9, tol
    # faults of the map itself show in attn_logprob, the others only in the gradients
    for f in ("no_relu", "taps_reversed", "pad_wrong_end", "temperature_sign", "logprob_masked"):
        assert mv[f][0] >= 10 * tol, (f, mv[f])
    for f in ("mask_off_by_one", "softmax_axis", "no_factor_2", "dk_sign"):
        assert mv[f][0] == 0.0 and mv[f][1] >= 10 * tol, (f, mv[f])


@pytest.mark.parametrize("A", [8, 80, 128])
@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_direct_form_contract_and_its_planted_faults(A, offset):
    g = torch.Generator().manual_seed(A)
    q, k = torch.randn(4096, A, generator=g) + offset, torch.randn(4096, A, generator=g) + offset
    ref = ((q.double() - k.double()) ** 2).sum(1)

    def units(form):
        return float(((R.sumsq_fp32(q, k, form).double() - ref).abs() / (R.U24 * ref)).max())

    direct, expanded, fp16 = units("direct"), units("expanded"), units("fp16")
    print(f"A {A} offset {offset}: direct {direct:.1f}, expanded {expanded:.3g}, fp16 operands {fp16:.3g} units of 2^-24; allowed {A + 4}")
    assert direct <= A + 4
    assert fp16 > A + 4
    if offset:
        assert expanded > 100 * (A + 4)


def test_bounds_helpers_on_an_exact_map():
    """the softmax restatement of the bounds: masked keys exactly 0, a fully masked row 1 / K, and a positive bound everywhere"""
    lp = torch.randn(3, 1, 4, 6)
    mask = R.mask_of([6, 3, 0], 6)
    p, bound = R.softmax_ref_and_bound(lp, mask)
    assert torch.equal(p[1, :, :, 3:], torch.zeros(1, 4, 3, dtype=torch.float64))
    assert torch.equal(p[2], torch.full((1, 4, 6), 1.0 / 6, dtype=torch.float64))
    assert float((p.sum(3) - 1).abs().max()) < 1e-14 and bool((bound > 0).all())
    ref = R.attention(torch.zeros(3, 4, 2, dtype=torch.float64), torch.zeros(3, 6, 2, dtype=torch.float64), mask, 1.0)[0]
    assert torch.equal(ref[2], p[2])


# ----------------------------------------------------------------------------- the package's host logic
def test_state_dict_names_shapes_and_prefixes():
    a = vbx.Aligner(dim_in=16, dim_hidden=24, attn_channels=8)
    want = R.shapes_of(16, 24, 8)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == want
    d = vbx.Aligner()
    assert {k: tuple(v.shape) for k, v in d.state_dict().items()} == R.shapes_of(80, 512, 80) and d.temperature == 0.0005
    sd = R.init_state(16, 24, 8, 1)
    a.load_state_dict(sd)
    assert all(torch.equal(a.state_dict()[k], sd[k]) for k in sd)
    b = vbx.Aligner(dim_in=16, dim_hidden=24, attn_channels=8)
    b.load_state_dict({"aligner." + k: v for k, v in sd.items()})
    assert all(torch.equal(b.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(RuntimeError):
        b.load_state_dict({k: v for k, v in sd.items() if k != "key_layers.2.bias"})
    assert "Aligner" in vbx.__all__ and "aligner_attention" in vbx.__all__


def test_refusals_come_before_any_launch():
    for kw in (dict(dim_in=20), dict(dim_hidden=100), dict(attn_channels=12), dict(attn_channels=136)):
        with pytest.raises(NotImplementedError):
            vbx.Aligner(**{**dict(dim_in=16, dim_hidden=24, attn_channels=8), **kw})
    a = vbx.Aligner(dim_in=16, dim_hidden=24, attn_channels=8)
    q, k = torch.randn(2, 16, 5), torch.randn(2, 3, 24)
    with pytest.raises(ValueError):
        a(q[:, :8], k)
    with pytest.raises(ValueError):
        a(q, k[:, :, :8])
    with pytest.raises(ValueError):
        a(q, k[:1])
    with pytest.raises(ValueError):
        a(q, k, mask=torch.ones(2, 4, dtype=torch.bool))
    with pytest.raises(ValueError):
        a(q, k, mask=torch.ones(2, 3))
    with pytest.raises(_lib.VbxError):  # a CPU tensor, after the shape checks
        a(q, k, mask=torch.ones(2, 1, 3, dtype=torch.bool))
    with pytest.raises(_lib.VbxError):
        a.align(q, k)
    with pytest.raises(ValueError):
        vbx.aligner_attention(torch.randn(2, 5, 8), torch.randn(2, 3, 16))
    with pytest.raises(NotImplementedError):
        vbx.aligner_attention(torch.randn(2, 5, 136), torch.randn(2, 3, 136))
    with pytest.raises(_lib.VbxError):
        vbx.aligner_attention(torch.randn(2, 5, 8), torch.randn(2, 3, 8), torch.ones(2, 3, dtype=torch.int32))


def _dp(**kw):
    return vbx.DurationPredictor(num_phoneme_tokens=12, dim_phoneme_emb=24, dim=64, depth=2, dim_head=64, heads=2, **kw)


def test_duration_predictor_default_is_unchanged():
    dp = _dp()
    assert dp.aligner is None and dp.aligner_kwargs == dict(dim_in=80, attn_channels=80)
    keys = set(dp.state_dict())
    assert not any(k.startswith("aligner.") for k in keys)
    sd = dict(dp.state_dict())
    sd["aligner.key_layers.0.weight"] = torch.zeros(2)  # a reference checkpoint's aligner: skipped
    dp.load_state_dict(sd)
    assert set(dp.state_dict()) == keys
    with pytest.raises(NotImplementedError):
        dp.train()(cond=torch.zeros(1, 4, 64), phoneme_ids=torch.zeros(1, 4, dtype=torch.long))
    for call in (lambda: dp.forward_aligner(torch.zeros(1, 2, 24), torch.ones(1, 1, 2), torch.zeros(1, 3, 80), torch.ones(1, 1, 3)),
                 lambda: dp.align_phoneme_ids(torch.zeros(1, 80, 3), torch.zeros(1, 2, dtype=torch.long))):
        with pytest.raises(RuntimeError, match="attach_aligner"):
            call()


def test_attach_aligner_changes_exactly_the_aligner_keys():
    dp = _dp(aligner_kwargs=dict(dim_in=16, attn_channels=8))
    before = set(dp.state_dict())
    a = dp.attach_aligner()
    assert isinstance(a, vbx.Aligner) and dp.aligner is a and (a.dim_in, a.dim_hidden, a.attn_channels) == (16, 24, 8)
    after = set(dp.state_dict())
    assert after - before == {"aligner." + k for k in R.shapes_of(16, 24, 8)} and before <= after
    assert any(p is a.key_layers[0].weight for p in dp.parameters())
    sd = {k: v.clone() for k, v in dp.state_dict().items()}
    sd["aligner.key_layers.2.bias"] = torch.full((8,), 3.0)
    dp.load_state_dict(sd)  # now loaded, not skipped
    assert torch.equal(dp.aligner.key_layers[2].bias.detach(), torch.full((8,), 3.0))
    with pytest.raises(NotImplementedError):  # training is still not built
        dp.train()(cond=torch.zeros(1, 4, 64), phoneme_ids=torch.zeros(1, 4, dtype=torch.long))
    mine = vbx.Aligner(dim_in=16, dim_hidden=24, attn_channels=8)
    assert _dp().attach_aligner(mine) is mine
    with pytest.raises(ValueError):
        _dp().attach_aligner(vbx.Aligner(dim_in=16, dim_hidden=32, attn_channels=8))
    with pytest.raises(TypeError):
        _dp().attach_aligner(torch.nn.Linear(2, 2))
