"""DurationPredictor over codec latents without a device: the fp64 restatement (tests/duration_codec_ref.py) against the fixture of
the unmodified reference (tests/golden/duration_codec.pt), the planted faults against the per-element bounds the GPU tests hold, and
the semantics of attach_codec (what raises, what proj_in becomes, the state-dict layout, the pinned constructor keyword)."""
import pytest
import torch
from torch import nn

import duration_codec_ref as C
import duration_train_ref as R
from oracle import ref_loader, restate
from toy_codec import ToyCodec

import voicebox_pytorch_amd as vbx

KW = dict(num_phoneme_tokens=37, dim_phoneme_emb=32, dim=64, depth=2, dim_head=64, heads=2)
ORACLE_TOL = 1e-4  # what tests/test_oracle.py::test_duration_predictor_inference holds for duration.pt


def _f64(state):
    return {k: v.double() if v.is_floating_point() else v for k, v in state.items()}


def test_restatement_against_the_reference_fixture(golden):
    cases = C.fixture_cases(golden("duration_codec"))
    assert sorted(c["latent_dim"] for c in cases.values()) == [100, 128]
    shorter = longer = False
    for name, c in cases.items():
        S, n = c["cond"].shape[1], c["ids"].shape[1]
        shorter, longer = shorter or S < n, longer or S > n
        assert c["cond"].shape[-1] == c["latent_dim"] and bool((c["ids"] == -1).any()) and bool(c["cond_mask"].any())
        p, cfg = c["state"], R.cfg_of()  # in the fixture's own fp32, as tests/test_oracle.py runs the restatement against duration.pt
        drop = torch.ones(3, dtype=torch.bool)
        with torch.no_grad():
            d1 = C.predict(p, cfg, c)
            dn = C.predict(p, cfg, dict(c, drop=drop))
            one = C.predict_one_line(p, cfg, c)
            one_n = C.predict_one_line(p, cfg, dict(c, drop=drop))
        d3 = dn + (d1 - dn) * 3.0
        for got, key in ((d1, "d1"), (dn, "d_null"), (d3, "d3")):
            err = float((got - c[key]).abs().max())
            print(name, key, err)
            assert err < ORACLE_TOL, (name, key, err)
        # the composition with its switches is the one-line model
        assert float((d1 - one).abs().max()) <= 1e-5 and float((dn - one_n).abs().max()) <= 1e-5
        p64, c64 = _f64(c["state"]), dict(c, cond=c["cond"].double())
        with torch.no_grad():
            assert float((C.predict(p64, cfg, c64) - C.predict_one_line(p64, cfg, c64)).abs().max()) <= 1e-12
            assert float((C.predict(p64, cfg, dict(c64, drop=drop)) - C.predict_one_line(p64, cfg, dict(c64, drop=drop))).abs().max()) <= 1e-12
        assert float((c["d1"] - c["d_null"]).abs().max()) > 1e-2, name
        assert torch.equal(restate.align_phoneme_ids_with_durations(c["ids"], c["d3"]), c["aligned"]), name
    assert shorter and longer


def _fault_case(fault):
    """the smallest inputs on which the fault can show: padding (S < n) for the faults about rows past S, a dropped batch for the
    faults about the drop.  S = 5 of n = 21: a fault that counts the padded rows adds 16 rows to a sum whose bound grows with the 5
    (or fewer, unmasked) rows that belong in it."""
    drop = fault in ("null_through_proj", "pad_rows_of_dropped_get_null", "dropped_counted")
    pad = fault in ("pad_rows_get_bias", "pad_rows_of_dropped_get_null", "pad_rows_counted_in_bias")
    return C.given_case(100, 32, 2, 21, drop, 5) if pad else C.given_case(100, 32, 3, 17, drop)


def _cond_bound(p, case):
    """the pack kernel's per-element bound on cond'' [B, n, D]; rows the contract fixes exactly (masked, dropped, r >= S) allow 0"""
    lat16, w16 = case["cond"].half().double(), p["proj_in.weight"].detach().half().double()
    y = lat16 @ w16.t() + p["proj_in.bias"].detach()
    bound = C.proj_bound(lat16, w16, p["proj_in.bias"].detach(), y)
    exact = case["cond_mask"].clone()
    if case.get("drop") is not None:
        exact |= case["drop"][:, None]
    bound = bound * ~exact[..., None]
    return restate.curtail_or_pad(bound, case["ids"].shape[-1])


def _wgrad(p, case, fault):
    """fp64 [ d proj_in.weight | d proj_in.bias ] of the front end under upstream gradients, and what its bound needs"""
    B, n = case["ids"].shape
    with restate.emulate_fp16_operands():
        x, e, emb, packed, c = C.front_end(p, case, fault)
    gx = torch.randn(B, n, 64, generator=torch.Generator().manual_seed(n)).double()
    de, dc = torch.autograd.grad(x, (e, c), gx, retain_graph=True)
    dw, db = torch.autograd.grad(x, (p["proj_in.weight"], p["proj_in.bias"]), gx, allow_unused=True)
    dw = torch.zeros_like(p["proj_in.weight"]) if dw is None else dw
    db = torch.zeros_like(p["proj_in.bias"]) if db is None else db
    return torch.cat((dw, db[:, None]), dim=1), de.reshape(B * n, 64), dc.reshape(B * n, 64)


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_fault_is_seen(fault):
    """a forward fault moves an element of cond'' by at least 10 x the bound the pack-kernel test holds there; a gradient fault
    leaves cond'' alone and moves an element of d proj_in.weight / bias by at least 10 x the bound the front-end test holds"""
    case = _fault_case(fault)
    p = R.leaves(case["state"])
    n = case["ids"].shape[-1]
    with torch.no_grad(), restate.emulate_fp16_operands():
        good = C.cond_rows(p, case["cond"], case["cond_mask"], case.get("drop"), n)
        bad = C.cond_rows(p, case["cond"], case["cond_mask"], case.get("drop"), n, fault)
    moved = (bad - good).abs()
    if fault in C.FORWARD_FAULTS:
        ratio = float((moved / _cond_bound(p, case).clamp(min=1e-300)).max())
        print(fault, "cond'' moves by", float(moved.max()), "=", ratio, "x its bound")
        assert ratio >= 10.0, (fault, ratio)
        return
    assert float(moved.max()) == 0.0  # the same values
    g_good, de, dc = _wgrad(p, case, None)
    g_bad, _, _ = _wgrad(p, case, fault)
    x = C.lcb_rows(case["cond"], case["cond_mask"], case.get("drop"), n).bfloat16().double()
    E = case["state"]["to_phoneme_emb.weight"].shape[1]
    bound = C.proj_wgrad_bound(de, p["to_embed.weight"].detach()[:, E:], dc, x)
    ratio = float(((g_bad - g_good).abs() / bound.clamp(min=1e-300)).max())
    print(fault, "the gradient moves by", float((g_bad - g_good).abs().max()), "=", ratio, "x its bound")
    assert ratio >= 10.0, (fault, ratio)
    if fault == "dropped_counted":
        assert float(g_good.abs().max()) == 0.0 and float(bound.max()) == 0.0  # every sample dropped: exactly nothing


def test_training_reference_holds_its_own_conditions():
    """what the GPU module tests rely on: planted targets at least 0.5 from a sign change, proj_in.* among the gradients, none of
    them to null_cond, and a bias far from 0"""
    for E, B, n, drop in ((32, 3, 17, False), (24, 2, 65, True), (32, 1, 1, False)):
        c = C.given_case(100, E, B, n, drop)
        assert R.margin(c["d_ref"], c["target"]) >= 0.5 - 1e-9
        assert float(c["state"]["proj_in.bias"].abs().mean()) > 0.1
    ref = C.given_reference(100, 32, 3, 17, False)
    assert "null_cond" not in ref["grads"]
    assert float(ref["grads"]["proj_in.weight"].abs().max()) > 0 and float(ref["grads"]["proj_in.bias"].abs().max()) > 0
    dropped = C.given_reference(100, 32, 3, 17, True)["grads"]
    assert float(dropped["proj_in.weight"].abs().max()) == 0.0 and float(dropped["proj_in.bias"].abs().max()) == 0.0


@pytest.mark.parametrize("E,B,n", [(32, 3, 17), (32, 2, 65), (24, 2, 65)])
def test_training_cases_are_well_conditioned(E, B, n):
    """the restatement's own gradients under a change of the latents by one part in 1000 (above what any operand rounding of the
    device does to them): no tensor moves by more than GRAD_TOL / 10, so a distance near GRAD_TOL on the device is the device's"""
    case = C.given_case(100, E, B, n, False)
    g = torch.Generator().manual_seed(1)
    moved = dict(case, cond=case["cond"] * (1 + 1e-3 * torch.randn(case["cond"].shape, generator=g)))
    a, b = C.reference(case), C.reference(moved)
    worst = max((R.rel_l2(b["grads"][k], v), k) for k, v in a["grads"].items() if v is not None and float(v.norm()) > 0)
    print(E, B, n, worst)
    assert worst[0] < R.GRAD_TOL / 10, worst


# ----------------------------------------------------------------------------- attach_codec
class _NoDecode(nn.Module):
    latent_dim, sampling_rate, downsample_factor = 100, 24000, 16

    def encode(self, x):
        return x


def test_attach_codec_semantics():
    dp = vbx.DurationPredictor(**KW)
    before = {k: v.clone() for k, v in dp.state_dict().items()}
    assert dp.audio_enc_dec is None and isinstance(dp.proj_in, nn.Identity) and dp.latent_dim == 64
    for bad in (object(), nn.Linear(2, 2), _NoDecode()):
        with pytest.raises(TypeError, match="attach_codec"):
            dp.attach_codec(bad)
    for L in (4, 7, 1025):
        with pytest.raises(NotImplementedError, match="8 .. 1024"):
            dp.attach_codec(ToyCodec(L))
    assert dp.audio_enc_dec is None and isinstance(dp.proj_in, nn.Identity)
    codec = ToyCodec(100)
    assert dp.attach_codec(codec) is dp
    assert dp.audio_enc_dec is codec and isinstance(dp.proj_in, nn.Linear) and dp.latent_dim == 100
    assert dp.proj_in.weight.requires_grad and dp.proj_in.bias.requires_grad and not dp.null_cond.requires_grad
    assert dp.proj_in.weight.device == dp.to_embed.weight.device
    sd = dp.state_dict()
    assert sd["proj_in.weight"].shape == (64, 100) and sd["proj_in.bias"].shape == (64,)
    assert set(sd) == set(before) | {"proj_in.weight", "proj_in.bias"}
    assert all(torch.equal(sd[k], v) for k, v in before.items())
    assert not any(k.startswith("audio_enc_dec.") for k in sd)  # as for VoiceBox: the test codec has no persistent state
    w = dp.proj_in.weight
    assert dp.attach_codec(ToyCodec(100)) is dp and dp.proj_in.weight is w  # the same width again: proj_in is kept
    with pytest.raises(ValueError, match="attach_codec"):
        dp.attach_codec(ToyCodec(128))
    with pytest.raises(ValueError, match="attach_codec"):
        dp.attach_codec(ToyCodec(64))
    assert dp.proj_in.weight is w and dp.latent_dim == 100
    # every width the kernel serves
    for L in (8, 1024):
        assert vbx.DurationPredictor(**KW).attach_codec(ToyCodec(L)).proj_in.in_features == L


def test_latent_dim_equal_to_dim_keeps_the_identity():
    dp = vbx.DurationPredictor(**KW)
    keys = list(dp.state_dict())
    codec = ToyCodec(64)
    dp.attach_codec(codec)
    assert dp.audio_enc_dec is codec and isinstance(dp.proj_in, nn.Identity) and list(dp.state_dict()) == keys
    with pytest.raises(ValueError, match="attach_codec"):
        dp.attach_codec(ToyCodec(100))


def test_state_dict_layout_and_fixture_load(golden):
    cases = C.fixture_cases(golden("duration_codec"))
    for name, c in cases.items():
        L = c["latent_dim"]
        dp = vbx.DurationPredictor(**KW).attach_codec(ToyCodec(L))
        sd = dp.state_dict()
        ours = {k: v.shape for k, v in sd.items() if "inv_freq" not in k}
        theirs = {k: v.shape for k, v in c["state"].items() if not k.startswith("aligner.") and "inv_freq" not in k}
        assert ours == theirs, name
        missing = dp.load_state_dict(c["state"], strict=False)
        assert not missing.unexpected_keys and all("inv_freq" in k for k in missing.missing_keys), missing
        assert torch.equal(dp.proj_in.weight, c["state"]["proj_in.weight"]) and torch.equal(dp.proj_in.bias, c["state"]["proj_in.bias"])
        # without attach_codec the same checkpoint does not fit
        plain = vbx.DurationPredictor(**KW).load_state_dict(c["state"], strict=False)
        assert sorted(plain.unexpected_keys) == ["proj_in.bias", "proj_in.weight"]


@pytest.mark.skipif(not ref_loader.reference_available(), reason="the reference checkout is not on this machine")
def test_state_dict_layout_against_the_live_reference():
    ref = ref_loader.load_reference()
    for L in (100, 128):
        rsd = ref.DurationPredictor(audio_enc_dec=ToyCodec(L), **KW).state_dict()
        sd = vbx.DurationPredictor(**KW).attach_codec(ToyCodec(L)).state_dict()
        theirs = {k: v.shape for k, v in rsd.items() if not k.startswith("aligner.") and "inv_freq" not in k}
        ours = {k: v.shape for k, v in sd.items() if "inv_freq" not in k}
        assert ours == theirs
        assert rsd["proj_in.weight"].shape == (64, L)


def test_constructor_keyword_still_raises_and_names_attach_codec():
    """two tests from before attach_codec pin the refusal of the keyword; the message now says where to go"""
    with pytest.raises(NotImplementedError, match="attach_codec"):
        vbx.DurationPredictor(audio_enc_dec=ToyCodec(100), **KW)
    with pytest.raises(NotImplementedError, match="attach_codec"):
        vbx.DurationPredictor(num_phoneme_tokens=37, audio_enc_dec=object())


def test_width_assertion_names_attach_codec():
    ids = torch.zeros(2, 5, dtype=torch.long)
    dp = vbx.DurationPredictor(**KW).eval()
    with pytest.raises(AssertionError, match="attach_codec"):
        dp._resolve(torch.zeros(2, 5, 100), ids, torch.zeros(2, 5, dtype=torch.bool), 0.0, None)
    dp._resolve(torch.zeros(2, 5, 64), ids, torch.zeros(2, 5, dtype=torch.bool), 0.0, None)
    dp.attach_codec(ToyCodec(100))
    dp._resolve(torch.zeros(2, 5, 100), ids, torch.zeros(2, 5, dtype=torch.bool), 0.0, None)
    with pytest.raises(AssertionError, match="latent_dim"):
        dp._resolve(torch.zeros(2, 5, 64), ids, torch.zeros(2, 5, dtype=torch.bool), 0.0, None)
    # the refusals around it are unchanged
    dp.train()
    with pytest.raises(NotImplementedError, match="no gradient to cond"):
        dp(cond=torch.zeros(2, 5, 100, requires_grad=True), phoneme_ids=ids, target=torch.ones(2, 5))
    with pytest.raises(vbx._lib.VbxError, match="no CPU fallback"):
        dp(cond=torch.zeros(2, 5, 100), phoneme_ids=ids, target=torch.ones(2, 5))
