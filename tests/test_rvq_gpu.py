"""The residual vector quantizer on the device (csrc/rvq.hip) against tests/rvq_ref.py: the search contract checked teacher-forced
(the bound is derived there, not measured), ties, exact codewords, bit-equality of the gather-sums, out-of-range indices, overrun
guards, reruns; ResidualVQ / EncodecVocoCodec through VoiceBox; VocosDecoder.from_checkpoint(bandwidth_id=...).  Parity with
vector_quantize_pytorch / encodec / vocos is UNPINNED (the libraries are absent).

Transformer asserts an even depth, so the smallest VoiceBox these tests can build has depth 2."""
import pytest
import torch

import rvq_ref as rr
import vocos_ref as vr
from test_vocos_gpu import BOUND_A

gpu = pytest.mark.gpu
dev = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def raw_encode(L, x, cb, codes_qn, want_quant=True):
    """vbx_rvq_encode with NaN / -1 guard rows behind every output; returns (codes as laid out, quantized [B, N, D] or None)"""
    B, N, D = x.shape
    Q, K, _ = cb.shape
    xd, cbd = x.to(dev), cb.to(dev)
    norms = torch.full((Q * K + 64,), NAN, device=dev)
    L.call("vbx_rvq_norms", cbd, norms, Q, K, D, st())
    assert bool(torch.isnan(norms[Q * K:]).all())
    ref = cb.double().pow(2).sum(2).reshape(-1)
    assert bool(((norms[:Q * K].double().cpu() - ref).abs() <= (D + 1) * 2.0 ** -24 * ref).all())
    codes = torch.full((B * N * Q + 64,), -7, dtype=torch.int64, device=dev)
    quant = torch.full((B * N + 3, D), NAN, device=dev) if want_quant else None
    L.call("vbx_rvq_encode", xd, cbd, norms, codes, quant, B, N, D, K, Q, int(codes_qn), st())
    assert bool((codes[B * N * Q:] == -7).all()) and (quant is None or bool(torch.isnan(quant[B * N:]).all()))
    codes = codes[:B * N * Q].reshape((B, Q, N) if codes_qn else (B, N, Q)).cpu()
    return codes, None if quant is None else quant[:B * N].reshape(B, N, D).cpu()


def raw_decode(L, codes, cb, codes_qn, channel_first):
    B, Qc, N = codes.shape if codes_qn else (codes.shape[0], codes.shape[2], codes.shape[1])
    Q, K, D = cb.shape
    out = torch.full((B * N * D + 64,), NAN, device=dev)
    L.call("vbx_rvq_decode", codes.to(dev), cb.to(dev), out, B, N, D, K, Qc, int(codes_qn), int(channel_first), st())
    assert bool(torch.isnan(out[B * N * D:]).all())
    return out[:B * N * D].reshape((B, D, N) if channel_first else (B, N, D)).cpu()


ALL_CASES = [c[0] for c in rr.CASES] + [p[0] for p in rr.PLANTED]


# ----------------------------------------------------------------------------- the search
@gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_search_contract_and_outputs(L, name):
    x, cb = rr.case_inputs(name)
    B, N, D = x.shape
    Q, K, _ = cb.shape
    codes, quant = raw_encode(L, x, cb, codes_qn=False)
    assert codes.dtype == torch.int64 and int(codes.min()) >= 0 and int(codes.max()) < K  # a padded codeword never wins
    flat = codes.reshape(B * N, Q)
    res = rr.check_search(x.reshape(B * N, D), cb, flat)
    print(f"rvq search {name} (frames {B * N}, D {D}, K {K}, Q {Q}): {res}")
    assert res["violations"] == 0, res
    assert res["forced_wrong"] == 0, res
    if name.startswith("planted"):
        assert res["forced"] == B * N
    # quantized: bit-equal to the fp32 loop over the kernel's own codes; both code layouts hold the same codes; reruns identical
    assert torch.equal(quant.reshape(B * N, D), rr.gather_sum(flat, cb))
    codes_qn, quant2 = raw_encode(L, x, cb, codes_qn=True)
    assert codes_qn.shape == (B, Q, N) and torch.equal(codes_qn.transpose(1, 2), codes) and torch.equal(quant2, quant)
    assert torch.equal(raw_encode(L, x, cb, codes_qn=False, want_quant=False)[0], codes)
    # vbx_rvq_decode from either code layout into either output layout: the same bits
    for qn, c in ((False, codes), (True, codes_qn)):
        assert torch.equal(raw_decode(L, c, cb, qn, False), quant)
        assert torch.equal(raw_decode(L, c, cb, qn, True), quant.transpose(1, 2))


@gpu
def test_ties_go_to_the_lower_index(L):
    x, cb, expect = rr.tie_case()
    codes, _ = raw_encode(L, x, cb, codes_qn=False)
    c0 = codes[0, :, 0]
    assert bool((c0[expect >= 0] == expect[expect >= 0]).all()), c0
    assert bool((c0[expect < 0] == 17).all())
    assert rr.check_search(x[0], cb, codes[0])["violations"] == 0


@gpu
def test_exact_codeword_leaves_a_zero_residual(L):
    x, cb, k0 = rr.exact_case()
    codes, quant = raw_encode(L, x, cb, codes_qn=True)
    assert torch.equal(codes[0, 0], k0)
    assert bool((codes[0, 1] == 5).all()), codes[0, 1]  # d(k) = |c_1k|^2: the shortest codeword, the lower of its two copies
    assert torch.equal(quant[0], cb[0][k0] + cb[1][5])


@gpu
def test_out_of_range_indices(L):
    import voicebox_pytorch_amd as vbx

    x, cb = rr.case_inputs("tail")
    B, N, D = x.shape
    Q, K, _ = cb.shape
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, K, (B, N, Q), generator=g)
    codes[0, 0, 0], codes[2, 5, 1], codes[6, 10, 3], codes[3, 3, 2] = -1, K, 2 ** 40, -2 ** 40
    ref = rr.gather_sum(codes.reshape(B * N, Q), cb).reshape(B, N, D)
    assert torch.equal(raw_decode(L, codes, cb, False, False), ref)
    assert torch.equal(raw_decode(L, codes.transpose(1, 2).contiguous(), cb, True, True), ref.transpose(1, 2))
    rvq = vbx.ResidualVQ(dim=D, codebook_size=K, num_quantizers=Q)
    rvq.load_state_dict({"codebooks": cb})
    rvq.to(dev)
    assert torch.equal(rvq.decode(codes.to(dev), check=False).cpu(), ref)
    with pytest.raises(ValueError, match="codes must lie in"):
        rvq.decode(codes.to(dev))
    ok = codes.clamp(0, K - 1)
    assert torch.equal(rvq.decode(ok.to(dev)).cpu(), rr.gather_sum(ok.reshape(B * N, Q), cb).reshape(B, N, D))
    assert torch.equal(rvq.decode(ok[..., :2].to(dev)).cpu(), rr.gather_sum(ok.reshape(B * N, Q)[:, :2], cb).reshape(B, N, D))  # fewer quantizers


# ----------------------------------------------------------------------------- modules
SMALL = dict(input_channels=32, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64)


def build_codec(seed=0, Q=4, K=64):
    import voicebox_pytorch_amd as vbx

    torch.manual_seed(seed)
    _, cb = rr.random_case(8, 32, K, Q, seed=seed)
    rvq = vbx.ResidualVQ(dim=32, codebook_size=K, num_quantizers=Q)
    rvq.load_state_dict({"codebooks": cb})
    voc = vbx.VocosDecoder(**SMALL)
    voc.load_state_dict(vr.random_state(32, 64, 192, 2, 256, seed))
    return vbx.EncodecVocoCodec(rvq=rvq, vocoder=voc, downsample_factor=64).to(dev).eval(), cb


@gpu
def test_residualvq_module():
    codec, cb = build_codec()
    rvq = codec.rvq
    x, _ = rr.random_case(3 * 21, 32, 64, 4, seed=0)
    z = x.reshape(3, 21, 32).to(dev)
    quant, codes, third = rvq(z)
    assert third is None and codes.shape == (3, 21, 4) and codes.dtype == torch.int64 and quant.shape == (3, 21, 32)
    assert rr.check_search(x, cb, codes.reshape(63, 4))["violations"] == 0
    assert torch.equal(rvq.encode(z), codes) and torch.equal(rvq.decode(codes), quant)
    assert torch.equal(rvq(z.half())[1], rvq(z.half().float())[1])  # other float dtypes are converted in
    with torch.no_grad():
        rvq.codebooks.mul_(2.0)  # in place: the version counter moves, the |c|^2 table is rebuilt
    assert rr.check_search(x, 2.0 * cb, rvq.encode(z).reshape(63, 4))["violations"] == 0


@gpu
def test_codec_codes_latents_features_decode():
    codec, cb = build_codec()
    x, _ = rr.random_case(2 * 9, 32, 64, 4, seed=5)
    z = x.reshape(2, 9, 32).to(dev)
    codes = codec.decode_to_codes(z)
    assert codes.shape == (2, 4, 9) and codes.dtype == torch.int64
    assert torch.equal(codes.transpose(1, 2), codec.rvq(z)[1])
    assert torch.equal(codec.codes_to_latents(codes), codec.rvq(z)[0])
    feats = codec.codes_to_features(codes)
    assert feats.shape == (2, 32, 9) and torch.equal(feats, codec.codes_to_latents(codes).transpose(1, 2))
    wave = codec.decode(z)
    assert wave.shape == (2, 8 * 64) and torch.isfinite(wave).all() and torch.equal(wave, codec.vocoder(feats))
    assert torch.equal(codec.decode(z), wave)
    # a feature table of its own (Vocos keeps one): features come from it, latents from rvq
    import voicebox_pytorch_amd as vbx

    frvq = vbx.ResidualVQ(dim=32, codebook_size=64, num_quantizers=4)
    frvq.load_state_dict({"codebooks": 0.5 * cb})
    c2 = vbx.EncodecVocoCodec(rvq=codec.rvq, vocoder=codec.vocoder, feature_rvq=frvq).to(dev)
    assert torch.equal(c2.codes_to_features(codes), rr.gather_sum(codes.transpose(1, 2).reshape(18, 4).cpu(), 0.5 * cb).reshape(2, 9, 32).transpose(1, 2).to(dev))
    # encode: the user's encoder, then the quantized latents
    c3 = vbx.EncodecVocoCodec(rvq=codec.rvq, vocoder=codec.vocoder, encoder=lambda a: a.reshape(a.shape[0], -1, 32)).to(dev)
    assert torch.equal(c3.encode(z.reshape(2, 288)), codec.rvq(z)[0])


@gpu
def test_voicebox_samples_codes_and_trains_on_latents_from_codes():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    codec, cb = build_codec(seed=2)
    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=64, depth=2, heads=2, audio_enc_dec=codec, condition_on_text=False).to(dev)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    x, _ = rr.random_case(2 * 24, 32, 64, 4, seed=6)
    latents = x.reshape(2, 24, 32).to(dev)
    y0 = torch.randn(2, 24, 32, generator=torch.Generator().manual_seed(1))
    with rng_override(y0=y0):
        codes = wrapper.sample(cond=latents, steps=3, decode_to_codes=True)
    with rng_override(y0=y0):
        sampled = wrapper.sample(cond=latents, steps=3, decode_to_audio=False)
    with rng_override(y0=y0):
        wave = wrapper.sample(cond=latents, steps=3)
    assert codes.shape == (2, 4, 24) and codes.dtype == torch.int64 and torch.equal(codes, codec.decode_to_codes(sampled))
    assert wave.shape == (2, 23 * 64) and torch.equal(wave, codec.decode(sampled))
    vb.train()
    loss = wrapper(codec.codes_to_latents(codes))
    assert loss.ndim == 0 and bool(torch.isfinite(loss))
    loss.backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in vb.parameters())


# ----------------------------------------------------------------------------- checkpoints
@gpu
def test_adanorm_checkpoint_decodes_as_the_folded_layernorm(tmp_path):
    import voicebox_pytorch_amd as vbx
    from test_rvq_cpu import adanorm_state

    sd = adanorm_state(0)
    path = str(tmp_path / "vocos_encodec.pt")
    torch.save(sd, path)
    m = vbx.VocosDecoder.from_checkpoint(path, hop_length=64, bandwidth_id=1).to(dev)
    folded = {k: v for k, v in vbx.VocosDecoder._fold_adanorm(sd, 1).items() if not k.startswith("feature_extractor.")}
    plain = {}
    for k, v in sd.items():  # the same fold written out here: rows 1 as LayerNorm weights
        if k.startswith("feature_extractor."):
            continue
        k2 = k.replace(".norm.scale.weight", ".norm.weight").replace(".norm.shift.weight", ".norm.bias")
        plain[k2] = v[1] if k2 != k else v
    assert set(plain) == set(folded) and all(torch.equal(plain[k], folded[k]) for k in plain)
    x = torch.randn(2, 32, 9, generator=torch.Generator().manual_seed(4))
    err = vr.wave_err(m(x.to(dev)), vr.decode(plain, x, emulate=True, n_fft=256, hop=64))
    other = vr.wave_err(m(x.to(dev)), vr.decode({**plain, "backbone.norm.weight": sd["backbone.norm.scale.weight"][0]}, x, emulate=True, n_fft=256, hop=64))
    print(f"adanorm fold: wave error {err:.3e} (bound {BOUND_A:.3e}); with row 0 in one norm instead {other:.3e}")
    assert err < BOUND_A and other > 10 * BOUND_A


@gpu
def test_from_vocos_checkpoint_decodes(tmp_path):
    import voicebox_pytorch_amd as vbx
    from test_rvq_cpu import adanorm_state

    sd = adanorm_state(1)
    path = str(tmp_path / "vocos_encodec.pt")
    torch.save(sd, path)
    codec = vbx.EncodecVocoCodec.from_vocos_checkpoint(path, bandwidth_id=1, codebook_size=16, hop_length=64).to(dev)
    cb = sd["feature_extractor.codebook_weights"][:64].reshape(4, 16, 32)
    x, _ = rr.random_case(9, 32, 16, 4, seed=8)
    z = (x * 0 + cb[0][:9] + cb[1][3:12] + 0.01 * x).reshape(1, 9, 32)
    codes = codec.decode_to_codes(z.to(dev))
    assert rr.check_search(z[0], cb, codes[0].t().cpu())["violations"] == 0
    wave = codec.decode(z.to(dev))
    voc = vbx.VocosDecoder.from_checkpoint(path, hop_length=64, bandwidth_id=1).to(dev)
    assert wave.shape == (1, 8 * 64) and torch.equal(wave, voc(codec.codes_to_features(codes)))
