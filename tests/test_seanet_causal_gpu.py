"""voicebox_pytorch_amd.CausalSEANetEncoder / CausalSEANetDecoder and the entry points that carry the side (vbx_seanet_conv_c,
vbx_seanet_conv0_c, vbx_seanet_conv_out_c, vbx_seanet_convtr_t; csrc/seanet.hip) on the device against tests/seanet_causal_ref.py.

Single kernels: fp64 on the same fp16 operands (teacher-forced) under the derived per-element bounds of include/vbx.h --
conv (K + 2) 2^-24 sum |w x| + 2^-11 |y|; convtr (2C + 2) 2^-24 (sum |w a| + |b|) + 2^-11 |y|; conv_out (k nf + 6) 2^-24 (sum |w a| + |b|)
-- at tile edges and padding corners, with a poisoned row behind the output.  Those bounds hold no term for an operand whose ELU
lies on an fp16 rounding boundary (expm1f need not round as the host's does), so the inputs of the kernels that round their ELU
are drawn without such operands: an element within 2 fp32 ulps of a boundary is replaced by its absolute value (_no_flip).
Bit-equalities: each old entry point against its new one, the shift identity between the two paddings at stride 1, reruns, a row
alone against the row in a batch.
The whole networks: max |delta| / RMS(reference) against the emulated-precision and the fp64 restatement within
seanet_causal_ref.tolerance() -- one tenth of the smallest movement of any planted fault, measured by
tests/test_seanet_causal_cpu.py, not fixed in advance.  Device causality: bit-equal before the perturbation, different after it,
and the non-causal encoder moves one frame earlier.  `pytest -s -m gpu tests/test_seanet_causal_gpu.py` prints the lines kept in
profiles/seanet_causal_parity.txt (and writes them to the file named by VBX_SEANET_CAUSAL_PARITY_OUT, when set).  Parity with the
`encodec` library itself is UNPINNED."""
import os

import pytest
import torch
import torch.nn.functional as F

import seanet_causal_ref as C
import seanet_ref as S
from test_seanet_causal_cpu import causality_inputs, synthetic_encodec_file, CAUSAL_FROM, CAUSAL_T
from test_seanet_gpu import _elu_operand

gpu = pytest.mark.gpu
dev = "cuda"
LINES = []


def _say(line):
    print(line)
    LINES.append(line)


def _no_flip(x16):
    """fp16 operands none of whose ELU sits within 2 fp32 ulps of an fp16 rounding boundary"""
    _, near = _elu_operand(x16)
    return torch.where(near, x16.abs(), x16)


def _st():
    from voicebox_pytorch_amd import _lib

    return _lib.current_stream()


# ------------------------------------------------------------------------------------ vbx_seanet_conv_c
#        name          C1  C2  Co  k  stride dil
CONVS = [("k7", 16, 0, 24, 7, 1, 1), ("k3 d4", 16, 0, 24, 3, 1, 4), ("k16 s8", 16, 0, 24, 16, 8, 1), ("k4 s2", 16, 0, 24, 4, 2, 1),
         ("tail 16|16", 16, 16, 24, 1, 1, 1)]  # the two-input Resnet form: no padding at all, `causal` must not disturb it


def _conv_operands(C1, C2, Co, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(Co, C1, k, generator=g) / (C1 * k) ** 0.5).half()
    w2 = (torch.randn(Co, max(C2, 8), 1, generator=g) / max(C2, 1) ** 0.5).half()[:, :C2]
    bias = 0.1 * torch.randn(Co, generator=g)
    wk = torch.cat([w.permute(0, 2, 1).reshape(Co, k * C1), w2[:, :, 0]], dim=1).contiguous().to(dev)
    return g, w, w2, bias, wk


def _conv_inputs(g, B, L, C1, C2):
    x = _no_flip(torch.randn(B, L, C1, generator=g).half())
    x[1] = 0.75  # a constant second row: a read across the batch boundary would show in row 0
    x2 = torch.randn(B, L, max(C2, 8), generator=g).half()
    x2[1] = -0.5
    return x, x2


def _conv_call(entry, x, x2, wk, bias, B, L, C1, C2, Co, k, stride, dil, elu, out_f32, *tail):
    from voicebox_pytorch_amd import _lib

    Lout = -(-L // stride)
    y = torch.full((B + 1, Lout, Co), float("nan"), dtype=torch.float32 if out_f32 else torch.float16, device=dev)
    _lib.call(entry, x.to(dev), x2.to(dev) if C2 else None, wk, bias.to(dev), y, B, L, C1, C2, Co, k, stride, dil, int(elu), int(out_f32),
              *tail, _st())
    assert bool(torch.isnan(y[B]).all()), (entry, L, "wrote past the last row")
    return y[:B]


@gpu
@pytest.mark.parametrize("case", CONVS, ids=[c[0] for c in CONVS])
def test_causal_convolution(case):
    from voicebox_pytorch_amd import _lib

    name, C1, C2, Co, k, stride, dil = case
    tile = _lib.call_value("vbx_seanet_conv_tile", C1, C2, k, stride, dil)
    total = (k - 1) * dil + 1 - stride
    g, w, w2, bias, wk = _conv_operands(C1, C2, Co, k, 31 + k + 7 * dil)
    K = k * C1 + C2
    for L in sorted({1, 2, max(total, 1), total + 1, 13, tile * stride + 1}):  # 13: extra != 0 at stride 8 and 2; Lout = tile + 1
        B = 2
        x, x2 = _conv_inputs(g, B, L, C1, C2)
        got16 = _conv_call("vbx_seanet_conv_c", x, x2, wk, bias, B, L, C1, C2, Co, k, stride, dil, True, False, 1)
        assert torch.equal(got16, _conv_call("vbx_seanet_conv_c", x, x2, wk, bias, B, L, C1, C2, Co, k, stride, dil, True, False, 1)), "rerun"
        for b in range(B):  # a row alone is the row in the batch
            alone = _conv_call("vbx_seanet_conv_c", x[b:b + 1], x2[b:b + 1], wk, bias, 1, L, C1, C2, Co, k, stride, dil, True, False, 1)
            assert torch.equal(alone[0], got16[b]), (name, L, b)
        got = got16.double().cpu()
        assert bool(torch.isfinite(got).all()), (name, L, "an output position was not written")
        a = _elu_operand(x)[0].transpose(1, 2)
        ref = C.sconv(a, w.double(), bias.double(), stride=stride, dilation=dil)
        mag = C.sconv(a.abs(), w.double().abs(), None, stride=stride, dilation=dil)
        if C2:
            b2 = x2.double().transpose(1, 2)
            ref, mag = ref + F.conv1d(b2, w2.double()), mag + F.conv1d(b2.abs(), w2.double().abs())
        ref, mag = ref.transpose(1, 2), mag.transpose(1, 2)
        assert got.shape == ref.shape == (B, -(-L // stride), Co)
        bound = (K + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs()
        err = (got - ref).abs()
        _say(f"causal conv {name} L {L} (tile <= {tile}) K {K}: max |err| {float(err.max()):.3e}, max |err| / bound {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (name, L)
        if total and L > 1:  # and it is not the non-causal result
            assert not torch.equal(got16, _conv_call("vbx_seanet_conv_c", x, x2, wk, bias, B, L, C1, C2, Co, k, stride, dil, True, False, 0))


@gpu
def test_causal_first_and_last_convolution():
    """vbx_seanet_conv0_c (1 -> 32, fp32) and vbx_seanet_conv_out_c (32 -> 1, fp32), k 7: T = 6 is the longest row the short-input
    rule serves (padding_total 6), 7 the first it does not, 300 a second block of 256 positions"""
    from voicebox_pytorch_amd import _lib

    g = torch.Generator().manual_seed(12)
    nf, k = 32, 7
    w0 = torch.randn(nf, 1, k, generator=g) / k ** 0.5
    b0 = 0.1 * torch.randn(nf, generator=g)
    wo = torch.randn(1, nf, k, generator=g) / (nf * k) ** 0.5
    bo = 0.1 * torch.randn(1, generator=g)
    for T in (1, 3, 6, 7, 300):
        x = torch.randn(2, T, generator=g)
        x[1] = 0.75
        y = torch.full((3, T, nf), float("nan"), dtype=torch.float16, device=dev)
        args = (x.to(dev), w0[:, 0].contiguous().to(dev), b0.to(dev), y, 2, T, nf, k)
        _lib.call("vbx_seanet_conv0_c", *args, 1, _st())
        first = y.clone()
        _lib.call("vbx_seanet_conv0_c", *args, 1, _st())
        assert torch.equal(first[:2], y[:2]) and bool(torch.isnan(y[2]).all())
        got = y[:2].double().cpu()
        ref = C.sconv(x.double()[:, None], w0.double(), b0.double()).transpose(1, 2)
        mag = (C.sconv(x.double().abs()[:, None], w0.double().abs(), None) + b0.double().abs()[None, :, None]).transpose(1, 2)
        bound = (k + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25  # tests/test_seanet_gpu.py's, for the fmaf chain on the bias
        err = (got - ref).abs()
        _say(f"causal conv0 T {T}: max |err| {float(err.max()):.3e}, max |err| / bound {float((err / bound).max()):.4f}")
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), T
        old = torch.empty(2, T, nf, dtype=torch.float16, device=dev)
        _lib.call("vbx_seanet_conv0", *args[:3], old, *args[4:], _st())
        new = torch.empty_like(old)
        _lib.call("vbx_seanet_conv0_c", *args[:3], new, *args[4:], 0, _st())
        assert torch.equal(old, new), ("conv0: the old entry point is the new one at causal = 0", T)

        h = torch.randn(2, T, nf, generator=g).half()
        h[1] = -0.75
        y = torch.full((3, T), float("nan"), dtype=torch.float32, device=dev)
        args = (h.to(dev), wo[0].t().contiguous().to(dev), bo.to(dev), y, 2, T, nf, k)
        _lib.call("vbx_seanet_conv_out_c", *args, 1, _st())
        first = y.clone()
        _lib.call("vbx_seanet_conv_out_c", *args, 1, _st())
        assert torch.equal(first[:2], y[:2]) and bool(torch.isnan(y[2]).all())
        got = y[:2].double().cpu()
        a = F.elu(h.double()).transpose(1, 2)
        ref = C.sconv(a, wo.double(), bo.double())[:, 0]
        mag = (C.sconv(a.abs(), wo.double().abs(), None) + bo.double().abs()[None, :, None])[:, 0]
        bound = (k * nf + 6) * 2.0 ** -24 * mag
        err = (got - ref).abs()
        _say(f"causal conv_out T {T}: max |err| {float(err.max()):.3e}, max |err| / bound {float((err / bound).max()):.4f}")
        assert bool(torch.isfinite(got).all()) and got.shape == ref.shape and bool((err <= bound).all()), T
        old = torch.empty(2, T, dtype=torch.float32, device=dev)
        _lib.call("vbx_seanet_conv_out", *args[:3], old, *args[4:], _st())
        new = torch.empty_like(old)
        _lib.call("vbx_seanet_conv_out_c", *args[:3], new, *args[4:], 0, _st())
        assert torch.equal(old, new), ("conv_out: the old entry point is the new one at causal = 0", T)


# ------------------------------------------------------------------------------------ vbx_seanet_convtr_t
def _convtr_call(entry, x, wp, bias, B, L, C, r, *tail):
    from voicebox_pytorch_amd import _lib

    y = torch.full((B + 1, L * r, C // 2), float("nan"), dtype=torch.float16, device=dev)
    _lib.call(entry, x.to(dev), wp, bias.to(dev), y, B, L, C, r, *tail, _st())
    assert bool(torch.isnan(y[B]).all()), (entry, L, "wrote past the last row")
    return y[:B]


@gpu
@pytest.mark.parametrize("r", [2, 5, 8])
def test_transposed_convolution_with_a_given_trim(r):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    C, Co = 32, 16
    tile = _lib.call_value("vbx_seanet_convtr_tile", C, r)
    g = torch.Generator().manual_seed(40 + r)
    w = (torch.randn(C, Co, 2 * r, generator=g) / (2 * C) ** 0.5).half()
    bias = 0.1 * torch.randn(Co, generator=g)
    wp = vbx.SEANetDecoder._convtr_weight(w, r).contiguous().to(dev)
    for L in sorted({1, 2, 15, 16, 17, tile, tile + 1}):
        B = 2
        x = _no_flip(torch.randn(B, L, C, generator=g).half())
        x[1] = 0.75
        a = _elu_operand(x)[0].transpose(1, 2)
        full = F.conv_transpose1d(a, w.double(), bias.double(), stride=r)  # [B, Co, (L + 1) r]: nothing trimmed yet
        fmag = F.conv_transpose1d(a.abs(), w.double().abs(), None, stride=r) + bias.double().abs()[None, :, None]
        seen = []
        for trim in sorted({0, r - r // 2, r}):
            got16 = _convtr_call("vbx_seanet_convtr_t", x, wp, bias, B, L, C, r, trim)
            assert torch.equal(got16, _convtr_call("vbx_seanet_convtr_t", x, wp, bias, B, L, C, r, trim)), "rerun"
            for b in range(B):
                assert torch.equal(_convtr_call("vbx_seanet_convtr_t", x[b:b + 1], wp, bias, 1, L, C, r, trim)[0], got16[b]), (r, L, trim, b)
            got = got16.double().cpu()
            assert bool(torch.isfinite(got).all()), (r, L, trim, "an output sample was not written")
            ref, mag = (t[..., trim:trim + L * r].transpose(1, 2) for t in (full, fmag))
            assert got.shape == ref.shape == (B, L * r, Co)
            bound = (2 * C + 2) * 2.0 ** -24 * mag + 2.0 ** -11 * ref.abs()
            err = (got - ref).abs()
            _say(f"convtr_t C {C} r {r} L {L} trim_left {trim} (tile <= {tile}): max |err| {float(err.max()):.3e}, "
                 f"max |err| / bound {float((err / bound).max()):.4f}")
            assert bool((err <= bound).all()), (r, L, trim)
            seen.append(got16)
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
        # the old entry point is the new one at the non-causal trim
        assert torch.equal(_convtr_call("vbx_seanet_convtr", x, wp, bias, B, L, C, r), seen[sorted({0, r - r // 2, r}).index(r - r // 2)])


@gpu
def test_trim_outside_its_range_is_refused():
    from voicebox_pytorch_amd import _lib

    x = torch.zeros(1, 4, 32, dtype=torch.float16, device=dev)
    w = torch.zeros(5 * 16, 64, dtype=torch.float16, device=dev)
    b = torch.zeros(16, device=dev)
    y = torch.full((1, 20, 16), float("nan"), dtype=torch.float16, device=dev)
    for trim in (-1, 6):
        with pytest.raises(_lib.VbxError, match="trim_left"):
            _lib.call("vbx_seanet_convtr_t", x, w, b, y, 1, 4, 32, 5, trim, _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())  # nothing was launched


# ------------------------------------------------------------------------------------ bit-equalities between the two forms
@gpu
@pytest.mark.parametrize("case", CONVS, ids=[c[0] for c in CONVS])
def test_old_entry_point_is_the_new_one_at_causal_0(case):
    name, C1, C2, Co, k, stride, dil = case
    g, w, w2, bias, wk = _conv_operands(C1, C2, Co, k, 5 + k)
    for L in (1, 13, 300):
        for elu, f32 in ((True, False), (False, True)):
            x, x2 = _conv_inputs(g, 2, L, C1, C2)
            old = _conv_call("vbx_seanet_conv", x, x2, wk, bias, 2, L, C1, C2, Co, k, stride, dil, elu, f32)
            new = _conv_call("vbx_seanet_conv_c", x, x2, wk, bias, 2, L, C1, C2, Co, k, stride, dil, elu, f32, 0)
            assert torch.equal(old, new) and bool(torch.isfinite(old).all()), (name, L, elu, f32)


@gpu
@pytest.mark.parametrize("k,dil", [(7, 1), (3, 2)])
def test_shift_identity_at_stride_1(k, dil):
    """y_causal[t] == y_noncausal[t - padding_total // 2] bit for bit for padding_total <= t <= L - 1: both sides read the same
    inputs, none of them padding, in the same order"""
    C1, Co, L = 16, 24, 300
    g, w, w2, bias, wk = _conv_operands(C1, 0, Co, k, 77 + k)
    x, x2 = _conv_inputs(g, 2, L, C1, 0)
    total = (k - 1) * dil
    yc = _conv_call("vbx_seanet_conv_c", x, x2, wk, bias, 2, L, C1, 0, Co, k, 1, dil, True, False, 1)
    yn = _conv_call("vbx_seanet_conv_c", x, x2, wk, bias, 2, L, C1, 0, Co, k, 1, dil, True, False, 0)
    assert torch.equal(yc[:, total:L], yn[:, total - total // 2:L - total // 2])
    assert not torch.equal(yc[:, :total], yn[:, :total])  # where the padding is read they part


# ------------------------------------------------------------------------------------ the whole networks
def _kw(cfg):
    return {k: cfg[k] for k in ("n_filters", "ratios", "dimension", "n_residual_layers", "trim_right_ratio") if k in cfg}


def _encoder(name, sd):
    import voicebox_pytorch_amd as vbx

    enc = vbx.CausalSEANetEncoder(**_kw(C.REAL if name == "real" else C.ENC_CONFIGS[name][0]))
    enc.load_state_dict(sd)
    return enc.to(dev).eval()


def _decoder(name, sd):
    import voicebox_pytorch_amd as vbx

    dec = vbx.CausalSEANetDecoder(**_kw(C.REAL if name == "real" else C.DEC_CONFIGS[name][0]))
    dec.load_state_dict(sd)
    return dec.to(dev).eval()


def _parity(what, name, size, got, emu, ref):
    tol = C.tolerance()
    a, b = C.rel_err(got, emu), C.rel_err(got, ref)
    _say(f"causal {what} {name} B {got.shape[0]} {size}: max |delta| / RMS vs emulated {a:.3e}, vs fp64 {b:.3e} (tolerance {tol:.4g}); "
         f"emulated vs fp64 {C.rel_err(emu, ref):.3e}")
    assert a <= tol and b <= tol, (what, name, size, a, b, tol)


@gpu
@pytest.mark.parametrize("name", list(C.ENC_CONFIGS))
def test_causal_encoder_parity(name):
    enc = None
    for T in C.ENC_T:
        sd, wave, emu, ref = C.encoder_case(name, T)
        enc = enc or _encoder(name, sd)
        got = enc(wave.to(dev))
        assert got.dtype == torch.float32 and got.shape == ref.shape == (wave.shape[0], enc.frames(T), enc.dimension)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, enc(wave.to(dev)))
        for b in range(wave.shape[0]):
            assert torch.equal(enc(wave[b:b + 1].to(dev))[0], got[b]), (name, T, b)
        _parity("encoder", name, f"T {T}", got, emu, ref)


@gpu
@pytest.mark.parametrize("name", list(C.DEC_CONFIGS))
def test_causal_decoder_parity(name):
    dec = None
    for fr in C.DEC_FRAMES:
        sd, z, emu, ref = C.decoder_case(name, fr)
        dec = dec or _decoder(name, sd)
        got = dec(z.to(dev))
        assert got.dtype == torch.float32 and got.shape == ref.shape == (z.shape[0], fr * dec.hop_length)
        assert bool(torch.isfinite(got).all()) and torch.equal(got, dec(z.to(dev)))
        for b in range(z.shape[0]):
            assert torch.equal(dec(z[b:b + 1].to(dev))[0], got[b]), (name, fr, b)
        _parity("decoder", name, f"frames {fr}", got, emu, ref)


@gpu
def test_the_24_khz_widths():
    sd, wave, emu, ref = C.encoder_case("real", 24000)
    got = _encoder("real", sd)(wave.to(dev))
    assert got.shape == (1, 75, 128)
    _parity("encoder", "real", "T 24000", got, emu, ref)
    sd, z, emu, ref = C.decoder_case("real", 75)
    got = _decoder("real", sd)(z.to(dev))
    assert got.shape == (1, 24000)
    _parity("decoder", "real", "frames 75", got, emu, ref)


@gpu
def test_the_device_is_causal_where_the_restatement_is():
    """the perturbations of tests/test_seanet_causal_cpu.py: samples >= 160 of 192 (frames >= 20 of 24) and latent frames >= 20"""
    import voicebox_pytorch_amd as vbx

    sd, wave, wave2, dsd, z, z2 = causality_inputs()
    f0 = CAUSAL_FROM // 8
    enc = _encoder("small-r1", sd)
    a, b = enc(wave.to(dev)), enc(wave2.to(dev))
    assert a.shape == (2, CAUSAL_T // 8, 32)
    assert torch.equal(a[:, :f0], b[:, :f0]) and not torch.equal(a[:, f0:], b[:, f0:])
    plain = vbx.SEANetEncoder(**_kw(C.ENC_CONFIGS["small-r1"][0]))
    plain.load_state_dict(sd)
    plain = plain.to(dev).eval()
    na, nb = plain(wave.to(dev)), plain(wave2.to(dev))
    assert not torch.equal(na[:, f0 - 1], nb[:, f0 - 1])  # the non-causal network looks ahead: the test discriminates
    dec = _decoder("small-r1", dsd)
    a, b = dec(z.to(dev)), dec(z2.to(dev))
    assert a.shape == (2, CAUSAL_T)
    assert torch.equal(a[:, :CAUSAL_FROM], b[:, :CAUSAL_FROM]) and not torch.equal(a[:, CAUSAL_FROM:], b[:, CAUSAL_FROM:])


# ------------------------------------------------------------------------------------ codec and model
@gpu
def test_the_published_form_end_to_end(tmp_path):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    path, _ = synthetic_encodec_file(tmp_path)
    codec = vbx.EncodecVocoCodec.from_encodec_checkpoint(path, causal=True).to(dev).eval()
    assert type(codec.encoder) is vbx.CausalSEANetEncoder and type(codec.vocoder) is vbx.CausalSEANetDecoder
    wave = (0.3 * torch.randn(2, 190, generator=torch.Generator().manual_seed(1))).to(dev)
    frames, hop = codec.encoder.frames(190), codec.downsample_factor
    assert (frames, hop) == (24, 8)
    lat = codec.encode(wave)
    assert lat.shape == (2, frames, 32) and lat.dtype == torch.float32
    assert torch.equal(lat, codec.codes_to_latents(codec.decode_to_codes(codec.encoder(wave))))  # encode is encoder -> RVQ
    plain = vbx.EncodecVocoCodec.from_encodec_checkpoint(path).to(dev).eval()
    assert not torch.equal(plain.encoder(wave), codec.encoder(wave))  # the same file is another network without causal=True
    out = codec.decode(lat)
    assert out.shape == (2, frames * hop) and bool(torch.isfinite(out).all())
    assert torch.equal(out, codec.vocoder(codec.codes_to_features(codec.decode_to_codes(lat))))
    torch.manual_seed(0)
    vb = vbx.VoiceBox(dim=64, depth=2, heads=2, audio_enc_dec=codec, condition_on_text=False).to(dev)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    g = torch.Generator().manual_seed(5)
    draws = dict(x0=torch.randn(2, frames, 32, generator=g), times=torch.rand(2, generator=g), frac_lengths=torch.tensor([0.8, 0.9]),
                 rand=torch.rand(2, generator=g))
    with rng_override(**draws):
        loss = wrapper(wave)
    assert bool(torch.isfinite(loss))
    with rng_override(y0=torch.randn(2, frames, 32, generator=g)):
        sampled = wrapper.sample(cond=wave, steps=2)
    assert sampled.shape == (2, frames * hop) and sampled.dtype == torch.float32 and bool(torch.isfinite(sampled).all())


@gpu
def test_zz_report():
    """not a check: the measured values (profiles/seanet_causal_parity.txt)"""
    path = os.environ.get("VBX_SEANET_CAUSAL_PARITY_OUT")
    if path and LINES:
        with open(path, "w") as fh:
            fh.write("CausalSEANetEncoder / CausalSEANetDecoder and their entry points, MI355X: tests/test_seanet_causal_gpu.py against "
                     "tests/seanet_causal_ref.py\n" + "\n".join(LINES) + "\n")
