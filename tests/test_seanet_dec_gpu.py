"""voicebox_pytorch_amd.SEANetDecoder on the device (csrc/seanet.hip) against the restatement tests/seanet_dec_ref.py.

Single kernels: fp64 on the same fp16-rounded operands under a DERIVED per-element bound, in the form of tests/test_seanet_gpu.py.
vbx_seanet_convtr: (2C + 2) * 2^-24 * (sum |w a| + |b|) for any fp32 summation order of the 2C products under an output sample plus
the bias, 2^-11 |y| + 2^-25 for the fp16 store, and one fp16 ulp times |w| for every operand whose ELU lies within 2 fp32 ulps of an
fp16 rounding boundary (expm1f need not round as the host's does).  vbx_seanet_conv_out: (k nf + 6) * 2^-24 * (sum |w a| + |b|): k nf
+ 2 covers any fp32 summation order, 4 an expm1f two fp32 ulps from the host's (the ELU is not rounded to fp16 there, so no flip
term, and the output is fp32).
The whole decoder: max |delta| / RMS(reference) against the emulated-precision restatement (BOUND_A_*: only fp32 summation order and
fp16 boundary flips differ) and against plain fp64 (BOUND_B_*: what fp16 operands cost), per configuration, each 2 x the largest
value measured on an MI355X over exactly the listed cases and seeds 0 .. 2 (profiles/seanet_dec_parity.txt; the factor 2 is for seeds
not drawn).  Parity with the `encodec` library itself is UNPINNED."""
import functools

import pytest
import torch
import torch.nn.functional as F

import seanet_dec_ref as D
import seanet_ref as S
from test_seanet_gpu import _elu_operand, _ulp16

gpu = pytest.mark.gpu
dev = "cuda"

# 2 x the largest measured (profiles/seanet_dec_parity.txt).  Worst cases: BOUND_A_REAL B 2 frames 70 seed 2 (1.194e-03);
# BOUND_B_REAL B 2 frames 70 seed 0 (1.210e-03); BOUND_A_SMALL B 3 frames 150 seed 0 (1.886e-03); BOUND_B_SMALL B 3 frames 1 seed 0 (4.205e-03).
BOUND_A_REAL = 0.00239
BOUND_B_REAL = 0.00242
BOUND_A_SMALL = 0.00378
BOUND_B_SMALL = 0.00841

SMALL_KW = dict(n_filters=16, ratios=(5, 2), dimension=32)


def _latents(B, dim, frames, seed):
    return 3.0 * torch.randn(B, dim, frames, generator=torch.Generator().manual_seed(2000 + seed))


# ------------------------------------------------------------------------------------ the transposed convolution
CONVTRS = [(32, 2), (64, 4), (128, 5), (512, 8), (1024, 8)]


@gpu
@pytest.mark.parametrize("C,r", CONVTRS, ids=[f"{c}-{c // 2} r{r}" for c, r in CONVTRS])
def test_single_transposed_convolution(C, r):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    Co = C // 2
    tile = _lib.call_value("vbx_seanet_convtr_tile", C, r)
    assert tile in (16, 32, 64, 128)
    g = torch.Generator().manual_seed(C + r)
    w = (torch.randn(C, Co, 2 * r, generator=g) / (2 * C) ** 0.5).half()
    bias = 0.1 * torch.randn(Co, generator=g)
    wp = vbx.SEANetDecoder._convtr_weight(w, r).contiguous().to(dev)
    for L in (1, 2, 3, 17, tile + 1):
        B = 2
        x = torch.randn(B, L, C, generator=g).half()
        x[1] = 0.75  # a constant second row: a halo read across the batch boundary would show in row 0
        y = torch.full((B + 1, L * r, Co), float("nan"), dtype=torch.float16, device=dev)
        args = (x.to(dev), wp, bias.to(dev), y, B, L, C, r, _lib.current_stream())
        _lib.call("vbx_seanet_convtr", *args)
        first = y.clone()
        _lib.call("vbx_seanet_convtr", *args)
        assert torch.equal(first[:B], y[:B]), (C, r, L, "rerun differs")
        assert bool(torch.isnan(y[B]).all()), (C, r, L, "wrote past the last row")
        got = y[:B].double().cpu()
        assert bool(torch.isfinite(got).all()), (C, r, L, "an output sample was not written")
        a, near = _elu_operand(x)  # fp64 on the same operands
        a, near = a.transpose(1, 2), near.transpose(1, 2)
        ref = D.sconvtr(a, w.double(), bias.double(), r).transpose(1, 2)
        mag = (D.sconvtr(a.abs(), w.double().abs(), None, r) + bias.double().abs()[None, :, None]).transpose(1, 2)
        flip = D.sconvtr(near.double() * _ulp16(a), w.double().abs(), None, r).transpose(1, 2)
        assert got.shape == ref.shape == (B, L * r, Co)
        bound = (2 * C + 2) * 2.0 ** -24 * mag + flip + 2.0 ** -11 * ref.abs() + 2.0 ** -25
        err = (got - ref).abs()
        ratio = float((err / bound).max())
        print(f"seanet convtr {C}-{Co} r {r} L {L} (tile <= {tile}): max |err| {float(err.max()):.3e}, max |err| / bound {ratio:.4f}, "
              f"operands near an fp16 boundary {int(near.sum())}")
        assert bool((err <= bound).all()), (C, r, L, ratio)


# ------------------------------------------------------------------------------------ the last convolution
@gpu
@pytest.mark.parametrize("nf,k", [(32, 7), (64, 7), (16, 3), (8, 1)])
def test_last_convolution(nf, k):
    """nf -> 1: lengths 1, the longest the short-input rule still serves and that plus 1, and 1025 (five blocks of 256 samples)"""
    from voicebox_pytorch_amd import _lib

    g = torch.Generator().manual_seed(nf + k)
    w = torch.randn(1, nf, k, generator=g) / (nf * k) ** 0.5
    bias = 0.1 * torch.randn(1, generator=g)
    wk = w[0].t().contiguous().to(dev)  # fp32 [k, nf]
    short = (k - 1) // 2  # pad_left = pad_right = (k - 1) / 2: the rule applies for L <= that
    for L in sorted({1, max(short, 1), short + 1, 1025}):
        x = torch.randn(2, L, nf, generator=g).half()
        x[1] = -0.75
        y = torch.full((3, L), float("nan"), dtype=torch.float32, device=dev)
        args = (x.to(dev), wk, bias.to(dev), y, 2, L, nf, k, _lib.current_stream())
        _lib.call("vbx_seanet_conv_out", *args)
        first = y.clone()
        _lib.call("vbx_seanet_conv_out", *args)
        assert torch.equal(first[:2], y[:2]) and bool(torch.isnan(y[2]).all())
        got = y[:2].double().cpu()
        assert bool(torch.isfinite(got).all())
        a = F.elu(x.double()).transpose(1, 2)
        ref = S.sconv(a, w.double(), bias.double())[:, 0]
        mag = (S.sconv(a.abs(), w.double().abs(), None) + bias.double().abs()[None, :, None])[:, 0]
        bound = (k * nf + 6) * 2.0 ** -24 * mag
        err = (got - ref).abs()
        print(f"seanet conv_out nf {nf} k {k} L {L}: max |err| {float(err.max()):.3e}, max |err| / bound {float((err / bound).max()):.4f}")
        assert got.shape == ref.shape and bool((err <= bound).all()), (nf, k, L)


@gpu
def test_pack_latents_rounds_once():
    from voicebox_pytorch_amd import _lib

    for B, Dm, T in ((2, 128, 70), (3, 32, 1), (1, 40, 33)):
        z = _latents(B, Dm, T, Dm)
        y = torch.full((B + 1, T, Dm), float("nan"), dtype=torch.float16, device=dev)
        _lib.call("vbx_seanet_pack_latents", z.to(dev), y, B, Dm, T, _lib.current_stream())
        assert torch.equal(y[:B].cpu(), z.transpose(1, 2).half()) and bool(torch.isnan(y[B]).all())


# ------------------------------------------------------------------------------------ the whole decoder
DECODER_CASES = [("real", 2, 1), ("real", 2, 11), ("real", 2, 70), ("small", 3, 1), ("small", 3, 2), ("small", 3, 150)]


@functools.lru_cache(maxsize=None)
def _reference(name, B, frames, seed):
    cfg = D.SMALL if name == "small" else D.config()
    sd = D.random_state(cfg, seed)
    z = _latents(B, cfg["dimension"], frames, seed)
    return sd, z, D.decode(sd, cfg, z, emulate=True), D.decode(sd, cfg, z)


def _decoder(name, sd):
    import voicebox_pytorch_amd as vbx

    dec = vbx.SEANetDecoder(**(SMALL_KW if name == "small" else {}))
    dec.load_state_dict(sd)
    return dec.to(dev).eval()


@gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name,B,frames", DECODER_CASES, ids=[f"{n}-B{b}-F{t}" for n, b, t in DECODER_CASES])
def test_decoder_parity(name, B, frames, seed):
    sd, z, emu, ref = _reference(name, B, frames, seed)
    dec = _decoder(name, sd)
    got = dec(z.to(dev))
    assert got.dtype == torch.float32 and got.shape == ref.shape == (B, frames * dec.hop_length) and got.is_contiguous()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, dec(z.to(dev)))  # reruns: the same bits
    assert torch.equal(got, dec(z.double().to(dev)))  # other float dtypes
    a, bb = D.rel_err(got, emu), D.rel_err(got, ref)
    bound_a, bound_b = (BOUND_A_SMALL, BOUND_B_SMALL) if name == "small" else (BOUND_A_REAL, BOUND_B_REAL)
    print(f"seanet decoder {name} B {B} frames {frames} seed {seed}: max |delta| / RMS vs emulated {a:.3e} (bound {bound_a}), "
          f"vs fp64 {bb:.3e} (bound {bound_b}); emulated vs fp64 {D.rel_err(emu, ref):.3e}")
    assert a <= bound_a, (name, B, frames, seed, a)
    assert bb <= bound_b, (name, B, frames, seed, bb)


@gpu
@pytest.mark.parametrize("name,B,frames", [("real", 2, 70), ("small", 3, 150), ("small", 3, 1)])
def test_a_row_alone_is_the_row_in_the_batch(name, B, frames):
    sd, z, _, _ = _reference(name, B, frames, 0)
    dec = _decoder(name, sd)
    got = dec(z.to(dev))
    for b in range(B):
        assert torch.equal(dec(z[b:b + 1].to(dev))[0], got[b]), (name, frames, b)


# ------------------------------------------------------------------------------------ codec and model
def _codec(tmp_path, seed=0):
    import voicebox_pytorch_amd as vbx

    sd = {"encoder." + k: v for k, v in S.random_state(dict(S.DEFAULT, **SMALL_KW), seed).items()}
    sd.update({"decoder." + k: v for k, v in D.random_state(D.SMALL, seed + 10).items()})
    g = torch.Generator().manual_seed(seed)
    for q in range(4):
        sd[f"quantizer.vq.layers.{q}._codebook.embed"] = 0.5 ** q * torch.randn(64, 32, generator=g)
    path = tmp_path / "encodec_small.pt"
    torch.save(sd, path)
    return vbx.EncodecVocoCodec.from_encodec_checkpoint(str(path)).to(dev).eval()


@gpu
def test_one_file_is_a_complete_codec(tmp_path):
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    codec = _codec(tmp_path)
    dec = codec.vocoder
    assert isinstance(dec, vbx.SEANetDecoder) and codec.downsample_factor == 10
    wave = (0.3 * torch.randn(2, 190, generator=torch.Generator().manual_seed(1))).to(dev)
    frames = codec.encoder.frames(190)
    assert frames == 19
    lat = codec.encode(wave)
    out = codec.decode(lat)
    assert out.shape == (2, frames * 10) and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert torch.equal(out, dec(codec.codes_to_features(codec.decode_to_codes(lat))))
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
    assert sampled.shape == (2, frames * 10) and sampled.dtype == torch.float32 and bool(torch.isfinite(sampled).all())


@gpu
def test_weights_repack_on_version_bump_or_mark_dirty():
    sd, z, _, _ = _reference("small", 3, 2, 1)
    dec = _decoder("small", sd)
    zd = z.to(dev)
    base = dec(zd)
    p = dec.model[3].convtr.convtr.weight_g
    p.data.mul_(2)  # through .data: neither the version counter nor the storage moves
    assert torch.equal(dec(zd), base)
    dec.mark_weights_dirty()
    doubled = dec(zd)
    assert not torch.equal(doubled, base)
    with torch.no_grad():
        p.mul_(0.5)  # in place: the version counter moves, the operands are packed again
    assert torch.equal(dec(zd), base)
