"""Host-side tests of voicebox_pytorch_amd.CausalSEANetEncoder / CausalSEANetDecoder: the fp64 restatement
tests/seanet_causal_ref.py against an independent construction from torch's own modules (padding and trimming written out again
here), the planted faults and the tolerance they give the GPU tests, constructors and loaders, that the restatement is causal
where EnCodec's causal form is, and the one-reflection-per-side rule of the kernels' padding.  Parity with the `encodec` library
itself is UNPINNED."""
import math

import pytest
import torch
from torch import nn
from torch.nn.utils.parametrizations import weight_norm

import seanet_causal_ref as C
import seanet_dec_ref as D
import seanet_ref as S


# ------------------------------------------------------------------------------------ the restatement
class _CausalConv(nn.Module):
    """EnCodec's SConv1d at causal=True from nn.Conv1d under torch's weight norm"""

    def __init__(self, ci, co, k, stride=1, dilation=1):
        super().__init__()
        self.conv = weight_norm(nn.Conv1d(ci, co, k, stride=stride, dilation=dilation))
        self.k_eff, self.stride = (k - 1) * dilation + 1, stride

    def load(self, sd, prefix):
        self.conv.parametrizations.weight.original0.data.copy_(sd[f"{prefix}.conv.conv.weight_g"])
        self.conv.parametrizations.weight.original1.data.copy_(sd[f"{prefix}.conv.conv.weight_v"])
        self.conv.bias.data.copy_(sd[f"{prefix}.conv.conv.bias"])
        return self

    def forward(self, x):
        n = x.shape[-1]
        total = self.k_eff - self.stride
        n_frames = (n - self.k_eff + total) / self.stride + 1  # encodec's get_extra_padding_for_conv1d
        extra = (math.ceil(n_frames) - 1) * self.stride + (self.k_eff - total) - n
        grow = max(total, extra) - n + 1 if n <= max(total, extra) else 0  # pad1d: reflect needs a row longer than the padding
        y = nn.functional.pad(nn.functional.pad(x, (0, grow)), (total, extra), mode="reflect")
        return self.conv(y[..., :total + n + extra])


class _CausalConvTr(nn.Module):
    """EnCodec's SConvTranspose1d at causal=True from nn.ConvTranspose1d under torch's weight norm (dim 0: per input channel)"""

    def __init__(self, ci, co, k, stride, ratio):
        super().__init__()
        self.convtr = weight_norm(nn.ConvTranspose1d(ci, co, k, stride=stride))
        self.keep_from = (k - stride) - math.ceil((k - stride) * ratio)
        self.stride = stride

    def load(self, sd, prefix):
        self.convtr.parametrizations.weight.original0.data.copy_(sd[f"{prefix}.convtr.convtr.weight_g"])
        self.convtr.parametrizations.weight.original1.data.copy_(sd[f"{prefix}.convtr.convtr.weight_v"])
        self.convtr.bias.data.copy_(sd[f"{prefix}.convtr.convtr.bias"])
        return self

    def forward(self, x):
        return self.convtr(x)[..., self.keep_from:self.keep_from + x.shape[-1] * self.stride]


class _Independent(nn.Module):
    def __init__(self, entries, sd, ratio=1.0):
        super().__init__()
        mods = []
        for e in entries:
            i, kind = e[0], e[1]
            if kind == "elu":
                mods.append(nn.ELU())
            elif kind == "conv":
                mods.append(_CausalConv(e[2], e[3], e[4], stride=e[5] if len(e) > 5 else 1).load(sd, f"model.{i}"))
            elif kind == "convtr":
                mods.append(_CausalConvTr(e[2], e[3], e[4], e[5], ratio).load(sd, f"model.{i}"))
            elif kind == "res":
                a = _CausalConv(e[2], e[3], e[4], dilation=e[5]).load(sd, f"model.{i}.block.1")
                b = _CausalConv(e[3], e[2], 1).load(sd, f"model.{i}.block.3")
                sc = _CausalConv(e[2], e[2], 1).load(sd, f"model.{i}.shortcut")
                mods.append(nn.ModuleDict(dict(block=nn.Sequential(nn.ELU(), a, nn.ELU(), b), shortcut=sc)))
            else:
                l = nn.LSTM(e[2], e[2], e[3])
                l.load_state_dict({k.split(".lstm.")[1]: v for k, v in sd.items() if k.startswith(f"model.{i}.lstm.")})
                mods.append(l)
        self.mods = nn.ModuleList(mods)

    def forward(self, x):
        for m in self.mods:
            if isinstance(m, nn.ModuleDict):
                x = m["shortcut"](x) + m["block"](x)
            elif isinstance(m, nn.LSTM):
                t = x.permute(2, 0, 1)  # SLSTM: time first
                x = (m(t)[0] + t).permute(1, 2, 0)
            else:
                x = m(x)
        return x


def _close(got, want):
    return got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


ENC_SHAPES = [(n, T) for n in C.ENC_CONFIGS for T in C.ENC_T] + [("real", 24000)]
DEC_SHAPES = [(n, f) for n in C.DEC_CONFIGS for f in C.DEC_FRAMES] + [("real", 75)]


@pytest.mark.parametrize("name", list(C.ENC_CONFIGS) + ["real"])
def test_encoder_restatement_equals_module_construction(name):
    cfg = C.REAL if name == "real" else C.ENC_CONFIGS[name][0]
    net = None
    for n, T in ENC_SHAPES:
        if n != name:
            continue
        sd, wave, _, got = C.encoder_case(name, T)
        net = net or _Independent(C.layout(cfg), sd).double().eval()
        with torch.no_grad():
            want = net(wave.double()[:, None]).transpose(1, 2)
        assert got.shape == (wave.shape[0], C.frames(cfg, T), cfg["dimension"])
        assert _close(got, want), (name, T)


@pytest.mark.parametrize("name", list(C.DEC_CONFIGS) + ["real"])
def test_decoder_restatement_equals_module_construction(name):
    cfg = C.REAL if name == "real" else C.DEC_CONFIGS[name][0]
    net = None
    for n, fr in DEC_SHAPES:
        if n != name:
            continue
        sd, z, _, got = C.decoder_case(name, fr)
        net = net or _Independent(D.layout(cfg), sd, ratio=cfg.get("trim_right_ratio", 1.0)).double().eval()
        with torch.no_grad():
            want = net(z.double())[:, 0]
        assert got.shape == (z.shape[0], fr * C.hop(cfg))
        assert _close(got, want), (name, fr)


def test_the_causal_form_is_not_the_non_causal_one():
    """the same weights and inputs through tests/seanet_ref.py / seanet_dec_ref.py: far apart (the GPU tests could tell)"""
    sd, wave, _, ref = C.encoder_case("small-r1", 192)
    assert C.rel_err(S.encode(sd, C.ENC_CONFIGS["small-r1"][0], wave), ref) > 0.1
    sd, z, _, ref = C.decoder_case("small-r1", 24)
    assert C.rel_err(D.decode(sd, C.DEC_CONFIGS["small-r1"][0], z), ref) > 0.1


# ------------------------------------------------------------------------------------ the planted faults and the tolerance
def test_every_fault_moves_the_output_and_the_tolerance_holds_the_reference():
    """The recipe of tests/test_seanet_cpu.py, measured here: every planted fault's smallest movement (max |delta| / RMS) over the
    GPU tests' SMALL inputs on which it can show; one tenth of the smallest of them is the whole-network tolerance of
    tests/test_seanet_causal_gpu.py.  The emulated-precision restatement must lie inside it against the fp64 one on every input
    of the GPU tests: the reference alone stays within the tolerance."""
    enc, dec = C.fault_movements()
    tol = C.tolerance()
    print("encoder, smallest max|delta|/RMS per fault:", {k: f"{v:.3g}" for k, v in enc.items()})
    print("decoder, smallest max|delta|/RMS per fault:", {k: f"{v:.3g}" for k, v in dec.items()})
    print(f"smallest movement {10 * tol:.4g}: whole-network tolerance {tol:.4g}")
    assert set(enc) == set(C.ENC_FAULTS) and set(dec) == set(C.DEC_FAULTS) and set(enc) | set(dec) == set(C.FAULTS)
    assert all(v > 0 and math.isfinite(v) for v in list(enc.values()) + list(dec.values()))
    worst = 0.0
    for name, T in ENC_SHAPES:
        _, _, emu, ref = C.encoder_case(name, T)
        worst = max(worst, C.rel_err(emu, ref))
        assert C.rel_err(emu, ref) <= tol, ("encoder", name, T)
    for name, fr in DEC_SHAPES:
        _, _, emu, ref = C.decoder_case(name, fr)
        worst = max(worst, C.rel_err(emu, ref))
        assert C.rel_err(emu, ref) <= tol, ("decoder", name, fr)
    print(f"emulated precision against fp64, worst over the GPU tests' inputs: {worst:.4g}")


def test_ratio_floor_shows_only_at_an_odd_stride_and_half_ratio():
    assert C.trims(5, 0.5) == (2, 3) and C.trims(5, 0.5, "ratio_floor") == (3, 2)
    assert C.trims(2, 0.5) == C.trims(2, 0.5, "ratio_floor") == (1, 1) and C.trims(5, 1.0) == C.trims(5, 1.0, "ratio_floor") == (0, 5)
    assert C.trims(8, 1.0) == (0, 8) and C.trims(8, 0.0) == (8, 0) and C.trims(8, 1.0, "trim_split") == (4, 4)
    assert C.trims(5, 1.0, "trim_left_instead") == (5, 0)


# ------------------------------------------------------------------------------------ constructors and loaders
def test_constructors():
    import voicebox_pytorch_amd as vbx

    small = dict(n_filters=16, ratios=(4, 2), dimension=32)
    for cls, base in ((vbx.CausalSEANetEncoder, vbx.SEANetEncoder), (vbx.CausalSEANetDecoder, vbx.SEANetDecoder)):
        assert issubclass(cls, base)
        assert cls(**small).causal is True and cls(causal=True, **small).causal is True
        assert base(**small).causal is False
        with pytest.raises(ValueError, match=base.__name__):
            cls(causal=False, **small)
        with pytest.raises(NotImplementedError, match=base.__name__):  # the other limits are the base class's
            cls(true_skip=True, **small)
        with pytest.raises(NotImplementedError, match="Causal" + base.__name__):  # the refusal names the way out
            base(causal=True, **small)
        assert {k: tuple(v.shape) for k, v in cls(**small).state_dict().items()} == \
            {k: tuple(v.shape) for k, v in base(**small).state_dict().items()}
    dec = vbx.CausalSEANetDecoder(**small)
    assert dec.trim_right_ratio == 1.0 and [dec.trim_left(r) for r in (2, 5, 8)] == [0, 0, 0]
    half = vbx.CausalSEANetDecoder(trim_right_ratio=0.5, **small)
    assert [half.trim_left(r) for r in (2, 5, 8)] == [1, 2, 4]  # 5 - ceil(2.5)
    zero = vbx.CausalSEANetDecoder(trim_right_ratio=0.0, **small)
    assert [zero.trim_left(r) for r in (2, 5, 8)] == [2, 5, 8]
    assert [vbx.SEANetDecoder(**small).trim_left(r) for r in (2, 5, 8)] == [1, 3, 4]
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="trim_right_ratio"):
            vbx.CausalSEANetDecoder(trim_right_ratio=bad, **small)
    with pytest.raises(NotImplementedError, match="SEANetDecoder"):
        vbx.SEANetDecoder(trim_right_ratio=0.5, **small)
    assert "CausalSEANetEncoder" in vbx.__all__ and "CausalSEANetDecoder" in vbx.__all__


def _other_layouts(sd, half):
    par = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v
           for k, v in sd.items()}
    whole = {f"{half}." + k: v for k, v in sd.items()}
    whole["quantizer.vq.layers.0._codebook.embed"] = torch.zeros(4, 32)
    return par, whole


def test_three_layouts_loaders_and_dirty_marks():
    import voicebox_pytorch_amd as vbx

    for cls, half, sd in ((vbx.CausalSEANetEncoder, "encoder", C.random_state(C.SMALL, 3)),
                          (vbx.CausalSEANetDecoder, "decoder", C.decoder_state(C.SMALL, 3))):
        nets = [cls.from_state_dict(d) for d in (sd,) + _other_layouts(sd, half)]
        assert all(type(n) is cls and n.causal and not n.training and n.ratios == (4, 2) for n in nets)
        ref = nets[0].folded_weights()
        for n in nets[1:]:
            assert all(torch.equal(n.folded_weights()[k], ref[k]) for k in ref)
        ops = nets[0].packed_ops()
        assert ops is nets[0].packed_ops()
        nets[0].mark_weights_dirty()
        assert nets[0].packed_ops() is not ops


def test_from_checkpoint_keeps_the_class_and_the_ratio(tmp_path):
    import voicebox_pytorch_amd as vbx

    cfg = dict(C.SMALL, ratios=(5, 2))
    path = tmp_path / "dec.pt"
    torch.save({"state_dict": {"decoder." + k: v for k, v in C.decoder_state(cfg, 1).items()}}, path)
    dec = vbx.CausalSEANetDecoder.from_checkpoint(str(path), trim_right_ratio=0.5)
    assert type(dec) is vbx.CausalSEANetDecoder and dec.ratios == (5, 2) and dec.trim_right_ratio == 0.5 and dec.hop_length == 10
    assert type(vbx.SEANetDecoder.from_checkpoint(str(path))) is vbx.SEANetDecoder
    path = tmp_path / "enc.pt"
    torch.save({"encoder." + k: v for k, v in C.random_state(cfg, 1).items()}, path)
    assert type(vbx.CausalSEANetEncoder.from_checkpoint(str(path))) is vbx.CausalSEANetEncoder


def synthetic_encodec_file(tmp_path, seed=0):
    """a file of the published layout at the SMALL widths: encoder.*, decoder.*, four codebooks of 64 x 32"""
    sd = {"encoder." + k: v for k, v in C.random_state(C.SMALL, seed).items()}
    sd.update({"decoder." + k: v for k, v in C.decoder_state(C.SMALL, seed + 10).items()})
    g = torch.Generator().manual_seed(seed)
    for q in range(4):
        sd[f"quantizer.vq.layers.{q}._codebook.embed"] = 0.5 ** q * torch.randn(64, 32, generator=g)
    path = tmp_path / "encodec_small.pt"
    torch.save(sd, path)
    return str(path), sd


def test_from_encodec_checkpoint_builds_what_it_is_asked_for(tmp_path):
    import voicebox_pytorch_amd as vbx

    path, sd = synthetic_encodec_file(tmp_path)
    causal = vbx.EncodecVocoCodec.from_encodec_checkpoint(path, causal=True)
    assert type(causal.encoder) is vbx.CausalSEANetEncoder and type(causal.vocoder) is vbx.CausalSEANetDecoder
    assert causal.vocoder.trim_right_ratio == 1.0 and causal.downsample_factor == 8 and causal.rvq.num_quantizers == 4
    half = vbx.EncodecVocoCodec.from_encodec_checkpoint(path, causal=True, trim_right_ratio=0.5)
    assert half.vocoder.trim_right_ratio == 0.5
    voc = nn.Identity()
    mixed = vbx.EncodecVocoCodec.from_encodec_checkpoint(path, causal=True, vocoder=voc)
    assert type(mixed.encoder) is vbx.CausalSEANetEncoder and mixed.vocoder is voc
    for plain in (vbx.EncodecVocoCodec.from_encodec_checkpoint(path), vbx.EncodecVocoCodec.from_encodec_checkpoint(path, causal=False)):
        assert type(plain.encoder) is vbx.SEANetEncoder and type(plain.vocoder) is vbx.SEANetDecoder
        assert not plain.encoder.causal and not plain.vocoder.causal
    for a, b in ((causal.encoder, plain.encoder), (causal.vocoder, plain.vocoder)):  # the same weights either way: only the class differs
        assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    with pytest.raises(ValueError, match="trim_right_ratio"):
        vbx.EncodecVocoCodec.from_encodec_checkpoint(path, trim_right_ratio=0.5)


# ------------------------------------------------------------------------------------ causality of the restatement
# Causal EnCodec is NOT causal at the very start of a signal: reflect padding makes output 0 read inputs 1 .. padding_total.  So
# the perturbation sits late: SMALL (hop 8), T = 192 = 24 frames, samples >= 160 = frames >= 20.
CAUSAL_T, CAUSAL_FROM = 192, 160


def causality_inputs():
    """(encoder state, wave, perturbed wave, decoder state, latents, perturbed latents): what the GPU causality test perturbs too"""
    sd, wave, _, _ = C.encoder_case("small-r1", CAUSAL_T)
    wave2 = wave.clone()
    wave2[:, CAUSAL_FROM:] += 0.1 * torch.randn(wave.shape[0], CAUSAL_T - CAUSAL_FROM, generator=torch.Generator().manual_seed(7))
    dsd, z, _, _ = C.decoder_case("small-r1", CAUSAL_T // 8)
    z2 = z.clone()
    z2[:, :, CAUSAL_FROM // 8:] += torch.randn(z.shape[0], z.shape[1], (CAUSAL_T - CAUSAL_FROM) // 8, generator=torch.Generator().manual_seed(8))
    return sd, wave, wave2, dsd, z, z2


def test_the_restatement_is_causal_late_in_the_signal():
    sd, wave, wave2, dsd, z, z2 = causality_inputs()
    cfg, f0 = C.ENC_CONFIGS["small-r1"][0], CAUSAL_FROM // 8
    assert C.frames(cfg, CAUSAL_T) == 24 and f0 == 20
    a, b = C.encode(sd, cfg, wave), C.encode(sd, cfg, wave2)
    assert torch.equal(a[:, :f0], b[:, :f0]) and not torch.equal(a[:, f0:], b[:, f0:])
    fa, fb = C.encode(sd, cfg, wave, fault="noncausal_pads"), C.encode(sd, cfg, wave2, fault="noncausal_pads")
    assert not torch.equal(fa[:, f0 - 1], fb[:, f0 - 1])  # the non-causal padding looks ahead: frame 19 moves
    na, nb = S.encode(sd, cfg, wave), S.encode(sd, cfg, wave2)
    assert not torch.equal(na[:, f0 - 1], nb[:, f0 - 1])  # and so does the non-causal network itself
    dcfg = C.DEC_CONFIGS["small-r1"][0]
    a, b = C.decode(dsd, dcfg, z), C.decode(dsd, dcfg, z2)
    assert a.shape == (2, CAUSAL_T)
    assert torch.equal(a[:, :CAUSAL_FROM], b[:, :CAUSAL_FROM]) and not torch.equal(a[:, CAUSAL_FROM:], b[:, CAUSAL_FROM:])
    fa, fb = C.decode(dsd, dcfg, z, fault="noncausal_pads"), C.decode(dsd, dcfg, z2, fault="noncausal_pads")
    assert not torch.equal(fa[:, CAUSAL_FROM - 1], fb[:, CAUSAL_FROM - 1])
    fa, fb = C.decode(dsd, dcfg, z, fault="trim_split"), C.decode(dsd, dcfg, z2, fault="trim_split")
    assert not torch.equal(fa[:, CAUSAL_FROM - 1], fb[:, CAUSAL_FROM - 1])
    # and at the start it is not: output frame 0 reads the reflection of samples 1 .. 6
    early = wave.clone()
    early[:, 3] += 0.1
    assert not torch.equal(C.encode(sd, cfg, early)[:, 0], C.encode(sd, cfg, wave)[:, 0])


# ------------------------------------------------------------------------------------ the kernels' padding rule, on the host
def _device_source(q, k, stride, dil, L, causal):
    """csrc/seanet.hip's sn_pads and sn_src, restated: the sample a padded position reads (None: an appended zero)"""
    total, extra = (k - 1) * dil + 1 - stride, -(-L // stride) * stride - L
    right = 0 if causal else total // 2
    left = total - right
    Lz = max(L, max(left, right + extra) + 1)
    i = q - left
    if i < 0:
        i = -i
    if i >= Lz:
        i = 2 * (Lz - 1) - i
    assert 0 <= i < Lz, "a second reflection would be needed"
    return i if i < L else None


def test_one_reflection_per_side_suffices_in_either_form():
    """every convolution the SEANet classes launch -- the largest padding_total is 8: k 16 at stride 8, k 3 at dilation 4 --, every
    length up to twice its span: the device's index rule reads what pad1d puts there"""
    shapes = [(7, 1, 1), (5, 1, 1), (3, 1, 1), (1, 1, 1), (3, 1, 2), (3, 1, 4)] + [(2 * r, r, 1) for r in range(2, 9)]
    assert max((k - 1) * d + 1 - s for k, s, d in shapes) == 8
    for k, stride, dil in shapes:
        for causal in (False, True):
            for L in range(1, 2 * ((k - 1) * dil + 1) + stride + 2):
                x = torch.arange(1.0, L + 1)[None, None]
                left, right = C.conv_pads(L, k, stride, dil) if causal else (lambda a, b, c: (a, b + c))(*S.conv_pads(L, k, stride, dil))
                want = S.pad1d(x, left, right)[0, 0].tolist()
                got = [_device_source(q, k, stride, dil, L, causal) for q in range(len(want))]
                assert [0.0 if i is None else i + 1.0 for i in got] == want, (k, stride, dil, causal, L)
