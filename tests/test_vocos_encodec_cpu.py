"""Host side of VocosEncodecDecoder (published layout, argument checks, the padding keyword of from_vocos_checkpoint) and checks of
tests/vocos_same_ref.py itself, the yardstick of tests/test_vocos_encodec_gpu.py: its hand-written "same" ISTFT against the way
Vocos writes it (torch.fft.irfft + F.fold) and against torch.istft, its AdaLayerNorm network against vocos_ref.decode of the folded
dict, and its emulation of the kernel's mixed-radix inverse transform (index map, stage order, table lookups) against torch.fft.ifft."""
import pytest
import torch
import torch.nn.functional as F

import vocos_ref as vr
import vocos_same_ref as sr
from test_vocos_encodec_gpu import BOUND_A, SEEDS, WHOLE, istft_bound, random_spectrum, whole_inputs

SMALL_ARGS = dict(input_channels=16, dim=64, intermediate_dim=192, num_layers=2, n_fft=320, hop_length=80)


def vocos_istft_same(spec, n_fft, hop, window):
    """ISTFT.forward of the vocos library at padding="same", as published (win_length = n_fft)"""
    pad = (n_fft - hop) // 2
    B, N, T = spec.shape
    ifft = torch.fft.irfft(spec, n_fft, dim=1, norm="backward") * window[None, :, None]
    output_size = (T - 1) * hop + n_fft
    y = F.fold(ifft, output_size=(1, output_size), kernel_size=(1, n_fft), stride=(1, hop))[:, 0, 0, pad:-pad]
    window_sq = window.square().expand(1, T, -1).transpose(1, 2)
    env = F.fold(window_sq, output_size=(1, output_size), kernel_size=(1, n_fft), stride=(1, hop)).squeeze()[pad:-pad]
    assert (env > 1e-11).all()
    return y / env


@pytest.mark.parametrize("n_fft,hop,frames", [(320, 80, 1), (320, 80, 9), (320, 81, 5), (1280, 320, 12), (256, 64, 2), (640, 200, 7)])
def test_istft_same_is_vocos(n_fft, hop, frames):
    spec = random_spectrum(2, n_fft, frames, seed=n_fft + frames)[2]
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    got = sr.istft_same(spec, n_fft, hop, window)
    ref = vocos_istft_same(spec, n_fft, hop, window)
    pad = (n_fft - hop) // 2
    assert got.shape == ref.shape == (2, (frames - 1) * hop + n_fft - 2 * pad)
    if (n_fft - hop) % 2 == 0:
        assert got.shape[1] == frames * hop
    assert float((got - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("n_fft,hop,frames", [(320, 80, 9), (1280, 320, 5), (256, 64, 4)])
def test_istft_same_meets_torch_istft_where_both_keep(n_fft, hop, frames):
    """even win - hop: "same" keeps [pad, total - pad), center keeps [n_fft / 2, total - n_fft / 2); the envelope is the same sum"""
    spec = random_spectrum(2, n_fft, frames, seed=7)[2]
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    same = sr.istft_same(spec, n_fft, hop, window)
    spec_r = spec.clone()  # torch.istft refuses nothing here, but it is a c2r transform: the same dropped imaginary parts
    center = torch.istft(spec_r, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True)
    off = n_fft // 2 - (n_fft - hop) // 2
    assert float((same[:, off:off + center.shape[1]] - center).abs().max()) < 1e-12
    assert float((sr.istft_same(spec, n_fft, hop, window, padding="center") - center).abs().max()) < 1e-12


@pytest.mark.parametrize("n", [320, 640, 1280])
def test_emulated_mixed_radix_inverse(n):
    g = torch.Generator().manual_seed(n)
    z = torch.complex(torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64))
    got, writes = sr.mixed_radix_inverse(z)
    ref = torch.fft.ifft(z) * n
    assert float((got - ref).abs().max()) < 1e-10
    used = {sr.skew(i) for i in range(n)}
    assert len(writes) == n + (n >> 6) and len(used) == n
    assert all(w == (1 if i in used else 0) for i, w in enumerate(writes))  # the input map is a permutation onto the skewed slots
    bad, _ = sr.mixed_radix_inverse(z, fault=("r5_twiddle_conj",))
    assert float((bad - ref).abs().max()) > 1.0


def test_restated_network_is_vocos_ref_of_the_folded_dict():
    sd = sr.random_state(16, 64, 192, 2, 320, seed=3)
    x = torch.randn(2, 16, 9, generator=torch.Generator().manual_seed(4))
    for emulate in (False, True):
        a = sr.decode(sd, x, n_fft=320, hop=80, bandwidth_id=1, padding="center", emulate=emulate)
        b = vr.decode(sr.fold(sd, 1), x, n_fft=320, hop=80, emulate=emulate)
        assert a.shape == b.shape == (2, 640) and float((a - b).abs().max()) < 1e-10 * float(b.abs().max())
    assert sr.decode(sd, x, n_fft=320, hop=80, bandwidth_id=1).shape == (2, 720)
    assert torch.equal(sd["backbone.norm.scale.weight"][0], vr.random_state(16, 64, 192, 2, 320, 3)["backbone.norm.weight"])


# ----------------------------------------------------------------------------- the class
def published_shapes(C, dim, inter, layers, n_fft, rows):
    s = {"backbone.embed.weight": (dim, C, 7), "backbone.embed.bias": (dim,), "head.out.weight": (n_fft + 2, dim),
         "head.out.bias": (n_fft + 2,), "head.istft.window": (n_fft,), "backbone.final_layer_norm.weight": (dim,),
         "backbone.final_layer_norm.bias": (dim,)}
    for name in ["backbone.norm"] + [f"backbone.convnext.{i}.norm" for i in range(layers)]:
        s[name + ".scale.weight"] = s[name + ".shift.weight"] = (rows, dim)
    for i in range(layers):
        p = f"backbone.convnext.{i}."
        s.update({p + "dwconv.weight": (dim, 1, 7), p + "dwconv.bias": (dim,), p + "pwconv1.weight": (inter, dim),
                  p + "pwconv1.bias": (inter,), p + "pwconv2.weight": (dim, inter), p + "pwconv2.bias": (dim,), p + "gamma": (dim,)})
    return s


def test_default_is_the_published_configuration():
    import voicebox_pytorch_amd as vbx

    m = vbx.VocosEncodecDecoder()
    assert isinstance(m, vbx.VocosDecoder)
    assert (m.input_channels, m.dim, m.intermediate_dim, m.num_layers, m.n_fft, m.hop_length, m.padding, m.adanorm_num_embeddings,
            m.bandwidth_id, m.input_log) == (128, 384, 1152, 8, 1280, 320, "same", 4, 2, False)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == published_shapes(128, 384, 1152, 8, 1280, 4)
    assert torch.equal(m.head.istft.window, torch.hann_window(1280, periodic=True))
    n = m.backbone.convnext[3].norm
    assert float(n.scale.weight.detach().min()) == 1.0 == float(n.scale.weight.detach().max()) and float(n.shift.weight.detach().abs().max()) == 0.0
    assert float(m.backbone.convnext[0].gamma[0].detach()) == pytest.approx(1.0 / 8)


def test_published_layout_loads_as_is(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = sr.random_state(16, 64, 192, 2, 320, seed=0, rows=4, codebooks=5)
    m = vbx.VocosEncodecDecoder(**SMALL_ARGS)
    m.load_state_dict(sd, strict=True)  # feature_extractor.* skipped
    kept = {k: v for k, v in sd.items() if not k.startswith("feature_extractor.")}
    got = m.state_dict()
    assert set(got) == set(kept) and all(torch.equal(got[k], kept[k]) for k in kept)
    for payload, rows in ((sd, 4), ({"state_dict": sr.random_state(16, 64, 192, 2, 320, seed=1, rows=3)}, 3)):
        path = str(tmp_path / f"vocos_encodec_{rows}.pt")
        torch.save(payload, path)
        m2 = vbx.VocosEncodecDecoder.from_checkpoint(path, bandwidth_id=1)
        assert (m2.input_channels, m2.dim, m2.intermediate_dim, m2.num_layers, m2.n_fft, m2.hop_length) == (16, 64, 192, 2, 320, 80)
        assert (m2.adanorm_num_embeddings, m2.bandwidth_id, m2.padding) == (rows, 1, "same") and not m2.training
    m3 = vbx.VocosEncodecDecoder.from_state_dict(sd, hop_length=100, padding="center", bandwidth_id=3)
    assert (m3.hop_length, m3.padding, m3.bandwidth_id) == (100, "center", 3)
    plain = vbx.VocosEncodecDecoder.from_state_dict(vr.random_state(16, 64, 192, 2, 320, 0))  # plain LayerNorms: a "same"-padded Vocos
    assert plain.adanorm_num_embeddings is None and plain.bandwidth_id is None and plain.padding == "same"
    assert "backbone.norm.weight" in plain.state_dict()
    with pytest.raises(ValueError, match="bandwidth_id 4"):
        vbx.VocosEncodecDecoder.from_state_dict(sd, bandwidth_id=4)


def test_arguments():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    m = vbx.VocosEncodecDecoder(**SMALL_ARGS)
    x = torch.zeros(1, 16, 4)
    for bad in (4, -1):
        with pytest.raises(ValueError, match="bandwidth_id"):
            m(x, bandwidth_id=bad)
    with pytest.raises(TypeError, match="Python int"):
        m(x, bandwidth_id=torch.tensor(1))
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
        m(x)
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
        m.decode(x, bandwidth_id=0)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 17, 4))
    with pytest.raises(ValueError, match="bandwidth_id"):
        vbx.VocosEncodecDecoder(**SMALL_ARGS, bandwidth_id=7)
    with pytest.raises(ValueError, match="padding"):
        vbx.VocosEncodecDecoder(**SMALL_ARGS, padding="reflect")
    with pytest.raises(ValueError, match="no bandwidth_id"):
        vbx.VocosEncodecDecoder(**SMALL_ARGS, adanorm_num_embeddings=None)(x, bandwidth_id=0)
    for bad in (dict(n_fft=384), dict(n_fft=160), dict(n_fft=2560), dict(n_fft=1000), dict(dim=96)):
        with pytest.raises(NotImplementedError):
            vbx.VocosEncodecDecoder(**{**SMALL_ARGS, **bad})
    with pytest.raises(NotImplementedError, match="keeps no sample"):  # center padding of one frame
        vbx.VocosEncodecDecoder(**SMALL_ARGS, padding="center")(torch.zeros(1, 16, 1))
    with pytest.raises(ValueError, match="NOLA"):  # a Hann window hopping by its whole length: zero at the first kept sample
        vbx.VocosEncodecDecoder(**{**SMALL_ARGS, "hop_length": 320})(x)
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):  # one frame is a defined result under "same"
        m(torch.zeros(1, 16, 1))


def test_vocos_decoder_takes_the_new_sizes_and_names_the_new_class():
    import voicebox_pytorch_amd as vbx

    m = vbx.VocosDecoder(n_fft=1280, hop_length=320)
    assert (m.n_fft, m.hop_length, m.padding) == (1280, 320, "center") and m.head.out.weight.shape == (1282, 512)
    for n_fft in (320, 640):
        assert vbx.VocosDecoder(input_channels=8, dim=64, intermediate_dim=192, num_layers=1, n_fft=n_fft, hop_length=n_fft // 4).n_fft == n_fft
    for bad in (dict(padding="same"), dict(adanorm_num_embeddings=4)):
        with pytest.raises(NotImplementedError, match="VocosEncodecDecoder"):
            vbx.VocosDecoder(**bad)
    # the forward transform keeps refusing them
    with pytest.raises(NotImplementedError, match="power of two"):
        vbx.LogMelCodec(n_fft=1280, win_length=640, hop_length=160)
    with pytest.raises(NotImplementedError, match="power of two"):
        vbx.griffin_lim(torch.zeros(1, 641, 9), n_fft=1280, win_length=1280, hop_length=320)


def test_from_vocos_checkpoint_padding_same(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = sr.random_state(32, 64, 192, 2, 1280, seed=1, codebooks=5)
    assert sd["head.out.weight"].shape[0] == 1282
    path = str(tmp_path / "vocos_encodec.pt")
    torch.save(sd, path)
    codec = vbx.EncodecVocoCodec.from_vocos_checkpoint(path, padding="same", codebook_size=16)
    voc = codec.vocoder
    assert type(voc) is vbx.VocosEncodecDecoder and (voc.n_fft, voc.hop_length, voc.padding, voc.bandwidth_id) == (1280, 320, "same", 2)
    assert codec.downsample_factor == 320 and codec.latent_dim == 32 and codec.rvq.num_quantizers == 5 and not codec.training
    assert torch.equal(voc.backbone.norm.shift.weight.detach(), sd["backbone.norm.shift.weight"])
    assert codec.rvq.num_quantizers == min(8, 5)
    center = vbx.EncodecVocoCodec.from_vocos_checkpoint(path, codebook_size=16)  # the default: folded to one id
    assert type(center.vocoder) is vbx.VocosDecoder
    assert torch.equal(center.vocoder.backbone.norm.bias.detach(), sd["backbone.norm.shift.weight"][2])
    with pytest.raises(ValueError, match="padding"):
        vbx.EncodecVocoCodec.from_vocos_checkpoint(path, padding="reflect", codebook_size=16)


# ----------------------------------------------------------------------------- the bounds against the planted faults
def test_bounds_are_far_below_every_fault():
    """fp64 only.  The whole-decoder bound (BOUND_A, max |difference| / RMS) against the wrong decoders, and the per-sample bound
    of the stand-alone inverse STFT against the wrong trims, the wrong envelope and the conjugated radix-5 twiddle."""
    for name, cfg, B, frames, ids in WHOLE:
        sd, x = whole_inputs(cfg, B, frames, SEEDS[0])
        kw = dict(n_fft=cfg["n_fft"], hop=cfg["hop_length"], bandwidth_id=ids[0])
        exact = sr.decode(sd, x, **kw)
        for fault in [("trim_off_by_one",), ("center_trim",), ("env_untrimmed",), ("id_swapped",), ("shift_dropped",)]:
            moved = vr.wave_err(sr.decode(sd, x, fault=fault, **kw), exact)
            assert BOUND_A <= 0.1 * moved, (name, fault, moved)
    n_fft, hop, frames = 320, 80, 5
    mag, ph, spec = random_spectrum(2, n_fft, frames, seed=0)
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    ref = sr.istft_same(spec, n_fft, hop, window)
    worst = float(istft_bound(spec, n_fft, hop, window, "same").max())
    for fault in [("trim_off_by_one",), ("center_trim",), ("env_untrimmed",)]:
        moved = float((sr.istft_same(spec, n_fft, hop, window, fault=fault) - ref).abs().max())
        assert 10.0 * worst <= moved, (fault, moved, worst)
    bad = sr.istft_same(spec, n_fft, hop, window, inverse=lambda z: sr.mixed_radix_inverse(z, fault=("r5_twiddle_conj",))[0])
    good = sr.istft_same(spec, n_fft, hop, window, inverse=lambda z: sr.mixed_radix_inverse(z)[0])
    assert float((good - ref).abs().max()) < 1e-12
    assert 10.0 * worst <= float((bad - ref).abs().max())


def test_rounding_noise_stays_below_half_the_bound():
    """tests/test_vocos_gpu.py's docstring: BOUND_A is worth asserting only where the position of the fp16 rounding boundaries does
    not by itself move the wave that far.  Relative noise of 2e-7 in front of each rounding of the emulated-precision restatement
    moves its own wave by less than BOUND_A / 2 on the shapes, seeds and ids of the GPU test (whose SEEDS were picked by this check)."""
    for name, cfg, B, frames, ids in WHOLE:
        for seed in SEEDS:
            sd, x = whole_inputs(cfg, B, frames, seed)
            for i in ids:
                kw = dict(n_fft=cfg["n_fft"], hop=cfg["hop_length"], bandwidth_id=i, emulate=True)
                moved = vr.wave_err(sr.decode(sd, x, noise=(2e-7, 99), **kw), sr.decode(sd, x, **kw))
                print(f"rounding noise {name} seed {seed} id {i}: {moved:.3e} (BOUND_A / 2 = {BOUND_A / 2:.3e})")
                assert moved < BOUND_A / 2, (name, seed, i, moved)
