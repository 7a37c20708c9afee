"""Host side of VocosDecoder (state dict, argument checks) and checks of tests/vocos_ref.py itself, the yardstick of
tests/test_vocos_gpu.py: its two formulations of the inverse STFT against each other and the gamma fold against the unfolded form."""
import pytest
import torch

import vocos_ref as vr


def expected_shapes(C, dim, inter, layers, n_fft):
    s = {"backbone.embed.weight": (dim, C, 7), "backbone.embed.bias": (dim,), "head.out.weight": (n_fft + 2, dim),
         "head.out.bias": (n_fft + 2,), "head.istft.window": (n_fft,)}
    for name in ["backbone.norm", "backbone.final_layer_norm"] + [f"backbone.convnext.{i}.norm" for i in range(layers)]:
        s[name + ".weight"] = s[name + ".bias"] = (dim,)
    for i in range(layers):
        p = f"backbone.convnext.{i}."
        s.update({p + "dwconv.weight": (dim, 1, 7), p + "dwconv.bias": (dim,), p + "pwconv1.weight": (inter, dim),
                  p + "pwconv1.bias": (inter,), p + "pwconv2.weight": (dim, inter), p + "pwconv2.bias": (dim,), p + "gamma": (dim,)})
    return s


@pytest.mark.parametrize("layers", [1, 3])
def test_state_dict_names_and_shapes(layers):
    import voicebox_pytorch_amd as vbx

    m = vbx.VocosDecoder(input_channels=8, dim=64, intermediate_dim=192, num_layers=layers, n_fft=256, hop_length=64)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == expected_shapes(8, 64, 192, layers, 256)
    assert torch.equal(m.head.istft.window, torch.hann_window(256, periodic=True))
    blk = m.backbone.convnext[0]
    assert float(blk.gamma[0].detach()) == pytest.approx(1.0 / layers) and float(blk.pwconv1.bias.detach().abs().max()) == 0.0
    assert 0.015 < float(blk.pwconv1.weight.detach().std()) < 0.025 and float(blk.pwconv1.weight.detach().abs().max()) <= 2.0
    assert float(vbx.VocosDecoder(dim=64, intermediate_dim=64, num_layers=2, layer_scale_init_value=0.25).backbone.convnext[1].gamma[3].detach()) == 0.25


def test_vocos_state_dict_loads_strictly(tmp_path):
    import voicebox_pytorch_amd as vbx

    sd = vr.random_state(8, 64, 192, 2, 256, seed=0)
    full = dict(sd)
    full["feature_extractor.mel_spec.spectrogram.window"] = torch.hann_window(1024)
    full["feature_extractor.mel_spec.mel_scale.fb"] = torch.zeros(513, 100)
    m = vbx.VocosDecoder(input_channels=8, dim=64, intermediate_dim=192, num_layers=2, n_fft=256, hop_length=64)
    m.load_state_dict(full, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    for payload in (full, {"state_dict": full}):
        path = tmp_path / "vocos.pt"
        torch.save(payload, path)
        m2 = vbx.VocosDecoder.from_checkpoint(str(path), hop_length=64)
        assert (m2.input_channels, m2.dim, m2.intermediate_dim, m2.num_layers, m2.n_fft, m2.hop_length) == (8, 64, 192, 2, 256, 64)
        assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items()) and not m2.training


def test_gamma_fold_is_an_identity_in_fp64():
    g = torch.Generator().manual_seed(1)
    gamma, w2, b2 = 0.5 + torch.rand(64, generator=g), torch.randn(64, 192, generator=g), torch.randn(64, generator=g)
    h = torch.randn(10, 192, generator=g, dtype=torch.float64)
    wf, bf = vr.fold_gamma(gamma, w2, b2, emulate=False)
    ref = gamma.double() * (h @ w2.double().t() + b2.double())
    assert float((h @ wf.t() + bf - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("n_fft,hop,frames", [(256, 64, 9), (256, 64, 2), (1024, 256, 12), (512, 200, 7)])
def test_restated_istft_two_ways(n_fft, hop, frames):
    g = torch.Generator().manual_seed(n_fft + frames)
    nb = n_fft // 2 + 1
    spec = torch.complex(torch.randn(2, nb, frames, generator=g, dtype=torch.float64), torch.randn(2, nb, frames, generator=g, dtype=torch.float64))
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    ref = torch.istft(spec, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True)
    got = vr.istft_by_hand(spec, n_fft, hop, window)
    assert got.shape == ref.shape == (2, (frames - 1) * hop)
    assert float((got - ref).abs().max()) < 1e-12


def test_restated_decoder_two_ways():
    sd = vr.random_state(8, 64, 192, 2, 256, seed=3)
    x = torch.randn(2, 8, 9, generator=torch.Generator().manual_seed(4))
    a = vr.decode(sd, x, n_fft=256, hop=64)
    b = vr.decode(sd, x, n_fft=256, hop=64, by_hand=True)
    assert a.shape == (2, 512) and float((a - b).abs().max()) < 1e-10 * float(a.abs().max())
    assert vr.wave_err(vr.decode(sd, x, n_fft=256, hop=64, emulate=True), a) < 0.1  # the roundings are small, and they are there
    assert vr.wave_err(vr.decode(sd, x, n_fft=256, hop=64, emulate=True), a) > 1e-6


def test_im2col_is_the_convolution():
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(2, 5, 4, generator=g, dtype=torch.float64), torch.randn(3, 5, 7, generator=g, dtype=torch.float64)
    cols = vr.im2col(x, 64)
    wp = torch.zeros(3, 64, dtype=torch.float64)
    wp[:, :35] = w.permute(0, 2, 1).reshape(3, 35)
    ref = torch.nn.functional.conv1d(x, w, padding=3).transpose(1, 2).reshape(8, 3)
    assert float((cols @ wp.t() - ref).abs().max()) < 1e-12 and float(cols[:, 35:].abs().max()) == 0.0


def test_not_built_raises():
    import voicebox_pytorch_amd as vbx

    small = dict(input_channels=8, dim=64, intermediate_dim=192, num_layers=1, n_fft=256, hop_length=64)
    for bad in (dict(padding="same"), dict(adanorm_num_embeddings=4), dict(n_fft=384), dict(n_fft=128), dict(n_fft=4096), dict(dim=96),
                dict(dim=2112), dict(intermediate_dim=100), dict(input_channels=513)):
        with pytest.raises(NotImplementedError):
            vbx.VocosDecoder(**{**small, **bad})
    m = vbx.VocosDecoder(**small)
    with pytest.raises(NotImplementedError, match="two frames"):
        m(torch.zeros(1, 8, 1))
    with pytest.raises(ValueError, match="NOLA"):  # a Hann window hopping by its whole length leaves zeros in the envelope
        vbx.VocosDecoder(**{**small, "hop_length": 256})(torch.zeros(1, 8, 4))
    with pytest.raises(NotImplementedError, match="LDS"):
        vbx.VocosDecoder(**{**small, "n_fft": 2048, "hop_length": 2048})(torch.zeros(1, 8, 4))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 9, 4))


def test_cpu_features_raise():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd import _lib

    m = vbx.VocosDecoder(input_channels=8, dim=64, intermediate_dim=192, num_layers=1, n_fft=256, hop_length=64)
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
        m(torch.zeros(1, 8, 4))
    with pytest.raises(_lib.VbxError, match="runs only on an MI355X"):
        m.decode(torch.zeros(1, 8, 4))
