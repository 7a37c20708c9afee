"""HiFiGANMelCodec / mel_spectrogram without a GPU: the fp64 restatement tests/hifigan_mel_ref.py against its independent construction,
the host tables of the package against the restatement, the frame count, Slaney's scale and unit areas, from_config, every refusal
(all raised before any launch), and a planted-fault table that says what the GPU test's tolerance can tell apart.

Measured here (max |delta ln mel| against the fp64 restatement, 2 x 1 s of hifigan_mel_ref.test_signal):
  symmetric Hann, the smallest fault   1.5e-2 .. 8.4e-2          sr // 2 at 22051 Hz   5.8e-3
  every other fault                    >= 1.2                    fp32 restatement      1.3e-6 .. 4.6e-6
"""
import json
import warnings

import pytest
import torch
import torch.nn.functional as F

import hifigan_mel_ref as R

V1 = R.V1
SMALL = dict(n_fft=256, num_mels=20, sr=22050, hop=64, win=256, fmin=0, fmax=None)
# the configurations of the fault table: (config, samples)
TABLE = (
    (V1, 22050),
    (SMALL, 8000),
    (dict(n_fft=2048, num_mels=128, sr=44100, hop=512, win=2048, fmin=0, fmax=8000), 16000),
    (dict(n_fft=1024, num_mels=80, sr=16000, hop=160, win=640, fmin=0, fmax=8000), 8000),
    (dict(n_fft=1024, num_mels=100, sr=24000, hop=256, win=1024, fmin=0, fmax=12000), 12000),
)
ODD_RATE = (dict(V1, sr=22051), 22051)  # sr // 2 != sr / 2


def _pkg(cfg):
    """a restatement config as the package's keywords"""
    return dict(n_fft=cfg["n_fft"], num_mels=cfg["num_mels"], sampling_rate=cfg["sr"], hop_size=cfg["hop"], win_size=cfg["win"],
                fmin=cfg["fmin"], fmax=cfg["fmax"])


@pytest.mark.parametrize("cfg,T", [(SMALL, 583), (SMALL, 97), (dict(SMALL, win=160, hop=63, fmin=80, fmax=9000), 700),
                                   (dict(V1, num_mels=12), 385)])
def test_restatement_equals_independent_construction(cfg, T):
    y = R.test_signal(T, cfg["sr"])
    a, b = R.mel_spectrogram(y, **cfg), R.mel_spectrogram_direct(y, **cfg)
    assert a.shape == b.shape == (2, cfg["num_mels"], R.frames_of(T, cfg["n_fft"], cfg["hop"]))
    assert float((a - b).abs().max()) <= 1e-10, float((a - b).abs().max())


@pytest.mark.parametrize("cfg", [V1, SMALL, dict(V1, fmin=80, num_mels=100, sr=24000, fmax=12000), dict(V1, sr=22051, fmax=None)])
def test_banks_agree(cfg):
    from voicebox_pytorch_amd.codec import _filter_runs, slaney_mel_filterbank

    a = R.filterbank(cfg["n_fft"], cfg["num_mels"], cfg["sr"], cfg["fmin"], cfg["fmax"])
    b = R.filterbank_scalar(cfg["n_fft"], cfg["num_mels"], cfg["sr"], cfg["fmin"], cfg["fmax"])
    pkg = slaney_mel_filterbank(cfg["n_fft"], cfg["num_mels"], cfg["sr"], cfg["fmin"], cfg["fmax"])
    assert float((a - b).abs().max()) <= 1e-14 and float((a - pkg).abs().max()) <= 1e-14
    # the runs the kernel reads hold exactly the bank: nothing non-zero outside a run, every run inside the spectrum
    start, length, offset, weights = _filter_runs(pkg.T)
    dense = torch.zeros_like(pkg)
    for m in range(cfg["num_mels"]):
        s, n, o = int(start[m]), int(length[m]), int(offset[m])
        assert 0 <= s and s + n <= cfg["n_fft"] // 2 + 1
        dense[m, s:s + n] = weights[o:o + n]
    assert torch.equal(dense, pkg)


def test_frame_count():
    from voicebox_pytorch_amd.codec import melspec_frames, melspec_pad

    for n_fft, hop in ((1024, 256), (1024, 255), (256, 64), (2048, 512), (1024, 160), (512, 512), (256, 1)):
        p = melspec_pad(n_fft, hop)
        assert p == int((n_fft - hop) / 2) == R.pad_of(n_fft, hop)
        for T in (p + 1, n_fft, n_fft + 1, 3 * n_fft + 17, 5 * hop, 5 * hop - 1, 5 * hop + 1):
            if T <= p or T + 2 * p < n_fft:
                continue
            frames = R.mel_spectrogram(torch.zeros(1, T), n_fft, 4, 22050, hop, n_fft).shape[-1]
            assert melspec_frames(T, n_fft, hop) == R.frames_of(T, n_fft, hop) == frames == 1 + (T + 2 * p - n_fft) // hop
            if (n_fft - hop) % 2 == 0:
                assert frames == T // hop, (n_fft, hop, T)
    assert R.frames_of(1275, 1024, 255) == 4 != 1275 // 255


def test_slaney_scale():
    from voicebox_pytorch_amd.codec import hz_to_mel_slaney, mel_to_hz_slaney

    for h2m, m2h in ((R.hz_to_mel, R.mel_to_hz), (hz_to_mel_slaney, mel_to_hz_slaney)):
        assert h2m(1000.0) == 15.0 and m2h(15.0) == 1000.0
        assert h2m(0.0) == 0.0 and abs(h2m(200.0) - 3.0) < 1e-15
        assert abs(h2m(6400.0) - 42.0) < 1e-12  # 27 steps of ln(6.4) / 27 above 1 kHz
        for f in (0.0, 80.0, 440.0, 999.9, 1000.0, 1000.1, 8000.0, 11025.0, 22050.0):
            assert abs(m2h(h2m(f)) - f) <= 1e-11 * max(f, 1.0)


@pytest.mark.parametrize("cfg", [V1, SMALL, dict(V1, num_mels=128, n_fft=2048, sr=44100), dict(V1, fmin=80), dict(V1, sr=24000, fmax=12000)])
def test_every_filter_has_unit_area_within_sampling_error(cfg):
    """sum_k w[k] df is the trapezoid rule on a piecewise-linear function with three kinks: each kink costs at most
    df^2 / 8 times its change of slope (h / a, h / a + h / b, h / b for a triangle of height h over a + b)"""
    from voicebox_pytorch_amd.codec import slaney_mel_filterbank

    fb = slaney_mel_filterbank(cfg["n_fft"], cfg["num_mels"], cfg["sr"], cfg["fmin"], cfg["fmax"])
    f = R.mel_points(cfg["num_mels"], cfg["fmin"], cfg["sr"] / 2.0 if cfg["fmax"] is None else cfg["fmax"])
    df = (cfg["sr"] / 2.0) / (cfg["n_fft"] // 2)
    area = fb.sum(dim=1) * df
    h = 2.0 / (f[2:] - f[:-2])
    bound = df * df / 8.0 * 2.0 * (h / (f[1:-1] - f[:-2]) + h / (f[2:] - f[1:-1]))
    assert bool(((area - 1.0).abs() <= bound + 1e-12).all()), float(((area - 1.0).abs() - bound).max())
    assert float(bound[-1]) < 0.01  # and the bound says something where a filter spans many bins


def test_empty_filter_warns():
    from voicebox_pytorch_amd.codec import slaney_mel_filterbank

    with pytest.warns(UserWarning, match="Empty filters"):
        fb = slaney_mel_filterbank(256, 128, 22050, 0, None)
    assert int((fb.max(dim=1).values == 0).sum()) > 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        slaney_mel_filterbank(1024, 80, 22050, 0, 8000)


def test_from_config(tmp_path):
    import voicebox_pytorch_amd as vbx

    v1 = dict(resblock="1", num_gpus=0, batch_size=16, upsample_rates=[8, 8, 2, 2], segment_size=8192, num_mels=80, num_freq=1025,
              n_fft=1024, hop_size=256, win_size=1024, sampling_rate=22050, fmin=0, fmax=8000, fmax_for_loss=None)
    c = vbx.HiFiGANMelCodec.from_config(v1)
    assert (c.num_mels, c.n_fft, c.hop_size, c.win_size, c.sampling_rate, c.fmin, c.fmax) == (80, 1024, 256, 1024, 22050, 0, 8000)
    assert (c.latent_dim, c.downsample_factor, c.vocoder, c.mean, c.std) == (80, 256, None, None, None)
    d = vbx.HiFiGANMelCodec()
    assert (d.num_mels, d.n_fft, d.hop_size, d.win_size, d.sampling_rate, d.fmin, d.fmax) == (80, 1024, 256, 1024, 22050, 0, 8000)
    big = dict(v1, num_mels=100, sampling_rate=24000, fmax=None, fmax_for_loss=12000, activation="snakebeta")
    path = tmp_path / "config.json"
    path.write_text(json.dumps(big))
    assert "null" in path.read_text()
    voc = torch.nn.Identity()
    for src in (big, path, str(path)):
        c = vbx.HiFiGANMelCodec.from_config(src, vocoder=voc, mean=-1.5, std=2.0)
        assert (c.num_mels, c.sampling_rate, c.fmax, c.vocoder, c.mean, c.std) == (100, 24000, 12000.0, voc, -1.5, 2.0)
    with pytest.raises(KeyError):
        vbx.HiFiGANMelCodec.from_config({k: v for k, v in v1.items() if k != "hop_size"})
    with pytest.raises(NotImplementedError):
        vbx.HiFiGANMelCodec.from_config(dict(v1, n_fft=1000))
    assert isinstance(c, vbx.AudioEncoderDecoder) and not list(c.parameters()) and not c.state_dict()


def test_argument_refusals():
    import voicebox_pytorch_amd as vbx

    y = torch.zeros(1, 4096)
    ok = _pkg(V1)
    cases = [(dict(n_fft=1000), NotImplementedError), (dict(n_fft=128, win_size=128, hop_size=32), NotImplementedError),
             (dict(n_fft=4096), NotImplementedError), (dict(win_size=0), ValueError), (dict(win_size=1025), ValueError),
             (dict(hop_size=0), ValueError), (dict(hop_size=1025), ValueError), (dict(num_mels=0), NotImplementedError),
             (dict(num_mels=513), NotImplementedError), (dict(fmin=-1), ValueError), (dict(fmin=8000), ValueError),
             (dict(fmin=9000), ValueError), (dict(fmax=11025.5), ValueError), (dict(fmax=None, fmin=11025), ValueError)]
    for change, exc in cases:
        with pytest.raises(exc):
            vbx.HiFiGANMelCodec(**dict(ok, **change))
        with pytest.raises(exc):
            vbx.mel_spectrogram(y, **dict(ok, **change))
    vbx.HiFiGANMelCodec(**dict(ok, fmax=11025))  # fmax = sr / 2 is served
    with pytest.raises(NotImplementedError):
        vbx.mel_spectrogram(y, center=True, **ok)
    with pytest.raises(NotImplementedError):
        vbx.HiFiGANMelCodec(vocoder="griffin_lim")
    with pytest.raises(ValueError):
        vbx.HiFiGANMelCodec(vocoder="vocos")
    for kw in (dict(mean=0.0), dict(std=1.0), dict(mean=0.0, std=0.0), dict(mean=0.0, std=-1.0), dict(mean=float("nan"), std=1.0)):
        with pytest.raises(ValueError):
            vbx.HiFiGANMelCodec(**kw)


def test_short_and_cpu_waves_raise():
    """a wave no longer than the pad raises RuntimeError as F.pad does, before the device is looked at; a CPU wave raises VbxError"""
    import voicebox_pytorch_amd as vbx

    codec = vbx.HiFiGANMelCodec()
    for T in (1, 384):
        with pytest.raises(RuntimeError):
            F.pad(torch.zeros(1, 1, T), (384, 384), mode="reflect")
        with pytest.raises(RuntimeError) as e:
            codec.encode(torch.zeros(1, T))
        assert not isinstance(e.value, vbx._lib.VbxError)
    F.pad(torch.zeros(1, 1, 385), (384, 384), mode="reflect")
    # hop = n_fft: no pad, and torch.stft refuses a wave shorter than one frame
    with pytest.raises(RuntimeError):
        torch.stft(torch.zeros(1, 255), 256, 256, 256, torch.hann_window(256), center=False, return_complex=True)
    with pytest.raises(RuntimeError) as e:
        vbx.mel_spectrogram(torch.zeros(1, 255), 256, 20, 22050, 256, 256, 0, None)
    assert not isinstance(e.value, vbx._lib.VbxError)
    for call in (lambda: codec.encode(torch.zeros(1, 385)), lambda: codec.encode(torch.zeros(2, 1, 4096)),
                 lambda: vbx.mel_spectrogram(torch.zeros(1, 4096), **_pkg(V1))):
        with pytest.raises(vbx._lib.VbxError):
            call()
    with pytest.raises(ValueError):
        codec.encode(torch.zeros(4096))
    with pytest.raises(ValueError):
        codec.encode(torch.zeros(1, 4096, dtype=torch.int16))


def test_decode_refusals():
    import voicebox_pytorch_amd as vbx

    class Voc(torch.nn.Module):
        def __init__(self, n_mels=80, hop_length=256, input_log=False):
            super().__init__()
            self.n_mels, self.hop_length, self.input_log = n_mels, hop_length, input_log

        def forward(self, mel):
            return mel.sum(dim=1).repeat_interleave(self.hop_length, dim=1)

    lat = torch.randn(2, 5, 80)
    with pytest.raises(NotImplementedError):
        vbx.HiFiGANMelCodec().decode(lat)
    for voc in (Voc(input_log=True), Voc(n_mels=100), Voc(hop_length=300)):
        with pytest.raises(ValueError):
            vbx.HiFiGANMelCodec(vocoder=voc).decode(lat)
    with pytest.raises(ValueError):
        vbx.HiFiGANMelCodec(vocoder=Voc()).decode(lat[..., :79])
    # a module with that call shape and none of the attributes is taken at its word; the normalisation is undone on the way
    plain = vbx.HiFiGANMelCodec(vocoder=lambda mel: mel).decode(lat)
    assert torch.equal(plain, lat.transpose(1, 2))
    normed = vbx.HiFiGANMelCodec(vocoder=Voc(), mean=-2.0, std=0.5).decode(lat)
    assert normed.shape == (2, 5 * 256) and torch.allclose(normed[:, ::256], (lat * 0.5 - 2.0).sum(dim=2))


def test_planted_faults_and_the_gpu_tolerance():
    """How far each planted fault moves ln mel (fp64, measured here) against the GPU test's tolerance, 2 x what the fp32 restatement
    loses on the same input: the tolerance stays under a tenth of the smallest movement, so the GPU test tells each fault apart."""
    table, smallest, tol = [], float("inf"), 0.0
    for cfg, T in TABLE + (ODD_RATE,):
        y = R.test_signal(T, cfg["sr"])
        ref = R.mel_spectrogram(y, **cfg)
        loss32 = float((R.mel_spectrogram(y, dtype=torch.float32, **cfg).double() - ref).abs().max())
        assert float(ref.min()) > -11.0  # nowhere near the clamp at ln 1e-5 = -11.51: nothing to mask out
        row = {}
        for fault in R.FAULTS:
            if (fault == "floor_half_rate") != (cfg["sr"] % 2 == 1):  # sr // 2 = sr / 2 at an even rate; the odd rate is that fault's row
                continue
            out = R.mel_spectrogram(y, fault=fault, **cfg)
            k = min(out.shape[-1], ref.shape[-1])  # the wider pad makes more frames
            row[fault] = float((out[..., :k] - ref[..., :k]).abs().max())
        table.append((cfg, T, loss32, float(ref.min()), float(ref.max()), row))
        smallest, tol = min(smallest, min(row.values())), max(tol, 2.0 * loss32)
    for cfg, T, loss32, lo, hi, row in table:
        print(f"{cfg} T={T}: fp32 restatement {loss32:.2e}, range {lo:.2f} .. {hi:.2f}, faults " +
              ", ".join(f"{k} {v:.2e}" for k, v in row.items()))
    seen = {k for *_, row in table for k in row}
    assert seen == set(R.FAULTS)
    assert tol < smallest / 10.0, (tol, smallest)
