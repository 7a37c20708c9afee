"""Checks of tests/griffinlim_ref.py itself (the yardstick of tests/test_griffinlim_gpu.py) and of the host-side argument checks of
the vocoder-free decode.  No device."""
import pytest
import torch

import griffinlim_ref as gl
import mel_ref

CONFIGS = [dict(n_fft=1024, win_length=640, hop_length=160, n_mels=100), dict(n_fft=256, win_length=160, hop_length=64, n_mels=64),
           dict(n_fft=512, win_length=400, hop_length=128, n_mels=64), dict(n_fft=2048, win_length=1200, hop_length=300, n_mels=64)]
stft_kw = lambda c: dict(n_fft=c["n_fft"], win_length=c["win_length"], hop_length=c["hop_length"])


def _signal(cfg):
    a = mel_ref.test_signal().double()
    return a[:, :(a.shape[1] // cfg["hop_length"]) * cfg["hop_length"]]  # istft returns (frames - 1) * hop samples


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: str(c["n_fft"]))
def test_istft_inverts_stft(cfg):
    """framing, window placement and envelope of the restatement: max error <= 1e-12 in fp64"""
    a = _signal(cfg)
    n, w, h = cfg["n_fft"], cfg["win_length"], cfg["hop_length"]
    back = gl.istft(gl.stft(a, n, w, h), n, w, h)
    err = float((back - a).abs().max())
    print(f"istft(stft(a)) n_fft {n}: max error {err:.2e}")
    assert back.shape == a.shape and err <= 1e-12, err


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: str(c["n_fft"]))
def test_zero_iterations_from_the_true_phase_return_the_signal(cfg):
    a = _signal(cfg)
    s = gl.stft(a, cfg["n_fft"], cfg["win_length"], cfg["hop_length"])
    back = gl.griffin_lim(s.abs(), s.angle(), n_iter=0, **stft_kw(cfg))
    err = float((back - a).abs().max())
    print(f"n_iter = 0 from the true phase, n_fft {cfg['n_fft']}: max error {err:.2e}")
    assert err <= 1e-12, err


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: str(c["n_fft"]))
def test_32_iterations_halve_the_spectral_convergence(cfg):
    """magnitude = the inverted mel spectrogram of test_signal(), random initial phase (seed 1): SC after 32 iterations is at most
    half of SC after 0"""
    a = mel_ref.test_signal()
    mel = mel_ref.log_mel(a, **cfg)
    mag = gl.mel_to_magnitude(mel, **cfg)
    phase = gl.random_phase(mag.shape, 1, round_fp32=False)
    sc0 = gl.spectral_convergence(gl.griffin_lim(mag, phase, n_iter=0, **stft_kw(cfg)), mag, **stft_kw(cfg))
    sc32 = gl.spectral_convergence(gl.griffin_lim(mag, phase, n_iter=32, **stft_kw(cfg)), mag, **stft_kw(cfg))
    print(f"spectral convergence n_fft {cfg['n_fft']}: {sc0:.4f} -> {sc32:.4f}")
    assert sc32 <= 0.5 * sc0, (sc0, sc32)


def test_envelope_table_matches_istft_and_nola_raises():
    from voicebox_pytorch_amd import codec

    renv = codec.ola_reciprocal_envelope(1024, 640, 160, 151)
    assert renv.dtype == torch.float64 and renv.shape == (150 * 160,)
    # istft of a spectrum whose frames are all the unit impulse response of the window: every frame contributes window[j], so the
    # un-normalised overlap-add is sum(window) and istft returns sum(window) / sum(window^2) = (sum_f w) * renv
    frames = torch.ones(1, 513, 151, dtype=torch.complex128)  # irfft -> delta at sample 0 of each frame
    w = torch.zeros(1024, dtype=torch.float64)
    w[192:832] = torch.hann_window(640, dtype=torch.float64)
    num = torch.zeros(1024 + 150 * 160, dtype=torch.float64)
    for f in range(151):
        num[f * 160] += w[0]
    assert torch.allclose(gl.istft(frames, 1024, 640, 160)[0], (num[512:512 + 24000] * renv), atol=1e-12)
    with pytest.raises(ValueError):
        codec.ola_reciprocal_envelope(256, 160, 200, 100)
    with pytest.raises(RuntimeError):  # what torch.istft itself says to the same pair
        gl.istft(torch.ones(1, 129, 100, dtype=torch.complex128), 256, 160, 200)


def test_codec_constructs_on_the_cpu_and_plain_decode_still_raises():
    import voicebox_pytorch_amd as vbx

    codec = vbx.LogMelCodec(vocoder="griffin_lim")
    assert codec.mel_pinv_t.shape == (100, 513) and codec.mel_pinv_t.dtype == torch.float32
    assert "mel_pinv_t" not in codec.state_dict() and len(codec.state_dict()) == 0
    fb = mel_ref.mel_filterbank(1024, 100, 24000, 8000)
    assert torch.equal(vbx.codec.mel_filter_dense(1024, 100, 24000, 8000), fb)
    assert torch.allclose(codec.mel_pinv_t.double().T, torch.linalg.pinv(fb.T), atol=1e-6)
    with pytest.raises(NotImplementedError):
        vbx.LogMelCodec().decode(torch.zeros(1, 151, 100))
    with pytest.raises(ValueError):
        vbx.LogMelCodec(vocoder="vocos")
    with pytest.raises(vbx._lib.VbxError):
        codec.decode(torch.zeros(1, 151, 100))
    with pytest.raises(vbx._lib.VbxError):
        vbx.griffin_lim(torch.zeros(1, 513, 151), n_fft=1024, win_length=640, hop_length=160)
