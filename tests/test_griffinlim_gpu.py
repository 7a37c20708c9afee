"""The vocoder-free decode (csrc/griffinlim.hip: mel -> magnitude, Griffin-Lim with the FFTs in the LDS) against the fp64 restatement
tests/griffinlim_ref.py.  Tolerance, as in tests/test_mel_gpu.py: what the published arithmetic itself loses -- the same restatement
in fp32 on the CPU, computed HERE on the same input -- times 2 (a different summation order).  No absolute constants.  Parity with
torchaudio itself is UNPINNED (tests/griffinlim_ref.py)."""
import pytest
import torch

import griffinlim_ref as gl
import mel_ref

pytestmark = pytest.mark.gpu
dev = "cuda"

DEFAULT = dict(n_fft=1024, win_length=640, hop_length=160, n_mels=100)
OTHERS = [dict(n_fft=256, win_length=160, hop_length=64, n_mels=64), dict(n_fft=512, win_length=400, hop_length=128, n_mels=64),
          dict(n_fft=2048, win_length=1200, hop_length=300, n_mels=64)]
stft_kw = lambda c: dict(n_fft=c["n_fft"], win_length=c["win_length"], hop_length=c["hop_length"])
ids = lambda c: str(c["n_fft"])


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def _magnitude(cfg, batch=3):
    """inverted mel spectrogram of test_signal() (38 % exact zeros), rounded to fp32: the same numbers for every side; an ODD number
    of frames and a batch of 3, so the two-frames-per-transform pairing has a remainder"""
    mag = gl.mel_to_magnitude(mel_ref.log_mel(mel_ref.test_signal(batch=batch), **cfg), **cfg).float().double()
    frames = mag.shape[2] - (1 - mag.shape[2] % 2)
    assert frames % 2 == 1
    return mag[:, :, :frames].contiguous()


def _wave_check(mag, phase, cfg, n_iter, what, yard=None):
    import voicebox_pytorch_amd as vbx

    got = vbx.griffin_lim(mag.float().to(dev), phase=phase.float().to(dev), n_iter=n_iter, **stft_kw(cfg)).cpu()
    ref64 = gl.griffin_lim(mag, phase, n_iter=n_iter, dtype=torch.float64, **stft_kw(cfg)) if yard is None else yard
    ref32 = gl.griffin_lim(mag, phase, n_iter=n_iter, dtype=torch.float32, **stft_kw(cfg))
    assert got.shape == ref64.shape and got.dtype == torch.float32, (got.shape, ref64.shape)
    err, cpu = _rel(got, ref64), _rel(ref32, ref64)
    print(f"griffin_lim {what} n_fft {cfg['n_fft']} B {mag.shape[0]} frames {mag.shape[2]} n_iter {n_iter}: rel L2 kernel {err:.3e} "
          f"fp32-CPU {cpu:.3e} ratio {err / cpu:.2f}")
    assert err <= 2.0 * cpu, (err, cpu)
    return got


def _mel_to_mag_check(cfg, log=True):
    import voicebox_pytorch_amd as vbx

    kw = dict(cfg, log=log)
    mel = mel_ref.log_mel(mel_ref.test_signal(), **kw).float()  # fp32 latents: the same numbers for every side
    codec = vbx.LogMelCodec(**kw).to(dev)
    got = codec.mel_to_magnitude(mel.to(dev))
    ref64 = gl.mel_to_magnitude(mel, dtype=torch.float64, **kw)
    ref32 = gl.mel_to_magnitude(mel, dtype=torch.float32, **kw).double()
    assert got.shape == ref64.shape and got.dtype == torch.float32 and got.device.type == "cuda", (got.shape, ref64.shape)
    got = got.double().cpu()
    err, cpu = float((got ** 2 - ref64 ** 2).abs().max()), float((ref32 ** 2 - ref64 ** 2).abs().max())
    print(f"mel_to_magnitude {kw}: max |power err| kernel {err:.3e} fp32-CPU {cpu:.3e} ratio {err / cpu:.2f}; max power "
          f"{float((ref64 ** 2).max()):.3e}; exact zeros {float((ref64 == 0).double().mean()):.2f}")
    assert err <= 2.0 * cpu, (err, cpu)


def test_mel_to_magnitude_default_and_power_input():
    _mel_to_mag_check(DEFAULT)
    _mel_to_mag_check(DEFAULT, log=False)


@pytest.mark.parametrize("cfg", OTHERS, ids=ids)
def test_mel_to_magnitude_other_fft_sizes(cfg):
    _mel_to_mag_check(cfg)


@pytest.mark.parametrize("n_iter", [0, 1, 2])
def test_griffin_lim_first_iterations_default(n_iter):
    """0 = synthesis + overlap-add alone; 1 = one analysis and normalisation; 2 = the momentum term is live.  The phase is random at
    the DC and Nyquist bins too: a complex-to-real transform ignores their imaginary parts"""
    mag = _magnitude(DEFAULT)
    _wave_check(mag, gl.random_phase(mag.shape, 1), DEFAULT, n_iter, "random phase")


@pytest.mark.parametrize("n_iter", [0, 2])
@pytest.mark.parametrize("cfg", OTHERS, ids=ids)
def test_griffin_lim_first_iterations_other_fft_sizes(cfg, n_iter):
    mag = _magnitude(cfg)
    _wave_check(mag, gl.random_phase(mag.shape, 1), cfg, n_iter, "random phase")


def test_round_trip_from_the_true_spectrum():
    """no torch.istft in the yardstick: magnitude and phase of the fp64 STFT of the signal, n_iter = 0, against the signal"""
    a = mel_ref.test_signal().double()
    s = gl.stft(a, 1024, 640, 160)
    mag, phase = s.abs().float().double(), s.angle().float().double()
    _wave_check(mag, phase, DEFAULT, 0, "true spectrum vs the signal", yard=a)


def test_32_iterations():
    """fp32 rounding is amplified over 32 iterations by an amount that depends on the initial phase, so the bound is taken over a
    distribution: the kernel's distance at seed 1 <= 2 x the maximum fp32-CPU distance over seeds 1-4.  And the loop converges as the
    restatement does: SC after 32 iterations <= half of SC after 0"""
    import voicebox_pytorch_amd as vbx

    mag = _magnitude(DEFAULT, batch=2)
    kw = stft_kw(DEFAULT)
    cpu = []
    for seed in (1, 2, 3, 4):
        ph = gl.random_phase(mag.shape, seed)
        ref64 = gl.griffin_lim(mag, ph, n_iter=32, dtype=torch.float64, **kw)
        cpu.append(_rel(gl.griffin_lim(mag, ph, n_iter=32, dtype=torch.float32, **kw), ref64))
        if seed == 1:
            yard, phase = ref64, ph
    g = lambda n: vbx.griffin_lim(mag.float().to(dev), phase=phase.float().to(dev), n_iter=n, **kw).cpu()
    got0, got = g(0), g(32)
    err = _rel(got, yard)
    sc0, sc, sc64 = (gl.spectral_convergence(w, mag, **kw) for w in (got0, got, yard))
    print(f"griffin_lim n_iter 32 seed 1: rel L2 kernel {err:.3e}; fp32-CPU seeds 1-4 {' '.join(f'{c:.3e}' for c in cpu)}; ratio to "
          f"their maximum {err / max(cpu):.2f}; spectral convergence kernel {sc0:.4f} -> {sc:.4f} (fp64 restatement {sc64:.4f})")
    assert err <= 2.0 * max(cpu), (err, cpu)
    assert sc <= 0.5 * sc0, (sc0, sc)


def test_reruns_are_bit_identical_and_silence_is_zero():
    import voicebox_pytorch_amd as vbx

    kw = stft_kw(DEFAULT)
    mag = _magnitude(DEFAULT).float().to(dev)
    phase = gl.random_phase(mag.shape, 1).float().to(dev)
    a, b = (vbx.griffin_lim(mag, phase=phase, n_iter=8, **kw) for _ in range(2))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    torch.manual_seed(5)
    c = vbx.griffin_lim(mag, n_iter=4, **kw)
    torch.manual_seed(5)
    d = vbx.griffin_lim(mag, n_iter=4, **kw)
    assert torch.equal(c, d) and not torch.equal(c, vbx.griffin_lim(mag, n_iter=4, **kw))
    with vbx.masks.rng_override(gl_phase=phase):
        assert torch.equal(vbx.griffin_lim(mag, n_iter=8, **kw), a)
    z = vbx.griffin_lim(torch.zeros_like(mag), phase=phase, n_iter=4, **kw)
    assert z.shape == (3, 150 * 160) and torch.equal(z, torch.zeros_like(z))  # 0 / (0 + 1e-16): no NaN


def test_voicebox_samples_a_wave_end_to_end():
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    torch.manual_seed(0)
    codec = vbx.LogMelCodec(vocoder="griffin_lim")
    vb = vbx.VoiceBox(dim=64, depth=2, heads=2, audio_enc_dec=codec, condition_on_text=False).to(dev)
    wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb)
    wave = mel_ref.test_signal().to(dev)
    y0 = torch.randn(2, 151, 100, device=dev)
    phase = gl.random_phase((2, 513, 151), 1).float().to(dev)
    with rng_override(y0=y0, gl_phase=phase):
        w = wrapper.sample(cond=wave, steps=3)
    with rng_override(y0=y0, gl_phase=phase):
        lat = wrapper.sample(cond=wave, steps=3, decode_to_audio=False)
        w2 = codec.decode(lat)
    assert w.shape == (2, 24000) and w.dtype == torch.float32 and torch.isfinite(w).all()
    assert lat.shape == (2, 151, 100) and torch.equal(w, w2)
    assert torch.isfinite(wrapper.sample(cond=wave, steps=3)).all()  # and with a phase drawn on the device
    enc = codec.encode(wave)
    assert codec.encode(codec.decode(enc)).shape == enc.shape


def test_argument_checks():
    import voicebox_pytorch_amd as vbx

    kw = stft_kw(DEFAULT)
    codec = vbx.LogMelCodec(vocoder="griffin_lim").to(dev)
    with pytest.raises(vbx._lib.VbxError):
        vbx.griffin_lim(torch.ones(1, 513, 151), **kw)
    with pytest.raises(vbx._lib.VbxError):
        codec.mel_to_magnitude(torch.zeros(1, 151, 100))
    with pytest.raises(RuntimeError, match="reflect"):  # (frames - 1) * hop = 480 <= n_fft / 2
        vbx.griffin_lim(torch.ones(1, 513, 4, device=dev), **kw)
    assert vbx.griffin_lim(torch.ones(1, 513, 5, device=dev), n_iter=1, **kw).shape == (1, 640)
    with pytest.raises(ValueError):  # NOLA: hop > window
        vbx.griffin_lim(torch.ones(1, 129, 100, device=dev), n_fft=256, win_length=160, hop_length=200)
    with pytest.raises(NotImplementedError):
        vbx.griffin_lim(torch.ones(1, 501, 100, device=dev), n_fft=1000, win_length=640, hop_length=160)
    with pytest.raises(ValueError):
        vbx.griffin_lim(torch.ones(1, 513, 151, device=dev), phase=torch.zeros(1, 513, 150, device=dev), **kw)
    with pytest.raises(NotImplementedError):
        vbx.LogMelCodec().to(dev).decode(torch.zeros(1, 151, 100, device=dev))
