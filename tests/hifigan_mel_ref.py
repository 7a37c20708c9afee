"""fp64 restatement of the mel front end HiFiGANMelCodec / mel_spectrogram serve: HiFi-GAN's meldataset.mel_spectrogram (BigVGAN ships
the same function) over librosa.filters.mel at its defaults, from the published formulas.

    p = int((n_fft - hop) / 2);  y' = reflect_pad(y, p, p);  frames of n_fft every hop, center=False
    window: periodic Hann of win samples centred in n_fft;  mag = sqrt(re^2 + im^2 + 1e-9)
    mel = fb @ mag, fb = Slaney-scale triangles over linspace(0, sr / 2, n_fft / 2 + 1), each times 2 / (f[m + 2] - f[m])
    out = ln(max(mel, 1e-5))                                              [B, num_mels, frames]

PARITY UNPINNED: neither hifi-gan, BigVGAN nor librosa is installed where these tests run and no vector of them is committed.  What
IS checked: this restatement (torch.stft, a vectorised bank) against an independent construction (a direct O(n^2) DFT over explicitly
sliced frames, a bank built filter by filter from the scalar formulas) in tests/test_hifigan_mel_cpu.py, and the kernel against it.

`dtype=torch.float32` runs the same code in fp32 (the bank built in fp64 and rounded once, as librosa hands it over): what the
arithmetic itself loses, the yardstick of the kernel's tolerance.  `fault=` plants one deviation (FAULTS) so that a test can measure
how far each would move the result."""
import functools
import math

import torch
import torch.nn.functional as F

FAULTS = ("htk_scale", "no_area_norm", "symmetric_hann", "power_for_magnitude", "log10_for_ln", "floor_half_rate", "pad_half_n_fft")

MIN_LOG_HZ = 1000.0  # linear below at 200 / 3 Hz per mel, logarithmic above
MIN_LOG_MEL = 15.0
LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f, htk=False):
    if htk:
        return 2595.0 * math.log10(1.0 + f / 700.0)
    return 3.0 * f / 200.0 if f < MIN_LOG_HZ else MIN_LOG_MEL + math.log(f / MIN_LOG_HZ) / LOGSTEP


def mel_to_hz(m, htk=False):
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return 200.0 * m / 3.0 if m < MIN_LOG_MEL else MIN_LOG_HZ * math.exp(LOGSTEP * (m - MIN_LOG_MEL))


def mel_points(num_mels, fmin, fmax, htk=False):
    """the num_mels + 2 corner frequencies in Hz, fp64"""
    lo, hi = hz_to_mel(float(fmin), htk), hz_to_mel(float(fmax), htk)
    return torch.tensor([mel_to_hz(lo + (hi - lo) * i / (num_mels + 1), htk) for i in range(num_mels + 2)], dtype=torch.float64)


def filterbank(n_fft, num_mels, sr, fmin=0.0, fmax=None, fault=None):
    """fp64 [num_mels, n_fft / 2 + 1]"""
    fmax = sr / 2.0 if fmax is None else fmax
    freqs = torch.linspace(0, (sr // 2) if fault == "floor_half_rate" else sr / 2.0, n_fft // 2 + 1, dtype=torch.float64)
    f = mel_points(num_mels, fmin, fmax, htk=fault == "htk_scale")
    d = f[1:] - f[:-1]
    ramps = f[:, None] - freqs[None, :]
    fb = torch.clamp(torch.minimum(-ramps[:-2] / d[:-1, None], ramps[2:] / d[1:, None]), min=0.0)
    if fault != "no_area_norm":
        fb = fb * (2.0 / (f[2:] - f[:-2]))[:, None]
    return fb


def filterbank_scalar(n_fft, num_mels, sr, fmin=0.0, fmax=None):
    """the same bank, filter by filter and bin by bin from the scalar formulas"""
    fmax = sr / 2.0 if fmax is None else fmax
    nb = n_fft // 2 + 1
    lo, hi = hz_to_mel(float(fmin)), hz_to_mel(float(fmax))
    pts = [mel_to_hz(lo + (hi - lo) * i / (num_mels + 1)) for i in range(num_mels + 2)]
    fb = torch.zeros(num_mels, nb, dtype=torch.float64)
    for m in range(num_mels):
        f0, f1, f2 = pts[m], pts[m + 1], pts[m + 2]
        for k in range(nb):
            fk = (sr / 2.0) * k / (nb - 1)
            if f0 < fk <= f1:
                w = (fk - f0) / (f1 - f0)
            elif f1 < fk < f2:
                w = (f2 - fk) / (f2 - f1)
            else:
                continue
            fb[m, k] = w * 2.0 / (f2 - f0)
    return fb


def pad_of(n_fft, hop):
    return int((n_fft - hop) / 2)


def frames_of(T, n_fft, hop):
    return 1 + (T + 2 * pad_of(n_fft, hop) - n_fft) // hop


def mel_spectrogram(y, n_fft, num_mels, sr, hop, win, fmin=0.0, fmax=None, dtype=torch.float64, fault=None, log=True):
    """y [B, T] -> [B, num_mels, frames] in `dtype`; log=False: the mel magnitudes before the clamp and the logarithm"""
    y = y.to(dtype)
    p = n_fft // 2 if fault == "pad_half_n_fft" else pad_of(n_fft, hop)
    y = F.pad(y.unsqueeze(1), (p, p), mode="reflect").squeeze(1)  # RuntimeError when T <= p
    window = torch.hann_window(win, periodic=fault != "symmetric_hann", dtype=dtype)
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=window, center=False, normalized=False, onesided=True,
                      return_complex=True)
    mag = spec.real ** 2 + spec.imag ** 2 + 1e-9
    if fault != "power_for_magnitude":
        mag = torch.sqrt(mag)
    mel = filterbank(n_fft, num_mels, sr, fmin, fmax, fault).to(dtype) @ mag
    if not log:
        return mel
    mel = torch.clamp(mel, min=1e-5)
    return torch.log10(mel) if fault == "log10_for_ln" else torch.log(mel)


def mel_spectrogram_direct(y, n_fft, num_mels, sr, hop, win, fmin=0.0, fmax=None):
    """the independent construction in fp64: explicit reflection, explicitly sliced frames, explicit window placement, a direct
    O(n^2) DFT, the scalar bank.  No F.pad, no torch.stft, no FFT."""
    y = y.double()
    B, T = y.shape
    p = pad_of(n_fft, hop)
    assert T > p
    padded = torch.cat((y[:, 1:p + 1].flip(-1), y, y[:, T - p - 1:T - 1].flip(-1)), dim=1)
    w = torch.zeros(n_fft, dtype=torch.float64)
    l0 = (n_fft - win) // 2
    w[l0:l0 + win] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(win, dtype=torch.float64) / win)
    frames = 1 + (T + 2 * p - n_fft) // hop
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None]
    j = torch.arange(n_fft, dtype=torch.float64)[None, :]
    ang = 2.0 * math.pi * torch.remainder(k * j, n_fft) / n_fft
    c, s = ang.cos(), ang.sin()
    fb = filterbank_scalar(n_fft, num_mels, sr, fmin, fmax)
    out = torch.empty(B, num_mels, frames, dtype=torch.float64)
    for f in range(frames):
        x = padded[:, f * hop:f * hop + n_fft] * w
        mag = torch.sqrt((x @ c.T) ** 2 + (x @ s.T) ** 2 + 1e-9)
        out[:, :, f] = torch.log(torch.clamp(mag @ fb.T, min=1e-5))
    return out


def test_signal(T, sr, batch=2, seed=0):
    """tests/mel_ref.test_signal at any length and rate: 0.1 randn + 0.5 sin(2 pi 440 t) + 0.2 sin(2 pi 3000 t (1 + t)), fp32 [batch, T]"""
    t = torch.arange(T, dtype=torch.float64) / sr
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(batch, T, generator=g, dtype=torch.float64)
    return (0.1 * noise + 0.5 * torch.sin(2 * math.pi * 440 * t) + 0.2 * torch.sin(2 * math.pi * 3000 * t * (1 + t))).float()


V1 = dict(n_fft=1024, num_mels=80, sr=22050, hop=256, win=1024, fmin=0, fmax=8000)

# the shapes of tests/test_hifigan_mel_gpu.py: (id, config, T, what it reaches); B = 2 throughout
CASES = (
    ("one_frame_reflects_both_sides", V1, 385, "one frame; it reflects on both sides; the minimum T > p = 384"),
    ("four_frames", V1, 1024, "4 frames: one full workgroup"),
    ("tail_dropped", V1, 1279, "4 frames; tail samples dropped"),
    ("five_frames", V1, 1280, "5 frames: one past a 4-frame workgroup"),
    ("one_second", V1, 22050, "86 frames"),
    ("n_fft_256", dict(n_fft=256, num_mels=20, sr=22050, hop=64, win=256, fmin=0, fmax=None), 583, "smallest transform, fmax=None"),
    ("n_fft_2048", dict(n_fft=2048, num_mels=128, sr=44100, hop=512, win=2048, fmin=0, fmax=8000), 2567, "largest transform"),
    ("win_below_n_fft", dict(n_fft=1024, num_mels=80, sr=16000, hop=160, win=640, fmin=0, fmax=8000), 1447, "win < n_fft"),
    ("bigvgan_24k", dict(n_fft=1024, num_mels=100, sr=24000, hop=256, win=1024, fmin=0, fmax=12000), 1287, "BigVGAN's 24 kHz bank"),
    ("odd_n_fft_minus_hop", dict(V1, hop=255), 1275, "n_fft - hop odd; frames != T // hop"),
    ("fmin_80", dict(V1, fmin=80), 1287, "non-zero fmin"),
)


@functools.lru_cache(maxsize=None)
def case(name):
    """(config, wave fp32 [2, T], fp64 restatement, fp32 restatement) of one of CASES, computed once; treat as read-only"""
    _, cfg, T, _ = next(c for c in CASES if c[0] == name)
    y = test_signal(T, cfg["sr"])
    return cfg, y, mel_spectrogram(y, dtype=torch.float64, **cfg), mel_spectrogram(y, dtype=torch.float32, **cfg)
