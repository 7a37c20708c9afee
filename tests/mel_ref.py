"""fp64 restatement of the log-mel arithmetic LogMelCodec serves (the reference's MelVoco.encode, voicebox_pytorch.py:518-541, at
torchaudio's defaults: power=2, center=True, pad_mode='reflect', normalized=False, f_min=0, norm=None, mel_scale='htk', top_db=None).

PARITY UNPINNED: torchaudio is not installed where these tests run and no vector of it is committed; this follows its published
formulas.  What IS checked: this restatement against a direct O(n^2) DFT (tests/test_codec_cpu.py), and the kernel against it."""
import math

import torch


def mel_filterbank(n_fft, n_mels, sampling_rate, f_max, dtype=torch.float64):
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    all_freqs = torch.linspace(0, sampling_rate // 2, n_fft // 2 + 1, dtype=dtype)
    f_pts = 700.0 * (10.0 ** (torch.linspace(mel(0.0), mel(f_max), n_mels + 2, dtype=dtype) / 2595.0) - 1.0)
    slopes = f_pts[None, :] - all_freqs[:, None]
    f_diff = f_pts[1:] - f_pts[:-1]
    return torch.clamp(torch.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)  # [n_fft/2+1, n_mels]


def power_spectrogram(a, n_fft, hop, win, dtype=torch.float64):
    a = a.to(dtype)
    spec = torch.stft(a, n_fft, hop, win, torch.hann_window(win, dtype=dtype), center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)
    return spec.abs() ** 2  # [B, n_fft/2+1, frames]


def log_mel(a, *, log=True, n_mels=100, sampling_rate=24000, f_max=8000, n_fft=1024, win_length=640, hop_length=160,
            dtype=torch.float64):
    """a [B, T] -> [B, 1 + T // hop, n_mels] in `dtype` (fp64: the yardstick; fp32: what the reference's own arithmetic loses)"""
    spec = power_spectrogram(a, n_fft, hop_length, win_length, dtype)
    out = spec.transpose(-1, -2) @ mel_filterbank(n_fft, n_mels, sampling_rate, f_max, dtype)
    return 10.0 * torch.log10(torch.clamp(out, min=1e-10)) if log else out


def power_spectrogram_direct(a, n_fft, hop, win):
    """the same frames by a direct O(n^2) DFT in fp64 (explicit reflect padding, explicit window placement): no FFT, no torch.stft"""
    a = a.double()
    B, T = a.shape
    pad = n_fft // 2
    left = a[:, 1:pad + 1].flip(-1)
    right = a[:, T - pad - 1:T - 1].flip(-1)
    p = torch.cat((left, a, right), dim=1)
    w = torch.zeros(n_fft, dtype=torch.float64)
    l0 = (n_fft - win) // 2
    n = torch.arange(win, dtype=torch.float64)
    w[l0:l0 + win] = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / win)
    frames = 1 + T // hop
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None]
    j = torch.arange(n_fft, dtype=torch.float64)[None, :]
    ang = 2.0 * math.pi * k * j / n_fft
    c, s = ang.cos(), ang.sin()
    out = torch.empty(B, n_fft // 2 + 1, frames, dtype=torch.float64)
    for f in range(frames):
        x = p[:, f * hop:f * hop + n_fft] * w
        out[:, :, f] = (x @ c.T) ** 2 + (x @ s.T) ** 2
    return out


def test_signal(batch=2, seconds=1.0, sampling_rate=24000, seed=0):
    """0.1 randn + 0.5 sin(2 pi 440 t) + 0.2 sin(2 pi 3000 t (1 + t)): every mel bin well above the 1e-10 clamp"""
    n = int(seconds * sampling_rate)
    t = torch.arange(n, dtype=torch.float64) / sampling_rate
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(batch, n, generator=g, dtype=torch.float64)
    return (0.1 * noise + 0.5 * torch.sin(2 * math.pi * 440 * t) + 0.2 * torch.sin(2 * math.pi * 3000 * t * (1 + t))).float()
