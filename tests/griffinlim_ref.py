"""Restatement of the vocoder-free decode LogMelCodec serves (csrc/griffinlim.hip) with torch.stft / torch.istft / torch.linalg.pinv.
dtype is a parameter: fp64 is the yardstick, fp32 is what the published arithmetic itself loses.

PARITY UNPINNED: torchaudio is not installed where these tests run.  griffin_lim follows the published loop of
torchaudio.functional.griffinlim (power=1, length=None, rand_init -> `phase`); mel_to_magnitude is the least-squares inverse of the
HTK filter bank clamped at zero, NOT torchaudio's InverseMelScale.  What IS checked: this restatement against itself
(tests/test_griffinlim_cpu.py: istft(stft(a)) = a, convergence), and the kernels against it."""
import torch

import mel_ref


def stft(x, n_fft, win, hop):
    return torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=x.dtype, device=x.device), center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)  # [B, n_fft/2+1, frames]


def istft(spec, n_fft, win, hop):
    return torch.istft(spec, n_fft, hop, win, torch.hann_window(win, dtype=spec.real.dtype, device=spec.device), center=True,
                       normalized=False, onesided=True, length=None)  # [B, (frames-1)*hop]


def mel_to_magnitude(mel, *, log=True, n_mels=100, sampling_rate=24000, f_max=8000, n_fft=1024, dtype=torch.float64, **_):
    """mel [B, frames, n_mels] -> [B, n_fft/2+1, frames]: sqrt(max(pinv(fb^T) @ P, 0))"""
    mel = mel.to(dtype)
    p = 10.0 ** (mel / 10.0) if log else mel
    fb = mel_ref.mel_filterbank(n_fft, n_mels, sampling_rate, f_max, dtype)  # [n_freqs, n_mels]
    lin = torch.linalg.pinv(fb.T) @ p.transpose(-1, -2)
    return torch.clamp(lin, min=0.0).sqrt()


def griffin_lim(magnitude, phase, *, n_fft, win_length, hop_length, n_iter=32, momentum=0.99, dtype=torch.float64):
    magnitude, phase = magnitude.to(dtype), phase.to(dtype)
    m = momentum / (1 + momentum)
    a = torch.polar(torch.ones_like(phase), phase)
    t = torch.zeros_like(a)
    for _ in range(n_iter):
        r = stft(istft(a * magnitude, n_fft, win_length, hop_length), n_fft, win_length, hop_length)
        a = r - m * t
        a = a / (a.abs() + 1e-16)
        t = r
    return istft(a * magnitude, n_fft, win_length, hop_length)


def spectral_convergence(wave, magnitude, *, n_fft, win_length, hop_length):
    """|| |stft(w)| - magnitude || / ||magnitude||, in fp64"""
    s = stft(wave.double(), n_fft, win_length, hop_length).abs()
    return float((s - magnitude.double()).norm() / magnitude.double().norm())


def random_phase(shape, seed, round_fp32=True):
    """(2 rand - 1) pi drawn in fp64; rounded to fp32 (and returned as fp64) so that a kernel, which takes fp32, and both
    restatements start from the same numbers"""
    g = torch.Generator().manual_seed(seed)
    ph = (2.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 1.0) * torch.pi
    return ph.float().double() if round_fp32 else ph
