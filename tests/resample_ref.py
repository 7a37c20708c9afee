"""fp64 restatement of the sample-rate conversion voicebox_pytorch_amd.resample serves: the polyphase windowed-sinc FIR of
torchaudio.functional.resample (sinc_interp_hann / sinc_interp_kaiser), written as a strided F.conv1d over a zero-padded wave.

PARITY UNPINNED: torchaudio is not installed where these tests run and no vector of it is committed; this follows its published
formulas.  What IS checked: this restatement against `resample_direct`, a per-sample evaluation of the same interpolation formula
that builds no bank and runs no convolution (tests/test_resample_cpu.py), against the analytic resampling of a sine, and the kernel
against it."""
import math

import torch
import torch.nn.functional as F

KAISER_BETA = 14.769656459379492


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def _window(t, lpw, method, beta):
    if method == "sinc_interp_hann":
        return torch.cos(t * math.pi / lpw / 2) ** 2
    assert method == "sinc_interp_kaiser", method
    b = torch.tensor(KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
    return torch.special.i0(b * torch.sqrt(1 - (t / lpw) ** 2)) / torch.special.i0(b)


def bank(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """(h float64 [new, K], width) for the reduced pair: K = 2 * width + orig taps per phase"""
    orig, new = reduced(orig_freq, new_freq)
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, :] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp(-lowpass_filter_width, lowpass_filter_width)
    window = _window(t, lowpass_filter_width, resampling_method, beta)
    t = t * math.pi
    h = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
    return h, width


def resample(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None,
             dtype=torch.float64, round_bank=True, return_bound=False):
    """x [..., L] -> [..., ceil(new L / orig)] in `dtype` (fp64: the yardstick; fp32: what the same arithmetic loses on the CPU).
    round_bank: the bank is rounded to fp32 first, as the product's is.  return_bound: also sum_k |h[p][k] x| per output sample."""
    orig, new = reduced(orig_freq, new_freq)
    if orig == new:
        return x
    h, width = bank(orig, new, lowpass_filter_width, rolloff, resampling_method, beta)
    if round_bank:
        h = h.float()
    h = h.to(dtype)
    lead, L = x.shape[:-1], x.shape[-1]
    xp = F.pad(x.reshape(-1, 1, L).to(dtype), (width, width + orig))
    target = -(-new * L // orig)
    y = F.conv1d(xp, h[:, None, :], stride=orig)  # [rows, new, frames]
    y = y.transpose(1, 2).reshape(y.shape[0], -1)[:, :target].reshape(*lead, target)
    if not return_bound:
        return y
    s = F.conv1d(xp.abs(), h.abs()[:, None, :], stride=orig)
    return y, s.transpose(1, 2).reshape(s.shape[0], -1)[:, :target].reshape(*lead, target)


def resample_direct(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """the same output one sample at a time, fp64, no bank and no convolution: output n sits at time n / new (in units of the
    reduced rates); it weighs input sample m by the windowed sinc at ((m - q orig) / orig - p / new) * base, n = q new + p,
    over the K taps m - q orig in [-width, width + orig) that the published kernel spans.  x [L] (one row)."""
    orig, new = reduced(orig_freq, new_freq)
    lpw = lowpass_filter_width
    base = min(orig, new) * rolloff
    width = math.ceil(lpw * orig / base)
    L = x.shape[-1]
    x = x.double()
    out = torch.zeros(-(-new * L // orig), dtype=torch.float64)
    for n in range(out.numel()):
        q, p = divmod(n, new)
        m = torch.arange(q * orig - width, q * orig + width + orig)
        t = (torch.arange(-width, width + orig, dtype=torch.float64) / orig + torch.tensor(-p, dtype=torch.float64) / new) * base
        t = t.clamp(-lpw, lpw)
        w = _window(t, lpw, resampling_method, beta)
        t = t * math.pi
        w = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * w * (base / orig)
        ok = (m >= 0) & (m < L)
        out[n] = (w[ok] * x[m[ok]]).sum()
    return out


def test_signal(batch=2, seconds=1.0, sampling_rate=24000, seed=0):
    """as mel_ref.test_signal at any rate: 0.1 randn + 0.5 sin(2 pi 440 t) + 0.2 sin(2 pi f t (1 + t)), f = 1 / 8 of the rate"""
    n = int(seconds * sampling_rate)
    t = torch.arange(n, dtype=torch.float64) / sampling_rate
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(batch, n, generator=g, dtype=torch.float64)
    f = sampling_rate / 8.0
    return (0.1 * noise + 0.5 * torch.sin(2 * math.pi * 440 * t) + 0.2 * torch.sin(2 * math.pi * f * t * (1 + t))).float()
