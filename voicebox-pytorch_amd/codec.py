"""The audio codec interface of VoiceBox(audio_enc_dec=...) (voicebox_pytorch.py:484-499) and LogMelCodec, the one encoder of the
reference that has no learned weights (MelVoco.encode, :518-541: STFT -> HTK mel filter bank -> dB), served by one native kernel
(csrc/mel.hip).  Pretrained codecs (EnCodec, Vocos) are downloads and are not part of this package: any nn.Module with the five
members below can be passed as audio_enc_dec, inheritance from AudioEncoderDecoder is not required.

PARITY UNPINNED: torchaudio is not a dependency and no fixture of it exists; LogMelCodec follows the published arithmetic of
torchaudio.transforms.Spectrogram / MelScale / AmplitudeToDB at their defaults (power=2, center=True, pad_mode='reflect',
normalized=False, f_min=0, norm=None, mel_scale='htk', top_db=None), restated in fp64 in tests/mel_ref.py.
"""
import math

import torch
from torch import nn

from . import _lib


class AudioEncoderDecoder(nn.Module):
    """Members a codec provides: encode(audio[B, T]) -> latents [B, frames, latent_dim], decode(latents) -> audio, and the
    properties latent_dim, sampling_rate, downsample_factor (samples per frame)."""
    pass


def hz_to_mel_htk(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_filter_runs(n_fft, n_mels, sampling_rate, f_max, f_min=0.0):
    """The triangular HTK filters (torchaudio.functional.melscale_fbanks, norm=None) in fp64, one contiguous run of bins per filter:
    (start int32 [n_mels], length int32 [n_mels], offset int32 [n_mels], weights float64 [sum(length)])."""
    n_freqs = n_fft // 2 + 1
    all_freqs = torch.linspace(0, sampling_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(hz_to_mel_htk(f_min), hz_to_mel_htk(f_max), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    fb = torch.clamp(torch.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)  # [n_freqs, n_mels]
    start, length, offset, weights = [], [], [], []
    for m in range(n_mels):
        nz = torch.nonzero(fb[:, m]).flatten()
        s, n = (int(nz[0]), int(nz[-1]) - int(nz[0]) + 1) if nz.numel() else (0, 0)
        start.append(s)
        length.append(n)
        offset.append(sum(length[:-1]))
        weights.append(fb[s:s + n, m])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    w = torch.cat(weights) if sum(length) else torch.zeros(0, dtype=torch.float64)
    return i32(start), i32(length), i32(offset), torch.cat((w, torch.zeros(1, dtype=torch.float64)))


class LogMelCodec(AudioEncoderDecoder):
    """Constructor of the reference's MelVoco (:501-516) plus `vocoder`: a module mapping mel [B, n_mels, frames] to a wave (Vocos
    is a download; without one decode raises).  encode runs on the GPU only (csrc/mel.hip), as everything else in this package."""

    def __init__(self, *, log=True, n_mels=100, sampling_rate=24000, f_max=8000, n_fft=1024, win_length=640, hop_length=160,
                 vocoder=None):
        super().__init__()
        if n_fft & (n_fft - 1) or not 256 <= n_fft <= 2048:
            raise NotImplementedError(f"n_fft must be a power of two in 256 .. 2048 (got {n_fft})")
        if not 0 < win_length <= n_fft or hop_length <= 0 or n_mels <= 0:
            raise ValueError("need 0 < win_length <= n_fft, hop_length > 0, n_mels > 0")
        self.log, self.n_mels, self.f_max, self.n_fft, self.win_length, self.hop_length = log, n_mels, f_max, n_fft, win_length, hop_length
        self._sampling_rate = sampling_rate
        self.vocoder = vocoder
        win = torch.zeros(n_fft, dtype=torch.float64)
        left = (n_fft - win_length) // 2  # torch.stft centres a short window in n_fft
        win[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
        ang = 2.0 * math.pi * torch.arange(n_fft // 2, dtype=torch.float64) / n_fft
        start, length, offset, weights = mel_filter_runs(n_fft, n_mels, sampling_rate, f_max)
        assert int((start + length).max()) <= n_fft // 2 + 1
        for name, t in (("window", win.float()), ("tw_re", ang.cos().float()), ("tw_im", (-ang.sin()).float()), ("fb_start", start),
                        ("fb_len", length), ("fb_off", offset), ("fb_w", weights.float())):
            self.register_buffer(name, t, persistent=False)

    @property
    def downsample_factor(self):
        return self.hop_length

    @property
    def latent_dim(self):
        return self.n_mels

    @property
    def sampling_rate(self):
        return self._sampling_rate

    def encode(self, audio):
        if audio.ndim == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.ndim != 2:
            raise ValueError(f"encode takes waves (batch, samples), got {tuple(audio.shape)}")
        if audio.shape[1] <= self.n_fft // 2:
            raise RuntimeError(f"reflect padding of n_fft // 2 = {self.n_fft // 2} samples needs a longer wave (got {audio.shape[1]} samples)")
        if audio.device.type != "cuda":
            raise _lib.VbxError(f"LogMelCodec.encode runs only on an MI355X (gfx950) through libvbx_hip.so; the wave is on '{audio.device}'")
        if self.window.device != audio.device:
            self.to(audio.device)
        audio = audio.detach().to(torch.float32).contiguous()
        B, T = audio.shape
        out = torch.empty(B, 1 + T // self.hop_length, self.n_mels, dtype=torch.float32, device=audio.device)
        _lib.call("vbx_logmel", audio, out, self.window, self.tw_re, self.tw_im, self.fb_start, self.fb_len, self.fb_off, self.fb_w,
                  B, T, self.n_fft, self.hop_length, self.n_mels, int(bool(self.log)), _lib.current_stream())
        return out

    def decode(self, mel):
        if self.vocoder is None:
            raise NotImplementedError("LogMelCodec.decode needs a vocoder (mel [B, n_mels, frames] -> wave): pass vocoder=")
        mel = mel.transpose(-1, -2)
        if self.log:
            mel = torch.pow(10.0, 0.05 * mel)  # DB_to_amplitude(ref=1, power=0.5)
        return self.vocoder(mel)
