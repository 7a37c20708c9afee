"""The audio codec interface of VoiceBox(audio_enc_dec=...) (voicebox_pytorch.py:484-499) and LogMelCodec, the one encoder of the
reference that has no learned weights (MelVoco.encode, :518-541: STFT -> HTK mel filter bank -> dB), served by one native kernel
(csrc/mel.hip), and its weight-free decode: least-squares inversion of the filter bank, then Griffin-Lim phase recovery on the device
(mel_to_magnitude / griffin_lim, csrc/griffinlim.hip).  Pretrained codec weights (EnCodec, Vocos) are downloads and are not part of this
package; the Vocos decoder NETWORK is (vocos.py: LogMelCodec(vocoder=VocosDecoder.from_checkpoint(path))).  Any nn.Module with the five
members below can be passed as audio_enc_dec, inheritance from AudioEncoderDecoder is not required.

PARITY UNPINNED: torchaudio is not a dependency and no fixture of it exists; LogMelCodec follows the published arithmetic of
torchaudio.transforms.Spectrogram / MelScale / AmplitudeToDB at their defaults (power=2, center=True, pad_mode='reflect',
normalized=False, f_min=0, norm=None, mel_scale='htk', top_db=None), restated in fp64 in tests/mel_ref.py.  The decode side is
UNPINNED likewise: griffin_lim follows the published loop of torchaudio.functional.griffinlim (power=1, length=None), restated with
torch.stft / torch.istft in tests/griffinlim_ref.py; mel_to_magnitude is a least-squares inverse clamped at zero and is NOT
torchaudio's InverseMelScale.  resample / Resample (csrc/resample.hip), the sample-rate conversion in front of a codec, are UNPINNED
too: the published arithmetic of torchaudio.functional.resample, restated in fp64 in tests/resample_ref.py.
"""
import functools
import math

import torch
from torch import nn

from . import _lib
from .masks import take_draw


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


def mel_filter_dense(n_fft, n_mels, sampling_rate, f_max):
    """the same filters as one fp64 matrix [n_fft / 2 + 1, n_mels]"""
    start, length, offset, weights = mel_filter_runs(n_fft, n_mels, sampling_rate, f_max)
    fb = torch.zeros(n_fft // 2 + 1, n_mels, dtype=torch.float64)
    for m in range(n_mels):
        s, n, o = int(start[m]), int(length[m]), int(offset[m])
        fb[s:s + n, m] = weights[o:o + n]
    return fb


def _check_stft_args(n_fft, win_length, hop_length):
    if n_fft & (n_fft - 1) or not 256 <= n_fft <= 2048:
        raise NotImplementedError(f"n_fft must be a power of two in 256 .. 2048 (got {n_fft})")
    if not 0 < win_length <= n_fft or hop_length <= 0:
        raise ValueError("need 0 < win_length <= n_fft, hop_length > 0")


def _stft_tables(n_fft, win_length):
    """fp64: the periodic Hann window of win_length samples centred in n_fft (torch.stft's placement), cos / -sin(2 pi k / n_fft)"""
    win = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    win[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.arange(n_fft // 2, dtype=torch.float64) / n_fft
    return win, ang.cos(), -ang.sin()


def ola_reciprocal_envelope(n_fft, win_length, hop_length, frames, window=None):
    """1 / (window-square envelope) of torch.istft on the kept range [n_fft / 2, n_fft / 2 + (frames - 1) * hop), fp64.  Raises
    ValueError where torch.istft does: an envelope <= 1e-11 anywhere on that range (NOLA).  `window` [n_fft]: a window other than
    the periodic Hann one (VocosDecoder's buffer)."""
    w2 = (_stft_tables(n_fft, win_length)[0] if window is None else window.double()) ** 2
    env = torch.zeros(n_fft + (frames - 1) * hop_length, dtype=torch.float64)
    for f in range(frames):
        env[f * hop_length:f * hop_length + n_fft] += w2
    env = env[n_fft // 2:n_fft // 2 + (frames - 1) * hop_length]
    if env.numel() == 0 or float(env.min()) <= 1e-11:
        raise ValueError(f"window overlap-add envelope is zero somewhere (NOLA): win_length {win_length}, hop_length {hop_length}, "
                         f"n_fft {n_fft}, {frames} frames")
    return 1.0 / env


@functools.lru_cache(maxsize=16)
def _gl_tables(n_fft, win_length, hop_length, frames, device):
    win, tw_re, tw_im = _stft_tables(n_fft, win_length)
    renv = ola_reciprocal_envelope(n_fft, win_length, hop_length, frames)
    return tuple(t.float().to(device) for t in (win, tw_re, tw_im, renv))


def griffin_lim(magnitude, *, n_fft, win_length, hop_length, n_iter=32, momentum=0.99, phase=None):
    """Griffin-Lim with momentum (Perraudin et al. 2013; the loop of torchaudio.functional.griffinlim at power=1, length=None,
    PARITY UNPINNED) on the device: magnitude [B, n_fft / 2 + 1, frames] -> wave fp32 [B, (frames - 1) * hop_length].

        m = momentum / (1 + momentum);  A_0 = exp(i phase);  T_0 = 0
        repeat n_iter times:  R = stft(istft(A_k magnitude));  A = R - m T_k;  A_{k+1} = A / (|A| + 1e-16);  T_{k+1} = R
        wave = istft(A_n magnitude)

    stft / istft as torch's with center=True, pad_mode='reflect', the periodic Hann window of win_length samples, onesided, not
    normalized.  `phase` [B, n_fft / 2 + 1, frames] in radians is the initial phase; None takes the `gl_phase` draw of rng_override
    or, without one, draws it uniformly in [-pi, pi) on the device.  Two launches per iteration, no host synchronisation."""
    _check_stft_args(n_fft, win_length, hop_length)
    if magnitude.ndim != 3 or magnitude.shape[1] != n_fft // 2 + 1:
        raise ValueError(f"griffin_lim takes magnitudes (batch, n_fft / 2 + 1 = {n_fft // 2 + 1}, frames), got {tuple(magnitude.shape)}")
    if n_iter < 0 or not 0 <= momentum < 1:
        raise ValueError("need n_iter >= 0 and 0 <= momentum < 1")
    B, nb, frames = magnitude.shape
    L = (frames - 1) * hop_length
    if L <= n_fft // 2:
        raise RuntimeError(f"reflect padding of n_fft // 2 = {n_fft // 2} samples in the analysis step needs (frames - 1) * hop_length "
                           f"= {L} to be larger")
    if magnitude.device.type != "cuda":
        raise _lib.VbxError(f"griffin_lim runs only on an MI355X (gfx950) through libvbx_hip.so; the magnitude is on '{magnitude.device}'")
    window, tw_re, tw_im, renv = _gl_tables(n_fft, win_length, hop_length, frames, magnitude.device)  # ValueError: NOLA
    if _lib.lib().vbx_griffinlim_lds_bytes(n_fft, win_length, hop_length) > 65536:
        raise NotImplementedError(f"3 * hop_length + win_length = {3 * hop_length + win_length} samples do not fit the LDS beside a "
                                  f"{n_fft}-point transform")
    dev = magnitude.device
    mag = magnitude.detach().to(torch.float32).transpose(1, 2).contiguous()  # frame-major [B, frames, bins]
    if phase is None:
        phase = take_draw("gl_phase")
    if phase is None:
        phase = (2.0 * torch.rand(B, nb, frames, device=dev) - 1.0) * math.pi
    if tuple(phase.shape) != (B, nb, frames):
        raise ValueError(f"phase must have the shape of magnitude {(B, nb, frames)}, got {tuple(phase.shape)}")
    ph = phase.detach().to(dev).transpose(1, 2).double()
    spec_a = torch.stack((ph.cos(), ph.sin()), dim=-1).float().contiguous()  # A_0, rounded once from fp64
    spec_b = torch.empty_like(spec_a)
    fb = torch.empty(B, frames, win_length, dtype=torch.float32, device=dev)
    wave = torch.empty(B, L, dtype=torch.float32, device=dev)
    _lib.call("vbx_griffinlim", mag, spec_a, spec_b, fb, wave, window, tw_re, tw_im, renv, B, frames, n_fft, win_length, hop_length,
              int(n_iter), float(momentum / (1.0 + momentum)), _lib.current_stream())
    return wave


RESAMPLE_METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")
RESAMPLE_KAISER_BETA = 14.769656459379492
RESAMPLE_BANK_BYTES = 16 << 20  # a dense fp32 bank above this raises (near-coprime rates)


def _check_resample_args(orig_freq, new_freq, lowpass_filter_width, resampling_method):
    """the argument checks of torchaudio.functional.resample; returns the rate pair reduced by its gcd"""
    if not (int(orig_freq) == orig_freq and int(new_freq) == new_freq):
        raise ValueError(f"frequencies must be integral (got orig_freq {orig_freq}, new_freq {new_freq}): round them, or scale both "
                         "by a common factor")
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError(f"need orig_freq > 0 and new_freq > 0 (got {orig_freq}, {new_freq})")
    if lowpass_filter_width <= 0:
        raise ValueError(f"need lowpass_filter_width > 0 (got {lowpass_filter_width})")
    if resampling_method not in RESAMPLE_METHODS:
        raise ValueError(f"resampling_method must be one of {RESAMPLE_METHODS} (got {resampling_method!r})")
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def resample_bank(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """The polyphase windowed-sinc filter bank of torchaudio.functional.resample (PARITY UNPINNED: its published arithmetic) for
    the gcd-reduced pair orig : new, built in fp64 and rounded once to fp32:

        base = min(orig, new) * rolloff;  width = ceil(lowpass_filter_width * orig / base);  K = 2 * width + orig
        t = clamp(((k - width) / orig - p / new) * base, +-lowpass_filter_width)
        h[p][k] = sinc(pi t) * window(t) * base / orig,  window = cos^2(pi t / (2 lpw))  or  i0(beta sqrt(1 - (t / lpw)^2)) / i0(beta)

    Returns (h float32 [new, K], width, start int32 [new], length int32 [new]): [start[p], start[p] + length[p]) is the run that
    holds every tap of phase p that is not exactly 0.0 in fp32 (with the Hann window everything past the clamp; a Kaiser row has no
    zeros).  Raises NotImplementedError for a bank above 16 MiB."""
    orig, new = _check_resample_args(orig_freq, new_freq, lowpass_filter_width, resampling_method)
    lpw = float(lowpass_filter_width)
    base = min(orig, new) * float(rolloff)
    width = int(math.ceil(lpw * orig / base))
    K = 2 * width + orig
    if new * K * 4 > RESAMPLE_BANK_BYTES:
        raise NotImplementedError(f"the filter bank of {orig_freq} -> {new_freq} ({new} phases x {K} taps, {new * K * 4 / 2 ** 20:.1f} MiB) "
                                  f"is above {RESAMPLE_BANK_BYTES >> 20} MiB: near-coprime rates are not served")
    k = torch.arange(-width, width + orig, dtype=torch.float64)[None, :] / orig
    p = torch.arange(new, dtype=torch.float64)[:, None] / new
    t = ((k - p) * base).clamp_(-lpw, lpw)
    if resampling_method == "sinc_interp_hann":
        window = torch.cos(t * (math.pi / (2.0 * lpw))) ** 2
    else:
        b = torch.tensor(RESAMPLE_KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
        window = torch.special.i0(b * torch.sqrt(1.0 - (t / lpw) ** 2)) / torch.special.i0(b)
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t)
    h = (sinc * window * (base / orig)).float()
    nz = h != 0
    has = nz.any(dim=1)
    first = torch.where(has, nz.int().argmax(dim=1), torch.zeros(new, dtype=torch.int64))
    last = torch.where(has, K - 1 - nz.flip(1).int().argmax(dim=1), first - 1)
    return h, width, first.int(), (last - first + 1).int()


_resample_tables_cache = {}  # (orig, new, lpw, rolloff, method, beta, device) -> device tables, least recently used first


def _resample_tables(orig, new, lpw, rolloff, method, beta, device):
    """the bank as vbx_resample takes it: run-major taps [run_max, new] (taps[i][p] = h[p][start[p] + i]), start, length, width, K"""
    key = (orig, new, float(lpw), float(rolloff), method, None if beta is None else float(beta), str(device))
    hit = _resample_tables_cache.pop(key, None)
    if hit is None:
        h, width, start, length = resample_bank(orig, new, lpw, rolloff, method, beta)
        K = h.shape[1]
        if K > _lib.lib().vbx_resample_max_taps():
            raise NotImplementedError(f"a filter of {K} taps ({orig} -> {new}, lowpass_filter_width {lpw}) does not fit the LDS "
                                      f"(at most {_lib.lib().vbx_resample_max_taps()})")
        run_max = max(int(length.max()), 1)
        idx = (start.long()[None, :] + torch.arange(run_max)[:, None]).clamp_(max=K - 1)  # [run_max, new]
        taps = h.t().gather(0, idx) * (torch.arange(run_max)[:, None] < length[None, :])
        hit = (taps.contiguous().to(device), start.to(device), length.to(device), width, K, run_max)
        if len(_resample_tables_cache) >= 8:
            _resample_tables_cache.pop(next(iter(_resample_tables_cache)))
    _resample_tables_cache[key] = hit
    return hit


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """torchaudio.functional.resample on the device (csrc/resample.hip, one launch): waveform [..., L] at orig_freq -> [...,
    ceil(new L / orig)] at new_freq (orig : new reduced by their gcd), bandlimited interpolation with the filter bank of
    resample_bank.  PARITY UNPINNED: torchaudio is not a dependency and no vector of it is committed; this follows its published
    arithmetic, restated in fp64 in tests/resample_ref.py.

    Leading dimensions are flattened to rows and restored.  Compute is fp32: other floating dtypes are converted on the way in and
    the result is converted back.  Equal rates return `waveform` itself and launch nothing.  Banks are cached per (rates, filter
    arguments, device).  Runs only on the GPU, like griffin_lim; no gradient is taken through it."""
    orig, new = _check_resample_args(orig_freq, new_freq, lowpass_filter_width, resampling_method)
    if orig == new:
        return waveform
    if not waveform.is_floating_point():
        raise TypeError(f"resample takes a floating-point waveform (got {waveform.dtype})")
    if waveform.ndim < 1:
        raise ValueError("resample takes waveforms (..., samples)")
    if waveform.device.type != "cuda":
        raise _lib.VbxError(f"resample runs only on an MI355X (gfx950) through libvbx_hip.so; the waveform is on '{waveform.device}'")
    taps, start, length, width, K, run_max = _resample_tables(orig, new, lowpass_filter_width, rolloff, resampling_method, beta,
                                                              waveform.device)
    lead, L = waveform.shape[:-1], waveform.shape[-1]
    Lout = -(-new * L // orig)
    x = waveform.detach().reshape(-1, L).to(torch.float32).contiguous()
    y = torch.empty(x.shape[0], Lout, dtype=torch.float32, device=x.device)
    if y.numel():
        _lib.call("vbx_resample", x, y, taps, start, length, x.shape[0], L, Lout, orig, new, width, K, run_max, _lib.current_stream())
    return y.reshape(*lead, Lout).to(waveform.dtype)


class Resample(nn.Module):
    """torchaudio.transforms.Resample over resample(): no parameters and no buffers (the banks live in resample's cache), so nothing
    of it appears in a state_dict()."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99,
                 beta=None):
        super().__init__()
        _check_resample_args(orig_freq, new_freq, lowpass_filter_width, resampling_method)
        self.orig_freq, self.new_freq, self.resampling_method = orig_freq, new_freq, resampling_method
        self.lowpass_filter_width, self.rolloff, self.beta = lowpass_filter_width, rolloff, beta

    def forward(self, waveform):
        return resample(waveform, self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method,
                        self.beta)


class LogMelCodec(AudioEncoderDecoder):
    """Constructor of the reference's MelVoco (:501-516) plus `vocoder`: a module mapping mel [B, n_mels, frames] to a wave (Vocos
    is a download), or "griffin_lim": the weight-free decode griffin_lim(mel_to_magnitude(latents)) with griffin_lim_iters
    iterations and griffin_lim_momentum.  Without either decode raises.  encode / decode run on the GPU only (csrc/mel.hip,
    csrc/griffinlim.hip), as everything else in this package."""

    def __init__(self, *, log=True, n_mels=100, sampling_rate=24000, f_max=8000, n_fft=1024, win_length=640, hop_length=160,
                 vocoder=None, griffin_lim_iters=32, griffin_lim_momentum=0.99):
        super().__init__()
        _check_stft_args(n_fft, win_length, hop_length)
        if n_mels <= 0:
            raise ValueError("need n_mels > 0")
        if isinstance(vocoder, str) and vocoder != "griffin_lim":
            raise ValueError(f'vocoder must be None, "griffin_lim" or a module (got "{vocoder}")')
        if griffin_lim_iters < 0 or not 0 <= griffin_lim_momentum < 1:
            raise ValueError("need griffin_lim_iters >= 0 and 0 <= griffin_lim_momentum < 1")
        self.log, self.n_mels, self.f_max, self.n_fft, self.win_length, self.hop_length = log, n_mels, f_max, n_fft, win_length, hop_length
        self._sampling_rate = sampling_rate
        self.vocoder = vocoder
        self.griffin_lim_iters, self.griffin_lim_momentum = griffin_lim_iters, griffin_lim_momentum
        win, tw_re, tw_im = _stft_tables(n_fft, win_length)
        start, length, offset, weights = mel_filter_runs(n_fft, n_mels, sampling_rate, f_max)
        assert int((start + length).max()) <= n_fft // 2 + 1
        # pinv(fb^T) [n_fft / 2 + 1, n_mels], taken once in fp64; stored mel-major so consecutive lanes read consecutive bins
        pinv_t = torch.linalg.pinv(mel_filter_dense(n_fft, n_mels, sampling_rate, f_max).T).T.contiguous()
        for name, t in (("window", win.float()), ("tw_re", tw_re.float()), ("tw_im", tw_im.float()), ("fb_start", start),
                        ("fb_len", length), ("fb_off", offset), ("fb_w", weights.float()), ("mel_pinv_t", pinv_t.float())):
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

    def mel_to_magnitude(self, mel):
        """latents [B, frames, n_mels] (dB if log, else power) -> linear magnitude fp32 [B, n_fft / 2 + 1, frames] (a view of the
        frame-major buffer the kernel writes): sqrt(max(pinv(fb^T) @ P, 0)) per frame, P = 10^(mel / 10) or mel.  PARITY UNPINNED
        (not torchaudio's InverseMelScale): the least-squares inverse of the filter bank, clamped at zero."""
        if mel.ndim != 3 or mel.shape[2] != self.n_mels:
            raise ValueError(f"mel_to_magnitude takes latents (batch, frames, n_mels = {self.n_mels}), got {tuple(mel.shape)}")
        if mel.device.type != "cuda":
            raise _lib.VbxError(f"LogMelCodec.mel_to_magnitude runs only on an MI355X (gfx950) through libvbx_hip.so; the latents are on '{mel.device}'")
        if self.mel_pinv_t.device != mel.device:
            self.to(mel.device)
        mel = mel.detach().to(torch.float32).contiguous()
        B, frames, _ = mel.shape
        nb = self.n_fft // 2 + 1
        mag = torch.empty(B, frames, nb, dtype=torch.float32, device=mel.device)
        _lib.call("vbx_mel_to_mag", mel, mag, self.mel_pinv_t, B, frames, self.n_mels, nb, int(bool(self.log)), _lib.current_stream())
        return mag.transpose(1, 2)

    def decode(self, mel):
        if self.vocoder is None:
            raise NotImplementedError('LogMelCodec.decode needs a vocoder (mel [B, n_mels, frames] -> wave): pass vocoder=, or '
                                      'vocoder="griffin_lim" for the weight-free decode')
        if isinstance(self.vocoder, str):  # "griffin_lim"
            return griffin_lim(self.mel_to_magnitude(mel), n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length,
                               n_iter=self.griffin_lim_iters, momentum=self.griffin_lim_momentum)
        mel = mel.transpose(-1, -2)
        if self.log:
            mel = torch.pow(10.0, 0.05 * mel)  # DB_to_amplitude(ref=1, power=0.5)
        return self.vocoder(mel)
