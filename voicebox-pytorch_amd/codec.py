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

ResidualVQ / EncodecVocoCodec (csrc/rvq.hip) are the reference's EncodecVoco (:551-592) around a residual vector quantizer on the device:
codes in and out, latents from codes, features for a VocosDecoder.  EnCodec's SEANet encoder is seanet.py's SEANetEncoder, passed as
encoder= (from_encodec_checkpoint builds both from one local file); parity with encodec / vocos / vector_quantize_pytorch is UNPINNED likewise (tests/rvq_ref.py restates the arithmetic).

HiFiGANMelCodec / mel_spectrogram (csrc/mel.hip, vbx_melspec) are the mel front end HiFi-GAN and BigVGAN were trained on -- Slaney
filters, magnitude, ln(clamp(., 1e-5)), center=False framing -- and the codec published weights of those generators want (the
Voicebox paper's own: 80-bin log mels decoded by HiFi-GAN).  Parity with HiFi-GAN / BigVGAN / librosa is UNPINNED likewise
(tests/hifigan_mel_ref.py restates the arithmetic in fp64).
"""
import functools
import math

import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights, read_checkpoint, tensors_key
from ._wnconv import read_config
from .masks import take_draw
from .wave_lens import device_lens, map_lens, resample_lens, zero_dead_frames  # noqa: F401  (resample_lens: part of this module's API)


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
    return _filter_runs(fb)


def _filter_runs(fb):
    """a dense bank fp64 [n_freqs, n_mels] as the runs vbx_logmel / vbx_melspec read: per filter the bins from its first to its last
    non-zero weight (an all-zero filter is a run of length 0); one zero weight is appended so the table is never empty"""
    n_mels = fb.shape[1]
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


def _check_istft_args(n_fft, win_length, hop_length):
    """what the inverse-only entries (vbx_istft, vbx_istft_trim) serve: the sizes above and 5 * 2^m = 320, 640, 1280"""
    if n_fft not in (320, 640, 1280) and (n_fft & (n_fft - 1) or not 256 <= n_fft <= 2048):
        raise NotImplementedError(f"n_fft must be a power of two in 256 .. 2048 or one of 320, 640, 1280 (got {n_fft})")
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


def ola_reciprocal_envelope_trim(n_fft, hop_length, frames, window, trim, out_len):
    """1 / (window-square envelope) on [trim, trim + out_len) of the (frames - 1) * hop + n_fft overlap-added samples, fp64: Vocos's
    ISTFT at padding="same" keeps trim = (win_length - hop) // 2 from each end.  `window` [n_fft].  Raises ValueError where Vocos
    asserts: an envelope <= 1e-11 on the kept range (NOLA)."""
    w2 = window.double() ** 2
    env = torch.zeros(n_fft + (frames - 1) * hop_length, dtype=torch.float64)
    for f in range(frames):
        env[f * hop_length:f * hop_length + n_fft] += w2
    if trim < 0 or out_len < 1 or trim + out_len > env.numel():
        raise ValueError(f"the kept range [{trim}, {trim + out_len}) is not inside the {env.numel()} overlap-added samples")
    env = env[trim:trim + out_len]
    if float(env.min()) <= 1e-11:
        raise ValueError(f"window overlap-add envelope is zero somewhere on the kept range (NOLA): hop_length {hop_length}, n_fft {n_fft}, "
                         f"{frames} frames, {trim} samples trimmed")
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


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None,
             lens=None):
    """torchaudio.functional.resample on the device (csrc/resample.hip, one launch): waveform [..., L] at orig_freq -> [...,
    ceil(new L / orig)] at new_freq (orig : new reduced by their gcd), bandlimited interpolation with the filter bank of
    resample_bank.  PARITY UNPINNED: torchaudio is not a dependency and no vector of it is committed; this follows its published
    arithmetic, restated in fp64 in tests/resample_ref.py.

    Leading dimensions are flattened to rows and restored.  Compute is fp32: other floating dtypes are converted on the way in and
    the result is converted back.  Equal rates return `waveform` itself and launch nothing.  Banks are cached per (rates, filter
    arguments, device).  Runs only on the GPU, like griffin_lim; no gradient is taken through it.

    lens (not a torchaudio keyword): per-row sample counts of a padded batch [B, L] or [B, 1, L], 1 <= len_b <= L (a list or CPU
    tensor is validated, a device tensor clamped) -- row b is resampled as the row alone: zeros from len_b on instead of whatever
    the padding holds, bit-equal to resample(waveform[b:b+1, :len_b]) up to resample_lens(lens, orig_freq, new_freq)[b] and exactly
    0.0 past it (vbx_resample_lens)."""
    orig, new = _check_resample_args(orig_freq, new_freq, lowpass_filter_width, resampling_method)
    if lens is not None:
        if waveform.ndim not in (2, 3) or (waveform.ndim == 3 and waveform.shape[1] != 1):
            raise ValueError(f"resample(lens=) takes a padded batch (batch, samples) or (batch, 1, samples), got {tuple(waveform.shape)}")
        if waveform.shape[-1] < 1:
            raise ValueError("resample(lens=): empty waveform")
        lens = device_lens(lens, waveform.shape[0], waveform.shape[-1], 1, waveform.device, "resample")
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
    if y.numel() and lens is not None:
        _lib.call("vbx_resample_lens", x, lens, y, taps, start, length, x.shape[0], L, Lout, orig, new, width, K, run_max,
                  _lib.current_stream())
    elif y.numel():
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

    def forward(self, waveform, lens=None):
        return resample(waveform, self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method,
                        self.beta, lens=lens)


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

    def frame_lens(self, sample_lens):
        """frames of a row of that many samples, 1 + l // hop_length: a list, a CPU tensor or a device tensor; the same kind back"""
        return map_lens(sample_lens, lambda l: 1 + l // self.hop_length)

    def encode(self, audio, lens=None):
        """lens: per-row sample counts of a padded batch, n_fft // 2 < len_b <= T (a list or CPU tensor is validated, a device tensor
        clamped): row b is the row alone -- bit-equal to encode(audio[b:b+1, :len_b])[0] up to frame_lens(lens)[b], 0.0 past it."""
        if audio.ndim == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.ndim != 2:
            raise ValueError(f"encode takes waves (batch, samples), got {tuple(audio.shape)}")
        if audio.shape[1] <= self.n_fft // 2:
            raise RuntimeError(f"reflect padding of n_fft // 2 = {self.n_fft // 2} samples needs a longer wave (got {audio.shape[1]} samples)")
        if lens is not None:  # checked (host values) or clamped (a device tensor) before anything else
            lens = device_lens(lens, audio.shape[0], audio.shape[1], self.n_fft // 2 + 1, audio.device, "LogMelCodec.encode")
        if audio.device.type != "cuda":
            raise _lib.VbxError(f"LogMelCodec.encode runs only on an MI355X (gfx950) through libvbx_hip.so; the wave is on '{audio.device}'")
        if self.window.device != audio.device:
            self.to(audio.device)
        audio = audio.detach().to(torch.float32).contiguous()
        B, T = audio.shape
        out = torch.empty(B, 1 + T // self.hop_length, self.n_mels, dtype=torch.float32, device=audio.device)
        if lens is not None:
            _lib.call("vbx_logmel_lens", audio, lens, out, self.window, self.tw_re, self.tw_im, self.fb_start, self.fb_len, self.fb_off,
                      self.fb_w, B, T, self.n_fft, self.hop_length, self.n_mels, int(bool(self.log)), _lib.current_stream())
            return out
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


def hz_to_mel_slaney(f):
    """Slaney's mel scale (the Auditory Toolbox; librosa's default, htk=False): linear below 1 kHz at 200 / 3 Hz per mel,
    logarithmic above with step ln(6.4) / 27, so 1000 Hz = 15 mel"""
    return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + math.log(f / 1000.0) * (27.0 / math.log(6.4))


def mel_to_hz_slaney(m):
    return 200.0 * m / 3.0 if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def slaney_mel_filterbank(n_fft, num_mels, sampling_rate, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) at its defaults (htk=False, norm='slaney'), restated from the published
    formulas (PARITY UNPINNED: librosa is not a dependency): fp64 [num_mels, n_fft / 2 + 1].  Triangles between the num_mels + 2
    points equally spaced on Slaney's mel scale from fmin to fmax (None: sampling_rate / 2), over the bin frequencies
    linspace(0, sampling_rate / 2, n_fft / 2 + 1) -- the float sampling_rate / 2 --, filter m times 2 / (f[m + 2] - f[m]) (unit area).
    An all-zero filter warns, as librosa does."""
    fmax = sampling_rate / 2.0 if fmax is None else float(fmax)
    freqs = torch.linspace(0, sampling_rate / 2.0, n_fft // 2 + 1, dtype=torch.float64)
    lo, hi = hz_to_mel_slaney(float(fmin)), hz_to_mel_slaney(fmax)
    mels = torch.linspace(lo, hi, num_mels + 2, dtype=torch.float64)
    f_pts = torch.where(mels < 15.0, 200.0 * mels / 3.0, 1000.0 * torch.exp((math.log(6.4) / 27.0) * (mels - 15.0)))
    f_diff = f_pts[1:] - f_pts[:-1]
    ramps = f_pts[:, None] - freqs[None, :]
    fb = torch.clamp(torch.minimum(-ramps[:-2] / f_diff[:-1, None], ramps[2:] / f_diff[1:, None]), min=0.0)
    fb = fb * (2.0 / (f_pts[2:] - f_pts[:-2]))[:, None]
    if not bool((fb.max(dim=1).values > 0).all()):
        import warnings

        warnings.warn("Empty filters detected in mel frequency basis. Some channels will produce empty responses. Try increasing "
                      "your sampling rate (and fmax) or reducing n_mels.", stacklevel=2)
    return fb


def melspec_pad(n_fft, hop_size):
    """the reflect pad of HiFi-GAN's mel_spectrogram on each side: int((n_fft - hop_size) / 2)"""
    return int((n_fft - hop_size) / 2)


def melspec_frames(samples, n_fft, hop_size):
    """frames of `samples` samples at center=False over that pad: samples // hop_size when n_fft - hop_size is even"""
    return 1 + (samples + 2 * melspec_pad(n_fft, hop_size) - n_fft) // hop_size


def _check_melspec_args(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """what vbx_melspec serves; returns fmax with None resolved to sampling_rate / 2"""
    if center:
        raise NotImplementedError("center=True is not built: HiFi-GAN / BigVGAN frame with center=False over a hop-aligned reflect pad "
                                  "(LogMelCodec is the centred front end)")
    if int(n_fft) != n_fft or n_fft & (n_fft - 1) or not 256 <= n_fft <= 2048:
        raise NotImplementedError(f"n_fft must be a power of two in 256 .. 2048 (got {n_fft})")
    if not 0 < win_size <= n_fft or not 0 < hop_size <= n_fft:
        raise ValueError(f"need 0 < win_size <= n_fft and 0 < hop_size <= n_fft (got win_size {win_size}, hop_size {hop_size}, n_fft {n_fft})")
    if not 1 <= num_mels <= 512:
        raise NotImplementedError(f"num_mels must be in 1 .. 512 (got {num_mels})")
    if sampling_rate <= 0:
        raise ValueError(f"need sampling_rate > 0 (got {sampling_rate})")
    fmax = sampling_rate / 2.0 if fmax is None else fmax
    if not 0 <= fmin < fmax <= sampling_rate / 2.0:
        raise ValueError(f"need 0 <= fmin < fmax <= sampling_rate / 2 (got fmin {fmin}, fmax {fmax}, sampling_rate {sampling_rate})")
    return fmax


_melspec_tables_cache = {}  # (n_fft, num_mels, sampling_rate, win_size, fmin, fmax, device) -> device tables, least recently used first


def _melspec_tables(n_fft, num_mels, sampling_rate, win_size, fmin, fmax, device):
    """(window, tw_re, tw_im, fb_start, fb_len, fb_off, fb_w) on `device`: built in fp64, rounded once to fp32"""
    key = (int(n_fft), int(num_mels), float(sampling_rate), int(win_size), float(fmin), float(fmax), str(device))
    hit = _melspec_tables_cache.pop(key, None)
    if hit is None:
        win, tw_re, tw_im = _stft_tables(n_fft, win_size)
        start, length, offset, weights = _filter_runs(slaney_mel_filterbank(n_fft, num_mels, sampling_rate, fmin, fmax).T)
        assert int((start + length).max()) <= n_fft // 2 + 1
        hit = tuple(t.to(device) for t in (win.float(), tw_re.float(), tw_im.float(), start, length, offset, weights.float()))
        if len(_melspec_tables_cache) >= 8:
            _melspec_tables_cache.pop(next(iter(_melspec_tables_cache)))
    _melspec_tables_cache[key] = hit
    return hit


def melspec_min_samples(n_fft, hop_size):
    """the shortest wave vbx_melspec takes: longer than the reflect pad, and one whole frame with it"""
    pad = melspec_pad(n_fft, hop_size)
    return max(pad + 1, n_fft - 2 * pad)


def _melspec(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, mean, std, channel_first, who, lens=None):
    """one launch of vbx_melspec (lens: vbx_melspec_lens) over waves [B, T] or [B, 1, T]; the arguments are already checked"""
    if y.ndim == 3 and y.shape[1] == 1:
        y = y[:, 0]
    if y.ndim != 2 or not y.is_floating_point():
        raise ValueError(f"{who} takes float waves (batch, samples), got {tuple(y.shape)} {y.dtype}")
    B, T = y.shape
    pad = melspec_pad(n_fft, hop_size)
    if T <= pad:
        raise RuntimeError(f"reflect padding of (n_fft - hop_size) / 2 = {pad} samples needs a longer wave (got {T} samples)")
    if T + 2 * pad < n_fft:
        raise RuntimeError(f"{T} samples and {pad} of padding on each side do not fill one frame of n_fft = {n_fft}")
    if lens is not None:  # checked (host values) or clamped (a device tensor) before anything else
        lens = device_lens(lens, B, T, melspec_min_samples(n_fft, hop_size), y.device, who)
    if y.device.type != "cuda":
        raise _lib.VbxError(f"{who} runs only on an MI355X (gfx950) through libvbx_hip.so; the wave is on '{y.device}'")
    tables = _melspec_tables(n_fft, num_mels, sampling_rate, win_size, fmin, fmax, y.device)
    y = y.detach().to(torch.float32).contiguous()
    frames = melspec_frames(T, n_fft, hop_size)
    out = torch.empty((B, num_mels, frames) if channel_first else (B, frames, num_mels), dtype=torch.float32, device=y.device)
    if B and lens is not None:
        _lib.call("vbx_melspec_lens", y, lens, out, *tables, B, T, n_fft, hop_size, pad, num_mels, 0.0 if mean is None else float(mean),
                  1.0 if std is None else 1.0 / float(std), int(channel_first), _lib.current_stream())
    elif B:
        _lib.call("vbx_melspec", y, out, *tables, B, T, n_fft, hop_size, pad, num_mels, 0.0 if mean is None else float(mean),
                  1.0 if std is None else 1.0 / float(std), int(channel_first), _lib.current_stream())
    return out


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """HiFi-GAN's meldataset.mel_spectrogram (BigVGAN ships the same function) on the device, one launch (csrc/mel.hip): waves
    y [B, T] -> ln(clamp(mel, 1e-5)) fp32 [B, num_mels, frames], frames = 1 + (T + 2 p - n_fft) // hop_size:

        p = int((n_fft - hop_size) / 2) samples of reflect padding on both sides (T > p, else RuntimeError as F.pad raises)
        frames of n_fft samples every hop_size (center=False), times the periodic Hann window of win_size samples centred in n_fft
        mag = sqrt(re^2 + im^2 + 1e-9);  mel = slaney_mel_filterbank(...) @ mag;  fmax=None: sampling_rate / 2

    PARITY UNPINNED: neither HiFi-GAN, BigVGAN nor librosa is a dependency and no vector of them is committed; this follows their
    published arithmetic, restated in fp64 in tests/hifigan_mel_ref.py.  Tables are cached per argument tuple and device.  Raises
    NotImplementedError for center=True, n_fft not a power of two in 256 .. 2048 and num_mels outside 1 .. 512, ValueError for the
    other argument ranges.  Runs only on the GPU; no gradient is taken through it."""
    fmax = _check_melspec_args(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center)
    return _melspec(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, None, None, True, "mel_spectrogram")


class HiFiGANMelCodec(AudioEncoderDecoder):
    """The mel front end HiFi-GAN and BigVGAN were trained on (mel_spectrogram above) as a codec: latents are ln(clamp(mel, 1e-5))
    fp32 [B, frames, num_mels], frames = samples // hop_size (n_fft - hop_size even), optionally (. - mean) / std with two scalars
    (the Voicebox paper's global normalisation; fit_normalization measures them).  The defaults are HiFi-GAN's V1 configuration.
    Published HiFi-GAN / BigVGAN weights want THIS codec, not LogMelCodec(vocoder=gen): that one hands HTK-scale, power, centred
    features no such checkpoint has seen.

    vocoder: a HiFiGANGenerator, a BigVGANGenerator or any module mel [B, num_mels, frames] -> wave, built with input_log=False
    (the codec already hands log features).  decode undoes the normalisation, transposes and calls it.  "griffin_lim" raises: that
    decode assumes centred framing.  PARITY with HiFi-GAN / BigVGAN / librosa is UNPINNED (mel_spectrogram's docstring)."""

    def __init__(self, *, num_mels=80, n_fft=1024, hop_size=256, win_size=1024, sampling_rate=22050, fmin=0, fmax=8000, vocoder=None,
                 mean=None, std=None):
        super().__init__()
        self.fmax = _check_melspec_args(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)
        if isinstance(vocoder, str):
            if vocoder == "griffin_lim":
                raise NotImplementedError('HiFiGANMelCodec(vocoder="griffin_lim") is not built: griffin_lim assumes centred framing '
                                          "(LogMelCodec serves it)")
            raise ValueError(f'vocoder must be None or a module (got "{vocoder}")')
        self.num_mels, self.n_fft, self.hop_size, self.win_size, self.fmin = int(num_mels), int(n_fft), int(hop_size), int(win_size), fmin
        self._sampling_rate = sampling_rate
        self.vocoder = vocoder
        self.mean = self.std = None
        self.set_normalization(mean, std)

    def set_normalization(self, mean, std):
        """both None: plain log mels; else the two scalars of (. - mean) / std, std > 0"""
        if (mean is None) != (std is None):
            raise ValueError("mean and std go together: give both or neither")
        if std is not None and not (float(std) > 0 and math.isfinite(float(std)) and math.isfinite(float(mean))):
            raise ValueError(f"need finite mean and std > 0 (got mean {mean}, std {std})")
        self.mean, self.std = (None, None) if mean is None else (float(mean), float(std))

    @classmethod
    def from_config(cls, config, vocoder=None, **kw):
        """config: a LOCAL config.json path or a dict with HiFi-GAN's / BigVGAN's keys num_mels, n_fft, hop_size, win_size,
        sampling_rate, fmin, fmax (null: sampling_rate / 2); every other key (fmax_for_loss, the generator's) is ignored.
        **kw: mean, std."""
        config = read_config(config)
        keys = ("num_mels", "n_fft", "hop_size", "win_size", "sampling_rate", "fmin", "fmax")
        missing = [k for k in keys if k not in config]
        if missing:
            raise KeyError(f"HiFiGANMelCodec.from_config: the config has no {missing}")
        return cls(vocoder=vocoder, **{k: config[k] for k in keys}, **kw)

    @classmethod
    def from_checkpoint(cls, generator_path, config, **kw):
        """A LOCAL generator file and its config.json (path or dict): a BigVGANGenerator when the config has an `activation` key,
        else a HiFiGANGenerator, built by their from_checkpoint, paired with the codec of the same config."""
        from .bigvgan import BigVGANGenerator
        from .hifigan import HiFiGANGenerator

        config = read_config(config)
        if not isinstance(config, dict):
            raise TypeError("HiFiGANMelCodec.from_checkpoint needs the generator's config (a local config.json path or a dict)")
        gen = (BigVGANGenerator if "activation" in config else HiFiGANGenerator).from_checkpoint(generator_path, config=config)
        return cls.from_config(config, vocoder=gen, **kw).eval()

    @property
    def downsample_factor(self):
        return self.hop_size

    @property
    def latent_dim(self):
        return self.num_mels

    @property
    def sampling_rate(self):
        return self._sampling_rate

    def _encode(self, audio, mean, std, lens=None):
        return _melspec(audio, self.n_fft, self.num_mels, self._sampling_rate, self.hop_size, self.win_size, self.fmin, self.fmax, mean,
                        std, False, "HiFiGANMelCodec.encode", lens=lens)

    def frame_lens(self, sample_lens):
        """melspec_frames of each length: a list, a CPU tensor or a device tensor; the same kind back"""
        return map_lens(sample_lens, lambda l: melspec_frames(l, self.n_fft, self.hop_size))

    def encode(self, audio, lens=None):
        """waves [B, T] or [B, 1, T] -> latents fp32 [B, frames, num_mels]; one launch, no host synchronisation.  lens: per-row
        sample counts of a padded batch, melspec_min_samples(n_fft, hop_size) <= len_b <= T (a list or CPU tensor is validated, a
        device tensor clamped): row b is the row alone up to frame_lens(lens)[b], exactly 0.0 (not the log floor) past it."""
        return self._encode(audio, self.mean, self.std, lens=lens)

    def fit_normalization(self, waves):
        """sets mean / std to the mean and (population) standard deviation of every plain log-mel value of `waves`, an iterable of
        device waves [B, T] (lengths may differ between items); plain torch reductions in fp64, one host read at the end"""
        n, s, ss = 0, None, None
        for w in waves:
            x = self._encode(w, None, None).double()
            n += x.numel()
            s = x.sum() if s is None else s + x.sum()
            ss = (x * x).sum() if ss is None else ss + (x * x).sum()
        if not n:
            raise ValueError("fit_normalization needs at least one wave")
        mean = float(s) / n
        self.set_normalization(mean, math.sqrt(max(float(ss) / n - mean * mean, 0.0)))
        return self.mean, self.std

    def decode(self, latents):
        """latents [B, frames, num_mels] -> vocoder(log mel [B, num_mels, frames]), the normalisation undone"""
        voc = self.vocoder
        if voc is None:
            raise NotImplementedError("HiFiGANMelCodec.decode needs a vocoder (log mel [B, num_mels, frames] -> wave): pass vocoder= "
                                      "(HiFiGANGenerator, BigVGANGenerator)")
        if getattr(voc, "input_log", False):
            raise ValueError("HiFiGANMelCodec hands LOG mels: build the vocoder with input_log=False")
        if getattr(voc, "n_mels", self.num_mels) != self.num_mels:
            raise ValueError(f"the vocoder takes {voc.n_mels} mel bins, the codec makes {self.num_mels}")
        if getattr(voc, "hop_length", self.hop_size) != self.hop_size:
            raise ValueError(f"the vocoder makes {voc.hop_length} samples per frame, the codec's hop_size is {self.hop_size}")
        if latents.ndim != 3 or latents.shape[2] != self.num_mels:
            raise ValueError(f"decode takes latents (batch, frames, num_mels = {self.num_mels}), got {tuple(latents.shape)}")
        mel = latents.transpose(1, 2)
        if self.mean is not None:
            mel = mel * self.std + self.mean
        return voc(mel)


RVQ_BANDWIDTH_QUANTIZERS = (2, 4, 8, 16)  # EnCodec 24 kHz: bandwidth ids 0 .. 3 (1.5, 3, 6, 12 kbps) -> codebooks in use


def _check_rvq_args(dim, codebook_size, num_quantizers):
    if dim % 8 or not 8 <= dim <= 256:
        raise NotImplementedError(f"ResidualVQ: dim must be a multiple of 8 in 8 .. 256 (got {dim})")
    if not 2 <= codebook_size <= 4096:
        raise NotImplementedError(f"ResidualVQ: codebook_size must be in 2 .. 4096 (got {codebook_size})")
    if not 1 <= num_quantizers <= 32:
        raise NotImplementedError(f"ResidualVQ: num_quantizers must be in 1 .. 32 (got {num_quantizers})")


class ResidualVQ(PackedWeights, nn.Module):
    """The residual vector quantizer of an EnCodec-style codec on the device (csrc/rvq.hip): one fp32 buffer `codebooks`
    [num_quantizers, codebook_size, dim], Euclidean codebooks, inference only.  Per frame, r_0 = x and for each quantizer q
    code_q = argmin_k |r_q - c_qk|^2 (the lowest index on an exact tie), r_{q+1} = r_q - c_q[code_q]; the quantized frame is
    c_0[code_0] + c_1[code_1] + ... summed in that order in fp32.  The search is fp32 throughout (include/vbx.h states its contract).

    forward(latents [B, N, dim]) -> (quantized [B, N, dim], codes int64 [B, N, Q], None): the triple the reference unpacks from
    `self.encodec.rq(latents)` (voicebox_pytorch.py:586-592); encode -> codes; decode(codes) -> latents.

    PARITY UNPINNED: vector_quantize_pytorch / encodec are not dependencies and no fixture of them exists; this follows their
    published arithmetic, restated in fp64 in tests/rvq_ref.py.  load_state_dict also takes two published layouts:
    `layers.{q}._codebook.embed` of shape [1, K, dim] or [K, dim] (vector_quantize_pytorch) and a flat [Q' * K, dim] table under
    `codebook_weights` (Vocos's EncodecFeatures; the first num_quantizers codebooks of a longer table are kept).

    Raises NotImplementedError outside dim a multiple of 8 in 8 .. 256, codebook_size 2 .. 4096, num_quantizers 1 .. 32.  GPU
    tensors only; float inputs of other dtypes are converted in."""

    def __init__(self, dim=128, codebook_size=1024, num_quantizers=8):
        super().__init__()
        _check_rvq_args(dim, codebook_size, num_quantizers)
        self.dim, self.codebook_size, self.num_quantizers = dim, codebook_size, num_quantizers
        self.register_buffer("codebooks", torch.randn(num_quantizers, codebook_size, dim))

    # -- state
    def _stacked(self, state_dict, prefix=""):
        """`codebooks` [Q, K, dim] from whichever of the three layouts the dict holds under `prefix`, or None"""
        Q, K, D = self.num_quantizers, self.codebook_size, self.dim
        if prefix + "codebooks" in state_dict:
            return state_dict[prefix + "codebooks"]
        if prefix + "layers.0._codebook.embed" in state_dict:
            rows = []
            for q in range(Q):
                e = state_dict[f"{prefix}layers.{q}._codebook.embed"]
                rows.append(e[0] if e.ndim == 3 else e)
            return torch.stack(rows)
        if prefix + "codebook_weights" in state_dict:
            flat = state_dict[prefix + "codebook_weights"]
            if flat.ndim != 2 or flat.shape[1] != D or flat.shape[0] % K or flat.shape[0] < Q * K:
                raise RuntimeError(f"ResidualVQ: codebook_weights {tuple(flat.shape)} does not hold {Q} codebooks of {K} x {D}")
            return flat[:Q * K].reshape(Q, K, D)
        return None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kw):
        """torch's per-module hook, so the published layouts load at any depth (ResidualVQ.load_state_dict as well as a codec's
        or a VoiceBox's with `rvq.` in front): they are rewritten to `codebooks` in the copy of the dict torch hands over"""
        cb = self._stacked(state_dict, prefix)
        if cb is not None and prefix + "codebooks" not in state_dict:
            for k in [k for k in state_dict if k.startswith(prefix + "layers.") or k == prefix + "codebook_weights"]:
                del state_dict[k]
            state_dict[prefix + "codebooks"] = cb.detach().to(torch.float32)
        return super()._load_from_state_dict(state_dict, prefix, *args, **kw)

    def _weights_key(self):
        return tensors_key((self.codebooks,))

    def _build_norms(self):
        Q, K, D = self.codebooks.shape
        norms = torch.empty(Q, K, dtype=torch.float32, device=self.codebooks.device)
        _lib.call("vbx_rvq_norms", self.codebooks, norms, Q, K, D, _lib.current_stream())
        return norms

    def _tables(self, device, who):
        """(codebooks, |c|^2 table) on `device`; the table is rebuilt when the buffer's storage or version counter changed
        (copy_, load_state_dict, .to()).  A write through `.data` changes neither: call mark_weights_dirty() after one.
        As LogMelCodec and VocosDecoder do, a module whose buffer is on another device than the input MOVES there (`self.to`): one
        ResidualVQ shared by several codecs follows the last input's device."""
        if device.type != "cuda":
            raise _lib.VbxError(f"{who} runs only on an MI355X (gfx950) through libvbx_hip.so; the input is on '{device}'")
        if self.codebooks.device != device:
            self.to(device)
        return self.codebooks, self._cached(self._build_norms)

    # -- device path
    def _search(self, latents, *, codes_qn, quantized, who):
        if latents.ndim != 3 or latents.shape[2] != self.dim:
            raise ValueError(f"{who} takes latents (batch, frames, dim = {self.dim}), got {tuple(latents.shape)}")
        if not latents.is_floating_point():
            raise TypeError(f"{who} takes floating-point latents (got {latents.dtype})")
        B, N, D = latents.shape
        if B < 1 or N < 1:
            raise ValueError(f"{who} needs at least one frame, got {tuple(latents.shape)}")
        cb, norms = self._tables(latents.device, who)
        Q, K = self.num_quantizers, self.codebook_size
        with torch.no_grad():  # plain tensors: the latents may go on into a training step
            x = latents.detach().to(torch.float32).contiguous()
            codes = torch.empty((B, Q, N) if codes_qn else (B, N, Q), dtype=torch.int64, device=x.device)
            quant = torch.empty(B, N, D, dtype=torch.float32, device=x.device) if quantized else None
            _lib.call("vbx_rvq_encode", x, cb, norms, codes, quant, B, N, D, K, Q, int(codes_qn), _lib.current_stream())
        return quant, codes

    def _gather(self, codes, *, codes_qn, channel_first, check, who):
        if codes.ndim != 3 or codes.dtype != torch.int64:
            raise ValueError(f"{who} takes int64 codes (batch, {'quantizers, frames' if codes_qn else 'frames, quantizers'}), got "
                             f"{codes.dtype} {tuple(codes.shape)}")
        B, Qc, N = codes.shape if codes_qn else (codes.shape[0], codes.shape[2], codes.shape[1])
        if not 1 <= Qc <= self.num_quantizers or B < 1 or N < 1:
            raise ValueError(f"{who}: codes of {Qc} quantizers x {N} frames for a quantizer of {self.num_quantizers}")
        cb, _ = self._tables(codes.device, who)
        K, D = self.codebook_size, self.dim
        with torch.no_grad():  # plain tensors: the latents may go on into a training step
            codes = codes.detach().contiguous()
            if check:
                lo, hi = torch.aminmax(codes)
                if int(lo) < 0 or int(hi) >= K:
                    raise ValueError(f"{who}: codes must lie in [0, {K}) (found {int(lo)} .. {int(hi)})")
            out = torch.empty((B, D, N) if channel_first else (B, N, D), dtype=torch.float32, device=codes.device)
            _lib.call("vbx_rvq_decode", codes, cb, out, B, N, D, K, Qc, int(codes_qn), int(channel_first), _lib.current_stream())
        return out

    def forward(self, latents):
        quant, codes = self._search(latents, codes_qn=False, quantized=True, who="ResidualVQ")
        return quant, codes, None

    def encode(self, latents):
        return self._search(latents, codes_qn=False, quantized=False, who="ResidualVQ.encode")[1]

    def decode(self, codes, check=True):
        """codes int64 [B, N, Q' <= Q] -> latents fp32 [B, N, dim].  check: one reduction over the codes and a ValueError for an
        index outside [0, codebook_size); with check=False such an index contributes zero."""
        return self._gather(codes, codes_qn=False, channel_first=False, check=check, who="ResidualVQ.decode")


class EncodecVocoCodec(AudioEncoderDecoder):
    """The reference's EncodecVoco (voicebox_pytorch.py:551-592) on the device: EnCodec's residual vector quantizer (ResidualVQ) and
    a Vocos decoder (VocosDecoder, or VocosEncodecDecoder: the published head) conditioned on EnCodec features.  Latents are the summed codewords [B, frames, rvq.dim].

      decode_to_codes(latents) -> codes int64 [B, Q, frames]        the RVQ search
      codes_to_latents(codes)  -> latents [B, frames, dim]          EncodecWrapper's get_emb_from_indices
      codes_to_features(codes) -> features [B, dim, frames]         Vocos.codes_to_features (from feature_rvq when given, else rvq)
      decode(latents)          -> wave = vocoder(codes_to_features(decode_to_codes(latents))), batched
      encode(audio)            -> codes_to_latents(decode_to_codes(encoder(audio)))

    `encoder` is a module audio [B, T] -> unquantized latents [B, frames, dim]: SEANetEncoder (seanet.py), EnCodec's encoder on the
    device, or the user's own; without one, encode raises.  from_encodec_checkpoint builds encoder, quantizer and -- when no
    vocoder is passed -- EnCodec's own decoder (SEANetDecoder, a vocoder by its call shape) from one local EnCodec state dict; the
    PUBLISHED encodec_24khz file is EnCodec's causal form and needs from_encodec_checkpoint(path, causal=True), which builds
    CausalSEANetEncoder / CausalSEANetDecoder (a state dict cannot say which form it is).  Neither weights nor the `encodec` / `vocos` libraries are
    part of this package; PARITY with them is UNPINNED (tests/rvq_ref.py restates the arithmetic)."""

    def __init__(self, *, rvq, vocoder, encoder=None, feature_rvq=None, sampling_rate=24000, downsample_factor=320):
        super().__init__()
        if not isinstance(rvq, ResidualVQ) or (feature_rvq is not None and not isinstance(feature_rvq, ResidualVQ)):
            raise TypeError("EncodecVocoCodec: rvq (and feature_rvq, when given) must be a ResidualVQ")
        if feature_rvq is not None and feature_rvq.num_quantizers < rvq.num_quantizers:
            raise ValueError("EncodecVocoCodec: feature_rvq must hold at least the quantizers of rvq")
        self.rvq, self.vocoder, self.encoder, self.feature_rvq = rvq, vocoder, encoder, feature_rvq
        self._sampling_rate, self._downsample_factor = sampling_rate, downsample_factor

    @property
    def downsample_factor(self):
        return self._downsample_factor

    @property
    def latent_dim(self):
        return self.rvq.dim

    @property
    def sampling_rate(self):
        return self._sampling_rate

    @classmethod
    def from_vocos_checkpoint(cls, path, *, bandwidth_id=2, encoder=None, codebook_size=1024, hop_length=None, sampling_rate=24000,
                              padding="center"):
        """A LOCAL Vocos-EnCodec state dict (torch.save of the dict, or {'state_dict': ...}): `feature_extractor.codebook_weights`
        [Q' * codebook_size, dim] becomes the codebooks, of which bandwidth ids 0 .. 3 use the first 2, 4, 8, 16 (capped by what
        the table holds).  padding="center" (the default): the vocoder is built as VocosDecoder.from_checkpoint(path,
        bandwidth_id=bandwidth_id) builds it, folded to that one id, (frames - 1) * hop samples.  padding="same": a
        VocosEncodecDecoder with the file's AdaLayerNorm tables kept and bandwidth_id as its default id -- for the published
        `vocos-encodec-24khz` file (n_fft 1280, hop 320) that is the reference's EncodecVoco, and decode returns [B, frames * 320].
        No such file is part of this package: the loader is exercised on synthetic files of that layout."""
        from .vocos import VocosDecoder, VocosEncodecDecoder

        if padding not in ("center", "same"):
            raise ValueError(f'padding must be "center" or "same" (got "{padding}")')

        sd = read_checkpoint(path)
        if "feature_extractor.codebook_weights" not in sd:
            raise KeyError("from_vocos_checkpoint: the state dict has no feature_extractor.codebook_weights (not a Vocos-EnCodec model)")
        if not 0 <= bandwidth_id < len(RVQ_BANDWIDTH_QUANTIZERS):
            raise ValueError(f"bandwidth_id must be in 0 .. {len(RVQ_BANDWIDTH_QUANTIZERS) - 1} (got {bandwidth_id})")
        flat = sd["feature_extractor.codebook_weights"]
        if flat.ndim != 2 or flat.shape[0] % codebook_size or flat.shape[0] < codebook_size:
            raise RuntimeError(f"from_vocos_checkpoint: codebook_weights {tuple(flat.shape)} is not a whole number of codebooks of "
                               f"{codebook_size}")
        rvq = ResidualVQ(dim=flat.shape[1], codebook_size=codebook_size,
                         num_quantizers=min(RVQ_BANDWIDTH_QUANTIZERS[bandwidth_id], flat.shape[0] // codebook_size))
        rvq.load_state_dict({"codebook_weights": flat})
        if padding == "same":
            vocoder = VocosEncodecDecoder.from_state_dict(sd, hop_length=hop_length, bandwidth_id=bandwidth_id)
        else:
            vocoder = VocosDecoder.from_state_dict(sd, hop_length=hop_length, bandwidth_id=bandwidth_id)
        return cls(rvq=rvq, vocoder=vocoder, encoder=encoder, sampling_rate=sampling_rate, downsample_factor=vocoder.hop_length).eval()

    @classmethod
    def from_encodec_checkpoint(cls, path, *, causal=False, trim_right_ratio=1.0, vocoder=None, bandwidth_id=2, feature_rvq=None,
                                sampling_rate=24000):
        """A LOCAL EnCodec state dict (torch.save of the dict, or {'state_dict': ...}): `encoder.*` becomes a SEANetEncoder (its
        limits apply), `quantizer.vq.layers.{q}._codebook.embed` [codebook_size, dim] the codebooks, of which bandwidth ids 0 .. 3
        use the first 2, 4, 8, 16 (capped by what the file holds); downsample_factor is the product of the encoder's ratios.
        Without `vocoder`, the file's `decoder.*` becomes a SEANetDecoder (EnCodec's own way back to a wave; KeyError when the file
        has no decoder half): the one file is then a complete codec.  A `vocoder` that is passed (a VocosDecoder) is used instead,
        and the decoder half of the file is not read.

        causal: the file cannot say whether its network is EnCodec's causal form (keys and shapes are the same), so the caller
        does.  The PUBLISHED `encodec_24khz` file is causal and needs causal=True, which builds CausalSEANetEncoder and (without
        `vocoder`) CausalSEANetDecoder with `trim_right_ratio`; with the default it loads without complaint and runs as a different
        network.  The default stays False only because existing callers depend on it: it builds exactly what it always built."""
        from .seanet import CausalSEANetDecoder, CausalSEANetEncoder, SEANetDecoder, SEANetEncoder

        if not causal and float(trim_right_ratio) != 1.0:
            raise ValueError("from_encodec_checkpoint: trim_right_ratio matters for causal=True alone")
        enc_cls, dec_cls, dec_kw = (CausalSEANetEncoder, CausalSEANetDecoder, dict(trim_right_ratio=trim_right_ratio)) if causal else \
            (SEANetEncoder, SEANetDecoder, {})

        sd = read_checkpoint(path)
        if not 0 <= bandwidth_id < len(RVQ_BANDWIDTH_QUANTIZERS):
            raise ValueError(f"bandwidth_id must be in 0 .. {len(RVQ_BANDWIDTH_QUANTIZERS) - 1} (got {bandwidth_id})")
        books, q = [], 0
        while f"quantizer.vq.layers.{q}._codebook.embed" in sd:
            books.append(sd[f"quantizer.vq.layers.{q}._codebook.embed"])
            q += 1
        if not books:
            raise KeyError("from_encodec_checkpoint: the state dict has no quantizer.vq.layers.0._codebook.embed (not an EnCodec model)")
        books = books[:RVQ_BANDWIDTH_QUANTIZERS[bandwidth_id]]
        encoder = enc_cls.from_state_dict({k: v for k, v in sd.items() if k.startswith("encoder.")})
        if vocoder is None:
            half = {k: v for k, v in sd.items() if k.startswith("decoder.")}
            if not any(k.startswith("decoder.model.") for k in half):
                raise KeyError("from_encodec_checkpoint: the state dict has no decoder.model.* (no decoder half); pass vocoder=")
            vocoder = dec_cls.from_state_dict(half, **dec_kw)
        rvq = ResidualVQ(dim=books[0].shape[1], codebook_size=books[0].shape[0], num_quantizers=len(books))
        rvq.load_state_dict({"codebook_weights": torch.cat([b.float() for b in books], dim=0)})
        return cls(rvq=rvq, vocoder=vocoder, encoder=encoder, feature_rvq=feature_rvq, sampling_rate=sampling_rate,
                   downsample_factor=encoder.hop_length).eval()

    def decode_to_codes(self, latents):
        return self.rvq._search(latents, codes_qn=True, quantized=False, who="EncodecVocoCodec.decode_to_codes")[1]

    def codes_to_latents(self, codes, check=True):
        return self.rvq._gather(codes, codes_qn=True, channel_first=False, check=check, who="EncodecVocoCodec.codes_to_latents")

    def codes_to_features(self, codes, check=True):
        table = self.rvq if self.feature_rvq is None else self.feature_rvq
        return table._gather(codes, codes_qn=True, channel_first=True, check=check, who="EncodecVocoCodec.codes_to_features")

    def frame_lens(self, sample_lens):
        """the encoder's frame counts: a list, a CPU tensor or a device tensor; the same kind back"""
        if not callable(getattr(self.encoder, "frame_lens", None)):
            raise NotImplementedError(f"EncodecVocoCodec.frame_lens needs an encoder with frame_lens (SEANetEncoder), got "
                                      f"{type(self.encoder).__name__}")
        return self.encoder.frame_lens(sample_lens)

    def encode(self, audio, lens=None):
        """lens: per-row sample counts of a padded batch, 1 <= len_b <= T, handed to the encoder (SEANetEncoder.forward(lens=)): row b
        is the row alone up to frame_lens(lens)[b]; the quantizer is per frame, and the frames past it are zero-filled after it."""
        if self.encoder is None:
            raise NotImplementedError("EncodecVocoCodec.encode needs an encoder (audio [B, T] -> latents [B, frames, dim]): EnCodec's "
                                      "SEANet encoder is not built; pass encoder=")
        if lens is None:
            with torch.no_grad():
                z = self.encoder(audio)
            return self.codes_to_latents(self.decode_to_codes(z), check=False)
        self.frame_lens([1])  # the encoder must serve lengths: NotImplementedError before anything is launched
        T = audio.shape[-1]
        lens = device_lens(lens, audio.shape[0], T, 1, audio.device, "EncodecVocoCodec.encode")
        with torch.no_grad():
            z = self.encoder(audio, lens=lens)
            lat = self.codes_to_latents(self.decode_to_codes(z), check=False)
            return zero_dead_frames(lat, self.frame_lens(lens))

    def decode(self, latents):
        """the reference loops over the batch and stacks (voicebox_pytorch.py:577-584); the same arithmetic, batched"""
        return self.vocoder(self.codes_to_features(self.decode_to_codes(latents), check=False))
