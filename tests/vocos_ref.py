"""fp64 restatement on the CPU of the decoder VocosDecoder serves (csrc/vocos.hip): the published arithmetic of Vocos's
VocosBackbone / ConvNeXtBlock / ISTFTHead (padding="center") from F.conv1d, F.layer_norm, F.gelu and torch.istft.  The `vocos`
library is absent, so parity with it is UNPINNED; what can be pinned is pinned here: tests/test_vocos_cpu.py checks this file's
second, hand-written inverse STFT against torch.istft and the gamma fold against the unfolded form, and the kernels are tested
against this file.

`emulate=True` is the project's emulated-precision form: the same fp64 arithmetic with a rounding to fp16 at each point where the
device path rounds -- the im2col operand of the input convolution (= the features, after the optional fp32 log), the outputs of
the LayerNorms that feed a GEMM, the GELU output, and every packed weight, pwconv2 with gamma folded in fp32 first.  What then
separates the device from it is the order of fp32 sums and the last bits of erf / exp / sin / cos.

`fault` restates a wrong decoder on purpose (tests/test_vocos_gpu.py: the parity bound must be far below what each moves):
("drop_block", i), ("zero_gamma", i), ("eps", value), ("no_clip",)."""
import torch
import torch.nn.functional as F

LOG_FLOOR = 1e-7


def r16(x):
    """fp64 -> fp16 (round to nearest even, saturating as the device's stores) -> fp64"""
    return x.float().clamp(-65504.0, 65504.0).half().double()


def random_state(input_channels, dim, intermediate_dim, num_layers, n_fft, seed, m_offset=1.5):
    """A state dict with the published names in which every term matters: gamma in U(0.5, 1.5) (Vocos's own 1 / num_layers would
    hide a missing block behind the residual), LayerNorm affine terms away from (1, 0), weights scaled for unit-variance
    activations, and a head whose log-magnitudes m ~ N(m_offset, ~1.6^2) cross log(100) on a few per cent of the bins and whose
    phases spread over several turns."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    sd = {"backbone.embed.weight": n(dim, input_channels, 7) * (7 * input_channels) ** -0.5, "backbone.embed.bias": 0.1 * n(dim)}
    for name in ["backbone.norm", "backbone.final_layer_norm"] + [f"backbone.convnext.{i}.norm" for i in range(num_layers)]:
        sd[name + ".weight"] = 1.0 + 0.3 * n(dim)
        sd[name + ".bias"] = 0.3 * n(dim)
    for i in range(num_layers):
        p = f"backbone.convnext.{i}."
        sd[p + "dwconv.weight"] = n(dim, 1, 7) * 7 ** -0.5
        sd[p + "dwconv.bias"] = 0.1 * n(dim)
        sd[p + "pwconv1.weight"] = n(intermediate_dim, dim) * dim ** -0.5
        sd[p + "pwconv1.bias"] = 0.3 * n(intermediate_dim)
        sd[p + "pwconv2.weight"] = n(dim, intermediate_dim) * intermediate_dim ** -0.5
        sd[p + "pwconv2.bias"] = 0.1 * n(dim)
        sd[p + "gamma"] = 0.5 + torch.rand(dim, generator=g)
    nb = n_fft // 2 + 1
    w = n(n_fft + 2, dim) * dim ** -0.5
    w[nb:] *= 3.0  # phases
    sd["head.out.weight"] = w
    sd["head.out.bias"] = torch.cat((m_offset + 1.2 * n(nb), 3.0 * n(nb)))
    sd["head.istft.window"] = torch.hann_window(n_fft, periodic=True)
    return sd


def im2col(x, Kp):
    """[B, C, frames] -> [B * frames, Kp]: column tap * C + c of row (b, t) = x[b, c, t + tap - 3], zero outside [0, frames) of
    that batch element, zero columns from 7 * C"""
    B, C, T = x.shape
    xp = F.pad(x, (3, 3))
    cols = torch.stack([xp[:, :, k:k + T] for k in range(7)], dim=1)  # [B, 7, C, T]
    out = torch.zeros(B * T, Kp, dtype=x.dtype)
    out[:, :7 * C] = cols.permute(0, 3, 1, 2).reshape(B * T, 7 * C)
    return out


def log_features(x, emulate):
    """log(clamp(x, min=1e-7)): in fp64, or in fp32 as the device takes it"""
    if emulate:
        return torch.log(torch.clamp(x.float(), min=LOG_FLOOR)).double()
    return torch.log(torch.clamp(x.double(), min=LOG_FLOOR))


def fold_gamma(gamma, w2, b2, emulate):
    """the pwconv2 operands with the layer scale folded in: in fp32 and then rounded to fp16 (weight) as the device packs them, or
    in fp64"""
    if emulate:
        return r16(gamma.float()[:, None] * w2.float()), (gamma.float() * b2.float()).double()
    return gamma.double()[:, None] * w2.double(), gamma.double() * b2.double()


def istft_by_hand(spec, n_fft, hop, window):
    """torch.istft(center=True, length=None) written out: irfft of every frame, times the window, overlap-add, division by the
    window-square envelope, n_fft / 2 samples trimmed from both ends.  spec complex128 [B, n_fft / 2 + 1, frames]."""
    B, _, T = spec.shape
    fr = torch.fft.irfft(spec, n=n_fft, dim=1) * window[None, :, None]  # [B, n_fft, frames]
    total = n_fft + hop * (T - 1)
    y = torch.zeros(B, total, dtype=torch.float64)
    env = torch.zeros(total, dtype=torch.float64)
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += fr[:, :, t]
        env[t * hop:t * hop + n_fft] += window ** 2
    keep = slice(n_fft // 2, total - n_fft // 2)
    return y[:, keep] / env[keep]


def head_spectrum(o, n_fft, clip=True):
    """o [B, frames, n_fft + 2] -> (mag, phase), each [B, frames, n_fft / 2 + 1]"""
    m, p = o.chunk(2, dim=-1)
    mag = torch.exp(m)
    if clip:
        mag = torch.clamp(mag, max=100.0)
    return mag, p


def decode(sd, features, *, n_fft, hop, input_log=False, emulate=False, fault=None, by_hand=False, parts=False):
    """wave fp64 [B, (frames - 1) * hop] (and, with parts, the head's log-magnitudes m [B, frames, bins])"""
    q = r16 if emulate else (lambda t: t)
    d = {k: v.double() for k, v in sd.items()}
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("backbone.convnext."))
    dim = d["backbone.embed.weight"].shape[0]
    eps = fault[1] if fault and fault[0] == "eps" else 1e-6
    ln = lambda t, name: F.layer_norm(t, (dim,), d[name + ".weight"], d[name + ".bias"], eps)
    x = log_features(features, emulate) if input_log else features.double()
    x = F.conv1d(q(x), q(d["backbone.embed.weight"]), d["backbone.embed.bias"], padding=3)  # [B, dim, frames]
    x = ln(x.transpose(1, 2), "backbone.norm")  # [B, frames, dim], the fp32 residual stream on the device
    for i in range(layers):
        if fault == ("drop_block", i):
            continue
        p = f"backbone.convnext.{i}."
        h = F.conv1d(x.transpose(1, 2), d[p + "dwconv.weight"], d[p + "dwconv.bias"], padding=3, groups=dim).transpose(1, 2)
        h = q(ln(h, p + "norm"))
        h = q(F.gelu(h @ q(d[p + "pwconv1.weight"]).t() + d[p + "pwconv1.bias"]))
        gamma = torch.zeros(dim) if fault == ("zero_gamma", i) else sd[p + "gamma"]
        w2, b2 = fold_gamma(gamma, sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"], emulate)
        x = x + h @ w2.t() + b2
    h = q(ln(x, "backbone.final_layer_norm"))
    o = h @ q(d["head.out.weight"]).t() + d["head.out.bias"]
    mag, ph = head_spectrum(o, n_fft, clip=fault != ("no_clip",))
    spec = (mag * torch.complex(torch.cos(ph), torch.sin(ph))).transpose(1, 2)  # [B, bins, frames]
    window = d["head.istft.window"]
    if by_hand:
        wave = istft_by_hand(spec, n_fft, hop, window)
    else:
        wave = torch.istft(spec, n_fft, hop_length=hop, win_length=n_fft, window=window, center=True)
    return (wave, o[..., :n_fft // 2 + 1]) if parts else wave


def wave_err(got, ref):
    """max |difference| over the wave's RMS"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.pow(2).mean().sqrt())

