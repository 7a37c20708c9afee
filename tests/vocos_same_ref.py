"""fp64 restatement on the CPU of what VocosEncodecDecoder adds to VocosDecoder (tests/vocos_ref.py restates the rest): Vocos's ISTFT
at padding="same", the AdaLayerNorm network, and a host emulation of the mixed-radix inverse transform of csrc/fft_lds.hpp.  The
`vocos` library is absent, so parity with it is UNPINNED; tests/test_vocos_encodec_cpu.py checks this file against independent
constructions (torch.fft.irfft + F.fold, torch.istft, torch.fft.ifft, vocos_ref.decode), and the kernels are tested against this file.

`fault` restates a wrong decoder on purpose (the parity bounds must be far below what each moves):
  istft_same / decode:      ("trim_off_by_one",), ("center_trim",), ("env_untrimmed",)
  decode:                   ("id_swapped",), ("shift_dropped",)
  mixed_radix_inverse:      ("r5_twiddle_conj",)   one twiddle of the radix-5 pass (r = 3) conjugated
"""
import math

import torch
import torch.nn.functional as F

import vocos_ref as vr

LN_EPS = 1e-6
_dft = {}


def inverse_dft_matrix(n):
    """[n, n] complex128 e^{+2 pi i k t / n}, the angle reduced mod n in integers first"""
    if n not in _dft:
        kt = (torch.arange(n)[:, None] * torch.arange(n)[None, :]) % n
        ang = 2.0 * math.pi * kt.double() / n
        _dft[n] = torch.complex(ang.cos(), ang.sin())
    return _dft[n]


def hermitian_extend(spec, n_fft):
    """spec complex128 [..., n_fft / 2 + 1] -> [..., n_fft]: Z[n_fft - k] = conj(Z[k]), the imaginary parts of DC and Nyquist dropped
    (what a complex-to-real transform does with them)"""
    half = n_fft // 2
    z = torch.zeros(*spec.shape[:-1], n_fft, dtype=torch.complex128)
    z[..., :half + 1] = spec
    z[..., 0] = spec[..., 0].real
    z[..., half] = spec[..., half].real
    z[..., half + 1:] = spec[..., 1:half].conj().flip(-1)
    return z


def frames_same(spec, n_fft, window, inverse=None):
    """spec complex128 [B, n_fft / 2 + 1, T] -> the windowed frames [B, T, n_fft] (irfft at norm="backward", times the window) and
    the extended spectra [B, T, n_fft].  `inverse`: a function Z [n_fft] -> n_fft * ifft(Z) to use in place of the DFT matrix."""
    z = hermitian_extend(spec.transpose(1, 2), n_fft)
    if inverse is None:
        x = (z @ inverse_dft_matrix(n_fft)).real / n_fft
    else:
        x = torch.stack([torch.stack([inverse(zz).real for zz in zb]) for zb in z]) / n_fft
    return x * window.double(), z


def same_trim(n_fft, hop, frames, padding="same", fault=None):
    """(trim, out_len) of the (frames - 1) * hop + n_fft overlap-added samples"""
    if padding == "center":
        return n_fft // 2, (frames - 1) * hop
    trim = (n_fft - hop) // 2
    out_len = (frames - 1) * hop + n_fft - 2 * trim
    if fault == ("trim_off_by_one",):
        trim += 1
    if fault == ("center_trim",):
        trim = n_fft // 2  # hop <= n_fft / 2 keeps the range inside the sum
    return trim, out_len


def overlap_add(fr, window, hop, trim, out_len, env_from=None):
    """fr [B, T, n_fft] -> (wave [B, out_len], reciprocal envelope [out_len]): samples [trim, trim + out_len) of the sum over the
    frames in ascending order, over the window-square envelope of that range (of [env_from, ...) instead when given: a fault)"""
    B, T, n_fft = fr.shape
    total = n_fft + hop * (T - 1)
    y = torch.zeros(B, total + 1, dtype=torch.float64)
    env = torch.zeros(total + 1, dtype=torch.float64)
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += fr[:, t]
        env[t * hop:t * hop + n_fft] += window.double() ** 2
    e0 = trim if env_from is None else env_from
    renv = 1.0 / (env[e0:e0 + out_len] if env_from is None else env[e0:e0 + out_len].clamp(min=1e-11))  # the fault meets zeros
    return y[:, trim:trim + out_len] * renv, renv


def istft_same(spec, n_fft, hop, window, padding="same", fault=None, inverse=None):
    """Vocos's ISTFT (win_length = n_fft) written out: spec complex128 [B, n_fft / 2 + 1, T] -> wave fp64 [B, out_len]"""
    fr, _ = frames_same(spec, n_fft, window, inverse)
    trim, out_len = same_trim(n_fft, hop, spec.shape[2], padding, fault)
    return overlap_add(fr, window, hop, trim, out_len, env_from=0 if fault == ("env_untrimmed",) else None)[0]


# ----------------------------------------------------------------------------- the kernel's transform, emulated
def skew(i):
    return i + (i >> 6)


def bitrev(a, m):
    return int(format(a, f"0{m}b")[::-1], 2) if m else 0


def map5(j, m):
    """fft_map5 before the skew: element j = 5 a + r of the input goes to r * 2^m + bitrev_m(a)"""
    a, r = divmod(j, 5)
    return (r << m) + bitrev(a, m)


C1, C2 = math.cos(2 * math.pi / 5), math.cos(4 * math.pi / 5)
S1, S2 = math.sin(2 * math.pi / 5), math.sin(4 * math.pi / 5)


def mixed_radix_inverse(z, fault=None):
    """fft_lds5_inverse of csrc/fft_lds.hpp restated in fp64 with its index map, stage order and table lookups: z complex [N],
    N = 5 * 2^m -> (N * ifft(z) as a complex128 tensor, writes per LDS slot by the input map [fft_ld(N)])"""
    n = len(z)
    M, half_n = n // 5, n // 2
    m = M.bit_length() - 1
    assert n == 5 << m
    tw = [complex(math.cos(2 * math.pi * k / n), -math.sin(2 * math.pi * k / n)) for k in range(half_n)]  # tw_re + i tw_im
    lds = [None] * (n + (n >> 6))
    writes = [0] * len(lds)
    for j in range(n):
        slot = skew(map5(j, m))
        lds[slot] = complex(z[j])
        writes[slot] += 1
    for s in range(m):  # fft_lds<true, 5>: every radix-2 butterfly of the five sub-arrays
        half, tstep = 1 << s, 5 * ((half_n // 5) >> s)
        for q in range(half_n):
            pos = q & (half - 1)
            base = ((q >> s) << (s + 1)) + pos
            i0, i1 = skew(base), skew(base + half)
            b = lds[i1] * tw[pos * tstep].conjugate()
            a = lds[i0]
            lds[i0], lds[i1] = a + b, a - b
    for k in range(M):  # the radix-5 pass
        y = [lds[skew(k)]]
        for r in range(1, 5):
            j = r * k
            neg = j >= half_n
            w = tw[j - half_n if neg else j].conjugate()
            if neg:
                w = -w
            if fault == ("r5_twiddle_conj",) and r == 3:
                w = w.conjugate()
            y.append(lds[skew((r << m) + k)] * w)
        t1, t2, t3, t4 = y[1] + y[4], y[2] + y[3], y[1] - y[4], y[2] - y[3]
        m1, m2 = y[0] + C1 * t1 + C2 * t2, y[0] + C2 * t1 + C1 * t2
        n1, n2 = 1j * (S1 * t3 + S2 * t4), 1j * (S2 * t3 - S1 * t4)
        out = (y[0] + t1 + t2, m1 + n1, m2 + n2, m2 - n2, m1 - n1)
        for q in range(5):
            lds[skew(q * M + k)] = out[q]
    return torch.tensor([lds[skew(i)] for i in range(n)], dtype=torch.complex128), writes


# ----------------------------------------------------------------------------- the AdaLayerNorm network
def random_state(input_channels, dim, intermediate_dim, num_layers, n_fft, seed, rows=4, codebooks=0, codebook_size=16):
    """vocos_ref.random_state in the published Vocos-EnCodec layout: every backbone norm but final_layer_norm as scale / shift tables
    of `rows` ids, each row drawn like the plain affine terms (1 + 0.3 n, 0.3 n) so that ids differ and shifts matter; with
    `codebooks`, feature_extractor.codebook_weights [codebooks * codebook_size, input_channels] as well"""
    sd = vr.random_state(input_channels, dim, intermediate_dim, num_layers, n_fft, seed)
    g = torch.Generator().manual_seed(seed + 50)
    out = {}
    for k, v in sd.items():
        if k.endswith(".norm.weight"):
            out[k[:-len("weight")] + "scale.weight"] = torch.cat((v[None], 1.0 + 0.3 * torch.randn(rows - 1, dim, generator=g)))
        elif k.endswith(".norm.bias"):
            out[k[:-len("bias")] + "shift.weight"] = torch.cat((v[None], 0.3 * torch.randn(rows - 1, dim, generator=g)))
        else:
            out[k] = v
    if codebooks:
        out["feature_extractor.codebook_weights"] = torch.randn(codebooks * codebook_size, input_channels, generator=g)
    return out


def fold(sd, bandwidth_id):
    """the plain-LayerNorm state dict that row `bandwidth_id` of every table gives (feature_extractor.* dropped)"""
    out = {}
    for k, v in sd.items():
        if k.startswith("feature_extractor."):
            continue
        if k.endswith(".norm.scale.weight"):
            out[k[:-len("scale.weight")] + "weight"] = v[bandwidth_id]
        elif k.endswith(".norm.shift.weight"):
            out[k[:-len("shift.weight")] + "bias"] = v[bandwidth_id]
        else:
            out[k] = v
    return out


def spectrum(sd, features, *, n_fft, bandwidth_id=None, input_log=False, emulate=False, fault=None, noise=None):
    """the head's spectrum complex128 [B, n_fft / 2 + 1, frames].  Every AdaLayerNorm is layer_norm(x) * scale[id] + shift[id].
    emulate: fp16 roundings where the device rounds (vocos_ref's docstring).  noise = (relative size, seed): Gaussian relative noise
    in front of each of those roundings, to see what the position of the rounding boundaries is worth."""
    gen = torch.Generator().manual_seed(noise[1]) if noise else None

    def q(t):
        if not emulate:
            return t
        if noise:
            t = t * (1.0 + noise[0] * torch.randn(t.shape, generator=gen, dtype=torch.float64))
        return vr.r16(t)

    d = {k: v.double() for k, v in sd.items()}
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("backbone.convnext."))
    dim = d["backbone.embed.weight"].shape[0]

    def norm(t, name):
        if name + ".scale.weight" not in d:
            return F.layer_norm(t, (dim,), d[name + ".weight"], d[name + ".bias"], LN_EPS)
        i = bandwidth_id
        if fault == ("id_swapped",):
            i = (i + 1) % d[name + ".scale.weight"].shape[0]
        y = F.layer_norm(t, (dim,), None, None, LN_EPS) * d[name + ".scale.weight"][i]
        return y if fault == ("shift_dropped",) else y + d[name + ".shift.weight"][i]

    x = vr.log_features(features, emulate) if input_log else features.double()
    x = F.conv1d(q(x), q(d["backbone.embed.weight"]), d["backbone.embed.bias"], padding=3)
    x = norm(x.transpose(1, 2), "backbone.norm")
    for i in range(layers):
        p = f"backbone.convnext.{i}."
        h = F.conv1d(x.transpose(1, 2), d[p + "dwconv.weight"], d[p + "dwconv.bias"], padding=3, groups=dim).transpose(1, 2)
        h = q(norm(h, p + "norm"))
        h = q(F.gelu(h @ q(d[p + "pwconv1.weight"]).t() + d[p + "pwconv1.bias"]))
        w2, b2 = vr.fold_gamma(sd[p + "gamma"], sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"], emulate)
        x = x + h @ w2.t() + b2
    h = q(F.layer_norm(x, (dim,), d["backbone.final_layer_norm.weight"], d["backbone.final_layer_norm.bias"], LN_EPS))
    o = h @ q(d["head.out.weight"]).t() + d["head.out.bias"]
    mag, ph = vr.head_spectrum(o, n_fft)
    return (mag * torch.complex(torch.cos(ph), torch.sin(ph))).transpose(1, 2)


def decode(sd, features, *, n_fft, hop, bandwidth_id=None, padding="same", input_log=False, emulate=False, fault=None, noise=None):
    """wave fp64 [B, out_len] of the published-layout state dict `sd` (scale / shift tables, or plain LayerNorms)"""
    spec = spectrum(sd, features, n_fft=n_fft, bandwidth_id=bandwidth_id, input_log=input_log, emulate=emulate, fault=fault, noise=noise)
    return istft_same(spec, n_fft, hop, d64(sd["head.istft.window"]), padding=padding, fault=fault)


def d64(t):
    return t.double()
