"""Host restatement of HiFi-GAN's generator (Kong et al. 2020; models.py as published: Generator, ResBlock1, ResBlock2) for the tests
of voicebox_pytorch_amd.HiFiGANGenerator.  PARITY with the HiFi-GAN library itself is UNPINNED: it is not a dependency and no
fixture of it exists.

  generate(sd, cfg, mel)                 plain fp64 from F.conv1d / F.conv_transpose1d / F.leaky_relu / torch.tanh
  generate(sd, cfg, mel, emulate=True)   the same with a rounding wherever the kernels' precision contract (include/vbx.h) rounds: the
                                         mel once to fp16, fp16 weights (folded in fp32), fp16 activations stored before the leaky
                                         ReLU, the leaky ReLU and the mean of the residual blocks in fp32, rounded to fp16 as an MFMA
                                         operand; in conv_post fp32 weights and an fp32 operand that is NOT rounded again, tanh in
                                         fp32; sums stay fp64 (the kernels' are fp32: what the GPU tests bound)
  generate(sd, cfg, mel, fault=NAME)     plain fp64 with one planted fault (FAULTS)
  random_state(cfg, seed)                He-scaled normal weights, weight_g = |v| (1 +- 0.2); conv_post scaled so that the argument
                                         of tanh has RMS 0.8 on a fixed probe input (the output RMS is then about 0.6)

State-dict keys are the published ones: conv_pre.*, ups.{i}.{weight_g [Cin, 1, 1], weight_v [Cin, Cout, k], bias},
resblocks.{i * nk + j}.convs1.{m}.* / convs2.{m}.* (ResBlock2: convs.{m}.*), conv_post.*.  mel [B, n_mels, frames] -> wave
[B, frames * prod(upsample_rates)]."""
import math

import torch
import torch.nn.functional as F

V1 = dict(n_mels=80, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4), resblock="1",
          resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)
SMALL = dict(n_mels=16, upsample_initial_channel=32, upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), resblock="1",
             resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3)
SMALL2 = dict(n_mels=20, upsample_initial_channel=64, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), resblock="2",
              resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)))  # ResBlock2; 20 mels: padded to 24 columns

FAULTS = ("final_slope", "no_mean", "c2_dilated", "no_residual", "swap_taps", "trim_off", "wn_dim", "no_tanh", "pad_dil1", "mrf_chain")
SLOPE, LAST_SLOPE = 0.1, 0.01


def hop(cfg):
    return math.prod(cfg["upsample_rates"])


def r16(t):
    """the kernels round an fp32 value to fp16"""
    return t.float().half().double()


def rel_err(got, ref):
    """max |got - ref| / RMS(ref)"""
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.pow(2).mean().sqrt())


def layout(cfg):
    """(prefix, kind, cin, cout, k, stride or dilation) of every convolution, in state-dict order"""
    c, nk = cfg["upsample_initial_channel"], len(cfg["resblock_kernel_sizes"])
    out = [("conv_pre", "conv", cfg["n_mels"], c, 7, 1)]
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        out.append((f"ups.{i}", "convtr", c, c // 2, k, u))
        c //= 2
        for j, (rk, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            for m, d in enumerate(ds):
                if cfg["resblock"] == "1":
                    out += [(f"{p}.convs1.{m}", "conv", c, c, rk, d), (f"{p}.convs2.{m}", "conv", c, c, rk, 1)]
                else:
                    out.append((f"{p}.convs.{m}", "conv", c, c, rk, d))
    out.append(("conv_post", "conv", c, 1, 7, 1))
    return out


def expected_shapes(cfg):
    out = {}
    for p, kind, ci, co, k, _ in layout(cfg):
        n = ci if kind == "convtr" else co
        out.update({f"{p}.weight_g": (n, 1, 1), f"{p}.weight_v": (ci, co, k) if kind == "convtr" else (co, ci, k), f"{p}.bias": (co,)})
    return out


def fold(sd, p, dtype=torch.float64, per_output_tr=False):
    """w = g * v / |v|, the norm over all but dim 0 (torch's weight_norm default): per output channel of a Conv1d [Co, Ci, k], per INPUT
    channel of a ConvTranspose1d [Ci, Co, k]; a plain `weight` is taken as it is.  per_output_tr: the planted fault on a transposed
    weight, the norm over (Ci, k) per output channel"""
    if f"{p}.weight" in sd:
        return sd[f"{p}.weight"].to(dtype)
    v, g = sd[f"{p}.weight_v"].to(dtype), sd[f"{p}.weight_g"].to(dtype)
    if per_output_tr:
        return g * v / v.transpose(0, 1).flatten(1).norm(dim=1).reshape(1, -1, 1)
    return g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)


def random_state(cfg, seed, calibrate=True):
    """fp32 state dict; the second convolution of a residual pair (and ResBlock2's) at half the He scale, so that the residual stream
    grows by a modest factor per block"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for p, kind, ci, co, k, s in layout(cfg):
        fan_in = ci * k // s if kind == "convtr" else ci * k
        scale = math.sqrt(2.0 / fan_in) * (0.5 if (".convs2." in p or ".convs." in p) else 1.0)
        v = scale * torch.randn((ci, co, k) if kind == "convtr" else (co, ci, k), generator=g)
        n = v.shape[0]
        sd[f"{p}.weight_v"] = v
        sd[f"{p}.weight_g"] = (v.flatten(1).norm(dim=1) * (1 + 0.2 * (2 * torch.rand(n, generator=g) - 1))).reshape(n, 1, 1)
        sd[f"{p}.bias"] = 0.05 * torch.randn(co, generator=g)
    if calibrate:
        pre = generate(sd, cfg, mels(2, cfg["n_mels"], 9, 12345), fault="no_tanh")
        sd["conv_post.weight_g"] = sd["conv_post.weight_g"] * float(0.8 / pre.pow(2).mean().sqrt())
        sd["conv_post.bias"] = 0.05 * torch.randn(1, generator=g)
    return sd


def mels(B, n_mels, frames, seed, amplitude=False):
    """log-mel-like features; amplitude=True: their exponentials with some exact zeros (what input_log=True clamps)"""
    x = torch.randn(B, n_mels, frames, generator=torch.Generator().manual_seed(3000 + seed))
    if amplitude:
        x = torch.exp(2.0 * x)
        x[:, ::5, ::3] = 0.0
    return x


def conv(x, w, b, dilation=1, fault=None):
    """Conv1d with zero padding (k d - d) / 2 on both sides"""
    k = w.shape[-1]
    if fault == "swap_taps":
        w = w.flip(-1)
    total = (k - 1) * dilation
    left = (k - 1) // 2 if fault == "pad_dil1" else total // 2  # the fault: the window shifts, the length is kept
    return F.conv1d(F.pad(x, (left, total - left)), w, b, dilation=dilation)


def convtr(x, w, b, stride, fault=None):
    """ConvTranspose1d(k = 2 stride, stride, padding (k - stride) / 2): x [B, C, L] -> [B, Co, L * stride]"""
    k = w.shape[-1]
    pad = (k - stride) // 2
    if fault != "trim_off":
        return F.conv_transpose1d(x, w, b, stride=stride, padding=pad)
    y = F.conv_transpose1d(x, w, b, stride=stride)
    return y[..., pad + 1:pad + 1 + x.shape[-1] * stride]


def generate(sd, cfg, mel, emulate=False, fault=None, input_log=False):
    """mel [B, n_mels, frames] -> [B, frames * hop] fp64"""
    assert fault is None or (fault in FAULTS and not emulate)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    q = r16 if emulate else (lambda t: t)
    W = (lambda p: fold(sd, p, torch.float32).half().double()) if emulate else (lambda p: fold(sd, p))
    bias = lambda p: sd[f"{p}.bias"].double()
    # the leaky ReLU in front of an MFMA operand: fp32 on the stored fp16 value (or on the fp32 mean), rounded to fp16
    act = (lambda t: r16(F.leaky_relu(t.float(), SLOPE))) if emulate else (lambda t: F.leaky_relu(t, SLOPE))
    nk = len(cfg["resblock_kernel_sizes"])

    def mean(xs):
        if fault == "no_mean":
            return sum(xs)
        if not emulate:
            return sum(xs) / len(xs)
        s = xs[0].float()
        for t in xs[1:]:
            s = s + t.float()
        return (s / len(xs) if len(xs) > 1 else s).double()  # fp32, in index order; NOT rounded to fp16 on its own

    x = mel.detach().cpu()
    if input_log:
        x = torch.log(torch.clamp(x.float(), min=1e-5)) if emulate else torch.log(torch.clamp(x.double(), min=1e-5))
    x = q(x.double())
    x = q(conv(x, W("conv_pre"), bias("conv_pre"), fault=fault))
    for i, u in enumerate(cfg["upsample_rates"]):
        p = f"ups.{i}"
        w = fold(sd, p, per_output_tr=True) if fault == "wn_dim" else W(p)
        x = q(convtr(act(x), w, bias(p), u, fault=fault))
        outs, chain = [], x
        for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
            rb = f"resblocks.{i * nk + j}"
            h = chain if fault == "mrf_chain" else x
            for m, d in enumerate(ds):
                if cfg["resblock"] == "1":
                    t = q(conv(act(h), W(f"{rb}.convs1.{m}"), bias(f"{rb}.convs1.{m}"), dilation=d, fault=fault))
                    t = conv(act(t), W(f"{rb}.convs2.{m}"), bias(f"{rb}.convs2.{m}"), dilation=d if fault == "c2_dilated" else 1, fault=fault)
                else:
                    t = conv(act(h), W(f"{rb}.convs.{m}"), bias(f"{rb}.convs.{m}"), dilation=d, fault=fault)
                h = q(t if fault == "no_residual" else t + h)
            outs.append(h)
            chain = h
        x = chain if fault == "mrf_chain" else mean(outs)
    slope = SLOPE if fault == "final_slope" else LAST_SLOPE
    if emulate:  # fp32 weights, the leaky ReLU in fp32 on the fp32 mean, not rounded again; fp32 sum, tanh in fp32
        x = F.leaky_relu(x.float(), slope).double()
        x = conv(x, fold(sd, "conv_post", torch.float32).double(), bias("conv_post"))
        return torch.tanh(x.float()).double()[:, 0].contiguous()
    x = conv(F.leaky_relu(x, slope), fold(sd, "conv_post"), bias("conv_post"), fault=fault)
    return (x if fault == "no_tanh" else torch.tanh(x))[:, 0].contiguous()
