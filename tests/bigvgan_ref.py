"""Host restatement of BigVGAN's generator (Lee et al. 2023; bigvgan.py, activations.py and alias_free_activation/torch as published:
BigVGAN, AMPBlock1, AMPBlock2, Snake, SnakeBeta, Activation1d, UpSample1d, DownSample1d, LowPassFilter1d) for the tests of
voicebox_pytorch_amd.BigVGANGenerator.  PARITY with the BigVGAN library itself is UNPINNED: it is not a dependency and no fixture of
it exists.

  generate(sd, cfg, mel)                 plain fp64 from F.conv1d / F.conv_transpose1d / F.pad(mode="replicate") / torch.sin /
                                         torch.tanh / torch.clamp
  generate(sd, cfg, mel, emulate=True)   the same with a rounding wherever the kernels' precision contract (include/vbx.h) rounds: the
                                         mel once to fp16, fp16 weights (folded in fp32), fp16 activations where stored, alpha and
                                         1 / (beta + 1e-9) in fp32 (the exp included), Activation1d's result rounded to fp16 as an
                                         operand, the mean of the residual blocks in fp32 (rounded to fp16 only as the transposed
                                         convolution's operand), fp32 weights in conv_post, tanh / clamp in fp32; sums stay fp64
  generate(sd, cfg, mel, fault=NAME)     plain fp64 with one planted fault (FAULTS)
  activation1d(x, alpha, inv_beta, f_u, f_d)   A(x) by the padded construction; activation1d_closed: the closed form with clamps
  random_state(cfg, seed)                He-scaled normal weights as hifigan_ref.random_state; alpha in [1, 4], beta in [2, 4] (as logs
                                         under snake_logscale), so that alpha u spans several periods of sin^2; conv_post scaled so
                                         that the argument of tanh / clamp has RMS 0.8 on a probe input: a clamp cuts about a fifth
                                         of the samples

State-dict keys are the published ones: conv_pre.*, ups.{i}.0.*, resblocks.{i * nk + j}.convs1.{m}.* / convs2.{m}.* (AMPBlock2:
convs.{m}.*), resblocks.{n}.activations.{l}.act.alpha / .act.beta / .upsample.filter / .downsample.lowpass.filter, activation_post.*,
conv_post.* (no .bias with use_bias_at_final=False).  mel [B, n_mels, frames] -> wave [B, frames * prod(upsample_rates)]."""
import math

import torch
import torch.nn.functional as F

from hifigan_ref import conv, convtr, fold, mels, r16, rel_err  # noqa: F401  (the same primitives; nothing of HiFi-GAN's network)

SMALL = dict(n_mels=16, upsample_initial_channel=32, upsample_rates=(4, 2), upsample_kernel_sizes=(8, 4), resblock="1",
             resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, activation="snakebeta", snake_logscale=True,
             use_tanh_at_final=True, use_bias_at_final=True)
SMALL2 = dict(n_mels=20, upsample_initial_channel=64, upsample_rates=(2, 2, 2), upsample_kernel_sizes=(4, 4, 4), resblock="2",
              resblock_kernel_sizes=(3, 5), resblock_dilation_sizes=((1, 2), (2, 6)), activation="snake", snake_logscale=False,
              use_tanh_at_final=False, use_bias_at_final=False)
WIDE = dict(n_mels=100, upsample_initial_channel=1536, upsample_rates=(4, 4, 2, 2, 2, 2), upsample_kernel_sizes=(8, 8, 4, 4, 4, 4),
            resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, activation="snakebeta",
            snake_logscale=True, use_tanh_at_final=False, use_bias_at_final=False)

# planted into the plain fp64 restatement; NETWORK_FAULTS (bigvgan_tol.py) are those a whole-network comparison can tell from rounding
FAULTS = ("up_zero_pad", "down_zero_pad", "down_pad_65", "up_no_gain", "up_phase_swap", "no_exp", "beta_is_alpha", "acts_halves", "lrelu_ups",
          "tanh_for_clamp", "c2_dilated")
SLOPE = 0.1  # of the planted leaky ReLU in front of ups
ALPHA_LO, ALPHA_HI, BETA_LO, BETA_HI = 1.0, 4.0, 2.0, 4.0  # random_state: |ds/du| <= 1 + alpha / beta <= 3


def hop(cfg):
    return math.prod(cfg["upsample_rates"])


def applies(fault, cfg):
    """a fault that changes nothing in this configuration is not planted into it"""
    if fault == "no_exp":
        return cfg["snake_logscale"]
    if fault == "beta_is_alpha":
        return cfg["activation"] == "snakebeta"
    if fault in ("acts_halves", "c2_dilated"):
        return cfg["resblock"] == "1"
    return True


def kaiser_sinc_filter(dtype=torch.float32):
    """kaiser_sinc_filter1d(cutoff=0.25, half_width=0.3, kernel_size=12) as published, [12]"""
    beta = kaiser_beta()
    window = torch.kaiser_window(12, beta=beta, periodic=False, dtype=dtype)
    time = torch.arange(-6, 6, dtype=dtype) + 0.5
    f = 2 * 0.25 * window * torch.sinc(2 * 0.25 * time)
    return f / f.sum()


def kaiser_beta():
    """A = 2.285 (6 - 1) pi (4 * 0.3) + 7.95 = 51.02 is ABOVE 50, where the library takes 0.1102 (A - 8.7) = 4.6638 (its 0.5842 (A - 21)^0.4 +
    0.07886 (A - 21) is the branch for 21 <= A <= 50 and would give 4.6454)"""
    A = 2.285 * (6 - 1) * math.pi * (4 * 0.3) + 7.95
    assert A > 50.0
    return 0.1102 * (A - 8.7)


def activation1d(x, alpha, inv_beta, f_u, f_d, fault=None):
    """x [B, C, L] -> [B, C, L]; alpha, inv_beta [C]; f_u, f_d [12]: the padded construction"""
    C = x.shape[1]
    wu, wd = f_u.to(x.dtype).reshape(1, 1, 12).expand(C, 1, 12), f_d.to(x.dtype).reshape(1, 1, 12).expand(C, 1, 12)
    xp = F.pad(x, (5, 5)) if fault == "up_zero_pad" else F.pad(x, (5, 5), mode="replicate")
    u = F.conv_transpose1d(xp, wu, stride=2, groups=C)
    u = u[..., 14:-16] if fault == "up_phase_swap" else u[..., 15:-15]
    if fault != "up_no_gain":
        u = 2 * u
    a, ib = alpha.to(x.dtype).reshape(1, C, 1), inv_beta.to(x.dtype).reshape(1, C, 1)
    s = u + ib * torch.sin(a * u) ** 2
    pad = (6, 5) if fault == "down_pad_65" else (5, 6)
    sp = F.pad(s, pad) if fault == "down_zero_pad" else F.pad(s, pad, mode="replicate")
    return F.conv1d(sp, wd, stride=2, groups=C)


def activation1d_parts(x, alpha, inv_beta, f_u, f_d):
    """the closed form with both replicate paddings as clamps, and what a derived error bound needs: (y, U, S, absu, abss) with
    u[m] = 2 sum_i f_u[m + 5 - 2 i] x[clamp(i, 0, L - 1)], y[t] = sum_tau f_d[tau] s[clamp(2 t + tau - 5, 0, 2 L - 1)], absu = 2 sum |f_u x|"""
    B, C, L = x.shape
    m = torch.arange(2 * L)
    ilo = torch.div(m - 5, 2, rounding_mode="floor")
    u, absu = torch.zeros(B, C, 2 * L, dtype=x.dtype), torch.zeros(B, C, 2 * L, dtype=x.dtype)
    for q in range(6):
        i = ilo + q
        tap = f_u.to(x.dtype)[m + 5 - 2 * i]
        xi = x[..., i.clamp(0, L - 1)]
        u, absu = u + tap * xi, absu + (tap * xi).abs()
    u, absu = 2 * u, 2 * absu
    a, ib = alpha.to(x.dtype).reshape(1, C, 1), inv_beta.to(x.dtype).reshape(1, C, 1)
    s = u + ib * torch.sin(a * u) ** 2
    t = torch.arange(L)
    y, abss = torch.zeros(B, C, L, dtype=x.dtype), torch.zeros(B, C, L, dtype=x.dtype)
    idx = []
    for tau in range(12):
        mm = (2 * t + tau - 5).clamp(0, 2 * L - 1)
        idx.append(mm)
        y, abss = y + f_d.to(x.dtype)[tau] * s[..., mm], abss + (f_d.to(x.dtype)[tau] * s[..., mm]).abs()
    return y, u, s, absu, abss, idx


def activation1d_closed(x, alpha, inv_beta, f_u, f_d):
    return activation1d_parts(x, alpha, inv_beta, f_u, f_d)[0]


def act_bound(x, alpha, inv_beta, f_u, f_d):
    """(reference fp64, the per-element bound of vbx_bigvgan_act derived in include/vbx.h) for x fp64 [B, C, L] holding the fp32 operand"""
    y, u, s, absu, _, idx = activation1d_parts(x, alpha, inv_beta, f_u, f_d)
    C, eps = x.shape[1], 2.0 ** -24
    a, ib = alpha.double().reshape(1, C, 1), inv_beta.double().reshape(1, C, 1)
    e_u = 7 * eps * absu
    e_s = (1 + a.abs() * ib.abs()) * e_u + ib.abs() * (eps * (a * u).abs() + 2.0 ** -20 + eps) + eps * s.abs()
    carried, abss = torch.zeros_like(y), torch.zeros_like(y)
    for tau, mm in enumerate(idx):
        fd = abs(float(f_d[tau]))
        carried, abss = carried + fd * e_s[..., mm], abss + fd * s[..., mm].abs()
    return y, carried + 13 * eps * abss + 2.0 ** -11 * y.abs() + 2.0 ** -25


def act_emulated(x, alpha, inv_beta, f_u, f_d, round_u=False):
    """vbx_bigvgan_act's documented order of operations in fp32 on the host (torch has no fmaf: each product-sum step is done in fp64
    and rounded to fp32 once, which is what a fused multiply-add returns unless the fp64 sum itself rounds -- a double rounding far
    below the bound's slack); sin in fp64 rounded to fp32 stands for sinf.  round_u: the planted mistake, u rounded to fp16 before
    the snake.  x fp32 [B, C, L] -> fp16 [B, C, L]"""
    B, C, L = x.shape
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).float()
    m = torch.arange(2 * L)
    ilo = torch.div(m - 5, 2, rounding_mode="floor")
    acc = torch.zeros(B, C, 2 * L)
    for q in range(6):
        i = ilo + q
        acc = fma(f_u.float()[m + 5 - 2 * i], x[..., i.clamp(0, L - 1)], acc)
    u = 2.0 * acc
    if round_u:
        u = u.half().float()
    al, ib = alpha.float().reshape(1, C, 1), inv_beta.float().reshape(1, C, 1)
    sn = torch.sin((al * u).double()).float()
    s = fma(ib, sn * sn, u)
    t = torch.arange(L)
    acc = torch.zeros(B, C, L)
    for tau in range(12):
        acc = fma(f_d.float()[tau], s[..., (2 * t + tau - 5).clamp(0, 2 * L - 1)], acc)
    return acc.half()


def snake_params(sd, prefix, cfg, dtype=torch.float64, fault=None):
    """(alpha, 1 / (beta + 1e-9)) of the Activation1d at `prefix`; dtype fp32: as the device packs them"""
    alpha = sd[f"{prefix}.act.alpha"].to(dtype)
    beta = sd[f"{prefix}.act.beta"].to(dtype) if cfg["activation"] == "snakebeta" and fault != "beta_is_alpha" else alpha
    if cfg["snake_logscale"] and fault != "no_exp":
        alpha, beta = torch.exp(alpha), torch.exp(beta)
    return alpha, 1.0 / (beta + 1e-9)


def layout(cfg):
    """(prefix, kind, cin, cout, k, stride or dilation) of every convolution, in state-dict order"""
    c, nk = cfg["upsample_initial_channel"], len(cfg["resblock_kernel_sizes"])
    out = [("conv_pre", "conv", cfg["n_mels"], c, 7, 1)]
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        out.append((f"ups.{i}.0", "convtr", c, c // 2, k, u))
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


def act_layout(cfg):
    """(prefix, channels) of every Activation1d, in state-dict order"""
    c, nk, out = cfg["upsample_initial_channel"], len(cfg["resblock_kernel_sizes"]), []
    for i in range(len(cfg["upsample_rates"])):
        c //= 2
        for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
            n = len(ds) * (2 if cfg["resblock"] == "1" else 1)
            out += [(f"resblocks.{i * nk + j}.activations.{l}", c) for l in range(n)]
    return out + [("activation_post", c)]


def expected_shapes(cfg):
    out = {}
    for p, kind, ci, co, k, _ in layout(cfg):
        n = ci if kind == "convtr" else co
        out.update({f"{p}.weight_g": (n, 1, 1), f"{p}.weight_v": (ci, co, k) if kind == "convtr" else (co, ci, k), f"{p}.bias": (co,)})
    if not cfg["use_bias_at_final"]:
        del out["conv_post.bias"]
    for p, c in act_layout(cfg):
        out.update({f"{p}.act.alpha": (c,), f"{p}.upsample.filter": (1, 1, 12), f"{p}.downsample.lowpass.filter": (1, 1, 12)})
        if cfg["activation"] == "snakebeta":
            out[f"{p}.act.beta"] = (c,)
    return out


def random_state(cfg, seed, calibrate=True):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for p, kind, ci, co, k, s in layout(cfg):
        fan_in = ci * k // s if kind == "convtr" else ci * k
        scale = math.sqrt(2.0 / fan_in) * (0.5 if (".convs2." in p or ".convs." in p) else 1.0)
        v = scale * torch.randn((ci, co, k) if kind == "convtr" else (co, ci, k), generator=g)
        n = v.shape[0]
        sd[f"{p}.weight_v"] = v
        sd[f"{p}.weight_g"] = (v.flatten(1).norm(dim=1) * (1 + 0.2 * (2 * torch.rand(n, generator=g) - 1))).reshape(n, 1, 1)
        if p != "conv_post" or cfg["use_bias_at_final"]:
            sd[f"{p}.bias"] = 0.05 * torch.randn(co, generator=g)
    store = torch.log if cfg["snake_logscale"] else (lambda t: t)
    filt = kaiser_sinc_filter().reshape(1, 1, 12)
    for p, c in act_layout(cfg):
        sd[f"{p}.act.alpha"] = store(ALPHA_LO + (ALPHA_HI - ALPHA_LO) * torch.rand(c, generator=g))
        if cfg["activation"] == "snakebeta":
            sd[f"{p}.act.beta"] = store(BETA_LO + (BETA_HI - BETA_LO) * torch.rand(c, generator=g))
        sd[f"{p}.upsample.filter"], sd[f"{p}.downsample.lowpass.filter"] = filt.clone(), filt.clone()
    if calibrate:
        pre = generate(sd, cfg, mels(2, cfg["n_mels"], 9, 12345), final="none")
        sd["conv_post.weight_g"] = sd["conv_post.weight_g"] * float(0.8 / pre.pow(2).mean().sqrt())
    return sd


def generate(sd, cfg, mel, emulate=False, fault=None, input_log=False, final=None):
    """mel [B, n_mels, frames] -> [B, frames * hop] fp64; final: None = the configuration's, "none" = the argument of tanh / clamp"""
    assert fault is None or (fault in FAULTS and not emulate)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    q = r16 if emulate else (lambda t: t)
    W = (lambda p: fold(sd, p, torch.float32).half().double()) if emulate else (lambda p: fold(sd, p))
    bias = lambda p: sd[f"{p}.bias"].double()
    nk = len(cfg["resblock_kernel_sizes"])

    def act(p, x):
        """the Activation1d at prefix p; emulate: fp32 parameters, the result rounded to fp16 (an operand)"""
        al, ib = snake_params(sd, p, cfg, torch.float32 if emulate else torch.float64, fault)
        y = activation1d(x, al.double(), ib.double(), sd[f"{p}.upsample.filter"].reshape(12).double(),
                         sd[f"{p}.downsample.lowpass.filter"].reshape(12).double(), fault=fault)
        return q(y)

    def mean(xs):
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
    x = q(conv(x, W("conv_pre"), bias("conv_pre")))
    for i, u in enumerate(cfg["upsample_rates"]):
        p = f"ups.{i}.0"
        a = F.leaky_relu(x, SLOPE) if fault == "lrelu_ups" else x
        x = q(convtr(q(a), W(p), bias(p), u))  # the mean is rounded to fp16 as the operand
        outs = []
        for j, ds in enumerate(cfg["resblock_dilation_sizes"]):
            rb = f"resblocks.{i * nk + j}"
            h, n = x, len(ds)
            for m, d in enumerate(ds):
                if cfg["resblock"] == "1":
                    l1, l2 = (m, n + m) if fault == "acts_halves" else (2 * m, 2 * m + 1)
                    t = q(conv(act(f"{rb}.activations.{l1}", h), W(f"{rb}.convs1.{m}"), bias(f"{rb}.convs1.{m}"), dilation=d))
                    t = conv(act(f"{rb}.activations.{l2}", t), W(f"{rb}.convs2.{m}"), bias(f"{rb}.convs2.{m}"),
                             dilation=d if fault == "c2_dilated" else 1)
                else:
                    t = conv(act(f"{rb}.activations.{m}", h), W(f"{rb}.convs.{m}"), bias(f"{rb}.convs.{m}"), dilation=d)
                h = q(t + h)
            outs.append(h)
        x = mean(outs)
    x = act("activation_post", x)
    b = bias("conv_post") if cfg["use_bias_at_final"] else None
    tanh = cfg["use_tanh_at_final"] != (fault == "tanh_for_clamp")  # the fault: the other final function
    if emulate:  # fp32 weights on the fp16 operand; fp32 sum; tanh / clamp in fp32
        x = conv(x, fold(sd, "conv_post", torch.float32).double(), b).float()
    else:
        x = conv(x, fold(sd, "conv_post"), b)
    if final != "none":
        x = torch.tanh(x) if tanh else torch.clamp(x, -1.0, 1.0)
    return x.double()[:, 0].contiguous()
