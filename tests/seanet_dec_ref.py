"""Host restatement of EnCodec's SEANet decoder (encodec/modules/seanet.py, conv.py, lstm.py as published, at the 24 kHz model's
settings: non-causal, reflect padding, weight norm, ELU, true_skip=False, no final activation) for the tests of
voicebox_pytorch_amd.SEANetDecoder.  PARITY with the `encodec` library itself is UNPINNED: it is not a dependency and no fixture of
it exists.  The pieces shared with the encoder (SConv1d, the LSTM loop, the fold, the fp16 rounding) are tests/seanet_ref.py's.

  decode(sd, cfg, z)                  plain fp64 from F.conv_transpose1d + the trim, seanet_ref.sconv / lstm and F.elu
  decode(sd, cfg, z, emulate=True)    the same with a rounding wherever the kernels' precision contract (include/vbx.h) rounds: the
                                      latents once to fp16, fp16 weights (folded in fp32), fp16 activations stored before the ELU, ELU
                                      in fp32 rounded to fp16 as an MFMA operand; in the last convolution fp32 weights and an fp32 ELU
                                      that is NOT rounded again; sums stay fp64 (the kernels' are fp32: what the GPU tests bound)
  decode(sd, cfg, z, fault=NAME)      plain fp64 with one planted fault (FAULTS)
  random_state(cfg, seed)             PyTorch's own default initialisation of nn.Conv1d / nn.ConvTranspose1d / nn.LSTM,
                                      weight_g = |v| (1 +- 0.2)

State-dict keys are the published ones: model.{i}.conv.conv.*, model.{i}.convtr.convtr.{weight_g [Cin, 1, 1], weight_v [Cin, Cout, k],
bias}, model.{i}.block.{1,3}.conv.conv.*, model.{i}.shortcut.conv.conv.*, model.{i}.lstm.*.  z [B, dimension, frames] channel-first
(EnCodec's own layout) -> wave [B, frames * prod(ratios)]."""
import math

import torch
import torch.nn.functional as F

from seanet_ref import fold, lstm, r16, rel_err, sconv  # noqa: F401  (rel_err: for the tests)

DEFAULT = dict(dimension=128, n_filters=32, n_residual_layers=1, ratios=(8, 5, 4, 2), kernel_size=7, last_kernel_size=7,
               residual_kernel_size=3, dilation_base=2, compress=2, lstm=2)
SMALL = dict(DEFAULT, n_filters=16, ratios=(5, 2), dimension=32)  # an odd ratio: swap_trim is invisible for even ones

FAULTS = ("swap_trim", "no_trim_left", "swap_taps", "no_elu_convtr", "wn_out", "no_lstm_skip", "zero_pad", "no_shortcut", "no_elu_last")


def config(**kw):
    return dict(DEFAULT, **kw)


def hop(cfg):
    return math.prod(cfg["ratios"])


def layout(cfg):
    """the `model` list: (index, kind, ...) with kind 'conv' (cin, cout, k), 'lstm' (dim, layers), 'elu', 'convtr' (cin, cout, k,
    stride), 'res' (dim, hidden, k, dilation)"""
    d = cfg["n_filters"] * 2 ** len(cfg["ratios"])
    out, i = [(0, "conv", cfg["dimension"], d, cfg["kernel_size"])], 0
    if cfg["lstm"]:
        i += 1
        out.append((i, "lstm", d, cfg["lstm"]))
    for r in cfg["ratios"]:
        out += [(i + 1, "elu"), (i + 2, "convtr", d, d // 2, 2 * r, r)]
        i, d = i + 2, d // 2
        for j in range(cfg["n_residual_layers"]):
            i += 1
            out.append((i, "res", d, d // cfg["compress"], cfg["residual_kernel_size"], cfg["dilation_base"] ** j))
    out += [(i + 1, "elu"), (i + 2, "conv", d, 1, cfg["last_kernel_size"])]
    return out


def expected_shapes(cfg):
    """key -> shape of the weight-norm layout"""
    conv = lambda p, ci, co, k: {f"{p}.conv.conv.weight_g": (co, 1, 1), f"{p}.conv.conv.weight_v": (co, ci, k), f"{p}.conv.conv.bias": (co,)}
    out = {}
    for e in layout(cfg):
        i, kind = e[0], e[1]
        if kind == "conv":
            out.update(conv(f"model.{i}", e[2], e[3], e[4]))
        elif kind == "convtr":
            p = f"model.{i}.convtr.convtr"
            out.update({f"{p}.weight_g": (e[2], 1, 1), f"{p}.weight_v": (e[2], e[3], e[4]), f"{p}.bias": (e[3],)})
        elif kind == "res":
            out.update(conv(f"model.{i}.block.1", e[2], e[3], e[4]))
            out.update(conv(f"model.{i}.block.3", e[3], e[2], 1))
            out.update(conv(f"model.{i}.shortcut", e[2], e[2], 1))
        elif kind == "lstm":
            for n in range(e[3]):
                out.update({f"model.{i}.lstm.weight_ih_l{n}": (4 * e[2], e[2]), f"model.{i}.lstm.weight_hh_l{n}": (4 * e[2], e[2]),
                            f"model.{i}.lstm.bias_ih_l{n}": (4 * e[2],), f"model.{i}.lstm.bias_hh_l{n}": (4 * e[2],)})
    return out


def random_state(cfg, seed):
    """fp32 state dict: the modules' own reset_parameters under a forked, seeded generator"""
    sd = {}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)

        def put(p, m):
            v = m.weight.detach().clone()
            n = v.shape[0]  # weight norm at dim 0: per output channel of a Conv1d, per INPUT channel of a ConvTranspose1d
            sd[f"{p}.weight_v"] = v
            sd[f"{p}.weight_g"] = (v.flatten(1).norm(dim=1) * (1 + 0.2 * (2 * torch.rand(n) - 1))).reshape(n, 1, 1)
            sd[f"{p}.bias"] = m.bias.detach().clone()

        conv = lambda p, ci, co, k: put(f"{p}.conv.conv", torch.nn.Conv1d(ci, co, k))
        for e in layout(cfg):
            i, kind = e[0], e[1]
            if kind == "conv":
                conv(f"model.{i}", e[2], e[3], e[4])
            elif kind == "convtr":
                put(f"model.{i}.convtr.convtr", torch.nn.ConvTranspose1d(e[2], e[3], e[4], stride=e[5]))
            elif kind == "res":
                conv(f"model.{i}.block.1", e[2], e[3], e[4])
                conv(f"model.{i}.block.3", e[3], e[2], 1)
                conv(f"model.{i}.shortcut", e[2], e[2], 1)
            elif kind == "lstm":
                for k, v in torch.nn.LSTM(e[2], e[2], e[3]).state_dict().items():
                    sd[f"model.{i}.lstm.{k}"] = v.detach().clone()
    return sd


def fold_tr(sd, prefix, dtype=torch.float64, per_output=False):
    """the transposed convolution's w [Cin, Cout, k] = g * v / |v|, the norm over (Cout, k) per input channel, in `dtype`;
    per_output: the planted fault, the norm over (Cin, k) per output channel (g broadcast as it is)"""
    v, g = sd[f"{prefix}.convtr.convtr.weight_v"].to(dtype), sd[f"{prefix}.convtr.convtr.weight_g"].to(dtype)
    if per_output:
        return g * v / v.transpose(0, 1).flatten(1).norm(dim=1).reshape(1, -1, 1)
    return g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)


def sconvtr(x, w, b, stride, fault=None):
    """the non-causal SConvTranspose1d: x [B, C, L] -> [B, Co, L * stride]; padding_total = k - stride is trimmed, right =
    padding_total // 2, left = padding_total - right"""
    k = w.shape[-1]
    if fault == "swap_taps":
        w = torch.cat([w[..., stride:], w[..., :stride]], dim=-1)
    y = F.conv_transpose1d(x, w, b, stride=stride)
    total = k - stride
    right = total // 2
    left = total - right
    if fault == "swap_trim":
        left, right = right, left
    if fault == "no_trim_left":
        left, right = 0, total
    return y[..., left:y.shape[-1] - right]


def decode(sd, cfg, z, emulate=False, fault=None):
    """z [B, dimension, frames] -> [B, frames * hop] fp64"""
    assert fault is None or (fault in FAULTS and not emulate)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    q = r16 if emulate else (lambda t: t)
    wfold = (lambda p: fold(sd, p, torch.float32).half().double()) if emulate else (lambda p: fold(sd, p))
    bias = lambda p: sd[f"{p}.conv.conv.bias"].double()
    elu = (lambda t: r16(F.elu(t.float()))) if emulate else F.elu
    pf = "zero_pad" if fault == "zero_pad" else None
    x = q(z.detach().cpu().double())
    act = False  # an ELU in front of the next layer
    last = layout(cfg)[-1][0]
    for e in layout(cfg):
        i, kind = e[0], e[1]
        if kind == "elu":
            act = True
        elif kind == "conv" and i != last:
            x = q(sconv(elu(x) if act else x, wfold(f"model.{i}"), bias(f"model.{i}"), fault=pf))
            act = False
        elif kind == "conv":  # the last one: fp32 weights, ELU in fp32 on the stored value, not rounded again; fp32 output
            w = fold(sd, f"model.{i}", torch.float32).double() if emulate else fold(sd, f"model.{i}")
            a = x if fault == "no_elu_last" else (F.elu(x.float()).double() if emulate else F.elu(x))
            x = sconv(a, w, bias(f"model.{i}"), fault=pf)
            if emulate:
                x = x.float().double()
        elif kind == "convtr":
            p = f"model.{i}"
            w = fold_tr(sd, p, torch.float32).half().double() if emulate else fold_tr(sd, p, per_output=fault == "wn_out")
            a = x if fault == "no_elu_convtr" else elu(x)
            x = q(sconvtr(a, w, sd[f"{p}.convtr.convtr.bias"].double(), e[5], fault=fault))
            act = False
        elif kind == "res":
            p = f"model.{i}"
            h = q(sconv(elu(x), wfold(f"{p}.block.1"), bias(f"{p}.block.1"), dilation=e[5], fault=pf))
            y = sconv(elu(h), wfold(f"{p}.block.3"), None, fault=pf)
            if fault != "no_shortcut":
                y = y + sconv(x, wfold(f"{p}.shortcut"), None, fault=pf)
                b = (sd[f"{p}.block.3.conv.conv.bias"].float() + sd[f"{p}.shortcut.conv.conv.bias"].float()).double() if emulate else \
                    bias(f"{p}.block.3") + bias(f"{p}.shortcut")
            else:
                b = bias(f"{p}.block.3")
            x = q(y + b[None, :, None])
        elif kind == "lstm":
            xt = x.transpose(1, 2)
            y = lstm(xt, sd, f"model.{i}.lstm", e[3], emulate=emulate)
            if fault != "no_lstm_skip":
                y = y + xt
            x = q(y).transpose(1, 2)
    return x[:, 0].contiguous()
