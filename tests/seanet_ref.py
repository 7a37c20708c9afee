"""Host restatement of EnCodec's SEANet encoder (encodec/modules/seanet.py, conv.py, lstm.py as published, at the 24 kHz model's
settings: non-causal, reflect padding, weight norm, ELU, true_skip=False) for the tests of voicebox_pytorch_amd.SEANetEncoder.
PARITY with the `encodec` library itself is UNPINNED: it is not a dependency and no fixture of it exists.

  encode(sd, cfg, wave)                  plain fp64 from F.pad / F.conv1d / F.elu and an explicit LSTM loop
  encode(sd, cfg, wave, emulate=True)    the same with a rounding wherever the kernels' precision contract (include/vbx.h) rounds:
                                         fp16 weights (folded in fp32), fp16 activations stored once-rounded before the ELU, ELU in
                                         fp32 rounded to fp16 as an operand, fp32 first convolution, h rounded to fp16 as the next
                                         product's operand; sums stay fp64 (the kernels' are fp32: that difference is what the GPU
                                         tests bound)
  encode(sd, cfg, wave, fault=NAME)      plain fp64 with one planted fault (FAULTS), for the test that the parity bound would see it
  random_state(cfg, seed)                PyTorch's own default initialisation of nn.Conv1d / nn.LSTM, weight_g = |v| (1 +- 0.2)

State-dict keys are the published ones: model.{i}.conv.conv.{weight_g, weight_v, bias}, model.{i}.block.{1,3}.conv.conv.*,
model.{i}.shortcut.conv.conv.*, model.{i}.lstm.{weight_ih, weight_hh, bias_ih, bias_hh}_l{n}.  Output [B, frames, dimension],
frames-major as SEANetEncoder returns it (EnCodec itself is channel-first)."""
import torch
import torch.nn.functional as F

DEFAULT = dict(dimension=128, n_filters=32, n_residual_layers=1, ratios=(8, 5, 4, 2), kernel_size=7, last_kernel_size=7,
               residual_kernel_size=3, dilation_base=2, compress=2, lstm=2)
SMALL = dict(DEFAULT, n_filters=16, ratios=(4, 2), dimension=32)

FAULTS = ("zero_pad", "swap_pads", "no_extra", "no_shortcut", "no_elu_strided", "no_lstm_skip", "gates_igfo", "no_b_hh", "layer1_lag")


def config(**kw):
    return dict(DEFAULT, **kw)


def layout(cfg):
    """the `model` list: (index, kind, ...) with kind 'conv' (cin, cout, k, stride), 'res' (dim, hidden, k, dilation), 'elu',
    'lstm' (dim, layers)"""
    nf, out, i = cfg["n_filters"], [], 0
    out.append((i, "conv", 1, nf, cfg["kernel_size"], 1))
    d = nf
    for r in reversed(cfg["ratios"]):
        for j in range(cfg["n_residual_layers"]):
            i += 1
            out.append((i, "res", d, d // cfg["compress"], cfg["residual_kernel_size"], cfg["dilation_base"] ** j))
        out += [(i + 1, "elu"), (i + 2, "conv", d, 2 * d, 2 * r, r)]
        i, d = i + 2, 2 * d
    if cfg["lstm"]:
        i += 1
        out.append((i, "lstm", d, cfg["lstm"]))
    out += [(i + 1, "elu"), (i + 2, "conv", d, cfg["dimension"], cfg["last_kernel_size"], 1)]
    return out


def expected_shapes(cfg):
    """key -> shape of the weight-norm layout"""
    conv = lambda p, ci, co, k: {f"{p}.conv.conv.weight_g": (co, 1, 1), f"{p}.conv.conv.weight_v": (co, ci, k), f"{p}.conv.conv.bias": (co,)}
    out = {}
    for e in layout(cfg):
        i, kind = e[0], e[1]
        if kind == "conv":
            out.update(conv(f"model.{i}", e[2], e[3], e[4]))
        elif kind == "res":
            out.update(conv(f"model.{i}.block.1", e[2], e[3], e[4]))
            out.update(conv(f"model.{i}.block.3", e[3], e[2], 1))
            out.update(conv(f"model.{i}.shortcut", e[2], e[2], 1))
        elif kind == "lstm":
            for n in range(e[3]):
                out.update({f"model.{i}.lstm.weight_ih_l{n}": (4 * e[2], e[2]), f"model.{i}.lstm.weight_hh_l{n}": (4 * e[2], e[2]),
                            f"model.{i}.lstm.bias_ih_l{n}": (4 * e[2],), f"model.{i}.lstm.bias_hh_l{n}": (4 * e[2],)})
    return out


def frames(cfg, T):
    for r in reversed(cfg["ratios"]):
        T = -(-T // r)
    return T


def random_state(cfg, seed):
    """fp32 state dict: nn.Conv1d's / nn.LSTM's own reset_parameters under a forked, seeded generator"""
    sd = {}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)

        def conv(p, ci, co, k):
            m = torch.nn.Conv1d(ci, co, k)
            v = m.weight.detach().clone()
            sd[f"{p}.conv.conv.weight_v"] = v
            sd[f"{p}.conv.conv.weight_g"] = (v.flatten(1).norm(dim=1) * (1 + 0.2 * (2 * torch.rand(co) - 1))).reshape(co, 1, 1)
            sd[f"{p}.conv.conv.bias"] = m.bias.detach().clone()

        for e in layout(cfg):
            i, kind = e[0], e[1]
            if kind == "conv":
                conv(f"model.{i}", e[2], e[3], e[4])
            elif kind == "res":
                conv(f"model.{i}.block.1", e[2], e[3], e[4])
                conv(f"model.{i}.block.3", e[3], e[2], 1)
                conv(f"model.{i}.shortcut", e[2], e[2], 1)
            elif kind == "lstm":
                for k, v in torch.nn.LSTM(e[2], e[2], e[3]).state_dict().items():
                    sd[f"model.{i}.lstm.{k}"] = v.detach().clone()
    return sd


def fold(sd, prefix, dtype=torch.float64):
    """w = g * v / |v| per output channel, in `dtype`"""
    v, g = sd[f"{prefix}.conv.conv.weight_v"].to(dtype), sd[f"{prefix}.conv.conv.weight_g"].to(dtype)
    return g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)


def r16(t):
    """the kernels round an fp32 value to fp16"""
    return t.float().half().double()


def pad1d(x, left, right, mode="reflect"):
    """encodec.modules.conv.pad1d: reflect padding that also serves inputs shorter than the padding"""
    if mode != "reflect":
        return F.pad(x, (left, right))
    L, extra = x.shape[-1], 0
    if L <= max(left, right):
        extra = max(left, right) - L + 1
        x = F.pad(x, (0, extra))
    y = F.pad(x, (left, right), mode="reflect")
    return y[..., :y.shape[-1] - extra]


def conv_pads(L, k, stride, dilation):
    """(pad_left, pad_right, extra) of the non-causal SConv1d"""
    keff = (k - 1) * dilation + 1
    total = keff - stride
    extra = -(-L // stride) * stride - L
    right = total // 2
    return total - right, right, extra


def sconv(x, w, b, stride=1, dilation=1, fault=None):
    """x [B, C, L] -> [B, Co, ceil(L / stride)]"""
    left, right, extra = conv_pads(x.shape[-1], w.shape[-1], stride, dilation)
    if fault == "swap_pads":
        left, right = right, left
    if fault == "no_extra":  # the positions of `extra` read as zeros instead of the reflection
        x = F.pad(pad1d(x, left, right), (0, extra))
    else:
        x = pad1d(x, left, right + extra, mode="zero" if fault == "zero_pad" else "reflect")
    return F.conv1d(x, w, b, stride=stride, dilation=dilation)


def lstm(x, sd, prefix, layers, emulate=False, fault=None):
    """x [B, T, H] -> [B, T, H]: nn.LSTM's recurrence (gates i, f, g, o; zero initial state) as an explicit loop.  emulate: fp16
    weights and matrix operands (x as given, h rounded), the two biases summed in fp32, layer 0's input projection stored as fp32"""
    B, T, H = x.shape
    q = r16 if emulate else (lambda t: t)
    wq = (lambda t: t.float().half().double()) if emulate else (lambda t: t.double())
    inp = q(x)
    for n in range(layers):
        wih, whh = wq(sd[f"{prefix}.weight_ih_l{n}"]), wq(sd[f"{prefix}.weight_hh_l{n}"])
        b_ih, b_hh = sd[f"{prefix}.bias_ih_l{n}"], sd[f"{prefix}.bias_hh_l{n}"]
        if fault == "no_b_hh":
            b_hh = torch.zeros_like(b_hh)
        bias = (b_ih.float() + b_hh.float()).double() if emulate else b_ih.double() + b_hh.double()
        h, c, outs = x.new_zeros(B, H), x.new_zeros(B, H), []
        for t in range(T):
            xt = inp[:, t]
            if fault == "layer1_lag" and n == 1:
                xt = inp[:, t - 1] if t > 0 else torch.zeros_like(xt)
            xp = xt @ wih.t() + bias
            if emulate and n == 0:
                xp = xp.float().double()
            gates = xp + q(h) @ whh.t()
            if fault == "gates_igfo":
                i, g, f, o = gates.chunk(4, dim=1)
            else:
                i, f, g, o = gates.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        out = torch.stack(outs, dim=1)
        inp = q(out)
    return out


def encode(sd, cfg, wave, emulate=False, fault=None):
    """wave [B, T] -> [B, frames, dimension] fp64"""
    assert fault is None or (fault in FAULTS and not emulate)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    q = r16 if emulate else (lambda t: t)
    wfold = (lambda p: fold(sd, p, torch.float32).half().double()) if emulate else (lambda p: fold(sd, p))
    bias = lambda p: sd[f"{p}.conv.conv.bias"].double()
    elu = (lambda t: r16(F.elu(t.float()))) if emulate else F.elu
    pf = None if fault in ("no_shortcut", "no_elu_strided", "no_lstm_skip", "gates_igfo", "no_b_hh", "layer1_lag") else fault
    x = wave.detach().cpu()
    x = (x.float() if emulate else x).double()[:, None]
    act = False  # an ELU in front of the next convolution
    last = layout(cfg)[-1][0]
    for e in layout(cfg):
        i, kind = e[0], e[1]
        if kind == "elu":
            act = True
        elif kind == "conv":
            if i == 0:
                w = fold(sd, "model.0", torch.float32).double() if emulate else fold(sd, "model.0")
            else:
                w = wfold(f"model.{i}")
            if act and not (fault == "no_elu_strided" and e[5] > 1):
                x = elu(x)
            x = sconv(x, w, bias(f"model.{i}"), stride=e[5], fault=pf)
            if i != last:
                x = q(x)
            elif emulate:
                x = x.float().double()  # the final convolution writes fp32
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
            y = lstm(xt, sd, f"model.{i}.lstm", e[3], emulate=emulate, fault=fault)
            if fault != "no_lstm_skip":
                y = y + xt
            x = q(y).transpose(1, 2)
    return x.transpose(1, 2).contiguous()


def rel_err(got, ref):
    """max |got - ref| / RMS(ref)"""
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.pow(2).mean().sqrt())
