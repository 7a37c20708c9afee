"""Host restatement of EnCodec's SEANet encoder and decoder in their CAUSAL form (encodec/modules/seanet.py, conv.py, lstm.py as
published, causal=True: what the published 24 kHz model is built with) for the tests of voicebox_pytorch_amd.CausalSEANetEncoder /
CausalSEANetDecoder.  PARITY with the `encodec` library itself is UNPINNED: it is not a dependency and no fixture of it exists.
What does not depend on the side (the layer lists, the weight-norm fold, the fp16 rounding, pad1d, the LSTM loop, the random
states) is tests/seanet_ref.py's and tests/seanet_dec_ref.py's, imported unchanged.

  SConv1d, causal           pad1d(x, (padding_total, extra), "reflect"): all of padding_total = k_eff - stride on the left, only
                            extra = ceil(L / stride) stride - L on the right; pad1d's short-input rule at max(padding_total, extra)
  SConvTranspose1d, causal  padding_right = ceil(padding_total * trim_right_ratio) trimmed behind, padding_total - padding_right in front

  encode(sd, cfg, wave) / decode(sd, cfg, z)   plain fp64
  ...(emulate=True)                            with a rounding wherever the kernels' precision contract (include/vbx.h) rounds, as in
                                               seanet_ref.encode / seanet_dec_ref.decode; sums stay fp64
  ...(fault=NAME)                              plain fp64 with one planted fault (FAULTS): each a way of getting the side wrong
  tolerance()                                  the whole-network tolerance of the GPU tests: one tenth of the smallest movement
                                               (max |delta| / RMS) any fault causes on the GPU tests' own inputs where it applies

cfg: seanet_ref.DEFAULT's keys; the decoder also reads cfg.get("trim_right_ratio", 1.0)."""
import functools
import math

import torch
import torch.nn.functional as F

import seanet_dec_ref as D
import seanet_ref as S
from seanet_dec_ref import fold_tr
from seanet_ref import fold, lstm, pad1d, r16, random_state, rel_err  # noqa: F401  (random_state, rel_err: for the tests)
from seanet_ref import layout  # the encoder's; the decoder's is seanet_dec_ref.layout

SMALL = S.SMALL  # n_filters 16, ratios (4, 2), dimension 32: hop 8
ENC_FAULTS = ("noncausal_pads", "extra_on_left", "zero_pad", "no_short_input_rule", "reflect_off_by_one")
DEC_FAULTS = ("noncausal_pads", "zero_pad", "no_short_input_rule", "reflect_off_by_one", "trim_left_instead", "trim_split", "ratio_floor")
FAULTS = ENC_FAULTS + DEC_FAULTS[4:]


def config(**kw):
    return dict(S.DEFAULT, **kw)


def frames(cfg, T):
    return S.frames(cfg, T)


def hop(cfg):
    return math.prod(cfg["ratios"])


def decoder_state(cfg, seed):
    return D.random_state(cfg, seed)


def conv_pads(L, k, stride, dilation):
    """(pad_left, pad_right) of the causal SConv1d: (padding_total, extra)"""
    total = (k - 1) * dilation + 1 - stride
    return total, -(-L // stride) * stride - L


def _gather(x, idx):
    """x[..., idx] with zeros where idx < 0"""
    i = torch.tensor(idx)
    return torch.where(i >= 0, x[..., i.clamp_min(0)], torch.zeros((), dtype=x.dtype))


def sconv(x, w, b, stride=1, dilation=1, fault=None):
    """the causal SConv1d: x [B, C, L] -> [B, Co, ceil(L / stride)]"""
    L = x.shape[-1]
    left, right = conv_pads(L, w.shape[-1], stride, dilation)
    if fault == "noncausal_pads":  # the old split: the smaller half and extra on the right
        total, extra = left, right
        left, right = total - total // 2, total // 2 + extra
    elif fault == "extra_on_left":
        left, right = left + right, 0
    if fault == "zero_pad":
        x = F.pad(x, (left, right))
    elif fault == "no_short_input_rule":  # no zeros appended: the row is mirrored again and again until the padding is filled
        P = max(2 * (L - 1), 1)
        x = _gather(x, [(m if m < L else P - m) for m in ((q - left) % P for q in range(left + L + right))])
    elif fault == "reflect_off_by_one":  # the mirror stands BETWEEN samples: the edge sample is repeated
        cut = max(max(left, right) - L, 0)
        x = F.pad(x, (0, cut))
        x = torch.cat([x[..., :left].flip(-1), x, x[..., x.shape[-1] - right:].flip(-1)], dim=-1)
        x = x[..., :x.shape[-1] - cut]
    else:
        x = pad1d(x, left, right)
    return F.conv1d(x, w, b, stride=stride, dilation=dilation)


def trims(stride, ratio, fault=None):
    """(trim_left, trim_right) of the causal SConvTranspose1d with k = 2 stride"""
    total = stride  # k - stride
    right = math.floor(total * ratio) if fault == "ratio_floor" else math.ceil(total * ratio)
    if fault == "trim_left_instead":
        right = 0
    elif fault == "trim_split":  # the non-causal trim
        right = total // 2
    return total - right, right


def sconvtr(x, w, b, stride, ratio=1.0, fault=None):
    """the causal SConvTranspose1d: x [B, C, L] -> [B, Co, L * stride]"""
    y = F.conv_transpose1d(x, w, b, stride=stride)
    left, right = trims(stride, ratio, fault)
    return y[..., left:y.shape[-1] - right]


def _resnet(x, sd, p, dilation, q, elu, wfold, bias, emulate, pf):
    h = q(sconv(elu(x), wfold(f"{p}.block.1"), bias(f"{p}.block.1"), dilation=dilation, fault=pf))
    y = sconv(elu(h), wfold(f"{p}.block.3"), None, fault=pf) + sconv(x, wfold(f"{p}.shortcut"), None, fault=pf)
    b = (sd[f"{p}.block.3.conv.conv.bias"].float() + sd[f"{p}.shortcut.conv.conv.bias"].float()).double() if emulate else \
        bias(f"{p}.block.3") + bias(f"{p}.shortcut")
    return q(y + b[None, :, None])


def _tools(sd, emulate):
    q = r16 if emulate else (lambda t: t)
    wfold = (lambda p: fold(sd, p, torch.float32).half().double()) if emulate else (lambda p: fold(sd, p))
    bias = lambda p: sd[f"{p}.conv.conv.bias"].double()
    elu = (lambda t: r16(F.elu(t.float()))) if emulate else F.elu
    return q, wfold, bias, elu


def encode(sd, cfg, wave, emulate=False, fault=None):
    """wave [B, T] -> [B, frames, dimension] fp64"""
    assert fault is None or (fault in ENC_FAULTS and not emulate)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    q, wfold, bias, elu = _tools(sd, emulate)
    x = wave.detach().cpu()
    x = (x.float() if emulate else x).double()[:, None]
    act, last = False, layout(cfg)[-1][0]
    for e in layout(cfg):
        i, kind = e[0], e[1]
        if kind == "elu":
            act = True
        elif kind == "conv":
            w = (fold(sd, "model.0", torch.float32).double() if emulate else fold(sd, "model.0")) if i == 0 else wfold(f"model.{i}")
            x = sconv(elu(x) if act else x, w, bias(f"model.{i}"), stride=e[5], fault=fault)
            x = q(x) if i != last else (x.float().double() if emulate else x)  # the final convolution writes fp32
            act = False
        elif kind == "res":
            x = _resnet(x, sd, f"model.{i}", e[5], q, elu, wfold, bias, emulate, fault)
        elif kind == "lstm":
            xt = x.transpose(1, 2)
            x = q(lstm(xt, sd, f"model.{i}.lstm", e[3], emulate=emulate) + xt).transpose(1, 2)
    return x.transpose(1, 2).contiguous()


def decode(sd, cfg, z, emulate=False, fault=None):
    """z [B, dimension, frames] -> [B, frames * hop] fp64"""
    assert fault is None or (fault in DEC_FAULTS and not emulate)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    q, wfold, bias, elu = _tools(sd, emulate)
    ratio = float(cfg.get("trim_right_ratio", 1.0))
    pf = fault if fault in ENC_FAULTS else None
    x = q(z.detach().cpu().double())
    act, last = False, D.layout(cfg)[-1][0]
    for e in D.layout(cfg):
        i, kind = e[0], e[1]
        if kind == "elu":
            act = True
        elif kind == "conv" and i != last:
            x = q(sconv(elu(x) if act else x, wfold(f"model.{i}"), bias(f"model.{i}"), fault=pf))
            act = False
        elif kind == "conv":  # the last one: fp32 weights, ELU in fp32 on the stored value, not rounded again; fp32 output
            w = fold(sd, f"model.{i}", torch.float32).double() if emulate else fold(sd, f"model.{i}")
            x = sconv(F.elu(x.float()).double() if emulate else F.elu(x), w, bias(f"model.{i}"), fault=pf)
            if emulate:
                x = x.float().double()
        elif kind == "convtr":
            p = f"model.{i}"
            w = fold_tr(sd, p, torch.float32).half().double() if emulate else fold_tr(sd, p)
            x = q(sconvtr(elu(x), w, sd[f"{p}.convtr.convtr.bias"].double(), e[5], ratio, fault=fault))
            act = False
        elif kind == "res":
            x = _resnet(x, sd, f"model.{i}", e[5], q, elu, wfold, bias, emulate, pf)
        elif kind == "lstm":
            xt = x.transpose(1, 2)
            x = q(lstm(xt, sd, f"model.{i}.lstm", e[3], emulate=emulate) + xt).transpose(1, 2)
    return x[:, 0].contiguous()


# ------------------------------------------------------------------------------------ the GPU tests' own inputs and their tolerance
ENC_T = (1, 3, 7, 8, 13, 192, 1003)
DEC_FRAMES = (1, 2, 3, 24, 131)
#               name        cfg                                                                        B
ENC_CONFIGS = {"small-r1": (dict(SMALL, n_residual_layers=1), 2), "small-r3": (dict(SMALL, n_residual_layers=3), 2)}
DEC_CONFIGS = {"small-r1": (dict(SMALL, n_residual_layers=1), 2), "small-r3": (dict(SMALL, n_residual_layers=3), 2),
               "r52-half": (dict(SMALL, ratios=(5, 2), trim_right_ratio=0.5), 2)}
REAL = config()  # the 24 kHz widths: one case, B = 1, 75 frames (24 000 samples)

# where a fault can show at all: `extra` is 0 when every stage's length is a multiple of its stride; the short-input rule runs only
# on a row no longer than its padding; ratio_floor needs an odd stride at a ratio whose product is no integer; a wave of ONE sample
# is one sample long in every layer of the encoder, where the rule's reflection of [x, 0, 0 ...] IS zero padding
_ENC_APPLIES = {"extra_on_left": lambda name, T: T % 8 != 0, "no_short_input_rule": lambda name, T: T <= 48,  # <= 6 frames
                "zero_pad": lambda name, T: T > 1}
_DEC_APPLIES = {"no_short_input_rule": lambda name, fr: fr <= 6, "ratio_floor": lambda name, fr: name == "r52-half"}


def wave(B, T, seed=0):
    return 0.3 * torch.randn(B, T, generator=torch.Generator().manual_seed(3000 + seed))


def latents(B, dim, fr, seed=0):
    return 3.0 * torch.randn(B, dim, fr, generator=torch.Generator().manual_seed(4000 + seed))


@functools.lru_cache(maxsize=None)
def encoder_case(name, T, seed=0):
    """(sd, wave, emulated, fp64) of one of the GPU tests' encoder inputs; computed once, shared, left unchanged"""
    cfg, B = (REAL, 1) if name == "real" else ENC_CONFIGS[name]
    sd, w = random_state(cfg, seed), wave(B, T, seed)
    return sd, w, encode(sd, cfg, w, emulate=True), encode(sd, cfg, w)


@functools.lru_cache(maxsize=None)
def decoder_case(name, fr, seed=0):
    cfg, B = (REAL, 1) if name == "real" else DEC_CONFIGS[name]
    sd, z = decoder_state(cfg, seed), latents(B, cfg["dimension"], fr, seed)
    return sd, z, decode(sd, cfg, z, emulate=True), decode(sd, cfg, z)


@functools.lru_cache(maxsize=None)
def fault_movements():
    """fault -> the smallest max |delta| / RMS it causes over the GPU tests' SMALL inputs on which it applies, per half:
    ({encoder fault: e}, {decoder fault: e})"""
    enc, dec = {}, {}
    for name, (cfg, _) in ENC_CONFIGS.items():
        for T in ENC_T:
            sd, w, _, ref = encoder_case(name, T)
            for f in ENC_FAULTS:
                if _ENC_APPLIES.get(f, lambda *a: True)(name, T):
                    enc[f] = min(enc.get(f, float("inf")), rel_err(encode(sd, cfg, w, fault=f), ref))
    for name, (cfg, _) in DEC_CONFIGS.items():
        for fr in DEC_FRAMES:
            sd, z, _, ref = decoder_case(name, fr)
            for f in DEC_FAULTS:
                if _DEC_APPLIES.get(f, lambda *a: True)(name, fr):
                    dec[f] = min(dec.get(f, float("inf")), rel_err(decode(sd, cfg, z, fault=f), ref))
    return enc, dec


def tolerance():
    """one tenth of the smallest movement of any fault: the whole-network tolerance (max |delta| / RMS) of the GPU tests"""
    enc, dec = fault_movements()
    return 0.1 * min(min(enc.values()), min(dec.values()))
