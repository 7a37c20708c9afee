"""SEANetEncoder and SEANetDecoder: the two halves of EnCodec (Defossez et al. 2022, "High fidelity neural audio compression") on
the device.

SEANetEncoder is the network behind `EncodecVoco.encode` of the reference (voicebox_pytorch.py:574-576): a 7-tap convolution,
four stages of (Resnet block, ELU, strided convolution), a 2-layer LSTM with a skip, ELU, a final 7-tap convolution.  Every
convolution is EnCodec's non-causal SConv1d: reflect padding by (pad_left, pad_right + extra) with pad1d's short-input rule, weight norm.  The
parameters carry the names and shapes of the published model (`model.{i}.conv.conv.weight_g` ...), so the `encoder.*` part of an
EnCodec state dict loads as is; neither the `encodec` library nor any weights are part of this package, and nothing here reaches a
hub: from_checkpoint reads a local file.

PARITY UNPINNED: the `encodec` library is not a dependency and no fixture of it exists.  This follows its published arithmetic
(encodec/modules/seanet.py, conv.py, lstm.py at the 24 kHz model's widths, causal=False), restated in fp64 with F.pad / F.conv1d / F.elu and an
explicit LSTM loop in tests/seanet_ref.py; the kernels are tested against that restatement (tests/test_seanet_gpu.py,
profiles/seanet_parity.txt).

Device path (csrc/seanet.hip, csrc/gemm.hip): a fixed launch sequence without host synchronisation.  Activations between layers
are fp16, channel-last, rounded once; weights are fp16 (weight norm folded in fp32 before the rounding); sums, ELU, the LSTM's
gates and cell state are fp32 (the precision contract in include/vbx.h).  Inference only.

SEANetDecoder is the other half of the same file: EnCodec's decoder (`decoder.*`), latents back into a wave -- a first convolution,
the LSTM, per ratio ELU + a strided transposed convolution (k = 2 r, as one product over the two input frames under every output
sample) + Resnet blocks, ELU and a last convolution to one channel; the same contract, the same state-dict layouts, restated in
tests/seanet_dec_ref.py.  EncodecVocoCodec.from_encodec_checkpoint(path) makes one local EnCodec state dict a complete codec.

CAUSAL OR NOT.  EnCodec's PUBLISHED 24 kHz model (`encodec_24khz`) is built with causal=True: every SConv1d pads all of
padding_total on the left, every SConvTranspose1d trims at the right end only (trim_right_ratio = 1.0).  SEANetEncoder and
SEANetDecoder are the NON-causal form; CausalSEANetEncoder and CausalSEANetDecoder at the end of this file are the causal one
(the same kernels, the padding side and the trim handed to them; restated in tests/seanet_causal_ref.py).  A state dict cannot
say which form it is -- keys and shapes are identical -- so the published file needs the Causal classes, or
from_encodec_checkpoint(path, causal=True); loaded into the non-causal classes it runs without complaint as a different
network.  The defaults stay non-causal only because existing callers depend on them.
"""
import math
import os

import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights, read_checkpoint
from ._wnconv import WNConv, weight_norm_key
from .wave_lens import device_lens, map_lens


class _NormConv(nn.Module):
    """NormConv1d: its `conv` is the nn.Conv1d, under weight norm or (norm="none") plain"""

    def __init__(self, cin, cout, k, norm):
        super().__init__()
        self.conv = WNConv(cin, cout, k, weight_norm=norm == "weight_norm")


class _SConv(nn.Module):
    def __init__(self, cin, cout, k, norm, stride=1, dilation=1):
        super().__init__()
        self.conv = _NormConv(cin, cout, k, norm)
        self.cin, self.cout, self.k, self.stride, self.dilation = cin, cout, k, stride, dilation

    @property
    def inner(self):
        return self.conv.conv


class _Resnet(nn.Module):
    def __init__(self, dim, compress, k, dilation, norm):
        super().__init__()
        hidden = dim // compress
        self.block = nn.ModuleList([nn.ELU(), _SConv(dim, hidden, k, norm, dilation=dilation), nn.ELU(), _SConv(hidden, dim, 1, norm)])
        self.shortcut = _SConv(dim, dim, 1, norm)


class _LSTMParams(nn.Module):
    """the parameters of nn.LSTM(dim, dim, layers) under its names (weight_ih_l{n} ..., gate order i, f, g, o), initialised as
    nn.LSTM initialises itself; a plain container, so moving it to the device touches no RNN library"""

    def __init__(self, dim, layers):
        super().__init__()
        for name, p in nn.LSTM(dim, dim, layers).named_parameters():
            self.register_parameter(name, nn.Parameter(p.detach().clone()))


class _SLSTM(nn.Module):
    def __init__(self, dim, layers):
        super().__init__()
        self.lstm = _LSTMParams(dim, layers)


class _NormConvTr(nn.Module):
    """NormConvTranspose1d: its `convtr` is the nn.ConvTranspose1d, weight [Cin, Cout, k]; torch's weight norm at its default dim=0
    gives it weight_g [Cin, 1, 1], the norm over (Cout, k) per INPUT channel"""

    def __init__(self, cin, cout, k, stride, norm):
        super().__init__()
        self.convtr = WNConv(cin, cout, k, stride=stride, transposed=True, weight_norm=norm == "weight_norm")


class _SConvTr(nn.Module):
    def __init__(self, cin, cout, stride, norm):
        super().__init__()
        self.convtr = _NormConvTr(cin, cout, 2 * stride, stride, norm)
        self.cin, self.cout, self.k, self.stride = cin, cout, 2 * stride, stride

    @property
    def inner(self):
        return self.convtr.convtr


def _check_keywords(who, channels, dimension, n_filters, n_residual_layers, ratios, activation, activation_params, norm, kernel_size,
                    last_kernel_size, residual_kernel_size, dilation_base, causal, pad_mode, true_skip, compress, lstm, causal_class=None):
    """what neither half of the network is built for; returns the exception factory for the caller's own refusals.  causal_class:
    the name of the Causal subclass that is being constructed (it alone admits causal=True, and nothing else), or None"""
    no = lambda what: NotImplementedError(f"{who}: {what} is not built")
    if causal_class and not causal:
        raise ValueError(f"{causal_class} is the causal network: causal=False is {who}")
    if causal and not causal_class:
        raise no(f"causal=True (use Causal{who})")
    if pad_mode != "reflect":
        raise no(f'pad_mode="{pad_mode}" (only "reflect")')
    if norm not in ("weight_norm", "none"):
        raise no(f'norm="{norm}" (only "weight_norm" and "none")')
    if activation != "ELU" or float((activation_params or {"alpha": 1.0}).get("alpha", 1.0)) != 1.0:
        raise no("an activation other than ELU(alpha=1)")
    if channels != 1:
        raise no(f"channels={channels} (only 1)")
    if true_skip:
        raise no("true_skip=True")
    if compress != 2:
        raise no(f"compress={compress} (only 2)")
    if n_filters <= 0 or n_filters % 16 or n_filters > 64:
        raise no(f"n_filters={n_filters} (a multiple of 16, at most 64)")
    if not 1 <= len(ratios) <= 4 or any(not 2 <= r <= 8 for r in ratios):
        raise no(f"ratios={ratios} (1 to 4 ratios, each in 2 .. 8)")
    if not 1 <= n_residual_layers <= 3:
        raise no(f"n_residual_layers={n_residual_layers} (1 .. 3)")
    if dilation_base != 2:
        raise no(f"dilation_base={dilation_base} (only 2)")
    if not 0 <= lstm <= 2:
        raise no(f"lstm={lstm} (0 .. 2)")
    if dimension <= 0 or dimension % 8 or dimension > 512:
        raise no(f"dimension={dimension} (a multiple of 8, at most 512)")
    for name, k in (("kernel_size", kernel_size), ("last_kernel_size", last_kernel_size)):
        if k < 1 or k % 2 == 0 or k > 7:
            raise no(f"{name}={k} (odd, at most 7)")
    if residual_kernel_size != 3:
        raise no(f"residual_kernel_size={residual_kernel_size} (only 3)")
    return no


class _SEANet(PackedWeights, nn.Module):
    """what SEANetEncoder and SEANetDecoder share: the state-dict layouts, the once-per-version operand packing, the launches of the
    convolution kernel and of the LSTM"""

    _HALF = ""  # "encoder" / "decoder": the prefix of this half in a whole EnCodec state dict
    _CAUSAL = None  # the name of a Causal subclass; None in the non-causal classes
    causal = False

    def _check_tiles(self, no):
        """whatever the convolution kernels cannot tile is refused at construction, not at the first forward; a Resnet block's 1 x 1
        tail is launched with the shortcut's input K-concatenated, and is asked about as launched"""
        tails = {id(m.block[3]): m.shortcut.cin for m in self.modules() if isinstance(m, _Resnet)}
        shortcuts = {id(m.shortcut) for m in self.modules() if isinstance(m, _Resnet)}
        for m in self.modules():
            try:
                # cin == 1 is the encoder's first convolution (vbx_seanet_conv0), cout == 1 the decoder's last (vbx_seanet_conv_out):
                # neither runs on the tiled kernel; the keyword ranges are all they need
                if isinstance(m, _SConv) and m.cin > 1 and m.cout > 1 and id(m) not in shortcuts:
                    _lib.call_value("vbx_seanet_conv_tile", m.cin, tails.get(id(m), 0), m.k, m.stride, m.dilation)
                elif isinstance(m, _SConvTr):
                    _lib.call_value("vbx_seanet_convtr_tile", m.cin, m.stride)
            except _lib.VbxError as e:
                if not os.path.exists(_lib.LIB_PATH):
                    raise
                raise no(f"a convolution {m.cin} -> {m.cout}, kernel {m.k}, stride {m.stride} ({e})") from None

    # -- state
    @classmethod
    def _canonical(cls, state_dict):
        """the two other layouts this accepts: a whole EnCodec dict (this half's prefix stripped, the other half and `quantizer.*`
        skipped) and newer torch's parametrizations.weight.original0 / original1 (= weight_g / weight_v)"""
        half = cls._HALF + "."
        if any(k.startswith(half) for k in state_dict):
            state_dict = {k[len(half):]: v for k, v in state_dict.items() if k.startswith(half)}
        out = {}
        for k, v in state_dict.items():
            if k.startswith(("encoder.", "decoder.", "quantizer.")):
                continue
            out[weight_norm_key(k)] = v
        return out

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict(self._canonical(state_dict), strict=strict, **kw)

    @classmethod
    def from_checkpoint(cls, path, **kw):
        """A LOCAL file written by torch.save: an EnCodec (or one half's) state dict or {'state_dict': ...}; see from_state_dict."""
        return cls.from_state_dict(read_checkpoint(path), **kw)

    # -- operand copies
    def packed_ops(self):
        """the launch list: fp16 GEMM operands and fp32 biases as the kernels read them; rebuilt when a parameter's storage or
        version counter changed (in-place updates, load_state_dict, .to()).  A write through `p.data` changes neither: call
        mark_weights_dirty() after one."""
        return self._cached(self._build_ops)

    @staticmethod
    def _gemm_weight(w):
        """folded fp32 [Co, Ci, k] -> fp32 [Co, k * Ci], column tap * Ci + c (the channel-last operand order)"""
        return w.permute(0, 2, 1).reshape(w.shape[0], -1)

    def folded_weights(self):
        """the folded fp32 weights by module path, e.g. 'model.3' -> [Co, Ci, k] (a transposed convolution's -> [Ci, Co, k]):
        what the three state-dict layouts agree on"""
        return {name: m.inner.folded() for name, m in self.named_modules() if isinstance(m, (_SConv, _SConvTr))}

    @classmethod
    def _conv_op(cls, m, elu, out_f32=False):
        return dict(op="conv", w=cls._gemm_weight(m.inner.folded()).half().contiguous(), b=m.inner.bias.detach().float().contiguous(), C1=m.cin,
                    C2=0, Co=m.cout, k=m.k, stride=m.stride, dil=m.dilation, elu=elu, out_f32=out_f32)

    @classmethod
    def _resnet_ops(cls, m):
        """a Resnet block: its dilated convolution (which reads x, kept for the tail), then the 1 x 1 tail and the shortcut in ONE product"""
        f = lambda t: t.detach().float().contiguous()
        c3, c1, sc = m.block[1], m.block[3], m.shortcut
        tail = torch.cat([cls._gemm_weight(c1.inner.folded()), cls._gemm_weight(sc.inner.folded())], dim=1)
        return [dict(cls._conv_op(c3, True), keep=True),
                dict(op="tail", w=tail.half().contiguous(), b=(f(c1.inner.bias) + f(sc.inner.bias)).contiguous(), C1=c1.cin, C2=sc.cin, Co=c1.cout,
                     k=1, stride=1, dil=1, elu=True, out_f32=False)]

    def _lstm_op(self, m):
        f = lambda t: t.detach().float().contiguous()
        h = lambda t: t.half().contiguous()
        l, H = m.lstm, self.hidden
        op = dict(op="lstm", H=H, layers=self.lstm, wih0=h(l.weight_ih_l0.detach().float()), whh0=h(l.weight_hh_l0.detach().float()),
                  b0=(f(l.bias_ih_l0) + f(l.bias_hh_l0)).contiguous(), wcat1=None, b1=None)
        if self.lstm == 2:
            op["wcat1"] = h(torch.cat([l.weight_ih_l1.detach().float(), l.weight_hh_l1.detach().float()], dim=1))
            op["b1"] = (f(l.bias_ih_l1) + f(l.bias_hh_l1)).contiguous()
        return op

    def _conv(self, op, x1, x2, y, B, L, st, lens=None):
        if lens is not None:
            _lib.call("vbx_seanet_conv_lens", x1, x2, lens, op["w"], op["b"], y, B, L, op["C1"], op["C2"], op["Co"], op["k"], op["stride"],
                      op["dil"], int(op["elu"]), int(op["out_f32"]), int(self.causal), st)
            return
        _lib.call("vbx_seanet_conv_c", x1, x2, op["w"], op["b"], y, B, L, op["C1"], op["C2"], op["Co"], op["k"], op["stride"], op["dil"],
                  int(op["elu"]), int(op["out_f32"]), int(self.causal), st)

    @staticmethod
    def lstm_forward(op, x, B, T, st, y32=None):
        """The SLSTM alone: x fp16 [B, T, H] on the device -> y fp16 [B, T, H] = LSTM(x) + x; one GEMM for layer 0's input projection,
        then T + layers - 1 steps.  op: dict(H, layers, wih0 / whh0 fp16 [4H, H], b0 fp32 [4H] = b_ih0 + b_hh0, and for two layers
        wcat1 fp16 [4H, 2H] = [W_ih1 | W_hh1], b1 fp32 [4H]; else None).  y32, when given, receives the sum before its rounding."""
        H, dev = op["H"], x.device
        xproj = torch.empty(B * T, 4 * H, dtype=torch.float32, device=dev)
        d = _lib.GemmDesc()
        d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16 = _lib.VBX_GEMM_NT, _lib.VBX_EPI_F32, B * T, 4 * H, H, H, H, 4 * H, 1
        d.A, d.B, d.C, d.bias, d.resid = x.data_ptr(), op["wih0"].data_ptr(), xproj.data_ptr(), op["b0"].data_ptr(), None
        rc = _lib.lib().vbx_gemm(d, st)
        if rc != 0:
            raise _lib.VbxError(f"vbx_gemm failed (rc={rc}): {_lib.lib().vbx_last_error().decode()}")
        h0 = torch.empty(B, T, H, dtype=torch.float16, device=dev)
        h1 = torch.empty(B, T, H, dtype=torch.float16, device=dev) if op["layers"] == 2 else None
        c = torch.empty(op["layers"], B, H, dtype=torch.float32, device=dev)
        y = torch.empty(B, T, H, dtype=torch.float16, device=dev)
        _lib.call("vbx_lstm", xproj, op["whh0"], op["wcat1"], op["b1"], h0, h1, c, x, y, y32, B, T, H, op["layers"], st)
        return y


class SEANetEncoder(_SEANet):
    """audio [B, T] or [B, 1, T] (any float dtype, on the GPU) -> unquantized latents fp32 [B, frames, dimension], frames =
    ceil(... ceil(T / r_last) ... / r_first) over reversed(ratios).  FRAMES-MAJOR, what EncodecVocoCodec.encode expects of
    `encoder=`; EnCodec's own SEANetEncoder returns channel-first [B, dimension, frames] -- transpose when comparing.

    Runs without gradients, in eval semantics.  The folded fp16 weights are packed once and re-packed when a parameter's version
    counter or storage changes; after a write through `p.data` call mark_weights_dirty().

    Raises NotImplementedError for what is not built: causal=True (served by CausalSEANetEncoder, not here), pad_mode other than "reflect", norm other than "weight_norm" /
    "none", an activation other than ELU(alpha=1), channels != 1, true_skip=True, compress != 2, n_filters not a multiple of 16 or
    above 64, other than 1 .. 4 ratios or a ratio outside 2 .. 8, n_residual_layers outside 1 .. 3, dilation_base != 2, lstm
    outside 0 .. 2, dimension not a multiple of 8 or above 512, kernel_size / last_kernel_size even or above 7,
    residual_kernel_size != 3, and any convolution of which 16 output positions do not fit the LDS (none inside these ranges: the
    widest, 512 -> 1024 with kernel 16 and stride 8, takes 138 of 160 KiB).  GPU tensors only; like its siblings, a forward on a
    device other than the parameters' MOVES THE MODULE there (`self.to(device)`) -- keep one instance per device."""

    _HALF = "encoder"

    def __init__(self, channels=1, dimension=128, n_filters=32, n_residual_layers=1, ratios=(8, 5, 4, 2), activation="ELU",
                 activation_params=None, norm="weight_norm", kernel_size=7, last_kernel_size=7, residual_kernel_size=3,
                 dilation_base=2, causal=False, pad_mode="reflect", true_skip=False, compress=2, lstm=2):
        super().__init__()
        ratios = tuple(int(r) for r in ratios)
        no = _check_keywords("SEANetEncoder", channels, dimension, n_filters, n_residual_layers, ratios, activation, activation_params, norm,
                             kernel_size, last_kernel_size, residual_kernel_size, dilation_base, causal, pad_mode, true_skip, compress, lstm,
                             causal_class=self._CAUSAL)
        self.causal = bool(causal)
        self.channels, self.dimension, self.n_filters, self.n_residual_layers, self.ratios = channels, dimension, n_filters, n_residual_layers, ratios
        self.norm, self.kernel_size, self.last_kernel_size, self.residual_kernel_size = norm, kernel_size, last_kernel_size, residual_kernel_size
        self.dilation_base, self.compress, self.lstm = dilation_base, compress, lstm
        self.hop_length = math.prod(ratios)
        model, d = [_SConv(channels, n_filters, kernel_size, norm)], n_filters
        for r in reversed(ratios):
            for j in range(n_residual_layers):
                model.append(_Resnet(d, compress, residual_kernel_size, dilation_base ** j, norm))
            model += [nn.ELU(), _SConv(d, 2 * d, 2 * r, norm, stride=r)]
            d *= 2
        if lstm:
            model.append(_SLSTM(d, lstm))
        model += [nn.ELU(), _SConv(d, dimension, last_kernel_size, norm)]
        self.model = nn.ModuleList(model)
        self.hidden = d
        self._check_tiles(no)

    def frames(self, T):
        for r in reversed(self.ratios):
            T = -(-T // r)
        return T

    @classmethod
    def from_state_dict(cls, sd, **kw):
        """A state dict already in memory, in any of the three layouts.  The widths are read off the shapes; the ratios off the
        strided kernels (k = 2 r); reflect padding and ELU are taken as given.  A state dict CANNOT say whether its network is
        causal -- the keys and shapes are the same -- so the class says it: SEANetEncoder.from_state_dict builds the non-causal
        network, CausalSEANetEncoder.from_state_dict the causal one (what the published `encodec_24khz` file needs)."""
        sd = cls._canonical(sd)
        idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("model.")})
        norm = "weight_norm" if "model.0.conv.conv.weight_g" in sd else "none"
        wkey = "weight_v" if norm == "weight_norm" else "weight"
        shape = lambda name: tuple(sd[f"{name}.conv.conv.{wkey}"].shape)
        n_filters, channels, kernel_size = shape("model.0")
        res = [i for i in idx if f"model.{i}.shortcut.conv.conv.bias" in sd]
        lstm_i = [i for i in idx if f"model.{i}.lstm.weight_ih_l0" in sd]
        convs = [i for i in idx if f"model.{i}.conv.conv.bias" in sd]
        strided = convs[1:-1]
        if not strided or not res or len(res) % len(strided):
            raise RuntimeError("SEANetEncoder.from_state_dict: not a SEANet encoder layout (Resnet blocks and strided convolutions)")
        ratios = tuple(reversed([shape(f"model.{i}")[2] // 2 for i in strided]))
        lstm = 0 if not lstm_i else 1 + max(int(k[-1]) for k in sd if k.startswith(f"model.{lstm_i[0]}.lstm.weight_ih_l"))
        first = res[0]
        hidden = shape(f"model.{first}.block.1")[0]
        dimension, _, last_k = shape(f"model.{convs[-1]}")
        self = cls(channels=channels, dimension=dimension, n_filters=n_filters, n_residual_layers=len(res) // len(strided), ratios=ratios,
                   norm=norm, kernel_size=kernel_size, last_kernel_size=last_k, residual_kernel_size=shape(f"model.{first}.block.1")[2],
                   compress=n_filters // hidden, lstm=lstm, **kw)
        self.load_state_dict(sd)
        return self.eval()

    def _build_ops(self):
        f = lambda t: t.detach().float().contiguous()
        first = self.model[0]
        ops = [dict(op="conv0", w=f(first.inner.folded()[:, 0, :]), b=f(first.inner.bias), nf=first.cout, k=first.k)]
        elu = False  # an nn.ELU in the list activates the input of the convolution behind it
        for m in list(self.model)[1:]:
            if isinstance(m, nn.ELU):
                elu = True
            elif isinstance(m, _Resnet):
                ops += self._resnet_ops(m)
                elu = False
            elif isinstance(m, _SLSTM):
                ops.append(self._lstm_op(m))
                elu = False
            else:
                ops.append(self._conv_op(m, elu, out_f32=m is self.model[-1]))
                elu = False
        return ops

    def frame_lens(self, sample_lens):
        """frames() of each length, the ceil chain over reversed(ratios): a list, a CPU tensor or a device tensor; the same kind back"""
        def chain(l):
            for r in reversed(self.ratios):
                l = (l + (r - 1)) // r
            return l
        return map_lens(sample_lens, chain)

    def forward(self, audio, lens=None):
        """lens: per-row sample counts of a padded batch, 1 <= len_b <= T (a list or CPU tensor is validated, a device tensor
        clamped): row b is the row alone -- every convolution pads about the row's own length (vbx_seanet_conv0_lens /
        vbx_seanet_conv_lens; the per-layer tables are integer torch ops on the device, no host read), bit-equal to
        forward(audio[b:b+1, :len_b])[0] up to frame_lens(lens)[b] and exactly 0.0 past it."""
        if audio.ndim == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.ndim != 2 or not audio.is_floating_point():
            raise ValueError(f"SEANetEncoder takes float audio (batch, samples) or (batch, 1, samples), got {tuple(audio.shape)} {audio.dtype}")
        if audio.shape[0] < 1 or audio.shape[1] < 1:
            raise ValueError("SEANetEncoder: empty audio")
        dev = audio.device
        if lens is not None:  # checked (host values) or clamped (a device tensor) before anything else
            lens = device_lens(lens, audio.shape[0], audio.shape[1], 1, dev, "SEANetEncoder")
        if dev.type != "cuda":
            raise _lib.VbxError(f"SEANetEncoder runs only on an MI355X (gfx950) through libvbx_hip.so; the audio is on '{dev}'")
        if self.model[0].inner.bias.device != dev:
            self.to(dev)
        with torch.inference_mode():
            return self._encode(audio, lens)

    def _encode(self, audio, lens=None):
        B, L = audio.shape
        dev, st = audio.device, _lib.current_stream()
        ops = self.packed_ops()
        wave = audio.detach().to(torch.float32).contiguous()
        x = torch.empty(B, L, ops[0]["nf"], dtype=torch.float16, device=dev)
        if lens is not None:
            return self._encode_lens(wave, x, lens, ops, st)
        _lib.call("vbx_seanet_conv0_c", wave, ops[0]["w"], ops[0]["b"], x, B, L, ops[0]["nf"], ops[0]["k"], int(self.causal), st)
        kept = None
        for op in ops[1:]:
            if op["op"] == "lstm":
                x = self.lstm_forward(op, x, B, L, st)
                continue
            Lout = -(-L // op["stride"])
            y = torch.empty(B, Lout, op["Co"], dtype=torch.float32 if op["out_f32"] else torch.float16, device=dev)
            if op["op"] == "tail":
                self._conv(op, x, kept, y, B, L, st)
            else:
                self._conv(op, x, None, y, B, L, st)
                if op.get("keep"):
                    kept = x
            x, L = y, Lout
        return x


    def _encode_lens(self, wave, x, lens, ops, st):
        """_encode with the rows' own lengths: `lens` int32 [B] on the device, in the units of each launch's input"""
        B, L = wave.shape
        _lib.call("vbx_seanet_conv0_lens", wave, lens, ops[0]["w"], ops[0]["b"], x, B, L, ops[0]["nf"], ops[0]["k"], int(self.causal), st)
        kept = None
        for op in ops[1:]:
            if op["op"] == "lstm":  # runs over the zero rows past a row's length too; the next convolution does not read them
                x = self.lstm_forward(op, x, B, L, st)
                continue
            Lout = -(-L // op["stride"])
            y = torch.empty(B, Lout, op["Co"], dtype=torch.float32 if op["out_f32"] else torch.float16, device=x.device)
            self._conv(op, x, kept if op["op"] == "tail" else None, y, B, L, st, lens=lens)
            if op.get("keep"):
                kept = x
            if op["stride"] > 1:
                lens = ((lens + (op["stride"] - 1)) // op["stride"]).to(torch.int32)
            x, L = y, Lout
        return x


class SEANetDecoder(_SEANet):
    """EnCodec's decoder on the device -- the network `EncodecWrapper.decode_from_codebook_indices` runs: a 7-tap convolution
    dimension -> 16 n_filters, a 2-layer LSTM with a skip, per ratio r in `ratios` (unreversed) ELU, a transposed convolution with
    kernel 2 r and stride r that halves the width, n_residual_layers Resnet blocks; ELU and a last 7-tap convolution to one channel,
    no final activation.  latents z [B, dimension, frames] (channel-first, any float dtype, on the GPU: what EnCodec's decoder and
    EncodecVocoCodec.codes_to_features use) -> wave fp32 [B, frames * prod(ratios)], the shape a VocosDecoder returns, so this is a
    `vocoder=` of EncodecVocoCodec by its call shape.  The parameters carry the published names and shapes
    (`model.{i}.convtr.convtr.weight_g` [Cin, 1, 1], `weight_v` [Cin, Cout, k] ...), so the `decoder.*` part of an EnCodec state dict
    loads as is.

    PARITY UNPINNED, as for the encoder: the `encodec` library is not a dependency and no fixture of it exists; the yardstick is the
    fp64 restatement tests/seanet_dec_ref.py (tests/test_seanet_dec_gpu.py, profiles/seanet_dec_parity.txt).

    Device path: vbx_seanet_pack_latents (one rounding to fp16, channel-last), vbx_seanet_conv for the first convolution and the
    Resnet blocks, SEANetEncoder.lstm_forward, vbx_seanet_convtr per stage (one product over [a_j | a_{j-1}] with the phase-packed
    weight), vbx_seanet_conv_out; no host synchronisation, the precision contract of include/vbx.h.  Inference only, eval semantics;
    weights are folded in fp32 and packed once per parameter version (mark_weights_dirty() after a write through `p.data`).

    Raises NotImplementedError for what SEANetEncoder refuses (same keywords, same ranges), for final_activation other than None
    and trim_right_ratio != 1.0 (causal=True and trim_right_ratio are served by CausalSEANetDecoder, not here), and for any layer without a tile in its kernel (none inside these ranges).  GPU tensors only; a
    forward on a device other than the parameters' MOVES THE MODULE there -- keep one instance per device."""

    _HALF = "decoder"

    def __init__(self, channels=1, dimension=128, n_filters=32, n_residual_layers=1, ratios=(8, 5, 4, 2), activation="ELU",
                 activation_params=None, final_activation=None, final_activation_params=None, norm="weight_norm", kernel_size=7,
                 last_kernel_size=7, residual_kernel_size=3, dilation_base=2, causal=False, pad_mode="reflect", true_skip=False,
                 compress=2, lstm=2, trim_right_ratio=1.0):
        super().__init__()
        ratios = tuple(int(r) for r in ratios)
        no = _check_keywords("SEANetDecoder", channels, dimension, n_filters, n_residual_layers, ratios, activation, activation_params, norm,
                             kernel_size, last_kernel_size, residual_kernel_size, dilation_base, causal, pad_mode, true_skip, compress, lstm,
                             causal_class=self._CAUSAL)
        if final_activation is not None:
            raise no(f"final_activation={final_activation!r} (only None)")
        if self._CAUSAL:
            if not 0.0 <= float(trim_right_ratio) <= 1.0:
                raise ValueError(f"{self._CAUSAL}: trim_right_ratio must be in [0, 1] (got {trim_right_ratio})")
        elif float(trim_right_ratio) != 1.0:
            raise no(f"trim_right_ratio={trim_right_ratio} (only 1.0; it matters for causal=True alone: use CausalSEANetDecoder)")
        self.causal, self.trim_right_ratio = bool(causal), float(trim_right_ratio)
        self.channels, self.dimension, self.n_filters, self.n_residual_layers, self.ratios = channels, dimension, n_filters, n_residual_layers, ratios
        self.norm, self.kernel_size, self.last_kernel_size, self.residual_kernel_size = norm, kernel_size, last_kernel_size, residual_kernel_size
        self.dilation_base, self.compress, self.lstm = dilation_base, compress, lstm
        self.hop_length = math.prod(ratios)
        d = n_filters * 2 ** len(ratios)
        self.hidden = d
        model = [_SConv(dimension, d, kernel_size, norm)]
        if lstm:
            model.append(_SLSTM(d, lstm))
        for r in ratios:
            model += [nn.ELU(), _SConvTr(d, d // 2, r, norm)]
            d //= 2
            for j in range(n_residual_layers):
                model.append(_Resnet(d, compress, residual_kernel_size, dilation_base ** j, norm))
        model += [nn.ELU(), _SConv(d, channels, last_kernel_size, norm)]
        self.model = nn.ModuleList(model)
        self._check_tiles(no)

    @classmethod
    def from_state_dict(cls, sd, **kw):
        """A state dict already in memory, in any of the three layouts.  The widths are read off the shapes; the ratios off the
        transposed kernels (k = 2 r); reflect padding and ELU are taken as given.  A state dict CANNOT say whether its network is
        causal: SEANetDecoder.from_state_dict builds the non-causal network, CausalSEANetDecoder.from_state_dict the causal one
        (what the published `encodec_24khz` file needs).  **kw: constructor keywords the shapes do not tell (trim_right_ratio)."""
        sd = cls._canonical(sd)
        idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("model.")})
        norm = "weight_norm" if "model.0.conv.conv.weight_g" in sd else "none"
        wkey = "weight_v" if norm == "weight_norm" else "weight"
        shape = lambda name, kind="conv": tuple(sd[f"{name}.{kind}.{kind}.{wkey}"].shape)
        res = [i for i in idx if f"model.{i}.shortcut.conv.conv.bias" in sd]
        lstm_i = [i for i in idx if f"model.{i}.lstm.weight_ih_l0" in sd]
        convs = [i for i in idx if f"model.{i}.conv.conv.bias" in sd]
        trs = [i for i in idx if f"model.{i}.convtr.convtr.bias" in sd]
        if len(convs) != 2 or not trs or not res or len(res) % len(trs):
            raise RuntimeError("SEANetDecoder.from_state_dict: not a SEANet decoder layout (transposed convolutions and Resnet blocks)")
        _, dimension, kernel_size = shape("model.0")
        channels, n_filters, last_k = shape(f"model.{convs[-1]}")
        ratios = tuple(shape(f"model.{i}", "convtr")[2] // 2 for i in trs)
        lstm = 0 if not lstm_i else 1 + max(int(k[-1]) for k in sd if k.startswith(f"model.{lstm_i[0]}.lstm.weight_ih_l"))
        hidden, dim, res_k = shape(f"model.{res[0]}.block.1")
        self = cls(channels=channels, dimension=dimension, n_filters=n_filters, n_residual_layers=len(res) // len(trs), ratios=ratios,
                   norm=norm, kernel_size=kernel_size, last_kernel_size=last_k, residual_kernel_size=res_k, compress=dim // hidden, lstm=lstm,
                   **kw)
        self.load_state_dict(sd)
        return self.eval()

    @staticmethod
    def _convtr_weight(w, r):
        """folded fp32 [C, Co, 2r] -> fp32 [r * Co, 2C]: row p * Co + o = [W[:, o, p] | W[:, o, p + r]], the two input frames under
        phase p of an output run"""
        t = w.permute(2, 1, 0)  # [2r, Co, C]
        return torch.cat([t[:r].reshape(-1, w.shape[0]), t[r:].reshape(-1, w.shape[0])], dim=1)

    def trim_left(self, stride):
        """what a transposed convolution of this stride cuts in FRONT of its padding_total = stride surplus samples: the larger half
        in the non-causal network; padding_total - ceil(padding_total * trim_right_ratio) in the causal one (0 at the ratio 1.0)"""
        if not self.causal:
            return stride - stride // 2
        return stride - math.ceil(stride * self.trim_right_ratio)

    def _build_ops(self):
        f = lambda t: t.detach().float().contiguous()
        ops, last = [self._conv_op(self.model[0], False)], self.model[-1]
        for m in list(self.model)[1:-1]:
            if isinstance(m, _SLSTM):
                ops.append(self._lstm_op(m))
            elif isinstance(m, _SConvTr):  # the nn.ELU in front of it is applied as the kernel stages its input
                ops.append(dict(op="convtr", w=self._convtr_weight(m.inner.folded(), m.stride).half().contiguous(), b=f(m.inner.bias), C=m.cin,
                                Co=m.cout, stride=m.stride))
            elif isinstance(m, _Resnet):
                ops += self._resnet_ops(m)
        ops.append(dict(op="conv_out", w=f(last.inner.folded()[0].t()), b=f(last.inner.bias), nf=last.cin, k=last.k))  # fp32 [k, nf]
        return ops

    def forward(self, z):
        if z.ndim != 3 or z.shape[1] != self.dimension or not z.is_floating_point():
            raise ValueError(f"SEANetDecoder takes float latents (batch, {self.dimension}, frames), got {tuple(z.shape)} {z.dtype}")
        if z.shape[0] < 1 or z.shape[2] < 1:
            raise ValueError("SEANetDecoder: empty latents")
        dev = z.device
        if dev.type != "cuda":
            raise _lib.VbxError(f"SEANetDecoder runs only on an MI355X (gfx950) through libvbx_hip.so; the latents are on '{dev}'")
        if self.model[0].inner.bias.device != dev:
            self.to(dev)
        with torch.inference_mode():
            return self._decode(z)

    def _decode(self, z):
        B, D, L = z.shape
        dev, st = z.device, _lib.current_stream()
        ops = self.packed_ops()
        f16 = lambda *s: torch.empty(*s, dtype=torch.float16, device=dev)
        z32 = z.detach().to(torch.float32).contiguous()
        x = f16(B, L, D)
        _lib.call("vbx_seanet_pack_latents", z32, x, B, D, L, st)
        kept = None
        for op in ops:
            if op["op"] == "lstm":
                x = self.lstm_forward(op, x, B, L, st)
            elif op["op"] == "convtr":
                y = f16(B, L * op["stride"], op["Co"])
                _lib.call("vbx_seanet_convtr_t", x, op["w"], op["b"], y, B, L, op["C"], op["stride"], self.trim_left(op["stride"]), st)
                x, L = y, L * op["stride"]
            elif op["op"] == "conv_out":
                y = torch.empty(B, L, dtype=torch.float32, device=dev)
                _lib.call("vbx_seanet_conv_out_c", x, op["w"], op["b"], y, B, L, op["nf"], op["k"], int(self.causal), st)
                x = y
            else:
                y = f16(B, L, op["Co"])
                self._conv(op, x, kept if op["op"] == "tail" else None, y, B, L, st)
                if op.get("keep"):
                    kept = x
                x = y
        return x


class CausalSEANetEncoder(SEANetEncoder):
    """SEANetEncoder in EnCodec's causal form -- what the PUBLISHED 24 kHz model (`encodec_24khz`) is built with.  Every SConv1d pads
    all of padding_total = k_eff - stride on the left and only `extra` on the right (reflect, pad1d's short-input rule at max pad =
    max(padding_total, extra)); the LSTM is unidirectional in either form; layers, state-dict keys, the three layouts, the limits
    and the precision contract are SEANetEncoder's.  The state dict of a causal and of a non-causal model cannot be told apart,
    so the caller chooses the class; a causal model loaded into SEANetEncoder runs, silently, as a different network.

    `causal` defaults to True; causal=False raises ValueError (that network is SEANetEncoder).  Causal in EnCodec's sense: frame f
    reads no sample behind its own hop, except that the FIRST frames also read the reflection of the samples just after the
    start.  Same kernels, through vbx_seanet_conv0_c / vbx_seanet_conv_c (include/vbx.h).  PARITY with the `encodec` library is
    UNPINNED here as well; the yardstick is tests/seanet_causal_ref.py."""

    _CAUSAL = "CausalSEANetEncoder"

    def __init__(self, channels=1, dimension=128, n_filters=32, n_residual_layers=1, ratios=(8, 5, 4, 2), activation="ELU",
                 activation_params=None, norm="weight_norm", kernel_size=7, last_kernel_size=7, residual_kernel_size=3,
                 dilation_base=2, causal=True, pad_mode="reflect", true_skip=False, compress=2, lstm=2):
        super().__init__(channels, dimension, n_filters, n_residual_layers, ratios, activation, activation_params, norm, kernel_size,
                         last_kernel_size, residual_kernel_size, dilation_base, causal, pad_mode, true_skip, compress, lstm)


class CausalSEANetDecoder(SEANetDecoder):
    """SEANetDecoder in EnCodec's causal form -- what the PUBLISHED 24 kHz model is built with.  Its convolutions pad as
    CausalSEANetEncoder's; each SConvTranspose1d trims padding_right = ceil(padding_total * trim_right_ratio) samples behind and
    padding_total - padding_right in front (padding_total = stride): at the published ratio 1.0 nothing in front, the first
    L * stride untrimmed samples are the output.  trim_right_ratio may be anything in [0, 1] (ValueError outside).  `causal`
    defaults to True; causal=False raises ValueError (that network is SEANetDecoder).  Everything else -- layers, keys, layouts,
    limits, the precision contract -- is SEANetDecoder's; the same kernels through vbx_seanet_conv_c / vbx_seanet_convtr_t /
    vbx_seanet_conv_out_c.  PARITY with the `encodec` library is UNPINNED; the yardstick is tests/seanet_causal_ref.py."""

    _CAUSAL = "CausalSEANetDecoder"

    def __init__(self, channels=1, dimension=128, n_filters=32, n_residual_layers=1, ratios=(8, 5, 4, 2), activation="ELU",
                 activation_params=None, final_activation=None, final_activation_params=None, norm="weight_norm", kernel_size=7,
                 last_kernel_size=7, residual_kernel_size=3, dilation_base=2, causal=True, pad_mode="reflect", true_skip=False,
                 compress=2, lstm=2, trim_right_ratio=1.0):
        super().__init__(channels, dimension, n_filters, n_residual_layers, ratios, activation, activation_params, final_activation,
                         final_activation_params, norm, kernel_size, last_kernel_size, residual_kernel_size, dilation_base, causal,
                         pad_mode, true_skip, compress, lstm, trim_right_ratio)
