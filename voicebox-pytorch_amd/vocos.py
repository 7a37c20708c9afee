"""VocosDecoder: the decoder half of a Vocos vocoder (Siuzdak 2023, "Vocos: closing the gap between time-domain and Fourier-based
neural vocoders") on the device -- the network the reference's MelVoco.decode calls as `self.vocos.decode(mel)`
(voicebox_pytorch.py:543-549).  A 7-tap input convolution, ConvNeXt blocks (depthwise 7-tap convolution, LayerNorm, Linear, erf-GELU,
Linear, layer scale, residual), a linear head that predicts log-magnitude and phase, one inverse STFT.  The parameters carry the
names and shapes of the published model, so a Vocos state dict loads as is; neither the `vocos` library nor any weights are part of
this package, and nothing here reaches a hub: from_checkpoint reads a local file.

PARITY UNPINNED: the `vocos` library is not a dependency and no fixture of it exists.  This follows its published arithmetic
(VocosBackbone, ConvNeXtBlock, ISTFTHead at padding="center"), restated in fp64 with F.conv1d / F.layer_norm / F.gelu / torch.istft
in tests/vocos_ref.py; the kernels are tested against that restatement (tests/test_vocos_gpu.py, profiles/vocos_parity.txt).

Device path (csrc/vocos.hip, csrc/gemm.hip, csrc/griffinlim.hip): a fixed launch sequence without host synchronisation.  The GEMM
operands are fp16 (weights packed once per parameter version, the layer scale gamma folded into pwconv2 in fp32 before the rounding:
gamma * (W g + b) = (gamma * W) g + gamma * b); the residual stream, LayerNorm, the head's exp / sin / cos and the inverse STFT are
fp32.  Inference only.

VocosEncodecDecoder is the EnCodec-conditioned variant as the published `vocos-encodec-24khz` file holds it: AdaLayerNorm tables kept
whole (the bandwidth id is chosen per call), n_fft 1280 (a mixed-radix inverse transform, csrc/fft_lds.hpp) and Vocos's
padding="same" inverse STFT (vbx_istft_trim), frames * hop_length samples.  PARITY UNPINNED likewise; tests/vocos_same_ref.py
restates it, tests/test_vocos_encodec_gpu.py and profiles/vocos_encodec_parity.txt hold the kernels against that.
"""
import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights, read_checkpoint, tensors_key  # read_checkpoint: importable from here as before
from .codec import _check_istft_args, _stft_tables, ola_reciprocal_envelope, ola_reciprocal_envelope_trim

LN_EPS = 1e-6


class _AdaLayerNorm(nn.Module):
    """Vocos's AdaLayerNorm: layer_norm(x) * scale[id] + shift[id], two embedding tables [num_embeddings, dim] (ones / zeros)"""

    def __init__(self, num_embeddings, dim):
        super().__init__()
        self.scale = nn.Embedding(num_embeddings, dim)
        self.shift = nn.Embedding(num_embeddings, dim)
        nn.init.ones_(self.scale.weight)
        nn.init.zeros_(self.shift.weight)


def _norm(dim, adanorm):
    return nn.LayerNorm(dim, eps=LN_EPS) if adanorm is None else _AdaLayerNorm(adanorm, dim)


def _norm_tables(norm):
    """fp32 (weight, bias) [dim] of a LayerNorm, or the (scale, shift) tables [num_embeddings, dim] of an _AdaLayerNorm"""
    w, b = (norm.scale.weight, norm.shift.weight) if isinstance(norm, _AdaLayerNorm) else (norm.weight, norm.bias)
    return w.detach().float().contiguous(), b.detach().float().contiguous()


class _ConvNeXtBlock(nn.Module):
    def __init__(self, dim, intermediate_dim, gamma0, adanorm=None):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = _norm(dim, adanorm)
        self.pwconv1 = nn.Linear(dim, intermediate_dim)
        self.pwconv2 = nn.Linear(intermediate_dim, dim)
        self.gamma = nn.Parameter(gamma0 * torch.ones(dim))


class _Backbone(nn.Module):
    def __init__(self, input_channels, dim, intermediate_dim, num_layers, gamma0, adanorm=None):
        super().__init__()
        self.embed = nn.Conv1d(input_channels, dim, kernel_size=7, padding=3)
        self.norm = _norm(dim, adanorm)
        self.convnext = nn.ModuleList([_ConvNeXtBlock(dim, intermediate_dim, gamma0, adanorm) for _ in range(num_layers)])
        self.final_layer_norm = nn.LayerNorm(dim, eps=LN_EPS)


class _ISTFT(nn.Module):
    def __init__(self, n_fft):
        super().__init__()
        self.register_buffer("window", torch.hann_window(n_fft, periodic=True))


class _Head(nn.Module):
    def __init__(self, dim, n_fft):
        super().__init__()
        self.out = nn.Linear(dim, n_fft + 2)
        self.istft = _ISTFT(n_fft)


class VocosDecoder(PackedWeights, nn.Module):
    """features [B, input_channels, frames] -> wave fp32 [B, (frames - 1) * hop_length].  forward = decode = Vocos.decode: the
    features are taken as given unless input_log, which applies log(clamp(x, min=1e-7)) first -- what Vocos's own mel feature
    extractor feeds its backbone (the published vocos-mel-24khz weights expect it, at hop_length 256).

    Raises NotImplementedError for what this class does not serve: padding="same" and adanorm_num_embeddings (the EnCodec-conditioned
    variant as a module: both are VocosEncodecDecoder's; from_checkpoint(bandwidth_id=...) here loads such a checkpoint folded to
    ONE fixed id), n_fft outside the powers of two 256 .. 2048 and 320 / 640 / 1280, dim not a multiple of 64 or above 2048, intermediate_dim not a multiple of 8,
    input_channels above 512, fewer than two frames, a hop / n_fft pair beyond the LDS of the inverse transform; ValueError, as
    ola_reciprocal_envelope, where window and hop violate NOLA.  GPU tensors only."""

    def __init__(self, input_channels=100, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256, padding="center",
                 layer_scale_init_value=None, input_log=False, adanorm_num_embeddings=None):
        super().__init__()
        if padding != "center":
            raise NotImplementedError(f'VocosDecoder: padding="{padding}" is not built here (only "center", torch.istft with center=True); '
                                      'VocosEncodecDecoder serves padding="same"')
        if adanorm_num_embeddings is not None:
            raise NotImplementedError("VocosDecoder: adanorm_num_embeddings (the EnCodec-conditioned AdaLayerNorm variant) is not built "
                                      "here; VocosEncodecDecoder keeps the tables")
        self._setup(input_channels, dim, intermediate_dim, num_layers, n_fft, hop_length, padding, layer_scale_init_value, input_log, None)

    def _setup(self, input_channels, dim, intermediate_dim, num_layers, n_fft, hop_length, padding, layer_scale_init_value, input_log,
               adanorm_num_embeddings):
        _check_istft_args(n_fft, n_fft, hop_length)
        if dim <= 0 or dim % 64 or dim > 2048:
            raise NotImplementedError(f"VocosDecoder: dim must be a multiple of 64, at most 2048 (got {dim})")
        if intermediate_dim <= 0 or intermediate_dim % 8:
            raise NotImplementedError(f"VocosDecoder: intermediate_dim must be a multiple of 8 (got {intermediate_dim})")
        if not 0 < input_channels <= 512:
            raise NotImplementedError(f"VocosDecoder: input_channels must be in 1 .. 512 (got {input_channels})")
        if num_layers < 1:
            raise ValueError("need num_layers >= 1")
        self.input_channels, self.dim, self.intermediate_dim, self.num_layers = input_channels, dim, intermediate_dim, num_layers
        self.n_fft, self.hop_length, self.padding, self.input_log = n_fft, hop_length, padding, bool(input_log)
        self.adanorm_num_embeddings = adanorm_num_embeddings
        self.backbone = _Backbone(input_channels, dim, intermediate_dim, num_layers, layer_scale_init_value or 1.0 / num_layers,
                                  adanorm_num_embeddings)
        self.head = _Head(dim, n_fft)
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
        self._tables, self._tables_key = None, None

    # -- state
    def load_state_dict(self, state_dict, strict=True, **kw):
        kept = {k: v for k, v in state_dict.items() if not k.startswith("feature_extractor.")}
        return super().load_state_dict(kept, strict=strict, **kw)

    @staticmethod
    def _fold_adanorm(sd, bandwidth_id):
        """The EnCodec-conditioned variant's AdaLayerNorm is layer_norm(x) * scale[id] + shift[id] with one id per call: for a
        fixed id, a plain LayerNorm whose weight / bias are row `id` of the two embedding tables."""
        out = {}
        for k, v in sd.items():
            for emb, name in ((".scale.weight", ".weight"), (".shift.weight", ".bias")):
                if k.startswith("backbone.") and k.endswith(".norm" + emb):
                    if not 0 <= bandwidth_id < v.shape[0]:
                        raise ValueError(f"VocosDecoder: bandwidth_id {bandwidth_id} is outside the {v.shape[0]} rows of {k}")
                    k, v = k[:-len(emb)] + name, v[bandwidth_id].clone()
            out[k] = v
        return out

    @classmethod
    def from_checkpoint(cls, path, *, hop_length=None, input_log=False, padding="center", bandwidth_id=None):
        """A LOCAL file written by torch.save: a Vocos state dict or {'state_dict': ...}; see from_state_dict."""
        return cls.from_state_dict(read_checkpoint(path), hop_length=hop_length, input_log=input_log, padding=padding,
                                   bandwidth_id=bandwidth_id)

    @classmethod
    def from_state_dict(cls, sd, *, hop_length=None, input_log=False, padding="center", bandwidth_id=None):
        """A Vocos state dict already in memory.  The widths are read off the shapes; hop_length is not in a state dict (default n_fft / 4, the published models' ratio).  bandwidth_id: for the
        EnCodec-conditioned variant (backbone.norm.scale / .shift embeddings), the one id this decoder is built for; its rows
        become the LayerNorm weights.  Without it such a dict raises NotImplementedError."""
        if any(k.startswith("backbone.norm.scale") or k.startswith("backbone.norm.shift") for k in sd):
            if bandwidth_id is None:
                raise NotImplementedError("VocosDecoder: adanorm_num_embeddings (the EnCodec-conditioned AdaLayerNorm variant) is not built "
                                          "here: pass bandwidth_id= for one fixed id, or load the file into a VocosEncodecDecoder")
            sd = cls._fold_adanorm(sd, int(bandwidth_id))
        dim, channels, _ = sd["backbone.embed.weight"].shape
        layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("backbone.convnext."))
        n_fft = sd["head.out.weight"].shape[0] - 2
        self = cls(input_channels=channels, dim=dim, intermediate_dim=sd["backbone.convnext.0.pwconv1.weight"].shape[0],
                   num_layers=layers, n_fft=n_fft, hop_length=hop_length or n_fft // 4, padding=padding, input_log=input_log)
        self.load_state_dict(sd)
        return self.eval()

    # -- operand copies
    def _pack(self):
        """fp16 GEMM operands and fp32 vectors as the launch sequence reads them; kept per parameter version (PackedWeights)"""
        bb, C, D = self.backbone, self.input_channels, self.dim
        f = lambda t: t.detach().float().contiguous()
        Kp = _lib.lib().vbx_vocos_kp(C)
        emb = torch.zeros(D, Kp, dtype=torch.float32, device=bb.embed.weight.device)
        emb[:, :7 * C] = bb.embed.weight.detach().float().permute(0, 2, 1).reshape(D, 7 * C)  # column tap * C + c
        nh = self.n_fft + 2
        nhp = (nh + 7) // 8 * 8  # vbx_gemm: N in whole 16-byte pieces; the pad rows are zero and never read
        hw = torch.zeros(nhp, D, dtype=torch.float32, device=emb.device)
        hw[:nh] = self.head.out.weight.detach().float()
        hb = torch.zeros(nhp, dtype=torch.float32, device=emb.device)
        hb[:nh] = self.head.out.bias.detach().float()
        layers = []
        for blk in bb.convnext:
            g = blk.gamma.detach().float()
            lnw, lnb = _norm_tables(blk.norm)
            layers.append(dict(
                taps=blk.dwconv.weight.detach().float()[:, 0, :].t().contiguous(),  # [7, D]
                cb=f(blk.dwconv.bias), lnw=lnw, lnb=lnb,
                w1=blk.pwconv1.weight.detach().float().half().contiguous(), b1=f(blk.pwconv1.bias),
                w2=(g[:, None] * blk.pwconv2.weight.detach().float()).half().contiguous(), b2=(g * blk.pwconv2.bias.detach().float()).contiguous()))
        n0w, n0b = _norm_tables(bb.norm)
        return dict(Kp=Kp, nhp=nhp, emb=emb.half(), emb_b=f(bb.embed.bias), n0w=n0w, n0b=n0b, layers=layers,
                    flw=f(bb.final_layer_norm.weight), flb=f(bb.final_layer_norm.bias), hw=hw.half(), hb=hb)

    def _istft_tables(self, frames, device):
        """window, twiddles and the reciprocal window-square envelope of the kept range, from the `head.istft.window` buffer
        (ValueError where it and hop_length violate NOLA, as torch.istft)"""
        win = self.head.istft.window
        key = (frames, str(device), tensors_key((win,)))
        if key != self._tables_key:
            win = win.detach().double().cpu()
            renv = self._reciprocal_envelope(frames, win)
            _, tw_re, tw_im = _stft_tables(self.n_fft, self.n_fft)
            self._tables = tuple(t.float().to(device) for t in (win, tw_re, tw_im, renv))
            self._tables_key = key
        return self._tables

    def _reciprocal_envelope(self, frames, win):
        return ola_reciprocal_envelope(self.n_fft, self.n_fft, self.hop_length, frames, window=win)

    @staticmethod
    def _gemm(epi, M, N, K, A, B, C, ldc, bias, resid=None):
        d = _lib.GemmDesc()
        d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16 = _lib.VBX_GEMM_NT, epi, M, N, K, K, K, ldc, 1
        d.A, d.B, d.C, d.bias = A.data_ptr(), B.data_ptr(), C.data_ptr(), bias.data_ptr()
        d.resid = None if resid is None else resid.data_ptr()
        rc = _lib.lib().vbx_gemm(d, _lib.current_stream())
        if rc != 0:
            raise _lib.VbxError(f"vbx_gemm failed (rc={rc}): {_lib.lib().vbx_last_error().decode()}")

    def forward(self, features):
        if features.ndim != 3 or features.shape[1] != self.input_channels:
            raise ValueError(f"VocosDecoder takes features (batch, input_channels = {self.input_channels}, frames), got {tuple(features.shape)}")
        frames, dev = features.shape[2], features.device
        if frames < 2:
            raise NotImplementedError(f"VocosDecoder: the inverse STFT needs at least two frames (got {frames})")
        if _lib.lib().vbx_griffinlim_lds_bytes(self.n_fft, self.n_fft, self.hop_length) > 65536:
            raise NotImplementedError(f"VocosDecoder: 3 * hop_length + n_fft = {3 * self.hop_length + self.n_fft} samples do not fit the "
                                      f"LDS beside a {self.n_fft}-point transform")
        if dev.type == "cuda" and self.head.out.weight.device != dev:
            self.to(dev)
        tables = self._istft_tables(frames, dev)  # ValueError: NOLA
        if dev.type != "cuda":
            raise _lib.VbxError(f"VocosDecoder runs only on an MI355X (gfx950) through libvbx_hip.so; the features are on '{dev}'")
        with torch.inference_mode():
            return self._decode(features, tables)

    def _decode(self, features, tables, norm_id=None):
        """norm_id: the row of the AdaLayerNorm tables the LayerNorm kernels read as weight / bias (None: plain LayerNorms)"""
        B, C, frames = features.shape
        n_fft, hop, D, I, dev = self.n_fft, self.hop_length, self.dim, self.intermediate_dim, features.device
        w = self._cached(self._pack)
        row = (lambda t: t) if norm_id is None else (lambda t: t[norm_id])
        st = _lib.current_stream()
        M, Kp, nhp, nb = B * frames, w["Kp"], w["nhp"], n_fft // 2 + 1
        x = features.detach().to(torch.float32).contiguous()
        f16 = lambda *s: torch.empty(*s, dtype=torch.float16, device=dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        a16 = f16(M, Kp)
        _lib.call("vbx_vocos_pack_input", x, a16, B, C, frames, int(self.input_log), st)
        xa, xb = f32(M, D), f32(M, D)  # the residual stream ping-pongs: pwconv2 reads one as `resid` and writes the other
        self._gemm(_lib.VBX_EPI_F32, M, D, Kp, a16, w["emb"], xb, D, w["emb_b"])
        _lib.call("vbx_layernorm_fwd", xb, row(w["n0w"]), row(w["n0b"]), None, xa, M, D, LN_EPS, st)
        h16, g16 = f16(M, D), f16(M, I)
        for l in w["layers"]:
            _lib.call("vbx_vocos_dwconv_ln", xa, l["taps"], l["cb"], row(l["lnw"]), row(l["lnb"]), h16, B, frames, D, LN_EPS, st)
            self._gemm(_lib.VBX_EPI_GELU, M, I, D, h16, l["w1"], g16, I, l["b1"])
            self._gemm(_lib.VBX_EPI_F32, M, D, I, g16, l["w2"], xb, D, l["b2"], resid=xa)
            xa, xb = xb, xa
        _lib.call("vbx_vocos_dwconv_ln", xa, None, None, w["flw"], w["flb"], h16, B, frames, D, LN_EPS, st)
        ho = f32(M, nhp)
        self._gemm(_lib.VBX_EPI_F32, M, nhp, D, h16, w["hw"], ho, nhp, w["hb"])
        mag, ph = f32(B, frames, nb), f32(B, frames, nb, 2)
        _lib.call("vbx_vocos_head", ho, mag, ph, M, nb, nhp, st)
        return self._istft(mag, ph, f32(B, frames, n_fft), tables, st)

    def _istft(self, mag, ph, fb, tables, st):
        B, frames, n_fft, hop = fb.shape[0], fb.shape[1], self.n_fft, self.hop_length
        window, tw_re, tw_im, renv = tables
        wave = torch.empty(B, (frames - 1) * hop, dtype=torch.float32, device=fb.device)
        _lib.call("vbx_istft", mag, ph, fb, wave, window, tw_re, tw_im, renv, B, frames, n_fft, n_fft, hop, st)
        return wave

    decode = forward


class VocosEncodecDecoder(VocosDecoder):
    """The EnCodec-conditioned Vocos decoder with its AdaLayerNorm tables kept and Vocos's padding="same" inverse STFT; the defaults
    are the published `vocos-encodec-24khz` configuration, whose state dict loads as is (`backbone.norm.scale.weight` /
    `.shift.weight` [adanorm_num_embeddings, dim], the same per block, a plain `backbone.final_layer_norm`; `feature_extractor.*` is
    skipped).

    forward(features [B, input_channels, frames], bandwidth_id=None) -> wave fp32 [B, frames * hop_length] at "same" (in general
    (frames - 1) * hop + n_fft - 2 * ((n_fft - hop) // 2); one frame is enough), [B, (frames - 1) * hop_length] at "center".  Every
    AdaLayerNorm is layer_norm(x) * scale[id] + shift[id]: the LayerNorm kernels of VocosDecoder reading row `id` of the packed fp32
    tables, so a decoder folded to that id (VocosDecoder.from_state_dict(bandwidth_id=id)) gives the same bits.  bandwidth_id is a
    Python int (None: the constructor's); it is never read from a device tensor.  adanorm_num_embeddings=None builds plain
    LayerNorms: a "same"-padded Vocos.

    "same" is Vocos's ISTFT: irfft per frame (imaginary DC / Nyquist ignored), times the window, overlap-add, (n_fft - hop) // 2
    samples trimmed from each end, divided by the window-square envelope of the kept range (ValueError "NOLA" where it is <= 1e-11).
    The other limits are VocosDecoder's."""

    def __init__(self, input_channels=128, dim=384, intermediate_dim=1152, num_layers=8, n_fft=1280, hop_length=320, padding="same",
                 adanorm_num_embeddings=4, bandwidth_id=2, layer_scale_init_value=None, input_log=False):
        nn.Module.__init__(self)
        if padding not in ("same", "center"):
            raise ValueError(f'VocosEncodecDecoder: padding must be "same" or "center" (got "{padding}")')
        if adanorm_num_embeddings is not None:
            if adanorm_num_embeddings < 1:
                raise ValueError("need adanorm_num_embeddings >= 1, or None for plain LayerNorms")
            self._check_id(bandwidth_id, adanorm_num_embeddings)
        self._setup(input_channels, dim, intermediate_dim, num_layers, n_fft, hop_length, padding, layer_scale_init_value, input_log,
                    adanorm_num_embeddings)
        self.bandwidth_id = bandwidth_id if adanorm_num_embeddings is not None else None

    @staticmethod
    def _check_id(bandwidth_id, rows):
        if isinstance(bandwidth_id, torch.Tensor) or not isinstance(bandwidth_id, int):
            raise TypeError(f"VocosEncodecDecoder: bandwidth_id is a Python int (got {type(bandwidth_id).__name__}); it is never read "
                            "from a tensor")
        if not 0 <= bandwidth_id < rows:
            raise ValueError(f"VocosEncodecDecoder: bandwidth_id {bandwidth_id} is outside the {rows} rows of the AdaLayerNorm tables")

    @classmethod
    def from_checkpoint(cls, path, *, hop_length=None, input_log=False, padding="same", bandwidth_id=2):
        """A LOCAL file written by torch.save: a Vocos state dict or {'state_dict': ...}; see from_state_dict."""
        return cls.from_state_dict(read_checkpoint(path), hop_length=hop_length, input_log=input_log, padding=padding,
                                   bandwidth_id=bandwidth_id)

    @classmethod
    def from_state_dict(cls, sd, *, hop_length=None, input_log=False, padding="same", bandwidth_id=2):
        """A Vocos state dict already in memory, loaded as is.  The widths and the number of AdaLayerNorm rows are read off the
        shapes (a dict without `backbone.norm.scale.weight` gives plain LayerNorms, and bandwidth_id is ignored); hop_length is not
        in a state dict (default n_fft / 4).  bandwidth_id is the default id of forward."""
        dim, channels, _ = sd["backbone.embed.weight"].shape
        layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("backbone.convnext."))
        n_fft = sd["head.out.weight"].shape[0] - 2
        rows = sd["backbone.norm.scale.weight"].shape[0] if "backbone.norm.scale.weight" in sd else None
        self = cls(input_channels=channels, dim=dim, intermediate_dim=sd["backbone.convnext.0.pwconv1.weight"].shape[0],
                   num_layers=layers, n_fft=n_fft, hop_length=hop_length or n_fft // 4, padding=padding, adanorm_num_embeddings=rows,
                   bandwidth_id=bandwidth_id, input_log=input_log)
        self.load_state_dict(sd)
        return self.eval()

    def _trim(self, frames):
        """(trim, out_len) of the overlap-add's (frames - 1) * hop + n_fft samples"""
        if self.padding == "center":
            return self.n_fft // 2, (frames - 1) * self.hop_length
        trim = (self.n_fft - self.hop_length) // 2
        return trim, (frames - 1) * self.hop_length + self.n_fft - 2 * trim

    def _reciprocal_envelope(self, frames, win):
        trim, out_len = self._trim(frames)
        return ola_reciprocal_envelope_trim(self.n_fft, self.hop_length, frames, win, trim, out_len)

    def forward(self, features, bandwidth_id=None):
        if features.ndim != 3 or features.shape[1] != self.input_channels:
            raise ValueError(f"VocosEncodecDecoder takes features (batch, input_channels = {self.input_channels}, frames), got "
                             f"{tuple(features.shape)}")
        if self.adanorm_num_embeddings is None:
            if bandwidth_id is not None:
                raise ValueError("VocosEncodecDecoder: built with plain LayerNorms (adanorm_num_embeddings=None), there is no bandwidth_id")
        else:
            bandwidth_id = self.bandwidth_id if bandwidth_id is None else bandwidth_id
            self._check_id(bandwidth_id, self.adanorm_num_embeddings)
        frames, dev = features.shape[2], features.device
        if frames < 1 or self._trim(frames)[1] < 1:
            raise NotImplementedError(f'VocosEncodecDecoder: padding="{self.padding}" keeps no sample of {frames} frame(s)')
        if _lib.lib().vbx_griffinlim_lds_bytes(self.n_fft, self.n_fft, self.hop_length) > 65536:
            raise NotImplementedError(f"VocosEncodecDecoder: 3 * hop_length + n_fft = {3 * self.hop_length + self.n_fft} samples do not "
                                      f"fit the LDS beside a {self.n_fft}-point transform")
        if dev.type == "cuda" and self.head.out.weight.device != dev:
            self.to(dev)
        tables = self._istft_tables(frames, dev)  # ValueError: NOLA
        if dev.type != "cuda":
            raise _lib.VbxError(f"VocosEncodecDecoder runs only on an MI355X (gfx950) through libvbx_hip.so; the features are on '{dev}'")
        with torch.inference_mode():
            return self._decode(features, tables, bandwidth_id)

    def _istft(self, mag, ph, fb, tables, st):
        B, frames, n_fft, hop = fb.shape[0], fb.shape[1], self.n_fft, self.hop_length
        window, tw_re, tw_im, renv = tables
        trim, out_len = self._trim(frames)
        wave = torch.empty(B, out_len, dtype=torch.float32, device=fb.device)
        _lib.call("vbx_istft_trim", mag, ph, fb, wave, window, tw_re, tw_im, renv, B, frames, n_fft, n_fft, hop, trim, out_len, st)
        return wave

    decode = forward
