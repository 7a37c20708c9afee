"""HiFiGANGenerator: the generator of HiFi-GAN (Kong et al. 2020, "HiFi-GAN: generative adversarial networks for efficient and
high fidelity speech synthesis") on the device -- the vocoder most mel-trained checkpoints come with, and the one the Voicebox
paper decodes its mels with.  mel fp32 [B, n_mels, frames] -> wave fp32 [B, frames * prod(upsample_rates)] in [-1, 1]: a
`vocoder=` of LogMelCodec by its call shape.

The network: conv_pre (7 taps), per stage leaky ReLU(0.1) + ConvTranspose1d(C, C / 2, 2u, stride u, padding u / 2) + the MEAN of
num_kernels residual blocks (the multi-receptive-field fusion), then leaky ReLU at torch's DEFAULT slope 0.01 (the original calls
F.leaky_relu(x) bare there), conv_post (7 taps, one channel) and tanh.  ResBlock1 is, per dilation d, x = c2(lrelu(c1(lrelu(x)))) + x
with c1 dilated by d and c2 not; ResBlock2 is x = c(lrelu(x)) + x.  All paddings are zeros.  Weight norm is torch's default dim=0:
per OUTPUT channel for a Conv1d, per INPUT channel for a ConvTranspose1d (weight_g [Cin, 1, 1]).  The parameters carry the
published names (`conv_pre`, `ups.{i}`, `resblocks.{i * nk + j}.convs1.{m}` / `.convs2.{m}` or `.convs.{m}`, `conv_post`; each
`weight_g` / `weight_v` / `bias`), so a `generator` checkpoint loads as is; neither the library nor any weights are part of this
package, and nothing here reaches a hub: from_checkpoint reads LOCAL files.

PARITY UNPINNED: the HiFi-GAN library is not a dependency and no fixture of it exists.  This follows its published arithmetic
(models.py: Generator, ResBlock1, ResBlock2), restated in fp64 with F.conv1d / F.conv_transpose1d / F.leaky_relu / torch.tanh in
tests/hifigan_ref.py; the kernels are tested against that restatement (tests/test_hifigan_gpu.py, profiles/hifigan_parity.txt).

DILATIONS.  A state dict CANNOT say its dilations: they change no shape and no key.  from_checkpoint takes them from `config=`
(HiFi-GAN's config.json, a path or a dict); without one it assumes the V1 / V2 defaults (1, 3, 5) per block for ResBlock1 and
V3's (1, 3) for ResBlock2.  A checkpoint trained with other dilations then loads without complaint and runs, silently, as a
different network.

Device path (csrc/hifigan.hip on the tile core of csrc/seanet_tile.hpp): a fixed launch sequence without host synchronisation,
under SEANet's precision contract (include/vbx.h): activations fp16 channel-last, rounded once and stored before the activation;
weights fp16, weight norm folded in fp32; sums fp32 on the matrix cores; no atomics.  Inference only.
"""
import json
import math
import os

import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights
from .seanet import SEANetDecoder

_PARAM = "parametrizations.weight.original"
LRELU_SLOPE = 0.1  # HiFi-GAN's LRELU_SLOPE; the last activation uses torch's default instead
LAST_SLOPE = 0.01

pack_convtr_weight = SEANetDecoder._convtr_weight  # folded fp32 [C, Co, 2r] -> [r * Co, 2C], row p * Co + o = [W[:, o, p] | W[:, o, p + r]]


class _WNConv(nn.Module):
    """weight_norm(nn.Conv1d) by its parameters: weight_g [Co, 1, 1] / weight_v [Co, Ci, k] / bias; after plain_(): weight / bias (a
    checkpoint saved after remove_weight_norm)"""

    transposed = False

    def __init__(self, cin, cout, k, dilation=1, stride=1):
        super().__init__()
        self.cin, self.cout, self.k, self.dilation, self.stride = cin, cout, k, dilation, stride
        ref = nn.ConvTranspose1d(cin, cout, k, stride=stride) if self.transposed else nn.Conv1d(cin, cout, k)
        w = ref.weight.detach()
        self.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).reshape(-1, 1, 1))
        self.weight_v = nn.Parameter(w.clone())
        self.bias = nn.Parameter(ref.bias.detach().clone())

    def plain_(self, plain):
        """switch between the weight_g / weight_v and the plain `weight` parametrisation, keeping the folded weight"""
        if plain == hasattr(self, "weight"):
            return
        w = self.folded()
        if plain:
            del self.weight_g, self.weight_v
            self.weight = nn.Parameter(w.clone())
        else:
            del self.weight
            self.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).reshape(-1, 1, 1))
            self.weight_v = nn.Parameter(w.clone())

    def folded(self):
        """fp32 w = g * v / |v|, the norm over all but dim 0: per output channel of a convolution [Co, Ci, k], per INPUT channel of
        a transposed one [Ci, Co, k]"""
        if hasattr(self, "weight"):
            return self.weight.detach().float()
        v = self.weight_v.detach().float()
        return self.weight_g.detach().float() * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)


class _WNConvTr(_WNConv):
    transposed = True


class _ResBlock1(nn.Module):
    def __init__(self, ch, k, dilations):
        super().__init__()
        self.convs1 = nn.ModuleList([_WNConv(ch, ch, k, d) for d in dilations])
        self.convs2 = nn.ModuleList([_WNConv(ch, ch, k, 1) for _ in dilations])


class _ResBlock2(nn.Module):
    def __init__(self, ch, k, dilations):
        super().__init__()
        self.convs = nn.ModuleList([_WNConv(ch, ch, k, d) for d in dilations])


def _read_config(config):
    if config is None or isinstance(config, dict):
        return config
    with open(os.fspath(config)) as fh:
        return json.load(fh)


class HiFiGANGenerator(PackedWeights, nn.Module):
    """mel [B, n_mels, frames] (any float dtype, on the GPU; amplitude mels with input_log=True for weights trained on log features:
    log(clamp(mel, 1e-5)) is then taken as the input is packed) -> wave fp32 [B, frames * hop_length].

    Runs without gradients, in eval semantics.  The folded fp16 weights are packed once and re-packed when a parameter's version
    counter or storage changes; after a write through `p.data` call mark_weights_dirty().

    Raises NotImplementedError, before any launch, for what is not built: n_mels outside 1 .. 512; upsample_initial_channel not a
    multiple of 16 * 2^(stages - 1) or above 1024; other than 1 .. 5 stages; a rate that is odd or outside 2 .. 8, or a kernel other
    than 2 * rate (those give frames * u + 1 samples or another phase structure); a residual kernel that is even or outside 3 .. 11;
    a dilation outside 1 .. 12; other than 1 .. 3 residual blocks per stage or 1 .. 3 dilations per block; resblock other than "1" /
    "2".  GPU tensors only (a CPU tensor raises VbxError); like its siblings, a forward on a device other than the parameters'
    MOVES THE MODULE there -- keep one instance per device.

    fuse_max_channels: residual pairs of ResBlock1 at widths up to this run as ONE launch (vbx_hifigan_respair, bit-equal to the
    two launches it replaces); the default is where it measured faster (profiles/hifigan_times.json)."""

    FUSE_MAX_CHANNELS = 64

    def __init__(self, n_mels=80, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                 resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, input_log=False):
        super().__init__()
        no = lambda what: NotImplementedError(f"HiFiGANGenerator: {what} is not built")
        rates, uks = tuple(int(r) for r in upsample_rates), tuple(int(k) for k in upsample_kernel_sizes)
        rks = tuple(int(k) for k in resblock_kernel_sizes)
        dils = tuple(tuple(int(d) for d in ds) for ds in resblock_dilation_sizes)
        resblock = str(resblock)
        if resblock not in ("1", "2"):
            raise no(f'resblock="{resblock}" (only "1" and "2")')
        if not 1 <= n_mels <= 512:
            raise no(f"n_mels={n_mels} (1 .. 512)")
        if not 1 <= len(rates) <= 5:
            raise no(f"{len(rates)} upsampling stages (1 .. 5)")
        if len(uks) != len(rates):
            raise ValueError("HiFiGANGenerator: upsample_rates and upsample_kernel_sizes differ in length")
        for u, k in zip(rates, uks):
            if u % 2 or not 2 <= u <= 8:
                raise no(f"upsample rate {u} (even, 2 .. 8)")
            if k != 2 * u:
                raise no(f"upsample kernel {k} at rate {u} (only kernel = 2 * rate)")
        c0, unit = int(upsample_initial_channel), 16 * 2 ** (len(rates) - 1)
        if c0 <= 0 or c0 % unit or c0 > 1024:
            raise no(f"upsample_initial_channel={c0} (a multiple of 16 * 2^(stages - 1) = {unit}, at most 1024)")
        if not 1 <= len(rks) <= 3:
            raise no(f"{len(rks)} residual blocks per stage (1 .. 3)")
        if len(dils) != len(rks):
            raise ValueError("HiFiGANGenerator: resblock_kernel_sizes and resblock_dilation_sizes differ in length")
        for k, ds in zip(rks, dils):
            if k % 2 == 0 or not 3 <= k <= 11:
                raise no(f"residual kernel {k} (odd, 3 .. 11)")
            if not 1 <= len(ds) <= 3:
                raise no(f"{len(ds)} dilations per residual block (1 .. 3)")
            if any(not 1 <= d <= 12 for d in ds):
                raise no(f"dilations {ds} (each 1 .. 12)")
        self.n_mels, self.upsample_initial_channel, self.upsample_rates, self.upsample_kernel_sizes = int(n_mels), c0, rates, uks
        self.resblock, self.resblock_kernel_sizes, self.resblock_dilation_sizes, self.input_log = resblock, rks, dils, bool(input_log)
        self.num_kernels, self.fuse_max_channels = len(rks), self.FUSE_MAX_CHANNELS
        block = _ResBlock1 if resblock == "1" else _ResBlock2
        self.conv_pre = _WNConv(self.n_mels, c0, 7)
        self.ups, self.resblocks, ch = nn.ModuleList(), nn.ModuleList(), c0
        for u, k in zip(rates, uks):
            self.ups.append(_WNConvTr(ch, ch // 2, k, stride=u))
            ch //= 2
            for rk, ds in zip(rks, dils):
                self.resblocks.append(block(ch, rk, ds))
        self.conv_post = _WNConv(ch, 1, 7)
        if os.path.exists(_lib.LIB_PATH):  # whatever the convolution kernel cannot tile is refused here, not at the first forward
            for m in self.modules():
                if isinstance(m, _WNConv) and not m.transposed and m is not self.conv_post:
                    try:
                        _lib.call_value("vbx_hifigan_conv_tile", -(-m.cin // 8) * 8, m.k, m.dilation)
                    except _lib.VbxError as e:
                        raise no(f"a convolution {m.cin} -> {m.cout}, kernel {m.k}, dilation {m.dilation} ({e})") from None

    @property
    def hop_length(self):
        return math.prod(self.upsample_rates)

    # -- state
    @staticmethod
    def _canonical(state_dict):
        """the other layouts this accepts: {'generator': sd} (the file HiFi-GAN's train.py writes), {'state_dict': sd}, and newer
        torch's parametrizations.weight.original0 / original1 (= weight_g / weight_v)"""
        for key in ("generator", "state_dict"):
            if key in state_dict and isinstance(state_dict[key], dict):
                state_dict = state_dict[key]
        out = {}
        for k, v in state_dict.items():
            if k.endswith(_PARAM + "0"):
                k = k[:-len(_PARAM) - 1] + "weight_g"
            elif k.endswith(_PARAM + "1"):
                k = k[:-len(_PARAM) - 1] + "weight_v"
            out[k] = v
        return out

    def load_state_dict(self, state_dict, strict=True, **kw):
        """weight_g / weight_v, parametrizations.weight.original0 / 1, or plain `weight` (saved after remove_weight_norm) per
        convolution; a layer given as plain `weight` becomes a plain layer (state_dict() then returns it that way)"""
        sd = self._canonical(state_dict)
        for name, m in self.named_modules():
            if isinstance(m, _WNConv):
                if f"{name}.weight" in sd:
                    m.plain_(True)
                elif f"{name}.weight_g" in sd:
                    m.plain_(False)
        return super().load_state_dict(sd, strict=strict, **kw)

    @classmethod
    def from_state_dict(cls, sd, config=None, **kw):
        """A state dict already in memory, in any of the layouts.  Widths, rates (kernel / 2) and kernel sizes are read off the shapes,
        the resblock type off the key names.  The DILATIONS are in no shape: they come from config["resblock_dilation_sizes"], else the
        V1 / V2 defaults (1, 3, 5) per block (ResBlock2: V3's (1, 3)) are assumed -- see the module docstring.  A config that
        contradicts the shapes raises ValueError.  **kw: constructor keywords no file tells (input_log)."""
        sd, config = cls._canonical(sd), _read_config(config) or {}
        shape = lambda name: tuple(sd[f"{name}.weight_v" if f"{name}.weight_v" in sd else f"{name}.weight"].shape)
        count = lambda prefix: 1 + max((int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix)), default=-1)
        stages, blocks = count("ups."), count("resblocks.")
        if "conv_pre.bias" not in sd or "conv_post.bias" not in sd or not stages or not blocks or blocks % stages:
            raise RuntimeError("HiFiGANGenerator.from_state_dict: not a HiFi-GAN generator layout (conv_pre, ups, resblocks, conv_post)")
        c0, n_mels, _ = shape("conv_pre")
        uks = tuple(shape(f"ups.{i}")[2] for i in range(stages))
        resblock = "1" if any(k.startswith("resblocks.0.convs1.") for k in sd) else "2"
        convs = "convs1" if resblock == "1" else "convs"
        nk = blocks // stages
        rks = tuple(shape(f"resblocks.{j}.{convs}.0")[2] for j in range(nk))
        depth = tuple(count(f"resblocks.{j}.{convs}.") for j in range(nk))
        found = dict(resblock=resblock, num_mels=n_mels, upsample_initial_channel=c0, upsample_kernel_sizes=uks, resblock_kernel_sizes=rks,
                     upsample_rates=tuple(k // 2 for k in uks))
        for key, val in found.items():
            if key in config:
                given = config[key] if isinstance(val, (int, str)) else tuple(config[key])
                if (str(given) if key == "resblock" else given) != val:
                    raise ValueError(f"HiFiGANGenerator.from_state_dict: config[{key!r}] = {config[key]} but the state dict has {val}")
        if "resblock_dilation_sizes" in config:
            dils = tuple(tuple(ds) for ds in config["resblock_dilation_sizes"])
        else:
            dils = (((1, 3, 5) if resblock == "1" else (1, 3)),) * nk
        if tuple(len(ds) for ds in dils) != depth:
            raise ValueError(f"HiFiGANGenerator.from_state_dict: the state dict has {depth} convolutions per residual block, the "
                             f"dilations {dils} say otherwise" + ("" if "resblock_dilation_sizes" in config else " (pass config=)"))
        self = cls(n_mels=n_mels, upsample_initial_channel=c0, upsample_rates=found["upsample_rates"], upsample_kernel_sizes=uks,
                   resblock=resblock, resblock_kernel_sizes=rks, resblock_dilation_sizes=dils, **kw)
        self.load_state_dict(sd)
        return self.eval()

    @classmethod
    def from_checkpoint(cls, path, config=None, **kw):
        """A LOCAL file written by torch.save: a generator state dict, {'generator': sd} or {'state_dict': sd}; config: HiFi-GAN's
        config.json (a LOCAL path or a dict) -- the only place the dilations are written down; see from_state_dict."""
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), config=config, **kw)

    # -- operand copies
    def folded_weights(self):
        """the folded fp32 weights by module path, e.g. 'ups.0' -> [Ci, Co, k]: what the state-dict layouts agree on"""
        return {name: m.folded() for name, m in self.named_modules() if isinstance(m, _WNConv)}

    def packed_ops(self):
        return self._cached(self._build_ops)

    @staticmethod
    def _conv_op(m, cin_padded=None):
        w = m.folded()  # [Co, Ci, k]
        if cin_padded and cin_padded != m.cin:
            w = torch.cat([w, w.new_zeros(m.cout, cin_padded - m.cin, m.k)], dim=1)
        return dict(w=w.permute(0, 2, 1).reshape(m.cout, -1).half().contiguous(), b=m.bias.detach().float().contiguous(), C=w.shape[1],
                    Co=m.cout, k=m.k, dil=m.dilation)

    def _build_ops(self):
        f = lambda t: t.detach().float().contiguous()
        ops = dict(pre=self._conv_op(self.conv_pre, -(-self.n_mels // 8) * 8), stages=[])
        for i, up in enumerate(self.ups):
            blocks = []
            for rb in self.resblocks[i * self.num_kernels:(i + 1) * self.num_kernels]:
                if self.resblock == "1":
                    blocks.append([(self._conv_op(c1), self._conv_op(c2)) for c1, c2 in zip(rb.convs1, rb.convs2)])
                else:
                    blocks.append([(self._conv_op(c), None) for c in rb.convs])
            ops["stages"].append(dict(w=pack_convtr_weight(up.folded(), up.stride).half().contiguous(), b=f(up.bias), C=up.cin, r=up.stride,
                                      blocks=blocks))
        post = self.conv_post
        ops["post"] = dict(w=f(post.folded()[0].t()), b=f(post.bias), C=post.cin, k=post.k)  # fp32 [k, C]
        return ops

    def forward(self, mel):
        if mel.ndim != 3 or mel.shape[1] != self.n_mels or not mel.is_floating_point():
            raise ValueError(f"HiFiGANGenerator takes float mels (batch, {self.n_mels}, frames), got {tuple(mel.shape)} {mel.dtype}")
        if mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError("HiFiGANGenerator: empty mel (at least one frame)")
        dev = mel.device
        if dev.type != "cuda":
            raise _lib.VbxError(f"HiFiGANGenerator runs only on an MI355X (gfx950) through libvbx_hip.so; the mel is on '{dev}'")
        if self.conv_pre.bias.device != dev:
            self.to(dev)
        with torch.inference_mode():
            return self._generate(mel)

    @staticmethod
    def _conv(op, x, res, B, L, st, act=True):
        y = torch.empty(B, L, op["Co"], dtype=torch.float16, device=x.device)
        _lib.call("vbx_hifigan_conv", x, op["w"], op["b"], res, y, B, L, op["C"], op["Co"], op["k"], op["dil"], int(act), LRELU_SLOPE, st)
        return y

    def _generate(self, mel):
        B, M, L = mel.shape
        dev, st = mel.device, _lib.current_stream()
        ops = self.packed_ops()
        mel32 = mel.detach().to(torch.float32).contiguous()
        x = torch.empty(B, L, ops["pre"]["C"], dtype=torch.float16, device=dev)
        _lib.call("vbx_hifigan_pack", mel32, x, B, M, L, int(self.input_log), st)
        xs = [self._conv(ops["pre"], x, None, B, L, st, act=False)]
        pad = lambda xs: (xs + [None, None])[:3]
        for stage in ops["stages"]:
            C, r = stage["C"], stage["r"]
            up = torch.empty(B, L * r, C // 2, dtype=torch.float16, device=dev)
            _lib.call("vbx_hifigan_convtr", *pad(xs), len(xs), stage["w"], stage["b"], up, B, L, C, r, LRELU_SLOPE, st)
            L, C, xs = L * r, C // 2, []
            for block in stage["blocks"]:
                h = up
                for c1, c2 in block:
                    if c2 is None:  # ResBlock2
                        h = self._conv(c1, h, h, B, L, st)
                    elif C <= self.fuse_max_channels:
                        y = torch.empty_like(h)
                        _lib.call("vbx_hifigan_respair", h, c1["w"], c1["b"], c2["w"], c2["b"], y, B, L, C, c1["k"], c1["dil"], LRELU_SLOPE, st)
                        h = y
                    else:
                        h = self._conv(c2, self._conv(c1, h, None, B, L, st), h, B, L, st)
                xs.append(h)
        post = ops["post"]
        wave = torch.empty(B, L, dtype=torch.float32, device=dev)
        _lib.call("vbx_hifigan_post", *pad(xs), len(xs), post["w"], post["b"], wave, B, L, post["C"], post["k"], LAST_SLOPE, st)
        return wave
