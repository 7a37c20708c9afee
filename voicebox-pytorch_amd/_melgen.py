"""_MelGenerator: what HiFiGANGenerator (hifigan.py) and BigVGANGenerator (bigvgan.py) share, written once -- the keyword refusals, the
layers under their published names, the state-dict layouts and the reader of a checkpoint's shapes, the once-per-version operand
packing, forward's checks, and the launch sequence's skeleton: pack the mel, conv_pre, per stage the transposed convolution over the
mean of the last stage's residual blocks and then those blocks, the post launch.  A subclass says what differs: its residual block
(the module, its operands, its launches), the up-sampling and the post launch, and whatever its activation needs."""
import math
import os

import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights, read_checkpoint
from ._wnconv import WNConv, weight_norm_key
from .seanet import SEANetDecoder

pack_convtr_weight = SEANetDecoder._convtr_weight  # folded fp32 [C, Co, 2r] -> [r * Co, 2C], row p * Co + o = [W[:, o, p] | W[:, o, p + r]]


class _MelGenerator(PackedWeights, nn.Module):
    MAX_STAGES, MAX_CHANNELS = 0, 0  # the limits of the subclass's kernels
    TILE_ENTRY = ""  # the library's entry that says whether a residual convolution can be tiled
    UP_KEY = "ups.{}"  # the state-dict name of stage i's transposed convolution
    LAYOUT = ""  # the layout from_state_dict expects, for its refusal
    PRE_SLOPE = 0.0  # the slope argument of conv_pre's launch, which applies no activation

    @classmethod
    def _no(cls, what):
        return NotImplementedError(f"{cls.__name__}: {what} is not built")

    def _build(self, n_mels, upsample_initial_channel, upsample_rates, upsample_kernel_sizes, resblock, resblock_kernel_sizes,
               resblock_dilation_sizes, input_log):
        """refuse what is not built, then the layers in the published order: conv_pre, ups, resblocks, _post_layers"""
        no, who = self._no, type(self).__name__
        rates, uks = tuple(int(r) for r in upsample_rates), tuple(int(k) for k in upsample_kernel_sizes)
        rks = tuple(int(k) for k in resblock_kernel_sizes)
        dils = tuple(tuple(int(d) for d in ds) for ds in resblock_dilation_sizes)
        resblock = str(resblock)
        if resblock not in ("1", "2"):
            raise no(f'resblock="{resblock}" (only "1" and "2")')
        if not 1 <= n_mels <= 512:
            raise no(f"n_mels={n_mels} (1 .. 512)")
        if not 1 <= len(rates) <= self.MAX_STAGES:
            raise no(f"{len(rates)} upsampling stages (1 .. {self.MAX_STAGES})")
        if len(uks) != len(rates):
            raise ValueError(f"{who}: upsample_rates and upsample_kernel_sizes differ in length")
        for u, k in zip(rates, uks):
            if u % 2 or not 2 <= u <= 8:
                raise no(f"upsample rate {u} (even, 2 .. 8)")
            if k != 2 * u:
                raise no(f"upsample kernel {k} at rate {u} (only kernel = 2 * rate)")
        c0, unit = int(upsample_initial_channel), 8 * 2 ** len(rates)  # the narrowest stage is a multiple of 8 wide
        if c0 <= 0 or c0 % unit or c0 > self.MAX_CHANNELS:
            raise no(f"upsample_initial_channel={c0} (a multiple of 8 * 2^stages = {unit}, at most {self.MAX_CHANNELS})")
        if not 1 <= len(rks) <= 3:
            raise no(f"{len(rks)} residual blocks per stage (1 .. 3)")
        if len(dils) != len(rks):
            raise ValueError(f"{who}: resblock_kernel_sizes and resblock_dilation_sizes differ in length")
        for k, ds in zip(rks, dils):
            if k % 2 == 0 or not 3 <= k <= 11:
                raise no(f"residual kernel {k} (odd, 3 .. 11)")
            if not 1 <= len(ds) <= 3:
                raise no(f"{len(ds)} dilations per residual block (1 .. 3)")
            if any(not 1 <= d <= 12 for d in ds):
                raise no(f"dilations {ds} (each 1 .. 12)")
        self.n_mels, self.upsample_initial_channel, self.upsample_rates, self.upsample_kernel_sizes = int(n_mels), c0, rates, uks
        self.resblock, self.resblock_kernel_sizes, self.resblock_dilation_sizes, self.input_log = resblock, rks, dils, bool(input_log)
        self.num_kernels = len(rks)
        self.conv_pre = WNConv(self.n_mels, c0, 7)
        self.ups, self.resblocks, ch = nn.ModuleList(), nn.ModuleList(), c0
        for u, k in zip(rates, uks):
            self.ups.append(self._up(WNConv(ch, ch // 2, k, stride=u, transposed=True)))
            ch //= 2
            for rk, ds in zip(rks, dils):
                self.resblocks.append(self._block(ch, rk, ds))
        self._post_layers(ch)
        if os.path.exists(_lib.LIB_PATH):  # whatever the convolution kernel cannot tile is refused here, not at the first forward
            for m in self.modules():
                if isinstance(m, WNConv) and not m.transposed and m is not self.conv_post:
                    try:
                        _lib.call_value(self.TILE_ENTRY, -(-m.cin // 8) * 8, m.k, m.dilation)
                    except _lib.VbxError as e:
                        raise no(f"a convolution {m.cin} -> {m.cout}, kernel {m.k}, dilation {m.dilation} ({e})") from None

    # -- what a subclass says about its layers
    def _up(self, conv):
        """the entry of `ups` that holds a stage's transposed convolution"""
        return conv

    def _block(self, ch, k, dilations):
        """one residual block's module"""
        raise NotImplementedError

    def _post_layers(self, ch):
        """what follows the last stage, registered in the published order"""
        self.conv_post = WNConv(ch, 1, 7)

    @property
    def hop_length(self):
        return math.prod(self.upsample_rates)

    # -- state
    @staticmethod
    def _canonical(state_dict):
        """the other layouts this accepts: {'generator': sd} (the file the libraries' train.py writes), {'state_dict': sd}, and newer
        torch's parametrizations.weight.original0 / original1 (= weight_g / weight_v)"""
        for key in ("generator", "state_dict"):
            if key in state_dict and isinstance(state_dict[key], dict):
                state_dict = state_dict[key]
        return {weight_norm_key(k): v for k, v in state_dict.items()}

    def _check_state(self, sd):
        """what a canonical state dict may not hold (ValueError); nothing here"""

    def load_state_dict(self, state_dict, strict=True, **kw):
        """weight_g / weight_v, parametrizations.weight.original0 / 1, or plain `weight` (saved after remove_weight_norm) per
        convolution; a layer given as plain `weight` becomes a plain layer (state_dict() then returns it that way)"""
        sd = self._canonical(state_dict)
        self._check_state(sd)
        for name, m in self.named_modules():
            if isinstance(m, WNConv):
                if f"{name}.weight" in sd:
                    m.plain_(True)
                elif f"{name}.weight_g" in sd:
                    m.plain_(False)
        return super().load_state_dict(sd, strict=strict, **kw)

    @staticmethod
    def _is_layout(sd):
        """whether the keys outside ups / resblocks are this generator's"""
        raise NotImplementedError

    @classmethod
    def _read_layout(cls, sd):
        """(found, depth) of a canonical state dict: the widths, the rates (kernel / 2) and the kernel sizes read off the shapes and the
        resblock type off the key names, under config.json's names; the number of convolutions in each of a stage's residual blocks"""
        shape = lambda name: tuple(sd[f"{name}.weight_v" if f"{name}.weight_v" in sd else f"{name}.weight"].shape)
        count = lambda prefix: 1 + max((int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix)), default=-1)
        stages, blocks = count("ups."), count("resblocks.")
        if not cls._is_layout(sd) or not stages or not blocks or blocks % stages:
            raise RuntimeError(f"{cls.__name__}.from_state_dict: not {cls.LAYOUT}")
        c0, n_mels, _ = shape("conv_pre")
        uks = tuple(shape(cls.UP_KEY.format(i))[2] for i in range(stages))
        resblock = "1" if any(k.startswith("resblocks.0.convs1.") for k in sd) else "2"
        convs = "convs1" if resblock == "1" else "convs"
        nk = blocks // stages
        rks = tuple(shape(f"resblocks.{j}.{convs}.0")[2] for j in range(nk))
        depth = tuple(count(f"resblocks.{j}.{convs}.") for j in range(nk))
        found = dict(resblock=resblock, num_mels=n_mels, upsample_initial_channel=c0, upsample_kernel_sizes=uks, resblock_kernel_sizes=rks,
                     upsample_rates=tuple(k // 2 for k in uks))
        return found, depth

    @classmethod
    def _check_config(cls, found, config):
        """a config that contradicts what the state dict says raises ValueError"""
        for key, val in found.items():
            if key in config:
                given = config[key] if isinstance(val, (int, str)) else tuple(config[key])
                if (str(given) if key == "resblock" else given) != val:
                    raise ValueError(f"{cls.__name__}.from_state_dict: config[{key!r}] = {config[key]} but the state dict has {val}")

    @classmethod
    def _from_layout(cls, sd, found, depth, dilations, hint="", **kw):
        """the module of _read_layout's findings and the dilations, which must agree with depth, with sd loaded; in eval mode"""
        if tuple(len(ds) for ds in dilations) != depth:
            raise ValueError(f"{cls.__name__}.from_state_dict: the state dict has {depth} convolutions per residual block, the "
                             f"dilations {dilations} say otherwise{hint}")
        self = cls(n_mels=found["num_mels"], upsample_initial_channel=found["upsample_initial_channel"], upsample_rates=found["upsample_rates"],
                   upsample_kernel_sizes=found["upsample_kernel_sizes"], resblock=found["resblock"],
                   resblock_kernel_sizes=found["resblock_kernel_sizes"], resblock_dilation_sizes=dilations, **kw)
        self.load_state_dict(sd)
        return self.eval()

    @classmethod
    def from_checkpoint(cls, path, config=None, **kw):
        """A LOCAL file written by torch.save: a generator state dict, {'generator': sd} or {'state_dict': sd}; config: the library's
        config.json (a LOCAL path or a dict); see from_state_dict."""
        return cls.from_state_dict(read_checkpoint(path), config=config, **kw)

    # -- operand copies
    def folded_weights(self):
        """the folded fp32 weights by module path, e.g. 'conv_pre' -> [Co, Ci, k], a transposed convolution's -> [Ci, Co, k]: what the
        state-dict layouts agree on"""
        return {name: m.folded() for name, m in self.named_modules() if isinstance(m, WNConv)}

    def packed_ops(self):
        return self._cached(self._build_ops)

    @staticmethod
    def _conv_op(m):
        """the input channels zero-padded to a multiple of 8: conv_pre's; every other width is one already"""
        w = m.folded()  # [Co, Ci, k]
        if m.cin % 8:
            w = torch.cat([w, w.new_zeros(m.cout, -m.cin % 8, m.k)], dim=1)
        return dict(w=w.permute(0, 2, 1).reshape(m.cout, -1).half().contiguous(), b=m.bias.detach().float().contiguous(), C=w.shape[1],
                    Co=m.cout, k=m.k, dil=m.dilation)

    def _block_ops(self, rb):
        """one residual block's operands: a list with one tuple per dilation"""
        raise NotImplementedError

    def _build_ops(self):
        f = lambda t: t.detach().float().contiguous()
        ops = dict(pre=self._conv_op(self.conv_pre), stages=[])
        for i, up in enumerate(m for m in self.ups.modules() if isinstance(m, WNConv)):
            blocks = [self._block_ops(rb) for rb in self.resblocks[i * self.num_kernels:(i + 1) * self.num_kernels]]
            ops["stages"].append(dict(w=pack_convtr_weight(up.folded(), up.stride).half().contiguous(), b=f(up.bias), C=up.cin, r=up.stride,
                                      blocks=blocks))
        post = self.conv_post
        ops["post"] = dict(w=f(post.folded()[0].t()), b=None if post.bias is None else f(post.bias), C=post.cin, k=post.k)  # fp32 [k, C]
        return ops

    def forward(self, mel):
        who = type(self).__name__
        if mel.ndim != 3 or mel.shape[1] != self.n_mels or not mel.is_floating_point():
            raise ValueError(f"{who} takes float mels (batch, {self.n_mels}, frames), got {tuple(mel.shape)} {mel.dtype}")
        if mel.shape[0] < 1 or mel.shape[2] < 1:
            raise ValueError(f"{who}: empty mel (at least one frame)")
        dev = mel.device
        if dev.type != "cuda":
            raise _lib.VbxError(f"{who} runs only on an MI355X (gfx950) through libvbx_hip.so; the mel is on '{dev}'")
        if self.conv_pre.bias.device != dev:
            self.to(dev)
        with torch.inference_mode():
            return self._generate(mel)

    # -- launches
    @staticmethod
    def _conv(op, x, res, B, L, st, act, slope):
        """conv(x) + bias (+ res), x through a leaky ReLU of `slope` first where act is 1"""
        y = torch.empty(B, L, op["Co"], dtype=torch.float16, device=x.device)
        _lib.call("vbx_hifigan_conv", x, op["w"], op["b"], res, y, B, L, op["C"], op["Co"], op["k"], op["dil"], act, slope, st)
        return y

    def _upsample(self, xs, n, stage, up, B, L, st):
        """the transposed convolution of a stage over the mean of the n tensors in xs (padded to three with None)"""
        raise NotImplementedError

    def _run_block(self, block, h, B, L, C, st):
        """one residual block's launches on h [B, L, C]; returns its result"""
        raise NotImplementedError

    def _post(self, xs, n, post, wave, B, L, st):
        """conv_post over the mean of the n tensors in xs and the final function, into wave"""
        raise NotImplementedError

    def _generate(self, mel):
        B, M, L = mel.shape
        dev, st = mel.device, _lib.current_stream()
        ops = self.packed_ops()
        mel32 = mel.detach().to(torch.float32).contiguous()
        x = torch.empty(B, L, ops["pre"]["C"], dtype=torch.float16, device=dev)
        _lib.call("vbx_hifigan_pack", mel32, x, B, M, L, int(self.input_log), st)
        xs = [self._conv(ops["pre"], x, None, B, L, st, 0, self.PRE_SLOPE)]
        pad = lambda xs: (xs + [None, None])[:3]
        for stage in ops["stages"]:
            up = torch.empty(B, L * stage["r"], stage["C"] // 2, dtype=torch.float16, device=dev)
            self._upsample(pad(xs), len(xs), stage, up, B, L, st)
            L, C = L * stage["r"], stage["C"] // 2
            xs = [self._run_block(block, up, B, L, C, st) for block in stage["blocks"]]
        wave = torch.empty(B, L, dtype=torch.float32, device=dev)
        self._post(pad(xs), len(xs), ops["post"], wave, B, L, st)
        return wave
