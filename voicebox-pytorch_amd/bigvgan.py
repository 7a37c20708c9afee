"""BigVGANGenerator: the generator of BigVGAN (Lee et al. 2023, "BigVGAN: a universal neural vocoder with large-scale training") on
the device -- the mel vocoder most 24 kHz / 100-band checkpoints come with, which is LogMelCodec's configuration.  mel fp32
[B, n_mels, frames] -> wave fp32 [B, frames * prod(upsample_rates)] in [-1, 1]: a `vocoder=` of LogMelCodec by its call shape.

The network is HiFi-GAN's generator (hifigan.py) with two differences.  Every activation is Activation1d, a periodic snake function
inside a 2x anti-aliasing filter: up-sample by 2 with a 12-tap Kaiser-sinc filter (replicate padding 5 / 5, the result doubled),
s = u + sin^2(alpha u) / (beta + 1e-9) per channel ("snake": beta = alpha), replicate padding 5 / 6, the 12-tap low-pass with stride 2.
And there is NO activation in front of the transposed convolutions.  conv_pre (7 taps); per stage ConvTranspose1d(C, C / 2, 2u,
stride u, padding u / 2) and the MEAN of num_kernels residual blocks; activation_post, conv_post (7 taps, one channel, with or
without a bias), then tanh or clamp(-1, 1).  AMPBlock1 is, per dilation d with index m, x = c2[m](acts[2m + 1](c1[m](acts[2m](x)))) + x
with c1 dilated and c2 not -- the `activations` list is INTERLEAVED; AMPBlock2 is x = c[m](acts[m](x)) + x.  All convolution
paddings are zeros; weight norm is torch's default dim=0.  The parameters and buffers carry the published names (conv_pre, ups.{i}.0,
resblocks.{n}.convs1.{m} / .convs2.{m} / .convs.{m}, resblocks.{n}.activations.{l}.act.alpha / .act.beta / .upsample.filter /
.downsample.lowpass.filter, activation_post.*, conv_post), so a `generator` state dict loads with strict=True.  Neither the library nor
any weights are part of this package, and nothing here reaches a hub: from_checkpoint reads LOCAL files.

PARITY UNPINNED: the BigVGAN library is not a dependency and no fixture of it exists.  The arithmetic is restated in fp64 in
tests/bigvgan_ref.py; the kernels are tested against that restatement (tests/test_bigvgan_gpu.py, profiles/bigvgan_parity.txt).

CONFIG IS REQUIRED by the loaders.  A state dict cannot say (1) its dilations, (2) whether alpha / beta are stored as logarithms
(snake_logscale), (3) whether the output is tanh or a clamp (use_tanh_at_final): none of them changes a shape or a key, and a wrong
guess loads cleanly and runs, silently, as a different network.

Device path (csrc/bigvgan.hip beside csrc/hifigan.hip, on the tile core of csrc/seanet_tile.hpp): a fixed launch sequence, under the
precision contract of include/vbx.h: activations fp16 channel-last, rounded once where stored; Activation1d in fp32 with the accurate
sinf, in one documented order of operations; weights fp16, weight norm folded in fp32; sums fp32; no atomics.  Inference only.
"""
import math

import torch
from torch import nn

from . import _lib
from ._melgen import _MelGenerator
from ._packing import tensors_key
from ._wnconv import WNConv, read_config

ACTIVATIONS = ("snake", "snakebeta")
FILTER_TAPS = 12
_CONFIG_REQUIRED = ("BigVGANGenerator: config (BigVGAN's config.json, a path or a dict) is required: a state dict cannot say its dilations "
                    "(resblock_dilation_sizes), whether alpha / beta are stored as logarithms (snake_logscale), or whether the output is "
                    "tanh or a clamp (use_tanh_at_final)")


def kaiser_sinc_filter1d(cutoff=0.25, half_width=0.3, kernel_size=FILTER_TAPS):
    """the library's anti-aliasing filter [1, 1, kernel_size]; it only fills a freshly constructed module -- a loaded state dict
    brings its own buffers"""
    half = kernel_size // 2
    A = 2.285 * (half - 1) * math.pi * (4 * half_width) + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    window = torch.kaiser_window(kernel_size, beta=beta, periodic=False)
    time = torch.arange(-half, half) + 0.5
    f = 2 * cutoff * window * torch.sinc(2 * cutoff * time)
    return (f / f.sum()).reshape(1, 1, kernel_size)


class _Snake(nn.Module):
    def __init__(self, ch, beta, logscale):
        super().__init__()
        init = torch.zeros if logscale else torch.ones
        self.alpha = nn.Parameter(init(ch))
        if beta:
            self.beta = nn.Parameter(init(ch))


class _Filter(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("filter", kaiser_sinc_filter1d())


class _DownSample(nn.Module):
    def __init__(self):
        super().__init__()
        self.lowpass = _Filter()


class _Activation1d(nn.Module):
    def __init__(self, ch, beta, logscale):
        super().__init__()
        self.act, self.upsample, self.downsample = _Snake(ch, beta, logscale), _Filter(), _DownSample()


class _AMPBlock1(nn.Module):
    def __init__(self, ch, k, dilations, act):
        super().__init__()
        self.convs1 = nn.ModuleList([WNConv(ch, ch, k, d) for d in dilations])
        self.convs2 = nn.ModuleList([WNConv(ch, ch, k, 1) for _ in dilations])
        self.activations = nn.ModuleList([act(ch) for _ in range(2 * len(dilations))])  # interleaved: 2m before convs1[m], 2m + 1 before convs2[m]


class _AMPBlock2(nn.Module):
    def __init__(self, ch, k, dilations, act):
        super().__init__()
        self.convs = nn.ModuleList([WNConv(ch, ch, k, d) for d in dilations])
        self.activations = nn.ModuleList([act(ch) for _ in dilations])


class BigVGANGenerator(_MelGenerator):
    """mel [B, n_mels, frames] (any float dtype, on the GPU; amplitude mels with input_log=True: log(clamp(mel, 1e-5)) is taken as the
    input is packed) -> wave fp32 [B, frames * hop_length].

    Runs without gradients, in eval semantics.  The folded fp16 weights, alpha and 1 / (beta + 1e-9) (fp32, the exp of snake_logscale
    included; 1 / (alpha + 1e-9) for "snake") and the filters are packed once and re-packed when a parameter's or buffer's version
    counter or storage changes; after a write through `p.data` call mark_weights_dirty().

    Raises NotImplementedError, before any launch, for what is not built: n_mels outside 1 .. 512; other than 1 .. 6 stages;
    upsample_initial_channel not a multiple of 8 * 2^stages or above 1536; a rate that is odd or outside 2 .. 8, or a kernel other
    than 2 * rate; a residual kernel that is even or outside 3 .. 11; a dilation outside 1 .. 12; other than 1 .. 3 residual blocks per
    stage or 1 .. 3 dilations per block; resblock other than "1" / "2"; an activation other than "snake" / "snakebeta"; an
    Activation1d other than ratio 2 / 2 with 12 / 12 taps.  GPU tensors only (a CPU tensor raises VbxError); a forward on a device
    other than the parameters' MOVES THE MODULE there.  load_state_dict loads the filter buffers and USES them; one of another shape
    than [1, 1, 12] raises ValueError.

    fuse_act_max_channels: up to this width a residual convolution computes its Activation1d while it stages its span
    (vbx_bigvgan_conv); above it the activation is a launch of its own (vbx_bigvgan_act) and the activated tensor goes through
    memory.  None: fuse everywhere; 0: nowhere; a number also keeps the fused form to launches of at most FUSE_ACT_MAX_ELEMENTS
    input elements (the default: measured, see below).  Both forms give the SAME BITS."""

    # Measured (tools/bigvgan_times.py, profiles/bigvgan_times.json: one stage's residual convolutions alone, fused / unfused time, min of
    # five alternating windows, one MI355X).  The fused form saves a launch, one write and one read of the tensor; it re-computes the
    # activation on the (k - 1) d halo positions of every tile and pays ten extra s values at the start of every run of positions a
    # thread walks.  So it wins where a launch is small and loses where the device is full:
    #   B x frames   channels x positions    elements   fused / unfused
    #   1 x 301      24 x 77056 .. 192 x 9632   1.8 M    0.72  0.73  0.78  0.91   (wide shape, stages 5 .. 2)
    #   1 x 301      32 x 77056 .. 128 x 19264  2.5 M    0.72  0.74  0.81         (base widths, stages 3 .. 1)
    #   1 x 301      384 x 4816                 1.8 M    0.99                     768 x 1204 (0.9 M): 1.05
    #   8 x 1024     256 x 8192                 2.1 M    0.98
    #   8 x 1024     96 x 65536                 6.3 M    0.98                     48 x 131072: 1.25   24 x 262144: 1.47
    #   8 x 1024     128 x 65536 .. 32 x 262144 8.4 M    0.95  1.16  1.36
    #   8 x 1024     192 x 32768 .. 768 x 4096  3 .. 6 M 1.06  1.07  1.05
    # The rule read off it: fuse up to 384 channels while the tensor has at most 4 Mi elements.  Whole calls under it, beside
    # fused-everywhere / fused-nowhere, are in the README.
    FUSE_ACT_MAX_CHANNELS = 384
    FUSE_ACT_MAX_ELEMENTS = 4 << 20  # B * L * C of the convolution's input; applies only while fuse_act_max_channels is a number

    MAX_STAGES, MAX_CHANNELS = 6, 1536
    TILE_ENTRY = "vbx_bigvgan_conv_tile"
    UP_KEY = "ups.{}.0"
    LAYOUT = "a BigVGAN generator layout (conv_pre, ups, resblocks, activation_post, conv_post)"
    PRE_SLOPE = 1.0

    def __init__(self, n_mels=100, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                 resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, activation="snakebeta",
                 snake_logscale=True, use_tanh_at_final=True, use_bias_at_final=True, input_log=False, up_ratio=2, down_ratio=2,
                 up_kernel_size=FILTER_TAPS, down_kernel_size=FILTER_TAPS):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise self._no(f'activation="{activation}" (only "snake" and "snakebeta")')
        if (up_ratio, down_ratio, up_kernel_size, down_kernel_size) != (2, 2, FILTER_TAPS, FILTER_TAPS):
            raise self._no(f"an Activation1d with ratios {up_ratio} / {down_ratio} and {up_kernel_size} / {down_kernel_size} taps (only 2 / 2, 12 / 12)")
        self.activation, self.snake_logscale = activation, bool(snake_logscale)
        self.use_tanh_at_final, self.use_bias_at_final = bool(use_tanh_at_final), bool(use_bias_at_final)
        self.fuse_act_max_channels = self.FUSE_ACT_MAX_CHANNELS
        self._build(n_mels, upsample_initial_channel, upsample_rates, upsample_kernel_sizes, resblock, resblock_kernel_sizes,
                    resblock_dilation_sizes, input_log)

    def _act(self, ch):
        return _Activation1d(ch, self.activation == "snakebeta", self.snake_logscale)

    def _up(self, conv):
        return nn.ModuleList([conv])  # the published name is ups.{i}.0

    def _block(self, ch, k, dilations):
        return (_AMPBlock1 if self.resblock == "1" else _AMPBlock2)(ch, k, dilations, self._act)

    def _post_layers(self, ch):
        self.activation_post = self._act(ch)
        super()._post_layers(ch)
        if not self.use_bias_at_final:
            self.conv_post.bias = None

    # -- state
    def _check_state(self, sd):
        for k, v in sd.items():
            if k.endswith(".filter") and tuple(v.shape) != (1, 1, FILTER_TAPS):
                raise ValueError(f"BigVGANGenerator: the filter buffer {k} has shape {tuple(v.shape)}; only [1, 1, {FILTER_TAPS}] is built")

    @staticmethod
    def _is_layout(sd):
        return "conv_pre.bias" in sd and any(k.startswith("conv_post.") for k in sd) and any(k.startswith("activation_post.") for k in sd)

    @classmethod
    def from_state_dict(cls, sd, config=None, **kw):
        """A state dict already in memory, in any of the layouts, and BigVGAN's config.json (a LOCAL path or a dict), which is
        REQUIRED: see the module docstring.  Widths, rates and kernel sizes are read off the shapes and must agree with the config
        where it states them (ValueError); `activation` must agree with whether act.beta keys exist and use_bias_at_final with whether
        conv_post.bias does.  Keys the config may omit take the library's defaults: use_tanh_at_final=True, use_bias_at_final=True,
        snake_logscale=False.  **kw: constructor keywords no file tells (input_log)."""
        if config is None:
            raise ValueError(_CONFIG_REQUIRED)
        sd, config = cls._canonical(sd), read_config(config)
        for key in ("resblock_dilation_sizes", "activation"):
            if key not in config:
                raise ValueError(f"BigVGANGenerator.from_state_dict: config[{key!r}] is missing")
        found, depth = cls._read_layout(sd)
        found.update(activation="snakebeta" if "activation_post.act.beta" in sd else "snake", use_bias_at_final="conv_post.bias" in sd)
        cls._check_config(found, dict({"use_bias_at_final": True}, **config))
        return cls._from_layout(sd, found, depth, tuple(tuple(ds) for ds in config["resblock_dilation_sizes"]), activation=found["activation"],
                                snake_logscale=bool(config.get("snake_logscale", False)),
                                use_tanh_at_final=bool(config.get("use_tanh_at_final", True)), use_bias_at_final=found["use_bias_at_final"], **kw)

    @classmethod
    def from_checkpoint(cls, path, config=None, **kw):
        """A LOCAL file written by torch.save: a generator state dict, {'generator': sd} or {'state_dict': sd}; config: BigVGAN's
        config.json (a LOCAL path or a dict), REQUIRED -- see from_state_dict."""
        if config is None:  # before the file is read
            raise ValueError(_CONFIG_REQUIRED)
        return super().from_checkpoint(path, config=config, **kw)

    # -- operand copies
    def _weights_key(self):
        return tensors_key(list(self.parameters()) + list(self.buffers()))  # the filters are buffers

    def _act_op(self, a):
        """alpha and 1 / (beta + 1e-9) as the kernels take them: fp32, single torch operations"""
        f = lambda t: t.detach().float()
        alpha = f(a.act.alpha)
        beta = f(a.act.beta) if self.activation == "snakebeta" else alpha
        if self.snake_logscale:
            alpha, beta = torch.exp(alpha), torch.exp(beta)
        return dict(alpha=alpha.contiguous(), invb=(1.0 / (beta + 1e-9)).contiguous(), fu=f(a.upsample.filter).reshape(-1).contiguous(),
                    fd=f(a.downsample.lowpass.filter).reshape(-1).contiguous())

    def _block_ops(self, rb):
        acts = [self._act_op(a) for a in rb.activations]
        if self.resblock == "1":
            return [(acts[2 * m], self._conv_op(c1), acts[2 * m + 1], self._conv_op(c2)) for m, (c1, c2) in enumerate(zip(rb.convs1, rb.convs2))]
        return [(acts[m], self._conv_op(c), None, None) for m, c in enumerate(rb.convs)]

    def _build_ops(self):
        ops = super()._build_ops()
        ops["post"]["act"] = self._act_op(self.activation_post)
        return ops

    def _act_conv(self, a, op, x, res, B, L, st):
        """conv(A(x)) + bias (+ res): one launch up to fuse_act_max_channels, else the activation on its own first; the same bits"""
        fuse = self.fuse_act_max_channels
        if fuse is None or (op["C"] <= fuse and B * L * op["C"] <= self.FUSE_ACT_MAX_ELEMENTS):
            y = torch.empty(B, L, op["Co"], dtype=torch.float16, device=x.device)
            _lib.call("vbx_bigvgan_conv", x, a["alpha"], a["invb"], a["fu"], a["fd"], op["w"], op["b"], res, y, B, L, op["C"], op["Co"], op["k"],
                      op["dil"], st)
            return y
        h = torch.empty_like(x)
        _lib.call("vbx_bigvgan_act", x, None, None, 1, a["alpha"], a["invb"], a["fu"], a["fd"], h, B, L, op["C"], st)
        return self._conv(op, h, res, B, L, st, 0, 1.0)

    def _upsample(self, xs, n, stage, up, B, L, st):
        _lib.call("vbx_bigvgan_convtr", *xs, n, stage["w"], stage["b"], up, B, L, stage["C"], stage["r"], st)

    def _run_block(self, block, h, B, L, C, st):
        for a1, c1, a2, c2 in block:
            if c2 is None:  # AMPBlock2
                h = self._act_conv(a1, c1, h, h, B, L, st)
            else:
                h = self._act_conv(a2, c2, self._act_conv(a1, c1, h, None, B, L, st), h, B, L, st)
        return h

    def _post(self, xs, n, post, wave, B, L, st):
        a = post["act"]
        _lib.call("vbx_bigvgan_post", *xs, n, a["alpha"], a["invb"], a["fu"], a["fd"], post["w"], post["b"], wave, B, L, post["C"], post["k"],
                  0 if self.use_tanh_at_final else 1, st)
