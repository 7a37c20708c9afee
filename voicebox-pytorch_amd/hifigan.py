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
import torch
from torch import nn

from . import _lib
from ._melgen import _MelGenerator, pack_convtr_weight  # noqa: F401  (pack_convtr_weight: imported from here by tests and tools)
from ._wnconv import WNConv, read_config

LRELU_SLOPE = 0.1  # HiFi-GAN's LRELU_SLOPE; the last activation uses torch's default instead
LAST_SLOPE = 0.01


class _ResBlock1(nn.Module):
    def __init__(self, ch, k, dilations):
        super().__init__()
        self.convs1 = nn.ModuleList([WNConv(ch, ch, k, d) for d in dilations])
        self.convs2 = nn.ModuleList([WNConv(ch, ch, k, 1) for _ in dilations])


class _ResBlock2(nn.Module):
    def __init__(self, ch, k, dilations):
        super().__init__()
        self.convs = nn.ModuleList([WNConv(ch, ch, k, d) for d in dilations])


class HiFiGANGenerator(_MelGenerator):
    """mel [B, n_mels, frames] (any float dtype, on the GPU; amplitude mels with input_log=True for weights trained on log features:
    log(clamp(mel, 1e-5)) is then taken as the input is packed) -> wave fp32 [B, frames * hop_length].

    Runs without gradients, in eval semantics.  The folded fp16 weights are packed once and re-packed when a parameter's version
    counter or storage changes; after a write through `p.data` call mark_weights_dirty().

    Raises NotImplementedError, before any launch, for what is not built: n_mels outside 1 .. 512; upsample_initial_channel not a
    multiple of 8 * 2^stages (16 at the narrowest stage's input) or above 1024; other than 1 .. 5 stages; a rate that is odd or outside 2 .. 8, or a kernel other
    than 2 * rate (those give frames * u + 1 samples or another phase structure); a residual kernel that is even or outside 3 .. 11;
    a dilation outside 1 .. 12; other than 1 .. 3 residual blocks per stage or 1 .. 3 dilations per block; resblock other than "1" /
    "2".  GPU tensors only (a CPU tensor raises VbxError); like its siblings, a forward on a device other than the parameters'
    MOVES THE MODULE there -- keep one instance per device.

    fuse_max_channels: residual pairs of ResBlock1 at widths up to this run as ONE launch (vbx_hifigan_respair, bit-equal to the
    two launches it replaces); the default is where it measured faster (profiles/hifigan_times.json)."""

    FUSE_MAX_CHANNELS = 64
    MAX_STAGES, MAX_CHANNELS = 5, 1024
    TILE_ENTRY = "vbx_hifigan_conv_tile"
    LAYOUT = "a HiFi-GAN generator layout (conv_pre, ups, resblocks, conv_post)"
    PRE_SLOPE = LRELU_SLOPE

    def __init__(self, n_mels=80, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
                 resblock="1", resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5),) * 3, input_log=False):
        super().__init__()
        self.fuse_max_channels = self.FUSE_MAX_CHANNELS
        self._build(n_mels, upsample_initial_channel, upsample_rates, upsample_kernel_sizes, resblock, resblock_kernel_sizes,
                    resblock_dilation_sizes, input_log)

    def _block(self, ch, k, dilations):
        return (_ResBlock1 if self.resblock == "1" else _ResBlock2)(ch, k, dilations)

    @staticmethod
    def _is_layout(sd):
        return "conv_pre.bias" in sd and "conv_post.bias" in sd

    @classmethod
    def from_state_dict(cls, sd, config=None, **kw):
        """A state dict already in memory, in any of the layouts.  Widths, rates (kernel / 2) and kernel sizes are read off the shapes,
        the resblock type off the key names.  The DILATIONS are in no shape: they come from config["resblock_dilation_sizes"], else the
        V1 / V2 defaults (1, 3, 5) per block (ResBlock2: V3's (1, 3)) are assumed -- see the module docstring.  A config that
        contradicts the shapes raises ValueError.  **kw: constructor keywords no file tells (input_log).  from_checkpoint(path,
        config=None, **kw) reads a LOCAL torch.save file first; HiFi-GAN's config.json is the only place the dilations are written down."""
        sd, config = cls._canonical(sd), read_config(config) or {}
        found, depth = cls._read_layout(sd)
        cls._check_config(found, config)
        if "resblock_dilation_sizes" in config:
            return cls._from_layout(sd, found, depth, tuple(tuple(ds) for ds in config["resblock_dilation_sizes"]), **kw)
        return cls._from_layout(sd, found, depth, (((1, 3, 5) if found["resblock"] == "1" else (1, 3)),) * len(depth), " (pass config=)", **kw)

    def _block_ops(self, rb):
        if self.resblock == "1":
            return [(self._conv_op(c1), self._conv_op(c2)) for c1, c2 in zip(rb.convs1, rb.convs2)]
        return [(self._conv_op(c), None) for c in rb.convs]

    def _upsample(self, xs, n, stage, up, B, L, st):
        _lib.call("vbx_hifigan_convtr", *xs, n, stage["w"], stage["b"], up, B, L, stage["C"], stage["r"], LRELU_SLOPE, st)

    def _run_block(self, block, h, B, L, C, st):
        for c1, c2 in block:
            if c2 is None:  # ResBlock2
                h = self._conv(c1, h, h, B, L, st, 1, LRELU_SLOPE)
            elif C <= self.fuse_max_channels:
                y = torch.empty_like(h)
                _lib.call("vbx_hifigan_respair", h, c1["w"], c1["b"], c2["w"], c2["b"], y, B, L, C, c1["k"], c1["dil"], LRELU_SLOPE, st)
                h = y
            else:
                h = self._conv(c2, self._conv(c1, h, None, B, L, st, 1, LRELU_SLOPE), h, B, L, st, 1, LRELU_SLOPE)
        return h

    def _post(self, xs, n, post, wave, B, L, st):
        _lib.call("vbx_hifigan_post", *xs, n, post["w"], post["b"], wave, B, L, post["C"], post["k"], LAST_SLOPE, st)
