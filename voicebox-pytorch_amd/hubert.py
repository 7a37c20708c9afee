"""HubertWithKmeans: HuBERT base (Hsu et al. 2021) up to one encoder layer plus a k-means codebook on the device -- waves into
semantic token ids, the module the reference calls `wav2vec` ("hubert usually", voicebox_pytorch.py:1374-1390, :1213-1257) and
audiolm_pytorch ships as HubertWithKmeans: forward(wav_input, flatten=True, input_sample_hz=None) -> int64 [B, frames].

The network is the BASE form only (feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False): a 1 -> C convolution with
GroupNorm(C, C) over time and erf-GELU, six strided C -> C convolutions with erf-GELU, LayerNorm + Linear(C, D), a grouped weight-normed
positional convolution (one norm per tap, the last output sample dropped), encoder.layer_norm, post-LN transformer layers
1 .. output_layer (later layers are loaded, never packed or launched), then the Euclidean argmin over `cluster_centers`.  The
parameters carry transformers.HubertModel's names and shapes, so its state_dict() loads as is; fairseq's names and the old
weight_g / weight_v pair are translated.  Neither library nor any weights are part of this package and nothing here reaches a hub:
from_checkpoint reads LOCAL files.

PARITY PINNED against transformers: tests/hubert_ref.py restates the network in fp64 and tests/test_hubert_cpu.py holds that
restatement to transformers.HubertModel (fp64, eager attention) within 1e-10 at every hidden state; the kernels are tested against
the restatement (tests/test_hubert_gpu.py, profiles/hubert_parity.txt).  fairseq and audiolm_pytorch themselves stay unpinned (absent),
including the claim that fairseq's output_layer = L is hidden_states[L].

Device path (csrc/hubert.hip, csrc/gemm.hip, csrc/attn.hip): a fixed launch sequence without host synchronisation; where each tensor
is rounded is stated in include/vbx.h.  Inference only, GPU tensors only.  Rows of unequal length: lens= (per-row sample counts; include/vbx.h
"ragged waves") makes every row of a padded batch the row it would be alone; a padding / attention mask is not served.

HubertLargeWithKmeans (below) is the LARGE form -- feat_extract_norm="layer", the pre-LN encoder of do_stable_layer_norm=True, an
optional convolution bias: hubert-large-ll60k -- beside it, as CausalSEANetEncoder stands beside SEANetEncoder; tests/hubert_large_ref.py
is its restatement, pinned to transformers.HubertModel the same way (tests/test_hubert_large_cpu.py).
"""
import math

import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights
from .wave_lens import device_lens, map_lens, resample_lens

_G0, _G1 = "encoder.pos_conv_embed.conv.parametrizations.weight.original0", "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
_LDS_MAX = 160 * 1024  # csrc/seanet_tile.hpp: SN_LDS_MAX


class _Box(nn.Module):
    """a bare container: the parameters below carry transformers.HubertModel's dotted names"""


def _ln(dim):
    b = _Box()
    b.weight, b.bias = nn.Parameter(torch.ones(dim)), nn.Parameter(torch.zeros(dim))
    return b


def _linear(out, inp):
    b = _Box()
    b.weight, b.bias = nn.Parameter(torch.randn(out, inp) / math.sqrt(inp)), nn.Parameter(torch.zeros(out))
    return b


_FAIRSEQ = (("self_attn_layer_norm.", "layer_norm."), ("self_attn.", "attention."), ("fc1.", "feed_forward.intermediate_dense."),
            ("fc2.", "feed_forward.output_dense."))
_SKIPPED = ("masked_spec_embed", "mask_emb", "label_embs_concat", "final_proj.")


def convert_state_dict(sd):
    """transformers' names from any of: a transformers.HubertModel state dict (optionally under `hubert.`), fairseq's names, the old
    weight_g / weight_v pair, a file's {'model': sd}.  masked_spec_embed / mask_emb / label_embs_concat / final_proj are skipped."""
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    out = {}
    for k, v in sd.items():
        if k.startswith("hubert."):
            k = k[len("hubert."):]
        if k.startswith(_SKIPPED):
            continue
        parts = k.split(".")
        if k.startswith("feature_extractor.conv_layers.") and len(parts) == 5 and parts[3] == "0" and parts[4] in ("weight", "bias"):
            k = f"feature_extractor.conv_layers.{parts[2]}.conv.{parts[4]}"  # fairseq: Sequential(conv, dropout, norm, gelu)
        elif k.startswith("feature_extractor.conv_layers.") and len(parts) == 6 and parts[3] == "2" and parts[4] == "1":
            # fairseq, mode "layer_norm": the norm is Sequential(TransposeLast, LayerNorm, TransposeLast) (from memory; unpinned)
            k = f"feature_extractor.conv_layers.{parts[2]}.layer_norm.{parts[5]}"
        elif k.startswith("feature_extractor.conv_layers.") and len(parts) == 5 and parts[3] == "2":
            k = f"feature_extractor.conv_layers.{parts[2]}.layer_norm.{parts[4]}"
        elif k.startswith("layer_norm."):
            k = "feature_projection." + k
        elif k.startswith("post_extract_proj."):
            k = "feature_projection.projection." + k[len("post_extract_proj."):]
        elif k.startswith("encoder.pos_conv.0."):
            k = "encoder.pos_conv_embed.conv." + k[len("encoder.pos_conv.0."):]
        elif k.startswith("encoder.layers."):
            for a, b in _FAIRSEQ:
                if "." + a in k:
                    k = k.replace("." + a, "." + b)
                    break
        if k == "encoder.pos_conv_embed.conv.weight_g":
            k = _G0
        elif k == "encoder.pos_conv_embed.conv.weight_v":
            k = _G1
        out[k] = v
    return out


def load_kmeans(path):
    """cluster centres fp32 [K, D] from a LOCAL file: a torch.save'd tensor, a .npy array, or a joblib-pickled sklearn estimator
    with cluster_centers_ (joblib / sklearn are imported only then)"""
    path = str(path)
    if path.endswith(".npy"):
        import numpy as np

        c = torch.from_numpy(np.load(path))
    else:
        try:
            c = torch.load(path, map_location="cpu", weights_only=True)
        except Exception:
            import joblib

            c = joblib.load(path)
        if not isinstance(c, torch.Tensor):
            c = torch.as_tensor(c.cluster_centers_ if hasattr(c, "cluster_centers_") else c)
    if c.ndim != 2:
        raise ValueError(f"HubertWithKmeans: cluster centres must be [K, D] (got {tuple(c.shape)})")
    return c.float().contiguous()


class HubertWithKmeans(PackedWeights, nn.Module):
    """wave fp32 [B, T] (or [B, 1, T]) at target_sample_hz -> ids int64 [B, frames]; features(wave) -> fp32 [B, frames, hidden_size],
    the output of encoder layer `output_layer` (transformers' hidden_states[output_layer]).  input_sample_hz: the wave is first
    resampled on the device with the package's resample(); seq_len_multiple_of then curtails it to a multiple (audiolm_pytorch's
    order).  frames: L <- (L - k) // s + 1 per convolution.

    Raises NotImplementedError, before any launch, for what is not served: feat_extract_norm="layer", do_stable_layer_norm=True (the
    large models), conv_bias=True; hidden_size / num_attention_heads != 64 (x-large); hidden_size not a multiple of 64 or above 2048;
    conv_dim not constant, not a multiple of 16 or above 512; conv_kernel[0] or conv_stride[0] above 16, later kernels outside 2 .. 3,
    later strides other than 2; hidden_size / groups not a multiple of 8, an odd num_conv_pos_embeddings, a positional convolution whose
    16-position span does not fit the LDS; codebook_size outside 2 .. 4096; output_layer outside 1 .. num_hidden_layers; a wave shorter than
    one frame; an attention / padding mask.  A CPU tensor raises VbxError."""

    _NAME = "HubertWithKmeans"

    @classmethod
    def _check_form(cls, feat_extract_norm, do_stable_layer_norm, conv_bias):
        """the base form only; the large form is HubertLargeWithKmeans"""
        who, other = cls._NAME, "HubertLargeWithKmeans serves the large form"
        if feat_extract_norm != "group":
            raise NotImplementedError(f'{who}: feat_extract_norm="{feat_extract_norm}" is not built here (only "group", the base form; {other})')
        if do_stable_layer_norm:
            raise NotImplementedError(f"{who}: do_stable_layer_norm=True (the pre-LN encoder of the large models) is not built here ({other})")
        if conv_bias:
            raise NotImplementedError(f"{who}: conv_bias=True is not built here ({other})")

    def __init__(self, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, conv_dim=(512,) * 7,
                 conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=128,
                 num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, output_layer=9, codebook_size=500, target_sample_hz=16000,
                 seq_len_multiple_of=None, feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False):
        super().__init__()
        who = self._NAME
        conv_dim, conv_kernel, conv_stride = tuple(conv_dim), tuple(conv_kernel), tuple(conv_stride)
        self._check_form(feat_extract_norm, do_stable_layer_norm, conv_bias)
        self.feat_extract_norm, self.do_stable_layer_norm, self.conv_bias = feat_extract_norm, bool(do_stable_layer_norm), bool(conv_bias)
        D, H, G, k = hidden_size, num_attention_heads, num_conv_pos_embedding_groups, num_conv_pos_embeddings
        if H < 1 or D != 64 * H:
            raise NotImplementedError(f"{who}: hidden_size / num_attention_heads must be 64, the head size the attention kernels serve (got {D} / {H})")
        if D % 64 or D > 2048:
            raise NotImplementedError(f"{who}: hidden_size must be a multiple of 64, at most 2048 (got {D})")
        if not (len(conv_dim) == len(conv_kernel) == len(conv_stride) >= 1):
            raise ValueError("conv_dim, conv_kernel and conv_stride must have one entry per convolution")
        C = conv_dim[0]
        if any(c != C for c in conv_dim) or C % 16 or not 16 <= C <= 512:
            raise NotImplementedError(f"{who}: conv_dim must be constant, a multiple of 16, at most 512 (got {conv_dim})")
        if not 1 <= conv_kernel[0] <= 16 or not 1 <= conv_stride[0] <= 16:
            raise NotImplementedError(f"{who}: conv_kernel[0] and conv_stride[0] must be at most 16 (got {conv_kernel[0]}, {conv_stride[0]})")
        if any(kk not in (2, 3) for kk in conv_kernel[1:]):
            raise NotImplementedError(f"{who}: conv_kernel after the first must be 2 or 3 (got {conv_kernel})")
        if any(s != 2 for s in conv_stride[1:]):
            raise NotImplementedError(f"{who}: conv_stride must be (s0, 2, 2, ...) (got {conv_stride})")
        if G < 1 or D % G or (D // G) % 8:
            raise NotImplementedError(f"{who}: hidden_size / num_conv_pos_embedding_groups must be a multiple of 8 (got {D} / {G})")
        if k < 2 or k % 2:
            raise NotImplementedError(f"{who}: num_conv_pos_embeddings must be even (got {k})")
        if (15 + k) * (D // G + 8) * 2 > _LDS_MAX:
            raise NotImplementedError(f"{who}: 16 positions of the positional convolution ({k} taps of {D // G} channels) do not fit the LDS")
        if not 2 <= codebook_size <= 4096:
            raise NotImplementedError(f"{who}: codebook_size must be in 2 .. 4096 (got {codebook_size})")
        if not 1 <= output_layer <= num_hidden_layers:
            raise NotImplementedError(f"{who}: output_layer must be in 1 .. num_hidden_layers = {num_hidden_layers} (got {output_layer})")
        if intermediate_size < 8 or intermediate_size % 8:
            raise NotImplementedError(f"{who}: intermediate_size must be a multiple of 8 (got {intermediate_size})")
        self.hidden_size, self.num_hidden_layers, self.num_attention_heads, self.intermediate_size = D, num_hidden_layers, H, intermediate_size
        self.conv_dim, self.conv_kernel, self.conv_stride = conv_dim, conv_kernel, conv_stride
        self.num_conv_pos_embeddings, self.num_conv_pos_embedding_groups, self.layer_norm_eps = k, G, float(layer_norm_eps)
        self.output_layer, self.codebook_size, self.target_sample_hz = output_layer, codebook_size, target_sample_hz
        self.seq_len_multiple_of, self.groups = seq_len_multiple_of, 1
        self.downsample_factor = math.prod(conv_stride)

        self.feature_extractor = _Box()
        self.feature_extractor.conv_layers = nn.ModuleList()
        cin = 1
        for i, kk in enumerate(conv_kernel):
            layer = _Box()
            layer.conv = _Box()
            layer.conv.weight = nn.Parameter(torch.randn(C, cin, kk) * math.sqrt(2.0 / (cin * kk)))
            if conv_bias:
                layer.conv.bias = nn.Parameter(torch.zeros(C))
            if i == 0 or feat_extract_norm == "layer":
                layer.layer_norm = _ln(C)
            self.feature_extractor.conv_layers.append(layer)
            cin = C
        self.feature_projection = _Box()
        self.feature_projection.layer_norm, self.feature_projection.projection = _ln(C), _linear(D, C)
        self.encoder = _Box()
        pce = _Box()
        pce.conv = _Box()
        pce.conv.bias = nn.Parameter(torch.zeros(D))
        pce.conv.parametrizations = _Box()
        pce.conv.parametrizations.weight = _Box()
        v = torch.randn(D, D // G, k) * (2.0 * math.sqrt(1.0 / (k * D)))
        pce.conv.parametrizations.weight.original0 = nn.Parameter(v.norm(dim=(0, 1), keepdim=True))  # [1, 1, k]: one norm per tap
        pce.conv.parametrizations.weight.original1 = nn.Parameter(v)
        self.encoder.pos_conv_embed = pce
        self.encoder.layer_norm = _ln(D)
        self.encoder.layers = nn.ModuleList()
        for _ in range(num_hidden_layers):
            l = _Box()
            l.attention = _Box()
            l.attention.q_proj, l.attention.k_proj, l.attention.v_proj, l.attention.out_proj = (_linear(D, D) for _ in range(4))
            l.layer_norm = _ln(D)
            l.feed_forward = _Box()
            l.feed_forward.intermediate_dense, l.feed_forward.output_dense = _linear(intermediate_size, D), _linear(D, intermediate_size)
            l.final_layer_norm = _ln(D)
            self.encoder.layers.append(l)
        self.register_buffer("cluster_centers", torch.randn(codebook_size, D))
        self.requires_grad_(False)
        self.eval()

    # -- state
    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = convert_state_dict(state_dict)
        sd.setdefault("cluster_centers", self.cluster_centers)  # a HuBERT state dict holds no codebook: the buffer stays
        return super().load_state_dict(sd, strict=strict, **kw)

    def set_cluster_centers(self, centers):
        c = torch.as_tensor(centers).detach().float()
        if tuple(c.shape) != (self.codebook_size, self.hidden_size):
            raise ValueError(f"{self._NAME}: cluster centres must be [{self.codebook_size}, {self.hidden_size}] (got {tuple(c.shape)})")
        self.cluster_centers = c.to(self.cluster_centers.device).contiguous()

    @classmethod
    def _form_of(cls, sd):
        """constructor keywords read off a converted state dict's KEYS; raises for a file of the other class"""
        for name, what in (("feature_extractor.conv_layers.0.conv.bias", "conv_bias=True"),
                           ("feature_extractor.conv_layers.1.layer_norm.weight", 'feat_extract_norm="layer"')):
            if name in sd:
                raise NotImplementedError(f"HubertWithKmeans: this state dict is of a model with {what}, which is not built here "
                                          f"(HubertLargeWithKmeans loads the large form)")
        return {}

    @classmethod
    def from_state_dict(cls, sd, cluster_centers, *, output_layer=9, conv_stride=None, target_sample_hz=16000, seq_len_multiple_of=None, **form):
        """A HuBERT state dict already in memory (any layout convert_state_dict takes) and cluster centres [K, D].  Every width is read
        off the shapes; the strides are not in a state dict (default (5, 2, 2, ...), the published models').  Further keywords go to
        the constructor."""
        sd = convert_state_dict(sd)
        n_conv = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("feature_extractor.conv_layers."))
        convs = [sd[f"feature_extractor.conv_layers.{i}.conv.weight"] for i in range(n_conv)]
        n_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
        D = sd["feature_projection.projection.weight"].shape[0]
        v = sd[_G1]
        cluster_centers = torch.as_tensor(cluster_centers)
        form = dict(cls._form_of(sd), **form)
        self = cls(hidden_size=D, num_hidden_layers=n_layers, num_attention_heads=max(D // 64, 1),
                   intermediate_size=sd["encoder.layers.0.feed_forward.intermediate_dense.weight"].shape[0],
                   conv_dim=tuple(w.shape[0] for w in convs), conv_kernel=tuple(w.shape[2] for w in convs),
                   conv_stride=tuple(conv_stride) if conv_stride is not None else (5,) + (2,) * (n_conv - 1),
                   num_conv_pos_embeddings=v.shape[2], num_conv_pos_embedding_groups=D // v.shape[1], output_layer=output_layer,
                   codebook_size=cluster_centers.shape[0], target_sample_hz=target_sample_hz, seq_len_multiple_of=seq_len_multiple_of,
                   **form)
        self.load_state_dict(sd)
        self.set_cluster_centers(cluster_centers)
        return self.eval()

    @classmethod
    def from_checkpoint(cls, checkpoint_path, kmeans_path, *, output_layer=9, conv_stride=None, target_sample_hz=16000, seq_len_multiple_of=None,
                        **form):
        """LOCAL files only: a torch.save'd state dict (transformers' or fairseq's names, or {'model': sd}) and the k-means file
        (load_kmeans)."""
        sd = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(sd, load_kmeans(kmeans_path), output_layer=output_layer, conv_stride=conv_stride,
                                   target_sample_hz=target_sample_hz, seq_len_multiple_of=seq_len_multiple_of, **form)

    # -- operand copies
    def _pack(self):
        """fp16 product operands and fp32 vectors as the launch sequence reads them, layers 1 .. output_layer only; kept per
        parameter version (PackedWeights)"""
        f = lambda t: t.detach().float().contiguous()
        h = lambda t: t.detach().float().half().contiguous()
        fe, fp, enc = self.feature_extractor.conv_layers, self.feature_projection, self.encoder
        D, k = self.hidden_size, self.num_conv_pos_embeddings
        convs = [h(l.conv.weight.permute(0, 2, 1).reshape(l.conv.weight.shape[0], -1)) for l in list(fe)[1:]]  # column tap * C + c
        pw = enc.pos_conv_embed.conv.parametrizations.weight
        g, v = pw.original0.detach().float(), pw.original1.detach().float()
        posw = v * (g / v.norm(dim=(0, 1), keepdim=True))  # weight norm at dim=2 folded in fp32, then rounded once
        layers = []
        for l in list(enc.layers)[:self.output_layer]:
            a, ff = l.attention, l.feed_forward
            layers.append(dict(
                wqkv=h(torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])), bqkv=f(torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias])),
                wo=h(a.out_proj.weight), bo=f(a.out_proj.bias), n1w=f(l.layer_norm.weight), n1b=f(l.layer_norm.bias),
                w1=h(ff.intermediate_dense.weight), b1=f(ff.intermediate_dense.bias), w2=h(ff.output_dense.weight), b2=f(ff.output_dense.bias),
                n2w=f(l.final_layer_norm.weight), n2b=f(l.final_layer_norm.bias)))
        return dict(w0=f(fe[0].conv.weight[:, 0, :]), gnw=f(fe[0].layer_norm.weight), gnb=f(fe[0].layer_norm.bias), convs=convs,
                    fplw=f(fp.layer_norm.weight), fplb=f(fp.layer_norm.bias), fpw=h(fp.projection.weight), fpb=f(fp.projection.bias),
                    posw=h(posw.permute(0, 2, 1).reshape(D, -1)), posb=f(enc.pos_conv_embed.conv.bias),
                    elw=f(enc.layer_norm.weight), elb=f(enc.layer_norm.bias), layers=layers)

    @staticmethod
    def _gemm(epi, M, N, K, A, B, C, bias, resid=None):
        d = _lib.GemmDesc()
        d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16 = _lib.VBX_GEMM_NT, epi, M, N, K, K, K, N, 1
        d.A, d.B, d.C, d.bias = A.data_ptr(), B.data_ptr(), C.data_ptr(), bias.data_ptr()
        d.resid = None if resid is None else resid.data_ptr()
        rc = _lib.lib().vbx_gemm(d, _lib.current_stream())
        if rc != 0:
            raise _lib.VbxError(f"vbx_gemm failed (rc={rc}): {_lib.lib().vbx_last_error().decode()}")

    def _products(self):
        """the matrix products of a call, name -> (epilogue, N, K, adds a residual): the one table both the launches (_product) and
        gemm_routes read"""
        C, D, I = self.conv_dim[0], self.hidden_size, self.intermediate_size
        return {"projection": (_lib.VBX_EPI_F32, D, C, False), "qkv": (_lib.VBX_EPI_F32, 3 * D, D, False),
                "out_proj": (_lib.VBX_EPI_F32, D, D, True), "intermediate": (_lib.VBX_EPI_GELU, I, D, False),
                "output": (_lib.VBX_EPI_F32, D, I, True)}

    def _product(self, name, M, A, B, C, bias, resid=None):
        epi, N, K, adds = self._products()[name]
        assert adds == (resid is not None), name
        self._gemm(epi, M, N, K, A, B, C, bias, resid=resid)

    def gemm_routes(self, rows):
        """vbx_gemm_route's answer for each product of a call with `rows` = batch * frames rows, in the order of _products().  A row
        of a batch under lens= is bit-equal to the row alone where both calls get the same answers (include/vbx.h, "ragged waves")."""
        out = []
        for epi, N, K, adds in self._products().values():
            d = _lib.GemmDesc()
            d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16 = _lib.VBX_GEMM_NT, epi, rows, N, K, K, K, N, 1
            d.A = d.B = d.C = d.bias = 4096  # the route looks at pointers for null and alignment only
            d.resid = 4096 if adds else None
            out.append(_lib.call_value("vbx_gemm_route", d))
        return tuple(out)

    def frames(self, samples):
        """frames of a wave of `samples` samples at target_sample_hz (0 or less: shorter than one frame)"""
        for k, s in zip(self.conv_kernel, self.conv_stride):
            samples = (samples - k) // s + 1 if samples >= k else 0
        return samples

    def min_samples(self):
        """the smallest sample count that gives one frame"""
        n = 1
        for k, s in zip(reversed(self.conv_kernel), reversed(self.conv_stride)):
            n = (n - 1) * s + k
        return n

    def frame_lens(self, lens):
        """frames of rows of that many samples at target_sample_hz: floored to seq_len_multiple_of as the wave is curtailed, then
        through the convolution chain.  A list, a CPU tensor or a device tensor; the same kind back."""
        m = self.seq_len_multiple_of

        def chain(l):
            if m is not None:
                l = l // m * m
            for k, s in zip(self.conv_kernel, self.conv_stride):
                l = (l - k) // s + 1
            return l
        return map_lens(lens, chain)

    def _target_lens(self, lens, B, T, resampled, input_sample_hz, device):
        """lens at the rate the wave [B, T] is given in -> int32 [B] on the device at target_sample_hz, curtailed like the wave, inside
        min_samples() .. the prepared wave's length: host values are checked (ValueError naming the row), a device tensor is clamped"""
        m = self.seq_len_multiple_of
        if resampled:
            lens, T = resample_lens(lens, input_sample_hz, self.target_sample_hz), resample_lens([T], input_sample_hz, self.target_sample_hz)[0]
        if m is not None:
            lens, T = map_lens(lens, lambda l: l // m * m), T // m * m
        if self.frames(T) < 1:
            raise NotImplementedError(f"{self._NAME}: a wave of {T} samples is shorter than one frame")
        return device_lens(lens, B, T, self.min_samples(), device, self._NAME)

    def _prepare(self, wave, input_sample_hz, attention_mask, lens=None):
        """-> (wave fp32 [B, T] at target_sample_hz, lens int32 [B] on the device at that rate, or None)"""
        if attention_mask is not None:
            raise NotImplementedError(f"{self._NAME}: an attention / padding mask is not served: rows of a batch are of equal length")
        if not isinstance(wave, torch.Tensor) or wave.ndim not in (2, 3) or (wave.ndim == 3 and wave.shape[1] != 1):
            raise ValueError(f"{self._NAME} takes a wave (batch, samples) or (batch, 1, samples)")
        if wave.ndim == 3:
            wave = wave[:, 0]
        resampled = input_sample_hz is not None and input_sample_hz != self.target_sample_hz
        lens_in = lens
        if lens is not None:  # checked (host values) or clamped (a device tensor) before anything else
            if resampled:
                lens_in = device_lens(lens, wave.shape[0], wave.shape[1], 1, wave.device, self._NAME)
            lens = self._target_lens(lens, wave.shape[0], wave.shape[1], resampled, input_sample_hz, wave.device)
        if wave.device.type != "cuda":
            raise _lib.VbxError(f"{self._NAME} runs only on an MI355X (gfx950) through libvbx_hip.so; the wave is on '{wave.device}'")
        wave = wave.detach().to(torch.float32)
        if resampled:
            from .codec import resample

            wave = resample(wave, input_sample_hz, self.target_sample_hz, lens=lens_in)
        if self.seq_len_multiple_of is not None:
            wave = wave[:, :wave.shape[1] // self.seq_len_multiple_of * self.seq_len_multiple_of]
        if self.frames(wave.shape[1]) < 1:
            raise NotImplementedError(f"{self._NAME}: a wave of {wave.shape[1]} samples is shorter than one frame")
        if self.cluster_centers.device != wave.device:
            self.to(wave.device)
        return wave.contiguous(), lens

    @torch.no_grad()
    def features(self, wav_input, input_sample_hz=None, attention_mask=None, lens=None):
        """lens: per-row sample counts of a padded batch at the rate the wave is given in (a list or CPU tensor is validated, a
        device tensor clamped; no host synchronisation): row b is the row alone -- bit-equal to features(wave[b:b+1, :len_b])[0] up to
        frame_lens(...)[b] frames, exactly 0.0 past them, whatever the padding holds."""
        return self._features(*self._prepare(wav_input, input_sample_hz, attention_mask, lens))[0]

    def _features(self, wave, lens=None):
        """-> (features fp32 [B, N, D], dead bool [B, N] -- the frames at or past each row's own count, zero-filled -- or None)"""
        w = self._cached(self._pack)
        st, dev, eps = _lib.current_stream(), wave.device, self.layer_norm_eps
        B, T = wave.shape
        C, D, H, I = self.conv_dim[0], self.hidden_size, self.num_attention_heads, self.intermediate_size
        f16 = lambda *s: torch.empty(*s, dtype=torch.float16, device=dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        k0, s0 = self.conv_kernel[0], self.conv_stride[0]
        L = (T - k0) // s0 + 1
        rec, stats = f32(B, _lib.lib().vbx_hubert_conv0_chunks(L), C, 3), f32(B, C, 2)
        a = f16(B, L, C)
        if lens is None:
            _lib.call("vbx_hubert_conv0_stats", wave, w["w0"], rec, stats, B, T, C, k0, s0, eps, st)
            _lib.call("vbx_hubert_conv0_apply", wave, w["w0"], stats, w["gnw"], w["gnb"], a, B, T, C, k0, s0, st)
        else:  # ragged waves (include/vbx.h): statistics over the row's own positions, zeros past them
            _lib.call("vbx_hubert_conv0_stats_lens", wave, lens, w["w0"], rec, stats, B, T, C, k0, s0, eps, st)
            _lib.call("vbx_hubert_conv0_apply_lens", wave, lens, w["w0"], stats, w["gnw"], w["gnb"], a, B, T, C, k0, s0, st)
            flens = self.frame_lens(lens).contiguous()  # int32 [B] on the device, 1 .. N
        for kk, wc in zip(self.conv_kernel[1:], w["convs"]):
            Lo = (L - kk) // 2 + 1
            y = f16(B, Lo, C)
            _lib.call("vbx_hubert_conv", a, wc, y, B, L, C, kk, st)
            a, L = y, Lo
        N, M = L, B * L
        a16 = f16(M, C)
        _lib.call("vbx_hubert_layernorm16", a, w["fplw"], w["fplb"], a16, M, C, eps, st)
        xa, xb, x16 = f32(M, D), f32(M, D), f16(M, D)  # the residual stream ping-pongs; x16: the operand copy of the current one
        self._product("projection", M, a16, w["fpw"], xa, w["fpb"])
        if lens is None:
            _lib.call("vbx_hubert_posconv", xa, w["posw"], w["posb"], xb, B, N, D, self.num_conv_pos_embedding_groups, self.num_conv_pos_embeddings, st)
        else:
            _lib.call("vbx_hubert_posconv_lens", xa, flens, w["posw"], w["posb"], xb, B, N, D, self.num_conv_pos_embedding_groups,
                      self.num_conv_pos_embeddings, st)
        _lib.call("vbx_hubert_layernorm", xb, w["elw"], w["elb"], xa, x16, M, D, eps, st)
        if not w["layers"]:
            return self._finish(xa.view(B, N, D), flens if lens is not None else None)
        qkv, q16, k16, v16 = f32(M, 3 * D), f16(B, H, N, 64), f16(B, H, N, 64), f16(B, H, N, 64)
        o16, lse, g16 = f16(M, D), f32(B, H, N), f16(M, I)
        scale = 64 ** -0.5
        pre = _lib.lib().vbx_attn_q_prescale(scale)
        for l in w["layers"]:
            self._product("qkv", M, x16, l["wqkv"], qkv, l["bqkv"])
            _lib.call("vbx_hubert_split_heads", qkv, q16, k16, v16, B, N, H, pre, st)
            if lens is None:
                _lib.call("vbx_attn_fwd", q16, k16, v16, None, o16, None, lse, B, H, N, scale, st)
            else:  # keys at or past the row's frames are never walked: live queries are those of the row alone
                _lib.call("vbx_attn_fwd_lens", q16, k16, v16, None, flens, o16, None, lse, B, H, N, scale, st)
            self._product("out_proj", M, o16, l["wo"], xb, l["bo"], resid=xa)
            _lib.call("vbx_hubert_layernorm", xb, l["n1w"], l["n1b"], xa, x16, M, D, eps, st)
            self._product("intermediate", M, x16, l["w1"], g16, l["b1"])
            self._product("output", M, g16, l["w2"], xb, l["b2"], resid=xa)
            _lib.call("vbx_hubert_layernorm", xb, l["n2w"], l["n2b"], xa, x16, M, D, eps, st)
        return self._finish(xa.view(B, N, D), flens if lens is not None else None)

    @staticmethod
    def _finish(h, flens):
        if flens is None:
            return h, None
        dead = torch.arange(h.shape[1], device=h.device)[None, :] >= flens[:, None]  # built once: forward fills the ids with it too
        return h.masked_fill_(dead[:, :, None], 0.0), dead

    def assign(self, feats):
        """vbx_kmeans_assign of features fp32 [.., D] -> int64 [..]"""
        if feats.device.type != "cuda":
            raise _lib.VbxError(f"{self._NAME} runs only on an MI355X (gfx950) through libvbx_hip.so; the features are on '{feats.device}'")
        if self.cluster_centers.device != feats.device:
            self.to(feats.device)
        h = feats.detach().to(torch.float32).contiguous()
        ids = torch.empty(h.shape[:-1], dtype=torch.int64, device=h.device)
        _lib.call("vbx_kmeans_assign", h, self.cluster_centers, ids, h.numel() // h.shape[-1], h.shape[-1], self.codebook_size, _lib.current_stream())
        return ids

    @torch.no_grad()
    def fit_kmeans(self, batches, n_clusters=None, init="k-means++", seed=0, input_sample_hz=None):
        """Fits the codebook on the device (kmeans.KMeans): per batch -- a wave batch or (waves, lens), lens as in features() --
        features(wave, lens=) -> KMeans.partial_fit(h, lens=frame lengths), one MiniBatchKMeans step at reassignment_ratio = 0; the
        first batch also initialises.  Then set_cluster_centers (codebook_size becomes n_clusters).  No host synchronisation; the
        KMeans comes back (counts_, inertia_)."""
        from .kmeans import KMeans

        K = self.codebook_size if n_clusters is None else n_clusters
        if not isinstance(K, int) or not 2 <= K <= 4096:
            raise NotImplementedError(f"{self._NAME}: codebook_size must be in 2 .. 4096 (got {K})")
        km = KMeans(K, self.hidden_size, init=init, seed=seed)
        resampled = input_sample_hz is not None and input_sample_hz != self.target_sample_hz
        for batch in batches:
            wave, lens = batch if isinstance(batch, (tuple, list)) else (batch, None)
            h = self.features(wave, input_sample_hz=input_sample_hz, lens=lens)
            if lens is not None:
                lens = self.frame_lens(resample_lens(lens, input_sample_hz, self.target_sample_hz) if resampled else lens)
            km.partial_fit(h, lens=lens)
        if km.cluster_centers_ is None:
            raise ValueError(f"{self._NAME}: fit_kmeans needs at least one batch")
        self.codebook_size = K
        self.set_cluster_centers(km.cluster_centers_)
        return km

    @torch.no_grad()
    def forward(self, wav_input, flatten=True, input_sample_hz=None, attention_mask=None, lens=None):
        """ids int64 [B, frames] (`flatten` is audiolm_pytorch's keyword: with groups = 1 both of its shapes are this one).  lens: as
        in features(); the ids at or past frame_lens(...)[b] are 0, a valid index of any embedding table."""
        wave, lens = self._prepare(wav_input, input_sample_hz, attention_mask, lens)
        h, dead = self._features(wave, lens)
        ids = self.assign(h)
        return ids if dead is None else ids.masked_fill_(dead, 0)


def normalize_wave(wave, lens=None, eps=1e-7):
    """Zero mean and unit variance per row on the device (vbx_wave_normalize): (x - mean) / sqrt(var + eps) with the biased variance,
    what transformers' Wav2Vec2FeatureExtractor(do_normalize=True) does to a wave (its eps is 1e-7).  wave fp32 [B, T] on the device.
    lens (a list or CPU tensor is validated, a device tensor clamped into 1 .. T): the statistics run over each row's own first
    lens[b] samples and the samples at or past them come back as 0, whatever they held.  The sums are shifted per chunk and combined in
    fp64: a DC offset costs nothing; the same bits on every run, and a row does not depend on its neighbours."""
    if not isinstance(wave, torch.Tensor) or wave.ndim != 2 or wave.shape[1] < 1:
        raise ValueError("normalize_wave takes a wave (batch, samples)")
    if not eps > 0:
        raise ValueError(f"normalize_wave: eps must be positive (got {eps})")
    B, T = wave.shape
    if lens is not None:
        lens = device_lens(lens, B, T, 1, wave.device, "normalize_wave")
    if wave.device.type != "cuda":
        raise _lib.VbxError(f"normalize_wave runs only on an MI355X (gfx950) through libvbx_hip.so; the wave is on '{wave.device}'")
    x = wave.detach().to(torch.float32).contiguous()
    y = torch.empty_like(x)
    chunks = -(-T // _lib.call_value("vbx_wave_normalize_chunk"))
    rec = torch.empty(B, chunks, 3, dtype=torch.float32, device=x.device)
    stats = torch.empty(B, 2, dtype=torch.float64, device=x.device)
    _lib.call("vbx_wave_normalize", x, lens, y, rec, stats, B, T, float(eps), _lib.current_stream())
    return y


class HubertLargeWithKmeans(HubertWithKmeans):
    """HubertWithKmeans for the LARGE form of HuBERT as transformers.HubertModel computes it (feat_extract_norm="layer",
    do_stable_layer_norm=True, conv_bias either way; the defaults are hubert-large-ll60k's): every convolution of the feature extractor
    is followed by its bias, LayerNorm over the channels of each position and erf-GELU -- no GroupNorm, no statistic over time --; the
    encoder is x + gelu(pos_conv(x)) with no LayerNorm after it, then per layer x + out_proj(attn(layer_norm(x))) and
    x + output_dense(gelu(intermediate_dense(final_layer_norm(x)))).  features() answers hidden_states[output_layer]: the
    un-normalised residual stream after that layer, and encoder.layer_norm of it only for output_layer == num_hidden_layers.

    The call shapes, lens=, frame_lens, fit_kmeans, assign, gemm_routes and the loaders are the base class's, and so is every limit but
    the three that name the form: here feat_extract_norm must be "layer" WITH do_stable_layer_norm=True (any other pair raises and names
    HubertWithKmeans); hidden_size / num_attention_heads == 64 stands, so x-large keeps raising.

    normalize_wave=True normalises the prepared wave (after resampling and seq_len_multiple_of, under lens= each row's own samples) to
    zero mean and unit variance on the device (normalize_wave(), eps = normalize_eps) before the first convolution.  hubert-large-ll60k
    WAS TRAINED ON NORMALISED WAVES (its preprocessor has do_normalize=True); the default is False only because audiolm_pytorch's
    module does not normalise.

    A state dict cannot say whether its encoder is pre-LN (the keys are the same): from_state_dict takes a file with per-layer
    convolution norms to have the pre-LN encoder, as every published such model does.  fairseq's large layout (bias at
    conv_layers.{i}.0.bias, the norm at conv_layers.{i}.2.1.*) is translated from memory of that library, which is absent: unpinned."""

    _NAME = "HubertLargeWithKmeans"

    @classmethod
    def _check_form(cls, feat_extract_norm, do_stable_layer_norm, conv_bias):
        if feat_extract_norm != "layer" or not do_stable_layer_norm:
            raise NotImplementedError(f'{cls._NAME}: serves feat_extract_norm="layer" with do_stable_layer_norm=True only (got '
                                      f'"{feat_extract_norm}", {bool(do_stable_layer_norm)}); HubertWithKmeans serves "group" with False, and '
                                      f"no model is published in a mixed form")

    def __init__(self, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, conv_dim=(512,) * 7,
                 conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_conv_pos_embeddings=128,
                 num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, output_layer=9, codebook_size=500, target_sample_hz=16000,
                 seq_len_multiple_of=None, feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, normalize_wave=False,
                 normalize_eps=1e-7):
        super().__init__(hidden_size=hidden_size, num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                         intermediate_size=intermediate_size, conv_dim=conv_dim, conv_kernel=conv_kernel, conv_stride=conv_stride,
                         num_conv_pos_embeddings=num_conv_pos_embeddings, num_conv_pos_embedding_groups=num_conv_pos_embedding_groups,
                         layer_norm_eps=layer_norm_eps, output_layer=output_layer, codebook_size=codebook_size,
                         target_sample_hz=target_sample_hz, seq_len_multiple_of=seq_len_multiple_of, feat_extract_norm=feat_extract_norm,
                         do_stable_layer_norm=do_stable_layer_norm, conv_bias=conv_bias)
        if not normalize_eps > 0:
            raise ValueError(f"{self._NAME}: normalize_eps must be positive (got {normalize_eps})")
        self.normalize_wave, self.normalize_eps = bool(normalize_wave), float(normalize_eps)

    @classmethod
    def _form_of(cls, sd):
        if "feature_extractor.conv_layers.1.layer_norm.weight" not in sd and "feature_extractor.conv_layers.0.conv.bias" in sd:
            raise ValueError(f"{cls._NAME}: this state dict has convolution biases but no feature_extractor.conv_layers.1.layer_norm "
                             f'(feat_extract_norm="group" with conv_bias=True): neither this class nor HubertWithKmeans serves that form')
        if "feature_extractor.conv_layers.1.layer_norm.weight" not in sd:
            raise ValueError(f"{cls._NAME}: this state dict has no feature_extractor.conv_layers.1.layer_norm: it is of the base form "
                             f'(feat_extract_norm="group"), which HubertWithKmeans loads')
        return dict(conv_bias="feature_extractor.conv_layers.0.conv.bias" in sd)

    def _pack(self):
        f = lambda t: t.detach().float().contiguous()
        w = super()._pack()
        fe = list(self.feature_extractor.conv_layers)
        w["cb"] = [f(l.conv.bias) if self.conv_bias else None for l in fe]
        w["lnw"], w["lnb"] = [f(l.layer_norm.weight) for l in fe], [f(l.layer_norm.bias) for l in fe]
        return w

    def _prepare(self, wave, input_sample_hz, attention_mask, lens=None):
        wave, lens = super()._prepare(wave, input_sample_hz, attention_mask, lens)
        if self.normalize_wave:
            wave = normalize_wave(wave, lens=lens, eps=self.normalize_eps)
        return wave, lens

    def _features(self, wave, lens=None):
        w = self._cached(self._pack)
        st, dev, eps = _lib.current_stream(), wave.device, self.layer_norm_eps
        B, T = wave.shape
        C, D, H, I = self.conv_dim[0], self.hidden_size, self.num_attention_heads, self.intermediate_size
        f16 = lambda *s: torch.empty(*s, dtype=torch.float16, device=dev)
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        k0, s0 = self.conv_kernel[0], self.conv_stride[0]
        L = (T - k0) // s0 + 1
        a = f16(B, L, C)
        # no statistic runs over time: under lens a frame inside a row's count reads only that row's own samples, so the plain
        # kernels run; what they make of the padding is dropped by vbx_hubert_posconv_lens and never enters a live frame
        _lib.call("vbx_hubert_conv0_ln", wave, w["w0"], w["cb"][0], w["lnw"][0], w["lnb"][0], a, B, T, C, k0, s0, eps, st)
        sums = None  # the fp32 intermediate of the layers that take the pair; the first of them is the largest
        for i, (kk, wc) in enumerate(zip(self.conv_kernel[1:], w["convs"]), 1):
            Lo = (L - kk) // 2 + 1
            y = f16(B, Lo, C)
            if _lib.call_value("vbx_hubert_conv_ln_route", B, L, C, kk):  # the same bits either way (include/vbx.h): speed only
                sums = f32(B * Lo * C) if sums is None else sums
                _lib.call("vbx_hubert_conv_f32", a, wc, w["cb"][i], sums, B, L, C, kk, st)
                _lib.call("vbx_hubert_ln_gelu", sums, w["lnw"][i], w["lnb"][i], y, B * Lo, C, eps, st)
            else:
                _lib.call("vbx_hubert_conv_ln", a, wc, w["cb"][i], w["lnw"][i], w["lnb"][i], y, B, L, C, kk, eps, st)
            a, L = y, Lo
        N, M = L, B * L
        flens = self.frame_lens(lens).contiguous() if lens is not None else None  # int32 [B] on the device, 1 .. N
        a16 = f16(M, C)
        _lib.call("vbx_hubert_layernorm16", a, w["fplw"], w["fplb"], a16, M, C, eps, st)
        xa, xb, x16 = f32(M, D), f32(M, D), f16(M, D)  # the residual stream ping-pongs; x16: the normalised operand of the next product
        self._product("projection", M, a16, w["fpw"], xa, w["fpb"])
        if lens is None:
            _lib.call("vbx_hubert_posconv", xa, w["posw"], w["posb"], xb, B, N, D, self.num_conv_pos_embedding_groups, self.num_conv_pos_embeddings, st)
        else:
            _lib.call("vbx_hubert_posconv_lens", xa, flens, w["posw"], w["posb"], xb, B, N, D, self.num_conv_pos_embedding_groups,
                      self.num_conv_pos_embeddings, st)
        xa, xb = xb, xa  # xa: the stream
        if w["layers"]:
            qkv, q16, k16, v16 = f32(M, 3 * D), f16(B, H, N, 64), f16(B, H, N, 64), f16(B, H, N, 64)
            o16, lse, g16 = f16(M, D), f32(B, H, N), f16(M, I)
            scale = 64 ** -0.5
            pre = _lib.lib().vbx_attn_q_prescale(scale)
        for l in w["layers"]:
            _lib.call("vbx_hubert_layernorm", xa, l["n1w"], l["n1b"], None, x16, M, D, eps, st)
            self._product("qkv", M, x16, l["wqkv"], qkv, l["bqkv"])
            _lib.call("vbx_hubert_split_heads", qkv, q16, k16, v16, B, N, H, pre, st)
            if lens is None:
                _lib.call("vbx_attn_fwd", q16, k16, v16, None, o16, None, lse, B, H, N, scale, st)
            else:
                _lib.call("vbx_attn_fwd_lens", q16, k16, v16, None, flens, o16, None, lse, B, H, N, scale, st)
            self._product("out_proj", M, o16, l["wo"], xb, l["bo"], resid=xa)
            _lib.call("vbx_hubert_layernorm", xb, l["n2w"], l["n2b"], None, x16, M, D, eps, st)
            self._product("intermediate", M, x16, l["w1"], g16, l["b1"])
            self._product("output", M, g16, l["w2"], xa, l["b2"], resid=xb)
        if self.output_layer == self.num_hidden_layers:  # hidden_states[n] alone carries encoder.layer_norm
            _lib.call("vbx_hubert_layernorm", xa, w["elw"], w["elb"], xb, None, M, D, eps, st)
            xa = xb
        return self._finish(xa.view(B, N, D), flens)
