"""DurationPredictor on the native kernels, inference and training.

Mirrors voicebox_pytorch.py:596-876 -- same constructor keywords, module tree and state-dict keys (`to_phoneme_emb`, `to_embed`,
`null_cond`, `conv_embed.dw_conv1d.0`, `transformer.*`, `to_pred.0`).

eval(): `forward` (:757-839), `forward_with_cond_scale` (:694-727) and `align_phoneme_ids_with_durations` (:689-692), the path the
sampler uses (:1231-1241).  Compute: vbx_pack_phoneme_input (embedding gather + condition masking / dropping / curtail_or_pad, fp16)
-> vbx_gemm (to_embed) -> vbx_convpos_fwd (+ residual) -> the native Transformer stack (plain RMSNorm, no registers) -> vbx_rowdot.

train(): `forward` returns the loss of :841-876, a 0-dim fp32 tensor on the device, and `loss.backward()` fills `.grad` of
`to_pred.0`, every `transformer.*` parameter, `conv_embed.dw_conv1d.0`, `to_embed`, `to_phoneme_emb.weight` (and `aligner.*`, see
below).  Two branches:
  * aligner branch -- all of `mel [B, T, dim_in], phoneme_len, mel_len, phoneme_mask, mel_mask` given (needs attach_aligner()):
    target = forward_aligner(phoneme_emb, phoneme_mask, mel, mel_mask)[0]; the phoneme embedding the aligner reads is the same
    differentiable tensor that feeds to_embed; a passed `target=` is ignored, as in the reference;
  * given durations -- none of the five given, `target=` [B, n] (any float or int dtype); no aligner needed.
  loss_mask = cond_mask & self_attn_mask; loss = mean_b( sum_n m |d - t| / max(sum_n m, 1e-5) ).
Two decisions:
  1. The L1 is taken on the PREDICTED durations d = to_pred(x).  The reference writes F.l1_loss(x, target) with x the hidden state
     [b, n, dim] against [b, n], which only broadcasts at degenerate shapes; this branch is therefore unpinned against the reference
     by construction, and its yardstick is the fp64 restatement tests/duration_train_ref.py.
  2. As in the reference, ForwardSumLoss(alignment_logprob, phoneme_len, mel_len) is added only with
     return_aligned_phoneme_ids=True.  With the default False the aligner receives NO gradient (alignment_hard is not
     differentiable) and its `.grad` stays None.
What raises instead of silently differing: some but not all of the five inputs (AssertionError, the reference's message); none of
them and no `target=` (NotImplementedError); the aligner branch without attach_aligner() (RuntimeError); `cond.shape[1] !=
phoneme_ids.shape[-1]` in training (ValueError: cond_mask & self_attn_mask cannot broadcast); `cond.requires_grad`
(NotImplementedError: the condition gets no gradient; null_cond has requires_grad=False and gets none either); CPU tensors (VbxError).
The path is three autograd nodes, each testable alone: _FrontEndFn (pack -> to_embed -> conv_embed + residual), the Transformer's
_StackFn, _HeadFn (to_pred + loss: csrc/duration.hip).  No host synchronisation in forward or backward; no atomics: the same seed
gives the same bits, the table gradient included.  ff_dropout / attn_dropout are live in train().  The activation arena of the
stand-alone Transformer holds ONE training forward per (B, n): run backward before the next training forward of the same shape.

Not built: `tokenizer` / `texts` (espeak phonemizer, third-party): pass `phoneme_ids`.

Codec latents (the reference's DurationPredictor(audio_enc_dec=codec), :627-630, :776).  The constructor keyword `audio_enc_dec` still
raises NotImplementedError -- two tests from before this path existed pin that -- and `attach_codec(codec)` serves it instead, as
attach_aligner() serves the aligner.  It checks the codec's members as VoiceBox does, sets `self.audio_enc_dec` (a submodule, as in
VoiceBox) and, when codec.latent_dim != dim, replaces `proj_in` by a trainable nn.Linear(latent_dim, dim) (state-dict keys
`proj_in.weight [dim, latent_dim]`, `proj_in.bias [dim]`, the reference's).  From then on `cond` is fp32 [B, S, latent_dim] -- latents;
as in the reference, forward never encodes audio, the wrapper does.  proj_in is applied FIRST (:776): the mask follows it, so a masked
row is 0 and not the bias; then the guidance drop; then curtail_or_pad, so rows past S are 0 even for a dropped sample.  One kernel
does all of it and the embedding gather: vbx_pack_phoneme_latent (csrc/duration.hip; fp16 operands, fp32 MFMA sums, the arithmetic of
vbx_proj_in_embed), fed by an fp16 pack of proj_in.weight that is cached per parameter version.  In train() the same launch writes the
bf16 operand `lcb` of the weight gradient (the latent row with a 1 in column latent_dim, zero on rows that pass no gradient), and
_FrontEndFn's backward adds three launches: d cond'' = de . W_embed[:, E:] (bf16), the split-K product d cond''^T . lcb, and
vbx_proj_in_wgrad_reduce, which splits it into d proj_in.weight and d proj_in.bias.  With latent_dim == dim proj_in stays nn.Identity()
and every path is the one without a codec, bit for bit.  No gradient reaches `cond`.

The aligner (align.py: `Aligner`, `maximum_path`, `ForwardSumLoss`) is optional.  By default `self.aligner` is None, `aligner.*`
entries of a reference checkpoint are skipped on load and `state_dict()` has no such keys.  `attach_aligner()` builds
`Aligner(dim_hidden=dim_phoneme_emb, **aligner_kwargs)` (or takes a given one); from then on `aligner.*` keys are loaded and saved,
`forward_aligner` (:730-754) returns the reference's four alignment tensors, and `align_phoneme_ids(mel, phoneme_ids)` gives the
frame-aligned phoneme ids that a text-conditioned VoiceBox takes as `cond_token_ids`.  Its parameters are ordinary parameters of
this module once attached.
"""
from random import random

import torch
from torch import nn

from . import _lib
from ._packing import tensors_key
from .align import Aligner, forward_sum_loss, maximum_path
from .masks import mask_from_frac_lengths, prob_mask_like, take_draw
from .model import ConvPositionEmbed, Transformer, exists


def generate_mask_from_repeats(repeats):
    """naturalspeech2_pytorch's helper (third-party, call site voicebox_pytorch.py:690): repeats (b, i) -> bool (b, i, j) with
    entry set when output position j lies in phoneme i's span [cumsum_i - repeats_i, cumsum_i); j < the longest total."""
    repeats = repeats.int()
    cumsum = repeats.cumsum(dim=-1)
    start = cumsum - repeats
    total = int(cumsum[..., -1].amax().item())
    pos = torch.arange(total, device=repeats.device)
    return (pos >= start[..., None]) & (pos < cumsum[..., None])


class DurationPredictor(nn.Module):
    def __init__(self, *, audio_enc_dec=None, tokenizer=None, num_phoneme_tokens=None, dim_phoneme_emb=512, dim=512, depth=10,
                 dim_head=64, heads=8, ff_mult=4, ff_dropout=0., conv_pos_embed_kernel_size=31, conv_pos_embed_groups=None,
                 attn_dropout=0, attn_flash=False, attn_qk_norm=True, use_gateloop_layers=False, p_drop_prob=0.2,
                 frac_lengths_mask=(0.1, 1.), aligner_kwargs: dict = dict(dim_in=80, attn_channels=80)):
        super().__init__()
        if exists(audio_enc_dec):
            raise NotImplementedError("DurationPredictor(audio_enc_dec=...) is not served by the constructor: build the predictor "
                                      "without it and call attach_codec(codec), then feed latents [B, S, codec.latent_dim]")
        assert not (exists(tokenizer) and exists(num_phoneme_tokens)), \
            'if a phoneme tokenizer was passed into duration module, number of phoneme tokens does not need to be specified'
        if exists(tokenizer) or not exists(num_phoneme_tokens):
            raise NotImplementedError("the espeak phoneme Tokenizer is third-party: pass num_phoneme_tokens and call with phoneme_ids")
        if dim_phoneme_emb % 8 != 0:
            raise NotImplementedError("dim_phoneme_emb must be a multiple of 8 (vectorised embedding gather)")
        # ff_dropout / attn_dropout go to the Transformer as in the reference (:631-642): the identity in eval mode, live in train()
        # (the stack's own dropout, seeded from torch's generator)
        self.audio_enc_dec = None
        self.proj_in = nn.Identity()
        self.tokenizer = None
        self.to_phoneme_emb = nn.Embedding(num_phoneme_tokens, dim_phoneme_emb)
        self.p_drop_prob = p_drop_prob
        self.frac_lengths_mask = frac_lengths_mask
        self.to_embed = nn.Linear(dim + dim_phoneme_emb, dim)
        self.null_cond = nn.Parameter(torch.zeros(dim), requires_grad=False)
        self.conv_embed = ConvPositionEmbed(dim=dim, kernel_size=conv_pos_embed_kernel_size, groups=conv_pos_embed_groups)
        self.transformer = Transformer(dim=dim, depth=depth, dim_head=dim_head, heads=heads, ff_mult=ff_mult, ff_dropout=ff_dropout,
                                       attn_dropout=attn_dropout, attn_flash=attn_flash, attn_qk_norm=attn_qk_norm,
                                       use_gateloop_layers=use_gateloop_layers)
        self.to_pred = nn.Sequential(nn.Linear(dim, 1), nn.Identity())  # [1]: Rearrange('... 1 -> ...'), done by vbx_rowdot
        self.dim, self.dim_phoneme_emb, self.ksize = dim, dim_phoneme_emb, conv_pos_embed_kernel_size
        self.aligner_kwargs = dict(aligner_kwargs)
        self.aligner = None  # attach_aligner(): Aligner(dim_hidden=dim_phoneme_emb, **aligner_kwargs)
        self.align_loss = None
        self._proj_pack = (None, None)  # (key of proj_in.weight, its fp16 pack [dim, Kp])

    @property
    def device(self):
        return next(self.parameters()).device

    def load_state_dict(self, state_dict, strict=True, **kw):
        if self.aligner is not None:
            return super().load_state_dict(state_dict, strict=strict, **kw)
        kept = {k: v for k, v in state_dict.items() if not k.startswith("aligner.")}
        return super().load_state_dict(kept, strict=strict, **kw)

    def attach_aligner(self, aligner=None):
        """Gives this module its aligner: the given one, or Aligner(dim_hidden=dim_phoneme_emb, **aligner_kwargs) on the device of
        the parameters.  From then on `aligner.*` keys are part of state_dict() and are loaded.  Returns the aligner."""
        if aligner is None:
            aligner = Aligner(dim_hidden=self.dim_phoneme_emb, **self.aligner_kwargs).to(self.device)
        elif not isinstance(aligner, Aligner):
            raise TypeError(f"attach_aligner takes a voicebox_pytorch_amd.Aligner (got {type(aligner).__name__})")
        elif aligner.dim_hidden != self.dim_phoneme_emb:
            raise ValueError(f"attach_aligner: the aligner's dim_hidden ({aligner.dim_hidden}) must be dim_phoneme_emb "
                             f"({self.dim_phoneme_emb})")
        self.aligner = aligner
        return aligner

    def attach_codec(self, codec):
        """Gives this module its audio codec (the reference's constructor keyword audio_enc_dec, :627-630): any nn.Module with
        encode / decode / latent_dim / sampling_rate / downsample_factor, the check VoiceBox makes.  With codec.latent_dim != dim,
        proj_in becomes a trainable nn.Linear(latent_dim, dim) (torch's default initialisation, on the device of the parameters) and
        `cond` is from then on fp32 [B, S, latent_dim]; with latent_dim == dim nothing else changes.  Returns self."""
        missing = [n for n in ("encode", "decode", "latent_dim", "sampling_rate", "downsample_factor") if not hasattr(codec, n)]
        if not isinstance(codec, nn.Module) or missing:
            raise TypeError(f"attach_codec takes an nn.Module with encode / decode / latent_dim / sampling_rate / downsample_factor "
                            f"(missing: {missing})")
        latent_dim = int(codec.latent_dim)
        if latent_dim != self.dim and not 8 <= latent_dim <= 1024:
            raise NotImplementedError(f"attach_codec: codec.latent_dim must be dim ({self.dim}) or in 8 .. 1024 (got {latent_dim})")
        if exists(self.audio_enc_dec) and latent_dim != self.latent_dim:
            raise ValueError(f"attach_codec: a codec of latent width {self.latent_dim} is attached already; one of width {latent_dim} "
                             "would change proj_in's shape")
        if latent_dim != self.dim and not isinstance(self.proj_in, nn.Linear):
            self.proj_in = nn.Linear(latent_dim, self.dim).to(self.device)
        self.audio_enc_dec = codec
        return self

    @property
    def latent_dim(self):
        """width of `cond`: the attached codec's latent_dim, or dim"""
        return self.proj_in.in_features if isinstance(self.proj_in, nn.Linear) else self.dim

    def _proj_operands(self):
        """(fp16 pack of proj_in.weight [dim, Kp], zero past column latent_dim; bias fp32 [dim]) -- the pack is rebuilt when the
        weight's storage or version counter moved (optimizer step, load_state_dict, .to())"""
        w = self.proj_in.weight
        key = tensors_key((w,))
        if key != self._proj_pack[0]:
            L, D = self.latent_dim, self.dim
            Kp = _lib.lib().vbx_proj_in_kp(L)
            pack = torch.empty(D, Kp, dtype=torch.float16, device=w.device)
            _lib.call("vbx_pack_weight", w.detach().float().contiguous(), D, L, None, pack, D, Kp, 0, 0, _lib.current_stream())
            self._proj_pack = (key, pack)
        return self._proj_pack[1], self.proj_in.bias.detach().float().contiguous()

    def _need_aligner(self, who):
        if self.aligner is None:
            raise RuntimeError(f"DurationPredictor.{who} needs an aligner: call attach_aligner() first")

    def forward_aligner(self, x, x_mask, y, y_mask):  # voicebox_pytorch.py:730-754
        """x [B, Tx, dim_phoneme_emb] phoneme embeddings, x_mask [B, 1, Tx], y [B, Ty, dim_in] mel, y_mask [B, 1, Ty] ->
        (alignment_hard fp32 [B, Tx], alignment_soft [B, Tx, Ty], alignment_logprob [B, 1, Ty, Tx], alignment_mas [B, Tx, Ty]).
        alignment_soft and alignment_mas are transposed views of the aligner's map and of maximum_path's path.  The masks must be
        PREFIX masks (real entries first): the search takes the lengths, the masks' sums, which stay on the device.  The soft map
        and the log-probabilities are differentiable; the hard alignment is not."""
        self._need_aligner("forward_aligner")
        soft, logprob = self.aligner(y.transpose(1, 2), x, x_mask)
        key_lens = (x_mask.reshape(x_mask.shape[0], -1) != 0).sum(-1)
        query_lens = (y_mask.reshape(y_mask.shape[0], -1) != 0).sum(-1)
        path, durations = maximum_path(soft, query_lens, key_lens)
        return durations.float(), soft[:, 0].transpose(1, 2), logprob, path[:, 0].transpose(1, 2)

    def align_phoneme_ids(self, mel, phoneme_ids, phoneme_len=None, mel_len=None):
        """mel [B, dim_in, T] and phoneme_ids [B, K] (-1 = padding) -> the phoneme id of every mel frame, int64 [B, frames]:
        embedding -> aligner.align -> align_phoneme_ids_with_durations.  phoneme_len / mel_len int [B] on the device (None: the
        count of ids != -1 / T).  This is what VoiceBox(condition_on_text=True) takes as cond_token_ids."""
        self._need_aligner("align_phoneme_ids")
        with torch.no_grad():
            ids = phoneme_ids.to(self.device, torch.long)
            if phoneme_len is None:
                phoneme_len = (ids != -1).sum(-1)
            emb = self.to_phoneme_emb(ids.clamp(min=0))
            durations, _ = self.aligner.align(mel, emb, key_lens=phoneme_len, query_lens=mel_len)
            return self.align_phoneme_ids_with_durations(ids.clamp(min=0), durations)

    def align_phoneme_ids_with_durations(self, phoneme_ids, durations):  # voicebox_pytorch.py:689-692
        repeat_mask = generate_mask_from_repeats(durations.clamp(min=1))
        # einsum('b i, b i j -> b j') of the reference: every output position belongs to at most one phoneme
        return torch.einsum('bi,bij->bj', phoneme_ids.float(), repeat_mask.float()).long()

    @torch.inference_mode()
    def forward_with_cond_scale(self, *args, texts=None, phoneme_ids=None, cond_scale=1., return_aligned_phoneme_ids=False,
                                **kwargs):  # voicebox_pytorch.py:694-727
        if exists(texts):
            raise NotImplementedError("texts need the espeak Tokenizer (third-party): pass phoneme_ids")
        fk = dict(return_aligned_phoneme_ids=False, phoneme_ids=phoneme_ids)
        durations = self.forward(*args, cond_drop_prob=0., **fk, **kwargs)
        if cond_scale != 1.:
            null_durations = self.forward(*args, cond_drop_prob=1., **fk, **kwargs)
            durations = null_durations + (durations - null_durations) * cond_scale
        if not return_aligned_phoneme_ids:
            return durations
        return durations, self.align_phoneme_ids_with_durations(phoneme_ids.to(durations.device), durations)

    def _resolve(self, cond, phoneme_ids, cond_mask, cond_drop_prob, self_attn_mask):
        """The shared host part of :774-809 on the device of the parameters: (cond fp32, ids, cond_mask bool, its uint8 copy, the
        classifier-free-guidance drop uint8 or None, self_attn_mask bool, its uint8 copy).  No host synchronisation."""
        dev = self.device
        cond = cond.detach().to(dev, torch.float32).contiguous()
        batch, seq_len, cond_dim = cond.shape
        assert cond_dim == self.latent_dim, \
            (f"cond has width {cond_dim}, this DurationPredictor takes {self.latent_dim}" +
             (" (the attached codec's latent_dim)" if exists(self.audio_enc_dec) else
              f" (dim): for codec latents of another width call attach_codec(codec) first"))
        ids = phoneme_ids.to(dev, torch.long).contiguous()
        assert ids.ndim == 2 and ids.shape[0] == batch
        if not exists(cond_mask):  # :786-791
            coin = take_draw("coin")
            if (random() < 0.5) if coin is None else bool(coin):
                frac = take_draw("frac_lengths")
                if frac is None:
                    frac = torch.zeros((batch,), device=dev).float().uniform_(*self.frac_lengths_mask)
                cond_mask = mask_from_frac_lengths(seq_len, frac.to(dev))
            else:
                cond_mask = prob_mask_like((batch, seq_len), self.p_drop_prob, dev)
        cond_mask = cond_mask.to(dev)
        cmask = cond_mask.to(torch.uint8).contiguous()
        drop = None
        if cond_drop_prob > 0.:  # :797-804
            drop = take_draw("cond_drop")
            drop = prob_mask_like((batch,), cond_drop_prob, dev) if drop is None else drop.to(dev)
            drop = drop.to(torch.uint8).contiguous()
        if not exists(self_attn_mask):
            self_attn_mask = ids != -1  # :808-809 (phoneme id -1 is padding)
        amask = self_attn_mask.to(dev).to(torch.bool)
        return cond, ids, cond_mask, cmask, drop, amask, amask.to(torch.uint8).contiguous()

    def forward(self, *, cond, texts=None, phoneme_ids=None, cond_drop_prob=0., target=None, cond_mask=None, mel=None,
                phoneme_len=None, mel_len=None, phoneme_mask=None, mel_mask=None, self_attn_mask=None,
                return_aligned_phoneme_ids=False):  # voicebox_pytorch.py:757-876
        """eval mode: the durations fp32 [B, n] (and the frame-aligned ids with return_aligned_phoneme_ids).  train mode: the loss,
        a 0-dim fp32 tensor on the device (see the module docstring for the two branches and what raises)."""
        if exists(texts) or not exists(phoneme_ids):
            raise NotImplementedError("texts need the espeak Tokenizer (third-party): pass phoneme_ids")
        if self.training:
            return self._forward_train(cond, phoneme_ids, cond_drop_prob, target, cond_mask, mel, phoneme_len, mel_len, phoneme_mask,
                                       mel_mask, self_attn_mask, return_aligned_phoneme_ids)
        dev = self.device
        if dev.type != "cuda":
            raise _lib.VbxError("DurationPredictor compute runs only on an MI355X (gfx950) through libvbx_hip.so; "
                                f"parameters are on '{dev}' and there is no CPU fallback")
        with torch.no_grad():
            cond, ids, _, cmask, drop, amask, am8 = self._resolve(cond, phoneme_ids, cond_mask, cond_drop_prob, self_attn_mask)
            batch, seq_len, _ = cond.shape
            n = ids.shape[-1]
            E, D = self.dim_phoneme_emb, self.dim
            st = _lib.current_stream()
            packed = torch.empty(batch * n, E + D, dtype=torch.float16, device=dev)
            table, null = self.to_phoneme_emb.weight.detach().float().contiguous(), self.null_cond.detach().float().contiguous()
            if isinstance(self.proj_in, nn.Linear):  # :776 + :793-823 in one launch
                pw16, pb = self._proj_operands()
                _lib.call("vbx_pack_phoneme_latent", ids, table, E, cond, seq_len, self.latent_dim, pw16, pb, cmask, drop, null, packed,
                          batch, n, D, st)
            else:
                _lib.call("vbx_pack_phoneme_input", ids, table, E, cond, seq_len, cmask, drop, null, packed, batch, n, D, st)
            w16 = self.to_embed.weight.detach().to(torch.float16).contiguous()
            bias = self.to_embed.bias.detach().float().contiguous()
            e = torch.empty(batch * n, D, dtype=torch.float32, device=dev)
            _gemm(_lib.VBX_GEMM_NT, _lib.VBX_EPI_F32, batch * n, D, E + D, packed, E + D, w16, E + D, e, D, bias=bias, f16=1)  # :823-824
            conv = self.conv_embed.dw_conv1d[0]
            x = torch.empty(batch, n, D, dtype=torch.float32, device=dev)
            _lib.call("vbx_convpos_fwd", e, conv.weight.detach().float().contiguous(), conv.bias.detach().float().contiguous(), am8,
                      None, x, batch, n, 0, D, self.ksize, st)  # conv_embed(x, mask) + x (:826)
            hid = self.transformer(x, mask=amask).contiguous()  # :828-831
            pred = self.to_pred[0]
            durations = torch.empty(batch, n, dtype=torch.float32, device=dev)
            _lib.call("vbx_rowdot", hid, pred.weight.detach().float().contiguous(), pred.bias.detach().float().contiguous(), durations,
                      batch * n, D, st)  # :833
        if not return_aligned_phoneme_ids:
            return durations
        return durations, self.align_phoneme_ids_with_durations(ids.clamp(min=0), durations)  # ids clamped as :811 does before :839

    def _forward_train(self, cond, phoneme_ids, cond_drop_prob, target, cond_mask, mel, phoneme_len, mel_len, phoneme_mask, mel_mask,
                       self_attn_mask, return_aligned_phoneme_ids):  # voicebox_pytorch.py:841-876
        five = (mel, phoneme_len, mel_len, phoneme_mask, mel_mask)
        given = sum(exists(el) for el in five)
        assert given in (0, 5), \
            'need to pass phoneme_len, mel_len, phoneme_mask, mel_mask, to train duration predictor module'
        use_aligner = given == 5
        if not use_aligner and not exists(target):
            raise NotImplementedError("DurationPredictor training needs its targets: pass target= (durations [B, n]), or attach an "
                                      "aligner (attach_aligner()) and pass mel, phoneme_len, mel_len, phoneme_mask and mel_mask")
        if use_aligner:
            self._need_aligner("forward (training on the aligner's durations)")
        if cond.ndim != 3 or phoneme_ids.ndim != 2 or cond.shape[1] != phoneme_ids.shape[-1]:
            raise ValueError("DurationPredictor training: cond [B, n, dim or latent_dim] must have the length of phoneme_ids [B, n] (got "
                             f"{tuple(cond.shape)} and {tuple(phoneme_ids.shape)}): the loss mask is cond_mask & self_attn_mask")
        if cond.requires_grad:
            raise NotImplementedError("DurationPredictor training passes no gradient to cond: detach it")
        dev = self.device
        if dev.type != "cuda":
            raise _lib.VbxError("DurationPredictor compute runs only on an MI355X (gfx950) through libvbx_hip.so; "
                                f"parameters are on '{dev}' and there is no CPU fallback")
        cond, ids, cond_mask, cmask, drop, amask, am8 = self._resolve(cond, phoneme_ids, cond_mask, cond_drop_prob, self_attn_mask)
        batch, n = ids.shape
        conv, pred = self.conv_embed.dw_conv1d[0], self.to_pred[0]
        proj = (self.proj_in.weight, self.proj_in.bias) if isinstance(self.proj_in, nn.Linear) else ()
        x, emb = _FrontEndFn.apply(self, ids, cond, cmask, drop, am8, use_aligner, self.to_phoneme_emb.weight, self.to_embed.weight,
                                   self.to_embed.bias, conv.weight, conv.bias, *proj)
        hid = self.transformer(x, mask=amask)  # :828-831 (_StackFn)
        align_loss = None
        if use_aligner:  # :847-848; a passed target= is overwritten there and never read
            target, _, logprob, _ = self.forward_aligner(emb, phoneme_mask.to(dev), mel.to(dev), mel_mask.to(dev))
            if return_aligned_phoneme_ids:  # :868-874: only then does the aligner receive a gradient
                align_loss = forward_sum_loss(logprob, phoneme_len.to(dev), mel_len.to(dev))
        else:
            target = target.detach().to(dev)
            if target.shape != (batch, n):
                raise ValueError(f"DurationPredictor training: target must be [B, n] = {(batch, n)} (got {tuple(target.shape)})")
        loss_mask = (cond_mask.to(torch.bool) & amask).to(torch.uint8).contiguous()  # :851
        loss = _HeadFn.apply(hid, pred.weight, pred.bias, target.to(torch.float32).contiguous(), loss_mask)
        return loss if align_loss is None else loss + align_loss


def _gemm(mode, epi, M, N, K, A, lda, B, ldb, C, ldc, bias=None, f16=0, splits=0):
    d = _lib.GemmDesc()
    d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16, d.splits = mode, epi, M, N, K, lda, ldb, ldc, f16, splits
    d.A, d.B, d.C, d.bias = A.data_ptr(), B.data_ptr(), C.data_ptr(), None if bias is None else bias.data_ptr()
    rc = _lib.lib().vbx_gemm(d, _lib.current_stream())
    if rc != 0:
        raise _lib.VbxError(f"vbx_gemm failed (rc={rc}): {_lib.lib().vbx_last_error().decode()}")


class _FrontEndFn(torch.autograd.Function):
    """pack -> to_embed -> conv_embed + residual (:811-826) as one node.  Outputs x [B, n, D] and, when asked, the phoneme embedding
    [B, n, E] that the aligner reads: the same rows that sit in columns 0:E of the packed operand, so the table gradient is one
    deterministic sum over both consumers (vbx_phoneme_emb_bwd).  cond and null_cond receive no gradient.  With proj_in a Linear
    (attach_codec) its weight and bias are two more inputs: the pack is vbx_pack_phoneme_latent_train, and the backward also forms
    d cond'' and, from it and the pack's lcb operand, d proj_in.weight / d proj_in.bias."""

    @staticmethod
    def forward(ctx, mod, ids, cond, cmask, drop, am8, want_emb, table, we, be, cw, cb, pw=None, pb=None):
        dev, st = ids.device, _lib.current_stream()
        B, n = ids.shape
        E, D, M = mod.dim_phoneme_emb, mod.dim, B * n
        table32 = table.detach().float().contiguous()
        packed = torch.empty(M, E + D, dtype=torch.float16, device=dev)
        packed_b = torch.empty(M, E + D, dtype=torch.bfloat16, device=dev)
        emb = torch.empty(B, n, E, dtype=torch.float32, device=dev) if want_emb else None
        null, lcb, L = mod.null_cond.detach().float().contiguous(), None, 0
        if pw is not None:
            L = pw.shape[1]
            pw16, pb32 = mod._proj_operands()
            lcb = torch.empty(M, pw16.shape[1], dtype=torch.bfloat16, device=dev)
            _lib.call("vbx_pack_phoneme_latent_train", ids, table32, E, cond, cond.shape[1], L, pw16, pb32, cmask, drop, null, packed,
                      packed_b, emb, lcb, B, n, D, st)
        else:
            _lib.call("vbx_pack_phoneme_input_train", ids, table32, E, cond, cond.shape[1], cmask, drop, null, packed, packed_b, emb,
                      B, n, D, st)
        e = torch.empty(M, D, dtype=torch.float32, device=dev)
        _gemm(_lib.VBX_GEMM_NT, _lib.VBX_EPI_F32, M, D, E + D, packed, E + D, we.detach().to(torch.float16).contiguous(), E + D, e, D,
              bias=be.detach().float().contiguous(), f16=1)
        cw32, cb32 = cw.detach().float().contiguous(), cb.detach().float().contiguous()
        x = torch.empty(B, n, D, dtype=torch.float32, device=dev)
        _lib.call("vbx_convpos_fwd", e, cw32, cb32, am8, None, x, B, n, 0, D, mod.ksize, st)
        ctx.save_for_backward(ids, am8, packed_b, e, cw32, cb32, we, lcb)
        ctx.dims = (B, n, E, D, mod.ksize, table.shape[0])
        ctx.latent = L  # 0: proj_in is the identity, and forward took 12 inputs
        ctx.set_materialize_grads(False)
        return x, emb

    @staticmethod
    def backward(ctx, gx, gemb):
        ids, am8, packed_b, e, cw32, cb32, we, lcb = ctx.saved_tensors
        B, n, E, D, ks, V = ctx.dims
        M, dev, st = B * n, ids.device, _lib.current_stream()
        L = ctx.latent
        if gx is None and gemb is None:
            return (None,) * (14 if L else 12)
        dwe = dbe = dcw = dcb = dpk = dpw = dpb = None
        if gx is not None:
            chunks = _lib.lib().vbx_convpos_bwd_chunks(B, n)
            dpre = torch.empty(M, D, dtype=torch.float32, device=dev)
            de = torch.empty(M, D, dtype=torch.float32, device=dev)
            deb = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
            wpart = torch.zeros(chunks, D, 64, dtype=torch.float32, device=dev)
            _lib.call("vbx_convpos_bwd", e, cw32, cb32, am8, gx.to(torch.float32).contiguous(), dpre, de, deb, wpart, None, B, n, 0, D,
                      ks, st)
            dcw = torch.empty(cw32.shape, dtype=torch.float32, device=dev)
            dcb = torch.empty(D, dtype=torch.float32, device=dev)
            _lib.call("vbx_conv_wgrad_finalize", wpart, chunks, D, ks, dcw, dcb, st)
            dbe = torch.empty(D, dtype=torch.float32, device=dev)
            scratch = torch.empty(_lib.lib().vbx_colsum_scratch_floats(M, D), dtype=torch.float32, device=dev)
            _lib.call("vbx_colsum_f32", de, M, D, D, dbe, scratch, st)
            splits = max(1, min(8, M // 256))  # every split keeps rows, as the aligner's weight gradients
            slabs = torch.empty(splits, D, E + D, dtype=torch.float32, device=dev)
            _gemm(_lib.VBX_GEMM_TN, _lib.VBX_EPI_SPLITK, D, E + D, M, deb, D, packed_b, E + D, slabs, E + D, splits=splits)
            dwe = torch.empty(D, E + D, dtype=torch.float32, device=dev)
            _lib.call("vbx_splitk_reduce", slabs, splits, D, E + D, dwe, D, E + D, E + D, 0, 0, 0, st)
            web = we.detach().to(torch.bfloat16).contiguous() if (ctx.needs_input_grad[7] or L) else None
            if ctx.needs_input_grad[7]:  # d(packed)[:, 0:E]: the table's columns
                dpk = torch.empty(M, E, dtype=torch.float32, device=dev)
                _gemm(_lib.VBX_GEMM_NN, _lib.VBX_EPI_F32, M, E, D, deb, D, web, E + D, dpk, E)
            if L:  # d cond'' = de . W_embed[:, E:E+D] (bf16), then [ d proj_in.weight | d proj_in.bias ] = d cond''^T . lcb
                Kp = lcb.shape[1]
                dcond = torch.empty(M, D, dtype=torch.bfloat16, device=dev)
                _gemm(_lib.VBX_GEMM_NN, _lib.VBX_EPI_BF16, M, D, D, deb, D, web[:, E:], E + D, dcond, D)
                pslabs = torch.empty(splits, D, Kp, dtype=torch.float32, device=dev)
                _gemm(_lib.VBX_GEMM_TN, _lib.VBX_EPI_SPLITK, D, Kp, M, dcond, D, lcb, Kp, pslabs, Kp, splits=splits)
                dpw = torch.empty(D, L, dtype=torch.float32, device=dev)
                dpb = torch.empty(D, dtype=torch.float32, device=dev)
                _lib.call("vbx_proj_in_wgrad_reduce", pslabs, splits, D, L, dpw, dpb, st)
        gtable = None
        if ctx.needs_input_grad[7] and (dpk is not None or gemb is not None):
            gtable = torch.empty(V, E, dtype=torch.float32, device=dev)
            ge = None if gemb is None else gemb.to(torch.float32).contiguous()
            _lib.call("vbx_phoneme_emb_bwd", ids, dpk, E, ge, gtable, M, V, E, st)
        out = (None, None, None, None, None, None, None, gtable, dwe, dbe, dcw, dcb)
        return out + (dpw, dpb) if L else out


class _HeadFn(torch.autograd.Function):
    """to_pred + the masked L1 of :858-866 on the predicted durations: vbx_duration_head_fwd / _bwd."""

    @staticmethod
    def forward(ctx, hid, w, b, target, m8):
        B, n, D = hid.shape
        dev, st = hid.device, _lib.current_stream()
        hid = hid.detach().to(torch.float32).contiguous()
        w32, b32 = w.detach().float().contiguous(), b.detach().float().contiguous()
        durations = torch.empty(B, n, dtype=torch.float32, device=dev)
        num, den = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.call("vbx_duration_head_fwd", hid, w32, b32, target, m8, durations, num, den, loss, B, n, D, st)
        ctx.save_for_backward(hid, w32, durations, target, m8, den)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        hid, w32, durations, target, m8, den = ctx.saved_tensors
        B, n, D = hid.shape
        dev = hid.device
        dhid = torch.empty_like(hid)
        dw, db = torch.empty(1, D, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
        scratch = torch.empty(_lib.lib().vbx_duration_head_bwd_scratch_floats(B, n, D), dtype=torch.float32, device=dev)
        _lib.call("vbx_duration_head_bwd", hid, w32, durations, target, m8, den, g.detach().to(torch.float32).reshape(1).contiguous(),
                  dhid, dw, db, scratch, B, n, D, _lib.current_stream())
        return dhid, dw, db, None, None
