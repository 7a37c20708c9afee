"""Aligner primitives on the device (csrc/align.hip): monotonic alignment search and the forward-sum loss.

The reference's DurationPredictor training branch (voicebox_pytorch.py:841-876) takes `maximum_path` and `ForwardSumLoss` from
naturalspeech2_pytorch, which is third-party and not a dependency.  PARITY with that library is UNPINNED; the semantics are the
published ones (the VITS / glow-tts monotonic_align rule, nn.CTCLoss(blank=0, zero_infinity=True) over a padded log-softmax),
restated in fp64 in tests/align_ref.py.  The `Aligner` network and DurationPredictor training are NOT built.

  path, durations = maximum_path(value, query_lens=None, key_lens=None)
  nll = forward_sum_loss(attn_logprob, key_lens, query_lens, blank_logprob=-1., reduction="mean" | "none")
  loss = ForwardSumLoss(blank_logprob=-1.)(attn_logprob, key_lens, query_lens)

GPU tensors only; the lengths stay on the device and nothing here synchronises with the host.  K (keys) is 1 .. 1024."""
import torch
from torch import nn

from . import _lib

MAX_KEYS = 1024


def _map(who, name, t):
    """[B, T, K] or [B, 1, T, K] floating point -> the [B, T, K] view; shape and dtype errors raise ValueError, K beyond the
    kernels' limit NotImplementedError; a CPU tensor raises VbxError after those (_on_device), all before any launch"""
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise ValueError(f"{who}: {name} must be a floating-point tensor (got {getattr(t, 'dtype', type(t))})")
    if t.ndim == 4 and t.shape[1] == 1:
        t = t[:, 0]
    elif t.ndim != 3:
        raise ValueError(f"{who}: {name} must be [B, T, K] or [B, 1, T, K] (got {tuple(t.shape)})")
    B, T, K = t.shape
    if B < 1 or T < 1 or K < 1:
        raise ValueError(f"{who}: {name} needs B, T, K >= 1 (got {tuple(t.shape)})")
    if K > MAX_KEYS:
        raise NotImplementedError(f"{who}: at most {MAX_KEYS} keys (one thread per key), got K = {K}")
    if B * T >= 2 ** 31:
        raise NotImplementedError(f"{who}: B * T must stay below 2^31 (got {B} x {T})")
    return t


def _on_device(who, name, t):
    if t.device.type != "cuda":
        raise _lib.VbxError(f"{who} runs only on an MI355X (gfx950) through libvbx_hip.so; {name} is on '{t.device}' and there is "
                            "no CPU fallback")


def _check_lens(who, name, lens, B):
    if lens is None:
        return
    if not isinstance(lens, torch.Tensor) or lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
        raise ValueError(f"{who}: {name} must be an integer tensor (got {getattr(lens, 'dtype', type(lens))})")
    if lens.shape != (B,):
        raise ValueError(f"{who}: {name} must have shape [{B}] (got {tuple(lens.shape)})")


def _lens(who, name, lens, device):
    if lens is None:
        return None
    if lens.device != device:
        raise ValueError(f"{who}: {name} must be on the device of the map ({device}), it is on '{lens.device}': lengths are never "
                         "read on the host")
    return lens.to(torch.int32).contiguous()


def maximum_path(value, query_lens=None, key_lens=None):
    """Monotonic alignment search.  value [B, T, K] or [B, 1, T, K]: the score of putting query frame t on key k (any float dtype,
    computed in fp32); query_lens / key_lens int [B] on the device (None: T / K).  Returns (path, durations): path in value's dtype
    and shape, 0 / 1, one 1 in every row t < query_len, columns non-decreasing from key 0 to key_len - 1, zeros outside the
    lengths; durations int64 [B, K] = path summed over t.  A tie stays on the same key.  A row with query_len < key_len or a zero
    length has no monotonic path: all zeros, no exception.  Not differentiable."""
    who = "maximum_path"
    v = _map(who, "value", value)
    B, T, K = v.shape
    _check_lens(who, "query_lens", query_lens, B)
    _check_lens(who, "key_lens", key_lens, B)
    _on_device(who, "value", v)
    ql, kl = _lens(who, "query_lens", query_lens, v.device), _lens(who, "key_lens", key_lens, v.device)
    with torch.no_grad():
        x = v.detach().to(torch.float32).contiguous()
        path = torch.empty_like(x)
        durations = torch.empty(B, K, dtype=torch.int64, device=x.device)
        bits = torch.empty(B, T, (K + 63) // 64, dtype=torch.int64, device=x.device)  # the backtrack's decision bits
        _lib.call("vbx_maximum_path", x, ql, kl, path, durations, bits, B, T, K, _lib.current_stream())
        path = path.to(value.dtype).reshape(value.shape)
    return path, durations


class _ForwardSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, key_lens, query_lens, blank):
        B, T, K = x.shape
        lse = torch.empty(B, T, dtype=torch.float64, device=x.device)
        alpha = torch.empty(B, T, K, dtype=torch.float64, device=x.device) if ctx.needs_input_grad[0] else None
        nll = torch.empty(B, dtype=torch.float32, device=x.device)
        logz = torch.empty(B, dtype=torch.float64, device=x.device)
        _lib.call("vbx_forward_sum_fwd", x, key_lens, query_lens, blank, lse, alpha, nll, logz, B, T, K, _lib.current_stream())
        ctx.save_for_backward(x, key_lens, query_lens, lse, alpha, logz)
        ctx.blank = blank
        return nll

    @staticmethod
    def backward(ctx, g):
        x, key_lens, query_lens, lse, alpha, logz = ctx.saved_tensors
        B, T, K = x.shape
        grad = torch.empty_like(x)
        _lib.call("vbx_forward_sum_bwd", x, key_lens, query_lens, ctx.blank, lse, alpha, logz, g.to(torch.float32).contiguous(), grad,
                  B, T, K, _lib.current_stream())
        return grad, None, None, None


def forward_sum_loss(attn_logprob, key_lens=None, query_lens=None, blank_logprob=-1., reduction="mean"):
    """The forward-sum (CTC) alignment loss.  attn_logprob [B, 1, T, K] or [B, T, K]; per row a blank column of constant
    blank_logprob goes in front of keys 0 .. key_len - 1, each frame t < query_len is log-softmaxed over those key_len + 1 entries,
    and nll = -log of the total probability of all monotonic alignments (CTC, blank 0, target 1 .. key_len).
    reduction "none": nll fp32 [B], NOT divided by key_len; "mean": mean_b(nll_b / key_len_b), which is
    nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True).  A row with query_len < key_len or a zero length contributes loss 0
    and gradient 0.  The gradient is fp32-computed, exactly 0 at t >= query_len and keys >= key_len."""
    who = "forward_sum_loss"
    if reduction not in ("mean", "none"):
        raise ValueError(f"{who}: reduction must be 'mean' or 'none' (got {reduction!r})")
    blank = float(blank_logprob)
    if blank != blank or blank in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: blank_logprob must be finite (got {blank_logprob})")
    x = _map(who, "attn_logprob", attn_logprob)
    B, T, K = x.shape
    _check_lens(who, "key_lens", key_lens, B)
    _check_lens(who, "query_lens", query_lens, B)
    _on_device(who, "attn_logprob", x)
    kl, ql = _lens(who, "key_lens", key_lens, x.device), _lens(who, "query_lens", query_lens, x.device)
    nll = _ForwardSum.apply(x.to(torch.float32).contiguous(), kl, ql, blank)
    if reduction == "none":
        return nll
    return (nll / (kl.clamp(min=1).to(torch.float32) if kl is not None else float(K))).mean()


class ForwardSumLoss(nn.Module):
    """forward_sum_loss(..., reduction="mean") as a module, with the call signature of naturalspeech2_pytorch's ForwardSumLoss:
    (attn_logprob, key_lens, query_lens)."""

    def __init__(self, blank_logprob=-1.):
        super().__init__()
        self.blank_logprob = blank_logprob

    def forward(self, attn_logprob, key_lens=None, query_lens=None):
        return forward_sum_loss(attn_logprob, key_lens, query_lens, blank_logprob=self.blank_logprob, reduction="mean")
