"""The aligner on the device: the `Aligner` network (csrc/aligner.hip + vbx_gemm), monotonic alignment search and the forward-sum
loss (csrc/align.hip).

The reference's DurationPredictor training branch (voicebox_pytorch.py:841-876) takes `Aligner`, `maximum_path` and
`ForwardSumLoss` from naturalspeech2_pytorch, which is third-party and not a dependency.  PARITY with that library is UNPINNED; the
semantics are the published ones (the convolutional attention of "One TTS Alignment To Rule Them All" / RAD-TTS; the VITS / glow-tts
monotonic_align rule; nn.CTCLoss(blank=0, zero_infinity=True) over a padded log-softmax), restated in fp64 in tests/aligner_ref.py
and tests/align_ref.py.  DurationPredictor training itself is NOT built.

  aligner = Aligner(dim_in=80, dim_hidden=512, attn_channels=80, temperature=0.0005)
  attn, attn_logprob = aligner(mel [B, dim_in, T], phoneme_emb [B, K, dim_hidden], mask=None)      # both fp32 [B, 1, T, K]
  durations, path = aligner.align(mel, phoneme_emb, key_lens=None, query_lens=None)                 # no_grad
  attn, attn_logprob = aligner_attention(q [B, T, A], k [B, K, A], mask=None, temperature=0.0005)  # the attention op alone
  path, durations = maximum_path(value, query_lens=None, key_lens=None)
  nll = forward_sum_loss(attn_logprob, key_lens, query_lens, blank_logprob=-1., reduction="mean" | "none")
  loss = ForwardSumLoss(blank_logprob=-1.)(attn_logprob, key_lens, query_lens)

`Aligner` and `aligner_attention` are differentiable in every parameter and both inputs, so ForwardSumLoss(aligner(...)[1], ...)
trains the network with nothing but this package.  GPU tensors only; the lengths stay on the device and nothing here synchronises
with the host.  maximum_path and the loss take K (keys) in 1 .. 1024; the attention itself has no key limit."""
import torch
from torch import nn

from . import _lib
from ._packing import PackedWeights

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


# ------------------------------------------------------------------ the Aligner network (csrc/aligner.hip + vbx_gemm)

def _gemm(mode, epi, M, N, K, A, lda, B, ldb, C, ldc, bias=None, f16=0, splits=0):
    d = _lib.GemmDesc()
    d.mode, d.epilogue, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.f16, d.splits = mode, epi, M, N, K, lda, ldb, ldc, f16, splits
    d.A, d.B, d.C, d.bias = A.data_ptr(), B.data_ptr(), C.data_ptr(), None if bias is None else bias.data_ptr()
    rc = _lib.lib().vbx_gemm(d, _lib.current_stream())
    if rc != 0:
        raise _lib.VbxError(f"vbx_gemm failed (rc={rc}): {_lib.lib().vbx_last_error().decode()}")


def _key_mask(who, mask, B, K):
    """[B, 1, K] or [B, K], bool or integer, true = a real key -> the [B, K] view (None stays None)"""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.is_floating_point() or mask.is_complex():
        raise ValueError(f"{who}: mask must be a bool or integer tensor (got {getattr(mask, 'dtype', type(mask))})")
    if mask.ndim == 3 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.shape != (B, K):
        raise ValueError(f"{who}: mask must be [{B}, 1, {K}] or [{B}, {K}] (got {tuple(mask.shape)})")
    return mask


def _mask_u8(who, mask, device):
    if mask is None:
        return None
    if mask.device != device:
        raise ValueError(f"{who}: mask must be on the device of the inputs ({device}), it is on '{mask.device}'")
    return (mask != 0).to(torch.uint8).contiguous()


def _check_batch(who, B, T):
    if B > 65535:
        raise NotImplementedError(f"{who}: at most 65535 batch rows (one grid row each), got {B}")
    if B * T >= 2 ** 31:
        raise NotImplementedError(f"{who}: B * T must stay below 2^31 (got {B} x {T})")


def _attn_fwd(q, k, mask8, tau):
    B, T, A = q.shape
    K = k.shape[1]
    attn = torch.empty(B, 1, T, K, dtype=torch.float32, device=q.device)
    logp = torch.empty(B, 1, T, K, dtype=torch.float32, device=q.device)
    _lib.call("vbx_aligner_attn_fwd", q, k, mask8, tau, attn, logp, B, T, K, A, _lib.current_stream())
    return attn, logp


def _attn_bwd(q, k, mask8, attn, g_logp, g_attn, tau, need_dq, need_dk):
    B, T, A = q.shape
    K = k.shape[1]
    f = lambda g: None if g is None else g.to(torch.float32).contiguous()
    g_logp, g_attn = f(g_logp), f(g_attn)
    gmap = torch.empty(B, T, K, dtype=torch.float32, device=q.device) if g_attn is not None else None
    dq = torch.empty_like(q) if need_dq else None
    dk = torch.empty_like(k) if need_dk else None
    _lib.call("vbx_aligner_attn_bwd", q, k, mask8, attn, g_logp, g_attn, tau, gmap, dq, dk, B, T, K, A, _lib.current_stream())
    return dq, dk


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, mask8, tau):
        attn, logp = _attn_fwd(q, k, mask8, tau)
        ctx.save_for_backward(q, k, mask8, attn)
        ctx.tau = tau
        ctx.set_materialize_grads(False)
        return attn, logp

    @staticmethod
    def backward(ctx, g_attn, g_logp):
        q, k, mask8, attn = ctx.saved_tensors
        if g_attn is None and g_logp is None:
            return None, None, None, None
        dq, dk = _attn_bwd(q, k, mask8, attn, g_logp, g_attn, ctx.tau, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dq, dk, None, None


def aligner_attention(q, k, mask=None, temperature=0.0005):
    """The Aligner's attention on given encodings.  q [B, T, A], k [B, K, A] (computed in fp32), mask [B, 1, K] or [B, K] bool / int,
    true = a real key.  Returns (attn, attn_logprob), both fp32 [B, 1, T, K]:
    attn_logprob[b, 0, t, j] = -temperature * sum_c (q[b, t, c] - k[b, j, c])^2 (NOT masked; the direct difference, an fp32 chain over
    the channels) and attn = softmax_j of it with masked keys filled with -FLT_MAX first: a masked key gets exactly 0, a row whose
    keys are all masked 1 / K.  One launch; differentiable in q and k (include/vbx.h states the error bounds).  A above 128 raises
    NotImplementedError, a CPU tensor VbxError."""
    who = "aligner_attention"
    for name, t in (("q", q), ("k", k)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.ndim != 3:
            raise ValueError(f"{who}: {name} must be a floating-point [B, n, A] tensor (got {getattr(t, 'shape', type(t))})")
    if q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2] or min(q.shape) < 1 or min(k.shape) < 1:
        raise ValueError(f"{who}: q [B, T, A] and k [B, K, A] must share B and A, all sizes >= 1 (got {tuple(q.shape)}, {tuple(k.shape)})")
    B, T, A = q.shape
    mask = _key_mask(who, mask, B, k.shape[1])
    if A > 128:
        raise NotImplementedError(f"{who}: at most 128 attention channels (a 64-key chunk of that width fills the LDS tile), got {A}")
    _check_batch(who, B, T)
    _on_device(who, "q", q)
    _on_device(who, "k", k)
    return _AttnFn.apply(q.to(torch.float32).contiguous(), k.to(torch.float32).contiguous(), _mask_u8(who, mask, q.device),
                         float(temperature))


def _stack_fwd(x, channel_first, B, T, layers):
    """x fp32 [B, T, C] or, channel_first, [B, C, T] -> the fp32 pre-activations [B * T, Cout] of every layer of a stack.  A layer
    in front of a ReLU multiplies three-piece operands (l["w16"] is then three times as wide): see Aligner"""
    M, st, pres, inp = B * T, _lib.current_stream(), [], x
    for i, l in enumerate(layers):
        kc = l["w16"].shape[1]
        a16 = torch.empty(M, kc, dtype=torch.float16, device=x.device)
        _lib.call("vbx_aligner_pack", inp, a16, B, T, l["cin"], l["taps"], int(i > 0), int(channel_first and i == 0),
                  2 if l["split"] else 0, st)
        pre = torch.empty(M, l["cout"], dtype=torch.float32, device=x.device)
        _gemm(_lib.VBX_GEMM_NT, _lib.VBX_EPI_F32, M, l["cout"], kc, a16, kc, l["w16"], kc, pre, l["cout"], bias=l["bias"], f16=1)
        pres.append(pre)
        inp = pre
    return pres


def _stack_bwd(g, x, channel_first, B, T, layers, pres, need_dx):
    """g fp32 [B * T, Cout of the last layer] (overwritten) -> (dx in x's layout or None, [(dW, db)] per layer).  Per layer: the ReLU
    mask and a bf16 cast, the bias column sum, the TN split-K wgrad against the bf16 packed input, the NN dgrad into the packed
    layout and, for three taps, its fold."""
    M, st, dev, n = B * T, _lib.current_stream(), x.device, len(layers)
    grads = [None] * n
    for i in range(n - 1, -1, -1):
        l = layers[i]
        cin, cout, taps = l["cin"], l["cout"], l["taps"]
        kc = cin * taps
        inp, cf = (pres[i - 1], False) if i > 0 else (x, channel_first)
        gb = torch.empty(M, cout, dtype=torch.bfloat16, device=dev)
        _lib.call("vbx_aligner_relu_bwd", g, pres[i] if i < n - 1 else None, gb, M * cout, st)
        db = torch.empty(cout, dtype=torch.float32, device=dev)
        scratch = torch.empty(_lib.lib().vbx_colsum_scratch_floats(M, cout), dtype=torch.float32, device=dev)
        _lib.call("vbx_colsum_f32", g, M, cout, cout, db, scratch, st)
        xb = torch.empty(M, kc, dtype=torch.bfloat16, device=dev)
        _lib.call("vbx_aligner_pack", inp, xb, B, T, cin, taps, int(i > 0), int(cf), 1, st)
        splits = max(1, min(8, M // 256))  # every split keeps rows: 32 s (s - 1) < 256 s <= M
        slabs = torch.empty(splits, cout, kc, dtype=torch.float32, device=dev)
        _gemm(_lib.VBX_GEMM_TN, _lib.VBX_EPI_SPLITK, cout, kc, M, gb, cout, xb, kc, slabs, kc, splits=splits)
        dw = torch.empty(cout, cin, taps, dtype=torch.float32, device=dev)  # column c * taps + tap IS the weight's layout
        _lib.call("vbx_splitk_reduce", slabs, splits, cout, kc, dw, cout, kc, kc, 0, 0, 0, st)
        grads[i] = (dw, db)
        if i == 0 and not need_dx:
            return None, grads
        d = torch.empty(M, kc, dtype=torch.float32, device=dev)
        _gemm(_lib.VBX_GEMM_NN, _lib.VBX_EPI_F32, M, kc, cout, gb, cout, l["wb"], kc, d, kc)
        if taps == 3:
            g = torch.empty(B, cin, T, dtype=torch.float32, device=dev) if cf else torch.empty(M, cin, dtype=torch.float32, device=dev)
            _lib.call("vbx_aligner_fold", d, g, B, T, cin, int(cf), st)
        else:
            g = d
    return g, grads


class _AlignerFn(torch.autograd.Function):
    """The whole module as one node: both stacks (pack + vbx_gemm per layer), the attention launch, and their backward."""

    @staticmethod
    def forward(ctx, xq, xk, mask8, mod, channel_first, *params):
        w = mod._cached(mod._pack)
        B, K = xk.shape[0], xk.shape[1]
        T = xq.shape[2] if channel_first else xq.shape[1]
        qpre = _stack_fwd(xq, channel_first, B, T, w["query"])
        kpre = _stack_fwd(xk, False, B, K, w["key"])
        A = mod.attn_channels
        attn, logp = _attn_fwd(qpre[-1].view(B, T, A), kpre[-1].view(B, K, A), mask8, mod.temperature)
        ctx.save_for_backward(xq, xk, mask8, attn, *qpre, *kpre)
        ctx.w, ctx.dims, ctx.tau, ctx.channel_first = w, (B, T, K, A, len(qpre)), mod.temperature, channel_first
        ctx.set_materialize_grads(False)
        return attn, logp

    @staticmethod
    def backward(ctx, g_attn, g_logp):
        xq, xk, mask8, attn, *pres = ctx.saved_tensors
        B, T, K, A, nq = ctx.dims
        none = (None,) * (5 + 2 * len(pres))
        if g_attn is None and g_logp is None:
            return none
        qpre, kpre, w = pres[:nq], pres[nq:], ctx.w
        need = ctx.needs_input_grad
        wq, wk = any(need[5:5 + 2 * nq]) or need[0], any(need[5 + 2 * nq:]) or need[1]
        dq, dk = _attn_bwd(qpre[-1].view(B, T, A), kpre[-1].view(B, K, A), mask8, attn, g_logp, g_attn, ctx.tau, wq, wk)
        out = []
        dxq = dxk = None
        if wq:
            dxq, gq = _stack_bwd(dq.view(B * T, A), xq, ctx.channel_first, B, T, w["query"], qpre, need[0])
            dxq = None if dxq is None else dxq.view(xq.shape)
        else:
            gq = [(None, None)] * nq
        if wk:
            dxk, gk = _stack_bwd(dk.view(B * K, A), xk, False, B, K, w["key"], kpre, need[1])
            dxk = None if dxk is None else dxk.view(xk.shape)
        else:
            gk = [(None, None)] * len(kpre)
        for dw, db in gq + gk:
            out += [dw, db]
        return (dxq, dxk, None, None, None, *out)


class Aligner(PackedWeights, nn.Module):
    """naturalspeech2_pytorch's Aligner (the alignment encoder of RAD-TTS) on the device, with its backward.

    forward(queries [B, dim_in, T], keys [B, K, dim_hidden], mask=None) -> (attn, attn_logprob), both fp32 [B, 1, T, K].  queries is
    the mel, channel-first; mask is [B, 1, K] or [B, K], bool or int, true = a real key.
      q = query_layers(queries): Conv1d(dim_in, 2 dim_in, 3, padding 1), ReLU, Conv1d(2 dim_in, dim_in, 1), ReLU,
                                 Conv1d(dim_in, attn_channels, 1)
      k = key_layers(keys^T):    Conv1d(dim_hidden, 2 dim_hidden, 3, padding 1), ReLU, Conv1d(2 dim_hidden, attn_channels, 1)
      attn_logprob[b, 0, t, j] = -temperature * sum_c (q[b, c, t] - k[b, c, j])^2            NOT masked
      attn = softmax_j(attn_logprob with masked keys filled with -FLT_MAX): a masked key gets exactly 0, a fully masked row 1 / K
    The zero padding of the 3-tap layers is at the ends of the tensor, not at per-row lengths: nn.Conv1d on the padded batch.

    The parameters are nn.Conv1d weights and biases under the published names (key_layers.0 / .2, query_layers.0 / .2 / .4);
    load_state_dict also takes them under an `aligner.` prefix.  No published weights exist: this is a network to train.

    Device path: per layer a pack kernel (the 16-bit operand row, zeros outside the tensor, the previous ReLU applied on read) and
    one vbx_gemm (fp16 operands, fp32 accumulation and pre-activation); one launch for both maps; the backward runs bf16 dgrad /
    split-K wgrad GEMMs per layer and the fp32 attention backward -- one autograd node, gradients written into fresh tensors, no
    atomics, no host synchronisation, the same bits on every run.  The fp16 weights are packed once per parameter version; after a
    write through `.data` call mark_weights_dirty().

    The last layer of each stack multiplies plain fp16 operands.  A layer in front of a ReLU multiplies the three-piece fp16
    operands of the model's precise mode ([hi | hi 2^-8 | lo 2^8] against [W_hi | W_lo 2^8 | W_hi 2^-8], K three times as long on
    the same tiles), so its pre-activations are fp32-accurate: the gradient is discontinuous where a pre-activation changes sign,
    and plain fp16 operands flip about 4 in 10^4 of the units, each a full-size error in one row of a weight gradient (measured:
    2.9e-2 relative L2 on query_layers.0.weight at 2 x 67 x 65 against the fp64 autograd, from the forward's rounding alone).

    NotImplementedError: a channel count that is not a multiple of 8 (16-byte operand rows), attn_channels above 128 (the attention
    kernels' LDS tile), more than 65535 batch rows.  A CPU tensor raises VbxError after the shape checks."""

    def __init__(self, dim_in=80, dim_hidden=512, attn_channels=80, temperature=0.0005):
        super().__init__()
        for name, v in (("dim_in", dim_in), ("dim_hidden", dim_hidden), ("attn_channels", attn_channels)):
            if v <= 0:
                raise ValueError(f"Aligner: {name} must be positive (got {v})")
            if v % 8:
                raise NotImplementedError(f"Aligner: {name} must be a multiple of 8 (16-byte GEMM operand rows), got {v}")
        if attn_channels > 128:
            raise NotImplementedError(f"Aligner: attn_channels must be at most 128 (the attention kernels' LDS tile), got {attn_channels}")
        self.dim_in, self.dim_hidden, self.attn_channels, self.temperature = dim_in, dim_hidden, attn_channels, float(temperature)
        self.key_layers = nn.Sequential(nn.Conv1d(dim_hidden, 2 * dim_hidden, 3, padding=1), nn.ReLU(),
                                        nn.Conv1d(2 * dim_hidden, attn_channels, 1))
        self.query_layers = nn.Sequential(nn.Conv1d(dim_in, 2 * dim_in, 3, padding=1), nn.ReLU(), nn.Conv1d(2 * dim_in, dim_in, 1),
                                          nn.ReLU(), nn.Conv1d(dim_in, attn_channels, 1))

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {(k[len("aligner."):] if k.startswith("aligner.") else k): v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

    def _convs(self):
        return [m for m in self.query_layers if isinstance(m, nn.Conv1d)], [m for m in self.key_layers if isinstance(m, nn.Conv1d)]

    def _pack(self):
        """per layer the weight's [Cout, Cin * taps] view in fp16 (forward operand; [W_hi | W_lo 2^8 | W_hi 2^-8] in front of a
        ReLU) and bf16 (dgrad operand) and the fp32 bias"""
        def layer(c, split):
            w = c.weight.detach().float().reshape(c.out_channels, -1)
            w16 = w.half()
            if split:
                w16 = torch.cat((w16, ((w - w16.float()) * 256.0).half(), (w16.float() / 256.0).half()), 1)
            return dict(cin=c.in_channels, cout=c.out_channels, taps=c.kernel_size[0], split=split, w16=w16.contiguous(),
                        wb=w.bfloat16().contiguous(), bias=c.bias.detach().float().contiguous())
        q, k = self._convs()
        return dict(query=[layer(c, c is not q[-1]) for c in q], key=[layer(c, c is not k[-1]) for c in k])

    def forward(self, queries, keys, mask=None):
        who = "Aligner"
        for name, t in (("queries", queries), ("keys", keys)):
            if not isinstance(t, torch.Tensor) or not t.is_floating_point() or t.ndim != 3:
                raise ValueError(f"{who}: {name} must be a floating-point 3-d tensor (got {getattr(t, 'shape', type(t))})")
        if queries.shape[1] != self.dim_in or keys.shape[2] != self.dim_hidden or queries.shape[0] != keys.shape[0]:
            raise ValueError(f"{who}: takes queries [B, dim_in = {self.dim_in}, T] and keys [B, K, dim_hidden = {self.dim_hidden}] "
                             f"(got {tuple(queries.shape)}, {tuple(keys.shape)})")
        B, _, T = queries.shape
        K = keys.shape[1]
        if T < 1 or K < 1 or B < 1:
            raise ValueError(f"{who}: needs B, T, K >= 1 (got {B}, {T}, {K})")
        mask = _key_mask(who, mask, B, K)
        _check_batch(who, B, max(T, K))
        _on_device(who, "queries", queries)
        _on_device(who, "keys", keys)
        params = [p for convs in self._convs() for c in convs for p in (c.weight, c.bias)]
        if params[0].device != queries.device:
            raise _lib.VbxError(f"{who}: the parameters are on '{params[0].device}', the inputs on '{queries.device}'")
        xq = queries.to(torch.float32)
        rows = xq.transpose(1, 2)
        channel_first = not rows.is_contiguous()  # a mel given as a transposed [B, T, dim_in] tensor is read in place
        xq = xq.contiguous() if channel_first else rows
        return _AlignerFn.apply(xq, keys.to(torch.float32).contiguous(), _mask_u8(who, mask, queries.device), self, channel_first, *params)

    def align(self, mel, phoneme_emb, key_lens=None, query_lens=None):
        """forward, then maximum_path on attn with the lengths on the device: (durations int64 [B, K], path fp32 [B, 1, T, K]).
        key_lens / query_lens int [B] on the device (None: K / T); keys at and beyond key_len are masked.  Runs under no_grad."""
        who = "Aligner.align"
        if isinstance(phoneme_emb, torch.Tensor) and phoneme_emb.ndim == 3:
            _check_lens(who, "key_lens", key_lens, phoneme_emb.shape[0])
            _check_lens(who, "query_lens", query_lens, phoneme_emb.shape[0])
        with torch.no_grad():
            mask = None
            if key_lens is not None:
                mask = torch.arange(phoneme_emb.shape[1], device=key_lens.device)[None, :] < key_lens[:, None]
            attn, _ = self.forward(mel, phoneme_emb, mask)
            path, durations = maximum_path(attn, query_lens, key_lens)
        return durations, path
