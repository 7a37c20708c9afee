"""CPU restatement of the codec-latent model path (voicebox_pytorch.py:1000-1006) on top of oracle/restate.py: proj_in on x and on
cond in torch, then the restated VoiceBox.forward at width dim (its to_pred is [latent_dim, dim], so the output is latent-wide).
Checked against the live reference's fixture in tests/test_codec_cpu.py; the GPU tests use it where no fixture value exists (the
euler / rk4 / dopri5 samplers) and for the fp64 restatement of the fused proj_in kernel."""
import torch

from oracle import restate


def proj_in(p, t):
    return t @ p["proj_in.weight"].to(t.dtype).t() + p["proj_in.bias"].to(t.dtype)


def codec_forward(p, cfg, x, times, cond, cond_mask, **kw):
    return restate.voicebox_forward(p, cfg, proj_in(p, x), times, proj_in(p, cond), cond_mask, **kw)


def codec_forward_with_cond_scale(p, cfg, x, times, cond, cond_mask, cond_token_ids=None, cond_scale=1.0):
    return restate.forward_with_cond_scale(p, cfg, proj_in(p, x), times, proj_in(p, cond), cond_mask, cond_token_ids=cond_token_ids,
                                           cond_scale=cond_scale)


def embed_operand(x, cond, w, b, cond_mask, drop=None, null_cond=None):
    """fp64 rows [ x' | cond' ] of the to_embed operand (no text columns): x' = x W^T + b,
    cond' = drop[b] ? null_cond : (cond_mask ? 0 : cond W^T + b).  x, cond [B, N, L]; cond_mask [B, N] bool; drop [B] bool."""
    x, cond, w, b = x.double(), cond.double(), w.double(), b.double()
    xp = x @ w.t() + b
    cp = (cond @ w.t() + b) * (~cond_mask)[..., None]
    if drop is not None:
        cp = torch.where(drop[:, None, None], null_cond.double(), cp)
    return xp, cp


def proj_in_grads(x, cond, dxp, dcp, cond_mask, drop=None):
    """fp64 d(proj_in.weight), d(proj_in.bias) from d(x') and d(cond'): masked / dropped rows of cond pass no gradient"""
    keep = ~cond_mask
    if drop is not None:
        keep = keep & ~drop[:, None]
    dcp = dcp.double() * keep[..., None]
    dxp = dxp.double()
    L = x.shape[-1]
    dw = dxp.reshape(-1, dxp.shape[-1]).t() @ x.double().reshape(-1, L) + dcp.reshape(-1, dcp.shape[-1]).t() @ cond.double().reshape(-1, L)
    db = dxp.sum(dim=(0, 1)) + dcp.sum(dim=(0, 1))
    return dw, db


def codec_cfm_loss(p, cfg, x1, x0, times, frac_lengths, rand, cond_token_ids=None, cond_drop_mask=None):
    """ConditionalFlowMatcherWrapper.forward on latents x1 [B, N, latent_dim] with the draws injected (restate.cfm_loss with proj_in
    in front): the condition defaults to the target, the target and the prediction are latent-wide."""
    w, flow = restate.cfm_inputs(x1, x0, times, cfg.sigma)
    cond_mask = restate.frac_lengths_mask(x1.shape[1], frac_lengths, rand)
    return codec_forward(p, cfg, w, times, flow, cond_mask, target=flow, cond_token_ids=cond_token_ids, cond_drop_mask=cond_drop_mask)
