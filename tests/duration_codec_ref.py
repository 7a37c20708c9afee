"""fp64 restatement of DurationPredictor over codec latents (DurationPredictor.attach_codec, csrc/duration.hip:
vbx_pack_phoneme_latent), the inputs the CPU and GPU tests share, and a list of planted faults.

The reference (voicebox_pytorch.py:776, :793-819) applies proj_in = Linear(latent_dim, dim) as the first line of forward, so the
model is restate.duration_predictor_forward(..., cond = latents @ W^T + b): the mask FOLLOWS proj_in (a masked row is 0, not the
bias), then the guidance drop (null_cond replaces the projected rows, it does not pass through proj_in), then curtail_or_pad (rows
past S are 0 even for a dropped sample).  Under restate.emulate_fp16_operands() the projection's own operands are rounded to fp16
as the kernel rounds them.  Loss, leaves, comparison and tolerances are tests/duration_train_ref.py's.

cond_rows() below composes cond'' [B, n, D] step by step so that each planted fault can be switched in; with no fault it equals the
one-line form above (tests/test_duration_codec_cpu.py asserts that to 1e-12)."""
import functools

import torch

import duration_train_ref as R
from oracle import restate

FORWARD_FAULTS = ("mask_before_proj",               # masked rows equal the bias
                  "null_through_proj",              # null_cond (cut / zero-extended to the latent width) sent through proj_in
                  "pad_rows_get_bias",              # proj_in after curtail_or_pad: rows r >= S receive the bias
                  "pad_rows_of_dropped_get_null",   # the drop after curtail_or_pad: rows r >= S of a dropped sample receive null_cond
                  "no_bias")
GRAD_FAULTS = ("masked_rows_counted",               # the same values, masked rows counted in d weight / d bias
               "dropped_counted",                   # ... dropped samples counted
               "pad_rows_counted_in_bias")          # ... rows r >= S counted in d bias
FAULTS = FORWARD_FAULTS + GRAD_FAULTS


def fixture_cases(g):
    """tests/golden/duration_codec.pt -> {name: case} with the full state dict of each model (common weights + its proj_in)"""
    return {name: dict(c, state={**c["state"], **g["common_state"]}) for name, c in g["cases"].items()}


def _pad_rows(t, n):
    return restate.curtail_or_pad(t, n)


def cond_rows(p, latents, cond_mask, drop, n, fault=None):
    """cond'' [B, n, D]: proj_in at length S -> mask -> drop -> curtail_or_pad to n, differentiable in proj_in.*"""
    W, b = p["proj_in.weight"], p["proj_in.bias"]
    lat = latents.to(W.dtype)
    B, S, L = lat.shape
    D = W.shape[0]
    null = p["null_cond"].to(W.dtype)
    m = cond_mask[..., None]
    dr = None if drop is None else drop[:, None, None]
    if fault == "pad_rows_get_bias":
        lat = _pad_rows(lat, n)
        m = _pad_rows(m.to(W.dtype), n) > 0.5
    if fault == "mask_before_proj":
        lat = lat * ~m
    y = restate._op(lat) @ restate._op(W).t()
    if fault != "no_bias":
        y = y + b
    c = y if fault == "mask_before_proj" else y * ~m
    if fault == "masked_rows_counted":
        c = c + (y - y.detach()) * m
    if dr is not None:
        if fault == "null_through_proj":
            k = min(L, D)
            nl = torch.zeros(L, dtype=W.dtype)
            nl[:k] = null[:k]
            c = torch.where(dr, nl @ W.t() + b, c)
        elif fault == "dropped_counted":
            c = torch.where(dr, null + (y - y.detach()), c)
        else:
            c = torch.where(dr, null, c)
    c = _pad_rows(c, n)
    if S < n and fault == "pad_rows_of_dropped_get_null" and dr is not None:
        c = torch.cat((c[:, :S], torch.where(dr, null, c[:, S:])), dim=1)
    if S < n and fault == "pad_rows_counted_in_bias":
        c = torch.cat((c[:, :S], c[:, S:] + (b - b.detach())), dim=1)
    return c


def predict(p, cfg, case, fault=None):
    """the durations [B, n]; case["cond"] holds the latents [B, S, L]"""
    ids = case["ids"]
    c = cond_rows(p, case["cond"], case["cond_mask"], case.get("drop"), ids.shape[-1], fault)
    none = torch.zeros(c.shape[:2], dtype=torch.bool)
    return restate.duration_predictor_forward(p, cfg, c, ids, none, self_attn_mask=case.get("self_attn_mask"))


def predict_one_line(p, cfg, case):
    """the model as the module docstring states it"""
    proj = restate._op(case["cond"].to(p["proj_in.weight"].dtype)) @ restate._op(p["proj_in.weight"]).t() + p["proj_in.bias"]
    return restate.duration_predictor_forward(p, cfg, proj, case["ids"], case["cond_mask"], cond_drop_mask=case.get("drop"),
                                              self_attn_mask=case.get("self_attn_mask"))


def reference(case, fault=None, emulate=True):
    """duration_train_ref.reference (loss, gradients of every leaf, proj_in.* among them) with the prediction above"""
    orig = R.predict
    R.predict = lambda p, cfg, c, f=None: predict(p, cfg, c, fault)
    try:
        return R.reference(case, emulate=emulate)
    finally:
        R.predict = orig


def front_end(p, case, fault=None, cond16=None):
    """the first autograd node alone, operand roundings as active: (x, e = to_embed's output, emb, packed, cond'').  cond16 [B, n, D]:
    the fp16 values the device's pack wrote for cond'' (held to their own bound elsewhere) -- to_embed then reads exactly the
    operand the device reads, where the fp32 sum and the fp64 one may round to neighbouring fp16 values; gradients pass straight
    through to cond''."""
    ids = case["ids"]
    sam = ids != -1
    c = cond_rows(p, case["cond"], case["cond_mask"], case.get("drop"), ids.shape[-1], fault)
    emb = p["to_phoneme_emb.weight"][ids.clamp(min=0)]
    packed = torch.cat((emb, c if cond16 is None else c + (cond16.to(c.dtype) - c).detach()), dim=-1)
    e = restate._op(packed) @ restate._op(p["to_embed.weight"]).t() + p["to_embed.bias"]
    x = restate.conv_pos_embed(e, p["conv_embed.dw_conv1d.0.weight"], p["conv_embed.dw_conv1d.0.bias"], sam) + e
    return x, e, emb, packed, c


# ----------------------------------------------------------------------------- models and inputs
def with_proj(state, L, seed, dim=64):
    """the state plus proj_in.*: the weight at the scale of nn.Linear's initialisation, the bias far from 0 (so that "0" and "the
    bias" are different rows)"""
    g = torch.Generator().manual_seed(seed)
    sd = dict(state)
    sd["proj_in.weight"] = torch.randn(dim, L, generator=g) * L ** -0.5
    sd["proj_in.bias"] = torch.randn(dim, generator=g) * 0.5
    return sd


def well_conditioned(state):
    """q_norm / k_norm gamma x 0.25, the small fixtures' recipe: attention logits at a scale where rounding is not amplified"""
    return {k: (v * 0.25 if k.endswith(("q_norm.gamma", "k_norm.gamma")) else v) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def given_case(L=100, E=32, B=3, n=17, drop=False, S=None):
    """duration_train_ref.given_case seen through proj_in: the same model (+ proj_in), ids and cond_mask, and latents [B, S, L] chosen
    so that proj_in maps them onto THAT case's condition, latents = (cond - b) pinv(W)^T (exact in fp64 for L >= dim, least squares
    below it), so the condition has that case's statistics.
    The weights are WELL-CONDITIONED by the recipe of the small fixtures (tests/golden/make_golden_codec.py::condition): q_norm /
    k_norm gamma x 0.25.  With the default gammas the qk-norm scale of 10 makes this restatement's OWN gradients move by 0.17 .. 0.39
    (relative L2) when the latents move by one part in 1000, and its durations by up to 0.39 frames: a comparison at GRAD_TOL =
    0.15 then measures the case, not the arithmetic.  (On an MI355X the default-gamma cases put every gradient, the stack's own
    included, 0.17 .. 0.33 from the restatement at 3 x 17 and 2 x 65, while every one of them was bit-equal to the codec-free
    predictor's fed the same projected rows.)  With the recipe the same perturbation moves no gradient by more than 0.011;
    tests/test_duration_codec_cpu.py holds that at GRAD_TOL / 10.  S (default n) is the length of the
    latents (training needs S == n); with S != n the condition is a fresh normal draw.  The same object for every test that asks
    (do not modify it)."""
    S = n if S is None else S
    state = well_conditioned(with_proj(R.init_state(E, seed=3), L, seed=5))
    cond, ids, cond_mask = R.make_inputs(B, n, seed=4)
    if S != n:
        cond = torch.randn(B, S, cond.shape[-1], generator=torch.Generator().manual_seed(7))
        cond_mask = (_pad_rows(cond_mask[..., None].double(), S) > 0.5)[..., 0]
        if S > n:
            cond_mask[:, n:] = torch.rand(B, S - n, generator=torch.Generator().manual_seed(6)) < 0.6
    W, b = state["proj_in.weight"].double(), state["proj_in.bias"].double()
    latents = ((cond.double() - b) @ torch.linalg.pinv(W).t()).float()
    case = dict(state=state, qk_norm=True, cond=latents, ids=ids, cond_mask=cond_mask, drop=torch.ones(B, dtype=torch.bool) if drop else None)
    if S == n:
        with torch.no_grad(), restate.emulate_fp16_operands():
            d = predict({k: v.double() if v.is_floating_point() else v for k, v in state.items()}, R.cfg_of(), case)
        case["target"] = R.planted_targets(d)
        case["d_ref"] = d
    return case


@functools.lru_cache(maxsize=None)
def given_reference(L=100, E=32, B=3, n=17, drop=False):
    return reference(given_case(L, E, B, n, drop))


def aligner_case(L=100, E=24, flag=True):
    """duration_train_ref.aligner_case with latents of width L in place of its condition"""
    case = dict(R.aligner_case(E, flag=flag))
    B, n = case["ids"].shape
    case["state"] = with_proj(case["state"], L, seed=5)
    case["cond"] = torch.randn(B, n, L, generator=torch.Generator().manual_seed(8))
    return case


# ----------------------------------------------------------------------------- the bounds of include/vbx.h
def proj_bound(lat16, w16, b, y):
    """per element: (L + 2) 2^-24 (sum |w x| + |b|) + 2^-11 |y| on the fp16-rounded operands (fp64 tensors)"""
    L = lat16.shape[-1]
    return (L + 2) * R.U24 * (lat16.abs() @ w16.abs().t() + b.abs()) + 2.0 ** -11 * y.abs()


def proj_wgrad_bound(de, w_cond, dc, x):
    """per element of [ d proj_in.weight | d proj_in.bias ] [D, L + 1]: de [M, D] the fp64 gradient of to_embed's output, w_cond =
    W_embed[:, E:] [D, D], dc [M, D] the fp64 d cond'', x [M, L + 1] the bf16-rounded rows of the weight-gradient operand (column L
    = 1, zero rows where no gradient passes):
        sum_r (rb[r, d] + 2^-9 |dc[r, d]|) |x[r, l]| + BF16_PRODUCT sum_r |dc[r, d] x[r, l]|,  rb = BF16_PRODUCT (|de| |w_cond|)
    -- the dgrad's own error and the rounding of its result to bf16, then the product of two bf16 operands"""
    rb = R.BF16_PRODUCT * (de.abs() @ w_cond.abs())
    return (rb + 2.0 ** -9 * dc.abs()).t() @ x.abs() + R.BF16_PRODUCT * (dc.abs().t() @ x.abs())


def lcb_rows(latents, cond_mask, drop, n):
    """the weight-gradient operand before rounding [B n, L + 1]: the latent row and a 1, zero on rows that pass no gradient"""
    B, S, L = latents.shape
    rows = torch.cat((latents.double(), torch.ones(B, S, 1, dtype=torch.float64)), dim=-1)
    keep = ~cond_mask
    if drop is not None:
        keep = keep & ~drop[:, None]
    return _pad_rows(rows * keep[..., None], n).reshape(B * n, L + 1)
