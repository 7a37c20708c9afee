"""Error metrics and input builders of the attention tests (tests/test_ops_gpu.py, tests/test_attn_edges_gpu.py,
tests/test_attn_lens_edges_gpu.py; tests/test_attn_check_cpu.py proves on CPU that the checks bite).

`rel_err` is one Frobenius norm over a whole tensor: an error confined to one (b, h) tile of 128 rows -- a ragged tail, one padded work
id, one ring slot -- hides under it (a 30 % error in one 16-row dq tail tile of (B, H, Np) = (2, 2, 1040) raises the global dq error by
0.3 * sqrt(16 / 4160) ~ 0.019).  `tile_errors` measures every (b, h, 128-row tile) on its own, at the kernels' own tiling: query tiles
for out, lse and dq, key tiles for dk and dv.

The length-aware entry points (vbx_attn_fwd_lens, vbx_attn_bwd_lens, vbx_attn_bwd_fused_lens, vbx_attn_fwd_segs) have their own
inputs (`edge_inputs`: the last live key of every batch row carries a share of every softmax, every dead key is a trap), their own
fp64 reference (`lens_reference`, `segs_reference`), their own checks (`check_lens_fwd`, `check_lens_bwd`, `check_lens_fused`,
`check_segs`) and the bound groups lens, lens_qknorm, lens_fused and segs of BOUNDS.  The checks take plain CPU tensors in the
[B, H, Np, 64] layout, so the same functions judge the kernels and the torch stand-in of tests/test_attn_check_cpu.py.
"""
import json
import math
import os

import torch


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def max_err(got, ref):
    return float((got.double().cpu() - ref.double().cpu()).abs().max())


def qpre(L, q16, scale):
    """The kernels' q operand and the q the exact reference must see (include/vbx.h, attention contract since round 5): q16 carries
    scale * log2(e), i.e. the kernel computes with fp16(q * c) -- the reference with that value divided by c in fp64."""
    c = L.lib().vbx_attn_q_prescale(scale)
    qs = (q16.float() * c).half()
    return qs, qs.double() / c


def attn_inputs(Bsz, H, Np, seed, qnorm=8.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Bsz, H, Np, 64, generator=g)
    k = torch.randn(Bsz, H, Np, 64, generator=g)
    if qnorm:
        q = q / q.norm(dim=-1, keepdim=True) * qnorm
        k = k / k.norm(dim=-1, keepdim=True) * qnorm
    v = torch.randn(Bsz, H, Np, 64, generator=g)
    return q.half(), k.half(), v.half()


def rot_tables(Np, R):
    from oracle import restate

    pos = torch.cat((torch.full((R,), -10000, dtype=torch.long), torch.arange(Np - R)))
    fr = restate.rotary_freqs(pos, 64, 50000.0)
    return fr, fr[:, :32].cos().contiguous(), fr[:, :32].sin().contiguous()


# Bounds of tests/test_attn_edges_gpu.py: ~1.5 x the largest value measured on MI355X over all cases of a group (the measured value is
# in the comment).  Global bounds are rel_err over the whole tensor, *_tile the worst (b, h, 128-row tile), lse an absolute max error in
# log2 units, zero_abs the max |error| of a gradient whose fp64 reference is exactly 0 (one valid key per row, Np = 1).
# In the reference's qk-norm regime (|q| = |k| = 8, scale 10) the softmax is one-hot: dS = P (dP - delta) cancels to the fp16 rounding
# of O inside delta (test_ops_gpu.py::test_attn_dropout_fwd_bwd), so a tile whose queries are all one-hot has a reference far below
# its rounding noise.  There the dq / dk tiles are measured against a floor of half the typical tile norm (`floor`); an error that
# moves a tile of ordinary size still shows at its relative size.  The loose drop_qknorm gradient bounds come from one case
# (Np = 17, p = 0.5: one batch row of 17 one-hot queries, 0.156 against <= 0.025 everywhere else).
_ONE_HOT_FLOOR = {"dq": 0.5, "dk": 0.5, "dpre_q": 0.5, "dpre_k": 0.5}
BOUNDS = dict(
    spread=dict(
        out16=0.00068,  # 0.000448
        out16_tile=0.00071,  # 0.000468
        out_bf16=0.0028,  # 0.00182
        out_bf16_tile=0.0034,  # 0.00221
        lse=1.6e-05,  # 1.05e-05
        lse_tile=1.6e-06,  # 1.03e-06
        dq=0.014,  # 0.00913
        dq_tile=0.056,  # 0.0367
        dk=0.0079,  # 0.00525
        dk_tile=0.034,  # 0.0224
        dv=0.0038,  # 0.00248
        dv_tile=0.0049,  # 0.00321
        zero_abs=0.0024,  # 0.00156
    ),
    qknorm=dict(
        out16=0.00019,  # 0.000122
        out16_tile=0.00035,  # 0.000229
        out_bf16=0.0028,  # 0.00182
        out_bf16_tile=0.0032,  # 0.00208
        lse=0.00011,  # 6.72e-05
        lse_tile=1.1e-07,  # 7.29e-08
        dq=0.027,  # 0.0174
        dq_tile=0.053,  # 0.035
        dk=0.025,  # 0.0163
        dk_tile=0.062,  # 0.0413
        dv=0.0027,  # 0.00175
        dv_tile=0.0036,  # 0.00235
        zero_abs=0.024,  # 0.0159
    ),
    fused=dict(
        dv=0.0025,  # 0.00165
        dv_tile=0.0032,  # 0.00212
        dpre_q=0.032,  # 0.0211
        dpre_q_tile=0.11,  # 0.0726
        dpre_k=0.031,  # 0.0201
        dpre_k_tile=0.11,  # 0.0693
        dgamma=0.034,  # 0.0226
        zero_abs=0.0011,  # 0.000713
        dgamma_zero_abs=0.0014,  # 0.000884
    ),
    drop_spread=dict(
        out16=0.00064,  # 0.000425
        out16_tile=0.00071,  # 0.000472
        out_bf16=0.0026,  # 0.00171
        out_bf16_tile=0.0036,  # 0.00236
        lse=1.9e-06,  # 1.22e-06
        lse_tile=2.3e-07,  # 1.52e-07
        dq=0.0053,  # 0.00351
        dq_tile=0.0077,  # 0.00508
        dk=0.0051,  # 0.0034
        dk_tile=0.0058,  # 0.00386
        dv=0.0036,  # 0.00237
        dv_tile=0.0039,  # 0.00256
        dpre_q=0.006,  # 0.00395
        dpre_q_tile=0.007,  # 0.00461
        dpre_k=0.0057,  # 0.0038
        dpre_k_tile=0.0062,  # 0.00412
        zero_abs=2.6e-05,  # 1.71e-05
    ),
    drop_qknorm=dict(
        out16=0.00032,  # 0.000213
        out16_tile=0.00042,  # 0.000274
        out_bf16=0.0027,  # 0.0018
        out_bf16_tile=0.003,  # 0.00196
        lse=0.00012,  # 7.54e-05
        lse_tile=2.4e-07,  # 1.59e-07
        dq=0.24,  # 0.156
        dq_tile=0.59,  # 0.39
        dk=0.22,  # 0.144
        dk_tile=0.53,  # 0.348
        dv=0.0027,  # 0.00179
        dv_tile=0.0029,  # 0.00192
        dpre_q=0.22,  # 0.144
        dpre_q_tile=0.52,  # 0.343
        dpre_k=0.23,  # 0.147
        dpre_k_tile=0.52,  # 0.341
        dgamma=0.25,  # 0.166
        zero_abs=0.0022,  # 0.00143
        dgamma_zero_abs=0.002,  # 0.0013
    ),
    f32=dict(
        out16=0.00032,  # 0.000207
        out16_tile=0.00037,  # 0.000246
        out_bf16=0.0025,  # 0.00166
        out_bf16_tile=0.0026,  # 0.0017
        out32=3.2e-06,  # 2.08e-06
        out32_tile=5.2e-06,  # 3.42e-06
        lse=0.00017,  # 0.000108
        lse_tile=1.3e-07,  # 8.55e-08
    ),
    module=dict(
        out16=0.00054,  # 0.000354
        out16_tile=0.0006,  # 0.000396
        dq=0.0045,  # 0.00293
        dq_tile=0.0045,  # 0.003
        dk=0.0044,  # 0.00292
        dk_tile=0.0046,  # 0.00305
        dv=0.0034,  # 0.00223
        dv_tile=0.0037,  # 0.0024
    ),
)
BOUNDS["qknorm"]["floor"] = BOUNDS["fused"]["floor"] = BOUNDS["drop_qknorm"]["floor"] = _ONE_HOT_FLOOR
# The length-aware entry points (tests/test_attn_lens_edges_gpu.py) inherit the bounds of the masked kernels, whose bits they must
# reproduce on live rows: lens = spread, lens_qknorm = qknorm, lens_fused = fused, segs = the forward part of spread.  They are NOT set
# from the length-aware kernels' own output.  A bound may only be widened where the torch stand-in of tests/test_attn_check_cpu.py
# shows, on the same input, an error within a factor 2 of the GPU's; it then becomes 1.5 x the larger of the two and both figures go in
# its comment.  profiles/attn_lens_edges_measured.json holds the values of one full run on MI355X.
BOUNDS["lens"] = dict(BOUNDS["spread"])
BOUNDS["lens_qknorm"] = dict(BOUNDS["qknorm"])
BOUNDS["lens_fused"] = dict(BOUNDS["fused"])
# Widened under that rule (worst case on MI355X / the stand-in on the same input); every other value is the inherited one:
BOUNDS["lens_qknorm"]["lse_tile"] = 3.7e-07  # 2.526e-07 / 2.526e-07 (Np 1040, key_lens 1: a tile with ONE live row, whose lse is the fp32
#                                              dot product itself; the inherited 1.1e-07 is an rms over 128 rows, below one fp32 ulp)
BOUNDS["lens_fused"]["dv"] = 0.0038  # 0.002543 / 0.002548 (Np 1029, spread softmax: the bf16 rounding of P; `fused` was measured on the
BOUNDS["lens_fused"]["dv_tile"] = 0.0049  # 0.0033 / 0.0033  one-hot softmax only, where P rounds to 1 -- spread's own dv bounds are these)
BOUNDS["lens_fused"]["zero_abs"] = 0.0031  # 0.002121 / 0.002121 (dpre_k at Np 1040, key_lens 1, scale 10: rows of |pre| down to 4, twice
#                                            the 1 / |pre| of the randn rows `fused` was measured on)
BOUNDS["segs"] = {k: BOUNDS["spread"][k] for k in ("out16", "out16_tile", "out_bf16", "out_bf16_tile", "lse", "lse_tile")}
BOUNDARY_ROW = 0.5  # dk / dv at key key_lens[b] - 1, derived: a dropped key is a zero row (error 1), a leaked trap far more, a computed
#                     row bf16 noise (measured: <= 0.027 spread, <= 0.12 one-hot with the row floor of _check_dead_and_boundary)

TILE = 128  # query / key rows per workgroup tile of every attention kernel


def tile_errors(got, ref, tile=TILE, axis=-2, floor=1e-3):
    """Relative error of every tile of `tile` rows along `axis`, separately for every index of the dimensions before `axis`.

    Returns a float64 tensor of shape (*shape[:axis], ceil(n / tile)).  A tile's error is ||got - ref|| / max(||ref||, floor) over the
    tile's rows and all dimensions after `axis`, floor = `floor` * rms(ref) * sqrt(elements of the tile), so that nearly-zero tiles do
    not blow up (`floor` 1e-3 by default; larger where the reference is ill-conditioned per tile, see BOUNDS).  A tile whose reference is exactly zero must be exactly zero: its error is 0 if it is, inf otherwise.  NaN propagates.
    For [B, H, Np, 64] tensors the default axis gives the (b, h, tile) errors; for lse [B, H, Np] pass axis=-1.
    """
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    axis = axis % ref.dim()
    lead, n = ref.shape[:axis], ref.shape[axis]
    trail = math.prod(ref.shape[axis + 1:])
    nt = -(-n // tile)
    pad = nt * tile - n

    def tiles(x):
        x = x.reshape(math.prod(lead), n, trail)
        x = torch.nn.functional.pad(x, (0, 0, 0, pad))
        return x.reshape(-1, nt, tile * trail)

    r, d = tiles(ref), tiles(got - ref)
    rows = torch.full((nt,), float(tile))
    rows[-1] = n - (nt - 1) * tile
    rms = float(ref.norm()) / math.sqrt(max(ref.numel(), 1))
    floor = floor * rms * torch.sqrt(rows * trail)
    rn, dn = r.norm(dim=-1), d.norm(dim=-1)
    err = dn / torch.maximum(rn, floor.expand_as(rn)).clamp(min=1e-300)
    zero = rn == 0
    gz = tiles(got).abs().amax(dim=-1)
    err = torch.where(zero, torch.where(gz == 0, torch.zeros_like(err), torch.full_like(err, math.inf)), err)
    err = torch.where(torch.isnan(dn) | torch.isnan(gz), torch.full_like(err, math.nan), err)
    return err.reshape(*lead, nt)


def worst_tile(err):
    """(largest tile error, its index) -- NaN counts as the largest."""
    flat = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err).flatten()
    i = int(flat.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
    return float(err.flatten()[i]), idx


class Checks:
    """Collects every bound of one test case and fails once, listing all violations (so one run reports every measured value).
    `got <= bound` is False for NaN, so a NaN error fails."""

    def __init__(self, case):
        self.case, self.bad, self.seen = case, [], []

    def le(self, name, value, bound):
        self.seen.append((name, value, bound))
        if not (value <= bound):
            self.bad.append(f"{name} = {value:.4g} > {bound:.4g}")

    def tiles(self, name, got, ref, bound, axis=-2, floor=1e-3):
        e, idx = worst_tile(tile_errors(got, ref, axis=axis, floor=floor))
        self.le(f"{name} tile{idx}", e, bound)

    def true(self, name, cond):
        self.seen.append((name, bool(cond), True))
        if not cond:
            self.bad.append(f"{name} failed")

    def done(self):
        if os.environ.get("ATTN_CHECK_LOG"):  # measured values, one JSON line per case (how the bounds of these tests were set)
            with open(os.environ["ATTN_CHECK_LOG"], "a") as f:
                f.write(json.dumps({"case": self.case, "values": [(n, v if isinstance(v, bool) else float(v), b) for n, v, b in self.seen]}) + "\n")
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)


# ----------------------------------------------------------------------------- small helpers shared by the GPU attention tests
def bf(x):
    return x.to(torch.bfloat16)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def same_bits(a, b):
    it = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}[a.dtype]
    return torch.equal(a.view(it), b.view(it))


def heads(t, B, Np, H):  # token-major [B * Np, H * 64] -> [B, H, Np, 64]
    return t.reshape(B, Np, H, 64).permute(0, 2, 1, 3)


def L_tiles(Np):
    return -(-Np // TILE)


# ----------------------------------------------------------------------------- length-aware attention: inputs
DEAD_LSE = 1e30  # what the forward kernels write as lse of a dead query row (include/vbx.h)
SHARE_MIN = 0.02  # regime "edge": the last live key holds at least this much of every live query's softmax weight (fp64, at build)


def q_prescale(scale):
    """vbx_attn_q_prescale on the host: scale * log2(e) in fp32."""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))


def q_operand(q16, c):
    """qpre for a given prescale c: the kernels' q operand fp16(q * c) and the q the exact reference must see."""
    qs = (q16.float() * c).half()
    return qs, qs.double() / c


def prefix_mask(key_lens, Np):
    return torch.arange(Np)[None, :] < torch.as_tensor(key_lens)[:, None]


def _unrotate(fr, t):  # the inverse of restate.apply_rotary (rotation by the negative angle)
    half = t.shape[-1] // 2
    rot = torch.cat((t[..., half:], -t[..., :half]), dim=-1)
    return t * fr.cos().to(t.dtype) + rot * fr.sin().to(t.dtype)


def _chain(fr, pre, gam):  # rotary(l2norm(pre) * 8 * gamma): what precedes the attention with qk-norm, q (which 0) then k (which 1)
    from oracle import restate

    return [restate.apply_rotary(fr, restate.l2norm_scale(pre[w], 64) * gam[w][:, None, :]) for w in range(2)]


def edge_inputs(B, H, Np, key_lens, regime="edge", seed=0, nan_dead=False):
    """Inputs of the length-aware attention entry points at which the boundary key_lens[b] decides the result.

    "edge": scale 1/8, q randn, k 0.5 randn (logit std ~0.5), column 0 taken over: q[..., 0] = 4, k[..., 0] = 0 except on the last
    live key klen_b - 1, where it is max(ln klen_b - ln 4, 0) / (4 scale): that key then holds >= SHARE_MIN of every live query's
    softmax (asserted below in fp64), so dropping it moves every live output row by far more than any bound.  Every dead key n >= klen_b
    is a finite trap: its column 0 is the boosted value plus 4 / (4 scale) (+4 nats) and its v is 64 -- a leaked dead key moves the
    output by orders of magnitude; finite, because vbx_attn_fwd_lens may load dead rows of a live tile before it masks them.
    "edge_qknorm": the temperature training runs at, |q| ~ |k| ~ 8 and scale 10 (one-hot softmax, so no boost): q[..., 0] = 6,
    k[..., 0] = 0 on live keys and 7 on dead ones (logit 420 against a live maximum of ~170), v = 64 on dead keys.

    The fused backward derives the qk-norm backward from q16 / k16 themselves, so q and k must BE rotary(l2norm(pre) * 8 * gamma) of
    some pre-norm activations: with gamma[0] = gamma[32] (rotary pairs column 0 with column 32, so the pair keeps its norm) the other
    62 columns of every row are scaled by one factor such that |unrotate(row) / gamma| = 8.  Columns 0 and 32 keep their values
    exactly; the gammas are chosen so that the factor is ~1 for a typical row (0.5 .. 1.7 over all rows of all cases).  The rotary-only chain (qk_scale = 0) is linear and
    takes the same q16 / k16.

    dout is bf16 randn * 1e-3 and exactly zero on rows >= klen_b (the backward entry points' precondition).  nan_dead (the segment
    kernel promises its results "whatever q / k / v hold there"): dead rows of q, k and v are NaN instead.
    Returns a dict: q16, k16, v16 (fp16 [B, H, Np, 64], q unscaled), scale, dout (bf16 [B * Np, H * 64]), key_lens, share (the smallest
    share of the last live key), fused (pre, gam, fr, rc, rs, qknorm=True: the arguments Case takes)."""
    g = torch.Generator().manual_seed(seed)
    kl = torch.as_tensor(key_lens, dtype=torch.long)
    assert kl.shape == (B,) and int(kl.min()) >= 1 and int(kl.max()) <= Np, (key_lens, Np)
    dead = ~prefix_mask(kl, Np)  # [B, Np]
    f64 = dict(generator=g, dtype=torch.float64)
    q, k, v = (torch.randn(B, H, Np, 64, **f64) for _ in range(3))
    if regime == "edge":
        scale = 0.125
        k *= 0.5
        q[..., 0], k[..., 0] = 4.0, 0.0
        boost = (kl.double().log() - math.log(4.0)).clamp(min=0) / (4 * scale)
        for b in range(B):
            k[b, :, int(kl[b]) - 1, 0] = boost[b]
            k[b, :, int(kl[b]):, 0] = boost[b] + 4.0 / (4 * scale)
        bulk_q, bulk_k, pair_k = 1.25, 0.5, 4.0
    elif regime == "edge_qknorm":
        scale = 10.0
        q[..., 0], k[..., 0] = 0.0, 0.0
        q = q / q.norm(dim=-1, keepdim=True) * math.sqrt(64 - 36.0)
        kn = torch.where(dead, math.sqrt(64 - 49.0), 8.0)[:, None, :, None]
        k = k / k.norm(dim=-1, keepdim=True) * kn
        q[..., 0] = 6.0
        k[..., 0] = torch.where(dead, 7.0, 0.0)[:, None, :].expand(B, H, Np)
        bulk_q, bulk_k, pair_k = 1.0, 1.0, 1.25
    else:
        raise ValueError(regime)
    v = torch.where(dead[:, None, :, None], torch.full_like(v, 64.0), v)
    # ---- q, k = rotary(l2norm(pre) * 8 * gamma) with columns 0 and 32 kept
    gam = torch.tensor([bulk_q, bulk_k], dtype=torch.float64)[:, None, None] * (1 + 0.2 * torch.randn(2, H, 64, **f64))
    gam[0][:, [0, 32]], gam[1][:, [0, 32]] = 1.0, pair_k
    gam = gam.float()
    fr, rc, rs = rot_tables(Np, 16 if Np > 16 else 0)
    pre = []
    for w, t in enumerate((q, k)):
        u = _unrotate(fr.double(), t) / gam[w].double()[:, None, :]
        pair = u[..., 0] ** 2 + u[..., 32] ** 2
        rest = (u ** 2).sum(-1) - pair
        assert float(pair.max()) < 48.0, (regime, w, float(pair.max()))  # the other columns keep at least a quarter of the norm
        fac = ((64.0 - pair) / rest).sqrt()
        keep0, keep32 = u[..., 0].clone(), u[..., 32].clone()
        u = u * fac[..., None]
        u[..., 0], u[..., 32] = keep0, keep32
        rows = 0.5 + torch.rand(B, H, Np, **f64)  # |pre| per row: the norm backward must divide by it
        pre.append((u * rows[..., None]).float())
    pre = torch.stack(pre)
    hats = _chain(fr.double(), pre.double(), gam.double())
    q16, k16, v16 = hats[0].half(), hats[1].half(), v.half()
    dout = bf(torch.randn(B * Np, H * 64, generator=g) * 1e-3)
    dout = torch.where(dead.reshape(B * Np, 1), torch.zeros_like(dout), dout)
    # ---- the condition, in fp64 on the rounded operands
    share = 1.0
    if regime == "edge":
        _, q_eff = q_operand(q16, q_prescale(scale))
        for b in range(B):
            n = int(kl[b])
            w = (torch.einsum("hid,hjd->hij", q_eff[b, :, :n], k16[b, :, :n].double()) * scale).softmax(-1)
            share = min(share, float(w[..., n - 1].min()))
        assert share >= SHARE_MIN, f"edge inputs {(B, H, Np, tuple(key_lens), seed)}: the last live key holds only {share:.4g}"
    if nan_dead:
        nan = dead[:, None, :, None]
        q16, k16, v16 = (torch.where(nan, torch.full_like(t, math.nan), t) for t in (q16, k16, v16))
    return dict(q16=q16, k16=k16, v16=v16, scale=scale, dout=dout, key_lens=tuple(int(x) for x in kl), share=share, B=B, H=H, Np=Np,
                fused=dict(pre=pre, gam=gam, fr=fr, rc=rc, rs=rs, qknorm=True))


# ----------------------------------------------------------------------------- length-aware attention: fp64 reference
def lens_reference(inp, c=None):
    """restate.attend in fp64 on the rounded operands with the prefix mask n < key_lens[b], autograd with the zeroed dout, then the
    fp64 chains of the fused backward: rotary(l2norm(pre) * 8 * gamma) (dpre, dgam) and rotary alone (dpre_rot).  c: the prescale q16
    carries (vbx_attn_q_prescale(scale); the host's value by default).  lse in log2 units."""
    from oracle import restate

    B, H, Np, scale, f = inp["B"], inp["H"], inp["Np"], inp["scale"], inp["fused"]
    mask = prefix_mask(inp["key_lens"], Np)
    _, q_eff = q_operand(inp["q16"], q_prescale(scale) if c is None else c)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q_eff, inp["k16"], inp["v16"]))
    out = restate.attend(qr, kr, vr, mask=mask, scale=scale)
    out.backward(heads(inp["dout"].double(), B, Np, H))
    sim = (torch.einsum("bhid,bhjd->bhij", qr.detach(), kr.detach()) * scale).masked_fill(~mask[:, None, None, :], -math.inf)
    ref = dict(out=out.detach(), lse=torch.logsumexp(sim, dim=-1) / math.log(2.0), dq=qr.grad, dk=kr.grad, dv=vr.grad)
    pre, gam, fr = f["pre"].double().requires_grad_(True), f["gam"].double().requires_grad_(True), f["fr"].double()
    torch.autograd.backward(_chain(fr, pre, gam), [qr.grad, kr.grad])
    ref["dpre"], ref["dgam"] = pre.grad, gam.grad
    ref["dpre_rot"] = torch.stack((_unrotate(fr, qr.grad), _unrotate(fr, kr.grad)))  # the transpose of a rotation is its inverse
    return ref


def segs_layout(klens, extra_tiles):
    """Segments of these key lengths, each aligned to 128 rows, `extra_tiles` tiles of -1 behind them -> (seg_start, Mp, tile_seg)."""
    starts, row = [], 0
    for kl in klens:
        starts.append(row)
        row += L_tiles(kl) * TILE
    tile_seg = [s for s, kl in enumerate(klens) for _ in range(L_tiles(kl))] + [-1] * extra_tiles
    return starts, row + TILE * extra_tiles, tile_seg


def segs_inputs(H, klens, extra_tiles, seed=0):
    """One packed row [1, H, Mp, 64] of "edge" segments (edge_inputs per segment, B = 1, Np = its aligned size); every dead row of q, k
    and v -- inside the segments and in the -1 tiles -- is NaN.  -> dict q16, k16, v16, scale, klens, seg_start, tile_seg, Mp, H."""
    starts, Mp, tile_seg = segs_layout(klens, extra_tiles)
    q16, k16, v16 = (torch.full((1, H, Mp, 64), math.nan, dtype=torch.float16) for _ in range(3))
    for s, kl in enumerate(klens):
        size = L_tiles(kl) * TILE
        e = edge_inputs(1, H, size, (kl,), "edge", seed=seed + 13 * s + kl, nan_dead=True)
        for dst, src in ((q16, "q16"), (k16, "k16"), (v16, "v16")):
            dst[:, :, starts[s]:starts[s] + size] = e[src]
    return dict(q16=q16, k16=k16, v16=v16, scale=0.125, klens=tuple(klens), seg_start=starts, tile_seg=tile_seg, Mp=Mp, H=H)


def segs_reference(inp, c=None):
    """Per segment, restate.attend in fp64 on that segment's live rows alone -> out [1, H, Mp, 64] and lse [1, H, Mp] (log2 units),
    zero on dead rows."""
    from oracle import restate

    H, Mp, scale = inp["H"], inp["Mp"], inp["scale"]
    out, lse = torch.zeros(1, H, Mp, 64, dtype=torch.float64), torch.zeros(1, H, Mp, dtype=torch.float64)
    for s0, kl in zip(inp["seg_start"], inp["klens"]):
        rows = slice(s0, s0 + kl)
        _, q = q_operand(inp["q16"][:, :, rows], q_prescale(scale) if c is None else c)
        k, v = inp["k16"][:, :, rows].double(), inp["v16"][:, :, rows].double()
        out[:, :, rows] = restate.attend(q, k, v, scale=scale)
        lse[:, :, rows] = torch.logsumexp(torch.einsum("bhid,bhjd->bhij", q, k) * scale, dim=-1) / math.log(2.0)
    return dict(out=out, lse=lse)


# ----------------------------------------------------------------------------- length-aware attention: checks
# Every tensor is a CPU tensor over the rows < Np: [B, H, Np, 64] (lse [B, H, Np], gpart [2, B, tiles, H, 64]).  The kernels' tests cut
# the guard rows off and check them on their own.
def _nan_free(chk, what, tensors):
    chk.true(f"{what}: no NaN in any row < Np", not any(bool(torch.isnan(t.float()).any()) for t in tensors))


def _live(t, key_lens, axis):
    """t with the rows >= key_lens[b] along `axis` set to 0"""
    Np = t.shape[axis]
    m = prefix_mask(key_lens, Np).reshape([len(key_lens)] + [Np if d == axis % t.dim() else 1 for d in range(1, t.dim())])
    return torch.where(m, t, torch.zeros_like(t))


def check_lens_fwd(chk, key_lens, got, ref, bounds, what="forward"):
    """got: out16, out_bf16 [B, H, Np, 64], lse [B, H, Np].  Live rows against the reference, globally and per tile (rows >= klen_b
    are padding: zeroed in both tensors first); rows of a 128-row tile wholly at or past klen_b exactly 0 with lse 1e30; no NaN."""
    o16, ob, lse = got["out16"].float().cpu(), got["out_bf16"].float().cpu(), got["lse"].float().cpu()
    _nan_free(chk, what, (o16, ob, lse))
    for name, t in (("out16", o16), ("out_bf16", ob)):
        g, r = _live(t, key_lens, 2), _live(ref["out"], key_lens, 2)
        chk.le(name, rel_err(g, r), bounds[name])
        chk.tiles(name, g, r, bounds[name + "_tile"])
    g, r = _live(lse, key_lens, 2), _live(ref["lse"], key_lens, 2)
    chk.le("lse max abs", max_err(g, r), bounds["lse"])
    chk.tiles("lse", g, r, bounds["lse_tile"], axis=-1)
    ok = True
    for b, kl in enumerate(key_lens):
        d0 = L_tiles(kl) * TILE  # the first row of the first wholly dead tile
        ok = ok and not bool(o16[b, :, d0:].any()) and not bool(ob[b, :, d0:].any()) and bool((lse[b, :, d0:] == DEAD_LSE).all())
    chk.true(f"{what}: rows of wholly dead tiles are 0 with lse 1e30", ok)


def _check_grads(chk, key_lens, got, refs, bounds, tag):
    """got / refs: name -> [B, H, Np, 64].  A batch row with ONE live key has reference gradients of q and k that are exactly 0
    (dS = P (dP - delta) with P = 1), where the kernels leave their rounding of dP against delta: those batch rows are held to
    zero_abs and left out of the relative errors; everything else is checked globally and per tile, dead rows included (their reference
    is exactly 0, and so must they be)."""
    for name, g in got.items():
        g, r = g.double().cpu().clone(), refs[name]
        flat = [b for b in range(len(key_lens)) if float(r[b].abs().max()) == 0]
        if flat:
            chk.le(f"{name}{tag} max abs (reference 0, batch rows {flat})", max_err(g[flat], r[flat]), bounds["zero_abs"])
            live = prefix_mask(key_lens, g.shape[2])
            for b in flat:  # only the live rows are excused: a dead row must be exactly 0 below
                g[b][:, live[b]] = 0
        if len(flat) < len(key_lens):
            chk.le(name + tag, rel_err(g, r), bounds[name])
            chk.tiles(name + tag, g, r, bounds[name + "_tile"], floor=bounds.get("floor", {}).get(name, 1e-3))


def _check_dead_and_boundary(chk, key_lens, got, refs, tag, boundary, row_floor=None):
    """Every row >= key_lens[b] of every tensor exactly 0, and the row of key key_lens[b] - 1 of the `boundary` tensors (got name,
    reference name) within BOUNDARY_ROW of the reference per (b, h).  row_floor (name -> fraction; the one-hot regime only, where
    dS = P (dP - delta) cancels and a single row of dk has a reference far below its rounding noise, see BOUNDS): the row's error is
    taken against at least that fraction of the rms row norm of the reference, as `floor` does for the tiles."""
    ok = {name: True for name in got}
    worst = {}
    row_floor = row_floor or {}
    rms = {rname: float(refs[rname].norm(dim=-1).pow(2).mean().sqrt()) for _, rname in boundary}
    for b, kl in enumerate(key_lens):
        for name, g in got.items():
            ok[name] = ok[name] and bool((g[b, :, kl:].float() == 0).all())
        for name, rname in boundary:
            g, r = got[name][b, :, kl - 1].double().cpu(), refs[rname][b, :, kl - 1]
            rn = r.norm(dim=-1)  # per head
            if float(rn.min()) == 0:
                continue  # one live key: the row's reference is exactly 0 (held to zero_abs above)
            e = float(((g - r).norm(dim=-1) / rn.clamp(min=row_floor.get(name, 0.0) * rms[rname])).max())
            e = math.inf if math.isnan(e) else e
            worst[name] = max(worst.get(name, 0.0), e)
    for name in got:
        chk.true(f"{name}{tag}: rows >= key_lens[b] are exactly 0", ok[name])
    for name, e in worst.items():
        chk.le(f"{name}{tag} boundary row key_lens[b] - 1", e, BOUNDARY_ROW)


def check_lens_bwd(chk, key_lens, got, ref, bounds, tag="", row_floor=None):
    """got: dq, dk, dv [B, H, Np, 64] of vbx_attn_bwd_lens."""
    got = {n: got[n].float().cpu() for n in ("dq", "dk", "dv")}
    _nan_free(chk, "backward" + tag, got.values())
    _check_grads(chk, key_lens, got, ref, bounds, tag)
    _check_dead_and_boundary(chk, key_lens, got, ref, tag, boundary=(("dk", "dk"), ("dv", "dv")), row_floor=row_floor)


def check_lens_fused(chk, key_lens, got, ref, bounds, qknorm=True, tag=" (fused)", row_floor=None):
    """got: dpre_q, dpre_k, dv [B, H, Np, 64] (the q | k | v columns of dqkv) and, with qk-norm, gpart [2, B, tiles, H, 64]."""
    dpre = ref["dpre"] if qknorm else ref["dpre_rot"]
    refs = dict(dpre_q=dpre[0], dpre_k=dpre[1], dv=ref["dv"])
    g = {n: got[n].float().cpu() for n in ("dpre_q", "dpre_k", "dv")}
    _nan_free(chk, "fused backward" + tag, g.values())
    _check_grads(chk, key_lens, g, refs, bounds, tag)
    # the boundary row of dk is judged before the norm backward mixes it: dpre_k of that row against the reference's
    _check_dead_and_boundary(chk, key_lens, g, refs, tag, boundary=(("dpre_k", "dpre_k"), ("dv", "dv")), row_floor=row_floor)
    if not qknorm:
        return
    gp = got["gpart"].float().cpu()
    chk.true(f"gpart{tag}: no NaN in any record", not bool(torch.isnan(gp).any()))
    chk.true(f"gpart{tag}: records of wholly dead tiles are exactly 0",
             all(bool((gp[:, b, L_tiles(kl):] == 0).all()) for b, kl in enumerate(key_lens)))
    dgam = gp.double().sum((1, 2))
    if float(ref["dgam"].abs().max()) == 0:
        chk.le(f"dgamma{tag} max abs (reference 0)", max_err(dgam, ref["dgam"]), bounds["dgamma_zero_abs"])
    else:
        chk.le("dgamma" + tag, rel_err(dgam, ref["dgam"]), bounds["dgamma"])


def check_segs(chk, inp, got, ref, bounds):
    """got: out16, out_bf16 [1, H, Mp, 64], lse [1, H, Mp] of vbx_attn_fwd_segs.  Live rows against the per-segment reference; every
    dead row and every row of a -1 tile exactly 0 with lse 1e30; no NaN anywhere although the dead inputs are NaN."""
    o16, ob, lse = got["out16"].float().cpu(), got["out_bf16"].float().cpu(), got["lse"].float().cpu()
    _nan_free(chk, "segments", (o16, ob, lse))
    live = torch.zeros(inp["Mp"], dtype=torch.bool)
    for s0, kl in zip(inp["seg_start"], inp["klens"]):
        live[s0:s0 + kl] = True
    chk.true("segments: dead rows and -1 tiles are 0 with lse 1e30",
             not bool(o16[:, :, ~live].any()) and not bool(ob[:, :, ~live].any()) and bool((lse[:, :, ~live] == DEAD_LSE).all()))
    zero = lambda t: torch.where(live.reshape([1, 1, -1] + [1] * (t.dim() - 3)), t, torch.zeros_like(t))
    for name, t in (("out16", o16), ("out_bf16", ob)):
        chk.le(name, rel_err(zero(t), ref["out"]), bounds[name])
        chk.tiles(name, zero(t), ref["out"], bounds[name + "_tile"])
    chk.le("lse max abs", max_err(zero(lse), ref["lse"]), bounds["lse"])
    chk.tiles("lse", zero(lse), ref["lse"], bounds["lse_tile"], axis=-1)


# The cases of tests/test_attn_lens_edges_gpu.py: (B, H, Np, key_lens, regime).  tests/test_attn_check_cpu.py builds every one, so
# the share condition of "edge" is asserted without a GPU.
LENS_CASES = [
    (3, 3, 1, (1, 1, 1)),  # one key: reference gradients exactly 0 (zero_abs)
    (3, 3, 16, (1, 15, 16)), (3, 3, 17, (1, 16, 17)),  # the 16 x 16 tail role alone; 17 leaves it
    (3, 3, 64, (1, 63, 64)), (3, 3, 65, (1, 63, 64)), (3, 3, 65, (64, 65, 2)),  # exactly one full key tile; one key in a second tile
    (3, 3, 129, (128, 129, 65)),  # query tile 1 is the 1-row tail role: wholly dead (128, 65) and live (129)
    (3, 3, 145, (2, 17, 130)), (3, 3, 145, (128, 129, 145)),  # tail role left (17 rows); boundary on and just past the tile seam
    (3, 3, 272, (257, 128, 63)), (3, 3, 272, (256, 272, 1)), (1, 17, 272, (256,)),  # 16-row tail role live with one key / dead
    (3, 3, 1029, (1028, 961, 129)), (3, 3, 1029, (1024, 1025, 1029)),  # 5-row tail; ntiles 17, 16, 3; tail tile dead / one row / full
    (3, 3, 1040, (1, 1025, 1040)), (3, 3, 1040, (64, 65, 1024)), (3, 3, 1040, (1039, 960, 193)),  # the benchmark's shape
]
LENS_CASES = [c + ("edge",) for c in LENS_CASES] + [
    (3, 3, 145, (2, 17, 130), "edge_qknorm"), (3, 3, 272, (257, 128, 63), "edge_qknorm"), (3, 3, 1040, (1, 1025, 1040), "edge_qknorm")]
SEGS_CASES = [  # (H, segment key lengths, trailing -1 tiles)
    (3, (1, 64, 65, 128, 129, 1025, 1040), 2),
    (3, (1040, 1025, 129, 128, 65, 64, 1), 2),
    (8, (1040, 1, 1029), 1),
]


def lens_case_id(case):
    B, H, Np, kl, regime = case
    return f"{regime}-B{B}H{H}-Np{Np}-" + "_".join(str(v) for v in kl)


def lens_case_seed(case):
    B, H, Np, kl, regime = case
    return 7 * Np + sum(kl) + (1000 if regime == "edge_qknorm" else 0)
