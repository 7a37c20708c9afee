"""Error metrics and input builders of the attention tests (tests/test_ops_gpu.py, tests/test_attn_edges_gpu.py).

`rel_err` is one Frobenius norm over a whole tensor: an error confined to one (b, h) tile of 128 rows -- a ragged tail, one padded work
id, one ring slot -- hides under it (a 30 % error in one 16-row dq tail tile of (B, H, Np) = (2, 2, 1040) raises the global dq error by
0.3 * sqrt(16 / 4160) ~ 0.019).  `tile_errors` measures every (b, h, 128-row tile) on its own, at the kernels' own tiling: query tiles
for out, lse and dq, key tiles for dk and dv.
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
