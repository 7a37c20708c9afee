"""Attention kernels at their edges, against the fp64 restatement of attend.py:121-135 (restate.attend, autograd for the backward) on
the same rounded operands, checked per (b, h, 128-row tile) as well as globally (tests/attn_check.py).

The kernels have several roles -- full 128-row tiles, a 16 x 16 MFMA role for tails of <= 16 rows, full-tile code with per-element
masks for longer tails, the dropout bodies, the fused qk-norm / rotary backward epilogue -- and an XCD-aware work order that pads
B * H up to a multiple of 8.  The cases below sweep the tail sizes and B * H values where those meet, the softmax regimes where the
online rescale between key tiles is not a no-op (the reference's qk-norm temperature makes the softmax one-hot, where it always is),
mask shapes down to one valid key and a fully masked batch, and dropout on every entry point that takes it.

Every output buffer is pre-filled with NaN and carries one guard row past its end; the q and k blocks of the [B * Np, 3 * H * 64]
buffer the dv of vbx_attn_bwd lands in stay NaN.  Every entry point is run twice and must repeat bit for bit.  Bounds are in
attn_check.BOUNDS with the values measured on MI355X.
"""
import math

import pytest
import torch

from attn_check import BOUNDS, Checks, L_tiles, all_nan, bf, heads, max_err, qpre, rel_err, rot_tables, same_bits
from oracle import restate

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return _lib


@pytest.fixture
def bwd_variant(request, L):
    """Both two-body attention backward kernels (as in test_ops_gpu.py): 1 = statistics folded into the MFMA accumulator (default),
    3 = the same bodies without the fold.  Parametrized per test through VARIANTS so that the two run back to back on one cached
    reference."""
    L.lib().vbx_attn_bwd_select(request.param)
    yield request.param
    L.lib().vbx_attn_bwd_select(0)


VARIANTS = pytest.mark.parametrize("bwd_variant", [3, 1], ids=["unfolded", "folded"], indirect=True)


def st():
    return torch.cuda.current_stream().cuda_stream


def nans(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


# ----------------------------------------------------------------------------- inputs
def make_qkv(B, H, Np, temp, seed):
    """q, k, v (fp16, q unscaled) and the softmax scale of one temperature regime.
    qknorm: |q| = |k| = 8, scale 10 (the reference's qk-norm regime; logits of std ~80, one-hot softmax)
    std1 / std8: randn q, k at scale 1/8 / 1 (logit std ~1 / ~8; std1 is the Transformer default attn_qk_norm=False, 64^-0.5)
    ramp / ramp_rev: logits = a staircase rising (falling) by 2 nats over the keys in steps of 64 keys, plus noise of std 0.02:
    the running maximum rises in every 64-key step (ramp) or is set by the first one (ramp_rev), and every 128-key tile keeps a
    softmax weight >= 1e-3 (both checked here)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, H, Np, 64, generator=g)
    if temp in ("qknorm", "std1", "std8"):
        q = torch.randn(B, H, Np, 64, generator=g)
        k = torch.randn(B, H, Np, 64, generator=g)
        if temp == "qknorm":
            q, k = q / q.norm(dim=-1, keepdim=True) * 8, k / k.norm(dim=-1, keepdim=True) * 8
        return q.half(), k.half(), v.half(), {"qknorm": 10.0, "std1": 0.125, "std8": 1.0}[temp]
    assert temp in ("ramp", "ramp_rev")
    scale, A, R = 0.125, 4.0, 2.0
    steps = max((Np - 1) // 64, 1)
    lvl = (torch.arange(Np) // 64).float() / steps
    if temp == "ramp_rev":
        lvl = 1 - lvl
    q = torch.randn(B, H, Np, 64, generator=g)
    k = torch.randn(B, H, Np, 64, generator=g) * 0.02
    q[..., 0], k[..., 0] = A, R * lvl / (A * scale)
    q, k = q.half(), k.half()
    s = torch.einsum("bhid,bhjd->bhij", q.double(), k.double()) * scale
    nb = -(-Np // 64)
    bmax = torch.stack([s[..., 64 * t:64 * (t + 1)].amax(-1) for t in range(nb)], -1)
    if temp == "ramp":
        assert (bmax[..., 1:] > bmax[..., :-1]).all(), "the running maximum must rise in every 64-key step"
    else:
        assert (bmax[..., 1:] < bmax[..., :1]).all(), "the first 64-key step must hold the maximum"
    w = s.softmax(-1)
    tw = torch.stack([w[..., 128 * t:128 * (t + 1)].sum(-1) for t in range(-(-Np // 128))], -1)
    assert float(tw.min()) >= 1e-3, float(tw.min())
    return q, k, v.half(), scale


def make_mask(kind, B, Np, seed=0):
    if kind is None:
        return None
    m = torch.ones(B, Np, dtype=torch.bool)
    if kind == "block":  # a whole key tile and a 32-key block
        m[:, 128:256] = False
        m[:, 448:480] = False
    elif kind == "one":  # exactly one valid key: the first in one batch row, the last in the other
        m[:] = False
        m[0, 0] = True
        m[B - 1, Np - 1] = True
    elif kind == "rand":
        m = torch.rand(B, Np, generator=torch.Generator().manual_seed(seed)) < 0.5
        m[:, 0] |= ~m.any(dim=1)
    elif kind == "empty":  # batch row 0 fully masked, the next one not masked at all
        m[0] = False
    else:
        raise ValueError(kind)
    return m


def make_pre(B, H, Np, qknorm, seed):
    """The fused backward's inputs: pre-norm q, k, qk-norm gammas and rotary tables; q, k = rotary(l2norm(pre) * 8 * gamma) with
    qk-norm (scale 10), rotary(pre) without (scale 1/8)."""
    g = torch.Generator().manual_seed(seed)
    pre = torch.randn(2, B, H, Np, 64, generator=g)
    gam = 1 + 0.2 * torch.randn(2, H, 64, generator=g)
    fr, rc, rs = rot_tables(Np, 16 if Np > 16 else 0)
    hats = [restate.apply_rotary(fr, restate.l2norm_scale(pre[w], 64) * gam[w][:, None, :] if qknorm else pre[w]) for w in range(2)]
    v = torch.randn(B, H, Np, 64, generator=g).half()
    return hats[0].half(), hats[1].half(), v, (10.0 if qknorm else 0.125), dict(pre=pre, gam=gam, fr=fr, rc=rc, rs=rs, qknorm=qknorm)


class Case:
    """One set of inputs, its fp64 reference (computed once, shared by every kernel variant that runs on it) and the device copies."""

    def __init__(self, L, B, H, Np, q16, k16, v16, scale, mask, p=None, fused=None, seed=0):
        self.B, self.H, self.Np, self.I, self.scale, self.mask, self.p, self.fused = B, H, Np, H * 64, scale, mask, p, fused
        qs, q_eff = qpre(L, q16, scale)
        self.qd, self.kd, self.vd = qs.to(dev), k16.to(dev), v16.to(dev)
        self.qb, self.kb, self.vb = bf(q16.float()).to(dev), bf(k16.float()).to(dev), bf(v16.float()).to(dev)
        self.md = mask.to(dev) if mask is not None else None
        g = torch.Generator().manual_seed(seed + 5)
        self.dout = bf(torch.randn(B * Np, H * 64, generator=g) * 1e-3)  # gradient-sized values (fp16 would flush these)
        self.doutd = self.dout.to(dev)
        drop = None
        if p is not None:
            import philox_ref as PR
            W = L.lib().vbx_dropout_bits_words(Np)
            self.rm = torch.full((B * H, Np, W), -1, dtype=torch.int32, device=dev)
            self.cm = torch.full((B * H, Np, W), -1, dtype=torch.int32, device=dev)
            L.call("vbx_attn_dropout_bits", self.rm, self.cm, B * H, Np, 1000 + seed, 4, p, st())
            torch.cuda.synchronize()
            keep = torch.from_numpy(PR.unpack_bits(self.rm.cpu().numpy(), Np)).view(B, H, Np, Np)
            drop = keep.double() * L.lib().vbx_dropout_keep_scale(p)
        # ---- fp64 reference on the rounded operands
        qr, kr, vr = (t.double().requires_grad_(True) for t in (q_eff, k16, v16))
        out = restate.attend(qr, kr, vr, mask=mask, scale=scale, drop=drop)
        out.backward(heads(self.dout.double(), B, Np, H))
        sim = torch.einsum("bhid,bhjd->bhij", qr.detach(), kr.detach()) * scale
        if mask is not None:
            sim = sim.masked_fill(~mask[:, None, None, :], -math.inf)
        lse = torch.logsumexp(sim, dim=-1) / math.log(2.0)
        if mask is not None:  # a fully masked batch: uniform softmax, logits taken as 0 (include/vbx.h)
            lse[~mask.any(dim=1)] = math.log2(Np)
        self.ref = dict(out=out.detach(), lse=lse, dq=qr.grad, dk=kr.grad, dv=vr.grad)
        if fused is not None:  # rotary + qk-norm backward of the reference's dq, dk in fp64
            pre = fused["pre"].double().requires_grad_(True)
            gam = fused["gam"].double().requires_grad_(True)
            fr = fused["fr"].double()
            hats = [restate.apply_rotary(fr, restate.l2norm_scale(pre[w], 64) * gam[w][:, None, :] if fused["qknorm"] else pre[w])
                    for w in range(2)]
            torch.autograd.backward(hats, [qr.grad, kr.grad])
            self.ref["dpre"] = pre.grad
            self.ref["dgam"] = gam.grad if fused["qknorm"] else None

    # ---- kernels; every buffer NaN-filled with one guard row past its end
    def fwd(self, L):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        o16, ob, lse = nans((B * Np + 1, I), torch.float16), nans((B * Np + 1, I), torch.bfloat16), nans((B * H * Np + 1,), torch.float32)
        if self.p is None:
            L.call("vbx_attn_fwd", self.qd, self.kd, self.vd, self.md, o16, ob, lse, B, H, Np, self.scale, st())
        else:
            L.call("vbx_attn_fwd_dropout", self.qd, self.kd, self.vd, self.md, o16, ob, lse, B, H, Np, self.scale, self.rm, self.p, st())
        torch.cuda.synchronize()
        return o16, ob, lse

    def bwd(self, L, o16, lse):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        dq, dk = nans((B * H * Np + 1, 64), torch.float32), nans((B * H * Np + 1, 64), torch.float32)
        d = nans((B * Np + 1, 3 * I), torch.bfloat16)
        delta = torch.empty(B, H, Np, device=dev)
        args = (self.qd, self.kd, self.qb, self.kb, self.vb, self.md, o16, 1, self.doutd, lse, delta, dq, dk, d[:, 2 * I:].data_ptr(),
                3 * I, B, H, Np, self.scale)
        if self.p is None:
            L.call("vbx_attn_bwd", *args, None, st())
        else:
            L.call("vbx_attn_bwd_dropout", *args, self.rm, self.cm, self.p, st())
        torch.cuda.synchronize()
        return dq, dk, d

    def bwd_fused(self, L, o16, lse):
        B, H, Np, I, f = self.B, self.H, self.Np, self.I, self.fused
        d = nans((B * Np + 1, 3 * I), torch.bfloat16)
        gp = torch.zeros(2, B * L.lib().vbx_attn_bwd_fused_tiles(Np), H, 64, device=dev)
        delta = torch.empty(B, H, Np, device=dev)
        rn = (1 / f["pre"].norm(dim=-1)).float().to(dev)
        gq, gk = f["gam"][0].float().to(dev), f["gam"][1].float().to(dev)
        args = (self.qd, self.kd, self.qb, self.kb, self.vb, self.md, o16, 1, self.doutd, lse, delta, rn[0], rn[1], gq, gk,
                f["rc"].to(dev), f["rs"].to(dev), 8.0 if f["qknorm"] else 0.0, d, 3 * I, gp, B, H, Np, self.scale, None)
        if self.p is None:
            L.call("vbx_attn_bwd_fused", *args, st())
        else:
            L.call("vbx_attn_bwd_fused_dropout", *args, self.rm, self.cm, self.p, st())
        torch.cuda.synchronize()
        return d, gp

    # ---- checks
    def check_fwd(self, chk, o16, ob, lse, bounds):
        B, H, Np, r = self.B, self.H, self.Np, self.ref
        n = B * Np
        chk.true("out16 / out_bf16 / lse guard rows untouched", all_nan(o16[n]) and all_nan(ob[n]) and all_nan(lse[B * H * Np:]))
        for name, t in (("out16", o16), ("out_bf16", ob)):
            got = heads(t[:n], B, Np, H)
            chk.le(name, rel_err(got, r["out"]), bounds[name])
            chk.tiles(name, got, r["out"], bounds[name + "_tile"])
        lg = lse[:B * H * Np].view(B, H, Np)
        chk.le("lse max abs", max_err(lg, r["lse"]), bounds["lse"])
        chk.tiles("lse", lg, r["lse"], bounds["lse_tile"], axis=-1)

    def check_grads(self, chk, got, bounds, names=("dq", "dk", "dv"), tag=""):
        for name in names:
            g = got[name]
            ref = {"dpre_q": lambda: self.ref["dpre"][0], "dpre_k": lambda: self.ref["dpre"][1]}.get(name, lambda: self.ref[name])()
            if float(ref.abs().max()) == 0:
                # a single valid key per row (Np = 1, one unmasked key): dS = P (dP - delta) is exactly 0 in fp64, but the kernels' dP
                # (bf16 v) and delta (fp16 O) round differently -- what is left must stay at that rounding level
                chk.le(name + tag + " max abs (reference 0)", max_err(g, ref), bounds["zero_abs"])
                continue
            chk.le(name + tag, rel_err(g, ref), bounds[name])
            chk.tiles(name + tag, g, ref, bounds[name + "_tile"], floor=bounds.get("floor", {}).get(name, 1e-3))

    def check_bwd(self, chk, dq, dk, d, bounds):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        n, m = B * Np, B * H * Np
        chk.true("dq / dk guard rows untouched", all_nan(dq[m]) and all_nan(dk[m]))
        chk.true("dv: q and k blocks and the guard row untouched", all_nan(d[:n, :2 * I]) and all_nan(d[n]))
        got = dict(dq=dq[:m].view(B, H, Np, 64), dk=dk[:m].view(B, H, Np, 64), dv=heads(d[:n, 2 * I:], B, Np, H))
        self.check_grads(chk, got, bounds)

    def check_fused(self, chk, d, gp, bounds):
        B, H, Np, I = self.B, self.H, self.Np, self.I
        n = B * Np
        chk.true("d(qkv) guard row untouched", all_nan(d[n]))
        got = dict(dpre_q=heads(d[:n, :I], B, Np, H), dpre_k=heads(d[:n, I:2 * I], B, Np, H), dv=heads(d[:n, 2 * I:], B, Np, H))
        self.check_grads(chk, got, bounds, names=("dpre_q", "dpre_k", "dv"), tag=" (fused)")
        if self.ref["dgam"] is not None:
            if float(self.ref["dgam"].abs().max()) == 0:
                chk.le("dgamma max abs (reference 0)", max_err(gp.sum(1), self.ref["dgam"]), bounds["dgamma_zero_abs"])
            else:
                chk.le("dgamma", rel_err(gp.sum(1), self.ref["dgam"]), bounds["dgamma"])
            if self.mask is not None:  # gamma partial rows of a fully masked batch are exactly zero
                tiles = L_tiles(Np)
                for b in range(B):
                    if not bool(self.mask[b].any()):
                        chk.true(f"gamma partials of masked batch {b} are 0", bool((gp[:, b * tiles:(b + 1) * tiles] == 0).all()))


def run_fwd_bwd(L, c, chk, bounds):
    o16, ob, lse = c.fwd(L)
    c.check_fwd(chk, o16, ob, lse, bounds)
    o16b, obb, lseb = c.fwd(L)
    chk.true("forward repeats bit for bit", same_bits(o16, o16b) and same_bits(ob, obb) and same_bits(lse, lseb))
    dq, dk, d = c.bwd(L, o16, lse)
    c.check_bwd(chk, dq, dk, d, bounds)
    dq2, dk2, d2 = c.bwd(L, o16, lse)
    chk.true("backward repeats bit for bit", same_bits(dq, dq2) and same_bits(dk, dk2) and same_bits(d, d2))
    return o16, lse


_CASES = {}


def cached(key, build):
    """The fp64 reference of a case is shared by the two backward variants (the dominant cost of these tests)."""
    if key not in _CASES:
        _CASES.clear()
        _CASES[key] = build()
    return _CASES[key]


# ----------------------------------------------------------------------------- (a) tail sizes x B * H, spread softmax
TAIL_NP = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 145]
BH_SHAPES = {3: (1, 3), 9: (3, 3), 17: (1, 17)}  # 9 and 17: padded, idle work ids of the XCD-aware order
TAIL_CASES = [(bh, Np) for Np in TAIL_NP for bh in (3, 9, 17)] + [(bh, Np) for Np in (1023, 1025, 1041) for bh in (3, 9)]


@VARIANTS
@pytest.mark.parametrize("BH,Np", TAIL_CASES)
def test_attn_tails(L, BH, Np, bwd_variant):
    """vbx_attn_fwd / vbx_attn_bwd at logit std ~1 (scale 1/8, randn q, k): every tail role and B * H around the padding to 8."""
    B, H = BH_SHAPES[BH]
    c = cached(("tails", BH, Np), lambda: Case(L, B, H, Np, *make_qkv(B, H, Np, "std1", seed=Np * 31 + BH), mask=None, seed=Np))
    chk = Checks(f"tails B={B} H={H} Np={Np} variant={bwd_variant}")
    run_fwd_bwd(L, c, chk, BOUNDS["spread"])
    chk.done()


@VARIANTS
@pytest.mark.parametrize("B,H,Np", [(3, 3, 1), (3, 3, 16), (3, 3, 17), (3, 3, 65), (3, 3, 129), (1, 3, 1041)])
def test_attn_bwd_fused_tails(L, B, H, Np, bwd_variant):
    """vbx_attn_bwd_fused with qk-norm + rotary (the training step's backward) against the fp64 chain attend -> rotary(l2norm * gamma)."""
    def build():
        q16, k16, v16, scale, f = make_pre(B, H, Np, True, seed=Np + 17)
        return Case(L, B, H, Np, q16, k16, v16, scale, mask=None, fused=f, seed=Np)
    c = cached(("fused", B, H, Np), build)
    chk = Checks(f"fused B={B} H={H} Np={Np} variant={bwd_variant}")
    o16, _, lse = c.fwd(L)
    d, gp = c.bwd_fused(L, o16, lse)
    c.check_fused(chk, d, gp, BOUNDS["fused"])
    d2, gp2 = c.bwd_fused(L, o16, lse)
    chk.true("fused backward repeats bit for bit", same_bits(d, d2) and same_bits(gp, gp2))
    chk.done()


# ----------------------------------------------------------------------------- (b) temperature x mask
TEMPS = ["qknorm", "std1", "std8", "ramp", "ramp_rev"]
MASKS = [None, "block", "one", "rand", "empty"]


@VARIANTS
@pytest.mark.parametrize("Np", [1029, 1040])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("mask", MASKS, ids=[str(m) for m in MASKS])
def test_attn_temperature_mask(L, Np, temp, mask, bwd_variant):
    """Online-softmax rescale between 9 key tiles (std1 / std8 / ramps), masks down to one valid key and a fully masked batch row
    (reference: uniform softmax over all keys, attend.py:126), at a 5-row and a 16-row tail."""
    B, H = 2, 2
    c = cached(("tm", Np, temp, mask), lambda: Case(L, B, H, Np, *make_qkv(B, H, Np, temp, seed=Np + 7 * TEMPS.index(temp)),
                                                  mask=make_mask(mask, B, Np, seed=Np), seed=Np + 1))
    chk = Checks(f"temperature/mask Np={Np} temp={temp} mask={mask} variant={bwd_variant}")
    run_fwd_bwd(L, c, chk, BOUNDS["qknorm" if temp == "qknorm" else "spread"])
    chk.done()


# ----------------------------------------------------------------------------- (c) dropout
@pytest.mark.parametrize("Np", [1, 16, 17, 129, 1025, 1040])
@pytest.mark.parametrize("qknorm", [False, True], ids=["spread", "qknorm"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attn_dropout_edges(L, Np, qknorm, p):
    """vbx_attn_fwd_dropout, vbx_attn_bwd_dropout and vbx_attn_bwd_fused_dropout (the runtime's training backward with
    attn_dropout > 0) against the fp64 reference given the kernels' own keep bits.  p = 0.5 runs with batch row 0 fully masked."""
    B, H = 2, 2
    q16, k16, v16, scale, f = make_pre(B, H, Np, qknorm, seed=3 * Np + 1)
    c = Case(L, B, H, Np, q16, k16, v16, scale, mask=make_mask("empty" if p == 0.5 else None, B, Np), p=p, fused=f, seed=Np + 2)
    chk = Checks(f"dropout Np={Np} qknorm={qknorm} p={p}")
    bounds = BOUNDS["drop_qknorm" if qknorm else "drop_spread"]
    o16, lse = run_fwd_bwd(L, c, chk, bounds)
    d, gp = c.bwd_fused(L, o16, lse)
    c.check_fused(chk, d, gp, bounds)
    d2, gp2 = c.bwd_fused(L, o16, lse)
    chk.true("fused dropout backward repeats bit for bit", same_bits(d, d2) and same_bits(gp, gp2))
    chk.done()


@pytest.mark.parametrize("p", [None, 0.5])
def test_attn_fwd_f32_fully_masked(L, p):
    """Precise mode's fp32 attention (vbx_attn_fwd_f32 / _dropout) with batch row 0 fully masked, at the reference's temperature."""
    import philox_ref as PR
    B, H, Np = 2, 2, 1040
    g = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(B, H, Np, 64, generator=g), dim=-1) * 8
    k = torch.nn.functional.normalize(torch.randn(B, H, Np, 64, generator=g), dim=-1) * 8
    v = torch.randn(B, H, Np, 64, generator=g)
    mask = make_mask("empty", B, Np)
    drop = None
    I = H * 64
    o32, o16, ob = nans((B * Np + 1, I), torch.float32), nans((B * Np + 1, I), torch.float16), nans((B * Np + 1, I), torch.bfloat16)
    lse = nans((B * H * Np + 1,), torch.float32)
    args = (q.to(dev), k.to(dev), v.to(dev), mask.to(dev), o32, o16, ob, lse, B, H, Np, 10.0)
    if p is None:
        L.call("vbx_attn_fwd_f32", *args, st())
    else:
        W = L.lib().vbx_dropout_bits_words(Np)
        rm, cm = (torch.zeros(B * H, Np, W, dtype=torch.int32, device=dev) for _ in range(2))
        L.call("vbx_attn_dropout_bits", rm, cm, B * H, Np, 99, 2, p, st())
        L.call("vbx_attn_fwd_f32_dropout", *args, rm, p, st())
        torch.cuda.synchronize()
        drop = torch.from_numpy(PR.unpack_bits(rm.cpu().numpy(), Np)).view(B, H, Np, Np).double() * L.lib().vbx_dropout_keep_scale(p)
    torch.cuda.synchronize()
    ref = restate.attend(q.double(), k.double(), v.double(), mask=mask, scale=10.0, drop=drop)
    sim = (torch.einsum("bhid,bhjd->bhij", q.double(), k.double()) * 10.0).masked_fill(~mask[:, None, None, :], -math.inf)
    ref_lse = torch.logsumexp(sim, dim=-1) / math.log(2.0)
    ref_lse[0] = math.log2(Np)
    bd = BOUNDS["f32"]
    chk = Checks(f"f32 p={p}")
    n = B * Np
    chk.true("guard rows untouched", all_nan(o32[n]) and all_nan(o16[n]) and all_nan(ob[n]) and all_nan(lse[B * H * Np:]))
    for name, t in (("out32", o32), ("out16", o16), ("out_bf16", ob)):
        got = heads(t[:n], B, Np, H)
        chk.le(name, rel_err(got, ref), bd[name])
        chk.tiles(name, got, ref, bd[name + "_tile"])
    lg = lse[:B * H * Np].view(B, H, Np)
    chk.le("lse max abs", max_err(lg, ref_lse), bd["lse"])
    chk.tiles("lse", lg, ref_lse, bd["lse_tile"], axis=-1)
    chk.done()


# ----------------------------------------------------------------------------- (d) module level
def test_attend_module_fully_masked_batch(L):
    """model.Attend through _AttendFn (dv at dv_ld = H * 64, the layout the op tests do not use) with one fully masked batch row,
    forward and backward against restate.attend in fp64 at the module's default scale 64^-0.5."""
    from voicebox_pytorch_amd.model import Attend
    B, H, Np = 2, 3, 200
    g = torch.Generator().manual_seed(21)
    q, k, v = (torch.randn(B, H, Np, 64, generator=g) for _ in range(3))
    mask = make_mask("empty", B, Np)
    mask[1, 150:] = False
    scale = 64 ** -0.5
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    out = Attend()(qd, kd, vd, mask=mask.to(dev))
    dout = torch.randn(B, H, Np, 64, generator=g) * 1e-3
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    c = L.lib().vbx_attn_q_prescale(scale)
    q_eff = (q * c).half().double() / c
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q_eff, k.half(), v.half()))
    ref = restate.attend(qr, kr, vr, mask=mask, scale=scale)
    ref.backward(dout.bfloat16().double())
    bd = BOUNDS["module"]
    chk = Checks("model.Attend")
    chk.le("out", rel_err(out, ref), bd["out16"])
    chk.tiles("out", out, ref, bd["out16_tile"])
    for name, got, want in (("dq", qd.grad, qr.grad), ("dk", kd.grad, kr.grad), ("dv", vd.grad, vr.grad)):
        chk.le(name, rel_err(got, want), bd[name])
        chk.tiles(name, got, want, bd[name + "_tile"])
    chk.done()
