"""Cases, fp64 references, fp32 stand-ins and per-element bounds of the row-kernel edge tests (tests/test_rows_check_cpu.py checks the
checks on the CPU, tests/test_rows_edges_gpu.py launches every case).  torch on the CPU only: nothing here touches the library or a
device.

The kernels: csrc/norm.hip (RMSNorm forward and backward, generic and lean, and the two reduce entry points over their partial
records), csrc/gateloop.hip (the chunked scan, forward and backward, and the post-LayerNorm) and the conv positional embedding of
csrc/ops.hip (forward fast and libm, backward, the weight-gradient finalize).  Every input is built here, seeded, and rounded once to
the type the kernel reads; every element of every output is compared with fp64, partial records one by one against the fp64 sum over
the record's own rows; every output buffer starts as a NaN sentinel with a guard row behind it, every operand row a launch must not
read is NaN.

The bounds are counted, not tuned.  For an output element: the fp32 roundings on its path in the kernel (u = 2^-24 each: a product, an
addition, sqrtf and the division are correctly rounded as the library is built without fast-math flags; rsqrtf counts one ulp = 2 u),
propagated to first order through the fp64 formula with absolute values, times MARGIN = 2 for a summation order that differs from the
one counted (as optim_check.py).  Beside the counted part stand, each as its own term without margin:
 * the Abramowitz-Stegun erf of the fast GELU: 6e-7 on erf, the figure csrc/common.hpp states for erf_as (fast conv entry only);
 * the scan's sigmoid 1 / (1 + __expf(-x)): no figure exists for the fast exponential, so the relative error of `a` was measured
   through the kernel itself at Np = 2 (kv_0 = 1, kv_1 = 0 makes h_1 = a_1) over the logits SWEEP against the fp64 sigmoid:
   SIGMOID_REL_MEASURED; the term is twice that (RHO_A), and every case's logits lie inside the sweep;
 * half an ulp of the stored format for bf16 / fp16 outputs, taken at the largest magnitude the fp32 value may have (|ref| + bound):
   2^(e - 8) for bf16, 2^(e - 11) for fp16 with e = floor(log2 |.|).
(The lean norm kernels use sqrtf and a division like the generic ones, not the v_rsq + Newton sequence of the gemm5 epilogue: no term.)
"""
import json
import math
import os
from dataclasses import astuple, dataclass
from functools import lru_cache

import torch
import torch.nn.functional as Fn

from attn_check import Checks, worst_tile
from optim_check import _gen, bits, ratios, sentinel
from oracle import restate

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
U = 2.0 ** -24
MARGIN = 2
ERF_AS = 6e-7  # csrc/common.hpp, erf_as: "<= 6e-7 in fp32 arithmetic"
SWEEP = (-6.0, 8.0)  # logits of the sigmoid sweep (test_rows_edges_gpu.py::test_sigmoid_sweep), step 1 / 256
SIGMOID_REL_MEASURED = 4.481e-07  # 7.5 u at x = -5.55: largest |a - sigmoid(x)| / sigmoid(x) over the sweep on MI355X (profiles/rows_edges_measured.json)
RHO_A = 2 * SIGMOID_REL_MEASURED
N_RSQ = 2  # rsqrtf: one ulp
N_REC = 9  # additions behind one element of a partial record of the norm backward kernels: 2 rows per wave, 8 waves (7)
N_ERF = 4  # erf's argument x / sqrt(2) (the constant, the product) and erf's own arithmetic beside the A-S term, in u
EPS_LN = float(torch.tensor(1e-5, dtype=F32))
SQRT1_2, INV_SQRT_2PI = 0.7071067811865476, 0.3989422804014327


def cdiv(a, b):
    return -(-a // b)


def k_lane(D):
    """additions behind one wave sum over a row of D floats: 4 per float4 chunk of a lane, six levels of the wave tree"""
    return 4 * cdiv(D // 4, 64) + 6


_PREC = {BF16: (8, -126), F16: (11, -14)}


def half_ulp(mag, dtype):
    p, emin = _PREC[dtype]
    _, e = torch.frexp(mag.double().clamp(min=2.0 ** emin))  # mag = m 2^e, m in [0.5, 1): floor(log2) = e - 1
    return torch.ldexp(torch.ones_like(mag, dtype=F64), e - 1 - p)


class RowChecks(Checks):
    """attn_check.Checks with the log of these tests: ROWS_CHECK_LOG=<file> appends one JSON line per case with every measured value
    (how profiles/rows_edges_measured.json was made)."""

    def ratio(self, cls, name, got, ref, counted, approx=0.0, fmt=None):
        ref = ref.double()
        b = (MARGIN * torch.as_tensor(counted, dtype=F64) + torch.as_tensor(approx, dtype=F64)).expand_as(ref)
        if fmt in _PREC:
            b = b + half_ulp(ref.abs() + b, fmt)
        w, idx = worst_tile(ratios(got.reshape(ref.shape), ref, b))
        self.le(f"{name} [{cls}] error / bound at {idx}", w, 1.0)

    def same_bits(self, name, got, want):
        self.true(name, got.shape == want.shape and bool((bits(got) == bits(want)).all()))

    def sentinel_kept(self, name, t):
        self.true(f"{name} keeps its sentinel", bool((bits(t) == bits(sentinel(t.numel(), t.dtype)).reshape(t.shape)).all()))

    def done(self):
        if os.environ.get("ROWS_CHECK_LOG"):
            with open(os.environ["ROWS_CHECK_LOG"], "a") as f:
                f.write(json.dumps({"case": self.case, "values": [(n, v if isinstance(v, bool) else float(v), b) for n, v, b in self.seen]}) + "\n")
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)


def rows_buf(rows, D, dtype):
    """[rows + 1, D] of sentinels: `rows` output rows and the guard row behind them"""
    return sentinel((rows + 1) * D, dtype).view(rows + 1, D)


def nan_guard(x, D):
    """x [..., D] flat as rows with one NaN row behind"""
    x = x.reshape(-1, D)
    return torch.cat([x, torch.full((1, D), math.nan, dtype=x.dtype)])


# ================================================================================================ A. RMSNorm forward
RMS_FWD_D = (4, 252, 260, 508, 512, 516, 1024, 1028, 1668, 2044, 2048)
ROW_RANGES = ((1, 1, 0, 1), (3, 5, 0, 5), (2, 9, 2, 4), (3, 7, 3, 3))  # (B, Np, n0, rpb)


@dataclass(frozen=True)
class RmsFwdCase:
    D: int
    B: int
    Np: int
    n0: int
    rpb: int
    adaptive: bool  # gb_stride = D with a beta; else one shared gamma (gb_stride = 0) and beta = NULL
    zero: bool = False  # one all-zero row

    @property
    def name(self):
        return f"rmsfwd-D{self.D}-B{self.B}-Np{self.Np}-n{self.n0}-r{self.rpb}-{'ada' if self.adaptive else 'shared'}{'-zero' if self.zero else ''}"


RMS_FWD_CASES = [RmsFwdCase(D, *rr, ad) for D in RMS_FWD_D for rr in ROW_RANGES for ad in (True, False)]
RMS_FWD_CASES += [RmsFwdCase(8, 1, 16389, 0, 16389, True),  # more rows than the 4096-block cap serves in one pass
                  RmsFwdCase(512, 3, 7, 3, 3, True, zero=True), RmsFwdCase(260, 2, 9, 2, 4, False, zero=True)]


def _live_rows(x, n0, rpb):
    live = torch.zeros(x.shape[1], dtype=torch.bool)
    live[n0: n0 + rpb] = True
    x[:, ~live] = math.nan
    return x


@lru_cache(maxsize=2)
def rms_fwd_inputs(c):
    g = _gen(("rmsfwd",) + astuple(c))
    nb = c.B if c.adaptive else 1
    x = _live_rows(torch.randn(c.B, c.Np, c.D, generator=g), c.n0, c.rpb)
    gamma = 1 + 0.3 * torch.randn(nb, c.D, generator=g)
    beta = 0.3 * torch.randn(nb, c.D, generator=g) if c.adaptive else None
    if c.zero:
        x[c.B - 1, c.n0 + c.rpb // 2] = 0
    return x, gamma, beta


def rms_fwd_reference(c, x, gamma, beta):
    """(ref, counted) [B rpb, D]: y = x / max(|x|, 1e-12) sqrt(D) gamma[b] (+ beta[b])"""
    xs, g = x[:, c.n0: c.n0 + c.rpb].double(), gamma.double()[:, None, :]
    t = restate.l2norm_scale(xs, c.D) * g
    ref = t + (beta.double()[:, None, :] if beta is not None else 0.0)
    # r = sqrtf(D) / max(sqrtf(ss), 1e-12): ss takes a product and k_lane additions per term (halved by the root), then sqrtf,
    # sqrtf(D) and the division; x * r * g: two products; + beta: one addition
    rel_r = (1 + k_lane(c.D)) / 2 + 3
    counted = U * (t.abs() * (rel_r + 2) + ref.abs())
    return ref.reshape(-1, c.D), counted.reshape(-1, c.D)


RMS_FWD_OUT = {"bf16": BF16, "f16": F16, "f32": F32}


def new_rms_fwd_out(c):
    return {k: rows_buf(c.B * c.rpb, c.D, dt) for k, dt in RMS_FWD_OUT.items()}


def standin_rms_fwd(c, fault=None):
    x, gamma, beta = rms_fwd_inputs(c)
    n0 = 0 if fault == "n0" else c.n0
    Dk = c.D - 4 if fault == "float4" else c.D
    xs = x[:, n0: n0 + c.rpb, :Dk]
    g, bt = (gamma[:1], beta[:1] if beta is not None else None) if fault == "gamma0" else (gamma, beta)
    ss = (xs * xs).sum(-1, keepdim=True)
    r = torch.sqrt(torch.tensor(float(c.D))) / torch.sqrt(ss).clamp(min=1e-12)
    o = xs * r * g[:, None, :Dk]
    if bt is not None and fault != "beta":
        o = o + bt[:, None, :Dk]
    out = new_rms_fwd_out(c)
    for k, dt in RMS_FWD_OUT.items():
        out[k][: c.B * c.rpb, :Dk] = o.reshape(-1, Dk).to(dt)
    return out


def check_rms_fwd(c, got):
    x, gamma, beta = rms_fwd_inputs(c)
    ref, counted = rms_fwd_reference(c, x, gamma, beta)
    rows = c.B * c.rpb
    ck = RowChecks(c.name)
    for k, dt in RMS_FWD_OUT.items():
        ck.ratio("rms_fwd_" + k, "y " + k, got[k][:rows], ref, counted, fmt=dt)
        ck.sentinel_kept(f"y {k} guard row", got[k][rows:])
        if c.zero:  # the zero row gives beta, or 0, exactly
            b, j = c.B - 1, c.rpb // 2
            want = (beta[b] if beta is not None else torch.zeros(c.D)).to(dt)
            ck.same_bits(f"y {k} of the zero row is beta", got[k][b * c.rpb + j], want)
    ck.done()


# ================================================================================================ B. RMSNorm backward
RMS_BWD_D = (4, 260, 512, 516, 1024, 1028, 1668, 2048)
RMS_BWD_RPB = (1, 7, 8, 9, 15, 16, 17, 33)
PTRS = ("all", "no_dx_in", "no_dxb", "no_colpart")  # colpart goes only with dx_in: "no_dx_in" drops both


@dataclass(frozen=True)
class RmsBwdCase:
    D: int
    B: int
    Np: int
    n0: int
    rpb: int
    adaptive: bool
    ptrs: str
    zero: bool = False

    @property
    def name(self):
        return (f"rmsbwd-D{self.D}-B{self.B}-Np{self.Np}-n{self.n0}-r{self.rpb}-{'ada' if self.adaptive else 'shared'}-{self.ptrs}"
                f"{'-zero' if self.zero else ''}")

    @property
    def chunks(self):
        return cdiv(self.rpb, 16)


def _rms_bwd_table():
    out = []
    for i, D in enumerate(RMS_BWD_D):
        for j, rpb in enumerate(RMS_BWD_RPB):  # every width meets every pointer combination, both n0, both B and both gamma forms
            n0 = (0, 3)[(i + j // 4) % 2] if j != 7 else 3
            out.append(RmsBwdCase(D, (1, 3)[(i + j) % 2], n0 + rpb + 2, n0, rpb, (i + j // 2) % 2 == 0, PTRS[(i + j) % 4]))
    out.append(RmsBwdCase(512, 3, 14, 3, 9, True, "all", zero=True))
    out.append(RmsBwdCase(260, 1, 19, 0, 17, False, "all", zero=True))
    return out


RMS_BWD_CASES = _rms_bwd_table()


@lru_cache(maxsize=2)
def rms_bwd_inputs(c):
    g = _gen(("rmsbwd",) + astuple(c))
    nb = c.B if c.adaptive else 1
    x = _live_rows(torch.randn(c.B, c.Np, c.D, generator=g), c.n0, c.rpb)
    gamma = 1 + 0.3 * torch.randn(nb, c.D, generator=g)
    dy = torch.randn(c.B, c.rpb, c.D, generator=g).to(BF16)
    dx_in = _live_rows(torch.randn(c.B, c.Np, c.D, generator=g), c.n0, c.rpb)
    if c.zero:
        b, j = c.B - 1, c.rpb // 2
        x[b, c.n0 + j] = 0
        dy[b, j] = 0
    return dict(x=x, gamma=gamma, dy=dy, dx_in=dx_in if c.ptrs != "no_dx_in" else None)


def _chunk_sums(t, rpb):
    """[B, rpb, D] -> [B, chunks, D]: the sum over each record's own rows (up to 16)"""
    B, _, D = t.shape
    ch = cdiv(rpb, 16)
    return Fn.pad(t, (0, 0, 0, ch * 16 - rpb)).reshape(B, ch, 16, D).sum(2)


def rms_bwd_reference(c, inp):
    """u = x / |x|; du = sqrt(D) gamma dy; dx = (du - u (u . du)) / |x| (+ dx_in); records sum sqrt(D) u dy | sum dy | sum dx_in"""
    xs, g, dy = inp["x"][:, c.n0: c.n0 + c.rpb].double(), inp["gamma"].double()[:, None, :], inp["dy"].double()
    sq, kl = math.sqrt(c.D), k_lane(c.D)
    nrm = (xs * xs).sum(-1, keepdim=True).sqrt().clamp(min=1e-12)
    inv = 1.0 / nrm
    rel_inv = (1 + kl) / 2 + 2  # ss as in the forward, sqrtf, the division
    u, rel_u = xs * inv, rel_inv + 1
    du, rel_du = dy * sq * g, 3  # sqrtf(D), sqrtD * g, * dy
    dot = (u * du).sum(-1, keepdim=True)
    d_dot = U * (rel_u + rel_du + 1 + kl) * (u * du).abs().sum(-1, keepdim=True)
    inner = du - u * dot
    o = inner * inv
    c_o = U * inv * (du.abs() * rel_du + (u * dot).abs() * (rel_u + 1) + inner.abs()) + inv * u.abs() * d_dot + U * o.abs() * (rel_inv + 1)
    if inp["dx_in"] is not None:
        a = inp["dx_in"][:, c.n0: c.n0 + c.rpb].double()
        o = o + a
        c_o = c_o + U * o.abs()
    tg = sq * u * dy  # sqrtf(D), two products, u's own error; N_REC additions behind a record
    rec = {"part0": (_chunk_sums(tg, c.rpb), U * (rel_u + 3 + N_REC) * _chunk_sums(tg.abs(), c.rpb)),
           "part1": (_chunk_sums(dy, c.rpb), U * N_REC * _chunk_sums(dy.abs(), c.rpb))}
    if c.ptrs == "all" or c.ptrs == "no_dxb":
        rec["cpart"] = (_chunk_sums(a, c.rpb), U * N_REC * _chunk_sums(a.abs(), c.rpb))
    return o, c_o, rec


def new_rms_bwd_out(c):
    out = dict(dx_out=rows_buf(c.B * c.Np, c.D, F32), part=rows_buf(c.B * c.chunks * 2, c.D, F32))
    if c.ptrs != "no_dxb":
        out["dxb"] = rows_buf(c.B * c.Np, c.D, BF16)
    if c.ptrs in ("all", "no_dxb"):
        out["cpart"] = rows_buf(c.B * c.chunks, c.D, F32)
    return out


def standin_rms_bwd(c, fault=None):
    inp = rms_bwd_inputs(c)
    n0 = 0 if fault == "n0" else c.n0
    Dk = c.D - 4 if fault == "float4" else c.D
    xs, dy = inp["x"][:, n0: n0 + c.rpb, :Dk], inp["dy"].float()[..., :Dk]
    g = (inp["gamma"][:1] if fault == "gamma0" else inp["gamma"])[:, None, :Dk]
    sq = torch.sqrt(torch.tensor(float(c.D)))
    inv = 1.0 / torch.sqrt((xs * xs).sum(-1, keepdim=True)).clamp(min=1e-12)
    u = xs * inv
    tg = sq * u * dy
    du = dy * (sq * g)
    dot = (u * du).sum(-1, keepdim=True)
    o = (du - u * dot) * inv
    a = inp["dx_in"][:, n0: n0 + c.rpb, :Dk] if inp["dx_in"] is not None else None
    if a is not None:
        o = o + a
    out = new_rms_bwd_out(c)
    live = (torch.arange(c.B)[:, None] * c.Np + c.n0 + torch.arange(c.rpb)[None]).reshape(-1)
    out["dx_out"][live, :Dk] = o.reshape(-1, Dk)
    if "dxb" in out:
        out["dxb"][live, :Dk] = o.reshape(-1, Dk).to(BF16)
    recs = [_chunk_sums(tg, c.rpb), _chunk_sums(dy, c.rpb)]
    if fault == "rowpast":  # the last record also takes the row behind the range (and the dy row that follows in memory)
        nxt = nan_guard(inp["dy"].float(), c.D).reshape(-1, c.D)
        for b in range(c.B):
            xr = inp["x"][b, c.n0 + c.rpb]
            dr = nxt[b * c.rpb + c.rpb]
            recs[0][b, -1] += sq * xr * dr
            recs[1][b, -1] += dr
    out["part"][: c.B * c.chunks * 2, :Dk] = torch.stack(recs, 2).reshape(-1, Dk)
    if "cpart" in out:
        out["cpart"][: c.B * c.chunks, :Dk] = _chunk_sums(a, c.rpb).reshape(-1, Dk)
    return out


def check_rms_bwd(c, got):
    inp = rms_bwd_inputs(c)
    ref, c_o, rec = rms_bwd_reference(c, inp)
    ck = RowChecks(c.name)
    live = torch.zeros(c.B * c.Np + 1, dtype=torch.bool)
    live[(torch.arange(c.B)[:, None] * c.Np + c.n0 + torch.arange(c.rpb)[None]).reshape(-1)] = True
    ck.ratio("rms_bwd_dx", "dx_out", got["dx_out"][live], ref.reshape(-1, c.D), c_o.reshape(-1, c.D))
    ck.sentinel_kept("dx_out outside the row range", got["dx_out"][~live])
    if "dxb" in got:
        ck.ratio("rms_bwd_dxb", "dxb", got["dxb"][live], ref.reshape(-1, c.D), c_o.reshape(-1, c.D), fmt=BF16)
        ck.sentinel_kept("dxb outside the row range", got["dxb"][~live])
        ck.same_bits("dxb is round-to-nearest-even of the stored dx_out", got["dxb"][live], got["dx_out"][live].to(BF16))
    n = c.B * c.chunks
    part = got["part"][: 2 * n].reshape(c.B, c.chunks, 2, c.D)
    ck.ratio("rms_bwd_part", "part[..][0] (gamma)", part[:, :, 0], *rec["part0"])
    ck.ratio("rms_bwd_part", "part[..][1] (beta)", part[:, :, 1], *rec["part1"])
    ck.sentinel_kept("part guard row", got["part"][2 * n:])
    if "cpart" in rec:
        ck.ratio("rms_bwd_cpart", "cpart", got["cpart"][:n].reshape(c.B, c.chunks, c.D), *rec["cpart"])
        ck.sentinel_kept("cpart guard row", got["cpart"][n:])
    if c.zero and inp["dx_in"] is not None:  # x = 0 and dy = 0 on a row: dx is dx_in
        r = (c.B - 1) * c.Np + c.n0 + c.rpb // 2
        ck.same_bits("dx_out of the zero row is dx_in", got["dx_out"][r], inp["dx_in"].reshape(-1, c.D)[r])
    ck.done()


# ================================================================================================ C. the two reduce entry points
@dataclass(frozen=True)
class ReduceCase:
    kind: str  # "norm": vbx_reduce_norm_partials over [B][chunks][2 D]; "col": vbx_reduce_col_partials over [B][chunks][D]
    B: int
    chunks: int
    D: int
    sum_batch: int
    pad: int = 0  # out_b_stride = 2 D + pad

    @property
    def name(self):
        return f"reduce-{self.kind}-B{self.B}-c{self.chunks}-D{self.D}-sb{self.sum_batch}-pad{self.pad}"

    @property
    def W(self):
        return 2 * self.D if self.kind == "norm" else self.D


REDUCE_CASES = [ReduceCase("norm", 3, ch, 36, sb) for ch in (1, 2, 65) for sb in (0, 1)]  # W = 72: a ragged last block of 64
REDUCE_CASES += [ReduceCase("norm", 3, 2, 36, 0, pad=8), ReduceCase("norm", 1, 65, 128, 1)]
REDUCE_CASES += [ReduceCase("col", B, ch, 36, 1) for B, ch in ((3, 1), (3, 2), (3, 65), (1, 65))]


@lru_cache(maxsize=2)
def reduce_input(c):
    return nan_guard(torch.randn(c.B, c.chunks, c.W, generator=_gen(("reduce",) + astuple(c))), c.W)


def new_reduce_out(c):
    if c.kind == "col":
        return dict(out=rows_buf(1, c.D, F32), tmp=rows_buf(c.B, c.D, F32))
    return dict(out=rows_buf(1 if c.sum_batch else c.B, c.W + c.pad, F32))


def standin_reduce(c):
    p = reduce_input(c)[:-1].reshape(c.B, c.chunks, c.W)
    out = new_reduce_out(c)
    if c.kind == "col":
        out["tmp"][: c.B] = p.sum(1)
        out["out"][0] = out["tmp"][: c.B].sum(0)
    elif c.sum_batch:
        out["out"][0] = p.sum((0, 1))
    else:
        out["out"][: c.B, : c.W] = p.sum(1)
    return out


def check_reduce(c, got):
    p = reduce_input(c)[:-1].reshape(c.B, c.chunks, c.W).double()
    ck = RowChecks(c.name)

    def k(n):  # four lanes share the n records, three additions join them
        return cdiv(n, 4) + 3

    if c.kind == "col":
        ck.ratio("reduce_col", "out", got["out"][0], p.sum((0, 1)), U * (k(c.chunks) + k(c.B)) * p.abs().sum((0, 1)))
        ck.ratio("reduce_col", "tmp", got["tmp"][: c.B], p.sum(1), U * k(c.chunks) * p.abs().sum(1))
        ck.sentinel_kept("tmp guard row", got["tmp"][c.B:])
        ck.sentinel_kept("out guard row", got["out"][1:])
    elif c.sum_batch:
        ck.ratio("reduce_norm", "out", got["out"][0, : c.W], p.sum((0, 1)), U * k(c.B * c.chunks) * p.abs().sum((0, 1)))
        ck.sentinel_kept("out guard row", got["out"][1:])
    else:
        ck.ratio("reduce_norm", "out", got["out"][: c.B, : c.W], p.sum(1), U * k(c.chunks) * p.abs().sum(1))
        ck.sentinel_kept("out between 2 D and the batch stride, and the guard row", torch.cat([got["out"][: c.B, c.W:].reshape(-1), got["out"][c.B]]))
    ck.done()


# ================================================================================================ D. LayerNorm
LN_NP = (1, 8, 9, 16, 17)


@dataclass(frozen=True)
class LnCase:
    D: int
    B: int
    Np: int
    resid: bool
    const: bool = False  # one constant row: variance 0, rstd = eps^-1/2
    fwd_only: bool = False

    @property
    def name(self):
        return f"ln-D{self.D}-B{self.B}-Np{self.Np}-{'resid' if self.resid else 'noresid'}{'-const' if self.const else ''}"

    @property
    def chunks(self):
        return cdiv(self.Np, 16)


LN_CASES = [LnCase(D, (1, 2)[(i + j) % 2], Np, (i + j) % 2 == 0) for i, D in enumerate(RMS_BWD_D) for j, Np in enumerate(LN_NP)]
LN_CASES += [LnCase(8, 1, 16389, True, fwd_only=True), LnCase(516, 2, 9, False, const=True), LnCase(512, 1, 17, True, const=True)]


@lru_cache(maxsize=2)
def ln_inputs(c):
    g = _gen(("ln",) + astuple(c))
    s = torch.randn(c.B, c.Np, c.D, generator=g) * 2 + 0.3
    w, b = 1 + 0.1 * torch.randn(c.D, generator=g), 0.1 * torch.randn(c.D, generator=g)
    resid = torch.randn(c.B, c.Np, c.D, generator=g) if c.resid else None
    dy = torch.randn(c.B, c.Np, c.D, generator=g)
    if c.const:
        s[c.B - 1, c.Np // 2] = 1.5
    return dict(s=s, w=w, b=b, resid=resid, dy=dy)


def _ln_stats(s, D):
    """mean, v = s - mean, rstd in fp64 with the bounds of their fp32 values (second order kept in the variance: on a constant row
    v is pure rounding error)"""
    kl = k_lane(D)
    mean = s.sum(-1, keepdim=True) / D
    d_mean = U * (kl + 2) * s.abs().sum(-1, keepdim=True) / D  # the wave sum, 1 / D, the product
    v = s - mean
    d_v = U * v.abs() + d_mean
    sv = (v * v).sum(-1, keepdim=True)
    d_var = ((2 * v.abs() * d_v + d_v * d_v).sum(-1, keepdim=True) + U * (1 + kl + 2) * sv) / D
    q = sv / D + EPS_LN
    rstd = q.rsqrt()
    d_rstd = rstd * ((1 + N_RSQ) * U + d_var / (2 * q))  # + eps, rsqrtf
    return v, d_v, rstd, d_rstd


def ln_fwd_reference(c, inp):
    s, w, b = inp["s"].double(), inp["w"].double(), inp["b"].double()
    v, d_v, rstd, d_rstd = _ln_stats(s, c.D)
    y = v * rstd * w + b
    ref = Fn.layer_norm(s, (c.D,), w, b, eps=EPS_LN)
    assert float((ref - y).abs().max()) < 1e-11
    counted = w.abs() * (d_v * rstd + v.abs() * d_rstd) + U * (2 * (v * rstd * w).abs() + ref.abs())
    if inp["resid"] is not None:
        ref = ref + inp["resid"].double()
        counted = counted + U * ref.abs()
    return ref.reshape(-1, c.D), counted.reshape(-1, c.D)


def ln_bwd_reference(c, inp):
    """xh = (s - mean) rstd; dw += dy xh; db += dy; dxh = dy w; ds = rstd (dxh - mean(dxh) - xh mean(dxh xh))"""
    s, w, dy = inp["s"].double(), inp["w"].double(), inp["dy"].double()
    kl = k_lane(c.D)
    v, d_v, rstd, d_rstd = _ln_stats(s, c.D)
    xh = v * rstd
    d_xh = d_v * rstd + v.abs() * d_rstd + U * xh.abs()
    rec = {"dw": (_chunk_sums(dy * xh, c.Np), _chunk_sums(dy.abs() * d_xh + U * (1 + N_REC) * (dy * xh).abs(), c.Np)),
           "db": (_chunk_sums(dy, c.Np), U * N_REC * _chunk_sums(dy.abs(), c.Np))}
    dxh = dy * w
    d_dxh = U * dxh.abs()
    m1 = dxh.sum(-1, keepdim=True) / c.D
    d_m1 = (d_dxh.sum(-1, keepdim=True) + U * (kl + 2) * dxh.abs().sum(-1, keepdim=True)) / c.D
    m2 = (dxh * xh).sum(-1, keepdim=True) / c.D
    d_m2 = ((d_dxh * xh.abs() + dxh.abs() * d_xh).sum(-1, keepdim=True) + U * (1 + kl + 2) * (dxh * xh).abs().sum(-1, keepdim=True)) / c.D
    inner = dxh - m1 - xh * m2
    d_inner = (d_dxh + d_m1 + xh.abs() * d_m2 + m2.abs() * d_xh + U * (xh * m2).abs() + 2 * U * (dxh.abs() + m1.abs() + (xh * m2).abs()))
    ds = rstd * inner
    return ds.reshape(-1, c.D), (rstd * d_inner + inner.abs() * d_rstd + U * ds.abs()).reshape(-1, c.D), rec


def new_ln_out(c):
    out = dict(y=rows_buf(c.B * c.Np, c.D, F32))
    if not c.fwd_only:
        out.update(ds=rows_buf(c.B * c.Np, c.D, F32), part=rows_buf(c.B * c.chunks * 2, c.D, F32))
    return out


def standin_ln(c, fault=None):
    inp = ln_inputs(c)
    s, w, b, dy = inp["s"], inp["w"], inp["b"], inp["dy"]
    invD = torch.tensor(1.0) / torch.tensor(float(c.D))
    mean = s.sum(-1, keepdim=True) * invD
    v = s - mean
    var = (v * v).sum(-1, keepdim=True) * (torch.tensor(1.0) / torch.tensor(float(c.D - 1)) if fault == "dm1" else invD)
    rstd = torch.rsqrt(var + torch.tensor(EPS_LN))
    y = v * rstd * w + b
    if inp["resid"] is not None:
        y = y + inp["resid"]
    out = new_ln_out(c)
    rows = c.B * c.Np
    out["y"][:rows] = y.reshape(-1, c.D)
    if c.fwd_only:
        return out
    xh = v * rstd
    dxh = dy * w
    m1 = dxh.sum(-1, keepdim=True) * invD
    m2 = (dxh * xh).sum(-1, keepdim=True) * invD
    out["ds"][:rows] = (rstd * (dxh - m1 - xh * m2)).reshape(-1, c.D)
    out["part"][: c.B * c.chunks * 2] = torch.stack([_chunk_sums(dy * xh, c.Np), _chunk_sums(dy, c.Np)], 2).reshape(-1, c.D)
    return out


def check_ln(c, got):
    inp = ln_inputs(c)
    rows = c.B * c.Np
    ck = RowChecks(c.name)
    ck.ratio("ln_fwd", "y", got["y"][:rows], *ln_fwd_reference(c, inp))
    ck.sentinel_kept("y guard row", got["y"][rows:])
    if c.const:
        r = (c.B - 1) * c.Np + c.Np // 2
        ck.true("the constant row has variance 0", float(inp["s"][c.B - 1, c.Np // 2].double().var(unbiased=False)) == 0.0)
        ck.true("y of the constant row is finite", bool(torch.isfinite(got["y"][r]).all()))
    if not c.fwd_only:
        ds, c_ds, rec = ln_bwd_reference(c, inp)
        ck.ratio("ln_bwd_ds", "ds", got["ds"][:rows], ds, c_ds)
        ck.sentinel_kept("ds guard row", got["ds"][rows:])
        n = c.B * c.chunks
        part = got["part"][: 2 * n].reshape(c.B, c.chunks, 2, c.D)
        ck.ratio("ln_bwd_part", "part[..][0] (dw)", part[:, :, 0], *rec["dw"])
        ck.ratio("ln_bwd_part", "part[..][1] (db)", part[:, :, 1], *rec["db"])
        ck.sentinel_kept("part guard row", got["part"][2 * n:])
    ck.done()


# ================================================================================================ E. the GateLoop scan
GL_CHUNKS = 32
SCAN_SHAPES = ((1, 1, 1), (2, 2, 33), (1, 31, 31), (2, 32, 32), (1, 33, 33), (2, 63, 1), (1, 64, 96), (2, 65, 31), (1, 1023, 33),
               (2, 1024, 32), (1, 1025, 96), (2, 1025, 1), (1, 33, 96), (1, 1024, 31))  # (B, Np, D)


@dataclass(frozen=True)
class ScanCase:
    B: int
    Np: int
    D: int
    gates: str  # "normal": logits from N(0, 1); "long": uniform in [3, 7], a in (0.95, 0.999): the carry crosses many chunks

    @property
    def name(self):
        return f"scan-B{self.B}-Np{self.Np}-D{self.D}-{self.gates}"

    @property
    def T(self):
        return cdiv(self.Np, GL_CHUNKS)


SCAN_CASES = [ScanCase(*sh, g) for sh in SCAN_SHAPES for g in ("normal", "long")]


def _scan_fwd_ref(c, qkva):
    """h_t = a_t h_{t-1} + kv_t, s_t = q_t h_t in fp64.  Bound of h: every term (prod a) kv_j of h_t meets, per frame it is carried
    over, one fmaf and one a (RHO_A), and one more fmaf where it enters a chunk through the fold over the chunk maps."""
    q, kv, lg = qkva.double().chunk(3, dim=-1)
    a = lg.sigmoid()
    h, Hh, E = (torch.zeros_like(kv[:, 0]) for _ in range(3))
    hs, Es = [], []
    for t in range(c.Np):
        carried = a[:, t] * Hh
        E = a[:, t] * E + (RHO_A + U + (U if t % c.T == 0 else 0.0)) * carried + U * kv[:, t].abs()
        h = a[:, t] * h + kv[:, t]
        Hh = carried + kv[:, t].abs()
        hs.append(h)
        Es.append(E)
    h, E = torch.stack(hs, 1), torch.stack(Es, 1)
    s = q * h
    return s, q.abs() * E + U * s.abs(), h, E


@lru_cache(maxsize=2)
def scan_inputs(c):
    g = _gen(("scan",) + astuple(c))
    qkva = torch.randn(c.B, c.Np, 3 * c.D, generator=g)
    if c.gates == "long":
        qkva[..., 2 * c.D:] = 3 + 4 * torch.rand(c.B, c.Np, c.D, generator=g)
    ds = torch.randn(c.B, c.Np, c.D, generator=g)
    ref = _scan_fwd_ref(c, qkva)
    return dict(qkva=qkva, ds=ds, hin=ref[2].float(), fwd=ref)  # hin: the state the backward reads, the fp64 h rounded once


def scan_bwd_reference(c, inp):
    """g_t = ds_t q_t + a_{t+1} g_{t+1}; dq = ds h; dkv = g; d(logit) = g h_{t-1} a (1 - a), from the given state"""
    q, _, lg = inp["qkva"].double().chunk(3, dim=-1)
    a, ds, h = lg.sigmoid(), inp["ds"].double(), inp["hin"].double()
    ut = ds * q
    G, Gh, E = (torch.zeros_like(ut[:, 0]) for _ in range(3))
    Gs, Es = [None] * c.Np, [None] * c.Np
    for t in reversed(range(c.Np)):
        an = a[:, t + 1] if t + 1 < c.Np else torch.zeros_like(G)
        carried = an * Gh
        E = an * E + (RHO_A + U + (U if (t + 1) % c.T == 0 else 0.0)) * carried + 2 * U * ut[:, t].abs()  # ds * q, the fmaf
        G = an * G + ut[:, t]
        Gh = carried + ut[:, t].abs()
        Gs[t], Es[t] = G, E
    G, E = torch.stack(Gs, 1), torch.stack(Es, 1)
    hp = torch.cat([torch.zeros_like(h[:, :1]), h[:, :-1]], 1)
    dq = ds * h
    dl = G * hp * a * (1 - a)
    c_dl = (hp * a * (1 - a)).abs() * E + (G * hp).abs() * (1 - 2 * a).abs() * RHO_A * a + 4 * U * dl.abs()  # three products, 1 - a
    return torch.cat([dq, G, dl], -1), torch.cat([U * dq.abs(), E, c_dl], -1)


def new_scan_out(c):
    return dict(s=rows_buf(c.B * c.Np, c.D, F32), s_nostate=rows_buf(c.B * c.Np, c.D, F32), h=rows_buf(c.B * c.Np, c.D, F32),
                dqkva=rows_buf(c.B * c.Np, 3 * c.D, BF16))


def fault_chunk(c):
    """the chunk whose carry-in (forward) or last frame (backward) the planted faults hit: in the middle of the live chunks"""
    return max(1, (cdiv(c.Np, c.T) - 1) // 2)


def standin_scan(c, fault=None):
    """The kernels' own order: every chunk of T = ceil(Np / 32) frames reduced to its affine map, the carries folded chunk by chunk,
    every chunk replayed from its carry."""
    inp = scan_inputs(c)
    q, kv, lg = inp["qkva"].chunk(3, dim=-1)
    a, ds, hin = torch.sigmoid(lg), inp["ds"], inp["hin"]
    T, Np, fc = c.T, c.Np, fault_chunk(c)
    zero = torch.zeros(c.B, c.D)
    s, hs, dq = torch.empty(c.B, Np, c.D), torch.empty(c.B, Np, c.D), torch.empty(c.B, Np, 3 * c.D)
    carry = zero
    for ch in range(GL_CHUNKS):
        t0, t1 = ch * T, min(Np, ch * T + T)
        P, H = torch.ones(c.B, c.D), zero
        h = zero if (fault == "seam" and ch == fc) else carry
        for t in range(t0, t1):
            H = a[:, t] * H + kv[:, t]
            P = P * a[:, t]
            h = a[:, t] * h + kv[:, t]
            s[:, t], hs[:, t] = q[:, t] * h, h
        carry = P * carry + H
    carry = zero
    for ch in reversed(range(GL_CHUNKS)):
        t0, t1 = ch * T, min(Np, ch * T + T)
        if t0 >= t1:
            continue
        an = a[:, t1] if t1 < Np else zero
        if fault == "an" and ch == fc and t1 < Np:
            an = a[:, t1 - 1]
        P, G, g = torch.ones(c.B, c.D), zero, carry
        for t in reversed(range(t0, t1)):
            ut = ds[:, t] * q[:, t]
            G = an * G + ut
            P = P * an
            g = an * g + ut
            hprev = hin[:, t - 1] if t > 0 else zero
            dq[:, t] = torch.cat([ds[:, t] * hin[:, t], g, g * hprev * a[:, t] * (1.0 - a[:, t])], -1)
            an = a[:, t]
        carry = P * carry + G
    out = new_scan_out(c)
    rows = c.B * Np
    out["s"][:rows], out["s_nostate"][:rows], out["h"][:rows] = s.reshape(rows, -1), s.reshape(rows, -1), hs.reshape(rows, -1)
    out["dqkva"][:rows] = dq.reshape(rows, -1).to(BF16)
    return out


def check_scan(c, got):
    inp = scan_inputs(c)
    s, c_s, h, c_h = (t.reshape(-1, c.D) for t in inp["fwd"])
    rows = c.B * c.Np
    ck = RowChecks(c.name)
    lg = inp["qkva"][..., 2 * c.D:]
    ck.true("the logits lie inside the sigmoid sweep", SWEEP[0] <= float(lg.min()) and float(lg.max()) <= SWEEP[1])
    ck.ratio("scan_s", "s", got["s"][:rows], s, c_s)
    ck.ratio("scan_s", "s (hstate = NULL)", got["s_nostate"][:rows], s, c_s)
    ck.ratio("scan_h", "hstate", got["h"][:rows], h, c_h)
    ck.same_bits("s is the same with and without hstate", got["s_nostate"], got["s"])
    ref, cb = (t.reshape(rows, 3 * c.D) for t in scan_bwd_reference(c, inp))
    for i, k in enumerate(("dq", "dkv", "da")):
        sl = slice(i * c.D, (i + 1) * c.D)
        ck.ratio("scan_" + k, k, got["dqkva"][:rows, sl], ref[:, sl], cb[:, sl], fmt=BF16)
    for k in ("s", "s_nostate", "h", "dqkva"):
        ck.sentinel_kept(k + " guard row", got[k][rows:])
    ck.done()


def sweep_logits():
    n = int((SWEEP[1] - SWEEP[0]) * 256) + 1
    return SWEEP[0] + torch.arange(n, dtype=F32) / 256


def sweep_qkva():
    """Np = 2, B = 1, D = the sweep: kv_0 = 1, kv_1 = 0, so that hstate[1] = fmaf(a_1, 1, 0) = a_1"""
    x = sweep_logits()
    D = x.numel()
    qkva = torch.zeros(1, 2, 3 * D)
    qkva[0, :, :D] = 1
    qkva[0, 0, D: 2 * D] = 1
    qkva[0, 1, 2 * D:] = x
    return qkva


def sigmoid_rel_error(a):
    """largest |a - sigmoid(x)| / sigmoid(x) over the sweep against the fp64 sigmoid, and the logit where it occurs"""
    x = sweep_logits().double()
    rel = (a.double() - x.sigmoid()).abs() / x.sigmoid()
    i = int(rel.argmax())
    return float(rel[i]), float(x[i])


# ================================================================================================ F. the conv positional embedding
CT = 64
CONV_N, CONV_D, CONV_KS = (1, 15, 16, 63, 64, 65, 129), (1, 40, 64, 72, 128), (1, 3, 31)
MASKS = ("none", "hole", "row", "last")


@dataclass(frozen=True)
class ConvCase:
    B: int
    N: int
    D: int
    ks: int
    R: int
    mask: str  # "hole": frames 62..65 false; "row": batch row B - 1 entirely false; "last": only the last frame true
    dreg_null: bool = False

    @property
    def name(self):
        return f"conv-B{self.B}-N{self.N}-D{self.D}-ks{self.ks}-R{self.R}-{self.mask}{'-nodreg' if self.dreg_null else ''}"

    @property
    def tiles(self):
        return cdiv(self.N, CT)


CONV_CASES = [ConvCase(*t) for t in (
    (1, 1, 1, 31, 0, "none"), (3, 15, 40, 31, 16, "last"), (1, 16, 64, 3, 0, "none"), (3, 63, 72, 31, 16, "none", True),
    (1, 64, 128, 31, 0, "none"), (3, 65, 40, 31, 16, "hole"), (3, 129, 72, 31, 16, "hole", True), (3, 129, 128, 3, 0, "row"),
    (1, 129, 1, 1, 16, "none"), (3, 65, 64, 1, 0, "hole"), (3, 64, 40, 3, 16, "row", True), (1, 15, 128, 1, 0, "last"),
    (3, 1, 72, 3, 16, "none"), (1, 63, 64, 31, 16, "last"), (3, 16, 1, 31, 0, "row"), (1, 129, 40, 31, 0, "hole"))]


def conv_mask(c):
    if c.mask == "none":
        return None
    m = torch.ones(c.B, c.N, dtype=torch.bool)
    if c.mask == "hole":
        m[:, 62:66] = False
    elif c.mask == "row":
        m[c.B - 1] = False
    else:
        m[:, : c.N - 1] = False
    return m


@lru_cache(maxsize=2)
def conv_inputs(c):
    g = _gen(("conv",) + astuple(c))
    return dict(e=torch.randn(c.B, c.N, c.D, generator=g), w=torch.randn(c.D, c.ks, generator=g) * c.ks ** -0.5,
                bias=0.1 * torch.randn(c.D, generator=g), reg=torch.randn(c.R, c.D, generator=g),
                dxs=torch.randn(c.B, c.N + c.R, c.D, generator=g), mask=conv_mask(c))


def _taps(xp, k, N):
    return xp[:, k: k + N]


def _tile_sums(t):
    """[B, N, D] -> [B tiles, D]: the sum over the frames of each 64-frame tile"""
    B, N, D = t.shape
    nt = cdiv(N, CT)
    return Fn.pad(t, (0, 0, 0, nt * CT - N)).reshape(B, nt, CT, D).sum(2).reshape(B * nt, D)


def conv_reference(c, inp):
    """Forward xs[:, R:] = e + m GELU(bias + sum_k w_k (m e)[n + k - half]) and the backward of it in fp64, with the bounds.  Returns a
    dict name -> (ref, counted, approx): approx is the A-S erf's share (fast forward, and everything behind the backward's GELU')."""
    e, w, bias, dxs = inp["e"].double(), inp["w"].double(), inp["bias"].double(), inp["dxs"].double()[:, c.R:]
    m = inp["mask"][..., None].double() if inp["mask"] is not None else torch.ones(c.B, c.N, 1, dtype=F64)
    ks, half, N = c.ks, c.ks // 2, c.N
    em = e * m
    xp = Fn.pad(em, (0, 0, half, half))
    pre, S = bias.expand(c.B, N, c.D).clone(), bias.abs().expand(c.B, N, c.D).clone()
    for k in range(ks):
        pre = pre + w[:, k] * _taps(xp, k, N)
        S = S + (w[:, k] * _taps(xp, k, N)).abs()
    d_pre = U * ks * S  # a chain of ks fused multiply-adds from the bias
    erf, phi = torch.special.erf(pre * SQRT1_2), torch.exp(-0.5 * pre * pre) * INV_SQRT_2PI
    d_erf = U * (N_ERF * 2 * (pre * phi).abs() + N_ERF * erf.abs())  # the argument's relative error through erf' = 2 phi sqrt(2), erf's own
    gelu, g1, g2 = 0.5 * pre * (1 + erf), 0.5 * (1 + erf) + pre * phi, phi * (2 - pre * pre)
    out = {}
    xs = e + m * gelu
    ref = restate.conv_pos_embed(e, w[:, None, :], bias, inp["mask"]) + e
    assert float((ref - xs).abs().max()) < 1e-11
    c_gelu = g1.abs() * d_pre + 0.5 * pre.abs() * (d_erf + U * (1 + erf).abs()) + 2 * U * gelu.abs()
    out["xs"] = (ref, m * c_gelu + U * ref.abs(), m * 0.5 * pre.abs() * ERF_AS)
    # GELU'(x) = 0.5 (1 + erf) + x phi(x), phi through __expf(-0.5 x x): two products into the argument, the product with log2(e)
    # inside and one ulp of v_exp_f32, (1.5 x^2 + 2) u relative; then the products x * c * exp and the addition
    c_g1 = g2.abs() * d_pre + 0.5 * (d_erf + U * (1 + erf).abs()) + U * (pre * phi).abs() * (1.5 * pre * pre + 2 + 3) + U * g1.abs()
    dpre = m * dxs * g1
    c_dp, a_dp = m * (dxs.abs() * c_g1 + U * dpre.abs()), m * dxs.abs() * 0.5 * ERF_AS
    dp, cp, ap = (Fn.pad(t, (0, 0, half, half)) for t in (dpre, c_dp, a_dp))
    acc, c_acc, a_acc, Sd = (torch.zeros(c.B, N, c.D, dtype=F64) for _ in range(4))
    for k in range(ks):  # dpre[n - k + half]
        sl = 2 * half - k
        acc = acc + w[:, k] * _taps(dp, sl, N)
        Sd = Sd + (w[:, k] * _taps(dp, sl, N)).abs()
        c_acc = c_acc + w[:, k].abs() * _taps(cp, sl, N)
        a_acc = a_acc + w[:, k].abs() * _taps(ap, sl, N)
    de = dxs + m * acc
    out["de"] = (de, m * (c_acc + U * ks * Sd) + U * de.abs(), m * a_acc)
    # wpart[b tiles + tile][d][k] = sum over the tile's frames of dpre[n] (m e)[n + k - half]; [63] = sum dpre: 16 additions per
    # thread, three across the four groups
    n_add = 16 + 3
    rec, c_rec, a_rec = (torch.zeros(c.B * c.tiles, c.D, 64, dtype=F64) for _ in range(3))
    for k in range(ks):
        x = _taps(xp, k, N)
        rec[..., k] = _tile_sums(dpre * x)
        c_rec[..., k] = _tile_sums(c_dp * x.abs() + U * (1 + n_add) * (dpre * x).abs())
        a_rec[..., k] = _tile_sums(a_dp * x.abs())
    rec[..., 63], c_rec[..., 63], a_rec[..., 63] = _tile_sums(dpre), _tile_sums(c_dp + U * n_add * dpre.abs()), _tile_sums(a_dp)
    out["wpart"] = (rec, c_rec, a_rec)
    dr = inp["dxs"].double()[:, : c.R]
    out["dreg"] = (dr.sum(0), U * c.B * dr.abs().sum(0), 0.0)
    return out


def new_conv_out(c):
    out = dict(xs=rows_buf(c.B * (c.N + c.R), c.D, F32), xs_libm=rows_buf(c.B * (c.N + c.R), c.D, F32), de=rows_buf(c.B * c.N, c.D, F32),
               deb=rows_buf(c.B * c.N, c.D, BF16), wpart=rows_buf(c.B * c.tiles * c.D, 64, F32))
    if c.R and not c.dreg_null:
        out["dreg"] = rows_buf(c.R, c.D, F32)
    return out


def _gelu32(x):
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def _gelu_grad32(x):
    return 0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x)


def standin_conv(c, fault=None):
    inp = conv_inputs(c)
    e, w, bias, dxs = inp["e"], inp["w"], inp["bias"], inp["dxs"][:, c.R:]
    mb = inp["mask"][..., None] if inp["mask"] is not None else torch.ones(c.B, c.N, 1, dtype=torch.bool)
    ks, half, N = c.ks, c.ks // 2, c.N
    em = torch.where(mb, e, torch.zeros(()))
    xp = Fn.pad(em, (0, 0, half, half))
    n = torch.arange(N)
    pre = bias.expand(c.B, N, c.D).clone()
    for k in range(ks):  # tap order
        term = w[:, k] * _taps(xp, k, N)
        if fault == "seam":  # a tap whose source frame lies across the 63 | 64 tile seam reads nothing
            src = n + k - half
            term[:, ((n < CT) & (src >= CT)) | ((n >= CT) & (n < 2 * CT) & (src < CT))] = 0
        pre = pre + term
    xs = (em if fault == "mask_e" else e) + torch.where(mb, _gelu32(pre), torch.zeros(()))
    out = new_conv_out(c)
    full = torch.cat([inp["reg"].expand(c.B, c.R, c.D), xs], 1).reshape(-1, c.D)
    out["xs"][: full.shape[0]] = full
    out["xs_libm"][: full.shape[0]] = full
    dpre = torch.where(mb, dxs * _gelu_grad32(pre), torch.zeros(()))
    dp = Fn.pad(dpre, (0, 0, half, half))
    acc = torch.zeros(c.B, N, c.D)
    for k in range(ks):
        acc = acc + w[:, k] * _taps(dp, 2 * half - k, N)
    de = dxs + torch.where(mb, acc, torch.zeros(()))
    out["de"][: c.B * N] = de.reshape(-1, c.D)
    out["deb"][: c.B * N] = de.reshape(-1, c.D).to(BF16)
    rec = out["wpart"][: c.B * c.tiles * c.D].view(c.B * c.tiles, c.D, 64)
    rec[..., :31] = 0  # the kernel stores its 32 accumulators: taps [0, ks), zeros up to 30, the bias gradient at 63
    for k in range(ks):
        rec[..., k] = _tile_sums(dpre * _taps(xp, k, N))
    rec[..., 31 if fault == "bias_slot" else 63] = _tile_sums(dpre)
    if "dreg" in out:
        out["dreg"][: c.R] = inp["dxs"][:, : c.R].sum(0)
    return out


def check_conv(c, got):
    inp = conv_inputs(c)
    ref = conv_reference(c, inp)
    ck = RowChecks(c.name)
    Np, rows = c.N + c.R, c.B * (c.N + c.R)
    for k, cls in (("xs", "conv_fwd"), ("xs_libm", "conv_fwd_libm")):
        xs = got[k][:rows].reshape(c.B, Np, c.D)
        r, cnt, apx = ref["xs"]
        ck.ratio(cls, k + "[:, R:]", xs[:, c.R:], r, cnt, apx if k == "xs" else 0.0)
        ck.same_bits(k + "[:, :R] is reg", xs[:, : c.R], inp["reg"].expand(c.B, c.R, c.D))
        ck.sentinel_kept(k + " guard row", got[k][rows:])
    ck.ratio("conv_de", "de", got["de"][: c.B * c.N], *(t.reshape(-1, c.D) if torch.is_tensor(t) else t for t in ref["de"]))
    ck.ratio("conv_deb", "deb", got["deb"][: c.B * c.N], *(t.reshape(-1, c.D) if torch.is_tensor(t) else t for t in ref["de"]), fmt=BF16)
    ck.same_bits("deb is round-to-nearest-even of the stored de", got["deb"][: c.B * c.N], got["de"][: c.B * c.N].to(BF16))
    ck.sentinel_kept("de guard row", got["de"][c.B * c.N:])
    ck.sentinel_kept("deb guard row", got["deb"][c.B * c.N:])
    nrec = c.B * c.tiles * c.D
    rec = got["wpart"][:nrec].reshape(c.B * c.tiles, c.D, 64)
    slots = list(range(c.ks)) + [63]  # entries [ks, 62] are unspecified and never read
    ck.ratio("conv_wpart", "wpart", rec[..., slots], *(t[..., slots] for t in ref["wpart"]))
    ck.sentinel_kept("wpart guard row", got["wpart"][nrec:])
    if c.R and not c.dreg_null:
        ck.ratio("conv_dreg", "dreg", got["dreg"][: c.R], *ref["dreg"])
        ck.sentinel_kept("dreg guard row", got["dreg"][c.R:])
    ck.done()


# vbx_conv_wgrad_finalize on records of its own: (chunks, D, ks) -- the 4-way unrolled loop at chunks % 4 = 1, 3, 0, 1 and 1
FINALIZE_CASES = ((1, 40, 31), (3, 1, 3), (4, 72, 1), (5, 40, 31), (9, 64, 3))


def finalize_name(f):
    return "finalize-c%d-D%d-ks%d" % f


@lru_cache(maxsize=2)
def finalize_input(f):
    chunks, D, ks = f
    w = torch.randn(chunks, D, 64, generator=_gen(("finalize",) + f))
    w[..., ks:63] = math.nan  # never read
    return nan_guard(w, 64)


def new_finalize_out(f):
    return dict(dw=rows_buf(f[1], f[2], F32), db=rows_buf(1, f[1], F32))


def standin_finalize(f):
    chunks, D, ks = f
    w = finalize_input(f)[:-1].reshape(chunks, D, 64)
    out = new_finalize_out(f)
    out["dw"][:D] = w[..., :ks].sum(0)
    out["db"][0] = w[..., 63].sum(0)
    return out


def check_finalize(f, got):
    chunks, D, ks = f
    w = finalize_input(f)[:-1].reshape(chunks, D, 64).double()
    ck = RowChecks(finalize_name(f))
    ck.ratio("conv_finalize", "dw", got["dw"][:D], w[..., :ks].sum(0), U * chunks * w[..., :ks].abs().sum(0))
    ck.ratio("conv_finalize", "db", got["db"][0], w[..., 63].sum(0), U * chunks * w[..., 63].abs().sum(0))
    ck.sentinel_kept("dw guard row", got["dw"][D:])
    ck.sentinel_kept("db guard row", got["db"][1:])
    ck.done()
