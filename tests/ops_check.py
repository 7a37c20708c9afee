"""Cases, fp64 references, fp32 stand-ins and per-element bounds of the conditioning and loss kernel edge tests
(tests/test_ops_check_cpu.py checks the checks on the CPU, tests/test_ops_edges_gpu.py launches every case).  torch on the CPU only:
nothing here touches the library or a device.

The kernels, all of csrc/ops.hip: the adaLN projection forward (the MFMA weight-streaming kernel and the scalar LDS-staged one), its
backward (v2 with LDS slices, v1 for J > 8192), vbx_adaln_dtemb_all with the wide row sum behind it, vbx_sum_rows_f32, the GEGLU
backward plain and with column-sum records, the column sums, the masked MSE forward and backward, the CFM inputs and the ODE glue
(axpy by index and by counter, ada_select, counter_add).  Inputs are seeded and rounded once to the type the kernel reads; every element
of every output is compared with fp64, partial records one by one against the fp64 sum over the record's own rows; every output starts
as NaN sentinels with a guard row behind it; every operand row or padding column a launch must not read is NaN; copies are compared by
bits.

The bounds are counted by the rules at the top of tests/rows_check.py (u = 2^-24 per fp32 rounding on the element's path, first order
through the fp64 formula with absolute values, MARGIN = 2 for another summation order, half an ulp of a bf16 store).  The device code
is compiled with contraction on: a product-sum may be fused, which removes roundings from the count and never adds one, so the counts
below are those of the unfused form.  Terms that stand beside the counted part without margin:
 * ERF_AS (rows_check): the Abramowitz-Stegun erf of gelu_erf / gelu_erf_grad;
 * RHO_A (rows_check): the relative error of __expf inside gelu_erf_grad, twice the figure measured through the scan's sigmoid over
   __expf arguments in [-8, 6]; every GEGLU gate here keeps 0.5 g^2 <= 6;
 * A_SINCOS and RHO_SILU: sinf / cosf of time_four_kernel and the expf inside the SiLU of time_linear_kernel and silu_grad, twice the
   values measured through vbx_time_embed_fwd over stated sweeps (section A below);
 * the hi + lo fp16 split of temb in the MFMA projection, per product t w: |w| (2^-22 |t| + 2^-25) -- lo = fp16(t - fp16(t)) carries
   |t - hi| <= 2^-11 |t| with a relative rounding of 2^-11 where it is a normal fp16 number and with half the subnormal spacing, 2^-25,
   where it is not.  This holds only under gradual underflow in the convert and in the MFMA; the `small` cases (|t| in [2^-10, 2^-3),
   every lo subnormal) test that.
"""
import json
import math
import os
from dataclasses import astuple, dataclass
from functools import lru_cache

import torch

from optim_check import _gen, bits, sentinel
from rows_check import BF16, ERF_AS, F16, F32, F64, INV_SQRT_2PI, N_ERF, RHO_A, SQRT1_2, U, RowChecks, cdiv, nan_guard, rows_buf

I32 = torch.int32
GRID_CAP = 4096 * 256  # grid_for(): at most 4096 blocks of 256 threads; more work items than this take the grid-stride loop
NAN = math.nan


class OpsChecks(RowChecks):
    """rows_check.RowChecks with the log of these tests: OPS_CHECK_LOG=<file> appends one JSON line per case with every measured value
    (how profiles/ops_edges_measured.json was made)."""

    def done(self):
        if os.environ.get("OPS_CHECK_LOG"):
            with open(os.environ["OPS_CHECK_LOG"], "a") as f:
                f.write(json.dumps({"case": self.case, "values": [(n, v if isinstance(v, bool) else float(v), b) for n, v, b in self.seen]}) + "\n")
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)

    def zeros(self, name, t):
        self.true(f"{name} is exactly zero", bool((t == 0).all()))


def flat_buf(n, dtype, guard=8):
    """n elements and `guard` more behind them, all sentinels"""
    return sentinel(n + guard, dtype)


def _nan_pad(x, pad):
    """[..., C] -> [..., C + pad] with NaN in the padding columns"""
    return torch.cat([x, torch.full(x.shape[:-1] + (pad,), NAN, dtype=x.dtype)], -1) if pad else x


# ================================================================================================ B. adaLN projection forward
def fwd_kernel(B, Th):
    """the dispatch of vbx_adaln_proj_fwd"""
    return "mfma" if B <= 16 and Th % 32 == 0 else "scalar"


@dataclass(frozen=True)
class AdaFwdCase:
    kernel: str
    B: int
    Th: int
    J: int
    group: int = 0  # 0: one group of J
    small: bool = False  # |temb| in [2^-10, 2^-3): every lo half of the MFMA kernel's split is an fp16 subnormal

    @property
    def name(self):
        return f"adafwd-{self.kernel}-B{self.B}-Th{self.Th}-J{self.J}-g{self.group}{'-small' if self.small else ''}"

    @property
    def G(self):
        return self.group or self.J


ADA_J = (1, 15, 16, 17, 63, 64, 65, 130)
ADA_GROUPS = ((130, 130), (72, 24), (136, 8), (512, 128))  # (J, group): 24 and 8 put a group seam inside a wave's 16 outputs


def _ada_fwd_table():
    out = []
    for i, B in enumerate((1, 4, 5, 12, 13, 16)):  # every B meets every Th, every J occurs three times
        for j, Th in enumerate((32, 256, 288, 544)):
            out.append(AdaFwdCase("mfma", B, Th, ADA_J[(4 * i + j) % 8]))
    out += [AdaFwdCase("mfma", 16, 544, J) for J in ADA_J if J != 65] + [AdaFwdCase("mfma", 13, 288, J) for J in ADA_J if J != 17]
    out += [AdaFwdCase("mfma", B, 288, J, g) for B in (5, 16) for J, g in ADA_GROUPS]
    out += [AdaFwdCase("mfma", 13, Th, 65, small=True) for Th in (32, 256, 288, 544)]
    for B, Th in ((17, 32), (3, 8), (3, 264), (9, 40), (16, 24), (8, 4104)):
        out += [AdaFwdCase("scalar", B, Th, J) for J in (1, 17, 64, 65)]
    out += [AdaFwdCase("scalar", B, Th, J, g) for B, Th in ((3, 264), (17, 32)) for J, g in ADA_GROUPS]
    return list(dict.fromkeys(out))


ADA_FWD_CASES = _ada_fwd_table()
SMALL_TH = 32  # the smallest Th at which the counted bound separates the stand-in (< 0.5) from the lo-half faults (> 1)


@lru_cache(maxsize=2)
def ada_fwd_inputs(c):
    g = _gen(("adafwd",) + astuple(c))
    if c.small:
        temb = torch.exp2(-10 + 7 * torch.rand(c.B, c.Th, generator=g)) * (1 - 2 * torch.randint(0, 2, (c.B, c.Th), generator=g))
        temb = temb.clamp(min=-(2.0 ** -3) * (1 - 2.0 ** -20), max=2.0 ** -3 * (1 - 2.0 ** -20)).float()
    else:
        temb = torch.nn.functional.silu(1.5 * torch.randn(c.B, c.Th, generator=g))  # what the time MLP hands over
    w = (torch.randn(c.J, c.Th, generator=g) * c.Th ** -0.5).to(F16)
    return dict(temb=temb, w=w, bias=torch.randn(c.J, generator=g))


def ada_fwd_reference(c, inp):
    """(ref, counted, approx) [B, J]: ada[b][j] = bias[j] + temb[b, :] . W[j, :]"""
    t, w = inp["temb"].double(), inp["w"].double()
    dot = t @ w.t()
    S = t.abs() @ w.abs().t()
    ref = dot + inp["bias"].double()
    if c.kernel == "mfma":
        # the products hi w and lo w are exact in fp32 (11 + 11 bits); an MFMA adds 32 of them to the accumulator: five tree levels and
        # the accumulation, and the accumulator passes through 2 Th / 32 MFMAs; then + bias
        n = 5 + 2 * c.Th // 32
        approx = 2.0 ** -22 * S + 2.0 ** -25 * w.abs().sum(1)[None, :]
    else:
        # a lane: 8 products and 8 additions per chunk of 8, cdiv(Th / 8, 64) chunks; six levels of the wave tree; + bias
        n = 1 + 8 * cdiv(c.Th // 8, 64) + 6
        approx = torch.zeros_like(S)
    return ref, U * (n * S + ref.abs()), approx


def ada_rows(c):
    return (c.J // c.G) * c.B


def new_ada_fwd_out(c):
    return dict(ada=rows_buf(ada_rows(c), c.G, F32))


def _ada_layout(c, x, jg=None):
    """[B, J] -> the grouped layout [(J / G) B, G]; jg: the group index each column j is stored under"""
    out = sentinel(ada_rows(c) * c.G, F32).view(c.J // c.G, c.B, c.G)
    j = torch.arange(c.J)
    out[(j // c.G) if jg is None else jg, :, j % c.G] = x.t()
    return out.reshape(-1, c.G)


def standin_ada_fwd(c, fault=None):
    inp = ada_fwd_inputs(c)
    t, w = inp["temb"], inp["w"].float()
    if fault == "kround":  # the partial round of k-steps behind the last full 256 never runs
        t = t.clone()
        t[:, c.Th // 256 * 256:] = 0
    if c.kernel == "mfma":
        hi = t.to(F16)
        lo = (t - hi.float()).to(F16)
        if fault == "flush_lo":
            lo = torch.where(lo.float().abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
        acc = hi.float() @ w.t()
        if fault != "no_lo":
            acc = acc + lo.float() @ w.t()
    else:
        acc = t @ w.t()
    x = acc + inp["bias"]
    j = torch.arange(c.J)
    out = new_ada_fwd_out(c)
    lay = _ada_layout(c, x, (j // 16 * 16) // c.G if fault == "group_first" else None)
    if fault == "rowshift":  # C-layout rows of lane quads 1..3 land on quad 0's batch rows
        lay = lay.view(c.J // c.G, c.B, c.G)
        keep = lay.clone()
        lay[:, 4:] = sentinel(1, F32)
        lay[:, : c.B - 4] = keep[:, 4:]
        lay = lay.reshape(-1, c.G)
    out["ada"][: ada_rows(c)] = lay
    return out


def check_ada_fwd(c, got):
    inp = ada_fwd_inputs(c)
    ref, counted, approx = ada_fwd_reference(c, inp)
    n = ada_rows(c)
    ck = OpsChecks(c.name)
    ck.true("the dispatch takes this kernel", fwd_kernel(c.B, c.Th) == c.kernel)
    if c.small:
        a = inp["temb"].abs()
        ck.true("temb magnitudes lie in [2^-10, 2^-3)", 2.0 ** -10 <= float(a.min()) and float(a.max()) < 2.0 ** -3)
    ada = got["ada"][:n].reshape(c.J // c.G, c.B, c.G).permute(1, 0, 2).reshape(c.B, c.J)
    ck.ratio("ada_fwd_" + c.kernel + ("_small" if c.small else ""), "ada", ada, ref, counted, approx)
    ck.sentinel_kept("ada guard row", got["ada"][n:])
    ck.done()
    return ck


# ================================================================================================ C. adaLN projection backward
ADA_SLICES, ADA_PER_MAX, ADA_TG = 128, 64, 8


def bwd_kernel(J):
    """the dispatch of vbx_adaln_proj_bwd"""
    return "v2" if J <= ADA_SLICES * ADA_PER_MAX else "v1"


@dataclass(frozen=True)
class AdaBwdCase:
    kernel: str
    B: int
    Th: int
    J: int
    dw: bool
    acc: int

    @property
    def name(self):
        return f"adabwd-{self.kernel}-B{self.B}-Th{self.Th}-J{self.J}-{'dw' if self.dw else 'nodw'}-acc{self.acc}"

    @property
    def per(self):
        return cdiv(self.J, ADA_SLICES)


def _ada_bwd_table():
    out, Bs = [], (1, 8, 9, 11)
    for i, J in enumerate((1, 4, 127, 129, 516, 1100, 8192)):  # per = 1, 1, 1, 2, 5, 9, 64
        for j, Th in enumerate((8, 264, 2056)):
            if J == 8192 and Th == 2056:  # 2 x 67 MB of operands: the slice length 64 is met at Th = 8 and 264
                continue
            out.append(AdaBwdCase("v2", Bs[(i + j) % 4], Th, J, (i + j) % 2 == 0, (i + j // 2) % 2))
    out += [AdaBwdCase("v2", B, 264, 129, dw, acc) for B in Bs for dw, acc in ((True, 1), (False, 0))]
    out += [AdaBwdCase("v2", B, 2056, 4, True, 1) for B in (9, 11)]
    out += [AdaBwdCase("v1", B, Th, 8196, (k + B) % 2 == 0, k) for k, Th in enumerate((8, 264)) for B in (1, 8, 9)]
    out.append(AdaBwdCase("v1", 1, 2056, 8196, False, 1))
    return list(dict.fromkeys(out))


ADA_BWD_CASES = _ada_bwd_table()


@lru_cache(maxsize=2)
def ada_bwd_inputs(c):
    g = _gen(("adabwd",) + astuple(c))
    return dict(temb=torch.randn(c.B, c.Th, generator=g), w=(torch.randn(c.J, c.Th, generator=g) * 0.05).to(F16),
                dada=torch.randn(c.B, c.J, generator=g), prior=torch.randn(c.B, c.Th, generator=g))


def _slice_sums(x, per, n):
    """[J, ...] -> [n, ...]: the sum over each slice's own rows (slices past the end are empty)"""
    J = x.shape[0]
    pad = torch.zeros((n * per - J,) + x.shape[1:], dtype=x.dtype)
    return torch.cat([x, pad]).reshape((n, per) + x.shape[1:]).sum(1)


def new_ada_bwd_out(c):
    inp = ada_bwd_inputs(c)
    out = dict(scratch=rows_buf(ADA_SLICES * c.B, c.Th, F32), dbias=rows_buf(1, c.J, F32), dtemb=rows_buf(c.B, c.Th, F32))
    if c.acc:
        out["dtemb"][: c.B] = inp["prior"]
    if c.dw:
        out["dw"] = rows_buf(c.J, c.Th, F32)
    return out


def standin_ada_bwd(c, fault=None):
    inp = ada_bwd_inputs(c)
    temb, w, dada = inp["temb"], inp["w"].float(), inp["dada"]
    out = new_ada_bwd_out(c)
    terms = dada.t()[:, :, None] * w[:, None, :]  # [J, B, Th]
    if fault == "tail":  # the last row of the last slice that has rows
        terms = terms.clone()
        terms[c.J - 1] = 0
    sc = _slice_sums(terms, c.per, ADA_SLICES)
    out["scratch"][: ADA_SLICES * c.B] = sc.reshape(-1, c.Th)
    d = sc.sum(0)
    out["dtemb"][: c.B] = d + inp["prior"] if c.acc and fault != "acc" else d
    out["dbias"][0] = dada[: 8 if fault == "dbias8" else c.B].sum(0)
    if c.dw:
        out["dw"][: c.J] = dada.t() @ temb
    return out


def check_ada_bwd(c, got):
    inp = ada_bwd_inputs(c)
    temb, w, dada = inp["temb"].double(), inp["w"].double(), inp["dada"].double()
    ck = OpsChecks(c.name)
    ck.true("the dispatch takes this kernel", bwd_kernel(c.J) == c.kernel)
    # scratch[slice][b][t] = sum over the slice's rows of dada[b][j] W[j][t]: a product and an addition per row
    ref, S = torch.zeros(ADA_SLICES, c.B, c.Th, dtype=F64), torch.zeros(ADA_SLICES, c.B, c.Th, dtype=F64)
    ns = cdiv(c.J, c.per)  # slices that have rows; built slice by slice to keep the [J, B, Th] product out of memory
    for s in range(ns):
        sl = slice(s * c.per, min(c.J, (s + 1) * c.per))
        ref[s], S[s] = dada[:, sl] @ w[sl], dada[:, sl].abs() @ w[sl].abs()
    c_sc = U * (1 + c.per) * S
    n = ADA_SLICES * c.B
    ck.ratio("ada_bwd_scratch", "scratch", got["scratch"][:n].reshape(ADA_SLICES, c.B, c.Th), ref, c_sc)
    if ns < ADA_SLICES:
        ck.zeros("scratch of the empty slices", got["scratch"][ns * c.B: n])
    ck.sentinel_kept("scratch guard row", got["scratch"][n:])
    # dtemb = (prior +) the sum of the 128 records: four row lanes of 32 additions, three to join them, the accumulation
    d, dS = ref.sum(0), ref.abs().sum(0)
    c_d = c_sc.sum(0) + U * (32 + 3) * dS
    if c.acc:
        d = d + inp["prior"].double()
        c_d = c_d + U * d.abs()
    ck.ratio("ada_bwd_dtemb", "dtemb", got["dtemb"][: c.B], d, c_d)
    ck.sentinel_kept("dtemb guard row", got["dtemb"][c.B:])
    ck.ratio("ada_bwd_dbias", "dbias", got["dbias"][0], dada.sum(0), U * c.B * dada.abs().sum(0))
    ck.sentinel_kept("dbias guard row", got["dbias"][1:])
    if c.dw:
        ck.ratio("ada_bwd_dw", "dw", got["dw"][: c.J], dada.t() @ temb, U * (1 + c.B) * (dada.abs().t() @ temb.abs()))
        ck.sentinel_kept("dw guard row", got["dw"][c.J:])
    ck.done()


# ================================================================================================ D. vbx_adaln_dtemb_all, the wide row sum
@dataclass(frozen=True)
class DtembCase:
    L: int
    J: int
    B: int
    Th: int

    @property
    def name(self):
        return f"dtemb-L{self.L}-J{self.J}-B{self.B}-Th{self.Th}-rows{self.rows}"

    @property
    def spl(self):
        return cdiv(self.J, ADA_PER_MAX)

    @property
    def rows(self):  # of the sum through sum_rows_wide_kernel
        return self.L * self.spl


def _dtemb_table():
    shapes = [(B, Th) for B in (1, 8, 9, 11) for Th in (8, 264, 2056)]
    LJ = ((1, 4), (1, 64), (1, 65), (3, 4), (3, 64), (3, 65), (1, 516), (3, 516), (3, 704), (1, 64), (3, 65), (3, 516))  # rows 1 1 2 3 3 6 9 27 33 ..
    out = [DtembCase(L, J, *shapes[(5 * i) % 12]) for i, (L, J) in enumerate(LJ)]
    # the wide sum at the row counts where its four-in-flight loop (i + 96 < rows) hands over to the tail loop: one weight row per layer
    out += [DtembCase(L, 1, (1, 9)[i % 2], 8) for i, L in enumerate((32, 33, 97, 128, 129, 161))]
    return out


DTEMB_CASES = _dtemb_table()


@lru_cache(maxsize=2)
def dtemb_inputs(c):
    g = _gen(("dtemb",) + astuple(c))
    return dict(w=(torch.randn(c.L, c.J, c.Th, generator=g) * 0.05).to(F16), dada=torch.randn(c.L, c.B, c.J, generator=g))


def new_dtemb_out(c):
    return dict(scratch=rows_buf(c.rows * c.B, c.Th, F32), dtemb=rows_buf(c.B, c.Th, F32))


def standin_dtemb(c, fault=None):
    inp = dtemb_inputs(c)
    w, dada = inp["w"].float(), inp["dada"]
    sc = torch.zeros(c.L, c.spl, c.B, c.Th)
    for s in range(c.spl):
        sl = slice(s * ADA_PER_MAX, min(c.J, (s + 1) * ADA_PER_MAX))
        sc[:, s] = torch.einsum("lbj,ljt->lbt", dada[:, :, sl], w[:, sl])
    if fault == "clamp":  # the rows that round the last slice up to ADA_TG carry the clamped row's weight instead of zero
        per = c.J - (c.spl - 1) * ADA_PER_MAX
        sc[:, -1] += (cdiv(per, ADA_TG) * ADA_TG - per) * dada[:, :, c.J - 1, None] * w[:, c.J - 1][:, None, :]
    out = new_dtemb_out(c)
    out["scratch"][: c.rows * c.B] = sc.reshape(-1, c.Th)
    out["dtemb"][: c.B] = sc.sum((0, 1))
    return out


def check_dtemb(c, got):
    inp = dtemb_inputs(c)
    w, dada = inp["w"].double(), inp["dada"].double()
    ref, S = torch.zeros(c.L, c.spl, c.B, c.Th, dtype=F64), torch.zeros(c.L, c.spl, c.B, c.Th, dtype=F64)
    for s in range(c.spl):
        sl = slice(s * ADA_PER_MAX, min(c.J, (s + 1) * ADA_PER_MAX))
        ref[:, s] = torch.einsum("lbj,ljt->lbt", dada[:, :, sl], w[:, sl])
        S[:, s] = torch.einsum("lbj,ljt->lbt", dada[:, :, sl].abs(), w[:, sl].abs())
    c_sc = U * (1 + min(c.J, ADA_PER_MAX)) * S
    n = c.rows * c.B
    ck = OpsChecks(c.name)
    ck.ratio("dtemb_scratch", "scratch", got["scratch"][:n].reshape(ref.shape), ref, c_sc)
    ck.sentinel_kept("scratch guard row", got["scratch"][n:])
    # 32 row lanes of cdiv(rows, 32) additions each, 32 additions to join them
    ck.ratio("dtemb_sum", "dtemb", got["dtemb"][: c.B], ref.sum((0, 1)), c_sc.sum((0, 1)) + U * (cdiv(c.rows, 32) + 32) * ref.abs().sum((0, 1)))
    ck.sentinel_kept("dtemb guard row", got["dtemb"][c.B:])
    ck.done()


# ================================================================================================ E. vbx_sum_rows_f32
@dataclass(frozen=True)
class SumRowsCase:
    rows: int
    cols: int
    pad: int  # ld = cols + pad, NaN in the padding
    acc: int

    @property
    def name(self):
        return f"sumrows-r{self.rows}-c{self.cols}-pad{self.pad}-acc{self.acc}"


# 1, 4, 5: the four row lanes; 12, 13, 16, 17, 33: around i + 12 < rows, where four rows in flight hand over to the tail loop
SUM_ROWS_CASES = [SumRowsCase(r, cl, (0, 3)[(i + j) % 2], (i + j // 2) % 2) for i, r in enumerate((1, 4, 5, 12, 13, 16, 17, 33))
                  for j, cl in enumerate((1, 63, 64, 65))]


@lru_cache(maxsize=2)
def sum_rows_inputs(c):
    g = _gen(("sumrows",) + astuple(c))
    return dict(x=torch.randn(c.rows, c.cols, generator=g), prior=torch.randn(c.cols, generator=g))


def sum_rows_operand(c):
    return nan_guard(_nan_pad(sum_rows_inputs(c)["x"], c.pad), c.cols + c.pad)


def new_sum_rows_out(c):
    out = rows_buf(1, c.cols, F32)
    if c.acc:
        out[0] = sum_rows_inputs(c)["prior"]
    return dict(out=out)


def standin_sum_rows(c):
    inp = sum_rows_inputs(c)
    out = new_sum_rows_out(c)
    out["out"][0] = inp["x"].sum(0) + (inp["prior"] if c.acc else 0)
    return out


def check_sum_rows(c, got):
    inp = sum_rows_inputs(c)
    x = inp["x"].double()
    ref = x.sum(0) + (inp["prior"].double() if c.acc else 0)
    ck = OpsChecks(c.name)
    ck.ratio("sum_rows", "out", got["out"][0], ref, U * ((cdiv(c.rows, 4) + 3) * x.abs().sum(0) + c.acc * ref.abs()))
    ck.sentinel_kept("out guard row", got["out"][1:])
    ck.done()


# ================================================================================================ F. GEGLU backward
GB_SLABS = 512
ZERO_OF_GELU_GRAD = -0.7517916


@dataclass(frozen=True)
class GegluCase:
    M: int
    Fp: int
    colsum: bool = True  # also the form with records (both forms are one kernel over 512 row slabs; the large case runs it once, without)

    @property
    def name(self):
        return f"geglu-M{self.M}-Fp{self.Fp}"


# M = 1, 3, 5: the four row lanes; 511, 512, 513, 1025: per = 1, 1, 2, 3 rows a slab with empty and ragged last slabs
GEGLU_CASES = [GegluCase(M, Fp) for Fp in (64, 192, 512, 576) for M in (1, 3, 5, 511, 512, 513, 1025)]
GEGLU_CASES.append(GegluCase(GRID_CAP // 8 + 5, 64, colsum=False))  # M Fp / 8 > 4096 x 256: 257 rows a slab


@lru_cache(maxsize=2)
def geglu_inputs(c):
    g = _gen(("geglu",) + astuple(c))
    h1 = (1.2 * torch.randn(c.M, 2 * c.Fp, generator=g)).view(c.M, c.Fp // 64, 2, 64)
    h1[:, :, 1] = h1[:, :, 1].clamp(-3.4, 3.4)  # gates: 0.5 g^2 <= 5.78
    near = torch.rand(c.M, c.Fp // 64, 64, generator=g) < 0.1
    h1[:, :, 1] = torch.where(near, ZERO_OF_GELU_GRAD + 0.01 * torch.randn(c.M, c.Fp // 64, 64, generator=g), h1[:, :, 1])
    return dict(h1=h1.reshape(c.M, 2 * c.Fp).to(BF16), dg=torch.randn(c.M, c.Fp, generator=g).to(BF16))


def geglu_reference(c, inp):
    """(ref, counted, approx) [M, 2 Fp] in the interleaved layout: per block of 128, dx = dg GELU(g) | dgate = dg x GELU'(g)"""
    h = inp["h1"].double().view(c.M, c.Fp // 64, 2, 64)
    x, g, dg = h[:, :, 0], h[:, :, 1], inp["dg"].double().view(c.M, c.Fp // 64, 64)
    erf, phi = torch.special.erf(g * SQRT1_2), torch.exp(-0.5 * g * g) * INV_SQRT_2PI
    d_erf = U * N_ERF * (2 * (g * phi).abs() + erf.abs())  # as rows_check.conv_reference: the argument through erf', erf_as's own arithmetic
    gelu, g1 = 0.5 * g * (1 + erf), 0.5 * (1 + erf) + g * phi
    dx = dg * gelu
    c_dx = dg.abs() * (0.5 * g.abs() * (d_erf + U * (1 + erf).abs()) + 2 * U * gelu.abs()) + U * dx.abs()
    a_dx = dg.abs() * 0.5 * g.abs() * ERF_AS
    # x c __expf(-0.5 x x): two products into the argument (g^2 u on the exponential), the products x c and (x c) e; then the addition
    c_g1 = 0.5 * (d_erf + U * (1 + erf).abs()) + U * (g * phi).abs() * (g * g + 2) + U * g1.abs()
    a_g1 = 0.5 * ERF_AS + (g * phi).abs() * RHO_A
    dgate = dg * x * g1
    c_dgate = (dg * x).abs() * c_g1 + 2 * U * dgate.abs()
    a_dgate = (dg * x).abs() * a_g1
    st = lambda a, b: torch.stack([a, b], 2).reshape(c.M, 2 * c.Fp)  # noqa: E731
    return st(dx, dgate), st(c_dx, c_dgate), st(a_dx, a_dgate), float((0.5 * g * g).max())


def new_geglu_out(c):
    out = dict(dh1=rows_buf(c.M, 2 * c.Fp, BF16))
    if c.colsum:
        out.update(dh1_cs=rows_buf(c.M, 2 * c.Fp, BF16), rec=rows_buf(GB_SLABS, 2 * c.Fp, F32))
    return out


def _trunc_bf16(x):
    return (bits(x.float()) & -65536).view(F32).to(BF16)


def standin_geglu(c, fault=None):
    inp = geglu_inputs(c)
    h = inp["h1"].float().view(c.M, c.Fp // 64, 2, 64)
    x, g, dg = h[:, :, 0].clone(), h[:, :, 1].clone(), inp["dg"].float().view(c.M, c.Fp // 64, 64)
    if fault == "swap":
        x[:, -1], g[:, -1] = h[:, -1, 1], h[:, -1, 0]
    gelu = 0.5 * g * (1.0 + torch.erf(g * SQRT1_2))
    g1 = 0.5 * (1.0 + torch.erf(g * SQRT1_2)) + g * INV_SQRT_2PI * torch.exp(-0.5 * g * g)
    o32 = torch.stack([dg * gelu, dg * x * g1], 2).reshape(c.M, 2 * c.Fp)
    ob = _trunc_bf16(o32) if fault == "trunc" else o32.to(BF16)
    out = new_geglu_out(c)
    out["dh1"][: c.M] = ob
    if c.colsum:
        out["dh1_cs"][: c.M] = ob
        out["rec"][:GB_SLABS] = _slice_sums(o32 if fault == "rec32" else ob.float(), cdiv(c.M, GB_SLABS), GB_SLABS)
    return out


def check_geglu(c, got):
    inp = geglu_inputs(c)
    ref, counted, approx, arg = geglu_reference(c, inp)
    ck = OpsChecks(c.name)
    ck.le("0.5 g^2 of the largest gate", arg, 6.0)
    ck.ratio("geglu_dh1", "dh1", got["dh1"][: c.M], ref, counted, approx, fmt=BF16)
    ck.sentinel_kept("dh1 guard row", got["dh1"][c.M:])
    if c.colsum:
        ck.same_bits("dh1 of the colsum form is dh1 of the plain form", got["dh1_cs"], got["dh1"])
        per = cdiv(c.M, GB_SLABS)
        stored = got["dh1_cs"][: c.M].double()  # the records sum the STORED bf16 values
        ck.ratio("geglu_rec", "slab records", got["rec"][:GB_SLABS], _slice_sums(stored, per, GB_SLABS),
                 U * (cdiv(per, 4) + 3) * _slice_sums(stored.abs(), per, GB_SLABS))  # four row lanes, three additions to join them
        ck.zeros("records of the empty slabs", got["rec"][cdiv(c.M, per): GB_SLABS])
        ck.sentinel_kept("record guard row", got["rec"][GB_SLABS:])
    ck.done()


# ================================================================================================ G. column sums
CS_SLABS = 128


@dataclass(frozen=True)
class ColsumCase:
    kind: str  # "bf16", "f32"
    M: int
    C: int
    pad: int
    rowmap: int = 0
    Fd: int = 0
    out_len: int = 0  # 0: the whole range

    @property
    def name(self):
        return f"colsum-{self.kind}-M{self.M}-C{self.C}-pad{self.pad}-map{self.rowmap}-F{self.Fd}-len{self.out_len}"

    @property
    def n_out(self):
        return self.out_len or (2 * self.Fd if self.rowmap else self.C)


# M = 1, 5: the four row lanes; 127, 128, 129, 257: per = 1, 1, 2, 3 rows a slab; C = 520 / 260: a second column block of one live group
COLSUM_CASES = [ColsumCase("bf16", M, C, (0, 8)[(i + j) % 2]) for i, C in enumerate((8, 512, 520)) for j, M in enumerate((1, 5, 127, 128, 129, 257))]
COLSUM_CASES += [ColsumCase("bf16", M, 2 * Fp, pad, 1, Fd) for (Fd, Fp), M, pad in (((60, 64), 5, 8), ((170, 192), 129, 0), ((60, 64), 257, 0), ((170, 192), 1, 8))]
COLSUM_CASES.append(ColsumCase("bf16", 129, 384, 8, 1, 170, out_len=300))  # out_len shorter than the mapped range 2 Fd = 340
COLSUM_CASES += [ColsumCase("f32", M, C, (0, 4)[(i + j) % 2]) for i, C in enumerate((4, 256, 260)) for j, M in enumerate((1, 5, 129, 257))]


def geglu_row_unmap(p, F):
    blk, w = p >> 7, p & 127
    f = blk * 64 + (w & 63)
    return -1 if f >= F else (f if w < 64 else F + f)


@lru_cache(maxsize=2)
def colsum_input(c):
    x = torch.randn(c.M, c.C, generator=_gen(("colsum",) + astuple(c)))
    return x.to(BF16) if c.kind == "bf16" else x


def colsum_operand(c):
    return nan_guard(_nan_pad(colsum_input(c), c.pad), c.C + c.pad)


def new_colsum_out(c):
    return dict(out=rows_buf(1, c.n_out, F32), rec=rows_buf(CS_SLABS, c.C, F32))


def _colsum_map(c, shift=0):
    """destination of every column (-1: dropped)"""
    if not c.rowmap:
        return list(range(c.C))
    dst = [geglu_row_unmap(p + shift, c.Fd) if p + shift < c.C else -1 for p in range(c.C)]
    return [d if d < c.n_out else -1 for d in dst]


def standin_colsum(c, fault=None):
    x = colsum_input(c).float()
    if fault == "pad":  # the first padding column is read as one more row of column 0's group
        x = x.clone()
        x[:, 0] += colsum_operand(c)[: c.M, c.C].float()
    per = cdiv(c.M, CS_SLABS)
    xs = x
    if fault == "lastrow":
        xs = x.clone()
        xs[min(c.M, per) - 1] = 0  # the last row of slab 0
    out = new_colsum_out(c)
    rec = _slice_sums(xs, per, CS_SLABS)
    out["rec"][:CS_SLABS] = rec
    tot = rec.sum(0)
    for p, d in enumerate(_colsum_map(c, 128 if fault == "mapblock" else 0)):
        if d >= 0:
            out["out"][0, d] = tot[p]
    return out


def check_colsum(c, got, partials_only=False):
    x = colsum_input(c).double()
    per = cdiv(c.M, CS_SLABS)
    ck = OpsChecks(c.name + ("-partials" if partials_only else ""))
    rec, Sr = _slice_sums(x, per, CS_SLABS), _slice_sums(x.abs(), per, CS_SLABS)
    c_rec = U * (cdiv(per, 4) + 3) * Sr  # four row lanes, three additions to join them
    ck.ratio("colsum_rec", "slab records", got["rec"][:CS_SLABS], rec, c_rec)
    ck.zeros("records of the empty slabs", got["rec"][cdiv(c.M, per): CS_SLABS])
    ck.sentinel_kept("record guard row", got["rec"][CS_SLABS:])
    if not partials_only:
        dst = torch.tensor(_colsum_map(c))
        live = dst >= 0
        ref, cnt = rec.sum(0), c_rec.sum(0) + U * CS_SLABS * rec.abs().sum(0)
        ck.ratio("colsum_out", "out", got["out"][0][dst[live]], ref[live], cnt[live])
        hit = torch.zeros(c.n_out, dtype=torch.bool)
        hit[dst[live]] = True
        ck.true("every output entry has its column", bool(hit.all()))
        ck.sentinel_kept("out guard row", got["out"][1:])
    ck.done()


# ================================================================================================ H. masked MSE
MSE_SPLITS = 64
EPS_DEN = float(torch.tensor(1e-5, dtype=F32))
MSE_MASKS = ("ones", "one", "late", "empty")
MSE_OUTS = ("f32", "bf16", "both")


@dataclass(frozen=True)
class MseCase:
    B: int
    N: int
    D: int
    mask: str  # "one": only frame min(3, N - 1) of every element; "late": only frame N - 1 >= 256; "empty": element B - 1 has no frame
    gscale: bool
    outs: str

    @property
    def name(self):
        return f"mse-B{self.B}-N{self.N}-D{self.D}-{self.mask}-{'gs' if self.gscale else 'nogs'}-{self.outs}"


def _mse_table():
    out = []
    for i, N in enumerate((1, 4, 255, 256, 257, 513)):  # 257, 513: a second and a third trip of the frame loop n += 256
        for j, D in enumerate((4, 252, 256, 260)):  # 260: a second trip of the lane loop c += 64
            mask = MSE_MASKS[(i + j) % 4]
            if mask == "late" and N <= 256:
                mask = "ones"
            B = 3 if mask == "empty" else (1, 3)[(i + j // 2) % 2]
            out.append(MseCase(B, N, D, mask, (i + j) % 2 == 0, MSE_OUTS[(i + 2 * j) % 3]))
    out += [MseCase(3, 513, 260, "late", True, "both"), MseCase(1, 257, 4, "late", False, "f32"), MseCase(3, 513, 4, "empty", True, "both")]
    out.append(MseCase(1, GRID_CAP // 64 + 16, 256, "ones", True, "both"))  # B N D / 4 > 4096 x 256
    return out


MSE_CASES = _mse_table()
GSCALE = float(torch.tensor(0.37, dtype=F32))


@lru_cache(maxsize=2)
def mse_inputs(c):
    g = _gen(("mse",) + astuple(c))
    pred, target = torch.randn(c.B, c.N, c.D, generator=g), torch.randn(c.B, c.N, c.D, generator=g)
    m = torch.ones(c.B, c.N, dtype=torch.bool)
    if c.mask == "one":
        m[:] = False
        m[:, min(3, c.N - 1)] = True
    elif c.mask == "late":
        m[:] = False
        m[:, c.N - 1] = True
    elif c.mask == "empty":
        m[c.B - 1] = False
    pred[~m] = NAN  # a masked frame is never read
    target[~m] = NAN
    return dict(pred=pred, target=target, mask=m)


def mse_floats(B):
    return 2 * B + 2 * MSE_SPLITS * B


def new_mse_out(c):
    out = dict(per_b=flat_buf(mse_floats(c.B), F32), loss=flat_buf(1, F32))
    if c.outs != "bf16":
        out["dpred"] = rows_buf(c.B * c.N, c.D, F32)
    if c.outs != "f32":
        out["dpb"] = rows_buf(c.B * c.N, c.D, BF16)
    return out


def _split_sums(x):
    """[B, N] -> [B, 64]: split sp takes the frames n with (n % 256) // 4 == sp"""
    B, N = x.shape
    trips = cdiv(N, 4 * MSE_SPLITS)
    pad = torch.zeros(B, trips * 4 * MSE_SPLITS - N, dtype=x.dtype)
    return torch.cat([x, pad], 1).reshape(B, trips, MSE_SPLITS, 4).sum((1, 3))


def standin_mse(c, fault=None):
    inp = mse_inputs(c)
    m = inp["mask"]
    diff = torch.where(m[..., None], inp["pred"] - inp["target"], torch.zeros(()))
    fr = (diff * diff).sum(-1) / torch.tensor(float(c.D // 4 if fault == "d4" else c.D))
    mf = m.float()
    if fault == "late":
        fr, mf = fr.clone(), mf.clone()
        fr[:, 256:], mf[:, 256:] = 0, 0
    num, cnt = _split_sums(fr), _split_sums(mf)
    den = cnt.sum(1) if fault == "noclamp" else cnt.sum(1).clamp(min=torch.tensor(1e-5))
    per_b = num.sum(1) / den
    out = new_mse_out(c)
    B = c.B
    out["per_b"][:B], out["per_b"][B: 2 * B] = per_b, den
    out["per_b"][2 * B: mse_floats(B)] = torch.stack([num, cnt], 2).reshape(-1)
    out["loss"][0] = per_b.sum() / torch.tensor(float(B))
    gs = torch.tensor(GSCALE if c.gscale and fault != "nogscale" else 1.0)
    k = gs * 2.0 / (torch.tensor(float(c.D)) * den * torch.tensor(float(B)))
    d = (k[:, None, None] * diff).reshape(-1, c.D)
    if "dpred" in out:
        out["dpred"][: B * c.N] = d
    if "dpb" in out:
        out["dpb"][: B * c.N] = d.to(BF16)
    return out


def check_mse(c, got):
    inp = mse_inputs(c)
    m, B, N, D = inp["mask"], c.B, c.N, c.D
    diff = torch.where(m[..., None], inp["pred"].double() - inp["target"].double(), torch.zeros((), dtype=F64))
    fr = (diff * diff).sum(-1) / D
    # a frame: p - t (u, twice through the square), the square, 4 additions per float4 chunk of a lane, six levels of the wave tree,
    # / D; then one addition per trip of the frame loop and three to join the four waves.  Every term is positive.
    n_fr = 3 + 4 * cdiv(D // 4, 64) + 6 + 1 + cdiv(N, 4 * MSE_SPLITS) + 3
    num, cnt = _split_sums(fr), _split_sums(m.double())
    ck = OpsChecks(c.name)
    part = got["per_b"][2 * B: mse_floats(B)].reshape(B, MSE_SPLITS, 2)
    ck.ratio("mse_split", "split numerators", part[..., 0], num, U * n_fr * num)
    ck.same_bits("split counts", part[..., 1], cnt.float())
    count = cnt.sum(1)
    den = count.clamp(min=EPS_DEN)
    ck.same_bits("denominators", got["per_b"][B: 2 * B], den.float())
    per_b = num.sum(1) / den
    c_pb = U * (n_fr + 6 + 1) * per_b  # the wave tree over the 64 splits, the division
    ck.ratio("mse_per_b", "per_b", got["per_b"][:B], per_b, c_pb)
    ck.ratio("mse_loss", "loss", got["loss"][:1], (per_b.sum() / B).reshape(1), (c_pb.sum() / B + U * (B + 1) * per_b.sum() / B).reshape(1))
    ck.sentinel_kept("per_b guard", got["per_b"][mse_floats(B):])
    ck.sentinel_kept("loss guard", got["loss"][1:])
    if c.mask == "empty":
        ck.same_bits("the empty element's denominator is 1e-5f", got["per_b"][2 * B - 1: 2 * B], torch.tensor([1e-5], dtype=F32))
        ck.zeros("the empty element's per_b", got["per_b"][B - 1: B])
    # dpred = gscale 2 (p - t) / (D den B) on the mask: gscale * 2 is exact; D den, * B, the division, p - t, the product
    gs = GSCALE if c.gscale else 1.0
    ref = (gs * 2.0 / (D * den * B))[:, None, None] * diff
    ref, cnt_d = ref.reshape(-1, D), U * 5 * ref.abs().reshape(-1, D)
    for k, fmt in (("dpred", None), ("dpb", BF16)):
        if k in got:
            ck.ratio("mse_" + k, k, got[k][: B * N], ref, cnt_d, fmt=fmt)
            ck.zeros(k + " of the masked frames", got[k][: B * N][~m.reshape(-1)])
            ck.sentinel_kept(k + " guard row", got[k][B * N:])
    if c.outs == "both":
        ck.same_bits("dpred_bf16 is round-to-nearest-even of the stored dpred", got["dpb"][: B * N], got["dpred"][: B * N].to(BF16))
    ck.done()


# ================================================================================================ I. CFM inputs and the ODE glue
SIGMA_01 = float(torch.tensor(0.1, dtype=F32))


@dataclass(frozen=True)
class CfmCase:
    B: int
    per: int
    sigma: float

    @property
    def name(self):
        return f"cfm-B{self.B}-per{self.per}-sigma{self.sigma:.3g}"


CFM_CASES = [CfmCase(3, per, s) for per in (1, 7, 1030) for s in (0.0, SIGMA_01)] + [CfmCase(3, GRID_CAP // 3 + 11, SIGMA_01)]


@lru_cache(maxsize=2)
def cfm_inputs(c):
    g = _gen(("cfm",) + astuple(c))
    return dict(x1=torch.randn(c.B, c.per, generator=g), x0=torch.randn(c.B, c.per, generator=g), times=torch.tensor([0.0, 1.0, 0.3137])[: c.B])


def new_cfm_out(c):
    return dict(w=rows_buf(c.B, c.per, F32), flow=rows_buf(c.B, c.per, F32))


def standin_cfm(c, fault=None):
    inp = cfm_inputs(c)
    x1, x0, t = inp["x1"], inp["x0"], inp["times"][:, None]
    om = torch.tensor(1.0) - torch.tensor(c.sigma)
    out = new_cfm_out(c)
    out["w"][: c.B] = (1.0 - om * t) * x0 + t * x1
    out["flow"][: c.B] = om * x1 - x0 if fault == "x1" else x1 - om * x0
    return out


def check_cfm(c, got):
    inp = cfm_inputs(c)
    x1, x0, t = inp["x1"].double(), inp["x0"].double(), inp["times"].double()[:, None]
    om = 1.0 - c.sigma
    coef = 1.0 - om * t
    w, flow = coef * x0 + t * x1, x1 - om * x0
    # 1 - sigma, * t, 1 - (.): the coefficient is off by (2 om t + |coef|) u; * x0; t * x1; the addition
    c_w = U * (x0.abs() * (2 * om * t + coef.abs()) + (coef * x0).abs() + (t * x1).abs() + w.abs())
    ck = OpsChecks(c.name)
    ck.ratio("cfm_w", "w", got["w"][: c.B], w, c_w)
    ck.ratio("cfm_flow", "flow", got["flow"][: c.B], flow, U * (2 * (om * x0).abs() + flow.abs()))
    ck.same_bits("w at t = 0 is x0", got["w"][0], inp["x0"][0])
    for k in ("w", "flow"):
        ck.sentinel_kept(k + " guard row", got[k][c.B:])
    ck.done()


AXPY_N = (4, 1028, 4 * (GRID_CAP + 3))
AXPY_IDX, AXPY_COUNTER, AXPY_SLOT = 2, 3, 1


@lru_cache(maxsize=2)
def axpy_inputs(n):
    g = _gen(("axpy", n))
    coef = torch.full((4,), NAN)
    coef[AXPY_IDX] = 0.0123
    table = torch.full((2 * AXPY_COUNTER + 2,), NAN)
    table[2 * AXPY_COUNTER + AXPY_SLOT] = -0.0456
    return dict(y=torch.randn(n, generator=g), f=torch.randn(n, generator=g), coef=coef, table=table, counter=torch.tensor([AXPY_COUNTER], dtype=I32))


def new_axpy_out(n):
    return dict(dev=flat_buf(n, F32), ctr=flat_buf(n, F32))


def standin_axpy(n):
    inp = axpy_inputs(n)
    out = new_axpy_out(n)
    out["dev"][:n] = inp["y"] + inp["f"] * inp["coef"][AXPY_IDX]
    out["ctr"][:n] = inp["y"] + inp["f"] * inp["table"][2 * AXPY_COUNTER + AXPY_SLOT]
    return out


def check_axpy(n, got):
    inp = axpy_inputs(n)
    y, f = inp["y"].double(), inp["f"].double()
    ck = OpsChecks(f"axpy-n{n}")
    for k, a in (("dev", float(inp["coef"][AXPY_IDX])), ("ctr", float(inp["table"][2 * AXPY_COUNTER + AXPY_SLOT]))):
        ref = y + f * a
        ck.ratio("axpy_" + k, k, got[k][:n], ref, U * ((f * a).abs() + ref.abs()))
        ck.sentinel_kept(k + " guard", got[k][n:])
    ck.done()


@dataclass(frozen=True)
class SelectCase:
    L: int
    B: int
    G: int
    stride: int
    slot: int
    counter: int

    @property
    def name(self):
        return f"select-L{self.L}-B{self.B}-G{self.G}-s{self.stride}-slot{self.slot}-c{self.counter}"

    @property
    def row(self):
        return self.stride * self.counter + self.slot


SELECT_CASES = [SelectCase(L, B, G, 2, 1, 3) for L in (1, 3) for B in (1, 5) for G in (4, 520)] + [SelectCase(3, 5, 520, 1, 0, 2)]


@lru_cache(maxsize=2)
def select_inputs(c):
    table = torch.full((c.row + 2, c.L, c.G), NAN)
    table[c.row] = torch.randn(c.L, c.G, generator=_gen(("select",) + astuple(c)))
    return dict(table=table, counter=torch.tensor([c.counter], dtype=I32))


def new_select_out(c):
    return dict(ada=rows_buf(c.L * c.B, c.G, F32))


def standin_select(c, fault=None):
    t = select_inputs(c)["table"]
    out = new_select_out(c)
    out["ada"][: c.L * c.B] = t[c.row - c.slot if fault == "slot" else c.row][:, None, :].expand(c.L, c.B, c.G).reshape(-1, c.G)
    return out


def check_select(c, got):
    t = select_inputs(c)["table"]
    ck = OpsChecks(c.name)
    ck.same_bits("ada is the selected row for every batch element", got["ada"][: c.L * c.B], t[c.row][:, None, :].expand(c.L, c.B, c.G).reshape(-1, c.G))
    ck.sentinel_kept("ada guard row", got["ada"][c.L * c.B:])
    ck.done()


def new_counter():
    t = torch.full((4,), -7, dtype=I32)
    t[1] = 5
    return t


def check_counter(got, inc):
    want = new_counter()
    want[1] += inc
    ck = OpsChecks(f"counter-add-{inc}")
    ck.true("the counter moved by inc, its neighbours did not", bool((got == want).all()))
    ck.done()


# ================================================================================================ G'. vbx_multi_reduce
VBX_MR_MAX = 48


@dataclass(frozen=True)
class MrJob:
    rows: int
    cols: int
    batches: int
    row_pad: int = 0  # row_stride = cols + row_pad
    b_pad: int = 0  # src_bstride = rows row_stride + b_pad
    dst_len: int = 0  # 0: cols
    d_pad: int = 0  # dst_bstride = n_dst + d_pad
    rowmap: int = 0
    F: int = 0

    @property
    def row_stride(self):
        return self.cols + self.row_pad

    @property
    def src_bstride(self):
        return self.rows * self.row_stride + self.b_pad

    @property
    def n_dst(self):
        return self.dst_len or self.cols

    @property
    def dst_bstride(self):
        return self.n_dst + self.d_pad


def _mr_jobs():
    R, Cc = (1, 15, 16, 17, 49, 64, 65, 113), (1, 63, 64, 65)  # 16 row lanes; r + 48 < rows: four rows in flight up to 48, then the tail
    out = []
    for k in range(VBX_MR_MAX - 2):
        rows, cols, nb = R[k % 8], Cc[(k // 8 + (k >= 32)) % 4], (1, 3)[(k + k // 8) % 2]
        out.append(MrJob(rows, cols, nb, (0, 5)[(k // 2) % 2], 7 * (nb > 1), cols - 1 if k % 5 == 0 and cols > 1 else 0, 3 * (nb > 1)))
    out += [MrJob(17, 128, 3, 0, 7, 120, 3, 1, 60), MrJob(113, 128, 1, 5, 0, 100, 0, 1, 60)]  # the GEGLU row map, once cut short by dst_len
    return out


MR_JOBS = _mr_jobs()
MR_SETS = {f"n1-job{k}": (k,) for k in (0, 3, 12, 13, 22, 23, 31, 46, 47)}
MR_SETS.update({f"n2-job{k}-{k + 9}": (k, k + 9) for k in (8, 17, 26, 37)})
MR_SETS["n48"] = tuple(range(VBX_MR_MAX))


@lru_cache(maxsize=64)
def mr_input(k):
    """(data [batches, rows, cols], the operand: the data at its strides inside NaN)"""
    j = MR_JOBS[k]
    x = torch.randn(j.batches, j.rows, j.cols, generator=_gen(("mr", k) + astuple(j)))
    buf = torch.full((j.batches * j.src_bstride + 8,), NAN)
    for b in range(j.batches):
        buf[b * j.src_bstride: b * j.src_bstride + j.rows * j.row_stride].view(j.rows, j.row_stride)[:, : j.cols] = x[b]
    return x, buf


def new_mr_out(k):
    j = MR_JOBS[k]
    return flat_buf(j.batches * j.dst_bstride, F32)


def _mr_dst(j):
    dst = [geglu_row_unmap(p, j.F) if j.rowmap else p for p in range(j.cols)]
    return torch.tensor([d if d < j.n_dst else -1 for d in dst])


def standin_mr(k):
    j = MR_JOBS[k]
    out, dst = new_mr_out(k), _mr_dst(j)
    s = mr_input(k)[0].sum(1)
    for b in range(j.batches):
        out[b * j.dst_bstride + dst[dst >= 0]] = s[b][dst >= 0]
    return out


def check_mr(name, ks, got):
    ck = OpsChecks("multireduce-" + name)
    for k, o in zip(ks, got):
        j = MR_JOBS[k]
        x, dst = mr_input(k)[0].double(), _mr_dst(j)
        live = dst >= 0
        idx = (torch.arange(j.batches)[:, None] * j.dst_bstride + dst[live][None, :]).reshape(-1)
        # 16 row lanes of cdiv(rows, 16) additions each, 16 additions to join them
        ck.ratio("multi_reduce", f"job {k}", o[idx].reshape(j.batches, -1), x.sum(1)[:, live], U * (cdiv(j.rows, 16) + 16) * x.abs().sum(1)[:, live])
        rest = torch.ones(o.numel(), dtype=torch.bool)
        rest[idx] = False
        ck.sentinel_kept(f"job {k}: dst outside the mapped columns", o[rest])
    ck.done()


# ================================================================================================ A. time embedding
# sinf / cosf (time_four_kernel) and expf (time_linear_kernel, silu_grad): the device library that the build machine carries states no
# ulp figures, so they were measured on MI355X through vbx_time_embed_fwd itself against fp64 (test_ops_edges_gpu.py::test_time_libm_sweep,
# profiles/ops_edges_measured.json); the terms are twice the measured values, as for the scan's sigmoid.
F_SWEEP = 32.0  # |f| <= 32 rad: times = 1, w_sin = +-(k / 4096) * 32 / (2 pi), 8192 arguments of either sign, for sin and for cos
P_SWEEP = 8.0  # |pre| <= 8 in steps of 1 / 256: w1 = 0 makes pre = b1
SINCOS_ABS_MEASURED = 5.805e-08  # 0.97 u: largest |four - sin / cos(f)| over the sweep, f the fp32 argument the kernel forms
SILU_REL_MEASURED = 1.396e-07  # 2.3 u: largest |temb - silu(pre)| / |silu(pre)| over the sweep: p / (1 + expf(-p)), the sigmoid's error and the division
A_SINCOS, RHO_SILU = 2 * SINCOS_ABS_MEASURED, 2 * SILU_REL_MEASURED
TB_SLICES = 32
PI32 = float(torch.tensor(math.pi, dtype=F32))


@dataclass(frozen=True)
class TimeCase:
    B: int
    D: int
    Th: int

    @property
    def name(self):
        return f"time-B{self.B}-D{self.D}-Th{self.Th}"


def _time_table():
    Ds, Ths, Bs = (2, 62, 64, 66, 130), (1, 3, 31, 32, 33, 65), (1, 3, 9)
    return [TimeCase(Bs[(i + j) % 3], D, Th) for i, D in enumerate(Ds) for j, Th in enumerate(Ths)]


TIME_CASES = _time_table()


@lru_cache(maxsize=2)
def time_inputs(c):
    g = _gen(("time",) + astuple(c))
    times = torch.cat([torch.tensor([1.0, 0.0, 0.7341]), torch.rand(6, generator=g)])[: c.B]
    wsin = torch.randn(c.D // 2, generator=g).clamp(-4.5, 4.5)  # up to 4.5 turns
    w1 = torch.randn(c.Th, c.D, generator=g) * c.D ** -0.5
    b1 = 0.1 * torch.randn(c.Th, generator=g)
    f = 2 * math.pi * times.double()[:, None] * wsin.double()[None, :]
    four = torch.cat([f.sin(), f.cos()], 1)
    pre = b1.double() + four @ w1.double().t()
    # the backward reads four and pre as given: the fp64 values rounded once
    return dict(times=times, wsin=wsin, w1=w1, b1=b1, four=four.float(), pre=pre.float(), dtemb=torch.randn(c.B, c.Th, generator=g))


def f_arg32(times, wsin):
    """the fp32 argument as time_four_kernel forms it: ((t w) 2) pi, three products, none of them fusable"""
    return (times[:, None] * wsin[None, :]) * 2.0 * torch.tensor(PI32)


def _silu(p):
    return p * p.sigmoid()


def _silu_grad(p):
    s = p.sigmoid()
    return s * (1 + p * (1 - s))


def time_fwd_reference(c, inp):
    """name -> (ref, counted, approx)"""
    t, ws, w1, b1 = inp["times"].double(), inp["wsin"].double(), inp["w1"].double(), inp["b1"].double()
    f = 2 * math.pi * t[:, None] * ws[None, :]
    four = torch.cat([f.sin(), f.cos()], 1)
    # f: t w, the constant pi, the product with it (x 2 is exact): 3 u of |f| through the derivative
    c_four = U * 3 * torch.cat([(f * f.cos()).abs(), (f * f.sin()).abs()], 1)
    a_four = torch.full_like(four, A_SINCOS)
    pre = b1 + four @ w1.t()
    S = four.abs() @ w1.abs().t()
    # a lane: cdiv(D, 64) products and additions; six levels of the wave tree; + b1
    c_pre = c_four @ w1.abs().t() + U * ((1 + cdiv(c.D, 64) + 6) * S + pre.abs())
    a_pre = a_four @ w1.abs().t()
    g1 = _silu_grad(pre).abs()
    temb = _silu(pre)
    return dict(four=(four, c_four, a_four), pre=(pre, c_pre, a_pre), temb=(temb, g1 * c_pre, g1 * a_pre + RHO_SILU * temb.abs()))


def time_bwd_reference(c, inp):
    t, w1 = inp["times"].double(), inp["w1"].double()
    four, pre, dtemb = inp["four"].double(), inp["pre"].double(), inp["dtemb"].double()
    B, D, Th, hd = c.B, c.D, c.Th, c.D // 2
    # silu'(p) = sg (1 + p (1 - sg)), sg = 1 / (1 + expf(-p)) with the measured relative error: 1 - sg, p (.), 1 + (.), sg (.)
    sg = pre.sigmoid()
    a_sp = (1 + pre - 2 * pre * sg).abs() * sg * RHO_SILU
    c_sp = U * (2 * (sg * pre * (1 - sg)).abs() + 2 * _silu_grad(pre).abs())
    dp = dtemb * _silu_grad(pre)
    c_dp, a_dp = dtemb.abs() * c_sp + U * dp.abs(), dtemb.abs() * a_sp
    out = {}
    out["dw1"] = (dp.t() @ four, c_dp.t() @ four.abs() + U * (1 + B) * (dp.abs().t() @ four.abs()), a_dp.t() @ four.abs())
    out["db1"] = (dp.sum(0), c_dp.sum(0) + U * B * dp.abs().sum(0), a_dp.sum(0))
    per = cdiv(Th, TB_SLICES)
    pad = TB_SLICES * per - Th

    def recs(d, w):  # [32, B, D]: the slice's own rows i
        dpp, wp = torch.cat([d, torch.zeros(B, pad, dtype=F64)], 1), torch.cat([w, torch.zeros(pad, D, dtype=F64)])
        return torch.einsum("bsi,sij->sbj", dpp.view(B, TB_SLICES, per), wp.view(TB_SLICES, per, D))

    part, Sp = recs(dp, w1), recs(dp.abs(), w1.abs())
    c_part, a_part = recs(c_dp, w1.abs()) + U * (2 + per) * Sp, recs(a_dp, w1.abs())
    out["partial"] = (part, c_part, a_part)
    dfour = part.sum(0)
    c_df, a_df = c_part.sum(0) + U * (8 + 3) * part.abs().sum(0), a_part.sum(0)  # four row lanes of 8 records, three additions to join
    out["dfour"] = (dfour, c_df, a_df)
    tw = (2 * math.pi * t)[:, None]  # t 2 (exact), the constant pi, the product
    sn, cs = four[:, :hd], four[:, hd:]
    inner = dfour[:, :hd] * cs - dfour[:, hd:] * sn
    c_in = cs.abs() * c_df[:, :hd] + sn.abs() * c_df[:, hd:] + U * ((dfour[:, :hd] * cs).abs() + (dfour[:, hd:] * sn).abs() + inner.abs())
    a_in = cs.abs() * a_df[:, :hd] + sn.abs() * a_df[:, hd:]
    out["dw_sin"] = ((tw * inner).sum(0), (tw * c_in).sum(0) + U * (3 + B) * (tw * inner).abs().sum(0), (tw * a_in).sum(0))
    return out


def time_scratch_floats(c):
    return (1 + TB_SLICES) * c.B * c.D


def new_time_out(c):
    return dict(four=rows_buf(c.B, c.D, F32), pre=rows_buf(c.B, c.Th, F32), temb=rows_buf(c.B, c.Th, F32), dw1=rows_buf(c.Th, c.D, F32),
                db1=rows_buf(1, c.Th, F32), dw_sin=rows_buf(1, c.D // 2, F32), scratch=flat_buf(time_scratch_floats(c), F32))


def standin_time(c, fault=None):
    inp = time_inputs(c)
    f = f_arg32(inp["times"], inp["wsin"])
    four = torch.cat([f.cos(), f.sin()] if fault == "swap" else [f.sin(), f.cos()], 1)
    pre = four @ inp["w1"].t() + inp["b1"]
    out = new_time_out(c)
    B, D, Th, hd = c.B, c.D, c.Th, c.D // 2
    out["four"][:B], out["pre"][:B], out["temb"][:B] = four, pre, pre / (1.0 + torch.exp(-pre))
    four, pre, w1 = inp["four"], inp["pre"], inp["w1"]
    sg = 1.0 / (1.0 + torch.exp(-pre))
    dp = inp["dtemb"] * (sg * (1.0 + pre * (1.0 - sg)))
    out["dw1"][:Th] = dp.t() @ four
    out["db1"][0] = dp[: B - 1 if fault == "db1" else B].sum(0)
    per = cdiv(Th, TB_SLICES)
    pad = TB_SLICES * per - Th
    dpp, wp = torch.cat([dp, torch.zeros(B, pad)], 1), torch.cat([w1, torch.zeros(pad, D)])
    part = torch.einsum("bsi,sij->sbj", dpp.view(B, TB_SLICES, per), wp.view(TB_SLICES, per, D))
    dfour = part.sum(0)
    out["scratch"][: B * D], out["scratch"][B * D: time_scratch_floats(c)] = dfour.reshape(-1), part.reshape(-1)
    tw = (inp["times"] * 2.0 * torch.tensor(PI32))[:, None]
    out["dw_sin"][0] = (tw * (dfour[:, :hd] * four[:, hd:] - dfour[:, hd:] * four[:, :hd])).sum(0)
    return out


def check_time(c, got):
    inp = time_inputs(c)
    B, D, Th = c.B, c.D, c.Th
    ck = OpsChecks(c.name)
    ck.true("the arguments lie inside the sweeps", float(f_arg32(inp["times"], inp["wsin"]).abs().max()) <= F_SWEEP and float(inp["pre"].abs().max()) <= P_SWEEP)
    fwd, bwd = time_fwd_reference(c, inp), time_bwd_reference(c, inp)
    for k, rows in (("four", B), ("pre", B), ("temb", B)):
        ck.ratio("time_" + k, k, got[k][:rows], *fwd[k])
        ck.sentinel_kept(k + " guard row", got[k][rows:])
    # temb against the SiLU of the pre that was stored: only the measured term and nothing else
    p = got["pre"][:B].double()
    ck.ratio("time_silu", "temb against silu(stored pre)", got["temb"][:B], _silu(p), 0.0, RHO_SILU * _silu(p).abs())
    ck.ratio("time_dw1", "dw1", got["dw1"][:Th], *bwd["dw1"])
    ck.ratio("time_db1", "db1", got["db1"][0], *bwd["db1"])
    ck.ratio("time_dw_sin", "dw_sin", got["dw_sin"][0], *bwd["dw_sin"])
    ck.ratio("time_dfour", "scratch: d(four)", got["scratch"][: B * D].reshape(B, D), *bwd["dfour"])
    ck.ratio("time_partial", "scratch: the 32 partial records", got["scratch"][B * D: time_scratch_floats(c)].reshape(TB_SLICES, B, D), *bwd["partial"])
    per = cdiv(Th, TB_SLICES)
    ck.zeros("records of the empty slices", got["scratch"][B * D:][cdiv(Th, per) * B * D: TB_SLICES * B * D])
    for k, rows in (("dw1", Th), ("db1", 1), ("dw_sin", 1)):
        ck.sentinel_kept(k + " guard row", got[k][rows:])
    ck.sentinel_kept("scratch guard", got["scratch"][time_scratch_floats(c):])
    ck.done()


def time_sweep_inputs():
    """D = 16384, B = 1, Th = 4097: four sweeps sin and cos over f = +-k / 8192 * 32 rad (the sign alternating), temb sweeps pre = b1"""
    n = 8192
    k = torch.arange(n, dtype=F64)
    wsin = ((k / n) * F_SWEEP / (2 * math.pi) * (1 - 2 * (k % 2))).float()
    b1 = -P_SWEEP + torch.arange(int(2 * P_SWEEP * 256) + 1, dtype=F32) / 256
    return dict(times=torch.ones(1), wsin=wsin, b1=b1, D=2 * n, Th=b1.numel())


def time_sweep_errors(sw, four, pre, temb):
    """(largest |four - sin / cos(f)|, largest |temb - silu(pre)| / |silu(pre)|) against fp64, f the fp32 argument"""
    f = f_arg32(sw["times"], sw["wsin"]).double()
    e_sc = float((four.double() - torch.cat([f.sin(), f.cos()], 1)).abs().max())
    p = pre.double().reshape(-1)
    nz = p != 0
    e_silu = float(((temb.double().reshape(-1) - _silu(p)).abs()[nz] / _silu(p).abs()[nz]).max())
    return e_sc, e_silu
