"""Cases, fp64 references, fp32 stand-ins and per-element bounds of the optimizer edge tests (tests/test_optim_check_cpu.py checks the
checks on the CPU, tests/test_optim_edges_gpu.py launches every case).  torch on the CPU only: nothing here touches the library or a
device.

What is checked, and why the model-level tests cannot see it: one Adam step from m = v = 0 moves every weight by lr * sign(g), so the
gradient scale, the clip coefficient, the gradient norm, beta2 and the bias corrections of step > 1 all cancel there.  Here every
kernel of the train step's optimizer runs on its own, from random m and v >= 0, at step 1, 2 and 1000, with and without a gradient
scale, and every output element is compared with fp64:

 * vbx_adam_step_packed on synthetic vbx_adam_seg tables (TABLES) that hold every form vbx_model_adam_segments and
   dp.filter_adam_segments emit, at the counts, offsets and strides that select the kernel's vector and scalar arms;
 * vbx_adam_adaln_factors and vbx_adaln_expand_dw at shapes that reach every index clamp (FACTOR_SHAPES, EXPAND_SHAPES);
 * vbx_sumsq, vbx_sumsq_ranges, vbx_sumsq_adaln_factors and vbx_clip_coef (SUMSQ_CASES, RANGES_CASES, GRAM_CASES, CLIP_CASES);
 * three steps of the whole chain on one flat buffer against clip_grad_norm_ + Adam on the materialised gradient (chain_*).

The bounds are counted, not tuned: the fp32 roundings on each output's path in csrc/ops.hip, propagated to first order in fp64, times
a margin of 2 per class (MARGIN; the count stands beside each term below).  u = 2^-24; divide and sqrtf are correctly rounded (the
library is built without fast-math flags) and contraction into fma only removes roundings.  Beside the bounds stand the rules that take
no tolerance: g = m = v = 0 leaves p, 0, 0; every bf16 / fp16 / fp32 operand copy is bit-equal to round-to-nearest-even of the fp32 p
the device stored; every element no segment maps keeps its sentinel bits (gaps, columns cols .. dst_ld, rows the GEGLU map pads, a
guard row behind every buffer).
"""
import json
import math
import os
import zlib
from dataclasses import dataclass
from functools import lru_cache

import torch

from attn_check import Checks, worst_tile
from gemm_check import SENTINEL

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
ADAM_BLOCK = 2048  # floats per block of vbx_adam_step_packed: 256 threads x 4 floats x 2 iterations
GUARD = 64  # floats behind every flat buffer


def f32(x):
    return float(torch.tensor(x, dtype=F32))


# the hyper-parameters as the C ABI receives them (float arguments): the references start from these exactly converted values
LR, B1, B2, EPS = f32(1e-3), f32(0.9), f32(0.99), f32(1e-8)
STEPS = (1, 2, 1000)
GSCALES = (None, f32(0.37))  # gscale NULL, and a device scalar

# margin over the counted bound per class (as gemm_check.LINEAR_FACTOR).  The comment holds the worst error / (margin x counted bound)
# measured on MI355X over all cases of tests/test_optim_edges_gpu.py (profiles/optim_edges_measured.json).  (The Adam classes sit just
# under 0.5, that is at the counted bound itself: the dominant terms of m, v and p count two or three roundings, and among 10^4
# elements one meets them all with the same sign at the bottom of a binade -- the fp32 stand-in gives the same worst figures.  The
# sums and the clip coefficient show how little of a worst-case count a tree of a few levels uses.)
MARGIN = dict(
    adam_p=2,  # 0.496
    adam_m=2,  # 0.468
    adam_v=2,  # 0.483
    factor_p=2,  # 0.494
    factor_m=2,  # 0.447
    factor_v=2,  # 0.488
    expand_dw=2,  # 0.369
    sumsq=2,  # 0.0133
    sumsq_ranges=2,  # 0.0484
    gram=2,  # 0.0776
    gram_sum=2,  # 0.0467
    clip_coef=2,  # 0.0648
    clip_norm=2,  # 0.134
)
# roundings counted in csrc/ops.hip
N_GR = 1  # adam_one: gr = gv * gs
N_M_OLD, N_M_NEW = 2, 3  # b1 * m, +   |   (1 - b1), * gr, +
N_V_OLD, N_V_NEW = 2, 4  # b2 * v, +   |   (1 - b2), * gr, * gr, +      (gr's own rounding enters twice through d(gr))
N_UPD = 2  # lr_bc1 * m, then / denominator
N_SQRT = 2  # sqrtf(v), / bc2_sqrt
N_POW = 2  # host powf(beta, step): one ulp = 2 u
N_TREE = 16  # levels of the trees behind the per-lane accumulators of the sums, as the (k + 16) u bound of the sums counts them
N_CLIP_NORM = 2  # clip_coef_kernel: sqrtf, * inv_world
N_CLIP_COEF = N_CLIP_NORM + 4  # ... + 1e-6f (the addition, and the constant's own conversion to fp32), /, * inv_world


# ------------------------------------------------------------------------------------------------ small helpers
def sentinel(n, dtype):
    it, val = SENTINEL[dtype]
    return torch.full((n,), val, dtype=it).view(dtype)


def bits(t):
    return t.contiguous().view(SENTINEL[t.dtype][0])


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ratios(got, ref, bound):
    """|got - ref| / bound per element; where the bound is 0 the result must be exact (0, inf otherwise).  NaN propagates."""
    err = (got.double() - ref.double()).abs()
    bound = bound.double().expand_as(err) if torch.is_tensor(bound) else torch.full_like(err, bound)
    r = err / bound.clamp(min=1e-300)
    r = torch.where(bound == 0, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)), r)
    return torch.where(torch.isnan(err), torch.full_like(err, math.nan), r)


class OptimChecks(Checks):
    """attn_check.Checks with the log of these tests: OPTIM_CHECK_LOG=<file> appends one JSON line per case with every measured value
    (how profiles/optim_edges_measured.json and the figures beside MARGIN were made)."""

    def ratio(self, cls, name, got, ref, bound):
        w, idx = worst_tile(ratios(got, ref, MARGIN[cls] * bound).reshape(-1))
        self.le(f"{name} [{cls}] error / bound at {idx}", w, 1.0)

    def done(self):
        if os.environ.get("OPTIM_CHECK_LOG"):
            with open(os.environ["OPTIM_CHECK_LOG"], "a") as f:
                f.write(json.dumps({"case": self.case, "values": [(n, v if isinstance(v, bool) else float(v), b) for n, v, b in self.seen]}) + "\n")
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)


# ------------------------------------------------------------------------------------------------ Adam: reference, stand-in, bound
def _bc_rel(beta, step):
    """relative error of the host's fp32 bc = 1.0f - powf(beta, step): the power's ulp amplified by the cancellation, and the
    subtraction's own rounding"""
    pw = beta ** step
    return N_POW * U * pw / (1.0 - pw) + U


def adam_reference(p, g, m, v, gs, step, dg=0.0, dgs=0.0):
    """torch.optim.Adam as include/vbx.h states it, in fp64, and the first-order bound of a correct fp32 kernel per element.
    p, g, m, v: fp64 tensors (the exactly converted fp32 inputs; g may be an fp64 product with its own absolute error dg);
    gs: gradient scale (None: 1) with absolute error dgs.  Returns (p', m', v', bound_p, bound_m, bound_v)."""
    gs = 1.0 if gs is None else float(gs)
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    gr = g * gs
    m1 = B1 * m + (1.0 - B1) * gr
    v1 = B2 * v + (1.0 - B2) * gr * gr
    a, s = LR / bc1, math.sqrt(bc2)
    q = v1.sqrt() / s
    D = q + EPS
    upd = a * m1 / D
    p1 = p - upd
    dgr = abs(gs) * dg + g.abs() * dgs + N_GR * U * gr.abs()
    dm = U * (N_M_OLD * (B1 * m).abs() + N_M_NEW * ((1.0 - B1) * gr).abs()) + (1.0 - B1) * dgr
    dv = U * (N_V_OLD * B2 * v + N_V_NEW * (1.0 - B2) * gr * gr) + (1.0 - B2) * (2 * gr.abs() * dgr + dgr * dgr)
    rel_a = _bc_rel(B1, step) + U  # host: lr / bc1
    rel_s = _bc_rel(B2, step) / 2 + U  # host: sqrtf(bc2)
    dsq = torch.where(v1 > 0, dv / (2 * v1.sqrt().clamp(min=1e-300)), dv.sqrt())  # dv pushed through the square root
    dD = dsq / s + q * (N_SQRT * U + rel_s) + U * D  # ... the division by bc2_sqrt, and the addition of eps
    dupd = a * dm / D + upd.abs() * (rel_a + N_UPD * U) + upd.abs() * dD / D
    dp = U * p1.abs() + dupd  # the subtraction's rounding, and the update's error
    return p1, m1, v1, dp, dm, dv + 2.0 ** -149


def adam_standin(p, g, m, v, gs, step, fault=None):
    """The same arithmetic in torch float32, host scalars included: what a correct kernel may answer."""
    one = torch.tensor(1.0)
    lr, b1, b2, eps = (torch.tensor(x, dtype=F32) for x in (LR, B1, B2, EPS))
    st = torch.tensor(float(step))
    bc1 = one - torch.pow(b1, st)
    bc2 = one - torch.pow(b1 if fault == "bc2" else b2, st)
    lr_bc1, bc2s = lr / bc1, torch.sqrt(bc2)
    gsv = torch.tensor(1.0 if gs is None or fault == "gscale" else gs, dtype=F32)
    gr = g * gsv
    m1 = b1 * m + (one - b1) * gr
    v1 = b2 * v + (one - b2) * gr * gr
    return p - lr_bc1 * m1 / (torch.sqrt(v1) / bc2s + eps), m1, v1


# ------------------------------------------------------------------------------------------------ A. vbx_adam_step_packed: tables
KINDS = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SEG_FIELDS = ("off", "count", "dst_bf16", "dst_f16", "dst_f32", "cols", "dst_ld", "rowmap", "F", "block0")


def dest_row(r, rowmap, F):
    """Python restatement of vbx_pack_weight's GEGLU row interleave (rowmap = 1): per 128 destination rows, 64 rows of the first half
    [0, F) and then 64 rows of the second half [F, 2 F)."""
    if rowmap != 1:
        return r
    half, q = (0, r) if r < F else (1, r - F)
    return (q // 64) * 128 + half * 64 + q % 64


def number_blocks(segs):
    """block0 and the launch's block count as vbx_model_adam_segments numbers them: 2048 floats per block, a rowmap == 2 entry (an
    adaLN weight block that stays in factor form) takes none."""
    blocks = 0
    for s in segs:
        s["block0"] = blocks
        blocks += 0 if s["rowmap"] == 2 else (s["count"] + ADAM_BLOCK - 1) // ADAM_BLOCK
    return blocks


class Table:
    """A vbx_adam_seg table and its destination buffers.  Destination pointers are VIRTUAL addresses (0 = NULL) inside `bufs`
    (name -> (dtype, elements with the guard row, virtual base)), so that dp.filter_adam_segments can move them as it moves real ones;
    the GPU test maps them onto device buffers with `resolve`."""

    def __init__(self, name):
        self.name, self.segs, self.bufs, self.cur, self._va, self.n, self.total_blocks = name, [], {}, 0, 1 << 20, 0, 0

    def gap(self, n):
        self.cur += n

    def align(self, a=4):
        self.cur = -(-self.cur // a) * a

    def seg(self, rows, cols, ld=0, kinds=(), rowmap=0, F=0):
        s = dict(off=self.cur, count=rows * cols, dst_bf16=0, dst_f16=0, dst_f32=0, cols=cols, dst_ld=ld, rowmap=rowmap, F=F, block0=0)
        drows = -(-F // 64) * 128 if rowmap == 1 else rows
        for k in kinds:
            numel = (drows + 1) * ld
            self.bufs[f"s{len(self.segs)}.{k}"] = (KINDS[k], numel, self._va)
            s["dst_" + k] = self._va
            self._va += -(-numel * 4 // 4096) * 4096 + 4096
        self.segs.append(s)
        self.cur += rows * cols
        return s

    def plain(self, count):  # the form of the builder's filler segments: cols = 1, no destination
        return self.seg(count, 1)

    def factor_marker(self, rows, cols):  # an adaLN weight block in factor mode: fp16 destination set, rowmap 2, no blocks
        return self.seg(rows, cols, cols, ("f16",), rowmap=2)

    def finish(self, frozen=()):
        if frozen:
            from voicebox_pytorch_amd.dp import filter_adam_segments

            self.segs, _ = filter_adam_segments(self.segs, list(frozen))
        self.total_blocks = number_blocks(self.segs)
        self.n = self.cur
        return self

    def resolve(self, addr):
        for name, (dt, numel, vb) in self.bufs.items():
            es = torch.empty(0, dtype=dt).element_size()
            if vb <= addr < vb + numel * es:
                assert (addr - vb) % es == 0
                return name, (addr - vb) // es
        raise KeyError(addr)

    def covered(self):
        c = torch.zeros(self.n + GUARD, dtype=torch.bool)
        for s in self.segs:
            if s["rowmap"] != 2:
                assert not c[s["off"]: s["off"] + s["count"]].any(), "segments overlap"
                c[s["off"]: s["off"] + s["count"]] = True
        return c

    def dst_map(self, fault=None):
        """{buffer: flat index each destination element copies, -1 where no segment maps}; asserts that no element is mapped twice
        and that the guard row stays free.  fault "rowmap": the first row of a row-mapped segment's second half lands one row late."""
        maps = {name: torch.full((numel,), -1, dtype=torch.long) for name, (_, numel, _) in self.bufs.items()}
        for s in self.segs:
            if s["rowmap"] == 2:
                continue
            if not (s["dst_bf16"] or s["dst_f16"] or s["dst_f32"]):
                continue
            j = torch.arange(s["count"])
            r, c = j // s["cols"], j % s["cols"]
            dr = torch.tensor([dest_row(int(x), s["rowmap"], s["F"]) for x in range(s["count"] // s["cols"])], dtype=torch.long)
            if fault == "rowmap" and s["rowmap"] == 1:
                dr[s["F"]] += 1
            for k in KINDS:
                if s["dst_" + k]:
                    name, base = self.resolve(s["dst_" + k])
                    pos = base + dr[r] * s["dst_ld"] + c
                    if fault is None:
                        assert int(pos.max()) < maps[name].numel() - s["dst_ld"] and bool((maps[name][pos] == -1).all()), (self.name, name)
                    maps[name][pos] = s["off"] + j
        return maps


def _table_edges():
    """The kernel's own edges: ragged counts, the vector arm's three conditions one at a time, every combination of copies, gaps."""
    t = Table("edges")
    t.plain(2 * ADAM_BLOCK + 1)  # a ragged last group, and a block that owns one element
    t.align()  # (a gap of 3)
    t.plain(1024)  # the second iteration breaks at once
    t.plain(1028)
    t.gap(1)
    assert t.cur % 2 == 1
    t.plain(7)  # odd offset: the whole segment on the scalar arm
    t.factor_marker(8, 8)  # a zero-block entry in the middle
    t.align()
    t.seg(5, 12, 16, ("bf16", "f16"))  # vector arm, both copies
    t.seg(5, 10, 12, ("bf16", "f16"))  # cols % 4 != 0
    t.align()
    t.seg(5, 8, 10, ("bf16", "f16"))  # dst_ld % 4 != 0
    t.seg(5, 12, 12, ("bf16",))
    t.seg(5, 12, 16, ("f16",))
    t.gap(8)
    t.seg(1, 37, 37, ("f32",))  # a bias: cols = count = 37
    t.align(64)
    row = t.seg(1, 41, 41, ("f32",))  # a one-row block that dp.filter_adam_segments cuts below: [0, 3) and [21, 41), the second at
    frozen = [(row["off"] + 3, row["off"] + 21)]  # an odd offset with a shifted destination and cols = 20
    t.gap(5)
    t.plain(5)
    t.factor_marker(4, 4)  # a zero-block entry at the end
    return t.finish(frozen)


def _table_forms():
    """Every form vbx_model_adam_segments emits, in a model's order, at toy sizes (D = 8, F = 70, Fp = 128, Th = 8, Lc = 6, Kp = 8)."""
    t = Table("forms")
    F = 70
    t.seg(8, 24, 24, ("bf16", "f16"))  # conv embed / prediction head: both copies, dst_ld = cols
    t.seg(8, 6, 8, ("f16",))  # proj_in: fp16 only, K padded
    t.plain(40)  # a filler between parameter slots
    t.seg(32, 8, 8, ("f16",))  # adaLN weights, materialised mode
    t.seg(1, 32, 32, ("f32",))  # adaLN biases: one row
    t.seg(24, 8, 8, ("bf16", "f16"))  # to_qkv
    t.seg(2 * F, 8, 8, ("bf16", "f16"), rowmap=1, F=F)  # FeedForward[0].weight: 256 destination rows
    t.seg(2 * F, 1, 1, ("f32",), rowmap=1, F=F)  # FeedForward[0].bias: one column, row-mapped
    t.gap(4)
    t.seg(8, F, 128, ("bf16", "f16"))  # FeedForward[2].weight: cols = F, dst_ld = Fp (scalar arm: 70 % 4)
    t.seg(8, 72, 128, ("bf16", "f16"))  # ... at an F that is a multiple of 4: the vector arm with dst_ld > cols
    t.factor_marker(32, 8)  # adaLN weights, factor mode: in the middle
    t.seg(2 * F, 20, 24, ("bf16", "f16"), rowmap=1, F=F)  # a row-mapped matrix of two blocks on the vector arm
    t.plain(3)
    t.factor_marker(32, 8)  # ... and at the end
    t.gap(6)
    return t.finish()


TABLES = {t.name: t for t in (_table_edges(), _table_forms())}


@dataclass(frozen=True)
class PackedCase:
    table: str
    step: int
    gs: object  # None or the device scalar

    @property
    def name(self):
        return f"packed-{self.table}-step{self.step}-{'gs' if self.gs else 'nogs'}"


PACKED_CASES = [PackedCase(t, s, g) for t in TABLES for s in STEPS for g in GSCALES]


def flat_inputs(key, n, covered):
    """p, g, m, v of n + GUARD floats: weights of order 1/2, gradients of order 0.1, v >= 0; exact zeros planted (every 11th element
    g = m = v = 0 -- Adam never meets v = 0 with m != 0 --, the next v = 0, the next g = 0); outside `covered` p / m / v hold the
    sentinel and g is NaN."""
    gen = _gen(key)
    N = n + GUARD
    p, g, m = (torch.randn(N, generator=gen) * s for s in (0.5, 0.1, 0.05))
    v = (torch.randn(N, generator=gen) * 0.1) ** 2
    i = torch.arange(N) % 11
    g[(i == 0) | (i == 2)] = 0
    m[i == 0] = 0
    v[(i == 0) | (i == 1)] = 0
    out = dict(p=p, g=g, m=m, v=v)
    for k in "pmv":
        out[k] = torch.where(covered, out[k], sentinel(N, F32))
    out["g"] = torch.where(covered, g, torch.full_like(g, math.nan))
    return out


@lru_cache(maxsize=4)
def packed_inputs(case):
    t = TABLES[case.table]
    return flat_inputs(("packed", case.table, case.step, case.gs), t.n, t.covered())


def new_dst(table):
    return {name: sentinel(numel, dt) for name, (dt, numel, _) in table.bufs.items()}


def truncate_bf16(x):
    return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


def standin_packed_state(table, inp, gs, step, fault=None):
    """{p, m, v, destination buffers} as a correct launch leaves them (fault: one of the planted faults)."""
    cov = table.covered()
    p1, m1, v1 = adam_standin(inp["p"], inp["g"], inp["m"], inp["v"], gs, step, fault)
    if fault == "tail":  # the last element of every ragged tail left as it was
        for s in table.segs:
            if s["rowmap"] != 2 and s["count"] % 4:
                cov[s["off"] + s["count"] - 1] = False
    out = {k: torch.where(cov, x, inp[k]) for k, x in (("p", p1), ("m", m1), ("v", v1))}
    if fault == "gap":
        out["p"][int((~table.covered()[: table.n]).nonzero()[0])] = 0.0
    for name, mp in table.dst_map(fault).items():
        dt = table.bufs[name][0]
        src = out["p"][mp.clamp(min=0)]
        val = truncate_bf16(src) if fault == "trunc" and dt == torch.bfloat16 else src.to(dt)
        out[name] = torch.where(mp >= 0, val, sentinel(mp.numel(), dt))
    return out


def check_untouched(ck, inp, got, covered):
    for k in "pmv":
        ck.true(f"{k} outside every segment keeps its bits", bool((bits(got[k])[~covered] == bits(inp[k])[~covered]).all()))


def check_packed_state(ck, table, inp, got, gs, step, dgs=0.0, cls="adam"):
    """vbx_adam_step_packed's outputs on `table` from the state `inp`: bounds on p / m / v where a segment maps, the exactness rules."""
    cov = table.covered()
    d = {k: inp[k][cov].double() for k in "pgmv"}
    p1, m1, v1, bp, bm, bv = adam_reference(d["p"], d["g"], d["m"], d["v"], gs, step, dgs=dgs)
    for k, ref, b in (("p", p1, bp), ("m", m1, bm), ("v", v1, bv)):
        ck.true(f"{k} finite", bool(torch.isfinite(got[k][cov]).all()))
        ck.ratio(f"{cls}_{k}", k, got[k][cov], ref, b)
    z = cov & (inp["g"] == 0) & (inp["m"] == 0) & (inp["v"] == 0)
    ck.true("g = m = v = 0 leaves p, 0, 0", bool((bits(got["p"])[z] == bits(inp["p"])[z]).all())
            and bool((got["m"][z] == 0).all()) and bool((got["v"][z] == 0).all()))
    for name, mp in table.dst_map().items():
        dt = table.bufs[name][0]
        want = torch.where(mp >= 0, got["p"][mp.clamp(min=0)].to(dt), sentinel(mp.numel(), dt))
        on = mp >= 0
        ck.true(f"{name} is round-to-nearest-even of the stored p", bool((bits(got[name])[on] == bits(want)[on]).all()))
        ck.true(f"{name} sentinel untouched", bool((bits(got[name])[~on] == bits(want)[~on]).all()))


def check_packed(case, got):
    t, inp = TABLES[case.table], packed_inputs(case)
    ck = OptimChecks(case.name)
    check_untouched(ck, inp, got, t.covered())
    check_packed_state(ck, t, inp, got, case.gs, case.step)
    ck.done()


def standin_packed(case, fault=None):
    return standin_packed_state(TABLES[case.table], packed_inputs(case), case.gs, case.step, fault)


# ------------------------------------------------------------------------------------------------ B. vbx_adam_adaln_factors
# (L, B, J4, Th): 8 rows x 1024 columns per block, groups of 4 rows in flight, batch passes of 8
FACTOR_SHAPES = [(1, 1, 1, 4), (2, 3, 13, 1028), (3, 9, 8, 260), (2, 8, 20, 1024), (1, 17, 9, 8)]


@dataclass(frozen=True)
class FactorCase:
    L: int
    B: int
    J4: int
    Th: int
    step: int
    gs: object
    dst: str  # fp16 copies: "all", "none" (the pointer array is NULL), "one" (NULL for layer 0 only)

    @property
    def name(self):
        return f"factor-L{self.L}-B{self.B}-J{self.J4}-Th{self.Th}-step{self.step}-{'gs' if self.gs else 'nogs'}-dst_{self.dst}"


FACTOR_CASES = [FactorCase(*sh, s, g, ("all", "none", "one")[(i + j + k) % 3])
                for i, sh in enumerate(FACTOR_SHAPES) for j, s in enumerate(STEPS) for k, g in enumerate(GSCALES)]


def factor_layout(L, J4, Th, dst="all", start=8):
    """Weight blocks out of order with gaps: layer L - 1 first; every offset a multiple of 4 floats (the entry point's contract)."""
    w_off, cur = [0] * L, start
    for l in reversed(range(L)):
        w_off[l] = cur
        cur += J4 * Th + 4 * (l + 1)
    has = [dst == "all" or (dst == "one" and l > 0) for l in range(L)]
    return dict(L=L, J4=J4, Th=Th, w_off=w_off, n=cur, has_dst=has, dst_array=dst != "none")


def factor_covered(lay):
    c = torch.zeros(lay["n"] + GUARD, dtype=torch.bool)
    for o in lay["w_off"]:
        assert not c[o: o + lay["J4"] * lay["Th"]].any()
        c[o: o + lay["J4"] * lay["Th"]] = True
    return c


def factor_operands(key, L, B, J4, Th):
    """dada [L, B, J4] and temb [B, Th], each behind 4 floats of NaN and in front of a NaN row: (buffer, element offset)"""
    gen = _gen(key)
    dada, temb = torch.randn(L, B, J4, generator=gen) * 0.1, torch.randn(B, Th, generator=gen)
    return dada, temb


def embed_nan(x):
    """x flat behind 16 bytes of NaN and in front of 64 NaN floats: (buffer, element offset of the base)"""
    buf = torch.full((4 + x.numel() + 64,), math.nan, dtype=x.dtype)
    buf[4: 4 + x.numel()] = x.reshape(-1)
    return buf, 4


@lru_cache(maxsize=4)
def factor_inputs(case):
    lay = factor_layout(case.L, case.J4, case.Th, case.dst)
    key = ("factor", case.L, case.B, case.J4, case.Th, case.step, case.gs)
    inp = flat_inputs(key, lay["n"], factor_covered(lay))
    inp["dada"], inp["temb"] = factor_operands(key, case.L, case.B, case.J4, case.Th)
    return lay, inp


def factor_gradient(dada, temb):
    """fp64 dada_l^T . temb [L, J4, Th] and its bound gamma_B sum_b |dada[b, j] temb[b, c]|: B products and B - 1 additions per element"""
    g = torch.einsum("lbj,bt->ljt", dada.double(), temb.double())
    S = torch.einsum("lbj,bt->ljt", dada.double().abs(), temb.double().abs())
    return g, dada.shape[1] * U * S


def new_factor_dst(lay):
    return {f"f16.{l}": sentinel((lay["J4"] + 1) * lay["Th"], torch.float16) for l in range(lay["L"]) if lay["has_dst"][l] and lay["dst_array"]}


def standin_factor_state(lay, inp, gs, step, fault=None):
    dada, temb = inp["dada"], inp["temb"]
    if fault == "lastb" and dada.shape[1] % 8:  # the last batch row dropped when B is no multiple of the pass
        dada, temb = dada[:, :-1], temb[:-1]
    out = {k: inp[k].clone() for k in "pmv"}
    out.update(new_factor_dst(lay))
    for l, o in enumerate(lay["w_off"]):
        sl = slice(o, o + lay["J4"] * lay["Th"])
        g = (dada[l].t().contiguous() @ temb).reshape(-1)
        out["p"][sl], out["m"][sl], out["v"][sl] = adam_standin(inp["p"][sl], g, inp["m"][sl], inp["v"][sl], gs, step, fault)
        if f"f16.{l}" in out:
            out[f"f16.{l}"][: lay["J4"] * lay["Th"]] = out["p"][sl].half()
    return out


def check_factor_state(ck, lay, inp, got, gs, step, dgs=0.0):
    g, dg = factor_gradient(inp["dada"], inp["temb"])
    n = lay["J4"] * lay["Th"]
    for l, o in enumerate(lay["w_off"]):
        sl = slice(o, o + n)
        p1, m1, v1, bp, bm, bv = adam_reference(inp["p"][sl].double(), g[l].reshape(-1), inp["m"][sl].double(), inp["v"][sl].double(), gs,
                                                step, dg=dg[l].reshape(-1), dgs=dgs)
        for k, ref, b in (("p", p1, bp), ("m", m1, bm), ("v", v1, bv)):
            ck.true(f"layer {l} {k} finite", bool(torch.isfinite(got[k][sl]).all()))
            ck.ratio(f"factor_{k}", f"layer {l} {k}", got[k][sl], ref, b)
        if f"f16.{l}" in got:
            buf = got[f"f16.{l}"]
            ck.true(f"layer {l} fp16 copy is round-to-nearest-even of the stored p", bool((bits(buf[:n]) == bits(got["p"][sl].half())).all()))
            ck.true(f"layer {l} fp16 guard row untouched", bool((bits(buf[n:]) == SENTINEL[torch.float16][1]).all()))


def check_factor(case, got):
    lay, inp = factor_inputs(case)
    ck = OptimChecks(case.name)
    check_untouched(ck, inp, got, factor_covered(lay))
    ck.true("a copy for every layer that has a destination", set(new_factor_dst(lay)) <= set(got))
    check_factor_state(ck, lay, inp, got, case.gs, case.step)
    ck.done()


def standin_factor(case, fault=None):
    lay, inp = factor_inputs(case)
    return standin_factor_state(lay, inp, case.gs, case.step, fault)


# ------------------------------------------------------------------------------------------------ C. vbx_adaln_expand_dw
# (B, J4, Th): 4 rows x 1024 columns per block, any B -- the shapes of B, then B = 70 and J4 = 6
EXPAND_SHAPES = [(B, J4, Th) for _, B, J4, Th in FACTOR_SHAPES] + [(70, 6, 260)]


def expand_name(sh):
    return "expand-B%d-J%d-Th%d" % sh


@lru_cache(maxsize=2)
def expand_inputs(sh):
    B, J4, Th = sh
    dada, temb = factor_operands(("expand",) + sh, 1, B, J4, Th)
    return dada, temb


def new_expand_dst(sh):
    return sentinel((sh[1] + 1) * sh[2], F32)


def standin_expand(sh, fault=None):
    dada, temb = expand_inputs(sh)
    if fault == "lastb" and sh[0] % 8:
        dada, temb = dada[:, :-1], temb[:-1]
    out = new_expand_dst(sh)
    out[: sh[1] * sh[2]] = (dada[0].t().contiguous() @ temb).reshape(-1)
    return out


def check_expand(sh, dw):
    B, J4, Th = sh
    ck = OptimChecks(expand_name(sh))
    g, dg = factor_gradient(*expand_inputs(sh))
    ck.true("dw finite", bool(torch.isfinite(dw[: J4 * Th]).all()))
    ck.ratio("expand_dw", "dw", dw[: J4 * Th], g.reshape(-1), dg.reshape(-1))
    ck.true("dw guard row untouched", bool((bits(dw[J4 * Th:]) == SENTINEL[F32][1]).all()))
    ck.done()


# ------------------------------------------------------------------------------------------------ D. the norm
def cdiv(a, b):
    return -(-a // b)


def grid_for(n, cap):  # csrc/ops.hip
    return max(1, min(cap, cdiv(n, 256)))


def sum_bound(k, S):
    """(k + 16) u S: a sum of fp32 terms of total magnitude S (non-negative terms: relative), k the largest number of terms any one
    accumulator takes, 16 for the levels of the trees behind the accumulators.  (Counted level by level the two stages have up to
    2 + 6 + 3 and 6 + 4 behind their accumulators; rounding errors of that many levels do not all add up, and the bound is kept at the
    tighter 16: the measured use is a few per cent of it.)"""
    return (k + N_TREE) * U * S


# vbx_sumsq: (n, element offset of the base inside a 16-byte aligned tensor).  4 * 256 * 1024 + 3 is over the 1024-block cap: the
# grid-stride loop and the scalar tail both run; offset 1 is the scalar arm
SUMSQ_CASES = [(1, 0), (5, 0), (1024, 0), (4 * 256 * 1024 + 3, 0), (1031, 1)]


def sumsq_k(n, off):
    nb = grid_for(n, 1024)
    T = nb * 256
    n4 = n // 4 if off % 4 == 0 else 0
    return max(cdiv(n4, T) + cdiv(n - 4 * n4, T), cdiv(nb, 256))


@lru_cache(maxsize=2)
def sumsq_input(n, off):
    x = torch.full((off + n + 8,), math.nan)
    x[off: off + n] = torch.randn(n, generator=_gen(("sumsq", n, off))) * 0.5
    return x


def standin_sumsq(n, off):
    x = sumsq_input(n, off)[off: off + n]
    return (x * x).sum()


def check_sumsq(n, off, out, out2=None):
    ck = OptimChecks(f"sumsq-n{n}-off{off}")
    ref = sumsq_input(n, off)[off: off + n].double().pow(2).sum()
    ck.ratio("sumsq", "sum", out.reshape(1), ref.reshape(1), sum_bound(sumsq_k(n, off), ref).reshape(1))
    if out2 is not None:
        ck.true("a second run gives the same bits", bool((bits(out.reshape(1)) == bits(out2.reshape(1))).all()))
    ck.done()


@dataclass(frozen=True)
class RangesCase:
    name: str
    ranges: tuple  # ((lo, hi), ...), multiples of 4 floats
    n_extra: int

    @property
    def size(self):
        return max(hi for _, hi in self.ranges) + 8


def _ranges_table():
    lay = {
        "one": ((8, 4008),),
        "r64": tuple((100 * i, 100 * i + 4 * (1 + i % 9)) for i in range(64)),  # 64 ranges of 4 .. 36 floats
        "empties": ((0, 0), (16, 216), (300, 300), (300, 300), (400, 1000), (1200, 1200)),  # empty first, in the middle (twice), last
        "fours": tuple((8 * i, 8 * i + 4) for i in range(64)),  # one float4 each: lane i walks past i ranges at once
        "short-many": tuple((16 * i + 4, 16 * i + 12) for i in range(40)) + ((1000, 3000),),
        "across": ((4, 4 + 1048000),),  # one range over all 1024 chunks (4 MB)
        "under256": ((4, 104), (200, 400), (512, 612)),  # 100 float4s
    }
    out = [RangesCase(f"ranges-{k}-x0", r, 0) for k, r in lay.items()]
    # the extra terms behind the block partials: none, one, the edges of a 1024-thread pass, and of the i + 3072 < nb unroll
    out += [RangesCase(f"ranges-empties-x{e}", lay["empties"], e) for e in (1, 1023, 1025, 4097, 5000)]
    out += [RangesCase("ranges-r64-x4097", lay["r64"], 4097)]
    return out


RANGES_CASES = _ranges_table()


def ranges_k(case):
    n4 = sum(hi - lo for lo, hi in case.ranges) // 4
    nb = grid_for(n4 * 4, 1024)
    per = cdiv(n4, nb)
    return max(cdiv(per, 256), cdiv(nb, 1024) + cdiv(case.n_extra, 1024))


@lru_cache(maxsize=2)
def ranges_input(case):
    """(x: NaN everywhere outside the ranges, scratch [1024 + n_extra + 8]: the extra terms at 1024 .., NaN behind them)"""
    gen = _gen(("ranges", case.name))
    x = torch.full((case.size,), math.nan)
    for lo, hi in case.ranges:
        x[lo:hi] = torch.randn(hi - lo, generator=gen) * 0.5
    scratch = torch.full((1024 + case.n_extra + 8,), math.nan)
    scratch[:1024] = 0
    scratch[1024: 1024 + case.n_extra] = torch.rand(case.n_extra, generator=gen) + 0.01
    return x, scratch


def standin_ranges(case, fault=None):
    x, scratch = ranges_input(case)
    rs = [r for r in case.ranges if r[1] > r[0]]
    parts = [(x[lo: hi - 4 if fault == "float4" and (lo, hi) == rs[-1] else hi] ** 2).sum() for lo, hi in rs]
    ex = scratch[1024: 1024 + case.n_extra]
    if fault == "extra":
        ex = ex[:-1]
    return torch.stack(parts).sum() + ex.sum()


def check_ranges(case, out, out2=None):
    x, scratch = ranges_input(case)
    ck = OptimChecks(case.name)
    ref = sum(x[lo:hi].double().pow(2).sum() for lo, hi in case.ranges) + scratch[1024: 1024 + case.n_extra].double().sum()
    ck.ratio("sumsq_ranges", "sum", out.reshape(1), ref.reshape(1), sum_bound(ranges_k(case), ref).reshape(1))
    if out2 is not None:
        ck.true("a second run gives the same bits", bool((bits(out.reshape(1)) == bits(out2.reshape(1))).all()))
    ck.done()


# vbx_sumsq_adaln_factors: (L, B, J4, Th)
GRAM_CASES = [(2, B, J4, Th) for B in (1, 3, 64) for J4 in (1, 255, 257, 520) for Th in (4, 260)]


def gram_name(sh):
    return "gram-L%d-B%d-J%d-Th%d" % sh


@lru_cache(maxsize=2)
def gram_inputs(sh):
    L, B, J4, Th = sh
    return factor_operands(("gram",) + sh, L, B, J4, Th)


def gram_reference(dada, temb):
    """The L B B terms (dada_l[b] . dada_l[b']) (temb[b] . temb[b']) in fp64 and their bounds.  Each dot product: one accumulator per
    lane of 256 (ceil(n / 256) products, each rounded, and as many additions), 6 levels of the wave sum, 3 of the sum over the waves;
    then the product of the two: ((kJ + 10) + (kT + 10) + 1) u |.|.|.| to first order."""
    da, te = dada.double(), temb.double()
    g1, g2 = torch.einsum("lbj,lcj->lbc", da, da), te @ te.t()
    s1, s2 = torch.einsum("lbj,lcj->lbc", da.abs(), da.abs()), te.abs() @ te.abs().t()
    k = cdiv(dada.shape[2], 256) + cdiv(temb.shape[1], 256)
    return g1 * g2, (k + 21) * U * s1 * s2


def standin_gram(dada, temb):
    return torch.einsum("lbj,lcj->lbc", dada, dada) * (temb @ temb.t())


def check_gram_terms(ck, dada, temb, terms):
    ref, bound = gram_reference(dada, temb)
    terms = terms.reshape(ref.shape)
    ck.true("terms finite", bool(torch.isfinite(terms).all()))
    ck.ratio("gram", "term", terms, ref, bound)
    g, _ = factor_gradient(dada, temb)
    ck.ratio("gram_sum", "sum over (b, b') against |dada^T temb|_F^2", terms.double().sum(dim=(1, 2)), g.pow(2).sum(dim=(1, 2)), bound.sum(dim=(1, 2)))


def check_gram(sh, terms, terms2=None):
    ck = OptimChecks(gram_name(sh))
    check_gram_terms(ck, *gram_inputs(sh), terms)
    if terms2 is not None:
        ck.true("a second run gives the same bits", bool((bits(terms) == bits(terms2)).all()))
    ck.done()


# vbx_clip_coef: (sumsq, max_norm, inv_world)
CLIP_CASES = [
    (f32(4.0), 0.5, 1.0),  # norm 2 above max_norm
    (f32(0.01), 0.5, 1.0),  # norm 0.1 below
    (f32(0.3), 0.5, 1.0),  # a norm that is no fp32 number
    (f32(4.0), 0.0, 1.0),  # max_norm <= 0: no clipping
    (f32(4.0), -1.0, 0.125),
    (f32(64.0), 0.5, 0.125),  # norm 8 / 8 above
    (f32(3.7), 0.5, 0.125),  # norm 0.24 below
    (0.0, 0.5, 1.0),  # sumsq = 0
    (f32(1e-10), f32(1e-6), 1.0),  # a norm of the size of the 1e-6 in the denominator
]


def clip_reference(ss, max_norm, inv_world):
    """(coef, norm) of include/vbx.h in fp64: norm = sqrt(sumsq) inv_world; coef = min(1, max_norm / (norm + 1e-6)) inv_world"""
    norm = math.sqrt(ss) * inv_world
    c = min(1.0, f32(max_norm) / (norm + 1e-6)) if max_norm > 0 else 1.0
    return c * inv_world, norm


def standin_clip(ss, max_norm, inv_world, fault=None):
    iw = torch.tensor(inv_world, dtype=F32)
    norm = torch.sqrt(torch.tensor(ss, dtype=F32)) * iw
    den = norm if fault == "1e-6" else norm + torch.tensor(1e-6, dtype=F32)
    c = torch.minimum(torch.tensor(1.0), torch.tensor(max_norm, dtype=F32) / den) if max_norm > 0 else torch.tensor(1.0)
    c = c * iw
    return torch.stack((c * iw if fault == "inv_world" else c, norm))


def check_clip_values(ck, ss, max_norm, inv_world, coef, dss_rel=0.0):
    """coef [2] against fp64; dss_rel: relative error of the sumsq the device started from (the chain), halved by the square root"""
    c, norm = clip_reference(ss, max_norm, inv_world)
    bc, bn = abs(c) * (N_CLIP_COEF * U + dss_rel / 2), norm * (N_CLIP_NORM * U + dss_rel / 2)
    ck.ratio("clip_coef", "coef[0]", coef[0:1], torch.tensor([c], dtype=F64), torch.tensor([bc], dtype=F64))
    ck.ratio("clip_norm", "coef[1]", coef[1:2], torch.tensor([norm], dtype=F64), torch.tensor([bn], dtype=F64))
    return c, MARGIN["clip_coef"] * bc


def clip_name(c):
    return "clip-ss%g-max%g-iw%g" % c


def check_clip(case, coef):
    ck = OptimChecks(clip_name(case))
    check_clip_values(ck, *case, coef)
    ck.done()


# ------------------------------------------------------------------------------------------------ E. the chain
CHAIN_STEPS = 3
CHAIN_MAX_NORM = 0.5  # the gradient norm is ~ 6: the clip is active in every step
CHAIN_B = 3


@lru_cache(maxsize=1)
def chain_layout():
    """One flat buffer with plain, packed and factor blocks: (table of the fused launch, factor layout, ranges of vbx_sumsq_ranges).
    The factor blocks (L = 2, J4 = 8, Th = 260, layer 1 first) and one gap are left out of the table as the product leaves them."""
    J4, Th = 8, 260
    t = Table("chain")
    t.plain(100)
    w1 = t.cur
    t.gap(J4 * Th)
    t.seg(5, 12, 16, ("bf16", "f16"))
    hole = (t.cur, t.cur + 8)
    t.gap(8)
    w0 = t.cur
    t.gap(J4 * Th)
    t.seg(1, 37, 37, ("f32",))
    t.gap(3)  # the padding behind a slot: zeros in every gradient buffer, inside the last range
    t.finish()
    lay = dict(L=2, J4=J4, Th=Th, w_off=[w0, w1], n=t.n, has_dst=[True, True], dst_array=True)
    ranges, cur = [], 0
    for lo, hi in sorted([(w1, w1 + J4 * Th), hole, (w0, w0 + J4 * Th)]):
        if lo > cur:
            ranges.append((cur, lo))
        cur = hi
    ranges.append((cur, t.n))
    assert all(lo % 4 == 0 and hi % 4 == 0 for lo, hi in ranges)
    return t, lay, tuple(ranges)


def chain_covered():
    t, lay, _ = chain_layout()
    return t.covered() | factor_covered(lay)


def chain_initial():
    t, lay, _ = chain_layout()
    inp = flat_inputs(("chain", "state"), t.n, chain_covered())
    del inp["g"]
    for k in "mv":  # Adam's state before the first step
        inp[k] = torch.where(chain_covered(), torch.zeros(()), inp[k])
    return inp


@lru_cache(maxsize=CHAIN_STEPS)
def chain_grads(step):
    """(gflat: NaN in the factor blocks and the gap, zero in the padding; dada; temb) of step 1 .. CHAIN_STEPS"""
    t, lay, _ = chain_layout()
    gen = _gen(("chain", "grads", step))
    g = torch.randn(t.n + GUARD, generator=gen) * 0.1
    g[torch.arange(t.n + GUARD) % 13 == 0] = 0
    g = torch.where(t.covered(), g, torch.full_like(g, math.nan))
    g[t.n - 3: t.n] = 0
    dada, temb = factor_operands(("chain", "factors", step), lay["L"], CHAIN_B, lay["J4"], lay["Th"])
    return g, dada, temb


def chain_nterms():
    return chain_layout()[1]["L"] * CHAIN_B * CHAIN_B


def chain_k():
    _, _, ranges = chain_layout()
    return ranges_k(RangesCase("chain", ranges, chain_nterms()))


def standin_chain_step(step, state, fault=None):
    """One step of the chain in fp32: Gram terms, the sum over the ranges and the terms, the clip coefficient, both Adam launches."""
    t, lay, ranges = chain_layout()
    g, dada, temb = chain_grads(step)
    terms = standin_gram(dada, temb)
    ss = torch.stack([(g[lo:hi] ** 2).sum() for lo, hi in ranges]).sum() + terms.sum()
    coef = standin_clip(float(ss), CHAIN_MAX_NORM, 1.0)
    gs = 1.0 if fault == "gscale" else float(coef[0])
    inp = dict(state, g=g, dada=dada, temb=temb)
    out = standin_packed_state(t, inp, gs, step)
    fac = standin_factor_state(lay, dict(inp, p=out["p"], m=out["m"], v=out["v"]), gs, step)
    out.update(fac)
    out.update(terms=terms.reshape(-1), sumsq=ss.reshape(1), coef=coef)
    return out


def check_chain_step(step, state, got):
    """One step from the device's own state `state` (p, m, v) against fp64 clip_grad_norm_ + Adam on the materialised gradient."""
    t, lay, ranges = chain_layout()
    g, dada, temb = chain_grads(step)
    ck = OptimChecks(f"chain-step{step}")
    inp = dict(state, g=g, dada=dada, temb=temb)
    check_untouched(ck, inp, got, chain_covered())
    check_gram_terms(ck, dada, temb, got["terms"])
    gfac, _ = factor_gradient(dada, temb)
    tref, tbound = gram_reference(dada, temb)
    sq_ranges = sum(g[lo:hi].double().pow(2).sum() for lo, hi in ranges)
    ss = sq_ranges + gfac.pow(2).sum()  # |g|^2 of the materialised gradient
    bss = sum_bound(chain_k(), sq_ranges + tref.abs().sum()) + tbound.sum()  # the sum's own roundings, and the terms' errors
    ck.ratio("sumsq_ranges", "sumsq", got["sumsq"].reshape(1), ss.reshape(1), bss.reshape(1))
    ck.true("the clip is active", float(ss) ** 0.5 > CHAIN_MAX_NORM)
    c, dc = check_clip_values(ck, float(ss), CHAIN_MAX_NORM, 1.0, got["coef"], dss_rel=MARGIN["sumsq_ranges"] * float(bss / ss))
    check_packed_state(ck, t, inp, got, c, step, dgs=dc)
    check_factor_state(ck, lay, inp, got, c, step, dgs=dc)
    ck.done()


# ------------------------------------------------------------------------------------------------ the real table's invariants
def check_segment_table(segs, total_blocks, n, factor_blocks, arena):
    """Invariants of a vbx_adam_seg table (dicts) over a flat buffer of n floats: sorted; the segments that take blocks and the factor
    blocks tile [0, n) without overlap; block0 consistent with count; destination extents disjoint and inside `arena` (lo, hi)."""
    ck = OptimChecks("segment-table")
    offs = [s["off"] for s in segs]
    ck.true("sorted by offset", offs == sorted(offs))
    ck.true("a rowmap 2 entry is a factor block", sorted((s["off"], s["off"] + s["count"]) for s in segs if s["rowmap"] == 2) == sorted(factor_blocks))
    cur, tiles = 0, True
    for s in segs:
        tiles &= s["off"] == cur and s["count"] > 0
        cur = s["off"] + s["count"]
    ck.true("segments and factor blocks tile [0, n)", tiles and cur == n)
    want = [dict(s) for s in segs]
    ck.true("block0 consistent with count", number_blocks(want) == total_blocks and [s["block0"] for s in want] == [s["block0"] for s in segs])
    ext = []
    for s in segs:
        rows = s["count"] // s["cols"]
        ck.true(f"segment at {s['off']}: count is rows x cols", rows * s["cols"] == s["count"])
        drows = -(-s["F"] // 64) * 128 if s["rowmap"] == 1 else rows
        for k, w in (("dst_bf16", 2), ("dst_f16", 2), ("dst_f32", 4)):
            if s[k]:
                ck.true(f"segment at {s['off']}: cols <= dst_ld", s["cols"] <= s["dst_ld"])
                ext.append((s[k], s[k] + ((drows - 1) * s["dst_ld"] + s["cols"]) * w))
    ext.sort()
    ck.true("destination extents disjoint", all(a[1] <= b[0] for a, b in zip(ext, ext[1:])))
    ck.true("destination extents inside the operand arena", all(arena[0] <= lo and hi <= arena[1] for lo, hi in ext))
    ck.done()
