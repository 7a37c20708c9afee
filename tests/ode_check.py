"""Cases, fp64 references, fp32 stand-ins and per-element bounds of the sampler kernel edge tests (tests/test_ode_check_cpu.py checks
the checks on the CPU, tests/test_ode_edges_gpu.py launches every case).  torch on the CPU only: nothing here touches the library or a
device.

The kernels: all of csrc/ode.hip -- vbx_ode_combine / _dp, vbx_ode_stage_time / _dp, vbx_ode_norm / _lens (the partial sums and the
controller behind them), vbx_ode_commit, vbx_ode_dense, vbx_zero_tail_rows -- and the copies a forward starts with: vbx_pack_embed_input,
vbx_stack_input, vbx_unet_cat / _split / _addskip (csrc/ops.hip) and vbx_copy_cols_f32 (csrc/codec.hip).  Inputs are seeded and rounded
once to the type the kernel reads; every output starts as NaN sentinels with a guard behind it; every operand element a launch must not
read is NaN; every slot of the fp64 step state a launch must not write holds a finite sentinel of its own and is compared by bits
afterwards; copies, the stage times and the combinations are compared by bits.

csrc/ode.hip is compiled with contraction off, so its fp32 arithmetic is restated here operation for operation (a product, then a sum:
torch on the CPU does not fuse) and vbx_ode_combine / _dp must return the stand-in's bits; every case carries a planted element on
which a fused product-sum gives other bits (PLANT, found on the CPU with exact rational arithmetic).  Beside that every element is
compared with fp64 at a bound counted by the rules at the top of tests/rows_check.py (u = 2^-24 per fp32 rounding on the element's
path, first order with absolute values, MARGIN = 2, half an ulp of a 16-bit store -- the 16-bit stores here are all compared by bits).
The fp64 sums of the error norm are bounded in units of 2^-53.  Terms that stand beside the counted part:
 * RHO_POW: the relative error of powf in the controller's INIT1 arm h1 = (0.01 / max(d1, d2))^(1/5), twice the figure measured
   through vbx_ode_norm itself over the sweep POW_SWEEP of max(d1, d2) against fp64 (test_powf_sweep, profiles/ode_edges_measured.json).
   Only the DT slot of an INIT1 case that takes the powf arm carries it.
 * N_POW64 = 8: fp64 roundings between the error ratio and the next step size on the device and in ode_ref._optimal_step_size together
   (pow counted as two on either side, the quotient, the product), in units of 2^-53.
"""
import json
import math
import os
from dataclasses import astuple, dataclass
from functools import lru_cache

import torch

import ode_ref
from optim_check import _gen, sentinel
from rows_check import BF16, F16, F32, F64, U, RowChecks

I16, I32, I64 = torch.int16, torch.int32, torch.int64
NAN, INF = math.nan, math.inf
U64 = 2.0 ** -53
GUARD = 8
GRID_CAP = 4096 * 256  # ode_grid() / grid_for(): at most 4096 blocks of 256 threads; more work items take the grid-stride loop
NORM_CAP = 1024 * 256  # the partial sums: at most 1024 blocks
SMALL_N = (4, 1020, 1024, 1028)
N_SLAB = 257 * 1024 + 8  # 257 full workgroups and two float4 in a 258th: the controller's slab loop takes a second trip, two entries long
N_NORM_CAP = NORM_CAP * 4 + 20  # five float4 in the second trip of the partial sums
N_CAP = GRID_CAP * 4 + 12  # three float4 in the second trip of combine / commit / dense
MAX_STAGES = 7
N_POW64 = 8
POW_SWEEP = (-24, 24, 1 / 8)  # max(d1, d2) = 2^e for e from -24 to 24 in steps of 1 / 8
POWF_REL_MEASURED = 9.396e-08  # 1.6 u at max(d1, d2) = 120194: the largest |DT - pow64| / pow64 over the sweep on MI355X (profiles/ode_edges_measured.json)
RHO_POW = 2 * POWF_REL_MEASURED

(DP_T, DP_DT, DP_T0, DP_T1, DP_DT32, DP_RATIO, DP_H0, DP_D1, DP_NFE, DP_ACCEPTED, DP_REJECTED, DP_LAST, DP_DONE, DP_BAD, DP_ATOL, DP_RTOL,
 DP_TEND) = range(17)
DP_STATE = 20
SLOT = ("T", "DT", "T0", "T1", "DT32", "RATIO", "H0", "D1", "NFE", "ACCEPTED", "REJECTED", "LAST", "DONE", "BAD", "ATOL", "RTOL", "TEND", "17",
        "18", "19")
TIME_TABLE, TIME_STAGE, TIME_END, TIME_PROBE = range(4)
NORM_ERROR, NORM_INIT0, NORM_INIT1 = range(3)
SENT64 = 0x7FF8000000000001


def f32(x):
    """the fp32 value of a python float, as a python float"""
    return float(torch.tensor(x, dtype=F64).to(F32))


def raw(t):
    return t.contiguous().view({8: I64, 4: I32, 2: I16, 1: torch.uint8}[t.element_size()])


def sent64(n):
    return torch.full((n,), SENT64, dtype=I64).view(F64)


def with_guard(x, dtype=None):
    """x flat with GUARD NaN sentinels behind it"""
    x = x.reshape(-1)
    return torch.cat([x, sent64(GUARD) if x.dtype == F64 else sentinel(GUARD, dtype or x.dtype)])


def out_buf(n, dtype=F32):
    return sent64(n + GUARD) if dtype == F64 else sentinel(n + GUARD, dtype)


def state_buf(fill, **slots):
    """DP_STATE doubles and a guard: `fill` "nan" (a launch that only reads) or "own" (slot i holds -(1000.5 + i): a launch that writes)"""
    s = torch.full((DP_STATE,), NAN, dtype=F64) if fill == "nan" else -(1000.5 + torch.arange(DP_STATE, dtype=F64))
    for k, v in slots.items():
        s[SLOT.index(k)] = v
    return with_guard(s)


class OdeChecks(RowChecks):
    """rows_check.RowChecks with the log of these tests: ODE_CHECK_LOG=<file> appends one JSON line per case with every measured value
    (how profiles/ode_edges_measured.json was made)."""

    def done(self):
        if os.environ.get("ODE_CHECK_LOG"):
            with open(os.environ["ODE_CHECK_LOG"], "a") as f:
                f.write(json.dumps({"case": self.case, "values": [(n, v if isinstance(v, bool) else float(v), b) for n, v, b in self.seen]}) + "\n")
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)

    def note(self, name, value):
        """logged, not asserted"""
        self.seen.append((name, value, None))

    def same_bits(self, name, got, want):
        """RowChecks.same_bits; the fp64 step state and slab go through it as pairs of 32-bit words"""
        if got.dtype == F64 and want.dtype == F64:
            got, want = got.reshape(-1).view(F32), want.reshape(-1).view(F32)
        super().same_bits(name, got, want)

    def sentinel_kept(self, name, t):
        if t.dtype == F64:
            return self.same_bits(f"{name} keeps its sentinel", t, sent64(t.numel()))
        super().sentinel_kept(name, t)

    def rel(self, name, got, want, bound):
        """|got - want| <= bound |want|, logged as error / bound"""
        got, want = float(got), float(want)
        err = abs(got - want)
        self.le(f"{name} error / bound", 0.0 if err == 0 else (err / (bound * abs(want)) if want != 0 and bound > 0 else INF), 1.0)


def fma32(a, b, c):
    """a b + c with one rounding, for the planted faults and the proof that the planted elements tell: the exact product in fp64, the
    sum rounded to fp64 and then to fp32 (a double rounding can differ from the fused result only on a tie of the second rounding)"""
    return (a.double() * b.double() + c.double()).float()


# ================================================================================================ A. vbx_ode_combine / _dp
# the first two coefficients of every case and the first element (k_0[0], k_1[0], y[0]; k_j[0] = 0 for j >= 2): fma(k_0, c_0, y) differs
# from y + k_0 c_0 (S = 1) and y + fma(k_1, c_1, k_0 c_0) from y + (k_0 c_0 + k_1 c_1) (S >= 2), both checked with exact rationals.
# The second element tells the stage order at S >= 3: k_0 c_0 = 2^20 c_0 and k_1 c_1 cancel but for a remainder, so the sum from the
# last stage down rounds the other products to the ulp of 2^20 c_0 before they meet it.
C01 = {"table": (0.30000001192092896, -1.7000000476837158), "dt": (0.20000000298023224, 0.07500000298023224),
       "h0": (0.20000000298023224, 0.07500000298023224)}  # dt / h0: the tableau entries beta_0, beta_1; c_j = fp32(beta_j fp32(slot))
SLOT_VALUE = {"dt": 0.1, "h0": 0.017}  # not fp32 numbers, and fp32(beta_0 slot) is not fp32(beta_0 fp32(slot))
PLANT = {"table": (0.51171875, -0.693359375, -0.1669921875), "dt": (-2.1259765625, 1.43359375, 0.1083984375),
         "h0": (-2.322265625, -1.7998046875, 0.001953125)}
TABLE_FORMS = [(dl, st, last, ctr) for dl in (0, 3) for st in ("1", "S", "S+2") for last in (False, True) for ctr in (0, 5)]


@dataclass(frozen=True)
class CombineCase:
    form: str  # "table", or the dopri5 form reading its step from the state: "dt" (VBX_DP_DT), "h0" (VBX_DP_H0)
    n: int
    S: int
    inplace: bool
    ld: int = 0
    stride: int = 1
    row: int = 0
    counter: int = 0

    @property
    def name(self):
        t = f"-ld{self.ld}-st{self.stride}-r{self.row}-c{self.counter}" if self.form == "table" else ""
        return f"combine-{self.form}-n{self.n}-S{self.S}-{'inplace' if self.inplace else 'distinct'}{t}"


def _table_case(n, S, inplace, i):
    dl, st, last, ctr = TABLE_FORMS[i % len(TABLE_FORMS)]
    stride = {"1": 1, "S": S, "S+2": S + 2}[st]
    return CombineCase("table", n, S, inplace, S + dl, stride, stride - 1 if last else 0, ctr)


def _combine_table():
    out, i = [], 0
    for n in SMALL_N:
        for S in range(1, MAX_STAGES + 1):
            out.append(_table_case(n, S, (i + S) % 2 == 0, 5 * i))
            out.append(CombineCase(("dt", "h0")[i % 2], n, S, (i + S) % 2 == 1))
            i += 1
    out += [_table_case(1028, 3, i % 2 == 0, i) for i in range(len(TABLE_FORMS))]  # every table form once at one size
    out += [CombineCase(f, 1028, S, ip) for f in ("dt", "h0") for S in (1, 7) for ip in (False, True)]
    out += [_table_case(N_CAP, 1, True, 23), CombineCase("dt", N_CAP, 7, False)]
    return list(dict.fromkeys(out))


COMBINE_CASES = _combine_table()


@lru_cache(maxsize=2)
def combine_inputs(c):
    g = _gen(("combine",) + astuple(c))
    y = torch.randn(c.n, generator=g)
    k = [torch.randn(c.n, generator=g) for _ in range(c.S)]
    coef = torch.randn(MAX_STAGES, generator=g)
    coef[:2] = torch.tensor(C01[c.form], dtype=F64).float()
    k0, k1, y0 = PLANT[c.form]
    y[0], k[0][0] = y0, k0
    for j in range(1, c.S):
        k[j][0] = k1 if j == 1 else 0.0
    if c.S >= 3:
        cj = coef if c.form == "table" else step_coefs(coef, SLOT_VALUE[c.form])
        k[0][1] = 2.0 ** 20
        k[1][1] = -(k[0][1] * cj[0]) / cj[1]
    return dict(y=y, k=k, coef=coef[: c.S])


def combine_operands(c):
    """what the launch is given: y, out (None: in place), k with NaN guards, and the table with its counter or the state"""
    inp = combine_inputs(c)
    ops = dict(y=with_guard(inp["y"]), out=None if c.inplace else out_buf(c.n), k=[with_guard(t) for t in inp["k"]])
    if c.form == "table":
        r = c.counter * c.stride + c.row
        table = torch.full(((r + 2) * c.ld,), NAN)
        table[r * c.ld: r * c.ld + c.S] = inp["coef"]
        ops.update(table=table, counter=torch.tensor([c.counter, -1], dtype=I32))
    else:
        ops.update(state=state_buf("nan", **{"DT" if c.form == "dt" else "H0": SLOT_VALUE[c.form]}), beta=[float(v) for v in inp["coef"]])
    return ops


def step_coefs(coef, dt, fault=None):
    """c_j = beta_j fp32(dt) in fp32, as load_coefs forms them"""
    if fault == "nocast":  # the product taken with the fp64 slot
        return (coef.double() * dt).float()
    return coef * torch.tensor(dt, dtype=F64).float()


def stage_sum(k, c, fault=None):
    """sum_j c_j k_j in stage order, a product and then a sum"""
    js = list(range(len(k)))[::-1] if fault == "reversed" else list(range(len(k)))
    acc = k[js[0]] * c[js[0]]
    for j in js[1:]:
        acc = fma32(k[j], c[j], acc) if fault == "fma" else acc + k[j] * c[j]
    return acc


def combine_values(c, fault=None):
    inp = combine_inputs(c)
    coef = inp["coef"] if c.form == "table" else step_coefs(inp["coef"], SLOT_VALUE[c.form], fault)
    if fault == "fma" and c.S == 1:
        return fma32(inp["k"][0], coef[0], inp["y"])
    return inp["y"] + stage_sum(inp["k"], coef, fault)


def standin_combine(c, fault=None):
    ops = combine_operands(c)
    out = ops["y"].clone() if c.inplace else ops["out"]
    m = min(c.n, 4 * GRID_CAP) if fault == "cap" else c.n
    out[:m] = combine_values(c, fault)[:m]
    return dict(out=out, y=out if c.inplace else ops["y"])


def check_combine(c, got):
    inp = combine_inputs(c)
    ck = OdeChecks(c.name)
    want = combine_values(c)
    ck.true("a fused product-sum gives other bits on the planted element", bool(raw(combine_values(c, "fma"))[0] != raw(want)[0]))
    ck.same_bits("out is the fp32 sum of fp32 products by bits", got["out"][: c.n], want)
    # fp64: a rounding per product (two in the dopri5 form: c_j itself is a rounded product), S - 1 additions of at most P = sum |c_j
    # k_j| each, the addition of y
    step = 1.0 if c.form == "table" else f32(SLOT_VALUE[c.form])
    cj = inp["coef"].double() * step
    ref, P = inp["y"].double(), torch.zeros(c.n, dtype=F64)
    for j in range(c.S):
        ref, P = ref + cj[j] * inp["k"][j].double(), P + (cj[j] * inp["k"][j].double()).abs()
    ck.ratio("combine_" + ("table" if c.form == "table" else "dp"), "out", got["out"][: c.n], ref, U * ((c.S + (c.form != "table")) * P + ref.abs()))
    ck.sentinel_kept("out guard", got["out"][c.n:])
    if not c.inplace:
        ck.same_bits("y is unchanged", got["y"], combine_operands(c)["y"])
    ck.done()


# ================================================================================================ B. vbx_ode_stage_time / _dp
TIME_B = (1, 63, 64, 65, 130)
STAGE_T, STAGE_DT, STAGE_ALPHA = 0.123456789, 0.1, 8 / 9  # fma(alpha, fp32(dt), fp32(t)) differs from the unfused sum (exact rationals)
PROBE_T, PROBE_H0 = 0.123456789, 0.0123456789
TIME_TABLES = ((1, 0, 0), (3, 2, 5), (3, 0, 5), (4, 3, 0), (2, 1, 1))  # (stride, slot, counter)
TIME_ENDS = {"one": (0.75, 0.25), "half": (0.25, 0.25), "zero": (-0.25, 0.25), "negative": (-1.0, 0.25), "min_normal": (0.0, 2.0 ** -126),
             "rounds_up": (0.5, 2.0 ** -25 + 2.0 ** -40)}  # (T, DT): T + DT is exact in fp64


@dataclass(frozen=True)
class TimeCase:
    mode: str  # table, stage, probe, end
    B: int
    which: str = ""

    @property
    def name(self):
        return f"time-{self.mode}-B{self.B}" + (f"-{self.which}" if self.which else "")


TIME_CASES = [TimeCase("table", B, str(i)) for i, B in enumerate(TIME_B)] + [TimeCase(m, B) for m in ("stage", "probe") for B in TIME_B]
TIME_CASES += [TimeCase("end", B, w) for B in TIME_B for w in TIME_ENDS]


def time_operands(c):
    ops = dict(times=out_buf(c.B))
    if c.mode == "table":
        stride, slot, counter = TIME_TABLES[int(c.which)]
        table = torch.full(((counter + 2) * stride,), NAN)
        table[counter * stride + slot] = 0.625 + int(c.which) / 1024
        ops.update(table=table, counter=torch.tensor([counter, -1], dtype=I32), stride=stride, slot=slot)
    elif c.mode == "stage":
        ops.update(state=state_buf("nan", T=STAGE_T, DT=STAGE_DT), alpha=STAGE_ALPHA, tmode=TIME_STAGE)
    elif c.mode == "probe":
        ops.update(state=state_buf("nan", T=PROBE_T, H0=PROBE_H0), alpha=0.0, tmode=TIME_PROBE)
    else:
        T, DT = TIME_ENDS[c.which]
        ops.update(state=state_buf("nan", T=T, DT=DT), alpha=1.0, tmode=TIME_END)
    return ops


def time_value(c, fault=None):
    """the one fp32 value every times[b] holds"""
    ops = time_operands(c)
    if c.mode == "table":
        return ops["table"][int(ops["counter"][0]) * ops["stride"] + ops["slot"]].reshape(1)
    s = ops["state"]
    if c.mode == "stage":
        t, a, d = s[DP_T].float(), torch.tensor(STAGE_ALPHA, dtype=F64).float(), s[DP_DT].float()
        return (fma32(a, d, t) if fault == "fma" else t + a * d).reshape(1)
    if c.mode == "probe":
        return (s[DP_T] + s[DP_H0]).float().reshape(1)
    t = (s[DP_T] + s[DP_DT]).float().reshape(1)
    return t if fault == "noprev" else torch.nextafter(t, torch.tensor([-INF]))


def standin_time(c, fault=None):
    out = time_operands(c)["times"]
    out[: c.B] = time_value(c, fault)
    return dict(times=out)


def check_time(c, got):
    ck = OdeChecks(c.name)
    want = time_value(c)
    if c.mode == "stage":
        ck.true("a fused product-sum gives other bits", bool(raw(time_value(c, "fma")) != raw(want)))
    if c.mode == "end":
        T, DT = TIME_ENDS[c.which]
        t = f32(T + DT)
        ck.true("the value is the fp32 number below fp32(t0 + dt)", float(want) < t and (c.which != "rounds_up" or t > T + DT))
    ck.same_bits("times", got["times"][: c.B], want.expand(c.B))
    ck.sentinel_kept("times guard", got["times"][c.B:])
    ck.done()


# ================================================================================================ C. vbx_ode_norm / _lens
C_ERROR = torch.tensor(ode_ref.DPS_C_ERROR, dtype=F64).float()
ATOL, RTOL = 1e-3, 1e-2  # not fp32 numbers: the kernel's casts are counted
NORM_T, NORM_DT, NORM_TEND = 0.3, 0.1, 1.0
NFE0, ACC0, REJ0 = 44.0, 3.0, 2.0  # the counters start from these
ATOL_C = 2.0 ** -10  # the controller cases: rtol = 0, c = (1, 0, ...), a power-of-two dt: the element term is k_1 dt / atol exactly
# name -> (the four element terms q, T, dt, TEND): ratio = sqrt(sum q^2 / 4) is exact in every case
CTRL = {
    "ratio0": ((0.0,) * 4, 0.25, 0.125, 1.0),
    "interior": ((0.25,) * 4, 0.25, 0.5, 1.0),
    "clamp10": ((2.0 ** -20,) * 4, 0.25, 0.125, 1.0),
    "one": ((1.0,) * 4, 0.25, 0.125, 1.0),
    "above1_f32": ((1 + 2.0 ** -23,) * 4, 0.25, 0.125, 1.0),
    "above1_f64": ((2.0, 2.0 ** -25, 2.0 ** -25, 0.0), 0.25, 0.125, 1.0),  # sum q^2 / 4 = 1 + 2^-51, its root rounds to 1 + 2^-52
    "clamp02": ((2048.0,) * 4, 0.25, 0.125, 1.0),
    "nan": ((0.5, NAN, 0.5, 0.5), 0.25, 0.125, 1.0),
    "inf": ((0.5, 0.5, INF, 0.5), 0.25, 0.125, 1.0),
    "underflow": ((0.0,) * 4, 1.0, 2.0 ** -60, 2.0),
    "done_eq": ((0.25,) * 4, 0.75, 0.25, 1.0),
    "done_gt": ((0.25,) * 4, 0.75, 0.5, 1.0),
    "done_dt01": ((0.0,) * 4, 0.95, 0.1, 1.0),
}
CTRL_RATIO = {"ratio0": 0.0, "interior": 0.25, "clamp10": 2.0 ** -20, "one": 1.0, "above1_f32": 1 + 2.0 ** -23, "above1_f64": 1 + 2.0 ** -52,
              "clamp02": 2048.0, "underflow": 0.0, "done_eq": 0.25, "done_gt": 0.25, "done_dt01": 0.0}
# name -> (factor of dt, accepted, DONE or None, BAD or None)
CTRL_OUTCOME = {"ratio0": (10.0, 1, 0, None), "interior": (0.9 * 4 ** 0.2, 1, 0, None), "clamp10": (10.0, 1, 0, None), "one": (0.9, 1, 0, None),
                "above1_f32": (0.9 * (1 + 2.0 ** -23) ** -0.2, 0, None, None), "above1_f64": (0.9, 0, None, None), "clamp02": (0.2, 0, None, None),
                "underflow": (10.0, 1, 0, 2), "done_eq": (0.9 * 4 ** 0.2, 1, 1, None), "done_gt": (0.9 * 4 ** 0.2, 1, 1, None),
                "done_dt01": (10.0, 1, 1, None)}
INIT_DATA = ("rand", "y0zero", "allzero")  # the arms of the initial step: the general one; d0 < 1e-5; d1 and d2 <= 1e-15


@dataclass(frozen=True)
class NormCase:
    mode: int
    n: int
    nfe: int = 1
    shape: tuple = None  # (B, N, D): vbx_ode_norm_lens
    lens: tuple = None
    data: str = "rand"  # ERROR: a key of CTRL; INIT0 / INIT1: one of INIT_DATA

    @property
    def name(self):
        l = "" if self.shape is None else "-lens" + "x".join(map(str, self.shape)) + "-" + "_".join(map(str, self.lens))
        return f"norm-{('error', 'init0', 'init1')[self.mode]}-n{self.n}-m{self.nfe}{l}-{self.data}"

    @property
    def S(self):
        return (MAX_STAGES, 1, 2)[self.mode]

    @property
    def nb(self):
        return min(-(-(self.n // 4) // 256), 1024)

    @property
    def kept(self):
        return self.n if self.shape is None else self.shape[2] * sum(self.lens)


# the last shape: B = 2, N = 131080, D = 4: float4 262144 ... 262159 are the second trip, frames 131064 ... of row 1
LENS_SHAPES = (((3, 37, 12), (0, 37, 20)), ((3, 37, 12), (37, 37, 37)), ((2, 9, 4), (5, 0)), ((2, 131080, 4), (131080, 131072)))


def _norm_table():
    out = []
    for i, n in enumerate(SMALL_N + (N_SLAB, N_NORM_CAP)):
        out += [NormCase(mode, n, 1 + (i + mode) % 2) for mode in range(3)]
    for i, (shape, lens) in enumerate(LENS_SHAPES):
        n = shape[0] * shape[1] * shape[2]
        out += [NormCase(mode, n, 1 + (i + mode) % 2, shape, lens) for mode in range(3) if n < NORM_CAP or mode == NORM_ERROR]
    out += [NormCase(NORM_ERROR, 4, m, data=d) for d in CTRL for m in (1, 2)]
    out += [NormCase(mode, n, m, data=d) for mode in (NORM_INIT0, NORM_INIT1) for d in INIT_DATA[1:] for n, m in ((4, 1), (1028, 2))]
    return out


NORM_CASES = _norm_table()


def keep_mask(c, fault=None):
    if c.shape is None:
        return None
    B, N, D = c.shape
    frame = torch.arange(N)[None, :, None].expand(B, N, D)
    lens = torch.tensor(c.lens)[:, None, None]
    return (frame <= lens if fault == "lens" else frame < lens).reshape(-1)


@lru_cache(maxsize=2)
def norm_inputs(c):
    g = _gen(("norm",) + astuple(c))
    y0, y1 = torch.randn(c.n, generator=g), torch.randn(c.n, generator=g)
    k = [torch.randn(c.n, generator=g) for _ in range(c.S)]
    st = dict(T=NORM_T, DT=NORM_DT, TEND=NORM_TEND, ATOL=ATOL, RTOL=RTOL, NFE=NFE0, ACCEPTED=ACC0, REJECTED=REJ0)
    coef = C_ERROR
    if c.mode == NORM_ERROR and c.data != "rand":
        q, T, dt, TEND = CTRL[c.data]
        coef = torch.tensor([1.0] + [0.0] * 6)
        k[0] = torch.tensor(q, dtype=F64).float() * ATOL_C / f32(dt)
        st.update(T=T, DT=dt, TEND=TEND, ATOL=ATOL_C, RTOL=0.0)
    if c.mode != NORM_ERROR:
        y0 = y0 if c.data == "rand" else torch.zeros(c.n)
        if c.data == "allzero":
            k = [torch.zeros(c.n) for _ in k]
        if c.mode == NORM_INIT1:
            if c.data != "allzero":
                k[1] = k[0] + 0.01 * k[1]
            first = NormCase(NORM_INIT0, c.n, c.nfe, c.shape, c.lens, c.data)  # H0 and D1 as INIT0 leaves them on the same y0, f0
            h = control(first, state_buf("own", **st), *norm_sums(first, dict(y0=y0, y1=None, k=k[:1], coef=coef, st=st)))[0]
            st.update(H0=float(h[DP_H0]), D1=float(h[DP_D1]))
    keep = keep_mask(c)
    if keep is not None:  # what the kernel must not read
        for t in [y0, y1] + k:
            t[~keep] = NAN
    return dict(y0=y0, y1=y1 if c.mode == NORM_ERROR else None, k=k, coef=coef, st=st)


def norm_operands(c):
    inp = norm_inputs(c)
    return dict(state=state_buf("own", **inp["st"]), slab=out_buf(2 * c.nb, F64), y0=with_guard(inp["y0"]),
                y1=None if inp["y1"] is None else with_guard(inp["y1"]), k=[with_guard(t) for t in inp["k"]],
                coef=[float(v) for v in inp["coef"]] if c.mode == NORM_ERROR else None,
                lens=None if c.lens is None else torch.tensor(c.lens, dtype=I32))


def norm_terms32(c, inp):
    """the kernel's own fp32 element terms (lane 0, lane 1 or None), dropped elements included"""
    atol, rtol = (torch.tensor(inp["st"][s], dtype=F64).float() for s in ("ATOL", "RTOL"))
    u = inp["y0"]
    if c.mode == NORM_ERROR:
        e = stage_sum(inp["k"], step_coefs(inp["coef"], inp["st"]["DT"]))
        return e / (atol + rtol * torch.maximum(u.abs(), inp["y1"].abs())), None
    s = atol + u.abs() * rtol
    if c.mode == NORM_INIT0:
        return u / s, inp["k"][0] / s
    return (inp["k"][1] - inp["k"][0]) / s, None


def norm_terms64(c, inp):
    """per slab lane: the element terms in fp64 throughout and the counted bound of the fp32 term per element"""
    atol, rtol, u = inp["st"]["ATOL"], inp["st"]["RTOL"], inp["y0"].double()
    if c.mode == NORM_ERROR:
        cj = inp["coef"].double() * f32(inp["st"]["DT"])
        e, P = torch.zeros(c.n, dtype=F64), torch.zeros(c.n, dtype=F64)
        for j in range(c.S):
            e, P = e + cj[j] * inp["k"][j].double(), P + (cj[j] * inp["k"][j].double()).abs()
        tol = atol + rtol * torch.maximum(u.abs(), inp["y1"].double().abs())
        # e: two roundings per product (c_j is one itself), S - 1 additions of at most P; tol: the casts of atol and rtol, the product,
        # the sum, all of one sign; the quotient
        return [(e / tol, U * ((c.S + 1) * P / tol + 5 * (e / tol).abs()))]
    s = atol + u.abs() * rtol  # scale: the casts of atol and rtol, the product, the sum, all of one sign; then the quotient
    if c.mode == NORM_INIT0:
        f0 = inp["k"][0].double()
        return [(u / s, U * 5 * (u / s).abs()), (f0 / s, U * 5 * (f0 / s).abs())]
    d = inp["k"][1].double() - inp["k"][0].double()
    return [(d / s, U * 6 * (d / s).abs())]  # the difference, then as above


def block_sums(c, sq, fault=None):
    """[nb] fp64: the sum over each workgroup's own float4 of the grid-stride loop"""
    per = c.nb * 1024
    trips = -(-c.n // per)
    sq = torch.cat([sq, torch.zeros(trips * per - c.n, dtype=F64)]).view(trips, c.nb, 1024)
    return (sq[:1] if fault == "cap" else sq).sum((0, 2))


def norm_sums(c, inp, fault=None):
    """(a, b): the slab lanes [nb] as the partial-sum launch leaves them, from the fp32 terms"""
    p, r = norm_terms32(c, inp)
    keep = keep_mask(c, fault)
    sq = [torch.zeros(c.n, dtype=F64) if t is None else (t.double() ** 2 if keep is None else torch.where(keep, t.double() ** 2, 0.0)) for t in (p, r)]
    return block_sums(c, sq[0], fault), block_sums(c, sq[1], fault)


def control(c, state, a, b, fault=None):
    """ode_control_kernel on the slab lanes: (the state afterwards, {slot: relative bound} of the slots not compared by bits)"""
    s, m = state.clone(), c.nfe
    if fault == "slab256":
        a, b = a[:256], b[:256]
    a, b, n = float(a.sum()), float(b.sum()), c.kept
    sumtol = (n + 2) * U64  # over the n kept elements: n - 1 additions of non-negatives in another order, the quotient, the root
    if c.mode == NORM_INIT0:
        d0, d1 = (torch.tensor(math.sqrt(v / n), dtype=F64).float() for v in (a, b))
        h0 = torch.tensor(1e-6) if bool(d0 < 1e-5) or bool(d1 < 1e-5) else torch.tensor(0.01) * d0 / d1
        s[DP_H0], s[DP_D1], s[DP_NFE] = h0.double(), d1.double(), s[DP_NFE] + m
        # a sum in another order can move fp32(sqrt(.)) to the neighbouring fp32 number (2 u); d0 and d1 so moved pass through a
        # product and a quotient that can each move by one more
        return s, {DP_H0: 8 * U, DP_D1: 2 * U}
    if c.mode == NORM_INIT1:
        h0, d1 = s[DP_H0].float(), s[DP_D1].float()
        d2 = torch.tensor(math.sqrt(a / n), dtype=F64).float() / h0
        tiny = bool(d1 <= 1e-15) and bool(d2 <= 1e-15)
        if tiny:
            h1 = torch.maximum(torch.tensor(1e-6), h0 * torch.tensor(1e-3))
        else:  # powf against fp64 on the fp32 operands: RHO_POW, and d2 moved by two fp32 numbers as above, a fifth of it through the power
            h1 = ((torch.tensor(0.01) / torch.maximum(d1, d2)).double() ** float(torch.tensor(1.0) / torch.tensor(5.0))).float()
        s[DP_DT], s[DP_NFE] = torch.minimum(100.0 * h0, h1).double(), s[DP_NFE] + m
        return s, {DP_DT: 2 * U + (0.0 if tiny or bool(100.0 * h0 < h1) else RHO_POW + 2 * U)}
    ratio, dt, t = math.sqrt(a / n) if a == a else NAN, float(s[DP_DT]), float(s[DP_T])
    s[DP_RATIO], s[DP_NFE] = ratio, s[DP_NFE] + 6 * m
    if not (ratio == ratio) or ratio > 1e300:
        s[DP_BAD], s[DP_LAST] = 1.0, 0.0
        return s, {}
    accept = ratio < 1.0 if fault == "less" else ratio <= 1.0
    dt_next = float(ode_ref._optimal_step_size(torch.tensor(dt, dtype=F64), torch.tensor(ratio, dtype=F64)))
    if accept:
        s[DP_T0], s[DP_T1], s[DP_DT32], s[DP_T] = t, t + dt, f32(dt), t + dt
        s[DP_ACCEPTED], s[DP_DONE] = s[DP_ACCEPTED] + 1, float(t + dt >= float(s[DP_TEND]))
    else:
        s[DP_REJECTED] = s[DP_REJECTED] + 1
    s[DP_LAST], s[DP_DT] = float(accept), dt_next
    if not (float(s[DP_T]) + dt_next > float(s[DP_T])):
        s[DP_BAD] = 2.0
    # the next step: N_POW64 roundings, and a fifth of the ratio's own bound through the power
    return s, {DP_RATIO: sumtol, DP_DT: N_POW64 * U64 + sumtol / 5}


def standin_norm(c, fault=None):
    inp, ops = norm_inputs(c), norm_operands(c)
    a, b = norm_sums(c, inp, fault)
    ops["slab"][: 2 * c.nb] = torch.stack([a, b], 1).reshape(-1)
    state = ops["state"].clone()
    state[:DP_STATE] = control(c, ops["state"][:DP_STATE], a, b, fault)[0]
    return dict(state=state, slab=ops["slab"])


def reference_initial_step(c, inp):
    """(h0, dt) of ode_ref._select_initial_step on the kept elements: fp32 where torchdiffeq is fp32"""
    keep = keep_mask(c)
    sel = (lambda t: t) if keep is None else (lambda t: t[keep])
    seen = []

    def func(t, y):
        seen.append(float(t))
        return sel(inp["k"][min(1, len(inp["k"]) - 1)])

    rtol, atol = torch.tensor(inp["st"]["RTOL"], dtype=F64), torch.tensor(inp["st"]["ATOL"], dtype=F64)
    dt = ode_ref._select_initial_step(func, torch.tensor(0.0, dtype=F64), sel(inp["y0"]), 4, rtol, atol, sel(inp["k"][0]))
    return seen[0], float(dt)


def check_norm(c, got):
    inp, ops = norm_inputs(c), norm_operands(c)
    ck = OdeChecks(c.name)
    nb, n, kind = c.nb, c.kept, ("error", "init0", "init1")[c.mode]
    slab = got["slab"][: 2 * nb].view(nb, 2)
    ck.true("every slab entry is written", bool((raw(slab) != SENT64).all()) and (bool(torch.isfinite(slab).all()) or c.data in ("nan", "inf")))
    ck.sentinel_kept("slab guard", got["slab"][2 * nb:])
    ck.sentinel_kept("state guard", got["state"][DP_STATE:])
    a, b = norm_sums(c, inp)
    exact = c.data not in ("nan", "inf")
    if exact:
        # the sum of the kept fp32 terms' squares (exact in fp64) in any order: n - 1 additions of non-negatives, however they are grouped
        # into threads, trees, slab entries and the sum taken here; (n + 2) 2^-53 as for the ratio
        for lane, name in ((a, "lane 0"), (b, "lane 1")):
            i = 0 if lane is a else 1
            if float(lane.sum()) == 0.0:
                ck.true(f"slab {name} is exactly zero", bool((slab[:, i] == 0).all()))
            else:
                ck.rel(f"slab {name} against the fp64 sum of the fp32 terms [norm_{kind}_sum]", slab[:, i].sum(), lane.sum(), (n + 2) * U64)
    want, rel = control(c, ops["state"][:DP_STATE], a, b)
    state = got["state"][:DP_STATE]
    for i in range(DP_STATE):
        if i in rel and exact and float(want[i]) != 0.0:
            ck.rel(f"state {SLOT[i]} [norm_{kind}_{SLOT[i]}]", state[i], want[i], rel[i])
        elif i == DP_RATIO and not exact:
            ck.true("state RATIO is not finite", not math.isfinite(float(state[i])))
        else:
            ck.same_bits(f"state {SLOT[i]}", state[i], want[i])
    if c.mode == NORM_ERROR and c.data in CTRL_OUTCOME:
        factor, acc, done, bad = CTRL_OUTCOME[c.data]
        dt = CTRL[c.data][2]
        ck.same_bits("state RATIO is the constructed value", state[DP_RATIO], torch.tensor(CTRL_RATIO[c.data], dtype=F64))
        ck.rel(f"state DT against {factor:.4g} dt [norm_error_factor]", state[DP_DT], factor * dt, (N_POW64 + 2) * U64)
        ck.true("accepted / rejected, DONE and BAD as constructed",
                float(state[DP_LAST]) == acc and float(state[DP_ACCEPTED]) == ACC0 + acc and float(state[DP_REJECTED]) == REJ0 + 1 - acc
                and (done is None or float(state[DP_DONE]) == done) and (bad is None or float(state[DP_BAD]) == bad)
                and float(state[DP_NFE]) == NFE0 + 6 * c.nfe and (not acc or float(state[DP_DT32]) == f32(dt)))
    if c.data == "rand":
        # against the formula in fp64 throughout: ||q32 - q64|| / sqrt(n) from the counted bound per element (with MARGIN); the rms of
        # the device is the root of its slab lane's sum over n, in STEP mode also the RATIO slot
        keep = keep_mask(c)
        for i, (q64, cq) in enumerate(norm_terms64(c, inp)):
            if keep is not None:
                q64, cq = q64[keep], cq[keep]
            r64 = float((q64 ** 2).mean().sqrt())
            bound = float(((2 * cq) ** 2).mean().sqrt()) + (n + 2) * U64 * r64
            ck.le(f"rms of slab lane {i} against fp64 throughout [norm_{kind}_rms64] error / bound", abs(math.sqrt(float(slab[:, i].sum()) / n) - r64) / bound, 1.0)
            if c.mode == NORM_ERROR:
                ck.true("the ratio is away from 1", abs(r64 - 1) > 1e-3)
                ck.le("state RATIO against fp64 throughout [norm_error_ratio64] error / bound", abs(float(state[DP_RATIO]) - r64) / bound, 1.0)
    if c.mode != NORM_ERROR and c.n <= SMALL_N[-1]:
        # ode_ref in fp32: the same element terms; its rms squares (1), sums (n - 1), divides (1) and takes the root (1) in fp32 where
        # the kernel rounds once (1): (n + 1) / 2 + 2 on d0, d1 and d2; h0 = 0.01 d0 / d1 carries two of them and two roundings of its
        # own on either side: (n + 9) u
        h0, dt = reference_initial_step(c, inp)
        nk = c.kept
        if c.mode == NORM_INIT0:
            ck.rel("state H0 against ode_ref._select_initial_step [norm_init0_ref]", state[DP_H0], h0, (nk + 9) * U)
        else:  # dt = min(100 h0, h1): 100 h0 carries a rounding more on either side, (n + 11) u; h1 a fifth of d2's ((n + 1) / 2 + 2, the
            # (n + 9) of h0, two for the quotient) and of the two of 0.01 / max through the power, (0.3 n + 3.1) u, then RHO_POW here,
            # 2 u (one ulp) for torch's pow and the rounding of the result: the larger of the two arms covers both
            ck.rel("state DT against ode_ref._select_initial_step [norm_init1_ref]", state[DP_DT], dt, (nk + 11) * U + RHO_POW + 2 * U)
    ck.done()


# ---- the powf sweep: INIT1 at n = 4, y0 = 0, atol = 1, f1 - f0 = 2^20 m, H0 = 2^20, D1 = 0: d2 = m exactly, DT = powf(0.01f / m, 0.2f)
def pow_sweep_values():
    lo, hi, step = POW_SWEEP
    return torch.exp2(lo + step * torch.arange(int((hi - lo) / step) + 1, dtype=F64)).float()


def pow_sweep_operands(m):
    z = torch.zeros(4)
    return dict(state=state_buf("own", ATOL=1.0, RTOL=0.0, H0=2.0 ** 20, D1=0.0, NFE=0.0), slab=out_buf(2, F64), y0=with_guard(z),
                k=[with_guard(z), with_guard(torch.full((4,), float(m) * 2.0 ** 20))])


def pow_sweep_error(m, dt):
    """the relative error of DT against fp64 on the fp32 operands"""
    arg = float(torch.tensor(0.01) / torch.tensor(float(m)))
    want = arg ** float(torch.tensor(1.0) / torch.tensor(5.0))
    return abs(float(dt) - want) / want


# ================================================================================================ D. vbx_ode_commit
@dataclass(frozen=True)
class CommitCase:
    n: int
    last: int
    done: int

    @property
    def name(self):
        return f"commit-n{self.n}-last{self.last}-done{self.done}"


COMMIT_CASES = [CommitCase(n, l, d) for n in SMALL_N for l in (0, 1) for d in (0, 1)] + [CommitCase(N_CAP, 1, 0)]


@lru_cache(maxsize=2)
def commit_inputs(c):
    g = _gen(("commit",) + astuple(c))
    return {k: torch.randn(c.n, generator=g) for k in ("y", "k1", "y1", "k7")}


def commit_operands(c):
    inp = commit_inputs(c)
    return dict(state=state_buf("nan", LAST=float(c.last), DONE=float(c.done)), **{k: with_guard(v) for k, v in inp.items()})


def standin_commit(c, fault=None):
    ops = commit_operands(c)
    if c.last and (not c.done or fault == "done"):
        m = min(c.n, 4 * GRID_CAP) if fault == "cap" else c.n
        ops["y"][:m], ops["k1"][:m] = ops["y1"][:m], ops["k7"][:m]
    return ops


def check_commit(c, got):
    ops = commit_operands(c)
    ck = OdeChecks(c.name)
    copies = c.last == 1 and c.done == 0
    ck.same_bits("y is y1" if copies else "y keeps its bits", got["y"], ops["y1" if copies else "y"])
    ck.same_bits("k1 is k7" if copies else "k1 keeps its bits", got["k1"], ops["k7" if copies else "k1"])
    ck.same_bits("y1 is unchanged", got["y1"], ops["y1"])
    ck.same_bits("k7 is unchanged", got["k7"], ops["k7"])
    ck.done()


# ================================================================================================ E. vbx_ode_dense
C_MID = torch.tensor(ode_ref.DPS_C_MID, dtype=F64).float()
DENSE_T0, DENSE_DT = 0.3, 0.1
DENSE_AT = ("inside", "t1", "t0")  # TEND strictly inside (T0, T1), at T1, at T0
DENSE_INSIDE = 0.37


@dataclass(frozen=True)
class DenseCase:
    n: int
    at: str

    @property
    def name(self):
        return f"dense-n{self.n}-{self.at}"


DENSE_CASES = [DenseCase(n, at) for n in SMALL_N for at in DENSE_AT] + [DenseCase(N_CAP, "inside")]


@lru_cache(maxsize=2)
def dense_inputs(c):
    g = _gen(("dense",) + astuple(c))
    y0 = torch.randn(c.n, generator=g)
    k = [torch.randn(c.n, generator=g) for _ in range(MAX_STAGES)]
    y1 = y0 + f32(DENSE_DT) * torch.randn(c.n, generator=g)
    t1 = DENSE_T0 + DENSE_DT
    tend = {"inside": DENSE_T0 + DENSE_INSIDE * DENSE_DT, "t1": t1, "t0": DENSE_T0}[c.at]
    return dict(y0=y0, y1=y1, k=k, st=dict(T0=DENSE_T0, T1=t1, DT32=f32(DENSE_DT), TEND=tend))


def dense_operands(c):
    inp = dense_inputs(c)
    return dict(state=state_buf("nan", **inp["st"]), out=out_buf(c.n), y0=with_guard(inp["y0"]), y1=with_guard(inp["y1"]),
                k=[with_guard(t) for t in inp["k"]], mid=[float(v) for v in C_MID])


def standin_dense(c, fault=None):
    inp, st = dense_inputs(c), dense_inputs(c)["st"]
    dt = torch.tensor(st["DT32"], dtype=F64).float()
    x = torch.tensor((st["TEND"] - st["T0"]) / (st["T1"] - st["T0"]), dtype=F64).float()
    x2 = x * x
    x3 = x2 * x
    x4 = x3 * x
    u, v, f0, f1 = inp["y0"], inp["y1"], inp["k"][0], inp["k"][-1]
    ym = u + stage_sum(inp["k"], C_MID * dt)
    qa = (2.0 * dt) * (f1 - f0) - 8.0 * (v + u) + 16.0 * ym
    qb = dt * (5.0 * f0 - 3.0 * f1) + 18.0 * u + 14.0 * v - 32.0 * ym
    qc = dt * (f1 - 4.0 * f0) - 11.0 * u - 5.0 * v + 16.0 * ym
    out = dense_operands(c)["out"]
    m = min(c.n, 4 * GRID_CAP) if fault == "cap" else c.n
    out[:m] = (u + (dt * f0) * x + qc * x2 + qb * x3 + qa * x4)[:m]
    return dict(out=out)


def dense_reference(c, inp):
    """(ref, counted): the quartic of ode_ref.interp_fit / interp_evaluate in fp64 on the fp32 inputs"""
    st = inp["st"]
    u, v, k = inp["y0"].double(), inp["y1"].double(), torch.stack(inp["k"], -1).double()
    dt = st["DT32"]
    coef = ode_ref.interp_fit(u, v, k, torch.tensor(dt, dtype=F64), C_MID.double())
    ref = ode_ref.interp_evaluate(coef, *(torch.tensor(st[s], dtype=F64) for s in ("T0", "T1", "TEND")))
    x = abs((st["TEND"] - st["T0"]) / (st["T1"] - st["T0"]))
    f0, f1 = k[..., 0].abs(), k[..., -1].abs()
    e, d, qc, qb, qa = (t.abs() for t in coef)
    # y_mid: as the combination, c_j = mid_j dt a rounded product
    P = (k.abs() * (C_MID.double() * dt).abs()).sum(-1)
    ym = (u + (k * (C_MID.double() * dt)).sum(-1)).abs()
    e_ym = U * ((MAX_STAGES + 1) * P + ym)
    # a, b, c: every term of the sum carries at most two roundings of its own (b's first: 5 f0, 3 f1, their difference, the product:
    # three against |5 f0| + |3 f1|), and each of the additions one of at most the sum of the terms' magnitudes M; y_mid's error enters
    # with the weights 16, 32, 16
    Ma = 2 * dt * (f1 + f0) + 8 * (v.abs() + u.abs()) + 16 * ym
    Mb = dt * (5 * f0 + 3 * f1) + 18 * u.abs() + 14 * v.abs() + 32 * ym
    Mc = dt * (f1 + 4 * f0) + 11 * u.abs() + 5 * v.abs() + 16 * ym
    e_a, e_b, e_c = U * (2 + 2) * Ma + 16 * e_ym, U * (3 + 3) * Mb + 32 * e_ym, U * (2 + 3) * Mc + 16 * e_ym
    # x is rounded once, x^2, x^3, x^4 carry 3, 5, 7 u; every product with a power one more; four additions of at most Mo
    Mo = e + d * x + qc * x ** 2 + qb * x ** 3 + qa * x ** 4
    counted = U * (3 * d * x + 4 * qc * x ** 2 + 6 * qb * x ** 3 + 8 * qa * x ** 4 + 4 * Mo) + e_c * x ** 2 + e_b * x ** 3 + e_a * x ** 4
    return ref, counted


def check_dense(c, got):
    inp = dense_inputs(c)
    ck = OdeChecks(c.name)
    ref, counted = dense_reference(c, inp)
    out = got["out"][: c.n]
    ck.ratio("dense", "out", out, ref, counted)
    if c.at == "t0":
        nz = inp["y0"] != 0
        ck.same_bits("out is y0 at TEND = T0", out[nz], inp["y0"][nz])
    ck.note("out is the fp32 stand-in by bits", bool((raw(out) == raw(standin_dense(c)["out"][: c.n])).all()))
    ck.sentinel_kept("out guard", got["out"][c.n:])
    ck.done()


# ================================================================================================ F. vbx_zero_tail_rows
@dataclass(frozen=True)
class ZeroTailCase:
    B: int
    N: int
    D: int
    lens: tuple

    @property
    def name(self):
        return f"zerotail-B{self.B}-N{self.N}-D{self.D}-" + "_".join(map(str, self.lens))


# the last: 1048600 elements, the second trip starts at 1048576, the boundary of row 1 lies at 131075 * 4 + 131070 * 4 = 1048580
ZERO_TAIL_CASES = [ZeroTailCase(3, 37, D, l) for D in (1, 3, 4, 12) for l in ((0, 37, 20), (37, 1, 36))] + [ZeroTailCase(2, 131075, 4, (7, 131070))]


@lru_cache(maxsize=2)
def zero_tail_input(c):
    g = _gen(("zerotail",) + astuple(c))
    x = torch.randn(c.B, c.N, c.D, generator=g)
    x.view(-1)[:: 5] = NAN  # NaNs among the kept and the dropped
    return x


def zero_tail_operands(c):
    return dict(x=with_guard(zero_tail_input(c)), lens=torch.tensor(c.lens, dtype=I32))


def standin_zero_tail(c, fault=None):
    ops = zero_tail_operands(c)
    x = ops["x"][: c.B * c.N * c.D].view(c.B, c.N, c.D)
    for b, l in enumerate(c.lens):
        x[b, l + (fault == "lens"):] = 0.0
    if fault == "cap":
        ops["x"][GRID_CAP: c.B * c.N * c.D] = zero_tail_input(c).reshape(-1)[GRID_CAP:]
    return ops


def check_zero_tail(c, got):
    x, n = zero_tail_input(c), c.B * c.N * c.D
    ck = OdeChecks(c.name)
    keep = (torch.arange(c.N)[None, :] < torch.tensor(c.lens)[:, None])[:, :, None].expand(c.B, c.N, c.D)
    out = got["x"][:n].view(c.B, c.N, c.D)
    ck.same_bits("kept elements keep their bits", out[keep], x[keep])
    ck.same_bits("dropped elements are +0", out[~keep], torch.zeros(int((~keep).sum())))
    ck.sentinel_kept("x guard", got["x"][n:])
    ck.done()


# ================================================================================================ G. copy and pack kernels
# values the 16-bit stores decide on: beyond +-65504, +-inf, NaN, round-to-nearest-even ties of fp16 and bf16, fp16 subnormals and the
# tie below the smallest of them, -0
SPECIAL = (65504.0, 65505.0, 65519.9, 65520.0, 70000.0, 1e30, -65504.0, -65520.0, -1e30, INF, -INF, NAN, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,
           1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -15, 3 * 2.0 ** -16, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 1e-8, -1e-8, -0.0,
           2.0 ** -14 * (1 - 2.0 ** -12), 3.3895e38, -3.3895e38, 2.0 ** -130)


def to_f16_sat(x, fault=None):
    """f32_to_f16_sat: clamp to +-65504, then round to nearest even; NaN stays NaN"""
    return (x if fault == "nosat" else x.clamp(-65504.0, 65504.0)).to(F16)


def same_16(ck, name, got, want):
    """by bits, any NaN for a NaN"""
    nan = torch.isnan(want)
    ck.true(f"{name}: NaN stays NaN", bool(torch.isnan(got)[nan].all()) and got.shape == want.shape)
    ck.same_bits(name, torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))


def _special(g, *shape):
    x = torch.randn(*shape, generator=g)
    flat = x.view(-1)
    k = min(len(SPECIAL), flat.numel())
    flat[:k] = torch.tensor(SPECIAL[:k], dtype=F64).float()
    if flat.numel() >= 4 * len(SPECIAL):
        flat[-len(SPECIAL):] = torch.tensor(SPECIAL, dtype=F64).float()
    return x


@dataclass(frozen=True)
class PackCase:
    B: int
    N: int
    D: int
    mask: bool
    bf: bool

    @property
    def name(self):
        return f"pack-B{self.B}-N{self.N}-D{self.D}-{'mask' if self.mask else 'nomask'}-{'bf16' if self.bf else 'f16only'}"


PACK_CASES = [PackCase(3, 7, D, m, b) for D in (8, 24, 512) for m in (False, True) for b in (False, True)]
PACK_CASES.append(PackCase(2, 262147, 8, True, True))  # rows D / 4 = 1048588 chunks


@lru_cache(maxsize=2)
def pack_inputs(c):
    g = _gen(("pack",) + astuple(c))
    x, cond = _special(g, c.B * c.N, c.D), _special(g, c.B * c.N, c.D).flip(0)
    mask = (torch.rand(c.B * c.N, generator=g) < 0.4) if c.mask else None
    if c.mask:
        mask[:2] = torch.tensor([True, False])
        cond[mask] = NAN  # a masked row is 0 whatever it holds
    return dict(x=x, cond=cond, mask=mask)


def pack_operands(c):
    inp, n = pack_inputs(c), c.B * c.N * 2 * c.D
    return dict(x=with_guard(inp["x"]), cond=with_guard(inp["cond"]), mask=None if inp["mask"] is None else inp["mask"].to(torch.uint8),
                f16=out_buf(n, F16), bf16=out_buf(n, BF16) if c.bf else None)


def standin_pack(c, fault=None):
    inp, ops = pack_inputs(c), pack_operands(c)
    cond = inp["cond"] if inp["mask"] is None else torch.where(inp["mask"][:, None], torch.zeros(()), inp["cond"])
    cat = torch.cat([inp["x"], cond], 1).reshape(-1)
    m = min(cat.numel(), 8 * GRID_CAP) if fault == "cap" else cat.numel()
    ops["f16"][:m] = to_f16_sat(cat, fault)[:m]
    if c.bf:
        ops["bf16"][:m] = cat.to(BF16)[:m]
    return dict(f16=ops["f16"], bf16=ops["bf16"])


def check_pack(c, got):
    want, n = standin_pack(c), c.B * c.N * 2 * c.D
    ck = OdeChecks(c.name)
    for k in ("f16", "bf16") if c.bf else ("f16",):
        same_16(ck, f"{k} is (x | cond) rounded once", got[k][:n], want[k][:n])
        ck.sentinel_kept(k + " guard", got[k][n:])
    ck.done()


@dataclass(frozen=True)
class StackCase:
    B: int
    N: int
    R: int
    D: int

    @property
    def name(self):
        return f"stack-B{self.B}-N{self.N}-R{self.R}-D{self.D}"


STACK_CASES = [StackCase(2, 5, R, D) for R in (0, 1, 16) for D in (4, 512)]


@lru_cache(maxsize=2)
def stack_inputs(c):
    g = _gen(("stack",) + astuple(c))
    return dict(x=_special(g, c.B, c.N, c.D), reg=_special(g, c.R, c.D).flip(0) if c.R else None)


def stack_operands(c):
    inp = stack_inputs(c)
    return dict(x=with_guard(inp["x"]), reg=None if inp["reg"] is None else with_guard(inp["reg"]), xs=out_buf(c.B * (c.N + c.R) * c.D))


def standin_stack(c, fault=None):
    inp, ops = stack_inputs(c), stack_operands(c)
    xs = ops["xs"][: c.B * (c.N + c.R) * c.D].view(c.B, c.N + c.R, c.D)
    xs[:, c.R:] = inp["x"]
    if c.R:
        xs[: 1 if fault == "reg0" else c.B, : c.R] = inp["reg"]
    return dict(xs=ops["xs"])


def check_stack(c, got):
    want, n = standin_stack(c)["xs"], c.B * (c.N + c.R) * c.D
    ck = OdeChecks(c.name)
    ck.same_bits("xs is (reg | x) per batch row", got["xs"][:n], want[:n])
    ck.sentinel_kept("xs guard", got["xs"][n:])
    ck.done()


UNET_SCALES = (1.0, 2.0 ** -0.5, 0.5)


@dataclass(frozen=True)
class UnetCase:
    kind: str  # cat, split, addskip
    rows: int
    D: int
    scale: float = 1.0
    f16: bool = False
    bf: bool = False

    @property
    def name(self):
        o = ("-f16" if self.f16 else "") + ("-bf16" if self.bf else "")
        return f"unet-{self.kind}-r{self.rows}-D{self.D}-s{self.scale:.3g}{o}"


UNET_CASES = [UnetCase("cat", r, D, s, f, b) for (r, D), s in zip(((5, 4), (3, 260), (7, 12)), UNET_SCALES) for f, b in ((1, 0), (0, 1), (1, 1))]
UNET_CASES += [UnetCase("cat", 5, 4, s, True, True) for s in UNET_SCALES[1:]]
UNET_CASES += [UnetCase("split", r, D, s, bf=b) for (r, D), s in zip(((5, 4), (3, 260)), UNET_SCALES[1:]) for b in (False, True)]
UNET_CASES += [UnetCase("addskip", r, D, bf=b) for r, D in ((1, 4), (3, 260)) for b in (False, True)]


@lru_cache(maxsize=2)
def unet_inputs(c):
    g = _gen(("unet",) + astuple(c))
    if c.kind == "split":
        return dict(dcat=_special(g, c.rows, 2 * c.D))
    return dict(x=_special(g, c.rows, c.D), skip=_special(g, c.rows, c.D).flip(0))


def unet_operands(c):
    inp, n = unet_inputs(c), c.rows * c.D
    if c.kind == "cat":
        return dict(x=with_guard(inp["x"]), skip=with_guard(inp["skip"]), f16=out_buf(2 * n, F16) if c.f16 else None,
                    bf16=out_buf(2 * n, BF16) if c.bf else None)
    if c.kind == "split":
        return dict(dcat=with_guard(inp["dcat"]), dx=out_buf(n), bf16=out_buf(n, BF16) if c.bf else None, dskip=out_buf(n))
    return dict(dx=with_guard(inp["x"]), dskip=with_guard(inp["skip"]), bf16=out_buf(n, BF16) if c.bf else None)


def standin_unet(c, fault=None):
    inp, ops, n = unet_inputs(c), unet_operands(c), c.rows * c.D
    scale = torch.tensor(c.scale, dtype=F64).float()
    if c.kind == "cat":
        cat = torch.cat([inp["x"], inp["skip"] * scale], 1).reshape(-1)
        if c.f16:
            ops["f16"][: 2 * n] = to_f16_sat(cat, fault)
        if c.bf:
            ops["bf16"][: 2 * n] = cat.to(BF16)
        return dict(f16=ops["f16"], bf16=ops["bf16"])
    if c.kind == "split":
        dx = inp["dcat"][:, : c.D].reshape(-1)
        ops["dx"][:n], ops["dskip"][:n] = dx, (inp["dcat"][:, c.D:] * scale).reshape(-1)
    else:
        dx = (inp["x"] + inp["skip"]).reshape(-1)
        ops["dx"][:n] = dx
    if c.bf:
        ops["bf16"][:n] = dx.to(BF16)
    return dict(dx=ops["dx"], bf16=ops["bf16"], dskip=ops["dskip"])


def check_unet(c, got):
    want, n = standin_unet(c), c.rows * c.D * (2 if c.kind == "cat" else 1)  # addskip: dskip is an operand and keeps its bits
    ck = OdeChecks(c.name)
    for k, w in want.items():
        if w is not None:
            same_16(ck, k, got[k][:n], w[:n])
            ck.sentinel_kept(k + " guard", got[k][n:])
    ck.done()


COPY_COLS_CASES = ((5, 7, 10), (3, 4, 5), (1, 1, 2), (4097, 257, 260))  # (rows, cols, ld_src); the last: rows cols > GRID_CAP


@lru_cache(maxsize=2)
def copy_cols_input(c):
    rows, cols, ld = c
    src = _special(_gen(("copycols",) + c), rows, ld)
    src[:, cols:] = NAN
    return src


def standin_copy_cols(c, fault=None):
    rows, cols, ld = c
    out = out_buf(rows * cols)
    out[: rows * cols] = (copy_cols_input(c).reshape(-1)[: rows * cols] if fault == "ld" else copy_cols_input(c)[:, :cols].reshape(-1))
    return dict(dst=out)


def check_copy_cols(c, got):
    rows, cols, ld = c
    ck = OdeChecks(f"copycols-r{rows}-c{cols}-ld{ld}")
    same_16(ck, "dst is src[:, :cols]", got["dst"][: rows * cols], copy_cols_input(c)[:, :cols].reshape(-1))
    ck.sentinel_kept("dst guard", got["dst"][rows * cols:])
    ck.done()
