"""Reference, fp32 stand-in, bound and inputs of the EMA tests (tests/test_ema_check_cpu.py checks the checks on the CPU,
tests/test_ema_gpu.py launches every case).  torch on the CPU only: nothing here touches the library or a device.

The average is kept inside the Adam launches (include/vbx.h "EMA"): the thread that stores the updated fp32 weight p' computes
    e' = fmaf(d, e - p', p')
and stores it as fp32.  The check is teacher-forced: it takes the p' the device stored and the previous e, so the Adam arithmetic (whose
own bounds tests/optim_check.py counts) does not enter.  Per element a correct kernel obeys
    |e' - exact| <= u (d |e - p'| + |exact|),   exact = p' + d (e - p') in fp64,   u = 2^-24
-- the subtraction's rounding times d, and the rounding of the fused multiply-add -- and three rules that take no tolerance: d == 0
stores the bits of p'; e == p' stores the bits of p'; an element the launch does not touch keeps its bits.

The cases are those of optim_check (PACKED_CASES on TABLES "edges" and "forms", FACTOR_CASES, and the plain kernel at PLAIN_NS), each at
the three decays DECAYS.  The previous average is e = p + 0.01 * randn (an average sits near its weights; E_SCALE is set here, before
anything ran on a device, so that the smallest planted fault of test_ema_check_cpu.py moves some element by more than 10 bounds), and
exactly e = p on every second element whose g = m = v = 0: Adam leaves p' = p there, so e == p' is known in advance.
"""
import math
from functools import lru_cache

import torch

import optim_check as oc
from optim_check import F32, U, bits, sentinel

EMA_STEPS = oc.STEPS


def f32(x):
    return float(torch.tensor(x, dtype=F32))


DECAYS = (f32(0.0), f32(0.9), f32(0.9999))  # as the C ABI receives them: exactly converted fp32
E_SCALE = 0.01
PLAIN_NS = (1, 5, 8191, 8193)
SWAP_CASES = ((1, 0, 0), (3, 0, 0), (4, 0, 0), (1027, 0, 0), (3, 1, 1), (4, 1, 2), (1027, 4, 4), (1027, 3, 0), (1027, 4, 8))  # n, offsets of a, b


# ------------------------------------------------------------------------------------------------ reference, stand-in
def ema_reference(p_new, e_old, d):
    """(exact, bound) in fp64 from the exactly converted fp32 p', e and d."""
    p, e, d = p_new.double(), e_old.double(), float(d)
    exact = p + d * (e - p)
    return exact, U * (d * (e - p).abs() + exact.abs())


def fma32(a, x, y):
    """fl32(a * x + y) for fp32 tensors: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32
    (a double rounding that differs from a true fma only at an fp32 tie seen through 29 more bits)."""
    return (a.double() * x.double() + y.double()).float()


def ema_standin(p_new, e_old, d, fault=None, p_old=None):
    """e' = fmaf(d, e - p', p') in torch float32: what a correct kernel may answer.  Planted faults:
    "pre_adam"  the average takes the weight of before the Adam update (p_old);
    "swapped"   d and 1 - d exchanged;
    "fp16"      the stored average rounded through fp16."""
    dd = torch.tensor(d, dtype=F32)
    p = p_old if fault == "pre_adam" else p_new
    if fault == "swapped":
        dd = torch.tensor(1.0, dtype=F32) - dd
    out = fma32(dd, e_old - p, p)
    if fault == "fp16":
        out = out.half().float()
    return out


def standin_state(p_new, e_old, d, touched, fault=None, p_old=None, tails=()):
    """The whole buffer as a launch leaves it: the stand-in where `touched`, the old bits elsewhere.  Further planted faults:
    "frozen"  an untouched range is overwritten (the first run of untouched elements gets the update as well);
    "tail"    the elements listed in `tails` (the last element of every ragged tail) are skipped."""
    touched = touched.clone()
    if fault == "frozen":
        first = int((~touched).nonzero()[0])
        touched[first: first + 4] = True
    if fault == "tail":
        assert len(tails) > 0
        touched[torch.as_tensor(list(tails))] = False
    new = ema_standin(p_new, e_old, d, fault, p_old)
    return torch.where(touched, new, e_old)


# ------------------------------------------------------------------------------------------------ the check
def ema_ratios(p_new, e_old, e_new, d):
    exact, bound = ema_reference(p_new, e_old, d)
    return oc.ratios(e_new, exact, bound)


def check_ema(name, p_new, e_old, e_new, d, touched=None, done=True):
    """e_new against the teacher-forced reference where `touched` (a bool mask; None: everywhere), bit-equal to e_old elsewhere; the
    exact rules.  Returns the OptimChecks (done=False: the caller adds checks and calls .done())."""
    ck = oc.OptimChecks(name)
    if touched is None:
        touched = torch.ones_like(p_new, dtype=torch.bool)
    ck.true("ema untouched outside the launch keeps its bits", bool((bits(e_new)[~touched] == bits(e_old)[~touched]).all()))
    p, e0, e1 = p_new[touched], e_old[touched], e_new[touched]
    ck.true("ema finite", bool(torch.isfinite(e1).all()))
    if p.numel():
        w, idx = oc.worst_tile(ema_ratios(p, e0, e1, d).reshape(-1))
        ck.le(f"ema error / bound at {idx}", w, 1.0)
    if d == 0:
        ck.true("d == 0 stores the bits of p'", bool((bits(e1) == bits(p)).all()))
    same = e0 == p
    ck.true("e == p' stores the bits of p'", bool((bits(e1)[same] == bits(p)[same]).all()))
    if done:
        ck.done()
    return ck


def worst_ratio(p_new, e_old, e_new, d, touched):
    """largest error / bound over the touched elements (inf when an exact rule is what fails): how far a planted fault moves"""
    r = ema_ratios(p_new[touched], e_old[touched], e_new[touched], d)
    return float(torch.where(torch.isnan(r), torch.full_like(r, math.inf), r).max())


# ------------------------------------------------------------------------------------------------ inputs
def ema_initial(key, inp, covered):
    """The previous average for the flat inputs `inp` (optim_check.flat_inputs): p + E_SCALE * randn where a segment maps, exactly p on
    every second element with g = m = v = 0 (Adam leaves those p), random fp32 of order 1 -- not a sentinel -- everywhere else."""
    gen = oc._gen(("ema",) + tuple(key))
    N = inp["p"].numel()
    e = inp["p"] + E_SCALE * torch.randn(N, generator=gen)
    z = (inp["g"] == 0) & (inp["m"] == 0) & (inp["v"] == 0) & (torch.arange(N) % 22 == 0)
    e = torch.where(z, inp["p"], e)
    return torch.where(covered, e, torch.randn(N, generator=gen))


@lru_cache(maxsize=4)
def packed_ema(case):
    t = oc.TABLES[case.table]
    return ema_initial(("packed", case.name), oc.packed_inputs(case), t.covered())


def packed_tails(table):
    """the last element of every segment whose count is no multiple of 4 (what the scalar arm's last group stores)"""
    return [s["off"] + s["count"] - 1 for s in table.segs if s["rowmap"] != 2 and s["count"] % 4]


@lru_cache(maxsize=4)
def factor_ema(case):
    lay, inp = oc.factor_inputs(case)
    return ema_initial(("factor", case.name), inp, oc.factor_covered(lay))


@lru_cache(maxsize=8)
def plain_inputs(n):
    """p, g, m, v, e of the plain kernel at n elements, behind them a guard the launch must not touch"""
    cov = torch.zeros(n + oc.GUARD, dtype=torch.bool)
    cov[:n] = True
    inp = oc.flat_inputs(("plain", n), n, cov)
    inp["e"] = ema_initial(("plain", n), inp, cov)
    return inp, cov


def swap_inputs(n, oa, ob):
    """two buffers with sentinels around the n elements at offsets oa, ob (floats from a 16-byte aligned base)"""
    gen = oc._gen(("swap", n, oa, ob))
    a, b = sentinel(oa + n + oc.GUARD, F32), sentinel(ob + n + oc.GUARD, F32)
    a[oa: oa + n] = torch.randn(n, generator=gen)
    b[ob: ob + n] = torch.randn(n, generator=gen)
    return a, b
