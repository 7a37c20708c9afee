"""The checks of the EMA tests (tests/ema_check.py) checked on the CPU: the decay schedule at hand-computed points, the fp32 stand-in
passing check_ema on every input tests/test_ema_gpu.py launches, and each planted fault failing on those inputs.

Measured on the CPU (python -m pytest tests/test_ema_check_cpu.py -s prints them): the stand-in's worst error / bound over all inputs is
0.999 -- the bound counts exactly its two roundings, and among 10^5 elements one meets both at the bottom of a binade.  How far each
planted fault moves the worst element of a family (packed "edges", packed "forms", factor, plain), in bounds; the smallest figure of
each fault is at d = 0.9999, where 1 - d scales the fault down:
    scalar tail skipped       13.6  (plain: one element; "forms" 143, "edges" 664)
    average from p before     3.2e3 (plain; "forms" 6.6e3, "edges" 1.3e4, factor 2.2e4)
    e rounded through fp16    8.0e3 (every family, every decay)
    d and 1 - d exchanged     1.5e7 (at d = 0.9; 1.7e7 at 0.9999, > 1e9 at d = 0)
    frozen range overwritten  fails the bit rule of untouched elements, not a bound
A case of one element (plain n = 1, whose g = m = v = 0 and so p' = p) cannot show every fault; each fault must fail in some case of
every family at every decay, and move some element there by at least MIN_FACTOR bounds.
"""
import math

import pytest
import torch

import ema_check as ec
import optim_check as oc
from ema_check import DECAYS, PLAIN_NS
from optim_check import FACTOR_CASES, PACKED_CASES, TABLES
from voicebox_pytorch_amd.dp import check_ema_hyper, ema_decay_at

FAULTS = ("pre_adam", "swapped", "fp16", "frozen", "tail")
MIN_FACTOR = 10.0  # the smallest fault must move some element of every family by this many bounds


# ------------------------------------------------------------------------------------------------ the schedule
def test_ema_decay_at_hand_computed_points():
    # t at, just below and just above update_after_step
    assert ema_decay_at(4, 0.9, 5) == 0.0 and ema_decay_at(5, 0.9, 5) == 0.0 and ema_decay_at(6, 0.9, 5) == 0.9
    assert ema_decay_at(1, 0.9) == 0.9 and ema_decay_at(0, 0.9) == 0.0  # update_after_step = 0: every step averages
    # power=None: the constant, whatever inv_gamma says
    assert ema_decay_at(100, 0.9999, 0, 7.0, None) == 0.9999
    # the warm-up: k = t - update_after_step; 1 - (1 + k / inv_gamma) ** -power
    assert ema_decay_at(1, 0.9999, 0, 1.0, 1.0) == 0.5                      # 1 - 1 / 2
    assert ema_decay_at(3, 0.9999, 0, 1.0, 1.0) == 0.75                     # 1 - 1 / 4
    assert ema_decay_at(5, 0.9999, 2, 1.0, 1.0) == 0.75                     # k = 3
    assert ema_decay_at(3, 0.9999, 0, 1.0, 0.5) == 0.5                      # 1 - 4 ** -1/2
    assert ema_decay_at(6, 0.9999, 0, 2.0, 2.0) == 1.0 - 1.0 / 16.0         # 1 - (1 + 3) ** -2
    assert math.isclose(ema_decay_at(10, 0.9999, 0, 1.0, 2 / 3), 1.0 - 11.0 ** (-2 / 3), rel_tol=1e-15)
    # the clamp at ema_decay
    assert ema_decay_at(3, 0.7, 0, 1.0, 1.0) == 0.7 and ema_decay_at(10 ** 9, 0.9999, 0, 1.0, 1.0) == 0.9999
    assert ema_decay_at(2, 0.0, 0, 1.0, 1.0) == 0.0


@pytest.mark.parametrize("hyper", [(0.9999, 0, 1.0, None), (0.9999, 10, 1.0, 2 / 3), (0.9, 3, 5.0, 1.0), (0.5, 0, 0.25, 3.0), (0.0, 2, 1.0, 1.0)])
def test_ema_decay_at_is_non_decreasing(hyper):
    vals = [ema_decay_at(t, *hyper) for t in range(0, 3000)]
    assert all(b >= a for a, b in zip(vals, vals[1:])) and all(0.0 <= v <= hyper[0] for v in vals)
    assert vals[-1] == hyper[0] or hyper[3] is not None


def test_hyper_parameter_refusals():
    check_ema_hyper(None, -3, -1.0, -1.0)  # off: nothing to check
    check_ema_hyper(0.0)
    check_ema_hyper(0.9999, 10, 1.0, 2 / 3)
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=1.5), dict(ema_decay="0.9"), dict(ema_decay=float("nan")),
                dict(ema_decay=0.9, ema_power=0.0), dict(ema_decay=0.9, ema_power=-1.0), dict(ema_decay=0.9, ema_inv_gamma=0.0),
                dict(ema_decay=0.9, ema_update_after_step=-1)):
        with pytest.raises(ValueError):
            check_ema_hyper(**bad)


# ------------------------------------------------------------------------------------------------ the reference and the rules
def test_reference_and_exact_rules_of_the_standin():
    p = torch.tensor([0.5, -0.25, 3.0, 1e-3])
    e = torch.tensor([0.75, -0.25, 1.0, 0.0])
    exact, bound = ec.ema_reference(p, e, 0.5)
    assert exact.tolist() == [0.625, -0.25, 2.0, torch.tensor(1e-3).double().item() / 2]
    assert bound[0].item() == oc.U * (0.5 * 0.25 + 0.625) and bound[1].item() == oc.U * 0.25
    assert torch.equal(oc.bits(ec.ema_standin(p, e, 0.0)), oc.bits(p))  # d == 0
    assert oc.bits(ec.ema_standin(p, e, DECAYS[2]))[1] == oc.bits(p)[1]  # e == p'
    with pytest.raises(AssertionError, match="d == 0 stores the bits"):
        ec.check_ema("rule", p, e, torch.nextafter(p, 2 * p), 0.0)
    with pytest.raises(AssertionError, match="e == p' stores the bits"):
        bad = ec.ema_standin(p, e, 0.5)
        bad[1] = torch.nextafter(bad[1], torch.tensor(0.0))
        ec.check_ema("rule", p, e, bad, 0.5)


# ------------------------------------------------------------------------------------------------ stand-in and planted faults
def _packed(case):
    t, inp = TABLES[case.table], oc.packed_inputs(case)
    return dict(p_old=inp["p"], p_new=oc.standin_packed(case)["p"], e_old=ec.packed_ema(case), touched=t.covered(),
                tails=ec.packed_tails(t), faults=FAULTS)


def _factor(case):
    lay, inp = oc.factor_inputs(case)
    return dict(p_old=inp["p"], p_new=oc.standin_factor(case)["p"], e_old=ec.factor_ema(case), touched=oc.factor_covered(lay), tails=(),
                faults=FAULTS[:4])


def _plain(n):
    inp, cov = ec.plain_inputs(n)
    p1 = torch.where(cov, oc.adam_standin(inp["p"], inp["g"], inp["m"], inp["v"], oc.GSCALES[1], 2)[0], inp["p"])
    return dict(p_old=inp["p"], p_new=p1, e_old=inp["e"], touched=cov, tails=(n - 1,), faults=FAULTS)


GROUPS = {}  # (family, fault, d) -> largest error / bound a fault reached in any case of the family
for _t in TABLES:
    GROUPS[f"packed-{_t}"] = [(c.name, _packed, c) for c in PACKED_CASES if c.table == _t]
GROUPS["factor"] = [(c.name, _factor, c) for c in FACTOR_CASES]
GROUPS["plain"] = [(f"plain-n{n}", _plain, n) for n in PLAIN_NS]


@pytest.mark.parametrize("family", sorted(GROUPS))
def test_standin_passes_and_planted_faults_fail(family):
    moved, worst_ok, caught = {}, 0.0, set()
    for name, make, arg in GROUPS[family]:
        c = make(arg)
        if family != "factor" and int(c["touched"].sum()) >= 64:  # e == p' is met (the factor kernel's gradient is never zero)
            assert int((c["e_old"][c["touched"]] == c["p_new"][c["touched"]]).sum()) > 0
        for d in DECAYS:
            ok = ec.standin_state(c["p_new"], c["e_old"], d, c["touched"])
            ec.check_ema(f"{name}-d{d}", c["p_new"], c["e_old"], ok, d, c["touched"])
            worst_ok = max(worst_ok, ec.worst_ratio(c["p_new"], c["e_old"], ok, d, c["touched"]))
            for fault in c["faults"]:
                bad = ec.standin_state(c["p_new"], c["e_old"], d, c["touched"], fault, p_old=c["p_old"], tails=c["tails"])
                try:  # (a case of one element, whose g = m = v = 0, cannot show every fault: each must fail somewhere in the family)
                    ec.check_ema(f"{name}-d{d}-{fault}", c["p_new"], c["e_old"], bad, d, c["touched"])
                except AssertionError:
                    caught.add((fault, d))
                if fault != "frozen":  # (that one breaks the bit rule of untouched elements, not a bound)
                    key = (fault, d)
                    moved[key] = max(moved.get(key, 0.0), ec.worst_ratio(c["p_new"], c["e_old"], bad, d, c["touched"]))
    print(f"{family}: stand-in worst error / bound {worst_ok:.3f}; faults move by "
          + ", ".join(f"{f} d={d:.4f}: {v:.3g}" for (f, d), v in sorted(moved.items())))
    assert worst_ok <= 1.0
    faults = GROUPS[family][0][1](GROUPS[family][0][2])["faults"]
    assert caught == {(f, d) for f in faults for d in DECAYS}, "a planted fault passed every case of the family"
    assert min(moved.values()) >= MIN_FACTOR, min(moved.items(), key=lambda kv: kv[1])


def test_swap_inputs_keep_their_guards():
    for n, oa, ob in ec.SWAP_CASES:
        a, b = ec.swap_inputs(n, oa, ob)
        sent = oc.SENTINEL[torch.float32][1]
        assert bool((oc.bits(a)[:oa] == sent).all()) and bool((oc.bits(a)[oa + n:] == sent).all()) and a.numel() == oa + n + oc.GUARD
        assert bool(torch.isfinite(a[oa: oa + n]).all()) and bool(torch.isfinite(b[ob: ob + n]).all())
    assert {n for n, _, _ in ec.SWAP_CASES} == {1, 3, 4, 1027} and any(oa % 4 or ob % 4 for _, oa, ob in ec.SWAP_CASES)
