"""The CPU restatement of torchdiffeq's euler / midpoint / rk4 / dopri5 (tests/ode_ref.py) against independent statements: the
oracle's midpoint, textbook convergence orders, analytic solutions and scipy's RK45, which shares dopri5's initial step, stages,
5th-order weights and RMS norm.  Also: the wrapper accepts exactly the methods the device serves."""
import math

import numpy as np
import pytest
import torch

import ode_ref


def _linear(c0, c1):
    return lambda t, y: (c0 + c1 * t) * y


def _exact(c0, c1, y0, t1=1.0):
    return y0 * math.exp(c0 * t1 + 0.5 * c1 * t1 * t1)


def test_restated_midpoint_is_the_oracles_bit_for_bit():
    from oracle.ref_loader import odeint_fixed_grid_midpoint

    g = torch.Generator().manual_seed(0)
    W = torch.randn(16, 16, generator=g) * 0.3
    fn = lambda t, y: torch.tanh(y @ W) * (1 + t)
    y0 = torch.randn(3, 16, generator=g)
    for steps in (2, 5, 17, 64):
        t = torch.linspace(0, 1, steps)
        ref = odeint_fixed_grid_midpoint(fn, y0, t, method="midpoint")[-1]
        got = ode_ref.odeint(fn, y0, t, method="midpoint")
        assert torch.equal(got, ref), steps


@pytest.mark.parametrize("method,order", [("euler", 1), ("rk4", 4)])
def test_fixed_grid_convergence_order(method, order):
    c0, c1 = -1.3, 0.7
    y0 = torch.tensor([1.0, -0.5], dtype=torch.float64)
    errs = []
    for n in (8, 16, 32):
        st = {}
        y = ode_ref.odeint(_linear(c0, c1), y0, torch.linspace(0, 1, n + 1, dtype=torch.float64), method=method, stats=st)
        assert st["nfe"] == n * (1 if method == "euler" else 4)
        errs.append(float((y - _exact(c0, c1, y0)).abs().max()))
    rates = [math.log2(errs[i] / errs[i + 1]) for i in range(2)]
    assert all(abs(r - order) < 0.25 for r in rates), (method, errs, rates)


def test_rk4_is_the_three_eighths_rule():
    """One step on y' = t^3 (exact for a 4th-order rule) and on a problem where the 3/8 rule and the classic RK4 differ."""
    y0 = torch.zeros(1, dtype=torch.float64)
    y = ode_ref.odeint(lambda t, y: t ** 3 + 0 * y, y0, torch.tensor([0.0, 1.0], dtype=torch.float64), method="rk4")
    assert abs(float(y) - 0.25) < 1e-15
    fn = lambda t, y: -2.0 * y + torch.sin(3 * t)
    y0 = torch.ones(1, dtype=torch.float64)
    h = 0.5
    k1 = fn(torch.tensor(0.0, dtype=torch.float64), y0)
    k2 = fn(torch.tensor(h / 3, dtype=torch.float64), y0 + h * k1 / 3)
    k3 = fn(torch.tensor(2 * h / 3, dtype=torch.float64), y0 + h * (k2 - k1 / 3))
    k4 = fn(torch.tensor(h, dtype=torch.float64), y0 + h * (k1 - k2 + k3))
    want = y0 + h * (k1 + 3 * (k2 + k3) + k4) / 8
    got = ode_ref.odeint(fn, y0, torch.tensor([0.0, h], dtype=torch.float64), method="rk4")
    assert abs(float(got - want)) < 1e-15


def _scipy_first_attempt(lam, y0, rtol, atol):
    from scipy.integrate import RK45
    from scipy.integrate._ivp.rk import rk_step

    f = lambda t, y: lam * y
    s = RK45(f, 0.0, y0, t_bound=1.0, rtol=rtol, atol=atol)
    h = s.h_abs
    K = np.empty((s.n_stages + 1, y0.size))
    y_new, _ = rk_step(s.fun, 0.0, y0, s.f, h, s.A, s.B, s.C, K)
    scale = atol + np.maximum(np.abs(y0), np.abs(y_new)) * rtol
    err = K.T @ s.E * h / scale
    return h, y_new, float(np.linalg.norm(err) / err.size ** 0.5)


def test_dopri5_first_attempt_matches_scipy_rk45():
    """Hairer's initial step, the DOPRI5 stages and 5th-order weights and the RMS norm are shared with scipy's RK45; the error
    weights are -2/3 of scipy's E (so the ratio is exactly 2/3 of scipy's error norm).  Only the first attempt is compared: the
    controllers differ (scipy also shrinks after an accepted step, and clips at t_bound)."""
    from ode_ref import _select_initial_step, _tableau, dopri5_step, _rms_norm

    lam = np.array([-0.4, -1.0, -2.5, 0.3, -6.0])
    y0 = np.array([1.0, -0.7, 0.4, 2.0, 0.9])
    rtol, atol = 1e-5, 1e-6
    h_s, y1_s, en_s = _scipy_first_attempt(lam, y0, rtol, atol)
    lam_t, y0_t = torch.tensor(lam), torch.tensor(y0)
    fn = lambda t, y: lam_t * y
    func = lambda t, y, prev=False: fn(t, y)
    t0 = torch.tensor(0.0, dtype=torch.float64)
    f0 = fn(t0, y0_t)
    rt, at = torch.tensor(rtol, dtype=torch.float64), torch.tensor(atol, dtype=torch.float64)
    h = _select_initial_step(func, t0, y0_t, 4, rt, at, f0)
    assert float(h) < 1.0
    y1, _, err, _ = dopri5_step(func, y0_t, f0, t0, h, _tableau(torch.float64))
    ratio = float(_rms_norm(err / (at + rt * torch.max(y0_t.abs(), y1.abs()))))
    print("h", float(h), h_s, "y1", float((y1 - torch.tensor(y1_s)).abs().max()), "ratio", ratio, en_s)
    assert abs(float(h) - h_s) <= 1e-12 * h_s
    assert float((y1 - torch.tensor(y1_s)).abs().max()) <= 1e-12
    # exactly 2/3 in exact arithmetic; the error estimate is a difference of O(1) terms of size ~1e-8, so the two sums (different
    # orders) agree to ~1e-16 / 1e-8 relative: measured 2.2e-11
    assert abs(ratio - 2 / 3 * en_s) <= 1e-9 * en_s
    st = {}
    ode_ref.odeint(fn, y0_t, torch.tensor([0.0, 1.0], dtype=torch.float64), atol=atol, rtol=rtol, method="dopri5", stats=st)
    assert st["h0"] == float(h) and st["trace"][0][1] == float(h) and abs(st["trace"][0][2] - ratio) <= 1e-15 * max(ratio, 1)


def test_dopri5_reaches_the_tolerance_and_rejects():
    # a spread of rates: the first step is too large for the fast ones -> rejections; accuracy ~ tolerance
    lam = torch.tensor([-0.3, -3.0, -20.0, -60.0, 0.5], dtype=torch.float64)
    c1 = 0.5
    y0 = torch.tensor([1.0, -1.0, 0.5, 2.0, 0.25], dtype=torch.float64)
    exact = y0 * torch.exp(lam + 0.5 * c1)
    for tol in (1e-4, 1e-6, 1e-8):  # measured: 24 / 5, 35 / 4, 68 / 1 accepted / rejected
        st = {}
        y = ode_ref.odeint(lambda t, y: (lam + c1 * t) * y, y0, torch.tensor([0.0, 1.0], dtype=torch.float64), atol=tol, rtol=tol,
                           method="dopri5", stats=st)
        err = float((y - exact).abs().max())
        print(tol, err, st["nfe"], st["accepted"], st["rejected"])
        assert err < 30 * tol, (tol, err)
        assert st["nfe"] == 2 + 6 * (st["accepted"] + st["rejected"])
        assert st["trace"][-1][0] + st["trace"][-1][1] >= 1.0  # the last accepted step overshoots / reaches t = 1
        assert st["rejected"] >= 1
    # steps does not change the result (only trajectory[-1] is returned; intermediate points are interpolated)
    ys = [ode_ref.odeint(lambda t, y: (lam + c1 * t) * y, y0, torch.linspace(0, 1, s), method="dopri5") for s in (2, 5)]
    assert torch.equal(ys[0], ys[1])


def test_dopri5_dense_output_reproduces_its_nodes():
    """_interp_fit's quartic passes through y0, y_mid, y1 at x = 0, 1/2, 1 with end slopes dt k1 and dt k7."""
    g = torch.Generator().manual_seed(3)
    y0, y1 = torch.randn(6, dtype=torch.float64, generator=g), torch.randn(6, dtype=torch.float64, generator=g)
    k = torch.randn(6, 7, dtype=torch.float64, generator=g)
    dt = torch.tensor(0.37, dtype=torch.float64)
    mid = torch.tensor(ode_ref.DPS_C_MID, dtype=torch.float64)
    e, d, c, b, a = ode_ref.interp_fit(y0, y1, k, dt, mid)
    y_mid = y0 + k.matmul(dt * mid)
    poly = lambda x: e + d * x + c * x ** 2 + b * x ** 3 + a * x ** 4
    slope = lambda x: d + 2 * c * x + 3 * b * x ** 2 + 4 * a * x ** 3
    for x, want in ((0.0, y0), (0.5, y_mid), (1.0, y1)):
        assert torch.allclose(poly(x), want, atol=1e-12)
    assert torch.allclose(slope(0.0), dt * k[:, 0], atol=1e-12) and torch.allclose(slope(1.0), dt * k[:, -1], atol=1e-12)


def test_dopri5_model_restatement_counts():
    """The issue's CPU data point: on small_wc at the default tolerances the fp32 restatement takes 12 accepted / 1 rejected steps."""
    import os

    from oracle import restate

    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "small_wc.pt"), map_location="cpu", weights_only=False)
    cfg = restate.Cfg(**g["cfg"])
    ones = torch.ones(g["y0"].shape[:2], dtype=torch.bool)
    fn = lambda t, y: restate.forward_with_cond_scale(g["state"], cfg, y, t, g["cond"], ones)
    st = {}
    with torch.no_grad():
        ode_ref.odeint(fn, g["y0"], torch.linspace(0, 1, 3), method="dopri5", stats=st)
    assert (st["accepted"], st["rejected"], st["nfe"]) == (12, 1, 80), st


def test_wrapper_accepts_the_served_methods_only():
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=64, num_cond_tokens=5, depth=2, dim_head=64, heads=2, condition_on_text=False)
    for m in ("euler", "midpoint", "rk4", "dopri5"):
        w = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=m, ode_atol=1e-4, ode_rtol=1e-3)
        assert w.odeint_kwargs == dict(atol=1e-4, rtol=1e-3, method=m)
    for m in ("bosh3", "implicit_adams", "dopri8", "adaptive_heun", "scipy_solver"):
        with pytest.raises(NotImplementedError, match="rk4"):
            vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=m)
    with pytest.raises(NotImplementedError):
        vbx.ConditionalFlowMatcherWrapper(voicebox=vb, use_torchode=True, torchdiffeq_ode_method="dopri5")


def test_ode_ref_rejects_unrestated_methods():
    with pytest.raises(NotImplementedError):
        ode_ref.odeint(lambda t, y: y, torch.ones(2), torch.linspace(0, 1, 3), method="bosh3")
