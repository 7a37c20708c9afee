"""CPU restatement of torchdiffeq.odeint for the methods the sampler serves: euler, midpoint, rk4 and dopri5.

torchdiffeq is third-party and not installed with the tests, so this restates its published algorithms, the way
oracle/ref_loader.odeint_fixed_grid_midpoint restates midpoint.  PARITY UNPINNED: no reference test or golden vector pins the
library's solvers, so agreement with torchdiffeq itself is not asserted anywhere; what is asserted is that the device samplers
(voicebox_pytorch_amd/solver.py) agree with THIS restatement, and that the restatement agrees with textbook convergence orders,
analytic solutions and scipy's RK45 where the two algorithms coincide.

* Fixed grids (FixedGridODESolver): the grid is t itself; per interval dt = t1 - t0 and y1 = y0 + dy.
  euler dy = dt f(t0, y0); midpoint dy = dt f(t0 + dt/2, y0 + f0 dt/2); rk4 is the 3/8 rule (rk4_alt_step_func).
* dopri5 (RKAdaptiveStepsizeODESolver, Dormand-Prince-Shampine, FSAL, order 5): times and step sizes in float64, stage arithmetic in
  the state's dtype, stages with c = 1 at the fp32 value below t0 + dt (Perturb.PREV), Hairer's initial step, the RMS norm over the
  whole state, safety 0.9 / ifactor 10 / dfactor 0.2, no clipping at the end: the result is the dense-output quartic at t[-1].

Only trajectory[-1] is returned (the reference keeps only that, voicebox_pytorch.py:1295-1296).
"""
import torch

METHODS = ("euler", "midpoint", "rk4", "dopri5")

_one_third = 1 / 3
_two_thirds = 2 / 3

DPS_ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.]
DPS_BETA = [[1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
            [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656], [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
DPS_C_SOL = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
DPS_C_ERROR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
               11 / 84 - 649 / 6300, -1. / 60.]
DPS_C_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
             187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


def _rms_norm(x):
    return x.abs().pow(2).mean().sqrt()


def _fixed_step(method, f, t0, dt, t1, y0):
    if method == "euler":
        return dt * f(t0, y0)
    if method == "midpoint":
        half_dt = 0.5 * dt
        f0 = f(t0, y0)
        y_mid = y0 + f0 * half_dt
        return dt * f(t0 + half_dt, y_mid)
    k1 = f(t0, y0)  # rk4: rk4_alt_step_func (3/8 rule)
    k2 = f(t0 + dt * _one_third, y0 + dt * k1 * _one_third)
    k3 = f(t0 + dt * _two_thirds, y0 + dt * (k2 - k1 * _one_third))
    k4 = f(t1, y0 + dt * (k1 - k2 + k3))
    return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def _select_initial_step(func, t0, y0, order, rtol, atol, f0):
    scale = atol + torch.abs(y0) * rtol
    d0 = _rms_norm(y0 / scale).abs()
    d1 = _rms_norm(f0 / scale).abs()
    if d0 < 1e-5 or d1 < 1e-5:
        h0 = torch.tensor(1e-6, dtype=y0.dtype)
    else:
        h0 = 0.01 * d0 / d1
    h0 = h0.abs()
    y1 = y0 + h0 * f0
    f1 = func(t0 + h0, y1)
    d2 = torch.abs(_rms_norm((f1 - f0) / scale) / h0)
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = torch.max(torch.tensor(1e-6, dtype=y0.dtype), h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1. / float(order + 1))
    h1 = h1.abs()
    return torch.min(100 * h0, h1).to(t0.dtype)


def _optimal_step_size(last_step, error_ratio, safety=0.9, ifactor=10.0, dfactor=0.2, order=5):
    if error_ratio == 0:
        return last_step * ifactor
    dfactor = torch.tensor(1.0 if error_ratio < 1 else dfactor, dtype=last_step.dtype)
    error_ratio = error_ratio.type_as(last_step)
    exponent = torch.tensor(order, dtype=last_step.dtype).reciprocal()
    factor = torch.min(torch.tensor(ifactor, dtype=last_step.dtype), torch.max(safety / error_ratio ** exponent, dfactor))
    return last_step * factor


def dopri5_step(func, y0, f0, t0, dt, tab):
    """One attempt (_runge_kutta_step): the 5th-order y1, k7 = f(t1, y1), the embedded error and the stage matrix k [..., 7]."""
    t1 = t0 + dt
    t0, dt, t1 = t0.to(y0.dtype), dt.to(y0.dtype), t1.to(y0.dtype)
    k = [f0]
    yi = y0
    for alpha_i, beta_i in zip(tab["alpha"], tab["beta"]):
        if alpha_i == 1.:
            ti, prev = t1, True
        else:
            ti, prev = t0 + alpha_i * dt, False
        yi = y0 + torch.stack(k, dim=-1).matmul(beta_i * dt).view_as(f0)
        k.append(func(ti, yi, prev))
    k = torch.stack(k, dim=-1)
    return yi, k[..., -1], k.matmul(dt * tab["c_error"]), k


def _tableau(dtype):
    return {"alpha": torch.tensor(DPS_ALPHA, dtype=torch.float64).to(dtype),
            "beta": [torch.tensor(b, dtype=torch.float64).to(dtype) for b in DPS_BETA],
            "c_error": torch.tensor(DPS_C_ERROR, dtype=torch.float64).to(dtype),
            "mid": torch.tensor(DPS_C_MID, dtype=torch.float64).to(dtype)}


def interp_fit(y0, y1, k, dt, mid):
    """_interp_fit: the quartic's coefficients [e, d, c, b, a] of y(x) = e + d x + c x^2 + b x^3 + a x^4 on the step [t0, t0 + dt]."""
    dt = dt.type_as(y0)
    y_mid = y0 + k.matmul(dt * mid).view_as(y0)
    f0, f1 = k[..., 0], k[..., -1]
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
    b = dt * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
    c = dt * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
    d = dt * f0
    e = y0
    return [e, d, c, b, a]


def interp_evaluate(coefficients, t0, t1, t):
    assert (t0 <= t) & (t <= t1), (t0, t, t1)
    x = ((t - t0) / (t1 - t0)).type(coefficients[0].dtype)
    xs = [torch.tensor(1).type(coefficients[0].dtype), x]
    for _ in range(2, len(coefficients)):
        xs.append(xs[-1] * x)
    total = coefficients[0] * xs[0]
    for coefficient, x_power in zip(coefficients[1:], xs[1:]):
        total = total + coefficient * x_power
    return total


def odeint(fn, y0, t, *, atol=1e-5, rtol=1e-5, method="midpoint", stats=None, max_attempts=10000):
    """odeint(fn, y0, t, atol=, rtol=, method=)[-1].  stats (a dict, optional) receives "method", "nfe", "accepted", "rejected" and,
    for dopri5, "h0" (the first step) and "trace": (t0, dt, error ratio, accepted) of every attempt."""
    if method not in METHODS:
        raise NotImplementedError(f"ode_ref: method {method!r} is not restated (have {METHODS})")
    nfe = [0]

    def f(tt, yy):
        nfe[0] += 1
        return fn(tt, yy)

    st = {"method": method}
    if method != "dopri5":
        y = y0
        for i in range(t.shape[0] - 1):
            t0, t1 = t[i], t[i + 1]
            y = y + _fixed_step(method, f, t0, t1 - t0, t1, y)
        st.update(nfe=nfe[0], accepted=t.shape[0] - 1, rejected=0)
        if stats is not None:
            stats.update(st)
        return y

    dtype = torch.promote_types(torch.float64, y0.dtype)
    t = t.to(dtype)
    rtol_t, atol_t = torch.as_tensor(rtol, dtype=dtype), torch.as_tensor(atol, dtype=dtype)
    tab = _tableau(y0.dtype)

    def func(tt, yy, prev=False):
        tt = tt.to(yy.dtype)
        if prev:
            tt = torch.nextafter(tt, tt - 1)  # Perturb.PREV
        return f(tt, yy)

    t0 = t[0]
    f0 = func(t0, y0)
    dt = _select_initial_step(func, t0, y0, 4, rtol_t, atol_t, f0)
    st["h0"] = float(dt)
    y, fy, tl0, tl1, coeff = y0, f0, t0, t0, None
    trace, attempts = [], 0
    out = y0
    for next_t in t[1:]:
        while next_t > tl1:
            if attempts >= max_attempts:
                raise RuntimeError(f"ode_ref dopri5: {attempts} attempts without reaching {float(next_t)}")
            attempts += 1
            ts = tl1
            if not (ts + dt > ts):
                raise RuntimeError(f"underflow in dt {dt.item()}")
            if not torch.isfinite(y).all():
                raise RuntimeError("non-finite values in state `y`")
            y1, f1, err, k = dopri5_step(func, y, fy, ts, dt, tab)
            error_tol = atol_t + rtol_t * torch.max(y.abs(), y1.abs())
            ratio = _rms_norm(err / error_tol)
            accept = bool(ratio <= 1)
            trace.append((float(ts), float(dt), float(ratio), accept))
            dt_next = _optimal_step_size(dt, ratio)
            if accept:
                coeff = interp_fit(y, y1, k, dt, tab["mid"])
                y, fy, tl0, tl1 = y1, f1, ts, ts + dt
            else:
                tl0, tl1 = ts, ts
            dt = dt_next
        out = interp_evaluate(coeff, tl0, tl1, next_t)
    st.update(nfe=nfe[0], accepted=sum(a for *_, a in trace), rejected=sum(not a for *_, a in trace), trace=trace)
    if stats is not None:
        stats.update(st)
    return out
