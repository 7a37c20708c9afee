"""euler, rk4 and dopri5 on the device (solver.RKSampler / solver.Dopri5Sampler, csrc/ode.hip) against the CPU restatement of
torchdiffeq (tests/ode_ref.py -- parity with the library itself UNPINNED, as for midpoint: oracle/ref_loader.py): the kernels on
closed-form problems, then the samplers through the public wrapper on the well-conditioned small_wc network, split, determinism,
guidance and precise mode.  Bounds are measured values with a stated margin."""
import ctypes as C
import math

import pytest
import torch

import ode_ref
from oracle import restate

pytestmark = pytest.mark.gpu
dev = "cuda"


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp(min=1e-30))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_fixed_grid_kernels_integrate_the_closed_form(method):
    """vbx_ode_stage_time + vbx_ode_combine with the sampler's own tables integrate y' = (c0 + c1 t) y to the closed form within the
    method's truncation error, and reproduce the host rule (same tables, torch arithmetic) to fp32 rounding."""
    from voicebox_pytorch_amd import _lib as L
    from voicebox_pytorch_amd.solver import FIXED_TABLEAUS, fixed_grid_tables

    c0, c1 = -1.3, 0.7
    S = len(FIXED_TABLEAUS[method][2])
    for steps in (3, 17, 65):
        t_tab, c_tab = fixed_grid_tables(method, steps)
        t_d, c_d = t_tab.to(dev), c_tab.to(dev)
        B, n = 2, 4096
        y = torch.linspace(-2, 2, B * n, device=dev).view(B, n).contiguous()
        y0 = y.clone()
        ys, times = torch.empty_like(y), torch.zeros(B, device=dev)
        ks = [torch.empty_like(y) for _ in range(S)]
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        yh = y0.cpu()
        for i in range(steps - 1):
            kh = []
            for s in range(S):
                x = y
                if s:
                    x = ys
                    L.call("vbx_ode_combine", ys, y, _ptrs(ks[:s]), s, c_d, S, counter, S, s - 1, y.numel(), _st())
                L.call("vbx_ode_stage_time", times, B, t_d, counter, S, s, _st())
                ks[s].copy_((c0 + c1 * times)[:, None] * x)
                # host: the same rule from the same tables
                th = t_tab[i * S + s]
                xh = yh if s == 0 else yh + sum(kh[j] * c_tab[i * S + s - 1, j] for j in range(s))
                kh.append((c0 + c1 * th) * xh)
            L.call("vbx_ode_combine", y, y, _ptrs(ks), S, c_d, S, counter, S, S - 1, y.numel(), _st())
            L.call("vbx_counter_add", counter, 1, _st())
            yh = yh + sum(kh[j] * c_tab[i * S + S - 1, j] for j in range(S))
        assert int(counter.item()) == steps - 1
        exact = y0.double().cpu() * math.exp(c0 + 0.5 * c1)
        h = 1.0 / (steps - 1)
        trunc = (3.0 * h) if method == "euler" else (0.02 * h ** 4)
        e_exact, e_host = rel(y, exact), rel(y, yh)
        print(method, steps, "vs closed form", e_exact, "vs host rule", e_host)
        assert e_host < 2e-6, (steps, e_host)  # measured 0: the same fp32 operations in the same order
        assert e_exact < trunc + 2e-6, (steps, e_exact, trunc)


def _dp_kernel_run(fn, y0, atol, rtol, max_attempts=1000):
    """dopri5 from the device kernels alone, f evaluated by torch on the device: the same launch sequence as Dopri5Sampler."""
    from voicebox_pytorch_amd import _lib as L
    from voicebox_pytorch_amd import solver as S

    n = y0.numel()
    y = y0.clone()
    ks = [torch.zeros_like(y) for _ in range(7)]
    ys, y1, out = torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y)
    times = torch.zeros(1, device=dev)
    state = torch.zeros(S.DP_STATE, dtype=torch.float64)
    state[S.DP_TEND], state[S.DP_ATOL], state[S.DP_RTOL] = 1.0, atol, rtol
    state = state.to(dev)
    slab = torch.zeros(L.lib().vbx_ode_norm_slab_doubles(n), dtype=torch.float64, device=dev)
    f = lambda x, k: k.copy_(fn(times[0], x))
    f(y, ks[0])
    L.call("vbx_ode_norm", state, slab, S.NORM_INIT0, y, None, _ptrs(ks[:1]), None, 1, n, 1, _st())
    L.call("vbx_ode_combine_dp", ys, y, _ptrs(ks[:1]), S._floats([1.0]), 1, state, S.DP_H0, n, _st())
    L.call("vbx_ode_stage_time_dp", times, 1, state, 0.0, S.TIME_PROBE, _st())
    f(ys, ks[1])
    L.call("vbx_ode_norm", state, slab, S.NORM_INIT1, y, None, _ptrs(ks[:2]), None, 2, n, 1, _st())
    h0 = float(state[S.DP_DT])
    trace = []
    for _ in range(max_attempts):
        t0, dt = float(state[S.DP_T]), float(state[S.DP_DT])
        for i in range(6):
            x = y1 if i == 5 else ys
            L.call("vbx_ode_combine_dp", x, y, _ptrs(ks[:i + 1]), S._floats(S.DP_BETA[i]), i + 1, state, S.DP_DT, n, _st())
            L.call("vbx_ode_stage_time_dp", times, 1, state, S.DP_ALPHA[i], S.TIME_END if S.DP_ALPHA[i] == 1.0 else S.TIME_STAGE, _st())
            f(x, ks[i + 1])
        L.call("vbx_ode_norm", state, slab, S.NORM_ERROR, y, y1, _ptrs(ks), S._floats(S.DP_C_ERROR), 7, n, 1, _st())
        L.call("vbx_ode_commit", y, ks[0], y1, ks[6], state, n, _st())
        s = state.tolist()
        assert not s[S.DP_BAD]
        trace.append((t0, dt, s[S.DP_RATIO], bool(s[S.DP_LAST])))
        if s[S.DP_DONE]:
            break
    L.call("vbx_ode_dense", out, y, y1, _ptrs(ks), S._floats(S.DP_C_MID), state, n, _st())
    s = state.tolist()
    return out, h0, trace, s


def test_dopri5_kernels_follow_the_host_restatement():
    """Diagonal linear system with a spread of rates (forces rejections), f by torch on the device: the kernels take the host
    restatement's accepted / rejected sequence exactly, and the same first step bit for bit.  Step starts and the final state agree
    to what an fp32 state allows: the embedded error is a heavily cancelling sum of the fp32 stages, which the host (torch matmul)
    and the device (stage order) round differently, so the ratios -- and through ratio^(-1/5) the next steps -- differ at ~1e-6 per
    step and compound along the run.  Measured at tol 1e-4 (28 attempts, 5 rejected): step starts 1.2e-5 relative, final state
    1.6e-6; the bounds are ~8x / 6x that."""
    from voicebox_pytorch_amd import solver as S

    lam = torch.tensor([-0.3, -3.0, -20.0, -60.0, 0.5]).repeat_interleave(256)
    c1 = 0.5
    y0 = torch.linspace(-1, 2, lam.numel())
    fn_h = lambda t, y: (lam + c1 * t) * y
    lam_d = lam.to(dev)
    fn_d = lambda t, y: (lam_d + c1 * t) * y
    for tol in (1e-4, 1e-5):
        st = {}
        want = ode_ref.odeint(fn_h, y0, torch.linspace(0, 1, 2), atol=tol, rtol=tol, method="dopri5", stats=st)
        got, h0, trace, s = _dp_kernel_run(fn_d, y0.to(dev), tol, tol)
        seq_h = [a for *_, a in st["trace"]]
        seq_d = [a for *_, a in trace]
        dt_rel = max(abs(a[0] - b[0]) / max(abs(b[0]), 1e-30) for a, b in zip(trace, st["trace"]) if b[0] > 0)
        print("tol", tol, "host", len(seq_h), sum(seq_h), "device", len(seq_d), sum(seq_d), "h0", h0, st["h0"], "max rel t0", dt_rel,
              "final rel", rel(got, want))
        assert abs(h0 - st["h0"]) <= 1e-6 * st["h0"]
        assert seq_d == seq_h and sum(not a for a in seq_h) >= 1
        assert int(s[S.DP_NFE]) == st["nfe"] and int(s[S.DP_ACCEPTED]) == st["accepted"] and int(s[S.DP_REJECTED]) == st["rejected"]
        assert dt_rel < 1e-4, dt_rel
        assert rel(got, want) < 1e-5, rel(got, want)


def _wrapper(g, method, **kw):
    import voicebox_pytorch_amd as vbx

    vb = vbx.VoiceBox(dim=g["cfg"]["dim"], num_cond_tokens=500, depth=g["cfg"]["depth"], dim_head=64, heads=g["cfg"]["heads"],
                      condition_on_text=False)
    vb.load_state_dict(g["state"], strict=False)
    vb = vb.to(dev)
    return vbx, vb, vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=method, **kw)


def _cpu_ref(g, method, steps, emulate=False):
    cfg = restate.Cfg(**g["cfg"])
    ones = torch.ones(g["y0"].shape[:2], dtype=torch.bool)
    fn = lambda t, y: restate.forward_with_cond_scale(g["state"], cfg, y, t, g["cond"], ones)
    st = {}
    with torch.no_grad():
        if emulate:
            with restate.emulate_fp16_operands():
                y = ode_ref.odeint(fn, g["y0"], torch.linspace(0, 1, steps), method=method, stats=st)
        else:
            y = ode_ref.odeint(fn, g["y0"], torch.linspace(0, 1, steps), method=method, stats=st)
    return y, st


def test_fixed_grid_methods_match_the_restatement(golden):
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_wc")
    for method in ("euler", "rk4"):
        vbx, vb, wrapper = _wrapper(g, method)
        for steps in (3, 9):
            ref, st = _cpu_ref(g, method, steps)
            for use_graph in (False, True):
                with rng_override(y0=g["y0"]):
                    s = wrapper.sample(cond=g["cond"].to(dev), steps=steps, use_graph=use_graph)
                e = rel(s, ref)
                print(method, steps, "graph" if use_graph else "eager", e, wrapper.last_sample_stats)
                assert wrapper.last_sample_stats == {"method": method, "nfe": st["nfe"], "accepted": steps - 1, "rejected": 0}
                assert e < 2e-3, (method, steps, use_graph, e)  # midpoint holds 2e-3 here (test_well_conditioned_sampler_is_tight)


def test_dopri5_matches_the_restatement(golden):
    """small_wc at the default tolerances: the fp32 CPU restatement takes 12 accepted / 1 rejected steps (80 NFE).  The fast path
    (fp16 / bf16 operands) flips that one borderline rejection: measured 12 / 0, 74 NFE, eager and under hipGraph alike -- so its
    NFE is asserted within one attempt of the CPU's; the sample is 5.0e-4 from the restatement's (bound 2e-3, as midpoint's)."""
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_wc")
    ref, st = _cpu_ref(g, "dopri5", 3)
    assert (st["accepted"], st["rejected"], st["nfe"]) == (12, 1, 80)
    vbx, vb, wrapper = _wrapper(g, "dopri5")
    outs = []
    for use_graph in (False, True, True):
        with rng_override(y0=g["y0"]):
            s = wrapper.sample(cond=g["cond"].to(dev), steps=3, use_graph=use_graph)
        ls = wrapper.last_sample_stats
        e = rel(s, ref)
        print("dopri5", "graph" if use_graph else "eager", e, ls, "cpu", st["nfe"])
        assert ls["method"] == "dopri5" and ls["nfe"] == 2 + 6 * (ls["accepted"] + ls["rejected"])
        assert abs(ls["nfe"] - st["nfe"]) <= 6, (ls, st["nfe"])
        assert e < 2e-3, e
        outs.append((s, ls))
    # determinism: same y0 -> bit-identical samples with the same counts (eager, graph, graph replayed again)
    assert torch.equal(outs[1][0], outs[2][0]) and outs[1][1] == outs[2][1]
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


def test_dopri5_precise_mode_takes_the_restatements_steps(golden):
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_wc")
    ref, st = _cpu_ref(g, "dopri5", 3)
    vbx, vb, wrapper = _wrapper(g, "dopri5")
    with vbx.precise_mode(), rng_override(y0=g["y0"]):
        s = wrapper.sample(cond=g["cond"].to(dev), steps=3)
    ls = wrapper.last_sample_stats
    print("dopri5 precise", rel(s, ref), ls)  # measured 1.1e-6, 12 / 1
    assert (ls["accepted"], ls["rejected"], ls["nfe"]) == (12, 1, 80), ls
    assert rel(s, ref) < 2e-4, rel(s, ref)


def test_fixed_grid_split_halves_are_bit_identical(golden):
    from voicebox_pytorch_amd.solver import RKSampler

    g = golden("small_wc")
    vbx, vb, wrapper = _wrapper(g, "rk4")
    vb.eval()
    gen = torch.Generator().manual_seed(5)
    cond = torch.cat([g["cond"], g["cond"].flip(0) * 0.5 + 0.1 * torch.randn(g["cond"].shape, generator=gen)]).to(dev)
    y0 = torch.randn(cond.shape, generator=gen).to(dev)
    B, N, _ = cond.shape
    with torch.no_grad():
        for method in ("euler", "rk4"):
            ref = RKSampler(vb, B, N, 5, method, use_graph=False, split=1).run(y0, cond)
            for use_graph in (False, True):
                smp = RKSampler(vb, B, N, 5, method, use_graph=use_graph, split=2)
                assert smp.split == 2
                out = smp.run(y0, cond)
                assert torch.equal(out, ref), (method, use_graph, float((out - ref).abs().max()))
                assert torch.equal(smp.run(y0, cond), ref)


def test_guided_text_model(golden):
    """rk4 and dopri5 with classifier-free guidance (cond_scale 1.3) on small_text against the emulated-precision restatement,
    at the bound the midpoint guided test uses.  Measured: rk4 3.8e-2; dopri5 4.0e-3 with 1324 NFE (88 / 22) against the CPU's
    1360 (2 x 680) -- small_text is the reference's own chaotic initialisation, so the NFE is bounded to 10 %, not pinned."""
    import voicebox_pytorch_amd as vbx
    from voicebox_pytorch_amd.masks import rng_override

    g = golden("small_text")
    vb = vbx.VoiceBox(dim=64, num_cond_tokens=50, dim_cond_emb=48, depth=2, dim_head=64, heads=2, condition_on_text=True)
    vb.load_state_dict(g["state"], strict=False)
    vb = vb.to(dev).eval()
    cfg = restate.Cfg(dim=64, depth=2, heads=2, dim_head=64)
    ones = torch.ones(g["y0"].shape[:2], dtype=torch.bool)
    fn = lambda t, y: restate.forward_with_cond_scale(g["state"], cfg, y, t, g["cond"], ones, cond_token_ids=g["ids_n"], cond_scale=1.3)
    for method in ("rk4", "dopri5"):
        st = {}
        with torch.no_grad(), restate.emulate_fp16_operands():
            emu = ode_ref.odeint(fn, g["y0"], torch.linspace(0, 1, 3), method=method, stats=st)
        wrapper = vbx.ConditionalFlowMatcherWrapper(voicebox=vb, torchdiffeq_ode_method=method)
        for use_graph in (False, True):
            with rng_override(y0=g["y0"]):
                s = wrapper.sample(cond=g["cond"].to(dev), semantic_token_ids=g["ids_n"].to(dev), steps=3, cond_scale=1.3,
                                   use_graph=use_graph)
            ls = wrapper.last_sample_stats
            print("guided", method, "graph" if use_graph else "eager", rel(s, emu), ls, "cpu nfe (single)", st["nfe"])
            assert rel(s, emu) < 0.1
            assert ls["nfe"] == 2 * st["nfe"] if method == "rk4" else abs(ls["nfe"] - 2 * st["nfe"]) <= 0.1 * 2 * st["nfe"] + 12
