"""The memory-bound row kernels on their own, per element against fp64 (tests/rows_check.py has the cases, the references and the
counted bounds; tests/test_rows_check_cpu.py shows on the CPU that the fp32 stand-in passes them and planted faults do not):
vbx_rmsnorm_fwd / _f32, vbx_rmsnorm_bwd with its partial records, vbx_reduce_norm_partials, vbx_reduce_col_partials,
vbx_layernorm_fwd / _bwd, vbx_gateloop_scan_fwd / _bwd, vbx_convpos_fwd / _libm / _bwd and vbx_conv_wgrad_finalize, at the widths, row
counts and frame counts where their guards, dispatches, chunk seams and tile seams decide.

Every output buffer starts as NaN sentinels with a guard row behind it, every operand row a launch must not read is NaN.  Each case is
a few launches, a synchronize, and rows_check's checks on CPU copies."""
import pytest
import torch

import rows_check as rc
from rows_check import CONV_CASES, FINALIZE_CASES, LN_CASES, REDUCE_CASES, RMS_BWD_CASES, RMS_FWD_CASES, SCAN_CASES

pytestmark = pytest.mark.gpu

dev = "cuda"


@pytest.fixture(scope="module")
def L():
    from voicebox_pytorch_amd import _lib

    _lib.lib()
    _lib.call("vbx_check_device", 0)
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def up(t):
    return None if t is None else t.contiguous().to(dev)


def cpu(d):
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in d.items()}


@pytest.mark.parametrize("c", RMS_FWD_CASES, ids=lambda c: c.name)
def test_rmsnorm_fwd(L, c):
    x, gamma, beta = (up(t) for t in rc.rms_fwd_inputs(c))
    out = {k: up(t) for k, t in rc.new_rms_fwd_out(c).items()}
    stride = c.D if c.adaptive else 0
    L.call("vbx_rmsnorm_fwd", x, gamma, beta, stride, out["bf16"], out["f16"], c.B, c.Np, c.n0, c.rpb, c.D, st())
    L.call("vbx_rmsnorm_fwd_f32", x, gamma, beta, stride, out["f32"], c.B, c.Np, c.n0, c.rpb, c.D, st())
    rc.check_rms_fwd(c, cpu(out))


@pytest.mark.parametrize("c", RMS_BWD_CASES, ids=lambda c: c.name)
def test_rmsnorm_bwd(L, c):
    inp = rc.rms_bwd_inputs(c)
    assert L.lib().vbx_rmsnorm_bwd_chunks(c.rpb) == c.chunks
    out = {k: up(t) for k, t in rc.new_rms_bwd_out(c).items()}
    L.call("vbx_rmsnorm_bwd", up(inp["x"]), up(inp["gamma"]), c.D if c.adaptive else 0, up(rc.nan_guard(inp["dy"], c.D)), up(inp["dx_in"]),
           out["dx_out"], out.get("dxb"), out["part"], out.get("cpart"), c.B, c.Np, c.n0, c.rpb, c.D, st())
    rc.check_rms_bwd(c, cpu(out))


@pytest.mark.parametrize("c", REDUCE_CASES, ids=lambda c: c.name)
def test_reduce_partials(L, c):
    part = up(rc.reduce_input(c))
    out = {k: up(t) for k, t in rc.new_reduce_out(c).items()}
    if c.kind == "col":
        L.call("vbx_reduce_col_partials", part, out["out"], out["tmp"], c.B, c.chunks, c.D, st())
    else:
        L.call("vbx_reduce_norm_partials", part, out["out"], 0 if c.sum_batch else c.W + c.pad, c.B, c.chunks, c.D, c.sum_batch, st())
    rc.check_reduce(c, cpu(out))


@pytest.mark.parametrize("c", LN_CASES, ids=lambda c: c.name)
def test_layernorm(L, c):
    inp = rc.ln_inputs(c)
    s, w = up(rc.nan_guard(inp["s"], c.D)), up(inp["w"])
    out = {k: up(t) for k, t in rc.new_ln_out(c).items()}
    L.call("vbx_layernorm_fwd", s, w, up(inp["b"]), up(inp["resid"]), out["y"], c.B * c.Np, c.D, rc.EPS_LN, st())
    if not c.fwd_only:
        L.call("vbx_layernorm_bwd", s, w, up(rc.nan_guard(inp["dy"], c.D)), out["ds"], out["part"], c.B, c.Np, c.D, rc.EPS_LN, st())
    rc.check_ln(c, cpu(out))


@pytest.mark.parametrize("c", SCAN_CASES, ids=lambda c: c.name)
def test_gateloop_scan(L, c):
    inp = rc.scan_inputs(c)
    qkva = up(rc.nan_guard(inp["qkva"], 3 * c.D))
    out = {k: up(t) for k, t in rc.new_scan_out(c).items()}
    L.call("vbx_gateloop_scan_fwd", qkva, out["s"], out["h"], c.B, c.Np, c.D, st())
    L.call("vbx_gateloop_scan_fwd", qkva, out["s_nostate"], None, c.B, c.Np, c.D, st())
    L.call("vbx_gateloop_scan_bwd", qkva, up(rc.nan_guard(inp["hin"], c.D)), up(rc.nan_guard(inp["ds"], c.D)), out["dqkva"], c.B, c.Np,
           c.D, st())
    rc.check_scan(c, cpu(out))


def test_sigmoid_sweep(L):
    """The scan's a = 1 / (1 + __expf(-x)) read back through the kernel at Np = 2 (h_1 = a_1 1 + 0) over the logits of rows_check.SWEEP,
    against the fp64 sigmoid: the figure RHO_A was made from still holds."""
    qkva = rc.sweep_qkva()
    D = qkva.shape[-1] // 3
    s, h = up(rc.rows_buf(2, D, rc.F32)), up(rc.rows_buf(2, D, rc.F32))
    L.call("vbx_gateloop_scan_fwd", up(rc.nan_guard(qkva, 3 * D)), s, h, 1, 2, D, st())
    torch.cuda.synchronize()
    rel, at = rc.sigmoid_rel_error(h.cpu()[1])
    ck = rc.RowChecks("sigmoid-sweep")
    ck.le(f"relative error of a against the fp64 sigmoid, largest at x = {at:g}", rel, rc.SIGMOID_REL_MEASURED)
    ck.same_bits("h_0 = kv_0", h.cpu()[0], torch.ones(D))
    ck.sentinel_kept("hstate guard row", h.cpu()[2:])
    ck.done()


@pytest.mark.parametrize("c", CONV_CASES, ids=lambda c: c.name)
def test_convpos(L, c):
    inp = rc.conv_inputs(c)
    assert L.lib().vbx_convpos_bwd_chunks(c.B, c.N) == c.B * c.tiles
    e, w, bias = up(rc.nan_guard(inp["e"], c.D)), up(inp["w"]), up(inp["bias"])
    mask = up(inp["mask"].to(torch.uint8)) if inp["mask"] is not None else None
    reg = up(inp["reg"]) if c.R else None
    out = {k: up(t) for k, t in rc.new_conv_out(c).items()}
    L.call("vbx_convpos_fwd", e, w, bias, mask, reg, out["xs"], c.B, c.N, c.R, c.D, c.ks, st())
    L.call("vbx_convpos_fwd_libm", e, w, bias, mask, reg, out["xs_libm"], c.B, c.N, c.R, c.D, c.ks, st())
    dpre = torch.empty(c.B * c.N * c.D + c.D, device=dev)  # scratch: not compared
    L.call("vbx_convpos_bwd", e, w, bias, mask, up(rc.nan_guard(inp["dxs"], c.D)), dpre, out["de"], out["deb"], out["wpart"], out.get("dreg"),
           c.B, c.N, c.R, c.D, c.ks, st())
    rc.check_conv(c, cpu(out))


@pytest.mark.parametrize("f", FINALIZE_CASES, ids=rc.finalize_name)
def test_conv_wgrad_finalize(L, f):
    chunks, D, ks = f
    out = {k: up(t) for k, t in rc.new_finalize_out(f).items()}
    L.call("vbx_conv_wgrad_finalize", up(rc.finalize_input(f)), chunks, D, ks, out["dw"], out["db"], st())
    rc.check_finalize(f, cpu(out))
